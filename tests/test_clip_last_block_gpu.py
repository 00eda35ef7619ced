"""GPU: the last block of the fp32 CLIP image tower on the class-token rows only (clip_forward, model_clip.hip) against the full last block
(FE_CLIP_FULL_LAST_BLOCK, read per call) and against the torch-CPU oracle (oracle/clip_vit.py).

Small towers: clip_vit_spec(width=128, layers=2 | 1, patch=14, grid=3, out_dim=64) - 2 heads of 64, 10 tokens, 42 x 42 input; with one layer
the pruned block is also the first. Batches 1, 3, 33 and 40 lie on both sides of the 32-row chunk of the few-row kernel that the pruned
block's one row per image runs on. Bound against the oracle: the 1e-3 of max|ref| of tests/test_clip_gpu.py, for both routes.

Route against route, max|pruned - full| / max|full| over the features (measured on MI355X, profiles/clip_last_block_perf.txt):
  small towers, batches 1 .. 40      <= 3.958e-07    asserted: 4 x 3.96e-7 = 1.6e-6
  ViT-L/14, 3 crops                     2.744e-07    asserted: 4 x 2.75e-7 = 1.1e-6
both under the 1e-5 the project allows between two routes of one model. The two routes differ in the summation order of the last block's
class-token rows only (few-row kernel against the tiled one); every other row of the full route is work the result never read.

Batch independence. Before this change one crop's features were bit-equal alone and in a batch of 3, and NOT in a batch of 40 (the tiled
kernel picks its tile by the row count: 1.0e-6 of max|feat| on the small towers and on ViT-L/14). The pruned block adds no dependence of
its own - its rows go through the few-row kernel whatever the batch is (tests/test_gemm_skinny_res_gpu.py asserts a row's bits there) - so
the test asserts what held before, alone == in a batch of 3, on both routes, and prints the figure for the batch of 40."""
import os

import numpy as np
import pytest
import torch

from facet_amd._lib import FE_MODEL_CLIP
from facet_amd.weights import clip_vit_spec, synthetic_state_dict

pytestmark = pytest.mark.gpu

HOOK = "FE_CLIP_FULL_LAST_BLOCK"
SMALL = dict(width=128, patch=14, grid=3, out_dim=64)
BATCHES = (1, 3, 33, 40)
ROUTE_BOUND_SMALL = 1.6e-6
ROUTE_BOUND_VITL = 1.1e-6


@pytest.fixture(scope="module")
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=4 << 30)
    yield e
    e.close()


def _features(eng, x, full, out_dim):
    """Features of x on the pruned (default) or the full last block; the hook is read per call."""
    assert HOOK not in os.environ
    if full:
        os.environ[HOOK] = "1"
    try:
        return eng.clip_encode_image(x, out_dim=out_dim)
    finally:
        os.environ.pop(HOOK, None)


@pytest.fixture(scope="module")
def small(eng):
    """layers -> (state dict, 40 inputs, oracle features); computed once."""
    from oracle.clip_vit import CLIPImage
    out = {}
    x = torch.randn(max(BATCHES), 3, 42, 42, generator=torch.Generator().manual_seed(4))
    for layers in (2, 1):
        sd = synthetic_state_dict("clip", seed=9, spec=clip_vit_spec(layers=layers, **SMALL))
        net = CLIPImage(heads=2, layers=layers, **SMALL).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            out[layers] = (sd, x.numpy(), net.encode_image(x).numpy())
    return out


@pytest.mark.parametrize("layers", (2, 1))
def test_small_tower_both_routes_against_oracle(eng, small, layers):
    sd, x, ref = small[layers]
    eng.load_weights(FE_MODEL_CLIP, sd)
    worst = 0.0
    for n in BATCHES:
        pruned, full = _features(eng, x[:n], False, 64), _features(eng, x[:n], True, 64)
        assert pruned.shape == full.shape == (n, 64)
        scale = np.abs(ref[:n]).max()
        ep, ef, rr = np.abs(pruned - ref[:n]).max() / scale, np.abs(full - ref[:n]).max() / scale, np.abs(pruned - full).max() / np.abs(full).max()
        print(f"\nlayers {layers} batch {n}: pruned / oracle {ep:.3e}, full / oracle {ef:.3e}, pruned / full {rr:.3e}")
        assert ep < 1e-3 and ef < 1e-3, (layers, n, ep, ef)
        worst = max(worst, rr)
    assert worst <= ROUTE_BOUND_SMALL < 1e-5, worst


def test_vit_l14_route_against_route(eng):
    eng.load_weights(FE_MODEL_CLIP, synthetic_state_dict("clip", seed=9))
    x = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(4)).numpy()
    pruned, full = _features(eng, x, False, 768), _features(eng, x, True, 768)
    rr = np.abs(pruned - full).max() / np.abs(full).max()
    print(f"\nViT-L/14, 3 crops: pruned / full {rr:.3e} (max abs {np.abs(pruned - full).max():.3e}, max|feat| {np.abs(full).max():.3e})")
    assert np.isfinite(pruned).all() and rr <= ROUTE_BOUND_VITL < 1e-5, rr
    assert np.array_equal(full, _features(eng, x, True, 768)) and np.array_equal(pruned, _features(eng, x, False, 768))      # each route repeats itself


@pytest.mark.parametrize("layers", (2, 1))
def test_one_crop_alone_and_in_a_batch(eng, small, layers):
    sd, x, _ = small[layers]
    eng.load_weights(FE_MODEL_CLIP, sd)
    for full in (False, True):
        one, three, forty = (_features(eng, x[:n], full, 64)[0] for n in (1, 3, 40))
        print(f"\nlayers {layers} {'full' if full else 'pruned'}: alone - in 3 {np.abs(one - three).max():.3e}, alone - in 40 {np.abs(one - forty).max():.3e} "
              f"of max|feat| {np.abs(one).max():.3e}")
        assert np.array_equal(one, three), (layers, full)
