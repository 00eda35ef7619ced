"""GPU: the GELU form of the in-register Winograd kernel (wino64_kernel<ACT_GELU>, facet_amd/csrc/kernels_wino64.hip) launched alone
through Engine.wino64_conv (no routing), then the TOPIQ fp32 head with its wino64 route on and off (FE_NO_HEAD_WINO64).

Op level: float64 F.gelu of the float64 convolution at tests/test_wino64_gpu.py's bound, 2e-4 * max(1, |ref|max); on integers the
pre-activation is exact, so the result must be the GELU that an identity 1x1 convolution applies to the exact convolution, bit for bit
(both epilogues call fe_gelu_erf).

End to end: the scores of the two routes differed by 3.43e-7 relative when measured (3 images of 512 x 512, levels 0 - 2 routed;
profiles/erf_gelu_perf.txt): MEASURED_ONOFF below, asserted at 4x, which must stay under the 1e-5 of the batch-invariance test. 2 images
of 96 x 128: no level reaches 1 MiB per image, nothing is routed, the scores are bit-equal."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facet_amd._lib import FE_MODEL_TOPIQ
from facet_amd.weights import synthetic_state_dict, synthetic_images

pytestmark = pytest.mark.gpu

WINO64 = "wino64 3x3"
SHAPES = [(2, 64, 64, 16, 16), (1, 64, 64, 19, 23), (3, 64, 64, 5, 70), (1, 64, 64, 1, 1), (2, 56, 40, 20, 20)]      # tests/test_wino64_gpu.py's kinds
EPILOGUES = ["shift", "scale_shift", "res_before_act", "res_after_act"]


@functools.lru_cache(maxsize=None)
def _case(n, cin, cout, h, w):
    """x, weights, epilogue vectors and the float64 convolution of one shape - computed once, shared, read-only"""
    rng = np.random.default_rng(1000 * cin + 10 * h + w + cout + 5)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    r = rng.standard_normal((n, cout, h, w)).astype(np.float32)
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), padding=1)
    for a in (x, wt, sc, sh, r):
        a.setflags(write=False)
    return x, wt, sc, sh, r, ref


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gelu_epilogues_against_float64(engine, shape, epi):
    x, wt, sc, sh, r, ref = _case(*shape)
    scd, shd, rd = (torch.from_numpy(np.array(a)).double() for a in (sc, sh, r))
    scd, shd = scd.view(1, -1, 1, 1), shd.view(1, -1, 1, 1)
    if epi == "shift":
        got, want = engine.wino64_conv(x, wt, shift=sh, act="gelu"), F.gelu(ref + shd)
    elif epi == "scale_shift":
        got, want = engine.wino64_conv(x, wt, scale=sc, shift=sh, act="gelu"), F.gelu(ref * scd + shd)
    elif epi == "res_before_act":
        got, want = engine.wino64_conv(x, wt, scale=sc, shift=sh, res=r, res_after_act=False, act="gelu"), F.gelu(ref * scd + shd + rd)
    else:
        got, want = engine.wino64_conv(x, wt, scale=sc, shift=sh, res=r, res_after_act=True, act="gelu"), F.gelu(ref * scd + shd) + rd
    want = want.numpy()
    err, bound = float(np.abs(got - want).max()), 2e-4 * max(1.0, float(np.abs(want).max()))
    print(f"{shape} {epi}: max |got - ref| = {err:.3e}, bound {bound:.3e}")
    assert got.shape == want.shape and err <= bound, (err, bound)


@pytest.mark.parametrize("cin,cout", [(64, 64), (56, 40)])
def test_gelu_on_integers_is_the_identity_convs_gelu_bit_for_bit(engine, cin, cout):
    """test_wino64_gpu.py's integer case: the kernel's pre-activation equals F.conv2d's exactly. The no-activation launch pins that; the
    GELU launch must then equal the GELU of a 1x1 identity convolution (another kernel, the same fe_gelu_erf) on those values."""
    rng = np.random.default_rng(cin + 19)
    x = rng.integers(-3, 4, (3, cin, 19, 23)).astype(np.float32)
    w = rng.integers(-2, 3, (cout, cin, 3, 3)).astype(np.float32)
    z = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), padding=1).numpy()
    assert np.array_equal(engine.wino64_conv(x, w), z)
    got = engine.wino64_conv(x, w, act="gelu")
    want = engine.conv2d(z, np.eye(cout, dtype=np.float32).reshape(cout, cout, 1, 1), act="gelu")
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} values differ"
    ref = F.gelu(torch.from_numpy(z).double()).numpy()
    assert np.abs(got - ref).max() <= 2e-4 * max(1.0, np.abs(ref).max())


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
MEASURED_ONOFF = 3.5e-7      # 3.430e-07 when measured (3 images of 512 x 512, micro-batch 2)
ONOFF_RTOL = 4 * MEASURED_ONOFF
assert ONOFF_RTOL <= 1e-5


@pytest.fixture(scope="module")
def topiq_loaded(engine):
    sd = synthetic_state_dict("topiq", seed=3)
    engine.load_weights(FE_MODEL_TOPIQ, sd)
    return sd


def _oracle_scores(sd, imgs):
    from oracle.topiq import CFANet
    net = CFANet().eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    x = torch.from_numpy(imgs.astype(np.float32) / 255.0).permute(0, 3, 1, 2)
    with torch.no_grad():
        return net(x).flatten().numpy()


def _scores_and_records(engine, imgs):
    engine.profile_enable(True)
    try:
        got = engine.topiq_score(imgs)
        names = [r["name"] for r in engine.profile_records()]
    finally:
        engine.profile_enable(False)
    return got, names


@pytest.mark.parametrize("hw,n,routed", [((512, 512), 3, True), ((96, 128), 2, False)])
def test_topiq_scores_with_head_route_on_and_off(engine, topiq_loaded, hw, n, routed):
    """(512, 512): the head's level 0 is 256 x 256 x 64 channels = 16 MiB per image and goes to the wino64 kernel, which leaves a profile
    record; (96, 128): every level is under 1 MiB per image, nothing is routed and the scores keep their bits."""
    imgs = synthetic_images(11, n, *hw)
    ref = _oracle_scores(topiq_loaded, imgs)
    engine.set_microbatch(2)
    saved = {k: os.environ.pop(k, None) for k in ("FE_NO_HEAD_WINO64", "FE_NO_WINO64")}
    try:
        on, names_on = _scores_and_records(engine, imgs)
        os.environ["FE_NO_HEAD_WINO64"] = "1"
        off, names_off = _scores_and_records(engine, imgs)
    finally:
        os.environ.pop("FE_NO_HEAD_WINO64", None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    for got in (on, off):
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)
        assert rel.max() < 1e-3, f"got {got} ref {ref} rel {rel}"
    # the head's level 0 works on the stem's map, H/2 x W/2 (the backbone's own 64 -> 64 ReLU layers, at H/4 x W/4, record this kernel in both runs)
    level0 = {f"{WINO64} M={k * (hw[0] // 2) * (hw[1] // 2)} K=576 N=64" for k in (1, 2)}
    head_on = [s for s in names_on if s in level0]
    head_off = [s for s in names_off if s in level0]
    d = (np.abs(on.astype(np.float64) - off) / np.maximum(np.abs(off), 1e-3)).max()
    print(f"{hw} n={n}: on/off max relative difference {d:.3e}; records with the route on {sorted(set(head_on))}, off {sorted(set(head_off))}")
    assert not head_off, head_off
    if routed:
        assert head_on, names_on
        assert d <= ONOFF_RTOL, f"route on/off differ by {d:.3e} relative"
    else:
        assert not head_on, head_on
        assert np.array_equal(on, off)
