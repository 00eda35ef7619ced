"""The pooled gate of the fp32 TOPIQ head: gated 1x1 conv with the row-pooling epilogue + finishing pass (kernels_conv_dma.hip MODE 3,
rowpool_finish_kernel) against float64 and against the plain conv + adaptive pool, through fe_op_gate_rowpool; then TOPIQ scores with the
route on and off (FE_NO_GATE_ROWPOOL).

Bounds. Against float64 both routes meet the fp32 conv bound of tests/test_ops_gpu.py (2e-4 of max|ref|). The two routes pool the same
fp32 values in a different order, so by the standard bound of a kh*kw-term fp32 sum |fused - unfused| <= kh*kw * 2^-23 * mean_window(|v|).
End to end the scores of the two routes differed by 8.7e-8 relative at 256 x 320 and by nothing at 250 x 300 when measured (profiles/gate_rowpool_perf.txt); asserted at 4x.
"""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

from facet_amd._lib import FE_MODEL_TOPIQ
from facet_amd.weights import synthetic_state_dict, synthetic_images

pytestmark = pytest.mark.gpu

RTOL = 2e-4      # tests/test_ops_gpu.py: fp32 contractions against a float64 / torch-CPU reference, of max|ref|

# (n, h, w, cin, cout, th, tw)
FUSED_CASES = [
    (1, 16, 16, 64, 64, 1, 1),        # one 16x16 window, M = 256
    (2, 32, 48, 64, 64, 2, 3),        # the level-0 form, 24 tiles
    (3, 8, 24, 256, 256, 1, 3),       # 8x8 windows; W = 24 < 128: a tile spans rows and images; M = 576 is no multiple of 128
    (2, 4, 12, 512, 512, 1, 3),       # 4x4 windows, M = 96 < one tile
    (2, 6, 10, 1024, 1024, 3, 5),     # 2x2 windows, M = 120
    (2, 32, 24, 64, 64, 2, 3),        # kh != kw: 16x8 windows
    (1, 16, 32, 64, 96, 1, 2),        # column tail: Cout is no multiple of the tile width
    (1, 130, 160, 64, 64, 5, 10),     # M = 20800: enough workgroups that launch_conv takes the 128x64 tile (the cases above run 64x64); ragged last tile
]
UNFUSED_CASES = [
    (2, 33, 47, 64, 64, 2, 3),        # windows do not tile the map (adaptive windows overlap)
    (1, 16, 48, 64, 64, 1, 1),        # kw = 48: not a supported width
]


def _act64(v, act):
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "gelu":
        return torch.nn.functional.gelu(torch.from_numpy(v)).numpy()
    if act == "softplus":
        return torch.nn.functional.softplus(torch.from_numpy(v)).numpy()
    raise ValueError(act)


def _pool64(v, th, tw):
    """torch adaptive_avg_pool2d windows on [n, c, h, w] float64"""
    n, c, h, w = v.shape
    out = np.empty((n, c, th, tw))
    for i in range(th):
        hs, he = (i * h) // th, -((-(i + 1) * h) // th)
        for j in range(tw):
            ws, we = (j * w) // tw, -((-(j + 1) * w) // tw)
            out[:, :, i, j] = v[:, :, hs:he, ws:we].mean(axis=(2, 3))
    return out


@functools.lru_cache(maxsize=None)
def _problem(case, act):
    n, h, w, cin, cout, th, tw = case
    rng = np.random.default_rng(zlib.crc32(repr((case, act)).encode()))
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    g = (1.0 / (1.0 + np.exp(-rng.standard_normal((n, h, w))))).astype(np.float32)
    pre = np.einsum("nchw,oc->nohw", x.astype(np.float64), wt.astype(np.float64)) + b.astype(np.float64)[None, :, None, None]
    v = _act64(pre, act) * g.astype(np.float64)[:, None]
    ref, refabs = _pool64(v, th, tw), _pool64(np.abs(v), th, tw)
    for a in (x, wt, b, g, ref, refabs):
        a.setflags(write=False)
    return x, wt, b, g, ref, refabs


def _check_fused(engine, case, act, ldx=None):
    n, h, w, cin, cout, th, tw = case
    x, wt, b, g, ref, refabs = _problem(case, act)
    fused, took = engine.gate_rowpool(x, wt, b, g, th, tw, act=act, fused=True, ldx=ldx)
    again, took2 = engine.gate_rowpool(x, wt, b, g, th, tw, act=act, fused=True, ldx=ldx)
    plain, took0 = engine.gate_rowpool(x, wt, b, g, th, tw, act=act, fused=False, ldx=ldx)
    assert took and took2 and not took0, "the row-pooling route must run exactly where it was asked for"
    assert np.array_equal(fused, again), "two runs of the row-pooling route differ: the summation order is not fixed"
    scale = max(np.abs(ref).max(), 1e-6)
    e_f, e_p = np.abs(fused - ref).max() / scale, np.abs(plain - ref).max() / scale
    kh, kw = h // th, w // tw
    bound = kh * kw * 2.0 ** -23 * refabs + 1e-30
    d = np.abs(fused.astype(np.float64) - plain.astype(np.float64))
    print(f"{case} {act}: fused vs f64 {e_f:.3e}, plain vs f64 {e_p:.3e}, max (fused-plain)/bound {(d / bound).max():.3f}")
    assert e_f < RTOL and e_p < RTOL
    assert (d <= bound).all(), f"fused vs unfused: {(d / bound).max():.3f} of the summation bound"


@pytest.mark.parametrize("case", FUSED_CASES)
def test_rowpool_matches_float64_and_plain_route(engine, case):
    _check_fused(engine, case, "gelu")


@pytest.mark.parametrize("act", ["relu", "gelu", "softplus"])
def test_rowpool_level0_form_every_gate_activation(engine, act):
    _check_fused(engine, FUSED_CASES[1], act)


def test_rowpool_input_rows_wider_than_channels(engine):
    """the input is a channel slice of a wider buffer (row stride 80 > 64 channels; the rest holds 3e4)"""
    _check_fused(engine, FUSED_CASES[1], "gelu", ldx=80)


@pytest.mark.parametrize("case", UNFUSED_CASES)
def test_unsupported_windows_take_the_plain_route(engine, case):
    n, h, w, cin, cout, th, tw = case
    x, wt, b, g, ref, _ = _problem(case, "gelu")
    routed, took = engine.gate_rowpool(x, wt, b, g, th, tw, act="gelu", fused=True)
    plain, took0 = engine.gate_rowpool(x, wt, b, g, th, tw, act="gelu", fused=False)
    assert not took and not took0
    assert np.array_equal(routed, plain)
    assert np.abs(plain - ref).max() / max(np.abs(ref).max(), 1e-6) < RTOL


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
ONOFF_RTOL = 4 * 8.8e-8      # 4 x the measured difference of the two routes' scores; must stay below the 1e-5 of the batch-invariance test
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


@pytest.mark.parametrize("hw,n", [((256, 320), 3), ((250, 300), 2)])
def test_topiq_scores_with_route_on_and_off(engine, topiq_loaded, hw, n):
    """(256, 320): every pooled level tiles (16x16 ... 2x2 windows); (250, 300): the levels fall back to the plain route."""
    imgs = synthetic_images(7, n, *hw)
    ref = _oracle_scores(topiq_loaded, imgs)
    engine.set_microbatch(2)
    saved = os.environ.pop("FE_NO_GATE_ROWPOOL", None)
    try:
        on = engine.topiq_score(imgs)
        os.environ["FE_NO_GATE_ROWPOOL"] = "1"
        off = engine.topiq_score(imgs)
    finally:
        os.environ.pop("FE_NO_GATE_ROWPOOL", None)
        if saved is not None:
            os.environ["FE_NO_GATE_ROWPOOL"] = saved
    for got in (on, off):
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)
        assert rel.max() < 1e-3, f"got {got} ref {ref} rel {rel}"
    d = (np.abs(on.astype(np.float64) - off) / np.maximum(np.abs(off), 1e-3)).max()
    print(f"{hw} n={n}: on/off max relative difference {d:.3e}")
    assert d <= ONOFF_RTOL, f"route on/off differ by {d:.3e} relative"
