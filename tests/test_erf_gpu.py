"""GPU: the erf GELU of the fp32 contraction epilogues (fe_gelu_erf, facet_amd/csrc/erf_core.h) alone. A 1x1 convolution with an identity
weight is exact (one product with 1, the others with 0), so its output is the device's GELU of the input: compared with
plain_ops_ref.act(v, "gelu") in float64 under plain_ops_ref.act_eval's bound, 4 u (|v| + |gelu(v)|) - the bound that file gave ocml's
erff (2 ulp) and that the branch-free erf has to meet as well (measured on the CPU: 1.25 ulp, tests/test_erf_host.py).

Inputs: a grid over [-6, 6], every fp32 value in a band around the erf's range threshold 0.921875 scaled by sqrt 2 (both signs), values
of 1e-30 .. 1e-3 (both signs) and +-20, shuffled so that every channel holds all kinds. Routes: the LDS-DMA kernel's narrow-tile
epilogue (the default of a 64 -> 64 layer), its wide-tile epilogue (forced 128x128 tile), the register-staged kernel conv_igemm (forced
64x64 tile) and the narrow-output kernel (Cout = 4, identity rows)."""
import functools

import numpy as np
import pytest

import plain_ops_ref as R

pytestmark = pytest.mark.gpu

C, H, W = 64, 64, 64
NARROW_CHANNELS = (0, 21, 42, 63)


@functools.lru_cache(maxsize=None)
def _inputs():
    """x [1, 64, 64, 64], float64 GELU of it and the bound - computed once, shared, read-only"""
    n = C * H * W
    thr = np.float32(0.921875) * np.float32(np.sqrt(2.0))
    band = (np.arange(-20000, 20000, dtype=np.int64) + int(np.float32(thr).view(np.uint32))).astype(np.uint32).view(np.float32)
    tiny = np.float32(10.0) ** np.linspace(-30, -3, 10000, dtype=np.float32)
    parts = [band, -band, tiny, -tiny, np.full(8, 20.0, np.float32), np.full(8, -20.0, np.float32), np.zeros(2, np.float32)]
    used = sum(p.size for p in parts)
    parts.append(np.linspace(-6.0, 6.0, n - used, dtype=np.float32))
    v = np.concatenate(parts).astype(np.float32)
    assert v.size == n
    np.random.default_rng(950).shuffle(v)
    x = v.reshape(1, C, H, W)
    ref = R.act(x, "gelu")
    bound = R.act_eval(x.astype(np.float64), ref, "gelu")
    for a in (x, ref, bound):
        a.setflags(write=False)
    return x, ref, bound


def _check(route, got, ref, bound):
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    i = int(np.argmax(ratio))
    print(f"{route}: worst err / bound {ratio.max():.3f} (err {err.flat[i]:.3e} at gelu = {ref.flat[i]:.9g})")
    assert ratio.max() <= 1.0, f"{route}: err / bound {ratio.max():.3f}"


@pytest.mark.parametrize("route,variant", [("dma_narrow_tile", 0), ("dma_wide_tile", 11), ("conv_igemm", 4)])
def test_gelu_of_an_identity_conv(engine, route, variant):
    x, ref, bound = _inputs()
    eye = np.eye(C, dtype=np.float32).reshape(C, C, 1, 1)
    try:
        engine.set_conv_variant(variant)
        got = engine.conv2d(x, eye, act="gelu")
        same = engine.conv2d(x, eye)
    finally:
        engine.set_conv_variant(0)
    assert np.array_equal(same, x), "the identity convolution is not exact: the test's premise"
    _check(route, got, ref, bound)


def test_gelu_of_identity_rows_on_the_narrow_kernel(engine):
    x, ref, bound = _inputs()
    rows = np.zeros((len(NARROW_CHANNELS), C, 1, 1), np.float32)
    for o, ch in enumerate(NARROW_CHANNELS):
        rows[o, ch] = 1.0
    got = engine.conv2d(x, rows, act="gelu")
    sel = list(NARROW_CHANNELS)
    assert np.array_equal(engine.conv2d(x, rows), x[:, sel]), "the identity rows are not exact: the test's premise"
    _check("conv_narrow", got, ref[:, sel], bound[:, sel])


def test_gelu_of_zero_infinity_nan_and_huge_values(engine):
    """gelu(0) = 0, gelu(inf) = inf, NaN stays NaN and the largest values pass through (erf = 1 exactly, nothing overflows on the way).
    The values enter through the per-channel shift: 0 * inf inside the contraction would be NaN."""
    eye = np.eye(C, dtype=np.float32).reshape(C, C, 1, 1)
    sh = np.zeros(C, np.float32)
    sh[0], sh[1], sh[2] = np.inf, np.nan, 3.0e38
    g = engine.conv2d(np.zeros((1, C, 1, 1), np.float32), eye, shift=sh, act="gelu")[0, :, 0, 0]
    assert g[0] == np.inf and np.isnan(g[1]) and g[2] == np.float32(3.0e38) and (g[3:] == 0).all(), g[:4]
