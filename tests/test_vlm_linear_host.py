"""CPU: the test hook of the VLM decode projections (fe_op_vlm_linear / Engine.vlm_linear) is exported, declared and bound; and the
checks of tests/test_vlm_linear_gpu.py can fail: planted faults, applied in numpy to the float64 reference at shapes of the GPU cases,
are rejected by the exact check and by the random-case bound; the exact-case generators satisfy their own premises."""
import ctypes
import os
import re

import numpy as np
import pytest

import vlm_linear_ref as R
from facet_amd import _lib
from facet_amd.weights import quantize_e4m3_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = ["bf16", "fp8"]
ROUTES = ["logits", "linear"]          # fp32 and bf16 results


def test_new_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "facet_amd", "libfacet_engine.so"))
    header = open(os.path.join(ROOT, "include", "facet_engine.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    name = "fe_op_vlm_linear"
    assert hasattr(lib, name)
    assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert name in doc and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == 21          # the header's parameter count
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
    assert len(decl.split(",")) == 21
    assert callable(_lib.Engine.vlm_linear)
    assert _lib.Engine.VLM_LINEAR_ROUTES == {"linear": 0, "logits": 1, "add_rmsnorm": 2, "silu_mul": 3}
    assert _lib.Engine.VLM_LINEAR_KERNELS == {"auto": 0, "gemv": 1, "gemm32": 2}


def test_split_formula_of_the_cases():
    """The dispatch formula as the cases rely on it: splits 1, 2, 9, 17 at these K; 17 splits are two full 8-wide load groups and one."""
    assert [R.gemm32_splits(33, K) for K in (128, 384, 1408, 4608, 8704)] == [(1, 1), (1, 3), (2, 6), (9, 4), (17, 4)]
    assert R.gemm32_splits(132, 4608, paired=True) == (9, 4) and R.gemm32_splits(4352, 384) == (1, 3)
    assert R.depth_gemv(12296, "bf16", True) == 8 * 7 + 9 and R.depth_gemv(24592, "fp8", False) == 16 * 7 + 8
    assert R.depth_gemm32(8704, 17, True) == 512 + 18 and R.depth_gemm32(384, 1, False, direct=True) == 384


def test_exact_generators_satisfy_their_premises():
    """Sums below 2^24 units, the e4m3 round trip is the identity, neighbouring rows differ in scale, no zeros, rows of x all differ."""
    shapes = [(4, K, 5) for K in R.GEMV_K["bf16"] + R.GEMV_K["fp8"] + [24]] + [(M, K, N) for M, K, N, _, _ in R.GEMM_CASES]
    shapes += [(32, K, N) for N, K in R.ADD_NORM_SHAPES + R.SILU_SHAPES] + [(33, 384, 33)]
    for M, K, N in shapes:
        for shift in (0, 3):
            x, w, b = R.exact_x(K + N, M, K, K + 24), R.exact_w(K + N, N, K, shift), R.exact_bias(K + N, N)
            assert all(R.exact_premises(x, w, b, shift)), (M, K, N)
            assert 24 * K < 2 ** 24 and (x != 0).all() and (w != 0).all() and np.abs(x).max() == 3
            assert np.abs(w / R.row_scales(N, shift)[:, None]).max() == 8 and (x[:, K:] == 3).all()
            assert len({x[m, :K].tobytes() for m in range(M)}) == M
            codes, exps = quantize_e4m3_rows(w)
            assert np.array_equal(R.dequantize_e4m3_rows(codes, exps), w)
            assert N == 1 or (exps[1:] != exps[:-1]).all()
            assert ((codes & 0x78) != 0).all()          # no subnormal codes
        if N > 1:          # the second matrix of the paired launch: another scale on every row
            assert (quantize_e4m3_rows(R.exact_w(1, N, K, 0))[1] != quantize_e4m3_rows(R.exact_w(2, N, K, 3))[1]).all()
    # a sum that breaks the premise is reported
    assert not R.exact_premises(np.full((1, 8), 3.0, np.float32) * 2.0 ** 21, R.exact_w(0, 2, 8))[0]


def test_bf16_rounding_term():
    """The rounding term of a bf16 result is half an ulp, 2^-9 times the power of two above the value. The correct rounding meets it with
    equality at a tie; 2^-9 |v| would reject correct roundings."""
    v = np.array([1.0 + 2.0 ** -8, 1.5 + 2.0 ** -8, 3.0, 255.5])
    err = np.abs(R.bf16(v).astype(np.float64) - v)
    assert np.array_equal(err, [2.0 ** -8, 2.0 ** -8, 0.0, 0.5])
    assert (err <= R.half_ulp_bf16(v)).all() and err[0] == R.half_ulp_bf16(v[0]) and err[0] > 2.0 ** -9 * v[0]
    rng = np.random.default_rng(0)
    v = rng.normal(0, 40, 100000).astype(np.float32).astype(np.float64)          # (fp32 values, as a kernel rounds them)
    err = np.abs(R.bf16(v).astype(np.float64) - v)
    assert (err <= R.half_ulp_bf16(v)).all() and (err > 2.0 ** -9 * np.abs(v)).any()
    assert (R.half_ulp_bf16(v) <= 2.0 ** -8 * np.abs(v)).all() and R.half_ulp_bf16(0.0) == 0.0


def _out(y, route):
    """A float64 result as the kernel would store it."""
    return np.asarray(y, np.float64).astype(np.float32) if route == "logits" else R.bf16(y)


def _case(kind, fmt, M, K, N):
    if kind == "exact":
        x, w, b = R.exact_x(1, M, K), R.exact_w(1, N, K), R.exact_bias(1, N)
    else:
        x, w, b = R.random_x(1, M, K), R.random_w(1, N, K), R.random_w(2, 1, N)[0]
    return R.bf16(x), w, R.weights_as(fmt, w), b


def _verdicts(kind, route, faulty, ref, bound):
    """(the fault is rejected, the unfaulted result is accepted) under the check of `kind`."""
    if kind == "exact":
        want = _out(ref, route)
        return not np.array_equal(_out(faulty, route), want), True
    return R.worst(_out(faulty, route), ref, bound) > 1.0, R.worst(_out(ref, route), ref, bound) <= 1.0


def _bound(route, ref, S, D):
    e = R.e32(D, S)
    return e if route == "logits" else R.add_bf16(ref, e)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("fmt", FMTS)
def test_planted_faults_gemv(fmt, kind, route):
    for M, K in ((2, 2056), (4, 12296)) if fmt == "bf16" else ((2, 4112), (4, 24592)):
        x, w, wk, b = _case(kind, fmt, M, K, 5)
        ref, S = R.ref_linear(x, wk, b)
        bound = _bound(route, ref, S, R.depth_gemv(K, fmt, True))
        faults = dict(chunk=R.fault_dropped_chunk(x, wk, b, 16 if fmt == "fp8" else 8), swap=R.fault_rows_swapped(x, wk, b, 0))
        if fmt == "fp8":
            codes, exps = quantize_e4m3_rows(w)
            if (exps != np.roll(exps, -1)).any():
                faults["scale"] = R.fault_neighbour_scale(x, codes, exps, b)
            else:          # random rows of one exponent: the neighbour's scale IS the row's, the fault changes nothing
                assert kind == "random" and np.array_equal(R.fault_neighbour_scale(x, codes, exps, b), ref)
        for name, y in faults.items():
            rejected, good_ok = _verdicts(kind, route, y, ref, bound)
            assert rejected and good_ok, (name, fmt, kind, route, M, K)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("fmt", FMTS)
def test_planted_faults_gemm32(fmt, kind, route):
    for M, K, N in ((5, 4608, 129), (32, 8704, 33)):
        x, w, wk, b = _case(kind, fmt, M, K, N)
        ref, S = R.ref_linear(x, wk, b)
        splits, per = R.gemm32_splits(N, K)
        bound = _bound(route, ref, S, R.depth_gemm32(K, splits, True))
        faults = dict(chunk=R.fault_dropped_chunk(x, wk, b, 8), swap=R.fault_rows_swapped(x, wk, b, M - 2),
                      lost_first=R.fault_split_left_out(x, wk, b, splits, per, 0), lost_last=R.fault_split_left_out(x, wk, b, splits, per, splits - 1),
                      # (random data: the bf16 rounding of 9 / 17 partial sums of ~sqrt(512) is 1.3 - 2.3 times the worst-case fp32 bound)
                      rounded=R.fault_partials_rounded(x, wk, b, splits, per))
        if fmt == "fp8":
            codes, exps = quantize_e4m3_rows(w)
            if kind == "exact" or N == 129:          # (129 random rows do not share one exponent; the 33 of the other shape do: a no-op there)
                assert (exps != np.roll(exps, -1)).any()
                faults["scale"] = R.fault_neighbour_scale(x, codes, exps, b)
        for name, y in faults.items():
            rejected, good_ok = _verdicts(kind, route, y, ref, bound)
            assert rejected and good_ok, (name, fmt, kind, route, M, K, N)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_planted_fault_tail_tile(kind, route):
    """The clamped weight row N - 1 stored for every column of the last partial tile (N = 129 and 33 have ONE column there and cannot
    show it: N = 100 and 31 of the same case list do)."""
    for M, K, N in ((32, 128, 100), (5, 128, 31)):
        x, w, wk, b = _case(kind, "bf16", M, K, N)
        ref, S = R.ref_linear(x, wk, b)
        bound = _bound(route, ref, S, R.depth_gemm32(K, 1, True))
        rejected, good_ok = _verdicts(kind, route, R.fault_tail_tile_last_row(ref), ref, bound)
        assert rejected and good_ok, (kind, route, N)
    assert np.array_equal(R.fault_tail_tile_last_row(np.arange(33.0)[None]), np.arange(33.0)[None])


def test_fused_bounds_accept_the_passes_done_in_float32_and_reject_a_lost_rounding():
    """The add_rmsnorm and silu_mul bounds on a numpy model of the two finishing passes (fp32 arithmetic in the kernels' order of
    roundings): accepted; the same passes fed a residual / a gate one bf16 ulp off: rejected."""
    rng = np.random.default_rng(3)
    M, N, K = 5, 512, 4608
    x, w = R.bf16(R.random_x(0, M, K)), R.bf16(R.random_w(0, N, K))
    proj, S = R.ref_linear(x, w)
    xres = R.bf16(rng.normal(0, 1, (M, N)))
    D = R.depth_gemm32(K, 9, False)
    f32 = np.float32
    r = R.bf16(xres + R.bf16(proj.astype(f32)))
    r0 = xres.astype(np.float64) + proj
    assert R.worst(r, r0, R.bound_residual(proj, S, r0, D)) <= 1.0
    off = r * f32(1 + 2.0 ** -7)          # every element one bf16 ulp up
    assert R.worst(off, r0, R.bound_residual(proj, S, r0, D)) > 1.0
    g = R.bf16(rng.normal(1, 0.25, N))
    eps = float(f32(1e-6))
    rs = (f32(1) / np.sqrt((r * r).sum(-1, keepdims=True, dtype=f32) / f32(N) + f32(eps))).astype(f32)
    n = R.bf16(g * R.bf16(r * rs))
    n_ref, n_bound = R.bound_rmsnorm(r, g, eps)
    assert R.worst(n, n_ref, n_bound) <= 1.0 and R.worst(n * f32(1 + 2.0 ** -6), n_ref, n_bound) > 1.0
    # silu_mul
    w2 = R.bf16(4.0 * R.random_w(5, N, K))
    up, Su = R.ref_linear(x, w2)
    gb, ub = R.bf16(proj.astype(f32)), R.bf16(up.astype(f32))
    with np.errstate(over="ignore"):
        h = R.bf16(R.bf16(gb / (f32(1) + np.exp(-gb))) * ub)
    bound = R.bound_silu_mul(proj, S, up, Su, D)
    assert R.worst(h, R.silu(proj) * up, bound) <= 1.0
    assert R.worst(h, R.silu(gb) * ub.astype(np.float64), R.bound_silu_mul(gb, None, ub, None, None)) <= 1.0
    assert R.worst(h, R.silu(proj) * up[:, ::-1], bound) > 1.0          # gate and up of different columns
