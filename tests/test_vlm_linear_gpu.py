"""GPU: the decode projection kernels of the VLM decoders (model_vlm.hip), each launched alone through Engine.vlm_linear
(fe_op_vlm_linear) and compared with float64. No model is loaded: the hook packs caller weights as build_vlm does and runs the decoder's
own routes - vlm_linear (bf16 out), the lm_head's logits form (fp32 out), o / down projection + vlm_finish_add_rmsnorm_kernel, gate | up
in one launch + vlm_finish_silu_mul_kernel - with the decoder's kernel choice or a forced one. Every case asserts from the returned
`info` that the kernel it is meant for ran (family, the GEMV's row template MR, the GEMM's K splits, the direct write).

Exact cases. x holds integers in [-3, 3], w integers in [-8, 8] (no zeros) with row n times 2^((n % 7) - 3), the bias integers: every
partial sum is an integer multiple of the row factor below 2^24 of them (24 K < 2^24), so ANY fp32 summation order is exact, and the
weights are exactly e4m3 values with a different scale on neighbouring rows. An fp32 result must equal the integer sum, a bf16 result
its one correct rounding: np.array_equal. A dropped or doubled K chunk, a neighbour's row scale, a lost split, a bf16 rounding of the
split sums, a clamped row that is stored, swapped batch rows - each moves some output by at least one unit.
  * add_rmsnorm: the returned residual is bf16(xres + bf16(sum)) (+ ds: bf16 of that + ds) - the fp32 additions are exact on these
    values (integers below 2^7 against 8-bit values below 2^24) - asserted exactly; the norm under its bound below.
  * silu_mul: the hook returns h only. Where the gate's exact sum is >= 40, 1 + expf(-g) is 1 in fp32 and in float64, silu(g) = g, and
    h = bf16(bf16(g) bf16(u)) is asserted exactly: that pins both inputs of the pass bit for bit. Everywhere, h is within the bound
    below taken with exact inputs (expf, the bf16 rounding of silu, the product, the store).

Random cases. Standard normal x and w; the reference is float64 on the values the kernel holds (bf16(x); bf16(w) or
dequantize(quantize(w))). u = 2^-24, S = sum_k |x_k w_k| + |bias|. Every bound is a sum of the roundings the code performs:
  fp32 result      |y - ref| <= E32 = 2 D u S, D = the longest chain of dependent fp32 additions of one output, every product inside a
                   v_dot2 or MFMA counted as one rounding (their internal order is not documented: the worst case)
    GEMV bf16      D = 8 ceil(K / 2048) + 6 + 2 (+ 1)   the busiest lane's 8-element chunks, the butterfly, (w0 + w1) + (w2 + w3), bias
    GEMV e4m3      D = 16 ceil(K / 4096) + 6 + 2 (+ 1)  16 codes per chunk; the row scale is a power of two (exact)
    GEMM           D = 128 ceil(K / 128 / splits) + splits (+ 1)   128 products per stage on one accumulator, the split sum, bias;
                   direct write: 128 K / 128 alone. splits is the count `info` returned, asserted equal to the dispatch formula
    wrapper        D = K (+ 1): any order of K additions (gemm_skinny / the conv kernel are not this file's subject)
  bf16 result      E32 + half_ulp(|ref| + E32), half_ulp(v) = 2^-9 2^ceil(log2 v): round to nearest on 8 significant bits, a theorem, no
                   margin. (2^-9 v itself is no bound: the correct rounding of 1 + 2^-8 is off by 2^-8. Every "bf16" below is this term.)
  add_rmsnorm      residual: E32 (D without bias), bf16(sum), the fp32 addition (2 u), bf16 of the stream; with ds the last two again.
                   norm, against float64 RMSNorm of the RETURNED residual: relative ((4 trips + 6 + 16 + 2) / 2 + 2) 2 u for rs
                   (sum of squares: square, two-level tree and running sum per 4096-column trip, butterfly, 16 wave sums; the mean and
                   + eps; halved by the square root; rsqrt's 1 ulp), then v rs (2 u), bf16, times g (2 u), bf16 store
  silu_mul         both inputs as the bf16 result above; through silu with slope <= 1.1; silu in fp32: expf 1 ulp (2 u), 1 + e (u), the
                   division (u), doubled; bf16(silu); the product's error es |u| + eu |silu| + es eu; the product (2 u); the bf16 store;
                   2^-121 on silu where expf overflows (g < -88.73: the quotient is 0), 2^-126 for a product below the normal range
The worst err / bound per route and format is printed by every test (pytest -s); DESIGN.md records them.

Which case reaches what:
  * vlm_gemv_kernel<1|2|4, TO, bf16> / vlm_gemv_kernel<1|2|4, TO, uint8_t>, bf16 and fp32 out: test_gemv, M = 1, 2, 3 auto and 4 forced. K = 8 / 16 (one
    lane), 520 / 1040 (wave 0 only, ragged), 2048 / 4096 (all four waves full), 2056 / 4112 (third loop twice for lane 0),
    6152 / 12304 (second loop + tail), 12296 / 24592 (one trip of each loop + a one-lane tail); N = 1, 2, 5 (single column, odd last pair)
  * ldx != K: test_gemv_ldx (K = 520 in rows of 544) and test_gemm32_ldx
  * e4m3 with K % 16 != 0 -> the wrapper on bf16 scratch: test_e4m3_odd_k_takes_the_wrapper; M = 33 -> the wrapper: test_wrapper_33_rows
  * vlm_gemm32_kernel<bf16|uint8_t> + vlm_gemm32_finish_kernel: test_gemm32. N = 1, 31, 33, 100, 129, 160: partial last tiles (row
    clamp, store guard, the e4m3 scale read), tile counts 1, 1, 2, 4, 5, 5 (idle waves in the last workgroup except at 4); splits 1, 2,
    9, 17 (K = 128 / 384, 1408, 4608, 8704); the direct write (fp32 out, K = 384, no bias) and its twins (bias; 9 splits)
  * vlm_finish_add_rmsnorm_kernel<false|true>: test_add_rmsnorm, d = 64, 512, 4352 (second trip of the 4096 loops) at 17, 9, 1 splits
    (17 = two full 8-wide load groups and one split)
  * the paired launch + vlm_finish_silu_mul_kernel: test_silu_mul, N = 36, 100, 132 (2, 4, 5 tiles per matrix: bx >= cols1 switches
    matrices inside and between workgroup columns), 1 and 9 splits
"""
import numpy as np
import pytest

import vlm_linear_ref as R

pytestmark = pytest.mark.gpu

FMTS = ["bf16", "fp8"]
KINDS = ["exact", "random"]
MR = {1: 1, 2: 2, 3: 4, 4: 4}
GEMV_K, GEMM_CASES, ADD_NORM_SHAPES, SILU_SHAPES = R.GEMV_K, R.GEMM_CASES, R.ADD_NORM_SHAPES, R.SILU_SHAPES
EPS = float(np.float32(1e-6))


@pytest.fixture(scope="module")
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 30)
    yield e
    e.close()


class Worst:
    """The worst err / bound of one test, per label; printed when the test ends."""
    def __init__(self, name):
        self.name, self.w = name, {}

    def add(self, label, y, ref, bound):
        q = R.worst(y, ref, bound)
        self.w[label] = max(self.w.get(label, 0.0), q)
        return q

    def show(self):
        print(f"[vlm_linear] {self.name}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.w.items())))


def _inputs(kind, seed, M, K, N, bias, ldx=None):
    if kind == "exact":
        x, w, b = R.exact_x(seed, M, K, ldx), R.exact_w(seed, N, K), (R.exact_bias(seed, N) if bias else None)
        sums_ok, codes_ok = R.exact_premises(x, w, b)
        assert sums_ok and codes_ok
        return x, w, b
    return R.random_x(seed, M, K, ldx), R.random_w(seed, N, K), (R.random_w(seed + 1, 1, N)[0] if bias else None)


def _check_linear(wst, label, kind, fmt, route, x, w, b, y, D):
    """One result of the linear / logits routes against its reference: exact equality, or the bound of its chain depth D."""
    ref, S = R.ref_linear(R.bf16(x), R.weights_as(fmt, w), b)
    if kind == "exact":
        want = ref.astype(np.float32) if route == "logits" else R.bf16(ref)
        assert np.array_equal(y, want), (label, np.argwhere(y != want)[:4], y[y != want][:4], want[y != want][:4])
        return
    e = R.e32(D, S)
    bound = e if route == "logits" else R.add_bf16(ref, e)
    q = wst.add(f"{fmt}/{route}", y, ref, bound)
    assert q <= 1.0, (label, q)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("fmt", FMTS)
def test_gemv(eng, fmt, M):
    wst = Worst(f"gemv {fmt} M={M}")
    kernel = "gemv" if M == 4 else "auto"          # 4 rows of K % 128 == 0 are the GEMM's in production; K % 128 != 0 ones are not
    for ki, K in enumerate(GEMV_K[fmt]):
        for N in (1, 2, 5):
            for kind in KINDS:
                for route in ("linear", "logits"):
                    for bias in (False, True):
                        x, w, b = _inputs(kind, 100 * ki + N, M, K, N, bias)
                        y, info = eng.vlm_linear(x, w, b, weight_format=fmt, route=route, kernel=kernel)
                        label = (fmt, M, K, N, kind, route, bias)
                        assert info == dict(family="gemv", mr=MR[M], splits=0, direct=False), (label, info)
                        _check_linear(wst, label, kind, fmt, route, x, w, b, y, R.depth_gemv(K, fmt, bias))
    wst.show()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_gemv_ldx(eng, fmt, kind):
    """Rows of x 24 elements longer than K (exact case: the padding holds 3s)."""
    wst = Worst(f"gemv ldx {fmt}")
    K = 520 if fmt == "bf16" else 1040
    for M in (2, 4):
        x, w, b = _inputs(kind, 5, M, K, 5, True, ldx=K + 24)
        y, info = eng.vlm_linear(x, w, b, weight_format=fmt, kernel="gemv")
        assert info["family"] == "gemv" and info["mr"] == MR[M], info
        _check_linear(wst, (fmt, M, kind), kind, fmt, "linear", x, w, b, y, R.depth_gemv(K, fmt, True))
    wst.show()


@pytest.mark.parametrize("kind", KINDS)
def test_e4m3_odd_k_takes_the_wrapper(eng, kind):
    """K = 24 is no multiple of a lane's 16 codes: vlm_linear widens the layer to bf16 scratch and runs the shared wrapper on it."""
    wst = Worst("e4m3 K=24")
    x, w, b = _inputs(kind, 9, 2, 24, 5, True)
    y, info = eng.vlm_linear(x, w, b, weight_format="fp8")
    assert info["family"] == "wrapper", info
    _check_linear(wst, kind, kind, "fp8", "linear", x, w, b, y, R.depth_wrapper(24, True))
    with pytest.raises(Exception, match="unsupported layer"):          # the forced kernel refuses it under its own check
        eng.vlm_linear(x, w, b, weight_format="fp8", kernel="gemv")
    wst.show()


@pytest.mark.parametrize("kind", KINDS)
def test_wrapper_33_rows(eng, kind):
    """More than 32 rows: the shared wrapper, for e4m3 on the dequantised scratch - bit for bit what the bf16 route gives on the
    dequantised weights."""
    wst = Worst("wrapper M=33")
    M, K, N = 33, 384, 33
    x, w, b = _inputs(kind, 11, M, K, N, True)
    for route in ("linear", "logits"):
        y8, info8 = eng.vlm_linear(x, w, b, weight_format="fp8", route=route)
        y16, info16 = eng.vlm_linear(x, R.dq(w), b, weight_format="bf16", route=route)
        assert info8["family"] == "wrapper" and info16["family"] == "wrapper", (info8, info16)
        assert np.array_equal(y8, y16)
        _check_linear(wst, (kind, route), kind, "fp8", route, x, w, b, y8, R.depth_wrapper(K, True))
    with pytest.raises(Exception, match="unsupported layer"):
        eng.vlm_linear(x, w, b, weight_format="bf16", kernel="gemm32")
    wst.show()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm32(eng, fmt, kind):
    wst = Worst(f"gemm32 {fmt} {kind}")
    seen = set()
    for ci, (M, K, N, route, bias) in enumerate(GEMM_CASES):
        x, w, b = _inputs(kind, 1000 + ci, M, K, N, bias)
        y, info = eng.vlm_linear(x, w, b, weight_format=fmt, route=route)          # auto: 4 .. 32 rows of K % 128 == 0 are the GEMM's
        splits = R.gemm32_splits(N, K)[0]
        direct = route == "logits" and not bias and splits == 1
        assert info == dict(family="gemm32", mr=0, splits=splits, direct=direct), ((M, K, N, route, bias), info)
        seen.add((splits, direct))
        _check_linear(wst, (fmt, M, K, N, kind, route, bias), kind, fmt, route, x, w, b, y, R.depth_gemm32(K, info["splits"], bias, direct))
    assert {s for s, _ in seen} == {1, 2, 9, 17} and (1, True) in seen and (1, False) in seen
    # 1 .. 3 rows through the forced GEMM (the batch rows past M are zero columns of the B operand)
    x, w, b = _inputs(kind, 77, 2, 1408, 33, True)
    y, info = eng.vlm_linear(x, w, b, weight_format=fmt, kernel="gemm32")
    assert info["family"] == "gemm32" and info["splits"] == 2, info
    _check_linear(wst, "forced", kind, fmt, "linear", x, w, b, y, R.depth_gemm32(1408, 2, True))
    wst.show()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm32_ldx(eng, fmt, kind):
    wst = Worst(f"gemm32 ldx {fmt}")
    M, K, N = 5, 384, 33
    x, w, b = _inputs(kind, 13, M, K, N, False, ldx=K + 24)
    y, info = eng.vlm_linear(x, w, b, weight_format=fmt)
    assert info["family"] == "gemm32" and info["splits"] == 1, info
    _check_linear(wst, kind, kind, fmt, "linear", x, w, b, y, R.depth_gemm32(K, 1, False))
    wst.show()


def _residual_inputs(kind, seed, M, N, n_ds):
    rng = np.random.default_rng(seed + 999331)
    slot = np.where(np.arange(M) % 3 == 0, -1, np.arange(M) % n_ds).astype(np.int32)          # text rows and image rows, every feature row used
    if kind == "exact":
        return rng.integers(-64, 65, (M, N)).astype(np.float32), rng.integers(-64, 65, (n_ds, N)).astype(np.float32), slot
    return rng.normal(0, 1, (M, N)).astype(np.float32), rng.normal(0, 1, (n_ds, N)).astype(np.float32), slot


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_ds", [False, True], ids=["plain", "ds"])
@pytest.mark.parametrize("fmt", FMTS)
def test_add_rmsnorm(eng, fmt, with_ds, kind):
    """o / down projection -> vlm_finish_add_rmsnorm_kernel<DS>: the new residual and the normed rows."""
    wst = Worst(f"add_rmsnorm {fmt} {'ds' if with_ds else 'plain'} {kind}")
    n_ds = 3
    for si, (N, K) in enumerate(ADD_NORM_SHAPES):
        for M in (5, 32):
            x, w, _ = _inputs(kind, 2000 + si, M, K, N, False)
            xres, ds, slot = _residual_inputs(kind, si, M, N, n_ds)
            g = np.random.default_rng(si).normal(1, 0.25, N).astype(np.float32)
            r, n, info = eng.vlm_linear(x, w, weight_format=fmt, route="add_rmsnorm", xres=xres, g=g, eps=EPS,
                                        slot=slot if with_ds else None, ds=ds if with_ds else None)
            assert info == dict(family="gemm32", mr=0, splits=R.gemm32_splits(N, K)[0], direct=False), info
            proj, S = R.ref_linear(R.bf16(x), R.weights_as(fmt, w))
            r0 = R.bf16(xres).astype(np.float64) + proj
            image = (slot >= 0)[:, None] & with_ds
            r1 = r0 + np.where(image, R.bf16(ds).astype(np.float64)[np.maximum(slot, 0)], 0.0)
            label = (fmt, with_ds, kind, M, N, K)
            if kind == "exact":
                want = R.bf16(xres.astype(np.float64) + R.bf16(proj))
                want = np.where(image, R.bf16(want.astype(np.float64) + ds[np.maximum(slot, 0)]), want)
                assert np.array_equal(r, want), (label, np.argwhere(r != want)[:4])
            else:
                D = R.depth_gemm32(K, info["splits"], False)
                bound = np.where(image, R.bound_residual(proj, S, r0, D, ds_sum=r1), R.bound_residual(proj, S, r0, D))
                assert wst.add(f"{fmt}/residual", r, r1, bound) <= 1.0, label
            n_ref, n_bound = R.bound_rmsnorm(r, R.bf16(g), EPS)
            assert wst.add(f"{fmt}/norm", n, n_ref, n_bound) <= 1.0, label
    wst.show()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_silu_mul(eng, fmt, kind):
    """gate | up as one launch -> vlm_finish_silu_mul_kernel."""
    from facet_amd.weights import quantize_e4m3_rows
    wst = Worst(f"silu_mul {fmt} {kind}")
    pinned = 0
    for si, (N, K) in enumerate(SILU_SHAPES):
        for M in (5, 32):
            x, w, _ = _inputs(kind, 3000 + si, M, K, N, False)
            if kind == "exact":
                w2 = R.exact_w(4000 + si, N, K, shift=3)
                assert all(R.exact_premises(x, w2, shift=3))
            else:
                w2 = 4.0 * R.random_w(4000 + si, N, K)
            assert not np.array_equal(w, w2) and (quantize_e4m3_rows(w)[1] != quantize_e4m3_rows(w2)[1]).all()
            h, info = eng.vlm_linear(x, w, weight_format=fmt, route="silu_mul", w2=w2)
            assert info == dict(family="gemm32", mr=0, splits=R.gemm32_splits(N, K, paired=True)[0], direct=False), info
            gs, Sg = R.ref_linear(R.bf16(x), R.weights_as(fmt, w))
            us, Su = R.ref_linear(R.bf16(x), R.weights_as(fmt, w2))
            label = (fmt, kind, M, N, K)
            if kind == "exact":
                gb, ub = R.bf16(gs).astype(np.float64), R.bf16(us).astype(np.float64)
                sat = gs >= 40.0
                pinned += int(sat.sum())
                assert np.array_equal(h[sat], R.bf16(gb * ub)[sat]), label
                assert wst.add(f"{fmt}/h(exact inputs)", h, R.silu(gb) * ub, R.bound_silu_mul(gb, None, ub, None, None)) <= 1.0, label
            else:
                D = R.depth_gemm32(K, info["splits"], False)
                assert wst.add(f"{fmt}/h", h, R.silu(gs) * us, R.bound_silu_mul(gs, Sg, us, Su, D)) <= 1.0, label
    assert kind != "exact" or pinned > 1000
    wst.show()


def test_repeated_calls_do_not_grow_device_memory(eng):
    """The hook frees what it packs: 60 calls that each pack 1.4 - 5.6 MB leave the free memory where it was (32 MiB of slack)."""
    import torch
    x, w, b = _inputs("random", 1, 5, 8704, 160, True)
    eng.vlm_linear(x, w, b, weight_format="fp8")
    free0 = torch.cuda.mem_get_info(0)[0]
    for fmt in FMTS * 10:
        eng.vlm_linear(x, w, b, weight_format=fmt)
        eng.vlm_linear(x, w, weight_format=fmt, route="silu_mul", w2=w[::-1].copy())
        with pytest.raises(Exception, match="unsupported layer"):          # the error path frees them too
            eng.vlm_linear(x, w, b, weight_format=fmt, kernel="gemv")
    lost = free0 - torch.cuda.mem_get_info(0)[0]
    assert lost < (32 << 20), f"{lost >> 20} MiB of device memory lost over 60 calls"
