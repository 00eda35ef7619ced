"""What tests/test_vlm_linear_gpu.py and tests/test_vlm_linear_host.py share: the inputs of the decode-projection cases, their float64
references, the rounding bounds of every route (derivations: the docstring of test_vlm_linear_gpu.py) and the planted faults that
show the checks can fail. numpy only; nothing here touches a GPU."""
import numpy as np

from facet_amd.weights import _round_bf16, dequantize_e4m3_rows, quantize_e4m3_rows

U32 = 2.0 ** -24          # unit roundoff of fp32
U16 = 2.0 ** -9           # bf16 has 8 significant bits: half an ulp of v is 2^-9 times the power of two above v (half_ulp_bf16)
TINY = 2.0 ** -126        # the smallest normal fp32 / bf16 value
SILU_TINY = 2.0 ** -121   # expf(-g) overflows for g < -88.73 and x / inf is 0, where silu(g) is still up to 88.73 e^-88.72 = 2.6e-37 < 2^-121


def bf16(a):
    """The nearest-even bf16 value of every element, as float32 (the values must be fp32-representable or the result of fp32 arithmetic)."""
    return _round_bf16(np.asarray(a, np.float64).astype(np.float32))


def dq(w):
    """What an e4m3 layer holds for w: dequantize(quantize(bf16(w))), float32."""
    return dequantize_e4m3_rows(*quantize_e4m3_rows(np.asarray(w, np.float32)))


def weights_as(fmt, w):
    return dq(w) if fmt == "fp8" else bf16(w)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _nonzero_ints(rng, lo, hi, shape):
    v = rng.integers(lo, hi, shape)          # [lo, hi) without zero: the upper half moves up by one
    return np.where(v >= 0, v + 1, v).astype(np.float32)


def row_scales(N, shift=0):
    return np.ldexp(1.0, ((np.arange(N) + shift) % 7) - 3).astype(np.float32)


def exact_w(seed, N, K, shift=0):
    """Integers in [-8, 8] without zeros, every row holding an 8 (so its e4m3 scale is decided by the row factor alone), row n times
    2^(((n + shift) % 7) - 3): neighbouring rows have different e4m3 scales (and with another shift, so have the same rows of a second
    matrix), and every value has at most 4 significant bits."""
    rng = np.random.default_rng(seed)
    w = _nonzero_ints(rng, -8, 8, (N, K))
    w[np.arange(N), np.arange(N) % K] = 8.0 * np.where(np.arange(N) % 2, -1.0, 1.0)
    return w * row_scales(N, shift)[:, None]


def exact_x(seed, M, K, ldx=None):
    """Integers in [-3, 3] without zeros, every row different; [M, ldx] with the columns past K filled with 3 (a kernel that read them
    would be off by whole units)."""
    rng = np.random.default_rng(seed + 7919)
    ldx = K if ldx is None else ldx
    x = np.full((M, ldx), 3.0, np.float32)
    x[:, :K] = _nonzero_ints(rng, -3, 3, (M, K))
    for m in range(1, M):          # no two rows equal (tiny K could repeat one by chance)
        while any(np.array_equal(x[m, :K], x[j, :K]) for j in range(m)):
            x[m, :K] = _nonzero_ints(rng, -3, 3, K)
    return x


def exact_bias(seed, N):
    return np.random.default_rng(seed + 104729).integers(-40, 41, N).astype(np.float32)


def exact_premises(x, w, bias=None, shift=0):
    """The two premises of an exact case. (1) Every partial sum of row n is an integer multiple of its row factor 2^s below 2^24 of
    them, and with the (integer) bias the sum is an integer multiple of min(2^s, 1) below 2^24 of those: any fp32 summation order is
    exact. (2) The e4m3 round trip of w is the identity."""
    K = w.shape[1]
    S = np.abs(np.asarray(x[:, :K], np.float64)) @ np.abs(np.asarray(w, np.float64)).T          # [M, N]
    if bias is not None:
        S = S + np.abs(bias)
    unit = np.minimum(row_scales(w.shape[0], shift).astype(np.float64), 1.0)
    return bool((S / unit < 2.0 ** 24).all()), bool(np.array_equal(dq(w), w) and np.array_equal(bf16(w), w))


def random_x(seed, M, K, ldx=None):
    rng = np.random.default_rng(seed + 15485863)
    ldx = K if ldx is None else ldx
    return rng.normal(0, 1, (M, ldx)).astype(np.float32)


def random_w(seed, N, K):
    return np.random.default_rng(seed).normal(0, 1, (N, K)).astype(np.float32)


# ---- references -----------------------------------------------------------------------------------------------------------------------
def ref_linear(x, w, bias=None):
    """float64 y = x[:, :K] w^T + bias and S = sum_k |x_k w_k| + |bias| on values as given (the callers pass what the kernel holds)."""
    K = w.shape[1]
    x64, w64 = np.asarray(x[:, :K], np.float64), np.asarray(w, np.float64)
    y, S = x64 @ w64.T, np.abs(x64) @ np.abs(w64).T
    if bias is not None:
        y, S = y + np.asarray(bias, np.float64), S + np.abs(np.asarray(bias, np.float64))
    return y, S


def silu(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


# ---- the split rule of vlm_gemm32_partials and the chain depths D of every route --------------------------------------------------------
def gemm32_splits(N, K, paired=False):
    """(splits, stages per split) of the 32-row GEMM: the formula of vlm_gemm32_partials."""
    ntiles = (N + 31) // 32
    cols = (ntiles + 3) // 4
    allcols = 2 * cols if paired else cols
    nst = K // 128
    splits = max(1, min(nst // 4, (768 + allcols - 1) // allcols))
    per = (nst + splits - 1) // splits
    return (nst + per - 1) // per, per


def depth_gemv(K, fmt, bias):
    """bf16: a lane's four dot2 per 8-element chunk (8 products), ceil(K / 2048) chunks for the busiest lane; e4m3: 16 products per
    16-code chunk, ceil(K / 4096) chunks. Then 6 butterfly additions, 2 levels over the four waves, the bias."""
    chunks = -(-K // 4096) * 16 if fmt == "fp8" else -(-K // 2048) * 8
    return chunks + 6 + 2 + (1 if bias else 0)


def depth_gemm32(K, splits, bias, direct=False):
    """128 products per stage on one accumulator (8 MFMA of 16 products per output), ceil(K / 128 / splits) stages per split; then the
    split sum (one addition per split, from zero) and the bias. A direct write has neither."""
    per = -(-(K // 128) // splits)
    return 128 * per + (0 if direct else splits + (1 if bias else 0))


def depth_wrapper(K, bias):
    """Any order of K fp32 additions (the shared layer wrapper is not this file's subject): the worst chain."""
    return K + (1 if bias else 0)


# ---- the shapes of the GPU cases ------------------------------------------------------------------------------------------------------
GEMV_K = {"bf16": [8, 520, 2048, 2056, 6152, 12296], "fp8": [16, 1040, 4096, 4112, 12304, 24592]}
# (M, K, N, route, bias)
GEMM_CASES = [
    (4, 128, 1, "linear", False), (5, 128, 31, "linear", True), (31, 128, 160, "logits", False), (32, 128, 100, "linear", False),
    (5, 384, 129, "logits", False), (5, 384, 129, "logits", True), (32, 384, 160, "linear", True), (31, 384, 33, "linear", False),
    (4, 1408, 31, "linear", False), (31, 1408, 100, "logits", True), (32, 1408, 129, "linear", False), (5, 1408, 160, "linear", True),
    (5, 4608, 129, "linear", True), (32, 4608, 129, "logits", False), (32, 4608, 33, "linear", False), (31, 4608, 1, "logits", True),
    (5, 8704, 33, "linear", False), (32, 8704, 33, "logits", True), (4, 8704, 100, "linear", True), (31, 8704, 31, "logits", False),
]
assert {gemm32_splits(N, K)[0] for _, K, N, _, _ in GEMM_CASES} == {1, 2, 9, 17}
assert {((N + 31) // 32) % 4 for _, _, N, _, _ in GEMM_CASES} >= {0, 1, 2} and any(N % 32 for _, _, N, _, _ in GEMM_CASES)
ADD_NORM_SHAPES = [(64, 8704), (512, 4608), (4352, 384)]          # (N = d, K): 17, 9 and 1 splits
assert [gemm32_splits(N, K)[0] for N, K in ADD_NORM_SHAPES] == [17, 9, 1]
SILU_SHAPES = [(N, K) for N in (36, 100, 132) for K in (384, 4608)]
assert {gemm32_splits(N, K, paired=True)[0] for N, K in SILU_SHAPES} == {1, 9}


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------
def e32(D, S):
    return 2.0 * D * U32 * S


def half_ulp_bf16(v):
    """Half a unit in the last of bf16's 8 significant bits at magnitude v: 2^-9 * 2^ceil(log2 v), i.e. between 2^-9 v and 2^-8 v. The
    error of round-to-nearest is at most this, and reaches it (a tie): 2^-9 v itself is NOT a bound - 1 + 2^-8 rounds to 1, off by
    2^-8 - which is why the power of two stands here (test_vlm_linear_host.py::test_bf16_rounding_term)."""
    f, x = np.frexp(np.abs(np.asarray(v, np.float64)))          # |v| = f 2^x, f in [0.5, 1): the power of two above v is 2^x
    return np.where(f > 0, np.ldexp(U16, x), 0.0)


def add_bf16(ref, e):
    """The bound after one more round-to-nearest bf16 rounding of a value within e of ref."""
    return e + half_ulp_bf16(np.abs(ref) + e)


def add_f32(ref, e, n=1):
    """... after n more fp32 roundings (2 u each, the convention of e32)."""
    return e + 2.0 * n * U32 * (np.abs(ref) + e)


def bound_residual(proj, S, r, D, ds_sum=None):
    """|returned residual - r|, r = xres + proj: the split sum within e32, its bf16 rounding, the fp32 addition of the residual, the bf16
    rounding of the stream; with DeepStack rows one more fp32 addition and bf16 rounding on r + ds."""
    e = add_bf16(proj, e32(D, S))
    e = add_bf16(r, add_f32(r, e))
    if ds_sum is not None:
        e = add_bf16(ds_sum, add_f32(ds_sum, e))
    return e


def bound_rmsnorm(r, g, eps):
    """(float64 RMSNorm(r) g, the bound of |returned norm - it|) for the RETURNED residual r [M, d]: the sum of squares has only
    positive terms, so its relative error is its chain depth in u - per 4096-column trip a square (1), a two-level tree (2) and the
    running addition (1), then 6 butterfly and 16 cross-wave additions; the mean (a division) and + eps; half of that through the
    inverse square root, whose instruction is good to 1 ulp = 2 u; then t = v rs, its bf16 rounding, the product with g, the bf16 store."""
    r, g = np.asarray(r, np.float64), np.asarray(g, np.float64)
    trips = -(-r.shape[-1] // 4096)
    rel_rs = ((4 * trips + 6 + 16 + 2) / 2.0 + 2.0) * 2.0 * U32
    t = r / np.sqrt((r * r).mean(-1, keepdims=True) + eps)
    e = add_bf16(t, add_f32(t, rel_rs * np.abs(t)))
    n = g * t
    return n, add_bf16(n, add_f32(n, np.abs(g) * e))


def bound_silu_mul(g, Sg, u, Su, D):
    """|returned h - silu(g) u|: both split sums within e32 and rounded to bf16; silu's slope is at most 1.1; its fp32 evaluation is
    expf (1 ulp = 2 u), 1 + e and the division (u each); its bf16 rounding; the fp32 product; the bf16 store. For a gate below
    -88.73 expf overflows and the quotient is 0 where silu is up to 2^-121: + 2^-121 on silu; a product below the smallest normal
    fp32 / bf16 value 2^-126 is rounded (or flushed to zero) absolutely: + 2^-126. D = None: g and u are the kernel's own bf16 inputs of silu and of the product (the exact cases), which
    leaves the terms after the slope."""
    eg, eu = (0.0, 0.0) if D is None else (add_bf16(g, e32(D, Sg)), add_bf16(u, e32(D, Su)))
    s = silu(g)
    es = add_bf16(s, add_f32(s, 1.1 * eg, n=4)) + SILU_TINY          # 2 u + u + u, doubled as every fp32 term is
    h = s * np.asarray(u, np.float64)
    ep = es * np.abs(u) + eu * np.abs(s) + es * eu
    return add_bf16(h, add_f32(h, ep)) + TINY


def worst(y, ref, bound):
    """max err / bound (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(y, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max())


# ---- planted faults: a wrong kernel's output, computed in float64 from the values the kernel holds ----------------------------------------
def fault_dropped_chunk(x, w, bias, chunk):
    """The last `chunk` (8 or 16) elements of K never multiplied: the tail chunk of the one lane that owns it."""
    K = w.shape[1]
    wz = np.array(w, np.float64)
    wz[:, K - chunk:] = 0
    return ref_linear(x, wz, bias)[0]


def fault_neighbour_scale(x, codes, exps, bias):
    """e4m3: row n's codes scaled by row n + 1's scale (the last row by the first's)."""
    return ref_linear(x, dequantize_e4m3_rows(codes, np.roll(exps, -1)), bias)[0]


def split_partials(x, w, splits, per):
    K = w.shape[1]
    x64, w64 = np.asarray(x[:, :K], np.float64), np.asarray(w, np.float64)
    return [x64[:, s * per * 128:(s + 1) * per * 128] @ w64[:, s * per * 128:(s + 1) * per * 128].T for s in range(splits)]


def fault_split_left_out(x, w, bias, splits, per, which):
    p = split_partials(x, w, splits, per)
    return sum(p[s] for s in range(splits) if s != which) + (0 if bias is None else np.asarray(bias, np.float64))


def fault_partials_rounded(x, w, bias, splits, per):
    return sum(bf16(p).astype(np.float64) for p in split_partials(x, w, splits, per)) + (0 if bias is None else np.asarray(bias, np.float64))


def fault_tail_tile_last_row(y):
    """Every column of the last (partial) 32-column tile holds column N - 1: the clamped row taken for all of them."""
    y = np.array(y)
    N = y.shape[1]
    y[:, (N - 1) // 32 * 32:] = y[:, N - 1:N]
    return y


def fault_rows_swapped(x, w, bias, m):
    xs = np.array(x)
    xs[[m, m + 1]] = xs[[m + 1, m]]
    return ref_linear(xs, w, bias)[0]
