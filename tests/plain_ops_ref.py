"""Plain numpy float64 references of the pooling, resampling, row and small-GEMM operations of kernels_misc.hip, each with the error
bound a correct fp32 kernel must meet. Every function is written from the operation's definition (the torch documentation), not from the
kernel; tests/test_plain_ops_host.py pins each to torch.nn.functional in float64. Inputs are taken AS ROUNDED to the element type
(`rnd`), so a reference never pays for the rounding of an operand.

Bounds. u = 2^-24 is the unit roundoff of fp32 (half an ulp, relative). Every non-exact check is |got - ref| <= A + store(ref), where A is
the bound of the kernel's fp32 arithmetic returned beside the reference and store(ref) = ulp_E(ref) / 2 * (1 + 2^-10) is the one rounding
to a 2-byte output type E (0 for fp32, whose store rounding is inside A). The (1 + 2^-10) covers the value that is rounded, ref + error,
lying in the binade above ref. The kernels are compiled without contraction, so every multiply and add rounds once.

  sums      a sum of n terms through a chain of c rounded additions is within c u sum|term| of the exact sum. The row kernels add
            ceil(d / 64) values per lane serially (the register forms: a 2-level tree and up to 8 accumulations, which is no more), then
            6 shuffle steps: c = ceil(d / 64) + 6 (+ 4 for the softmax register forms at small d, `SUM_EXTRA`).
  bilinear  out = sum of four w v. Each term passes through at most 6 roundings (1 - l, two products, inner sum, outer product, outer
            sum): 8 u sum|w v|. The source coordinate ((dst + 0.5) * (in / out) - 0.5 in fp32: quotient, product, difference) is within
            u (2 t + |src|) of the exact one, t = (dst + 0.5) in / out; bilinear interpolation is continuous and piecewise linear, so
            that moves the result by at most the coordinate error times the steepest slope of the cells the coordinate can fall into
            (the cell of the exact coordinate and its two neighbours).
  avg pool  (window + 1) u sum|x| / window: window - 1 additions and the division.
  LayerNorm y = (x - mean) rstd g + b.  e_mean = c u sum|x| / d + u |mean| (sum, division).  The centred values t carry e_mean + u |t|
            each, so sum t^2 is off by at most 2 e_mean sum|t| + (c + 4) u sum t^2 (squares, their sum, the division by d), and
            rstd = 1 / sqrt(var + eps) by the relative e_rstd = dvar / (2 (var + eps)) + 5 u (the sum with eps, sqrtf and the division at
            2 u each). A = |g| rstd e_mean + |y - b| (e_rstd + 3 u) + u |y|: the shift of the mean, the scale, the three products'
            roundings and the final sum's.
  softmax   p_i = exp(x_i - max) / sum. x - max rounds by u |x - max|, which is a relative u |x_i - max| of the exponential; expf is
            within 1 ulp (2 u). The sum inherits the weighted mean of its terms' relative errors plus c u; reciprocal and product 3 u.
            A = p_i u (|x_i - max| + E_p|x - max| + c + 7).
  GEMM/conv z = sum x w through a chain of `chain` roundings (given by the caller per route): (chain + 6) u sum|x w| |scale|, plus u for the
            product with scale and u for the sum with shift, pushed through the activation's Lipschitz constant, plus the error of
            evaluating the activation itself (`act_eval`).
  tap route the 2-byte narrow convolution rounds each of the KH KW per-tap partial sums z_t to the element type before they are added:
            sum_t ulp_E(z_t) / 2 |scale| more (conv2d returns the z_t)."""
import zlib

import numpy as np

U = 2.0 ** -24
SUM_EXTRA = 4
F16_MAX = 65504.0
MANT = {"f32": 23, "bf16": 7, "f16": 10}


# ---- element types ---------------------------------------------------------------------------------------------------------------------
def rnd(a, elem):
    """a rounded to nearest even in `elem` ("f32", "bf16", "f16": saturating, as every f16 store of the engine), as float64."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if elem == "f32":
        return a.astype(np.float64)
    if elem == "f16":
        return np.clip(a, -F16_MAX, F16_MAX).astype(np.float16).astype(np.float64)
    assert elem == "bf16", elem
    b = a.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32).astype(np.float64)


def ulp(v, elem):
    """Spacing of `elem` at |v| (the binade of v; f16 below 2^-14: the subnormal spacing 2^-24)."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(np.where(v > 0, v, 1e-300))
    out = np.ldexp(1.0, e - 1 - MANT[elem])
    return np.maximum(out, 2.0 ** -24) if elem == "f16" else np.maximum(out, 2.0 ** -149)


def store(ref, elem):
    """The rounding of the one store to `elem` (module docstring); 0 for fp32."""
    return 0.0 * np.abs(ref) if elem == "f32" else ulp(ref, elem) / 2 * (1 + 2.0 ** -10)


# ---- pooling and resampling: x [n, c, h, w] --------------------------------------------------------------------------------------------
def pool_out(size, k, stride, pad, ceil_mode):
    """torch.nn.MaxPool2d's output size: floor or ceil of (size + 2 pad - k) / stride + 1; with ceil_mode the last window must start
    inside the input or its left padding."""
    num = size + 2 * pad - k
    o = (-(-num // stride) if ceil_mode else num // stride) + 1
    if ceil_mode and (o - 1) * stride >= size + pad:
        o -= 1
    return o


def maxpool(x, k, stride, pad, ceil_mode=False):
    """max over the window [i stride - pad, i stride - pad + k) clipped to the input (padding counts as -inf)."""
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    ho, wo = pool_out(h, k, stride, pad, ceil_mode), pool_out(w, k, stride, pad, ceil_mode)
    big = np.full((n, c, (ho - 1) * stride + k + pad, (wo - 1) * stride + k + pad), -np.inf)
    big[:, :, pad:pad + h, pad:pad + w] = x
    out = np.full((n, c, ho, wo), -np.inf)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, big[:, :, dy:dy + (ho - 1) * stride + 1:stride, dx:dx + (wo - 1) * stride + 1:stride])
    assert np.isfinite(out).all()
    return out


def _src(o, size_in, size_out):
    """align_corners=False: exact source coordinate of output index o, clamped at 0 -> (i0, i1, l, fp32 coordinate error)."""
    t = (o + 0.5) * size_in / size_out
    s = np.maximum(t - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), size_in - 1)
    i1 = np.minimum(i0 + 1, size_in - 1)
    return i0, i1, s - i0, U * (2 * t + s)


def bilinear(x, ho, wo):
    """F.interpolate(mode="bilinear", align_corners=False) -> (ref, A)."""
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    y0, y1, ly, ey = _src(np.arange(ho), h, ho)
    x0, x1, lx, ex = _src(np.arange(wo), w, wo)
    Y0, X0, Y1, X1 = y0[:, None], x0[None, :], y1[:, None], x1[None, :]
    LY, LX = ly[:, None], lx[None, :]
    terms = [((1 - LY) * (1 - LX), x[:, :, Y0, X0]), ((1 - LY) * LX, x[:, :, Y0, X1]), (LY * (1 - LX), x[:, :, Y1, X0]), (LY * LX, x[:, :, Y1, X1])]
    ref = sum(wt * v for wt, v in terms)
    mag = sum(np.abs(wt * v) for wt, v in terms)
    # steepest slope along each axis over the cells the coordinate can fall into: rows y0 - 1 .. y0 + 1 (columns x0 - 1 .. x0 + 1) of the
    # first differences, in the columns (rows) that take part; past the border the clamped interpolation is flat
    dy = np.zeros((n, c, h + 2, w))
    dy[:, :, 1:h, :] = np.abs(np.diff(x, axis=2))          # dy[r + 1] = |x[r + 1] - x[r]|, r = -1 and r >= h - 1: 0
    dx = np.zeros((n, c, h, w + 2))
    dx[:, :, :, 1:w] = np.abs(np.diff(x, axis=3))
    sy = np.zeros_like(ref)
    sx = np.zeros_like(ref)
    for r in (-1, 0, 1):
        for col in (X0, X1):
            sy = np.maximum(sy, dy[:, :, np.clip(Y0 + r + 1, 0, h + 1), col])
        for row in (Y0, Y1):
            sx = np.maximum(sx, dx[:, :, row, np.clip(X0 + r + 1, 0, w + 1)])
    return ref, 8 * U * mag + ey[:, None] * sy + ex[None, :] * sx


def adaptive_windows(size_in, size_out):
    """[floor(i size_in / size_out), ceil((i + 1) size_in / size_out)) for every output index."""
    return [((i * size_in) // size_out, -(-((i + 1) * size_in) // size_out)) for i in range(size_out)]


def adaptive_avgpool(x, ho, wo):
    """F.adaptive_avg_pool2d -> (ref, A)."""
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    ref, A = np.empty((n, c, ho, wo)), np.empty((n, c, ho, wo))
    for i, (hs, he) in enumerate(adaptive_windows(h, ho)):
        for j, (ws, we) in enumerate(adaptive_windows(w, wo)):
            win = x[:, :, hs:he, ws:we]
            cnt = (he - hs) * (we - ws)
            ref[:, :, i, j] = win.sum(axis=(2, 3)) / cnt
            A[:, :, i, j] = (cnt + 1) * U * np.abs(win).sum(axis=(2, 3)) / cnt
    return ref, A


# ---- rows: x [rows, d] -----------------------------------------------------------------------------------------------------------------
def _chain(d):
    return -(-d // 64) + 6


def layernorm(x, g, b, eps):
    """F.layer_norm over the last axis (biased variance) -> (ref, A)."""
    x, g, b = np.asarray(x, np.float64), np.asarray(g, np.float64), np.asarray(b, np.float64)
    d = x.shape[1]
    c = _chain(d)
    mean = x.mean(axis=1, keepdims=True)
    t = x - mean
    var = (t * t).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    ref = t * rstd * g + b
    e_mean = c * U * np.abs(x).sum(axis=1, keepdims=True) / d + U * np.abs(mean)
    dvar = (2 * e_mean * np.abs(t).sum(axis=1, keepdims=True) + (c + 4) * U * (t * t).sum(axis=1, keepdims=True)) / d
    e_rstd = dvar / (2 * (var + eps)) + 5 * U
    A = np.abs(g) * rstd * e_mean + np.abs(ref - b) * (e_rstd + 3 * U) + U * np.abs(ref)
    return ref, A


def softmax(x):
    """softmax over the last axis -> (ref, A)."""
    x = np.asarray(x, np.float64)
    d = x.shape[1]
    dist = x.max(axis=1, keepdims=True) - x
    e = np.exp(-dist)
    ref = e / e.sum(axis=1, keepdims=True)
    A = ref * U * (dist + (ref * dist).sum(axis=1, keepdims=True) + _chain(d) + SUM_EXTRA + 7)
    return ref, A


def split_pair(y):
    """The f16 pair of a value: hi = rn_f16(y), lo = rn_f16(y - hi)."""
    hi = rnd(y, "f16")
    return hi, rnd(np.asarray(y, np.float64) - hi, "f16")


# ---- contractions -----------------------------------------------------------------------------------------------------------------------
LIPSCHITZ = {None: 1.0, "relu": 1.0, "gelu": 1.13, "sigmoid": 0.25, "softplus": 1.0, "quickgelu": 1.1}


def act(v, name):
    """The activations of fe_apply_act by their definitions (torch: relu, gelu (erf form), sigmoid, softplus, x sigmoid(1.702 x))."""
    from math import erf
    v = np.asarray(v, np.float64)
    if name is None:
        return v
    if name == "relu":
        return np.maximum(v, 0.0)
    if name == "gelu":
        return 0.5 * v * (1.0 + np.vectorize(erf)(v / np.sqrt(2.0)))
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if name == "softplus":
        return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))
    assert name == "quickgelu", name
    return v / (1.0 + np.exp(-1.702 * v))


def act_eval(v, out, name):
    """Error of evaluating the activation in fp32 at an exact argument v (out = act(v)).
    gelu: erff within 2 ulp, its argument's rounding and the sum 1 + erf leave 1 + erf within 6 u absolutely: 3 u |v|, and three more
    roundings 3 u |out|. sigmoid: the fast exponential is the hardware's 2^z (1 ulp) of z = -v log2 e, whose rounding is a relative
    u |v| of the result: e within (2 |v| + 4) u; d sigmoid / d e <= sigmoid / e, so sigmoid (2 |v| + 4) u, and two roundings. softplus: expf
    and log1pf within 1 ulp each, their conditioning <= 1: 8 u |out|. quickgelu: as sigmoid at 1.702 v (the product rounds too)."""
    v, out = np.abs(v), np.abs(out)
    if name in (None, "relu"):
        return 0.0 * v
    if name == "gelu":
        return 4 * U * (v + out)
    if name == "sigmoid":
        return out * (2 * v + 6) * U
    if name == "softplus":
        return 8 * U * out
    return out * (3.5 * v + 8) * U


def epilogue(z, mag, chain, scale, shift, name, res=None, res_after_act=False):
    """act(z scale + shift (+ res)) (+ res) and its bound from z = sum x w, mag = sum |x w| -> (ref, A). scale / shift broadcast or None."""
    sc = 1.0 if scale is None else np.asarray(scale, np.float64)
    sh = 0.0 if shift is None else np.asarray(shift, np.float64)
    v = z * sc + sh
    e = (chain + 6) * U * mag * np.abs(sc) + U * np.abs(z * sc) + U * np.abs(v)
    if res is not None and not res_after_act:
        v = v + res
        e = e + U * np.abs(v)
    out = act(v, name)
    A = LIPSCHITZ[name] * e + act_eval(v, out, name)
    if res is not None and res_after_act:
        out = out + res
        A = A + U * np.abs(out)
    return out, A


def gemm(x, w, K, chain=None):
    """x [M, >= K] . w [N, >= K]^T over the first K columns -> (z, sum |x w|, chain of the skinny kernel: ceil(K / 256) iterations of a lane,
    each a 4-term dot product (4 roundings) and one accumulation)."""
    x, w = np.asarray(x, np.float64)[:, :K], np.asarray(w, np.float64)[:, :K]
    return x @ w.T, np.abs(x) @ np.abs(w).T, -(-K // 256) + 4


def conv2d(x, w, stride=1, pad=0, dil=1):
    """Cross-correlation as torch.nn.functional.conv2d defines it: out[n, o, i, j] = sum_{c, a, b} x[n, c, i s - p + a d, j s - p + b d]
    w[o, c, a, b], zero padding -> (z, sum |x w|, per-tap partial sums z_t [KH KW, n, o, ho, wo])."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, cin, h, ww = x.shape
    cout, _, kh, kw = w.shape
    ho, wo = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1, (ww + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    big = np.zeros((n, cin, h + 2 * pad, ww + 2 * pad))
    big[:, :, pad:pad + h, pad:pad + ww] = x
    taps = np.empty((kh * kw, n, cout, ho, wo))
    mag = np.zeros((n, cout, ho, wo))
    for a in range(kh):
        for b in range(kw):
            win = big[:, :, a * dil:a * dil + (ho - 1) * stride + 1:stride, b * dil:b * dil + (wo - 1) * stride + 1:stride]
            taps[a * kw + b] = np.einsum("nchw,oc->nohw", win, w[:, :, a, b])
            mag += np.einsum("nchw,oc->nohw", np.abs(win), np.abs(w[:, :, a, b]))
    return taps.sum(axis=0), mag, taps


# ---- shared by the GPU tests ------------------------------------------------------------------------------------------------------------
class Worst:
    """Collects failures and the worst err / bound per key; report() prints the ratios, then asserts."""

    def __init__(self, title):
        self.title, self.ratio, self.fails = title, {}, []

    def exact(self, key, what, got, want):
        self.ratio.setdefault(key, 0.0)
        if got.shape != want.shape or not np.array_equal(got, want):
            self.fails.append(f"{key} {what}: not bit-equal" + (f" ({int((got != want).sum())} of {got.size})" if got.shape == want.shape else f" shape {got.shape} != {want.shape}"))

    def close(self, key, what, got, ref, bound):
        err = np.abs(got.astype(np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(err == 0, 0.0, err / bound).max()) if np.isfinite(got).all() else float("inf")
        self.ratio[key] = max(self.ratio.get(key, 0.0), r)
        if not r <= 1.0:
            self.fails.append(f"{key} {what}: err / bound {r:.3g} (worst err {err.max():.3g})")

    def report(self):
        print(f"\n{self.title}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.ratio.items())))
        assert not self.fails, f"{len(self.fails)} failures, first: " + "; ".join(self.fails[:5])


def case_rng(*key):
    """A generator seeded by the case (stable across processes: str hashes are salted)."""
    return np.random.default_rng(zlib.crc32(repr(key).encode()))
