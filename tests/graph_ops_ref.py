"""Plain numpy float64 references of the operators of the ONNX-subset graph runtime (facet_amd/csrc/onnx_graph.hip over kernels_graph.hip
and the shared kernels), one function per operator, each written from the ONNX operator specification on ONNX-layout arrays (NCHW) and the
node's attributes. Nothing here reads oracle/onnx_ref.py or torch; tests/test_graph_ops_host.py holds the two against each other.

Every function returns (ref, A): the float64 value and the elementwise bound of a correct fp32 evaluation, |got - ref| <= A + ulp32(ref) / 2,
built the way tests/plain_ops_ref.py builds its bounds (u = 2^-24; every multiply and add rounds once). A is None where the operator only
moves or selects stored values: the result must then be equal bit for bit. Inputs are taken as stored (fp32 values in float64), so a
reference never pays for the rounding of an operand.

  exact          Relu, MaxPool, nearest Resize, Concat, Flatten, Transpose, Reshape, Squeeze, Unsqueeze, Identity, Dropout
  LeakyRelu/PRelu, Add/Sub/Mul   u |ref|                                  (one rounding)
  Div            3 u |ref|            (a constant divisor becomes a rounded reciprocal followed by a multiply)
  affine         u (|x s| + |ref|)    (BatchNormalization alone, tensor (op) constant: x s rounds, the sum with the shift rounds)
  AveragePool    (taps + 1) u sum|x| / divisor                            (taps - 1 additions and the division)
  GlobalAveragePool, linear Resize, Softmax: the bounds of plain_ops_ref (the same kernels)
  Conv/Gemm/MatMul  z = sum x w over K terms: (K + 2) u sum|x w| |scale| + u |v|, v = z scale + shift: the worst-case fp32 dot product in
                 any order, the product with the scale, the sum with the shift. Depthwise: K = taps. A residual added before the
                 activation: + u |v + res|. Then the activation's Lipschitz constant times that, plus the error of evaluating the
                 activation itself (Sigmoid: plain_ops_ref.act_eval, the fast exponential; PRelu on the negative side: u |out|); a residual
                 added after the activation: + u |out|.

Folded constants. An inference BatchNormalization is a per-channel scale s = gamma / sqrt(var + eps) and shift beta - mean s (+ bias s
behind a convolution). These are operands of the kernel, prepared once per model, not part of its arithmetic: `fold` evaluates them in
fp32, one rounding per operation in the order written there, as any fp32 runtime does, and the references use them as stored.
The second opinion (torch, which does not fold) sees the difference of a few u |x s| and allows for it."""
from fractions import Fraction

import numpy as np

import plain_ops_ref as R

U = R.U


def ulp32(v):
    return R.ulp(v, "f32")


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def _chan(v, rank):
    """A per-channel vector (or None / scalar) shaped to broadcast along axis 1 of a rank-`rank` array."""
    if v is None or np.ndim(v) == 0:
        return v
    return np.asarray(v, np.float64).reshape((1, -1) + (1,) * (rank - 2))


# ---- activations -----------------------------------------------------------------------------------------------------------------------
def slope_for(slope, x):
    """PRelu's slope against x. The specification asks for unidirectional broadcasting; a 1-D slope of C values against [N, C, H, W] is the
    per-channel form legacy exporters write (C values, one per channel), read as [C, 1, 1]."""
    s = np.asarray(slope, np.float64)
    if s.ndim == 1 and x.ndim >= 3 and s.shape[0] == x.shape[1]:
        s = s.reshape((-1,) + (1,) * (x.ndim - 2))
    return np.broadcast_to(s, x.shape)


def act(v, kind, slope=None):
    """kind: None, "relu", "sigmoid", "prelu" (LeakyRelu is PRelu with a constant slope) -> (out, Lipschitz constant, evaluation error)."""
    v = np.asarray(v, np.float64)
    if kind is None:
        return v, 1.0, 0.0 * v
    if kind == "relu":
        return np.maximum(v, 0.0), 1.0, 0.0 * v
    if kind == "sigmoid":
        with np.errstate(over="ignore"):
            out = 1.0 / (1.0 + np.exp(-v))
        return out, 0.25, R.act_eval(v, out, "sigmoid")
    assert kind == "prelu", kind
    s = slope_for(slope, v)
    out = np.where(v > 0, v, v * s)
    return out, np.maximum(1.0, np.abs(s)), np.where(v > 0, 0.0, U * np.abs(out))


def activation(x, kind, slope=None):
    """A standalone activation node -> (ref, A); Relu is exact."""
    out, _, err = act(x, kind, slope)
    return out, (None if kind in (None, "relu") else err)


# ---- per-channel constants -------------------------------------------------------------------------------------------------------------
def fold(cout, bias=None, bn=None):
    """(scale, shift) of v = z scale + shift for a bias and / or BatchNormalization (gamma, beta, mean, var, eps), in fp32 (module docstring).
    scale is None without a BatchNormalization, shift None without either."""
    f = np.float32
    if bn is None:
        return None, (None if bias is None else np.asarray(bias, f).astype(np.float64))
    g, beta, mu, var = (np.asarray(t, f) for t in bn[:4])
    eps = f(bn[4])
    inv = f(1.0) / np.sqrt(var + eps)
    sc = g * inv
    sh = (np.zeros(cout, f) if bias is None else np.asarray(bias, f)) * sc + (beta - mu * sc)
    assert sc.dtype == f and sh.dtype == f
    return sc.astype(np.float64), sh.astype(np.float64)


def batchnorm_spec(x, bn):
    """BatchNormalization by its definition, (x - mean) / sqrt(var + eps) gamma + beta, all in float64 (what `fold` is checked against)."""
    g, beta, mu, var = (_chan(np.asarray(t, np.float64), x.ndim) for t in bn[:4])
    return (x - mu) / np.sqrt(var + float(np.float32(bn[4]))) * g + beta


def affine(x, scale, shift, kind=None, slope=None):
    """act(x scale + shift) per channel (axis 1): BatchNormalization alone, with the activation the runtime fuses behind it -> (ref, A)."""
    x = np.asarray(x, np.float64)
    sc = 1.0 if scale is None else _chan(scale, x.ndim)
    sh = 0.0 if shift is None else _chan(shift, x.ndim)
    v = x * sc + sh
    out, lip, err = act(v, kind, slope)
    return out, lip * U * (np.abs(x * sc) + np.abs(v)) + err


def binary_const(x, k, op, const_left=False):
    """x (op) k for a constant k broadcast by numpy's rules from ONNX layout ([C, 1, 1], [1, C, 1, 1], scalar); Add and Mul commute -> (ref, A)."""
    x, k = np.asarray(x, np.float64), np.asarray(k, np.float64)
    assert not const_left or op in ("Add", "Mul")
    ref = {"Add": x + k, "Sub": x - k, "Mul": x * k, "Div": x / k}[op]
    if op == "Div":
        return ref, 3 * U * np.abs(ref)
    xs = x * k if op == "Mul" else x
    return ref, U * (np.abs(xs) + np.abs(ref))


def binary(a, b, op):
    """a (op) b, equal shapes -> (ref, A)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    ref = {"Add": a + b, "Sub": a - b, "Mul": a * b, "Div": a / b}[op]
    return ref, (3 if op == "Div" else 1) * U * np.abs(ref)


# ---- contractions ----------------------------------------------------------------------------------------------------------------------
def conv(x, w, strides=1, pads=0, dilations=1, group=1):
    """ONNX Conv without its bias: out[n, o, i, j] = sum_{c, a, b} x[n, g(o) cpg + c, i sh - ph + a dh, j sw - pw + b dw] w[o, c, a, b], zero padding
    (pads: one value or (h, w), applied at both ends) -> (z, sum |x w|, K = terms per output)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, cin, h, wd = x.shape
    cout, cpg, kh, kw = w.shape
    (sh, sw), (ph, pw), (dh, dw) = _pair(strides), _pair(pads), _pair(dilations)
    assert cin == cpg * group and cout % group == 0
    opg = cout // group
    ho, wo = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (wd + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    big = np.zeros((n, cin, h + 2 * ph, wd + 2 * pw))
    big[:, :, ph:ph + h, pw:pw + wd] = x
    z, mag = np.zeros((n, cout, ho, wo)), np.zeros((n, cout, ho, wo))
    for g in range(group):
        xs, ws = big[:, g * cpg:(g + 1) * cpg], w[g * opg:(g + 1) * opg]
        for a in range(kh):
            for b in range(kw):
                win = xs[:, :, a * dh:a * dh + (ho - 1) * sh + 1:sh, b * dw:b * dw + (wo - 1) * sw + 1:sw]
                z[:, g * opg:(g + 1) * opg] += np.einsum("nchw,oc->nohw", win, ws[:, :, a, b])
                mag[:, g * opg:(g + 1) * opg] += np.einsum("nchw,oc->nohw", np.abs(win), np.abs(ws[:, :, a, b]))
    return z, mag, cpg * kh * kw


def gemm(x, w, transB=0):
    """Gemm without its bias (alpha = beta = 1, transA = 0) and MatMul by a constant matrix: x [M, K] . (w^T if transB else w) -> (z, sum |x w|, K)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    wm = w.T if transB else w
    assert x.ndim == 2 and x.shape[1] == wm.shape[0], (x.shape, w.shape, transB)
    return x @ wm, np.abs(x) @ np.abs(wm), x.shape[1]


def epilogue(z, mag, K, scale=None, shift=None, kind=None, slope=None, res=None, res_after_act=False, relu_last=False):
    """What follows a contraction inside one fused group: v = z scale + shift; a residual joins before the activation (then an optional
    Relu closes the group) or after it -> (ref, A), module docstring."""
    sc = 1.0 if scale is None else _chan(scale, z.ndim)
    sh = 0.0 if shift is None else _chan(shift, z.ndim)
    v = z * sc + sh
    e = (K + 2) * U * mag * np.abs(sc) + U * np.abs(v)
    if res is not None and not res_after_act:
        v = v + np.asarray(res, np.float64)
        e = e + U * np.abs(v)
    out, lip, err = act(v, kind, slope)
    A = lip * e + err
    if res is not None and res_after_act:
        out = out + np.asarray(res, np.float64)
        A = A + U * np.abs(out)
    if relu_last:
        out = np.maximum(out, 0.0)
    return out, A


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------
def pool_starts(size, k, stride, pad, ceil_mode):
    """Window starts (input coordinates) along one axis, by enumeration. Floor mode: every window that lies inside the padded extent
    [-pad, size + pad). Ceil mode (torch's rule): windows go on while the previous one has not reached the end of the padded extent, and a
    window must start inside the input or its left padding (start < size)."""
    starts, i = [], 0
    while True:
        s0 = i * stride - pad
        if ceil_mode:
            ok = i == 0 or ((i - 1) * stride - pad + k < size + pad and s0 < size)
        else:
            ok = s0 + k <= size + pad
        if not ok:
            return starts
        starts.append(s0)
        i += 1


def maxpool(x, k, stride, pad, ceil_mode=0):
    """MaxPool: the maximum over the in-image part of every window (padding never wins) -> (ref, None)."""
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    ys, xs = pool_starts(h, k, stride, pad, ceil_mode), pool_starts(w, k, stride, pad, ceil_mode)
    out = np.empty((n, c, len(ys), len(xs)))
    for i, y0 in enumerate(ys):
        for j, x0 in enumerate(xs):
            out[:, :, i, j] = x[:, :, max(y0, 0):min(y0 + k, h), max(x0, 0):min(x0 + k, w)].max(axis=(2, 3))
    return out, None


def avgpool(x, k, stride, pad, ceil_mode=0, count_include_pad=0):
    """AveragePool: the sum over the in-image part of a window divided by the number of in-image taps, or with count_include_pad by the
    number of taps inside the padded extent (a ceil-mode window is clipped to it) -> (ref, A)."""
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    ys, xs = pool_starts(h, k, stride, pad, ceil_mode), pool_starts(w, k, stride, pad, ceil_mode)
    ref, A = np.empty((n, c, len(ys), len(xs))), np.empty((n, c, len(ys), len(xs)))
    for i, y0 in enumerate(ys):
        for j, x0 in enumerate(xs):
            win = x[:, :, max(y0, 0):min(y0 + k, h), max(x0, 0):min(x0 + k, w)]
            taps = win.shape[2] * win.shape[3]
            padded = (min(y0 + k, h + pad) - max(y0, -pad)) * (min(x0 + k, w + pad) - max(x0, -pad))
            div = padded if count_include_pad else taps
            ref[:, :, i, j] = win.sum(axis=(2, 3)) / div
            A[:, :, i, j] = (taps + 1) * U * np.abs(win).sum(axis=(2, 3)) / div
    return ref, A


def global_avgpool(x):
    return R.adaptive_avgpool(x, 1, 1)


# ---- Resize / Upsample -----------------------------------------------------------------------------------------------------------------
def resize_len(size, scale):
    """Output length from a scale: floor(size * scale), the scale as the fp32 value the file holds."""
    return int(np.floor(size * float(np.float32(scale))))


def nearest_index(size_in, size_out, scale=None):
    """asymmetric + floor: x_orig = x_out / scale, scale = size_out / size_in when sizes are given, else the given fp32 scale. Exact (rationals)."""
    sc = Fraction(size_out, size_in) if scale is None else Fraction(float(np.float32(scale)))
    return np.array([min(int(Fraction(o) / sc), size_in - 1) for o in range(size_out)], np.int64)


def resize_nearest(x, ho, wo, scales=None):
    """-> (ref, None). scales: None (sizes given) or (scale_h, scale_w)."""
    x = np.asarray(x, np.float64)
    iy = nearest_index(x.shape[2], ho, None if scales is None else scales[0])
    ix = nearest_index(x.shape[3], wo, None if scales is None else scales[1])
    return x[:, :, iy][:, :, :, ix], None


def linear_coords(size_in, size_out, mode, scale=None):
    """Source coordinate of every output index for the specification's coordinate_transformation_mode, clamped to [0, size_in - 1]."""
    o = np.arange(size_out, dtype=np.float64)
    sc = size_out / size_in if scale is None else float(np.float32(scale))
    if mode == "half_pixel":
        s = (o + 0.5) / sc - 0.5
    elif mode == "pytorch_half_pixel":
        s = (o + 0.5) / sc - 0.5 if size_out > 1 else 0.0 * o
    elif mode == "align_corners":
        s = o * (size_in - 1) / (size_out - 1) if size_out > 1 else 0.0 * o
    else:
        assert mode == "asymmetric", mode
        s = o / sc
    return np.clip(s, 0.0, size_in - 1)


def resize_linear(x, ho, wo, mode="half_pixel", scales=None):
    """Linear Resize -> (ref, A). For half_pixel coordinates taken from the sizes (the only form the kernel runs) A is plain_ops_ref.bilinear's
    and the two references must agree; for the other forms A holds the interpolation's arithmetic only (8 u sum|w v|)."""
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    sy = linear_coords(h, ho, mode, None if scales is None else scales[0])
    sx = linear_coords(w, wo, mode, None if scales is None else scales[1])
    y0, x0 = np.minimum(np.floor(sy).astype(np.int64), h - 1), np.minimum(np.floor(sx).astype(np.int64), w - 1)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    LY, LX = (sy - y0)[:, None], (sx - x0)[None, :]
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    terms = [((1 - LY) * (1 - LX), x[:, :, Y0, X0]), ((1 - LY) * LX, x[:, :, Y0, X1]), (LY * (1 - LX), x[:, :, Y1, X0]), (LY * LX, x[:, :, Y1, X1])]
    ref = sum(wt * v for wt, v in terms)
    A = 8 * U * sum(np.abs(wt * v) for wt, v in terms)
    whole = scales is None or (h * float(np.float32(scales[0])) == ho and w * float(np.float32(scales[1])) == wo)   # then 1 / scale = in / out
    same_as_ratio = whole and (mode == "half_pixel" or (mode == "pytorch_half_pixel" and (ho > 1 or h == 1) and (wo > 1 or w == 1)))
    if same_as_ratio:
        ref2, A = R.bilinear(x, ho, wo)
        assert np.abs(ref2 - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    return ref, A


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
def concat(parts, axis=1):
    return np.concatenate([np.asarray(p, np.float64) for p in parts], axis=axis), None


def flatten(x, axis=1):
    x = np.asarray(x, np.float64)
    return x.reshape(int(np.prod(x.shape[:axis], dtype=np.int64)), -1), None


def transpose(x, perm=None):
    x = np.asarray(x, np.float64)
    return np.ascontiguousarray(np.transpose(x, list(perm) if perm else None)), None


def reshape(x, shape):
    """0 copies the input's dimension at that position, -1 is inferred."""
    x = np.asarray(x, np.float64)
    shape = [x.shape[k] if d == 0 else int(d) for k, d in enumerate(shape)]
    return x.reshape(shape), None


def squeeze(x, axes=None):
    x = np.asarray(x, np.float64)
    axes = [k for k, d in enumerate(x.shape) if d == 1] if axes is None else [a % x.ndim for a in axes]
    assert all(x.shape[a] == 1 for a in axes)
    return x.reshape([d for k, d in enumerate(x.shape) if k not in axes]), None


def unsqueeze(x, axes):
    x = np.asarray(x, np.float64)
    rank = x.ndim + len(axes)
    axes = sorted(a % rank for a in axes)
    shape, it = [], iter(x.shape)
    for k in range(rank):
        shape.append(1 if k in axes else next(it))
    return x.reshape(shape), None


def identity(x):
    return np.asarray(x, np.float64), None


def softmax(x, axis, opset):
    """opset < 13: the input is coerced to 2-D [prod(d[:axis]), prod(d[axis:])] and every row normalised; opset >= 13: along `axis` alone."""
    x = np.asarray(x, np.float64)
    axis %= x.ndim
    if opset < 13:
        rows = x.reshape(int(np.prod(x.shape[:axis], dtype=np.int64)), -1)
        ref, A = R.softmax(rows)
        return ref.reshape(x.shape), A.reshape(x.shape)
    moved = np.moveaxis(x, axis, -1)
    ref, A = R.softmax(moved.reshape(-1, moved.shape[-1]))
    return np.moveaxis(ref.reshape(moved.shape), -1, axis), np.moveaxis(A.reshape(moved.shape), -1, axis)
