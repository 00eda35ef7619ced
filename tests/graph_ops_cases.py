"""The graphs of the operator-by-operator tests of the ONNX graph runtime (host and GPU): each case is one operator, or the shortest chain that
reaches it, written with standins.onnx_writer.GraphBuilder, with the float64 reference of every declared output (tests/graph_ops_ref.py).

A `Net` writes nodes and records one `Check` per graph output, in output order. A check's reference is a function of the values that feed
it AS THE RUNTIME RETURNED THEM (the graph input, or earlier outputs), so every output is judged for its own operator's arithmetic and
nothing has to be propagated along a chain: `evaluate` walks the checks, hands each the outputs before it, and yields (check, got, ref, A).
Without outputs (host) the fp32-rounded references stand in. Nodes that the runtime runs as one launch (Conv | Gemm | MatMul ->
BatchNormalization -> activation -> Add -> Relu, BatchNormalization -> activation) are written by one method and checked as one unit: their
intermediates are not graph outputs, because a value that is an output, or has a second consumer, is not fused away.

Shapes are the smallest that reach the layouts: maps of 5x6, 7x9, 9x7 (6x6 for the dropped ceil-mode window), logical channels 3 (4 physical),
6 (8), 20 (20) and 21 (32), graph inputs of 3 and of 6 channels, batches of 2 and then 3 through one loaded graph."""
import numpy as np

import graph_ops_ref as G
import plain_ops_ref as R
from standins import onnx_writer as W

F32 = np.float32


class Check:
    def __init__(self, name, key, fn, alts):
        self.name, self.key, self.fn, self.alts = name, key, fn, tuple(alts)


class Net:
    def __init__(self, name, family, cin, hw, opset=11):
        self.name, self.family, self.cin, self.hw, self.opset = name, family, cin, tuple(hw), opset
        self.g = W.GraphBuilder(0, opset)
        self.rng = R.case_rng("graph_ops", name)
        self.checks, self.nearest, self.shape_alts = [], [], []
        self.env = {"x": self.input(1)}          # a batch of one, carried along while the graph is written: shapes for the weights

    # -- data ---------------------------------------------------------------------------------------------------------------------------
    def input(self, n):
        return R.case_rng("graph_ops_x", self.name, n).uniform(-1.5, 1.5, (n, self.cin) + self.hw).astype(F32).astype(np.float64)

    def rand(self, shape, scale=1.0):
        return (self.rng.standard_normal(shape) * scale).astype(F32)

    def away_from_zero(self, shape):
        return (self.rng.uniform(0.5, 2.0, shape) * self.rng.choice([-1.0, 1.0], shape)).astype(F32)

    def bn_params(self, c):
        r = self.rng
        return (r.uniform(0.6, 1.2, c).astype(F32), self.rand(c, 0.3), self.rand(c, 0.3), r.uniform(0.5, 1.5, c).astype(F32), 1e-5)

    def shape(self, v):
        return self.env[v].shape

    def _out(self, y, key, fn, alts=()):
        ref, _ = fn(self.env)
        self.env[y] = ref.astype(F32).astype(np.float64)
        self.checks.append(Check(y, key, fn, alts))
        return y

    def finish(self):
        self.data = self.g.build([("x", ["N", self.cin, self.hw[0], self.hw[1]])], [(c.name, ["N"]) for c in self.checks])
        return self

    # -- node writers -------------------------------------------------------------------------------------------------------------------
    def _bn_node(self, y, c):
        p = self.bn_params(c)
        names = [self.g.const(t, s) for t, s in zip(p[:4], ("g", "beta", "mu", "var"))]
        return self.g.op("BatchNormalization", [y] + names, epsilon=float(p[4]), momentum=0.9), p

    def _act_node(self, y, act, c, slope_shape="c11", alpha=None):
        """act: None, relu, sigmoid, leaky (alpha None: the attribute is left out, default 0.01), prelu -> (value, kind, slope)."""
        if act is None:
            return y, None, None
        if act == "relu":
            return self.g.op("Relu", [y]), "relu", None
        if act == "sigmoid":
            return self.g.op("Sigmoid", [y]), "sigmoid", None
        if act == "leaky":
            a = 0.01 if alpha is None else alpha
            out = self.g.op("LeakyRelu", [y]) if alpha is None else self.g.op("LeakyRelu", [y], alpha=float(alpha))
            return out, "prelu", np.asarray(F32(a), np.float64)
        assert act == "prelu", act
        shp = {"c": (c,), "c11": (c, 1, 1), "1c11": (1, c, 1, 1), "scalar": ()}[slope_shape]
        slope = self.rng.uniform(0.05, 0.6, shp).astype(F32)
        return self.g.op("PRelu", [y, self.g.const(slope, "slope")]), "prelu", slope.astype(np.float64)

    @staticmethod
    def _slope_alt(slope, alt):
        if alt == "slope0" and slope is not None:
            return np.full_like(slope, slope.ravel()[0])
        return slope

    def _tail(self, y, c, bn, act, slope_shape, alpha, add, add_first, relu_last):
        """-> (last value, bn parameters, kind, slope): the nodes behind a contraction that the planner takes into its group."""
        assert not (relu_last and (act is not None or add is None)), "a closing Relu is fused only behind an Add without an activation before it"
        bnp = None
        if bn:
            y, bnp = self._bn_node(y, c)
        y, kind, slope = self._act_node(y, act, c, slope_shape, alpha)
        if add is not None:
            y = self.g.op("Add", [add, y] if add_first else [y, add])
        if relu_last:
            y = self.g.op("Relu", [y])
        return y, bnp, kind, slope

    def conv(self, x, cout, k=3, s=1, p=0, d=1, group=1, bias=True, bn=False, act=None, slope_shape="c11", alpha=None, add=None, add_first=False,
             relu_last=False, key=None, gain=1.0, bias_shift=0.0):
        cin = self.shape(x)[1]
        kh, kw = G._pair(k)
        w = self.rand((cout, cin // group, kh, kw), gain * np.sqrt(2.0 / (cin // group * kh * kw)))
        b = (self.rand(cout, 0.3) + F32(bias_shift)).astype(F32) if bias else None
        ins = [x, self.g.const(w, "w")] + ([self.g.const(b, "b")] if bias else [])
        (sh, sw), (ph, pw), (dh, dw) = G._pair(s), G._pair(p), G._pair(d)
        y = self.g.op("Conv", ins, kernel_shape=[kh, kw], strides=[sh, sw], pads=[ph, pw, ph, pw], dilations=[dh, dw], group=group)
        y, bnp, kind, slope = self._tail(y, cout, bn, act, slope_shape, alpha, add, add_first, relu_last)
        sc, sf = G.fold(cout, b, bnp)

        def fn(env, alt=None):
            z, mag, K = G.conv(env[x], w, s, p, d, group)
            return G.epilogue(z, mag, K, sc, sf, kind, self._slope_alt(slope, alt), None if add is None else env[add], kind is not None, relu_last)
        alts = ["slope0"] if act == "prelu" and slope_shape != "scalar" else []
        return self._out(y, key or ("dwconv" if group > 1 else "conv"), fn, alts)

    def projection_block(self, x, cout):
        """Conv 1x1 -> BN (the shortcut) and Conv 3x3 -> BN, joined by Add -> Relu: neither chain's end is a graph output, so the first chain
        takes the Add and the Relu into its launch and reads the second chain's result as its residual. That result is not visible here:
        its own bound joins the group's (the Add and the Relu pass an error on unchanged)."""
        cin = self.shape(x)[1]
        ws = self.rand((cout, cin, 1, 1), np.sqrt(2.0 / cin))
        wm = self.rand((cout, cin, 3, 3), np.sqrt(2.0 / (9 * cin)))
        a = self.g.op("Conv", [x, self.g.const(ws, "w")], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], dilations=[1, 1], group=1)
        a, pa = self._bn_node(a, cout)
        b = self.g.op("Conv", [x, self.g.const(wm, "w")], kernel_shape=[3, 3], strides=[1, 1], pads=[1, 1, 1, 1], dilations=[1, 1], group=1)
        b, pb = self._bn_node(b, cout)
        y = self.g.op("Relu", [self.g.op("Add", [b, a])])
        (sa, fa), (sb, fb) = G.fold(cout, None, pa), G.fold(cout, None, pb)

        def fn(env, alt=None):
            zb, mb, Kb = G.conv(env[x], wm, 1, 1)
            rb, Ab = G.epilogue(zb, mb, Kb, sb, fb)
            za, ma, Ka = G.conv(env[x], ws)
            ref, A = G.epilogue(za, ma, Ka, sa, fa, res=rb, relu_last=True)
            return ref, A + Ab + G.ulp32(rb) / 2
        return self._out(y, "conv", fn)

    def gemm(self, x, cout, transB=1, bias=True, matmul=False, bn=False, act=None, add=None, add_first=False, relu_last=False, flat_of=None, key=None):
        cin = self.shape(x)[1]
        w = self.rand((cout, cin) if transB else (cin, cout), np.sqrt(1.0 / cin))
        b = self.rand(cout, 0.3) if bias else None
        ins = [x, self.g.const(w, "w")] + ([self.g.const(b, "b")] if bias else [])
        y = self.g.op("MatMul", ins) if matmul else self.g.op("Gemm", ins, alpha=1.0, beta=1.0, transB=int(transB))
        assert not (matmul and (transB or bias))
        y, bnp, kind, slope = self._tail(y, cout, bn, act, "c", None, add, add_first, relu_last)
        sc, sf = G.fold(cout, b, bnp)

        def fn(env, alt=None):
            xv, wv, tb = env[x], w, transB
            if alt == "transB":           # the same bytes read under the other setting
                wv, tb = w.reshape(w.shape[::-1]), 1 - transB
            if alt == "nhwc":             # the features of the flattened map in the order the runtime stores them
                xv = env[flat_of].transpose(0, 2, 3, 1).reshape(xv.shape)
            z, mag, K = G.gemm(xv, wv, tb)
            return G.epilogue(z, mag, K, sc, sf, kind, slope, None if add is None else env[add], kind is not None, relu_last)
        alts = ([] if matmul or cout == 1 else ["transB"]) + (["nhwc"] if flat_of else [])
        return self._out(y, key or ("matmul" if matmul else "gemm"), fn, alts)

    def bn(self, x, act=None, slope_shape="c11", alpha=None):
        c = self.shape(x)[1]
        y, p = self._bn_node(x, c)
        y, kind, slope = self._act_node(y, act, c, slope_shape, alpha)
        sc, sf = G.fold(c, None, p)

        def fn(env, alt=None):
            return G.affine(env[x], sc, sf, kind, self._slope_alt(slope, alt))
        return self._out(y, "bn", fn)

    def act(self, x, act, slope_shape="c11", alpha=None):
        y, kind, slope = self._act_node(x, act, self.shape(x)[1], slope_shape, alpha)

        def fn(env, alt=None):
            return G.activation(env[x], kind, self._slope_alt(slope, alt))
        return self._out(y, act, fn, ["slope0"] if act == "prelu" and slope_shape != "scalar" else [])

    def binary(self, a, b, op):
        return self._out(self.g.op(op, [a, b]), op.lower(), lambda env, alt=None: G.binary(env[a], env[b], op))

    def binary_const(self, x, op, kshape="scalar", const_left=False):
        c = self.shape(x)[1]
        k = self.away_from_zero({"scalar": (), "c11": (c, 1, 1), "1c11": (1, c, 1, 1), "one": (1,)}[kshape])
        kn = self.g.const(k, "k")
        y = self.g.op(op, [kn, x] if const_left else [x, kn])
        return self._out(y, op.lower() + "_const", lambda env, alt=None: G.binary_const(env[x], k, op, const_left))

    def maxpool(self, x, k, s, p, ceil=0):
        y = self.g.op("MaxPool", [x], kernel_shape=[k, k], strides=[s, s], pads=[p] * 4, ceil_mode=int(ceil))
        if G.maxpool(self.env[x], k, s, p, 1 - ceil)[0].shape != G.maxpool(self.env[x], k, s, p, ceil)[0].shape:
            self.shape_alts.append(y)
        return self._out(y, "maxpool", lambda env, alt=None: G.maxpool(env[x], k, s, p, ceil))

    def avgpool(self, x, k, s, p, ceil=0, cip=0):
        y = self.g.op("AveragePool", [x], kernel_shape=[k, k], strides=[s, s], pads=[p] * 4, ceil_mode=int(ceil), count_include_pad=int(cip))
        if G.avgpool(self.env[x], k, s, p, 1 - ceil)[0].shape != G.avgpool(self.env[x], k, s, p, ceil)[0].shape:
            self.shape_alts.append(y)
        differs = not np.array_equal(G.avgpool(self.env[x], k, s, p, ceil, 0)[0], G.avgpool(self.env[x], k, s, p, ceil, 1)[0])
        return self._out(y, "avgpool", lambda env, alt=None: G.avgpool(env[x], k, s, p, ceil, 1 - cip if alt == "cip" else cip), ["cip"] if differs else [])

    def gap(self, x):
        return self._out(self.g.op("GlobalAveragePool", [x]), "gap", lambda env, alt=None: G.global_avgpool(env[x]))

    def resize(self, x, mode, out_hw=None, scales=None, ctm=None, form="resize", nearest_mode="floor", write_only=False):
        """form: "resize" (opset 11+: X, roi, scales, sizes), "resize2" (opset 10: X, scales), "upsample" (X, scales). out_hw: by sizes."""
        _, c, h, w = self.shape(x)
        if scales is not None:
            ho, wo = G.resize_len(h, scales[0]), G.resize_len(w, scales[1])
            sc = self.g.const(np.asarray([1, 1, scales[0], scales[1]], F32), "scales")
        else:
            ho, wo = out_hw
        attrs = {"mode": mode}
        if form == "resize":
            attrs["coordinate_transformation_mode"] = ctm or ("asymmetric" if mode == "nearest" else "half_pixel")
            if mode == "nearest" and nearest_mode:
                attrs["nearest_mode"] = nearest_mode
            roi = self.g.const(np.zeros(0, F32), "roi")
            ins = [x, roi, sc] if scales is not None else [x, roi, self.g.const(np.zeros(0, F32), "scales"), self.g.const(np.asarray([2, c, ho, wo], np.int64), "sizes")]
            y = self.g.op("Resize", ins, **attrs)
        else:
            assert scales is not None and mode == "nearest"
            y = self.g.op("Resize" if form == "resize2" else "Upsample", [x, sc], **attrs)
        if write_only:
            return y
        if mode == "nearest":
            self.nearest += [(h, ho), (w, wo)]
            return self._out(y, "nearest", lambda env, alt=None: G.resize_nearest(env[x], ho, wo, None if alt == "ratio" else scales))
        mode_ = attrs["coordinate_transformation_mode"]
        return self._out(y, "linear", lambda env, alt=None: G.resize_linear(env[x], ho, wo, "align_corners" if alt == "align_corners" else mode_,
                                                                           None if alt == "ratio" else scales), ["align_corners"] if (ho, wo) != (h, w) else [])

    def concat(self, parts):
        return self._out(self.g.op("Concat", list(parts), axis=1), "concat", lambda env, alt=None: G.concat([env[p] for p in parts], 1))

    def flatten(self, x):
        def fn(env, alt=None):
            v = env[x]
            return G.flatten(v.transpose(0, 2, 3, 1) if alt == "nhwc" else v)
        four = len(self.shape(x)) == 4 and self.shape(x)[1] > 1 and self.shape(x)[2] * self.shape(x)[3] > 1
        return self._out(self.g.op("Flatten", [x], axis=1), "flatten", fn, ["nhwc"] if four else [])

    def transpose(self, x, perm):
        y = self.g.op("Transpose", [x], perm=list(perm)) if perm else self.g.op("Transpose", [x])

        def fn(env, alt=None):
            return (G.identity(env[x]) if alt == "identity" else G.transpose(env[x], perm))
        return self._out(y, "transpose", fn, ["identity"])

    def reshape(self, x, shape, as_attr=False):
        y = self.g.op("Reshape", [x], shape=list(shape)) if as_attr else self.g.op("Reshape", [x, self.g.const(np.asarray(shape, np.int64), "shape")])
        return self._out(y, "reshape", lambda env, alt=None: G.reshape(env[x], shape))

    def squeeze(self, x, axes, as_input=False):
        y = self.g.op("Squeeze", [x, self.g.const(np.asarray(axes, np.int64), "axes")]) if as_input else self.g.op("Squeeze", [x], axes=list(axes))
        return self._out(y, "squeeze", lambda env, alt=None: G.squeeze(env[x], axes))

    def unsqueeze(self, x, axes, as_input=False):
        y = self.g.op("Unsqueeze", [x, self.g.const(np.asarray(axes, np.int64), "axes")]) if as_input else self.g.op("Unsqueeze", [x], axes=list(axes))
        return self._out(y, "unsqueeze", lambda env, alt=None: G.unsqueeze(env[x], axes))

    def softmax(self, x, axis=None):
        y = self.g.op("Softmax", [x]) if axis is None else self.g.op("Softmax", [x], axis=int(axis))
        ax = (-1 if self.opset >= 13 else 1) if axis is None else axis
        coerced = self.opset < 13 and len(self.shape(x)) > 2 and ax % len(self.shape(x)) != len(self.shape(x)) - 1

        def fn(env, alt=None):
            return G.softmax(env[x], ax, 13 if alt == "per_axis" else self.opset)
        return self._out(y, "softmax", fn, ["per_axis"] if coerced else [])

    def identity(self, x, op="Identity"):
        return self._out(self.g.op(op, [x]), op.lower(), lambda env, alt=None: G.identity(env[x]))


def evaluate(case, x, outs=None):
    """Yields (check, got, ref, A) per graph output; outs: the runtime's outputs for x, or None (the fp32-rounded references stand in)."""
    env = {"x": np.asarray(x, np.float64)}
    for i, c in enumerate(case.checks):
        ref, A = c.fn(env)
        got = ref.astype(F32) if outs is None else np.asarray(outs[i])
        yield c, got, ref, A
        env[c.name] = got.astype(np.float64) if got.shape == ref.shape else ref


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
SLOPES = ("c", "c11", "1c11", "scalar")
OPS = ("Add", "Sub", "Mul", "Div")


def _activations():
    for cin, hw in ((3, (5, 6)), (6, (7, 9))):
        n = Net(f"act_map_{cin}", "activations", cin, hw)
        maps = ["x", n.conv("x", 20, 1), n.conv("x", 21, 1)]
        for m in maps:
            for a in ("relu", "sigmoid"):
                n.act(m, a)
            n.act(m, "leaky")
            n.act(m, "leaky", alpha=0.2)
            for s in SLOPES:
                n.act(m, "prelu", s)
            n.bn(m)
            n.bn(m, "relu")
            n.bn(m, "prelu", "c")
            n.bn(m, "leaky", alpha=0.3)
            n.bn(m, "sigmoid")
        yield n.finish()
    n = Net("act_plain", "activations", 3, (7, 9))         # 3 x 7 x 9 = 189 per image: 378 and 567 elements, neither a multiple of 4
    assert (2 * 189) % 4 and (3 * 189) % 4
    p = n.reshape("x", [0, -1])
    n.act(p, "relu")
    n.act(p, "sigmoid")
    q = n.reshape("x", [0, 27, 7])
    n.act(q, "sigmoid")
    yield n.finish()


def _binary():
    for cin, hw in ((3, (5, 6)), (6, (9, 7))):
        n = Net(f"binary_maps_{cin}", "binary", cin, hw)
        for c in (6, 21):
            a, b = n.conv("x", c, 1), n.conv("x", c, 3, p=1)
            for op in OPS:
                n.binary(a, b, op)
            n.binary(b, a, "Sub")
            n.binary(b, a, "Div")
        for m in ("x", a):
            for op in OPS:
                n.binary_const(m, op, "scalar")
                n.binary_const(m, op, "c11")
            n.binary_const(m, "Mul", "1c11")
            n.binary_const(m, "Div", "one")
            for op in ("Add", "Mul"):
                n.binary_const(m, op, "c11", const_left=True)
                n.binary_const(m, op, "scalar", const_left=True)
        yield n.finish()
    n = Net("binary_plain", "binary", 3, (7, 9))
    p, q = n.reshape("x", [0, -1]), n.reshape(n.act("x", "sigmoid"), [0, -1])
    for op in OPS:
        n.binary(p, q, op)
        n.binary_const(p, op, "scalar")
    n.binary_const(p, "Add", "scalar", const_left=True)
    n.binary_const(p, "Mul", "one", const_left=True)
    yield n.finish()


def _fusion():
    for cin, hw, c in ((3, (5, 6), 6), (6, (7, 9), 21), (3, (9, 7), 20)):
        n = Net(f"fusion_conv_{c}", "fusion", cin, hw)
        base = n.conv("x", c, 3, p=1)                                   # the residual operand of every Add below
        n.conv("x", c, 3, p=1, bn=True)
        n.conv("x", c, 3, p=1, bn=True, act="relu")
        n.conv("x", c, 3, p=1, bn=True, act="prelu", slope_shape="c")
        n.conv("x", c, 1, bias=False, bn=True, act="leaky")
        n.conv("x", c, 3, p=1, act="sigmoid")
        n.conv("x", c, 3, p=1, act="relu", add=base)                    # Conv -> act -> Add: the residual joins after the activation
        n.conv("x", c, 3, p=1, act="prelu", add=base, add_first=True)
        n.conv("x", c, 3, p=1, bn=True, add=base, relu_last=True)       # Conv -> BN -> Add -> Relu
        n.conv("x", c, 3, p=1, bn=True, add=base, add_first=True, relu_last=True)
        n.conv("x", c, 3, p=1, add=base)
        # a projection-shortcut block: both inputs of the Add are Conv -> BN chains; the first stays a value of its own (it is an output)
        short = n.conv("x", c, 1, bias=False, bn=True)
        n.conv(base, c, 3, p=1, bias=False, bn=True, add=short, relu_last=True)
        n.projection_block("x", c)
        n.projection_block(base, c)
        # an intermediate that is also a graph output is not fused away: Conv, BN, Relu, Add, Relu one by one
        t = n.conv("x", c, 3, p=1)
        t = n.bn(t)
        t = n.act(t, "relu")
        t = n.binary(t, base, "Add")
        n.act(t, "relu")
        # depthwise groups
        n.conv(base, c, 3, p=1, group=c, bias=False, bn=True, act="prelu")
        n.conv(base, c, 3, p=1, group=c, add=base, relu_last=True)
        n.conv(base, c, 3, p=1, group=c, add=base, add_first=True)
        yield n.finish()
    for cin, hw in ((3, (5, 6)), (6, (5, 6))):
        n = Net(f"fusion_gemm_{cin}", "fusion", cin, hw)
        f = n.flatten("x")
        for cout in (6, 21):
            base = n.gemm(f, cout, flat_of="x")
            n.gemm(f, cout, flat_of="x", add=base)                                   # Gemm -> Add
            n.gemm(f, cout, flat_of="x", act="relu", add=base, add_first=True)       # Gemm -> act -> Add
            n.gemm(f, cout, flat_of="x", act="sigmoid", add=base)
            n.gemm(f, cout, flat_of="x", add=base, relu_last=True)
            n.gemm(f, cout, flat_of="x", bn=True, act="prelu")
            n.gemm(f, cout, 0, flat_of="x", act="sigmoid")
            n.gemm(f, cout, 0, bias=False, flat_of="x", bn=True)
        yield n.finish()


def _depthwise():
    for cin, hw in ((6, (7, 9)), (3, (9, 7))):
        n = Net(f"depthwise_{cin}", "depthwise", cin, hw)
        for m in ("x", n.conv("x", 20, 1), n.conv("x", 21, 1)):
            c = n.shape(m)[1]
            for k, s, p in ((3, 1, 1), (3, 2, 1), (3, 1, 0), (3, 2, 0), (5, 1, 2), (5, 2, 2), (5, 1, 0), (5, 2, 1), (3, (1, 2), (1, 0))):
                n.conv(m, c, k, s, p, group=c, bias=True)
            n.conv(m, c, 3, 2, 1, group=c, bias=False, bn=True)
            n.conv(m, c, 5, 1, 2, group=c, bias=True, bn=True, act="relu")
            n.conv(m, c, 3, 1, 1, group=c, bias=False)
        yield n.finish()
    # dense convolutions: strides, pads, dilations, with and without a bias, non-square kernels and steps
    for cin, hw in ((3, (7, 9)), (6, (9, 7))):
        n = Net(f"conv_dense_{cin}", "depthwise", cin, hw)
        for m in ("x", n.conv("x", 20, 1), n.conv("x", 21, 1)):
            for cout in (6, 21):
                n.conv(m, cout, 3, 1, 1)
                n.conv(m, cout, 3, 2, 1, bias=False)
                n.conv(m, cout, 3, 1, 2, d=2)
                n.conv(m, cout, (1, 3), (2, 1), (0, 1))
                n.conv(m, cout, 3, 1, (2, 1), d=(2, 1))
                n.conv(m, cout, 5, 2, 2)
                n.conv(m, cout, 1, 2, 0)
        yield n.finish()


def _pools():
    for cin, hw in ((3, (7, 9)), (6, (6, 6))):
        n = Net(f"pools_{cin}", "pools", cin, hw)
        for m in ("x", n.conv("x", 21, 1)):
            for k in (2, 3):
                for s in (1, 2):
                    for p in (0, 1):
                        for ceil in (0, 1):
                            n.maxpool(m, k, s, p, ceil)
                            for cip in (0, 1):
                                n.avgpool(m, k, s, p, ceil, cip)
            n.gap(m)
        yield n.finish()


def _resize():
    n = Net("resize_nearest", "resize", 3, (5, 6))
    for m in ("x", n.conv("x", 21, 1)):
        n.resize(m, "nearest", (10, 12))
        n.resize(m, "nearest", (15, 18))
        n.resize(m, "nearest", (7, 8))
        n.resize(m, "nearest", scales=(2.0, 2.0))
        n.resize(m, "nearest", scales=(3.0, 2.0))
    yield n.finish()
    n = Net("resize_linear_up", "resize", 6, (5, 6))
    for m in ("x", n.conv("x", 21, 1)):
        for ctm in ("half_pixel", "pytorch_half_pixel"):
            n.resize(m, "linear", (10, 12), ctm=ctm)
            n.resize(m, "linear", (7, 11), ctm=ctm)
            n.resize(m, "linear", scales=(2.0, 1.5), ctm=ctm)          # 5 x 2 and 6 x 1.5 are whole numbers
        n.resize(m, "linear", (1, 1), ctm="half_pixel")                # an output of length 1: the centre of the input
        n.resize(m, "linear", (1, 12), ctm="half_pixel")
    yield n.finish()
    n = Net("resize_linear_down", "resize", 3, (9, 7))
    for ctm in ("half_pixel", "pytorch_half_pixel"):
        n.resize("x", "linear", (4, 3), ctm=ctm)
        n.resize("x", "linear", (9, 7), ctm=ctm)
    yield n.finish()
    n = Net("resize_opset10", "resize", 3, (5, 6), opset=10)
    n.resize("x", "nearest", scales=(2.0, 2.0), form="resize2")
    n.resize(n.conv("x", 6, 1), "nearest", scales=(2.0, 3.0), form="resize2")
    yield n.finish()
    n = Net("upsample_opset9", "resize", 6, (5, 6), opset=9)
    n.resize("x", "nearest", scales=(2.0, 2.0), form="upsample")
    n.resize(n.conv("x", 21, 1), "nearest", scales=(3.0, 2.0), form="upsample")
    yield n.finish()


def _layout():
    n = Net("layout_concat", "layout", 3, (5, 6))
    a, b = n.conv("x", 6, 1), n.conv("x", 21, 1)
    n.concat(["x", a, b])                         # 3 + 6 + 21 = 30 -> 32 physical
    n.concat([b, a])
    n.concat([a, "x", a])                          # 15 -> 16 physical
    n.concat([n.conv("x", 20, 1), a, a])           # 32: nothing padded in the result
    n.identity(a)
    n.identity(b, "Dropout")
    yield n.finish()
    n = Net("layout_transpose", "layout", 3, (7, 9))
    dense = n.conv("x", 20, 1)
    for m in ("x", dense, n.conv("x", 21, 1)):
        t = n.transpose(m, (0, 2, 3, 1))           # from a padded map: gathered; from the 20-channel one: the map's own memory
        n.transpose(t, (0, 3, 1, 2))
        n.transpose(m, (0, 1, 3, 2))
        n.transpose(m, ())                         # empty perm: all axes reversed
        n.transpose(m, (3, 1, 0, 2))
    r3 = n.reshape("x", [0, 3, -1])
    n.transpose(r3, (0, 2, 1))
    n.transpose(r3, (2, 0, 1))
    n.transpose(r3, (1, 2, 0))
    r5 = n.reshape("x", [0, 3, 7, 3, 3])
    n.transpose(r5, (0, 3, 1, 4, 2))
    n.transpose(r5, (4, 3, 2, 1, 0))
    r6 = n.reshape(dense, [-1, 2, 10, 7, 3, 3])
    n.transpose(r6, (0, 5, 2, 3, 1, 4))
    yield n.finish()
    n = Net("layout_reshape", "layout", 6, (5, 6))
    n.reshape("x", [0, -1, 6])
    n.reshape("x", [0, 0, -1])
    n.reshape("x", [-1, 6, 30])
    n.reshape("x", [0, 6, 5, 6], as_attr=True)
    u = n.unsqueeze("x", [-1])
    n.squeeze(u, [-1])
    u2 = n.unsqueeze("x", [1, -1])
    n.squeeze(u2, [-1, 1])
    g = n.gap(n.conv("x", 21, 1))
    n.squeeze(g, [-1, -2])
    n.squeeze(g, [2])
    yield n.finish()
    n = Net("layout_axes_as_input", "layout", 3, (5, 6), opset=13)
    u = n.unsqueeze("x", [-1], as_input=True)
    n.squeeze(u, [-1], as_input=True)
    u2 = n.unsqueeze("x", [0, -2], as_input=True)
    n.squeeze(u2, [0], as_input=True)
    g = n.gap(n.conv("x", 6, 1))
    n.squeeze(g, [-1, -2], as_input=True)
    yield n.finish()
    for cin in (6, 3):
        n = Net(f"layout_flatten_gemm_{cin}", "layout", cin, (5, 6))
        for m in ("x", n.conv("x", 6, 1), n.conv("x", 21, 3, p=1)):
            f = n.flatten(m)                                   # h w > 1 with padded channels: the weight columns are permuted to NHWC
            for cout in (7, 21):
                n.gemm(f, cout, 1, flat_of=m)
                n.gemm(f, cout, 0, flat_of=m)
                n.gemm(f, cout, 0, bias=False, flat_of=m)
            f1 = n.flatten(n.gap(m))                           # Flatten of a 1 x 1 map
            n.gemm(f1, 5, 1)
            n.gemm(f1, 5, 0)
        p = n.reshape("x", [0, -1])                            # a PLAIN matrix
        n.gemm(p, 7, matmul=True, bias=False, transB=0)
        n.gemm(p, 21, 1)
        yield n.finish()


def _softmax():
    n = Net("softmax_opset11", "softmax", 3, (5, 6))
    f = n.flatten("x")
    n.softmax(f)                                   # rank 2, rows of 90
    for d in (1, 7, 200):
        n.softmax(n.gemm(f, d, flat_of="x"), axis=1)
    r3 = n.reshape("x", [0, 9, -1])
    n.softmax(r3, axis=1)                          # rank 3, axis 1 below opset 13: rows of 9 x 10 after the coercion to 2-D
    n.softmax(r3, axis=2)
    n.softmax("x", axis=1)                         # rank 4: rows of 3 x 5 x 6
    n.softmax(n.transpose("x", (0, 2, 3, 1)), axis=-1)
    yield n.finish()
    n = Net("softmax_opset13", "softmax", 6, (5, 6), opset=13)
    f = n.flatten("x")
    n.softmax(f)
    n.softmax(f, axis=1)
    r3 = n.reshape("x", [0, 9, -1])
    n.softmax(r3, axis=-1)                         # rank 3: rows of 20 along the last axis alone
    n.softmax(r3)
    n.softmax(n.reshape("x", [0, -1, 1]), axis=2)  # rows of one element
    n.softmax(n.transpose("x", (0, 2, 3, 1)), axis=3)
    yield n.finish()


def _hygiene():
    """Maps whose padding lanes are (or were, before binary_kernel wrote zeros there) not zero, fed to every class of consumer."""
    for cin, hw, c in ((3, (5, 6), 6), (6, (7, 9), 21)):
        for how in ("sigmoid", "div", "div_sigmoid"):
            n = Net(f"hygiene_{how}_{c}", "hygiene", cin, hw)
            # the divisors stay away from zero (small weights, a bias of 4), so that the quotients are of the size of the other maps; their
            # padding lanes hold 0 all the same
            if how == "sigmoid":
                m = n.conv("x", c, 3, p=1, act="sigmoid")                       # 0.5 in the padding lanes
            elif how == "div":
                m = n.binary(n.conv("x", c, 1), n.conv("x", c, 3, p=1, gain=0.2, bias_shift=4.0), "Div")   # 0 / 0 in the padding lanes
            else:
                m = n.binary(n.conv("x", c, 1, act="sigmoid"), n.conv("x", c, 3, p=1, gain=0.2, bias_shift=4.0), "Div")   # 0.5 / 0
            other = n.conv("x", c, 1)
            n.conv(m, 7, 1)
            n.conv(m, 21, 3, p=1)
            n.conv(m, c, 3, p=1, group=c)
            n.gemm(n.flatten(n.gap(m)), 5)
            n.gemm(n.flatten(m), 7, flat_of=m)
            n.concat([m, "x"])
            n.concat(["x", m, other])
            n.binary(m, other, "Add")
            n.binary(other, m, "Mul")
            n.binary(n.binary(m, other, "Sub"), m, "Div")
            n.maxpool(m, 3, 2, 1)
            n.avgpool(m, 3, 2, 1, 1, 1)
            n.gap(m)
            n.resize(m, "nearest", (2 * hw[0], 2 * hw[1]))
            n.resize(m, "linear", (hw[0] + 2, hw[1] + 5))
            n.transpose(m, (0, 2, 3, 1))
            n.softmax(m, axis=1)
            n.act(m, "sigmoid")
            n.bn(m)
            yield n.finish()


def build_cases():
    out = []
    for fam in (_activations, _binary, _fusion, _depthwise, _pools, _resize, _layout, _softmax, _hygiene):
        out += list(fam())
    assert len({c.name for c in out}) == len(out)
    return out


CASES = build_cases()
FAMILIES = sorted({c.family for c in CASES})


# ---- graphs the runtime must reject at run time, with a clear message, leaving the context usable ------------------------------------------
class Rejected:
    def __init__(self, name, net, match, spec=None):
        self.name, self.data, self.cin, self.hw, self.match, self.spec = name, None, net.cin, net.hw, match, spec
        self.net = net


def _reject(name, cin, hw, match, write, opset=11, spec=None):
    """write(net) -> the value to declare as the graph's only output. spec(x) -> the specification's result, where the point of the case is
    that a guess would differ from it."""
    n = Net("rejected_" + name, "rejected", cin, hw, opset)
    y = write(n)
    n.data = n.g.build([("x", ["N", cin, hw[0], hw[1]])], [(y, ["N"])])
    r = Rejected(name, n, match, spec)
    r.data = n.data
    return r


def build_rejected():
    out = []
    k6 = np.asarray([[[0.5]], [[1.0]], [[2.0]], [[-1.0]], [[4.0]], [[0.25]]], F32)
    out.append(_reject("sub_const_left", 6, (5, 6), "Sub.*constant on the left", lambda n: n.g.op("Sub", [n.g.const(k6), "x"])))
    out.append(_reject("div_const_left", 6, (5, 6), "Div.*constant on the left", lambda n: n.g.op("Div", [n.g.const(np.asarray(2.0, F32)), "x"])))
    out.append(_reject("div_const_left_plain", 3, (5, 6), "Div.*constant on the left",
                       lambda n: n.g.op("Div", [n.g.const(np.asarray(2.0, F32)), n.reshape("x", [0, -1])])))

    def dilated_dw(n):
        w = n.rand((6, 1, 3, 3))
        return n.g.op("Conv", ["x", n.g.const(w)], kernel_shape=[3, 3], strides=[1, 1], pads=[2, 2, 2, 2], dilations=[2, 2], group=6)
    out.append(_reject("dilated_depthwise", 6, (7, 9), "dilated depthwise", dilated_dw))
    for mode in ("nearest", "linear"):
        for s in (1.3, 1.5):
            nm = "graph: Resize .*scales"
            # (nearest at 1.5: floor(o / 1.5) = floor(o 5 / 7) for every o < 7, no difference to show; rejected all the same)
            spec = None if (mode, s) == ("nearest", 1.5) else (lambda x, s=s: G.resize_nearest(x, G.resize_len(5, s), G.resize_len(6, s), (s, s))[0]) if mode == "nearest" else \
                   (lambda x, s=s: G.resize_linear(x, G.resize_len(5, s), G.resize_len(6, s), "half_pixel", (s, s))[0])
            out.append(_reject(f"resize_{mode}_scales_{s}", 3, (5, 6), nm, lambda n, mode=mode, s=s: n.resize("x", mode, scales=(s, s), write_only=True), spec=spec))
    out.append(_reject("resize_pytorch_half_pixel_len1", 3, (5, 6), "graph: Resize .*pytorch_half_pixel",
                       lambda n: n.resize("x", "linear", (1, 1), ctm="pytorch_half_pixel", write_only=True),
                       spec=lambda x: G.resize_linear(x, 1, 1, "pytorch_half_pixel")[0]))
    out.append(_reject("resize_pytorch_half_pixel_len1_w", 6, (5, 6), "graph: Resize .*pytorch_half_pixel",
                       lambda n: n.resize("x", "linear", (10, 1), ctm="pytorch_half_pixel", write_only=True),
                       spec=lambda x: G.resize_linear(x, 10, 1, "pytorch_half_pixel")[0]))
    out.append(_reject("resize_nearest_round_prefer_floor", 3, (5, 6), "graph: Resize .*nearest",
                       lambda n: n.resize("x", "nearest", (10, 12), nearest_mode="round_prefer_floor", write_only=True)))
    out.append(_reject("resize_nearest_default_mode", 3, (5, 6), "graph: Resize .*nearest",
                       lambda n: n.resize("x", "nearest", (10, 12), nearest_mode=None, write_only=True)))
    out.append(_reject("resize_nearest_half_pixel", 3, (5, 6), "graph: Resize .*nearest",
                       lambda n: n.resize("x", "nearest", (10, 12), ctm="half_pixel", write_only=True)))
    out.append(_reject("resize_align_corners", 3, (5, 6), "graph: Resize .*align_corners",
                       lambda n: n.resize("x", "linear", (10, 12), ctm="align_corners", write_only=True)))
    out.append(_reject("resize_cubic", 3, (5, 6), "graph: Resize .*cubic", lambda n: n.resize("x", "cubic", (10, 12), write_only=True)))
    return out


REJECTED = build_rejected()
# of these, the ones whose result under the runtime's (and the torch oracle's) size-ratio / half_pixel arithmetic differs from the
# specification's: the reason they are rejected and not run
OFF_SPEC = [r.name for r in REJECTED if r.spec is not None]
