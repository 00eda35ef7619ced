"""GPU: the in-register Winograd F(2x2,3x3) kernel for fp32 3x3 convolutions over 64 packed input channels
(facet_amd/csrc/kernels_wino64.hip), through engine.conv2d: exact on integers, against float64, its epilogues, against the direct
kernel, the routing in conv_forward, and the tile-count guard of the split-K route.

Tolerance 2e-4 * max(1, |ref|max): the bound tests/test_ops_gpu.py uses for the Winograd and direct kernels."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from standins import onnx_writer as W

pytestmark = pytest.mark.gpu

WINO64 = "wino64 3x3"          # profile record name of the new route
SHAPES = [(2, 64, 64, 16, 16),       # one exact block per image
          (1, 64, 64, 19, 23),       # partial tiles and partial blocks
          (3, 64, 64, 5, 70),        # tile groups crossing image ends
          (1, 64, 64, 1, 1),
          (2, 56, 56, 20, 20),       # Cin 56: zero rows of U
          (1, 64, 28, 9, 9),
          (1, 64, 40, 33, 17)]
EPI = (2, 64, 64, 19, 23)


@functools.lru_cache(maxsize=None)
def _case(n, cin, cout, h, w):
    """x, weights and the float64 convolution of one shape - computed once, shared, read-only"""
    rng = np.random.default_rng(1000 * cin + 10 * h + w + cout)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), padding=1).numpy()
    for a in (x, wt, ref):
        a.setflags(write=False)
    return x, wt, ref


def _close(got, ref):
    err, bound = float(np.abs(got - ref).max()), 2e-4 * max(1.0, float(np.abs(ref).max()))
    print(f"max |got - ref| = {err:.3e}, bound {bound:.3e}")
    assert got.shape == ref.shape and err <= bound, (err, bound)


def _names(engine, fn):
    engine.profile_enable(True)
    try:
        out = fn()
        recs = engine.profile_records()
    finally:
        engine.profile_enable(False)
    return out, [r["name"] for r in recs]


@pytest.mark.parametrize("cin,cout", [(64, 64), (56, 40)])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (19, 23)])
def test_exact_on_integers(engine, cin, cout, hw):
    """U holds quarters of integers and V integer sums: every product and sum is exact in fp32, the result equals F.conv2d's."""
    rng = np.random.default_rng(cin + hw[0])
    x = rng.integers(-3, 4, (3, cin, hw[0], hw[1])).astype(np.float32)
    w = rng.integers(-2, 3, (cout, cin, 3, 3)).astype(np.float32)
    got, names = _names(engine, lambda: engine.conv2d(x, w, stride=1, pad=1))
    assert any(n.startswith(WINO64) for n in names), names
    assert np.array_equal(got, F.conv2d(torch.from_numpy(x), torch.from_numpy(w), padding=1).numpy())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_float64(engine, shape):
    x, w, ref = _case(*shape)
    got, names = _names(engine, lambda: engine.conv2d(x, w, stride=1, pad=1))
    # in-family shapes record the new kernel's name; at Cout <= 32 half of its waves would multiply zero rows: the direct kernel keeps those
    assert any(n.startswith(WINO64) for n in names) == (shape[2] > 32), names
    _close(got, ref)


def _epilogue_vectors():
    rng = np.random.default_rng(77)
    return (rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.standard_normal(64).astype(np.float32),
            rng.standard_normal((EPI[0], 64, EPI[3], EPI[4])).astype(np.float32))


@pytest.mark.parametrize("epi", ["scale_shift_relu", "gelu", "sigmoid", "res_before_act", "res_after_act"])
def test_epilogues(engine, epi):
    """The ReLU forms run on the new kernel. conv_forward keeps GELU and sigmoid on the direct kernel (an erf / exp per output in an epilogue
    that nothing overlaps made the new kernel slower, profiles/wino64_perf.txt): those two cases pin that decision - no record of the new
    route - and check the direct kernel's result at the same bound. When those activations return to the new kernel, flip the assertions."""
    x, w, ref = _case(*EPI)
    sc, sh, r = _epilogue_vectors()
    t = torch.from_numpy(ref)
    aff = t * torch.from_numpy(sc).double().view(1, -1, 1, 1) + torch.from_numpy(sh).double().view(1, -1, 1, 1)
    rd = torch.from_numpy(r).double()
    if epi == "scale_shift_relu":
        (got, names), want = _names(engine, lambda: engine.conv2d(x, w, scale=sc, shift=sh, stride=1, pad=1, act="relu")), F.relu(aff)
        assert any(n.startswith(WINO64) for n in names), names
    elif epi == "gelu":
        (got, names), want = _names(engine, lambda: engine.conv2d(x, w, shift=sh, stride=1, pad=1, act="gelu")), F.gelu(t + torch.from_numpy(sh).double().view(1, -1, 1, 1))
        assert names and not any(n.startswith(WINO64) for n in names), names
    elif epi == "sigmoid":
        (got, names), want = _names(engine, lambda: engine.conv2d(x, w, scale=sc, stride=1, pad=1, act="sigmoid")), torch.sigmoid(t * torch.from_numpy(sc).double().view(1, -1, 1, 1))
        assert names and not any(n.startswith(WINO64) for n in names), names
    elif epi == "res_before_act":
        (got, names), want = _names(engine, lambda: engine.conv2d(x, w, scale=sc, shift=sh, res=r, res_after_act=False, stride=1, pad=1, act="relu")), F.relu(aff + rd)
        assert any(n.startswith(WINO64) for n in names), names
    else:
        (got, names), want = _names(engine, lambda: engine.conv2d(x, w, scale=sc, shift=sh, res=r, res_after_act=True, stride=1, pad=1, act="relu")), F.relu(aff) + rd
        assert any(n.startswith(WINO64) for n in names), names
    _close(got, want.numpy())


def test_prelu_epilogue_through_a_graph(engine):
    """engine.conv2d has no slopes argument: Conv + PRelu of a tiny ONNX graph (fused into the conv's epilogue by the graph runtime)."""
    g = W.GraphBuilder(64)
    y = g.prelu(g.conv("x", 64, 64, 3, 1), 64)
    data = g.build([("x", ["N", 64, EPI[3], EPI[4]])], [(y, ["N", 64, EPI[3], EPI[4]])])
    by_shape = {tuple(v.shape): v for v in g.init.values()}
    wt, b, sl = by_shape[(64, 64, 3, 3)], by_shape[(64,)], by_shape[(64, 1, 1)]
    x = _case(*EPI)[0]
    engine.graph_load(3, data)
    try:
        (got,), names = _names(engine, lambda: engine.graph_run(3, x))
    finally:
        engine.graph_unload(3)
    assert any(n.startswith(WINO64) for n in names), names
    pre = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    _close(got, torch.where(pre > 0, pre, pre * torch.from_numpy(sl).double()).numpy())


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=lambda s: "x".join(map(str, s)))
def test_against_the_direct_kernel(engine, shape):
    """The same call under a forced tile variant runs the direct kernel (whose forced variants need Cin % 16 == 0)."""
    x, w, _ = _case(*shape)
    sc, sh, _ = _epilogue_vectors()
    sc, sh = sc[:shape[2]], sh[:shape[2]]
    got = engine.conv2d(x, w, scale=sc, shift=sh, stride=1, pad=1, act="relu")
    try:
        engine.set_conv_variant(17)
        direct, names = _names(engine, lambda: engine.conv2d(x, w, scale=sc, shift=sh, stride=1, pad=1, act="relu"))
    finally:
        engine.set_conv_variant(0)
    assert not any(n.startswith(WINO64) for n in names), names          # a forced variant keeps the direct kernel
    _close(got, direct.astype(np.float64))


@pytest.mark.parametrize("name,cin,cout,kw", [("stride2", 64, 64, dict(stride=2, pad=1)), ("cin128", 128, 64, dict(stride=1, pad=1)),
                                              ("cout128", 64, 128, dict(stride=1, pad=1)), ("dilation2", 64, 64, dict(stride=1, pad=2, dil=2))])
def test_shapes_outside_the_family_keep_their_route(engine, name, cin, cout, kw):
    rng = np.random.default_rng(cin + cout)
    x = rng.standard_normal((2, cin, 20, 20)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    got, names = _names(engine, lambda: engine.conv2d(x, w, **kw))
    assert names and not any(n.startswith(WINO64) for n in names), names
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), stride=kw["stride"], padding=kw["pad"], dilation=kw.get("dil", 1)).numpy()
    _close(got, ref)


def test_split_k_guard_keeps_wide_outputs_on_the_plain_kernel(engine):
    """M = 64 rows, K = 2048, Cout = 4096: 64 output tiles already fill the chip, so the tile-count guard of the split-K route sends the
    layer to the plain kernel. Bound: the existing split-K test's 2e-5 * max(1, |ref|max) against float64."""
    rng = np.random.default_rng(2048)
    x = rng.standard_normal((64, 2048, 1, 1)).astype(np.float32)
    w = (rng.standard_normal((4096, 2048, 1, 1)) / np.sqrt(2048)).astype(np.float32)
    got, names = _names(engine, lambda: engine.conv2d(x, w))
    assert names and not any("splitk" in n for n in names), names
    ref = x[:, :, 0, 0].astype(np.float64) @ w[:, :, 0, 0].astype(np.float64).T
    err, bound = float(np.abs(got[:, :, 0, 0] - ref).max()), 2e-5 * max(1.0, float(np.abs(ref).max()))
    print(f"max |got - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
