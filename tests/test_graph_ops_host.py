"""CPU: the float64 references of the graph runtime's operators (tests/graph_ops_ref.py) and the cases built on them (tests/graph_ops_cases.py)
are held to a second opinion and to themselves, so that the GPU test (tests/test_graph_ops_gpu.py) measures the runtime and not the test.

  second opinion   every output of every case agrees with oracle.onnx_ref.run (torch, fp32, its own file reader) on the same bytes. The oracle
                   stands where the runtime stands on the GPU: each reference is computed from the oracle's own values of the inputs, so only
                   one operator's fp32 arithmetic separates the two. Exact operators must agree bit for bit; the others within 8 A +
                   2 ulp32(ref) + 16 u max(1, max|ref|): torch's own fp32 error obeys the same worst-case bound A; it evaluates BatchNormalization
                   unfolded, (x - mean) / sqrt(var + eps) gamma + beta, whose roundings are of the size of u |x s| (in A) and u (|mean s| + |beta|)
                   (constants of the size of the outputs: the last term). A semantic difference is hundreds of times larger (discrimination below).
                   The graphs that the runtime rejects because its coordinates would not be the specification's (OFF_SPEC) are the exclusions:
                   for each the oracle's result DIFFERS from the specification's, which is asserted, so the list cannot grow unnoticed.
  discrimination   for every attribute or layout alternative a case claims, the reference under the other setting differs from the right one by
                   more than 100 A somewhere.
  nearest rule     every nearest case uses (in, out) pairs for which the kernel's fp32 rule equals the exact one.
  round trip       every graph parses with the oracle's reader and with the engine's (fe_onnx_probe, no GPU needed)."""
import numpy as np
import pytest

import graph_ops_cases as C
import graph_ops_ref as G
from oracle import onnx_ref

CASES = {c.name: c for c in C.CASES}


@pytest.mark.parametrize("name", sorted(CASES))
def test_second_opinion(name):
    case = CASES[name]
    for n in (2, 3):
        x = case.input(n)
        outs = onnx_ref.run(case.data, x.astype(np.float32))
        assert len(outs) == len(case.checks)
        for chk, got, ref, A in C.evaluate(case, x, outs):
            what = f"{name} {chk.name} ({chk.key}) n={n}"
            assert got.shape == ref.shape, (what, got.shape, ref.shape)
            if A is None:
                assert np.array_equal(got.astype(np.float64), ref), what
            else:
                err = np.abs(got.astype(np.float64) - ref)
                tol = 8 * A + 2 * G.ulp32(ref) + 16 * G.U * max(1.0, float(np.abs(ref).max()))
                assert np.isfinite(ref).all() and (err <= tol).all(), (what, float((err / tol).max()))


def test_off_spec_graphs_are_the_only_exclusions():
    """Resize by scales that do not give whole pixels, and pytorch_half_pixel with an output length of 1: the size-ratio / half_pixel arithmetic
    (the oracle's, and the runtime's kernels') is not the specification's there. Asserted as a difference; the runtime rejects these graphs."""
    assert sorted(C.OFF_SPEC) == ["resize_linear_scales_1.3", "resize_linear_scales_1.5", "resize_nearest_scales_1.3",
                                  "resize_pytorch_half_pixel_len1", "resize_pytorch_half_pixel_len1_w"]
    for r in C.REJECTED:
        if r.spec is None:
            continue
        x = r.net.input(2)
        want = r.spec(x)
        (got,) = onnx_ref.run(r.data, x.astype(np.float32))
        assert got.shape == want.shape, r.name
        assert np.abs(got - want).max() > 1e-2, r.name


def test_suspect_arithmetic():
    """h = 5, scale 1.3: 6 rows; the specification's last source row is floor(5 / 1.3) = 3, the size ratio's floor(5 * 5 / 6) = 4."""
    assert G.resize_len(5, 1.3) == 6
    assert G.nearest_index(5, 6, 1.3)[-1] == 3 and G.nearest_index(5, 6)[-1] == 4
    assert G.linear_coords(5, 1, "pytorch_half_pixel")[0] == 0.0 and G.linear_coords(5, 1, "half_pixel")[0] == 2.0
    x = np.arange(2 * 3 * 5 * 3, dtype=np.float64).reshape(2, 3, 5, 3)
    assert not np.array_equal(G.softmax(x, 1, 11)[0], G.softmax(x, 1, 13)[0])        # 2-D coercion is not softmax along axis 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_discriminate(name):
    case = CASES[name]
    x = case.input(2)
    env = {"x": x}
    for chk, got, ref, A in C.evaluate(case, x):
        for alt in chk.alts:
            other, _ = chk.fn(env, alt=alt)
            assert other.size == ref.size, (name, chk.name, alt)
            gap = np.abs(other.reshape(-1) - ref.reshape(-1)) - 100 * (0.0 if A is None else A.reshape(-1))
            assert (gap > 0).any(), f"{name} {chk.name}: '{alt}' gives the same result"
        env[chk.name] = got.astype(np.float64)


def test_every_alternative_is_claimed_somewhere():
    """count_include_pad, align_corners, 2-D-coerced softmax, transB, permutations, flatten order and per-channel slopes each discriminate in some
    case. ceil_mode cannot be held against its alternative at an equal output shape: equal shapes mean equal window starts, hence equal
    results; it is the shape that differs, and some pool of every kind changes shape with it. The scales / size-ratio alternative belongs to the
    rejected graphs (test_off_spec_graphs_are_the_only_exclusions)."""
    claimed = {a for c in C.CASES for chk in c.checks for a in chk.alts}
    assert claimed >= {"cip", "align_corners", "per_axis", "transB", "identity", "nhwc", "slope0"}, claimed
    pools = [c for c in C.CASES if c.family == "pools"]
    assert pools and all(c.shape_alts for c in pools)
    # the 7 x 9 input has the ceil-mode window that starts in the right padding and is dropped (k 2, s 2, p 1: 5 windows would start at 7)
    assert len(G.pool_starts(7, 2, 2, 1, 1)) == 4 and len(G.pool_starts(9, 2, 2, 1, 1)) == 5 and len(G.pool_starts(6, 3, 2, 0, 1)) == 3


def test_pool_output_sizes_match_torch():
    import torch
    import torch.nn.functional as F
    for size in range(1, 14):
        for k in range(1, 6):
            for s in range(1, 4):
                for p in range(0, k // 2 + 1):
                    if size + 2 * p < k:
                        continue
                    for ceil in (False, True):
                        want = F.avg_pool2d(torch.zeros(1, 1, size, size), k, s, p, ceil_mode=ceil).shape[-1]
                        assert len(G.pool_starts(size, k, s, p, ceil)) == want, (size, k, s, p, ceil)


def test_fold_is_batchnorm():
    """The folded fp32 scale and shift against BatchNormalization's definition in float64: within the roundings of the fold."""
    rng = np.random.default_rng(3)
    c = 21
    bn = (rng.uniform(0.6, 1.2, c).astype(np.float32), rng.standard_normal(c).astype(np.float32), rng.standard_normal(c).astype(np.float32),
          rng.uniform(0.5, 1.5, c).astype(np.float32), 1e-5)
    x = rng.uniform(-2, 2, (2, c, 3, 4))
    sc, sh = G.fold(c, None, bn)
    ref, A = G.affine(x, sc, sh)
    spec = G.batchnorm_spec(x, bn)
    s = sc.reshape(1, c, 1, 1)
    assert (np.abs(ref - spec) <= 6 * G.U * (np.abs(x * s) + np.abs(bn[2].reshape(1, c, 1, 1) * s) + np.abs(bn[1].reshape(1, c, 1, 1)))).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_nearest_rule(name):
    """min(floor(f32(o) f32(in / out)), in - 1) = floor(o in / out) for every output index of every nearest case."""
    for size_in, size_out in CASES[name].nearest:
        ratio = np.float32(size_in) / np.float32(size_out)
        fp32 = np.minimum(np.floor(np.arange(size_out, dtype=np.float32) * ratio).astype(np.int64), size_in - 1)
        assert np.array_equal(fp32, G.nearest_index(size_in, size_out)), (name, size_in, size_out)


def test_nearest_cases_exist():
    assert sum(len(c.nearest) for c in C.CASES) >= 20


def test_graphs_round_trip():
    from facet_amd._lib import onnx_probe
    for g in list(C.CASES) + C.REJECTED:
        m = onnx_ref.parse(g.data)
        n_out = len(g.checks) if hasattr(g, "checks") else 1
        assert m["inputs"] == ["x"] and len(m["outputs"]) == n_out and m["opset"] == (g.opset if hasattr(g, "opset") else g.net.opset)
        info = onnx_probe(g.data)
        assert info["nodes"] == len(m["nodes"]) and info["initializers"] == len(m["init"]) and info["outputs"] == n_out
        assert info["input_dims"][1:] == [g.cin, g.hw[0], g.hw[1]]
