"""GPU: the face-clustering sweeps (fe_knn_core_distances, fe_mreach_mst, fe_cosine_best_match) and FaceClusterer on top of them,
against tests/golden/face_cluster_golden.npz (float64 brute force, scipy / Prim MST, sklearn.cluster.HDBSCAN 1.7.2 on float64
distances - parity with the `hdbscan` package and cuML is unpinned).

Tolerances are derived, not fitted. Every returned distance is recomputed exactly (fp64 from the fp32 rows), so only the CHOICE of a
neighbour or an edge rests on a swept value, whose error for unit rows is at most eps = 2 d 2^-24 (6.1e-5 at d = 512: the
worst-case bound of an fp32 dot product of length d, doubled by the factor 2 in front of it). Order statistics and sorted MST
weights are 1-Lipschitz in the sup norm of the weights: |core^2 - core64^2| <= 2 eps, sorted squared MST weights within 4 eps.
Largest values seen on one MI355X (profiles/face_cluster_perf.txt; the tests print them before they assert): |core^2 - core64^2|
3.1e-7 (the device normalises the rows itself, one fp32 rounding away from numpy's), sorted squared MST weights 6.7e-16 off the
golden and returned weights 2.7e-16 relative off the float64 recomputation when the rows are handed over normalised - every
neighbour and every edge was the float64 choice; Boruvka rounds 1 - 5 against bounds 2 - 12.
"""
import math

import numpy as np
import pytest

from facet_amd import EngineError
from facet_amd.face_cluster import FaceClusterer, normalise_rows
from test_face_cluster_host import (CASES, EPSILONS, MIN_SAMPLES, assert_same_partition, case_input, check_assign_persons, check_match_face,
                                    golden, planted)  # noqa: F401  (golden is a fixture)

pytestmark = pytest.mark.gpu
D = 512
EPS = 2 * D * 2.0 ** -24


def exact_dist(xn, u, v):
    a, b = xn[u].astype(np.float64), xn[v].astype(np.float64)
    return np.sqrt(((a - b) ** 2).sum(axis=-1))


def check_tree(n, eu, ev):
    """n - 1 edges that span n points without a cycle."""
    assert len(eu) == len(ev) == n - 1
    assert ((eu >= 0) & (ev < n) & (eu < ev)).all()
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(eu.tolist(), ev.tolist()):
        ra, rb = find(a), find(b)
        assert ra != rb, "the edges close a cycle"
        parent[ra] = rb
    assert len({find(i) for i in range(n)}) == 1


@pytest.mark.parametrize("name", list(CASES))
def test_core_distances(engine, golden, name):
    x, _ = case_input(golden, name)
    n = len(x)
    for ms in MIN_SAMPLES:
        if ms > n:
            continue
        core, idx = engine.core_distances(x, ms)
        want = golden[f"{name}_core_{ms}"]
        err = float(np.abs(core ** 2 - want ** 2).max())
        print(f"[core] case {name} k={ms}: max |core^2 - core64^2| = {err:.3e} (bound {2 * EPS:.3e})")
        assert err <= 2 * EPS
        # the value is the exact distance to the reported neighbour, from rows normalised the same way in fp32
        xn = normalise_rows(x)
        assert np.abs(core - exact_dist(xn, np.arange(n), idx)).max() <= 1e-6
        if ms == 1:
            assert np.array_equal(idx, np.arange(n)) or (core == 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_mst_is_valid_exact_and_matches_the_golden(engine, golden, name):
    x, _ = case_input(golden, name)
    n = len(x)
    xn = np.ascontiguousarray(normalise_rows(x))
    bound = math.ceil(math.log2(n)) + 1
    for ms in MIN_SAMPLES:
        if ms > n:
            continue
        # rows normalised on the host and taken as they are: the float64 recomputation below sees the very rows the device saw
        eu, ev, ew, core, rounds = engine.mreach_mst(xn, ms, normalise=False)
        check_tree(n, eu, ev)
        assert 1 <= rounds <= bound
        want_w = np.maximum(np.maximum(core[eu], core[ev]), exact_dist(xn, eu, ev))
        rel = float((np.abs(ew - want_w) / np.maximum(want_w, 1e-300)).max()) if (want_w > 0).all() else float(np.abs(ew - want_w).max())
        print(f"[mst] case {name} k={ms}: rounds {rounds} (bound {bound}), max relative |w - w64| = {rel:.3e}")
        assert np.all(np.abs(ew - want_w) <= 1e-12 * want_w)
        err = float(np.abs(np.sort(ew) ** 2 - np.sort(golden[f"{name}_mst_w_{ms}"]) ** 2).max())
        print(f"[mst] case {name} k={ms}: max |sorted w^2 - golden| = {err:.3e} (bound {4 * EPS:.3e})")
        assert err <= 4 * EPS
        # normalising on the device gives the same tree up to the rounding of the rows
        eu2, ev2, ew2, _, _ = engine.mreach_mst(x, ms, normalise=True)
        check_tree(n, eu2, ev2)
        assert np.abs(np.sort(ew2) ** 2 - np.sort(golden[f"{name}_mst_w_{ms}"]) ** 2).max() <= 4 * EPS


@pytest.mark.parametrize("name", list(CASES))
def test_cluster_embeddings_equal_the_golden_partition(engine, golden, name):
    x, _ = case_input(golden, name)
    for ms in MIN_SAMPLES:
        if ms > len(x):
            continue
        for ei, eps in enumerate(EPSILONS):
            fc = FaceClusterer(engine, min_faces=2, min_samples=ms, auto_merge_distance=eps * eps / 2)
            assert abs(fc.euclidean_epsilon - eps) < 1e-12
            got = fc.cluster_embeddings(x)
            assert_same_partition(got, golden[f"{name}_labels_{ms}_{ei}"], f"case {name} min_samples {ms} eps {eps:.3f}")


def test_host_and_device_input_and_two_runs_are_bit_identical(engine, golden):
    import torch
    x, _ = case_input(golden, "a")
    first = engine.mreach_mst(x, 2)
    again = engine.mreach_mst(x, 2)
    t = torch.from_numpy(x).cuda()
    dev = engine.mreach_mst((t.data_ptr(), x.shape[0], x.shape[1]), 2)
    for other in (again, dev):
        for a, b in zip(first[:4], other[:4]):
            assert a.tobytes() == b.tobytes()
        assert first[4] == other[4]
    c0 = engine.core_distances(x, 5)
    c1 = engine.core_distances((t.data_ptr(), x.shape[0], x.shape[1]), 5)
    assert c0[0].tobytes() == c1[0].tobytes() and c0[1].tobytes() == c1[1].tobytes()


def test_other_widths_and_k(engine):
    """d = 32 and 1024, k up to 32, n off the tile grid: against float64 brute force."""
    for d, n, k in ((32, 131, 32), (1024, 300, 7), (96, 129, 1)):
        x, _ = planted(77 + d, 12, 4, 12, n, d=d)
        x = x[:n]
        xn = normalise_rows(x)
        x64 = xn.astype(np.float64)
        d64 = np.sqrt(np.maximum(((x64[:, None, :] - x64[None, :, :]) ** 2).sum(axis=2), 0))
        want = np.sort(d64, axis=1)[:, k - 1]
        core, idx = engine.core_distances(x, k)
        eps = 2 * d * 2.0 ** -24
        assert np.abs(core ** 2 - want ** 2).max() <= 2 * eps
        eu, ev, ew, _, rounds = engine.mreach_mst(x, k)
        check_tree(n, eu, ev)
        assert rounds <= math.ceil(math.log2(n)) + 1


def test_bad_arguments_are_errors(engine):
    x = np.random.default_rng(0).standard_normal((40, 512)).astype(np.float32)
    for bad in (lambda: engine.core_distances(x[:1], 1), lambda: engine.core_distances(x[:, :48], 2), lambda: engine.core_distances(x[:, :16], 2),
                lambda: engine.core_distances(x, 0), lambda: engine.core_distances(x, 33), lambda: engine.core_distances(x[:4], 5),
                lambda: engine.mreach_mst(x[:1], 1), lambda: engine.mreach_mst(x, 41), lambda: engine.mreach_mst(np.zeros((4, 2048), np.float32), 2),
                lambda: engine.cosine_best_match(x[:, :40], x[:, :40]), lambda: engine.cosine_best_match(x[:0], x)):
        with pytest.raises(EngineError):
            bad()
    # the context stays usable
    assert engine.core_distances(x, 2)[0].shape == (40,)


def test_cosine_best_match(engine):
    rng = np.random.default_rng(5)
    c = rng.standard_normal((301, 512)).astype(np.float32) * 3
    q = np.concatenate([c[[7, 200, 300]] * 0.5 + 0.01 * rng.standard_normal((3, 512)).astype(np.float32),
                        rng.standard_normal((140, 512)).astype(np.float32)])
    c[250] = c[40]                                    # equal candidates: the first one wins
    q[5] = c[40] * 2
    sim, idx = engine.cosine_best_match(q, c)
    qn, cn = normalise_rows(q).astype(np.float64), normalise_rows(c).astype(np.float64)
    s = qn @ cn.T
    assert idx[:3].tolist() == [7, 200, 300] and idx[5] == 40
    assert np.abs(sim - s.max(axis=1)).max() <= 512 * 2.0 ** -24
    # wherever the best is clear of the runner-up by more than the fp32 dot-product error, the index is the float64 argmax
    top = np.sort(s, axis=1)
    clear = top[:, -1] - top[:, -2] > 2 * 512 * 2.0 ** -24
    clear[5] = False
    assert np.array_equal(idx[clear], np.argmax(s, axis=1)[clear])
    one, at = engine.cosine_best_match(q[:1], c[:1])
    assert at.tolist() == [0] and abs(float(one[0]) - s[0, 0]) <= 512 * 2.0 ** -24


def test_person_assignment_on_the_engine(engine, golden):
    check_assign_persons(engine, golden)
    check_match_face(engine, golden)


def test_twenty_thousand_planted_faces(engine):
    """No golden: 1000 identities of 20 faces. The labels recover the planted identities exactly, within the round bound."""
    n_id, per = 1000, 20
    rng = np.random.default_rng(31)
    centres = rng.standard_normal((n_id, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = np.repeat(centres, per, axis=0) + 0.035 * rng.standard_normal((n_id * per, D))
    x = (x * rng.uniform(5.0, 30.0, (len(x), 1))).astype(np.float32)
    ident = np.repeat(np.arange(n_id), per)
    order = rng.permutation(len(x))
    x, ident = np.ascontiguousarray(x[order]), ident[order]
    eu, ev, ew, core, rounds = engine.mreach_mst(x, 2)
    check_tree(len(x), eu, ev)
    assert rounds <= math.ceil(math.log2(len(x))) + 1
    got = FaceClusterer(engine).cluster_embeddings(x)
    assert_same_partition(got, ident, "20000 planted faces")
