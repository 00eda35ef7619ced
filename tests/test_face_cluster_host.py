"""CPU: the host side of face clustering (facet_amd/face_cluster.py).

* `hdbscan_labels` on the golden minimum spanning trees gives the partitions sklearn.cluster.HDBSCAN 1.7.2 gave on the float64
  distance matrices (tests/golden/make_face_cluster_golden.py), for min_samples 1 / 2 / 5 and epsilon 0 / sqrt(0.3); trees with
  tied weights are fed with the equal edges in two orders. Parity with the `hdbscan` package and cuML is unpinned (not installed).
* parameter derivations of `FaceClusterer` (reference faces/clusterer.py:70-72, :163-165).
* `assign_persons` / `match_face_to_person` against what the reference's own `_update_database` / `match_face_to_person` wrote on
  a scratch database. The many-to-many comparison is the engine's (`cosine_best_match`, a GPU sweep); here a numpy stand-in with
  the same contract takes its place - the package itself has no host path for it.
"""
import hashlib
import os

import numpy as np
import pytest

from facet_amd.face_cluster import FaceClusterer, hdbscan_labels, normalise_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "face_cluster_golden.npz")
MIN_SAMPLES = (1, 2, 5)
EPSILONS = (0.0, float(np.sqrt(0.3)))
SPREAD = 0.035
D = 512
# name -> (seed, identities, lo, hi, randoms, duplicates): tests/golden/make_face_cluster_golden.py::CASES, repeated
CASES = {
    "a": (101, 40, 2, 29, 60, 0),
    "b": (204, 120, 6, 22, 300, 0),
    "c": (303, 10, 3, 12, 8, 6),
    "n2": (404, 1, 2, 2, 0, 0),
    "n3": (505, 1, 3, 3, 0, 0),
}


def planted(seed, identities, lo, hi, randoms, duplicates=0, d=D):
    """tests/golden/make_face_cluster_golden.py::planted, repeated (d is 512 there)."""
    rng = np.random.default_rng(seed)
    rows, ident = [], []
    for k in range(identities):
        c = rng.standard_normal(d)
        c /= np.linalg.norm(c)
        for _ in range(int(rng.integers(lo, hi + 1))):
            rows.append(c + SPREAD * rng.standard_normal(d))
            ident.append(k)
    for _ in range(randoms):
        rows.append(rng.standard_normal(d))
        ident.append(-1)
    x = np.asarray(rows)
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * rng.uniform(5.0, 30.0, (len(rows), 1))
    order = rng.permutation(len(rows))
    x, ident = x[order].astype(np.float32), np.asarray(ident, np.int64)[order]
    if duplicates:
        src = rng.choice(len(x), size=duplicates, replace=False)
        x, ident = np.concatenate([x, x[src]]), np.concatenate([ident, ident[src]])
    return np.ascontiguousarray(x), ident


def person_inputs(seed=606):
    """tests/golden/make_face_cluster_golden.py::person_inputs, repeated."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((14, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows, labels = [], []
    for k in range(14):
        for _ in range(int(rng.integers(2, 9))):
            rows.append(centres[k] + SPREAD * rng.standard_normal(D))
            labels.append(k)
    for _ in range(9):
        rows.append(rng.standard_normal(D))
        labels.append(-1)
    order = rng.permutation(len(rows))
    emb = np.asarray(rows)[order]
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    labels = np.asarray(labels, np.int64)[order]
    face_ids = (1000 + 3 * rng.permutation(len(rows))).tolist()

    def near(k, noise):
        v = centres[k] + noise * rng.standard_normal(D)
        return (v * rng.uniform(0.5, 4.0)).astype(np.float32)

    existing = {7: near(0, 0.030), 3: near(0, 0.012), 12: near(3, 0.02), 5: ((centres[5] + centres[6]) * 0.7).astype(np.float32),
                9: rng.standard_normal(D).astype(np.float32)}
    queries = [near(0, 0.02).tobytes(), near(3, 0.03).tobytes(), near(8, 0.02).tobytes(), rng.standard_normal(D).astype(np.float32).tobytes(),
               near(5, 0.05).tobytes(), np.ones(256, np.float32).tobytes()]
    return emb, labels, face_ids, existing, queries


def canonical(labels):
    """Clusters renamed by first occurrence; noise stays -1."""
    names, out = {}, []
    for v in np.asarray(labels).tolist():
        out.append(-1 if v < 0 else names.setdefault(v, len(names)))
    return np.asarray(out, np.int64)


def assert_same_partition(got, want, what=""):
    got, want = canonical(got), canonical(want)
    assert np.array_equal(got < 0, want < 0), f"{what}: the noise sets differ at {np.flatnonzero((got < 0) != (want < 0))[:10]}"
    assert np.array_equal(got, want), f"{what}: partitions differ at {np.flatnonzero(got != want)[:10]}"


def case_input(g, name):
    x, ident = planted(*CASES[name])
    assert hashlib.sha1(x.tobytes()).hexdigest() == str(g[f"{name}_sha1"]), f"case {name}: the seeded generator gives other rows than at golden time"
    return x, ident


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


class HostMatch:
    """The contract of Engine.cosine_best_match in numpy (float32 rows normalised, largest similarity, first index among equals)."""

    @staticmethod
    def cosine_best_match(queries, candidates):
        q = np.asarray(queries, np.float32)
        c = np.asarray(candidates, np.float32)
        q = q / (np.linalg.norm(q, axis=1, keepdims=True) + np.float32(1e-10))
        c = c / (np.linalg.norm(c, axis=1, keepdims=True) + np.float32(1e-10))
        s = q @ c.T
        idx = np.argmax(s, axis=1)
        return s[np.arange(len(q)), idx].astype(np.float32), idx.astype(np.int32)


@pytest.mark.parametrize("name", list(CASES))
def test_hdbscan_labels_equal_the_sklearn_partition(golden, name):
    n = int(golden[f"{name}_n"])
    for ms in MIN_SAMPLES:
        if ms > n:
            continue
        u, v, w = golden[f"{name}_mst_u_{ms}"].astype(np.int64), golden[f"{name}_mst_v_{ms}"].astype(np.int64), golden[f"{name}_mst_w_{ms}"]
        assert len(u) == n - 1
        rng = np.random.default_rng(ms)
        orders = [np.arange(n - 1), np.arange(n - 1)[::-1], rng.permutation(n - 1)]      # equal weights meet in three different orders
        for ei, eps in enumerate(EPSILONS):
            want = golden[f"{name}_labels_{ms}_{ei}"]
            for k, o in enumerate(orders):
                got = hdbscan_labels(n, u[o], v[o], w[o], 2, eps)
                assert_same_partition(got, want, f"case {name} min_samples {ms} eps {eps:.3f} order {k}")


def test_fixture_has_tied_weights_and_duplicates(golden):
    """Case c carries exact duplicate rows: zero-weight edges and tied weights must be in the fixture, or the order test shows nothing."""
    w = golden["c_mst_w_2"]
    assert (w == 0).sum() >= 6 and len(np.unique(w)) < len(w)
    assert len(np.unique(golden["a_mst_w_5"])) < len(golden["a_mst_w_5"])


def test_hdbscan_labels_numbering_and_arguments():
    # two tight pairs (joined at 1.0) and a tight triple, the groups joined at 5.0: three clusters, numbered from 0
    u, v = np.array([0, 2, 0, 4, 5, 0]), np.array([1, 3, 2, 5, 6, 4])
    w = np.array([0.1, 0.1, 1.0, 0.1, 0.1, 5.0])
    got = hdbscan_labels(7, u, v, w, 2)
    assert got.dtype == np.int64 and sorted(set(got.tolist())) == [0, 1, 2]
    assert got[0] == got[1] and got[2] == got[3] and got[0] != got[2] and got[4] == got[5] == got[6] and got[4] not in (got[0], got[2])
    # epsilon 2.0: the pairs were born at 1.0 < 2.0 and climb to their ancestor born at 5.0; the triple already is next to the root
    merged = hdbscan_labels(7, u, v, w, 2, 2.0)
    assert merged[0] == merged[1] == merged[2] == merged[3] and merged[4] == merged[5] == merged[6] != merged[0]
    assert sorted(set(merged.tolist())) == [0, 1]
    # a far outlier is noise
    assert hdbscan_labels(8, np.append(u, 0), np.append(v, 7), np.append(w, 50.0), 2)[7] == -1
    assert hdbscan_labels(1, [], [], [], 2).tolist() == [-1]
    with pytest.raises(ValueError):
        hdbscan_labels(4, [0, 1], [1, 2], [1.0, 1.0], 2)
    with pytest.raises(ValueError):
        hdbscan_labels(3, [0, 0], [1, 1], [1.0, 1.0], 2)          # a cycle, not a tree
    with pytest.raises(ValueError):
        hdbscan_labels(3, [0, 1], [1, 2], [1.0, 1.0], 1)


def test_parameter_derivations():
    c = FaceClusterer(None)
    assert (c.min_faces, c.min_samples, c.cluster_selection_epsilon, c.merge_threshold) == (2, 2, 0.15, 0.6)
    assert c.euclidean_epsilon == float(np.sqrt(2 * 0.15))
    assert FaceClusterer(None, min_faces=1).min_samples == 1
    assert FaceClusterer(None, min_faces=7).min_samples == 2
    assert FaceClusterer(None, min_faces=7, min_samples=4).min_samples == 4
    off = FaceClusterer(None, auto_merge_distance=0)
    assert off.cluster_selection_epsilon is None and off.euclidean_epsilon == 0.0


def test_too_few_faces_are_all_noise_and_no_engine_is_an_error():
    x = np.random.default_rng(0).standard_normal((3, D)).astype(np.float32)
    assert FaceClusterer(None, min_faces=5).cluster_embeddings(x).tolist() == [-1, -1, -1]
    assert FaceClusterer(None).cluster_embeddings(x[:1]).tolist() == [-1]
    assert FaceClusterer(None).cluster_embeddings(np.zeros((0, D), np.float32)).tolist() == []
    with pytest.raises(RuntimeError, match="GPU"):
        FaceClusterer(None).cluster_embeddings(x)


def test_normalise_rows_is_the_reference_expression():
    x = np.random.default_rng(1).standard_normal((5, D)).astype(np.float32) * 17
    want = x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-10)
    got = normalise_rows(x)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def check_assign_persons(engine_like, golden):
    """Shared with the GPU test: our assign_persons against what the reference's _update_database wrote."""
    emb, labels, face_ids, existing, _ = person_inputs()
    assert hashlib.sha1(emb.tobytes() + b"".join(existing[k].tobytes() for k in existing)).hexdigest() == str(golden["persons_sha1"])
    fc = FaceClusterer(engine_like, merge_threshold=0.6)
    for tag in ("fresh", "merge"):
        order = golden[f"persons_{tag}_read_order"].tolist()
        persons = {pid: existing[pid] for pid in order}        # the order the reference read them in
        assert (tag == "merge") == bool(persons)
        assignment, new = fc.assign_persons(labels, emb, face_ids, persons)
        new_ids = golden[f"persons_{tag}_new_id"].tolist()
        assert len(new) == len(new_ids)
        want = golden[f"persons_{tag}_face_person"].tolist()
        for fid, lab, w in zip(face_ids, labels.tolist(), want):
            if lab < 0:
                assert fid not in assignment and w == -1
                continue
            key = assignment[fid]
            got = new_ids[key[1]] if isinstance(key, tuple) else key
            assert got == w, (tag, fid, key, w)
        for i, rec in enumerate(new):
            assert rec["representative_face_id"] == int(golden[f"persons_{tag}_new_rep"][i])
            assert rec["face_count"] == int(golden[f"persons_{tag}_new_count"][i]) == len(rec["face_ids"])
            assert rec["centroid"] == golden[f"persons_{tag}_new_centroid"][i].tobytes()       # same numpy expression: same bytes
    return fc, existing


def check_match_face(engine_like, golden):
    _, _, _, existing, queries = person_inputs()
    fc = FaceClusterer(engine_like, merge_threshold=0.6)
    got = [fc.match_face_to_person(q, existing) for q in queries]
    assert [-1 if g is None else g for g in got] == golden["persons_match"].tolist()
    got = [fc.match_face_to_person(q, existing, threshold=0.95) for q in queries]
    assert [-1 if g is None else g for g in got] == golden["persons_match_095"].tolist()
    assert fc.match_face_to_person(np.ones(256, np.float32).tobytes(), existing) is None          # wrong length
    assert fc.match_face_to_person(queries[0], {}) is None
    assert 3 in golden["persons_match"].tolist() and -1 in golden["persons_match"].tolist()


def test_assign_persons_equals_the_reference(golden):
    check_assign_persons(HostMatch, golden)


def test_match_face_to_person_equals_the_reference(golden):
    check_match_face(HostMatch, golden)


def test_module_does_not_import_cpu_clustering_libraries():
    import re
    import facet_amd.face_cluster as m
    text = open(m.__file__).read()
    assert not re.search(r"^\s*(from|import)\s+(sklearn|scipy|hdbscan|oracle)\b", text, flags=re.M)


def test_engine_exposes_the_three_calls():
    from facet_amd import Engine
    from facet_amd._lib import SIGNATURES
    for name in ("fe_knn_core_distances", "fe_mreach_mst", "fe_cosine_best_match"):
        assert name in SIGNATURES
    for name in ("core_distances", "mreach_mst", "cosine_best_match"):
        assert callable(getattr(Engine, name))
