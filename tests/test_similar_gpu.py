"""GPU: fe_similar_topk / fe_similar_pairs against a float64 brute force, and the similar-photo / person-merge mirrors against the
recorded results of the reference (tests/golden/similar_golden.json). Bounds come from facet_amd/similar.py's derivation."""
import json
import os

import numpy as np
import pytest

from facet_amd import EngineError
from facet_amd._lib import FE_SIM_K_MAX, SimRows
from facet_amd.similar import SimilarPhotoIndex, cosine_error_bound, score_error_bound
from facet_amd.person_merge import merge_candidates, merge_groups
from similar_standin import brute_scores, random_rows
from similar_golden_lib import build_index_inputs, build_persons, load_golden

pytestmark = pytest.mark.gpu
W = (0.4, 0.3, 0.2, 0.1)


def check_topk(q, c, idx, score, k, weights, cosine, bound, q_self=None, visible=None, tag=""):
    s, elig = brute_scores(q, c, weights, cosine, q_self, visible)
    worst = low = beat = 0.0
    for r in range(q.n):
        got = idx[r][idx[r] >= 0]
        assert len(set(got.tolist())) == len(got)
        assert elig[r, got].all(), "a dropped candidate was returned"
        err = np.abs(score[r, :len(got)].astype(np.float64) - s[r, got])
        worst = max(worst, float(err.max(initial=0.0)))
        keys = list(zip((-score[r, :len(got)].astype(np.float64)).tolist(), got.tolist()))
        assert keys == sorted(keys), f"row {r}: not (score descending, index ascending)"
        alive = elig[r] & ((s[r] == s[r]) if cosine else (s[r] > bound))        # surely kept by the device
        ref = np.sort(s[r, alive])[::-1]
        if len(got) < k:
            assert len(got) >= alive.sum(), f"row {r}: {len(got)} returned, {alive.sum()} candidates surely score above 0"
            continue
        kth = float(score[r, k - 1])
        if len(ref) >= k:
            low = max(low, ref[k - 1] - kth)
        out = np.ones(c.n, bool)
        out[got] = False
        out &= elig[r]
        beat = max(beat, float((s[r, out] - kth).max(initial=-1.0)))
    print(f"[similar topk{tag}] nq={q.n} n={c.n} d={q.d} k={k}: max |score - f64| = {worst:.3e} (bound {bound:.3e}), "
          f"f64 k-th above returned k-th by {low:.3e}, best omitted above returned k-th by {beat:.3e} (2 bound {2 * bound:.3e})")
    assert worst <= bound
    assert low <= 2 * bound
    assert beat <= 2 * bound


@pytest.mark.parametrize("n", [131, 300, 4099])
@pytest.mark.parametrize("d", [32, 512, 768, 1024])
def test_topk_matches_float64(engine, n, d):
    rows = random_rows(n * 7 + d, n, d, clusters=9)
    k = 32 if n != 300 else 7
    idx, score = engine.similar_topk(rows, rows, k, W)
    check_topk(rows, rows, idx, score, k, W, False, score_error_bound(d, W))
    idx, score = engine.similar_topk(rows, rows, k, cosine=True)
    check_topk(rows, rows, idx, score, k, W, True, cosine_error_bound(d), tag=" cosine")


@pytest.mark.parametrize("nq", [1, 5, 8])
def test_topk_small_query_path(engine, nq):
    c = random_rows(11, 4099, 768, clusters=5)
    q = random_rows(12 + nq, nq, 768, clusters=5)
    w = (0.5, 0.25, 0.15, 0.6)
    vis = (np.random.default_rng(3).random(c.n) > 0.2).astype(np.uint8)
    q_self = np.arange(nq, dtype=np.int32) * 3 - 1                 # -1 (none), 2, 5, ...
    idx, score = engine.similar_topk(q, c, 20, w, q_self=q_self, visible=vis)
    check_topk(q, c, idx, score, 20, w, False, score_error_bound(768, w), q_self, vis, tag=" gemv")
    for r in range(nq):
        assert q_self[r] not in idx[r] and vis[idx[r][idx[r] >= 0]].all()


def test_topk_exclusions_on_tile_path(engine):
    c = random_rows(21, 1000, 512)
    vis = (np.random.default_rng(4).random(c.n) > 0.5).astype(np.uint8)
    q_self = np.arange(c.n, dtype=np.int32)
    idx, score = engine.similar_topk(c, c, 16, W, q_self=q_self, visible=vis)
    check_topk(c, c, idx, score, 16, W, False, score_error_bound(512, W), q_self, vis, tag=" masked")
    assert not (idx == q_self[:, None]).any()


def check_pairs(q, c, pairs, score, thr, weights, cosine, bound, upper, tag=""):
    s, elig = brute_scores(q, c, weights, cosine, upper=upper)
    t = np.broadcast_to(np.asarray(thr, np.float64).reshape(-1), (q.n,)) if np.ndim(thr) == 0 or len(thr) == 1 else np.asarray(thr, np.float64)
    keep = elig & ((s == s) if cosine else (s > bound))
    sure = keep & (s >= t[:, None] + bound)
    maybe = elig & (s >= t[:, None] - bound) & ((s == s) if cosine else (s > -bound))
    got = np.zeros(s.shape, bool)
    got[pairs[:, 0], pairs[:, 1]] = True
    assert got.sum() == len(pairs), "a pair was reported twice"
    order = pairs[:, 0].astype(np.int64) * c.n + pairs[:, 1]
    assert (np.diff(order) > 0).all(), "pairs are not in ascending (q, c) order"
    err = np.abs(score.astype(np.float64) - s[pairs[:, 0], pairs[:, 1]]).max(initial=0.0)
    print(f"[similar pairs{tag}] nq={q.n} n={c.n} d={q.d}: {len(pairs)} pairs, {int(sure.sum())} surely above, {int(maybe.sum() - sure.sum())} in the "
          f"+-{bound:.2e} band, max |score - f64| = {err:.3e}")
    assert (got | ~sure).all(), "a pair surely above the threshold is missing"
    assert (maybe | ~got).all(), "a pair surely below the threshold was reported"
    assert err <= bound
    return int(sure.sum()), int(maybe.sum())


@pytest.mark.parametrize("n,d", [(131, 32), (300, 768), (4099, 512)])
def test_pairs_match_float64(engine, n, d):
    rows = random_rows(n + d, n, d, clusters=40)
    b = cosine_error_bound(d)
    pairs, score = engine.similar_pairs(rows, rows, 0.55, cosine=True, upper=True)
    lo, hi = check_pairs(rows, rows, pairs, score, 0.55, W, True, b, True, tag=" cosine upper")
    assert lo > 0
    thr = np.random.default_rng(n).uniform(0.55, 0.75, n).astype(np.float32)
    pairs, score = engine.similar_pairs(rows, rows, thr, W)
    check_pairs(rows, rows, pairs, score, thr, W, False, score_error_bound(d, W), False, tag=" fused per-query thr")
    q = random_rows(n + 1, 3, d, clusters=40)
    pairs, score = engine.similar_pairs(q, rows, 0.5, W)
    check_pairs(q, rows, pairs, score, 0.5, W, False, score_error_bound(d, W), False, tag=" gemv")


def test_pairs_capacity_protocol(engine):
    rows = random_rows(5, 700, 256, clusters=10)
    full, score = engine.similar_pairs(rows, rows, 0.5, cosine=True, upper=True)
    assert len(full) > 64
    assert engine.similar_pairs_count(rows, rows, 0.5, cosine=True, upper=True) == len(full)
    # too little room on the first attempt: the binding sees count > room and calls again with exactly enough
    again, score2 = engine.similar_pairs(rows, rows, 0.5, cosine=True, upper=True, max_pairs=8)
    assert np.array_equal(full, again) and score.tobytes() == score2.tobytes()
    exact, _ = engine.similar_pairs(rows, rows, 0.5, cosine=True, upper=True, max_pairs=len(full))
    assert np.array_equal(full, exact)


def test_host_and_device_inputs_and_two_runs_give_the_same_bytes(engine):
    for nq in (3, 600):
        c = random_rows(31, 2000, 768, clusters=7)
        q = random_rows(32, nq, 768, clusters=7)
        a = engine.similar_topk(q, c, 24, W)
        b = engine.similar_topk(q, c, 24, W)
        cd, qd = engine.upload_sim_rows(c), engine.upload_sim_rows(q)
        e = engine.similar_topk(qd, cd, 24, W)
        for x, y in ((a, b), (a, e)):
            assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
        pa = engine.similar_pairs(q, c, 0.6, W)
        pb = engine.similar_pairs(qd, cd, 0.6, W)
        pc = engine.similar_pairs(q, c, 0.6, W)
        assert len(pa[0]) > 0
        for y in (pb, pc):
            assert pa[0].tobytes() == y[0].tobytes() and pa[1].tobytes() == y[1].tobytes()


def test_bad_arguments_raise_and_the_context_stays_usable(engine):
    good = random_rows(1, 200, 64)
    for bad in (lambda: engine.similar_topk(good, good, 0, W),
                lambda: engine.similar_topk(good, good, FE_SIM_K_MAX + 1, W),
                lambda: engine.similar_topk(SimRows(np.zeros((4, 48), np.float32)), SimRows(np.zeros((9, 48), np.float32)), 2, W),
                lambda: engine.similar_topk(SimRows(np.zeros((4, 2048), np.float32)), SimRows(np.zeros((9, 2048), np.float32)), 2, W),
                lambda: engine.similar_pairs(good, good, np.zeros(7, np.float32), W),
                lambda: engine.similar_pairs(random_rows(2, 5, 64), good, 0.5, W, upper=True)):
        with pytest.raises(EngineError):
            bad()
    idx, score = engine.similar_topk(good, good, 4, W)
    check_topk(good, good, idx, score, 4, W, False, score_error_bound(64, W), tag=" after errors")


# ---- the mirrors against the reference's recorded results -----------------------------------------------------------------------
def test_similar_photos_reproduce_the_reference(engine):
    g = load_golden()
    index = SimilarPhotoIndex(engine)
    index.add(**build_index_inputs(g["library"]))
    for case in g["cases"]:
        vis = None if case["hidden"] is None else [p not in set(case["hidden"]) for p in index.paths]
        got = index.similar(case["source"], case["limit"], *case["weights"], visible=vis)
        assert json.loads(json.dumps(got)) == case["result"], case["name"]
    batch = [c for c in g["cases"] if c["hidden"] is None and c["weights"] == list(W) and c["limit"] == 20]
    got = index.similar_batch([c["source"] for c in batch], 20)
    assert [json.loads(json.dumps(x)) for x in got] == [c["result"] for c in batch]
    print("[similar golden]", index.stats)
    assert index.stats["guard_passed"] > 0 and index.stats["guard_failed"] > 0


def test_merge_groups_reproduce_the_reference(engine):
    g = load_golden()["merge"]
    persons = build_persons(g)
    assert json.loads(json.dumps(merge_groups(engine, persons, g["threshold"]))) == g["groups"]
    cands = merge_candidates(engine, persons, g["threshold"])
    assert [(c["person1"]["id"], c["person2"]["id"]) for c in cands] == [tuple(p) for p in g["candidate_ids"]]


def test_planted_library_of_20000(engine):
    rng = np.random.default_rng(77)
    n, d, groups = 20000, 768, 500
    base = rng.standard_normal((n, d)).astype(np.float32)
    member = rng.permutation(n)[:groups * 4].reshape(groups, 4)            # each group: one photo and three planted near-copies
    for grp in member:
        base[grp[1:]] = base[grp[0]] + 0.05 * rng.standard_normal((3, d)).astype(np.float32)
    index = SimilarPhotoIndex(engine)
    index.add([f"/lib/{i:05d}.jpg" for i in range(n)], [base[i].tobytes() for i in range(n)], [None] * n, [None] * n, [()] * n)
    sources = member[:64].reshape(-1).tolist()
    got = index.similar_batch(sources, 5)
    for row, res in zip(sources, got):
        mates = {f"/lib/{i:05d}.jpg" for i in member[np.nonzero(member == row)[0][0]] if i != row}
        assert {e["path"] for e in res["similar"][:3]} == mates
    one = index.similar(sources[0], 5)
    assert one == got[0]
    print("[similar planted]", index.stats)


def test_planted_merge_of_2000_persons(engine):
    rng = np.random.default_rng(78)
    n, d = 2000, 512
    cent = rng.standard_normal((n, d)).astype(np.float32)
    planted = rng.permutation(n)[:150].reshape(50, 3)
    for a, b, c in planted:
        cent[b] = cent[a] + 0.3 * rng.standard_normal(d).astype(np.float32)
        cent[c] = cent[a] + 0.3 * rng.standard_normal(d).astype(np.float32)
    persons = [{"id": i + 1, "name": None, "face_count": int(rng.integers(1, 5000)), "centroid": cent[i].tobytes()} for i in range(n)]
    groups = merge_groups(engine, persons, 0.6)
    assert sorted(sorted(p["id"] for p in g["persons"]) for g in groups) == sorted(sorted(int(v) + 1 for v in t) for t in planted)
    for g in groups:
        assert g["min_similarity"] >= 0.6 and [p["face_count"] for p in g["persons"]] == sorted((p["face_count"] for p in g["persons"]), reverse=True)
    assert [g["avg_similarity"] for g in groups] == sorted((g["avg_similarity"] for g in groups), reverse=True)
