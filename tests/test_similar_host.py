"""CPU: the similar-photo and person-merge mirrors against the reference's recorded results (tests/golden/similar_golden.json),
driven through a numpy stand-in for the two engine calls whose scores are perturbed inside the derived fp32 bound - so the guard's
fallback (the pair fetch) runs as well as its fast path, and any reliance on more than the calls' contracts shows."""
import json

import numpy as np
import pytest

from facet_amd.person_merge import merge_candidates, merge_groups
from facet_amd.similar import SimilarPhotoIndex, cosine_error_bound, guard_margin, score_error_bound
from similar_golden_lib import build_index_inputs, build_persons, load_golden
from similar_standin import StandInEngine, brute_scores, random_rows

G = load_golden()
W = (0.4, 0.3, 0.2, 0.1)


def plain(x):
    return json.loads(json.dumps(x))


def make_index(wobble_of_bound, seed):
    eng = StandInEngine(wobble_of_bound * score_error_bound(G["library"]["d"], (1.0, 1.0, 1.0, 1.0)), seed)
    index = SimilarPhotoIndex(eng)
    index.add(**build_index_inputs(G["library"]))
    return index, eng


@pytest.mark.parametrize("case", G["cases"], ids=[c["name"] for c in G["cases"]])
@pytest.mark.parametrize("wobble,seed", [(0.0, 0), (1.0, 1), (1.0, 2)])
def test_similar_reproduces_the_reference(case, wobble, seed):
    index, _ = make_index(wobble, seed)
    vis = None if case["hidden"] is None else [p not in set(case["hidden"]) for p in index.paths]
    got = index.similar(case["source"], case["limit"], *case["weights"], visible=vis)
    assert plain(got) == case["result"]


def test_both_guard_branches_run():
    index, eng = make_index(1.0, 3)
    for case in G["cases"]:
        vis = None if case["hidden"] is None else [p not in set(case["hidden"]) for p in index.paths]
        index.similar(case["source"], case["limit"], *case["weights"], visible=vis)
    print(index.stats, eng.calls)
    assert index.stats["guard_passed"] > 0, "no query was answered from the shortlist alone"
    assert index.stats["guard_failed"] > 0 and index.stats["pairs_calls"] > 0, "no query needed the pair fetch"


def test_batch_equals_single_queries():
    index, _ = make_index(1.0, 4)
    rows = list(range(len(index)))
    batch = index.similar_batch(rows, 6)
    for r in (0, 3, 7, 20, len(index) - 1):
        assert batch[r] == index.similar(r, 6)
    assert index.similar_batch(["/photos/src.jpg", "nowhere", 10 ** 6], 3)[1:] == [{'error': 'Photo not found'}] * 2


def test_response_shape_and_roundings():
    index, _ = make_index(0.0, 0)
    res = index.similar("/photos/src.jpg")
    assert list(res) == ['source', 'weights', 'similar'] and res['weights'] == {'clip': 0.4, 'person': 0.3, 'date': 0.2, 'score': 0.1}
    assert len(res['similar']) == 20
    for e in res['similar']:
        assert list(e) == ['path', 'filename', 'similarity', 'breakdown', 'aggregate', 'aesthetic', 'date_taken']
        assert e['similarity'] == round(e['similarity'], 4) and e['similarity'] > 0
        assert set(e['breakdown']) <= {'clip', 'persons', 'date', 'score'} and all(v == round(v, 3) for v in e['breakdown'].values())
    sims = [e['similarity'] for e in res['similar']]
    assert sims == sorted(sims, reverse=True)


def test_margin_is_the_derived_one():
    u = 2.0 ** -24
    assert cosine_error_bound(768) == (768 + 40) * u
    assert score_error_bound(768, W) == pytest.approx(u * (0.4 * (808 / 2 + 4) + 0.9 + 0.8 + 2.4 + 3.0))
    assert guard_margin(768, W) == pytest.approx(1e-4 + score_error_bound(768, W) + 0.4 * 808 * u / 2)
    assert 1e-4 < guard_margin(768, W) < 1.4e-4


def test_stand_in_honours_the_contract():
    rows = random_rows(5, 90, 64)
    eng = StandInEngine()
    s, elig = brute_scores(rows, rows, W, q_self=np.arange(90))
    idx, score = eng.similar_topk(rows, rows, 8, W, q_self=np.arange(90))
    for r in range(90):
        keep = np.nonzero(elig[r] & (s[r] > 0))[0]
        want = keep[np.lexsort((keep, -s[r, keep].astype(np.float32).astype(np.float64)))][:8]
        assert idx[r][:len(want)].tolist() == want.tolist()
    pairs, sc = eng.similar_pairs(rows, rows, 0.5, cosine=True, upper=True)
    cos, _ = brute_scores(rows, rows, cosine=True)
    assert all(a < b and cos[a, b].astype(np.float32) >= np.float32(0.5) for a, b in pairs.tolist())


@pytest.mark.parametrize("wobble,seed", [(0.0, 0), (1.0, 5), (1.0, 6)])
def test_merge_groups_reproduce_the_reference(wobble, seed):
    g = G["merge"]
    eng = StandInEngine(wobble * cosine_error_bound(g["d"]), seed)
    persons = build_persons(g)
    assert plain(merge_groups(eng, persons, g["threshold"])) == g["groups"]
    cands = merge_candidates(eng, persons, g["threshold"])
    assert [[c["person1"]["id"], c["person2"]["id"]] for c in cands] == g["candidate_ids"]
    assert all(list(c) == ['person1', 'person2', 'similarity'] and list(c['person1']) == ['id', 'name', 'face_count'] for c in cands)
    assert merge_groups(eng, persons[:1], 0.6) == [] and merge_groups(eng, [], 0.6) == []
