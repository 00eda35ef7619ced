"""Subject-region detection on the GPU: fe_external_contours and fe_subject_region against the restatement (tests/subject_ref.py) and
the golden file made with the reference's own function. Integer work throughout, so every comparison is exact. Shapes are no multiple
of the 16x16 labelling tile and span several tiles both ways."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subject_ref as S                                   # noqa: E402
from test_subject_host import spiral                      # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(97, 131), (200, 260), (64, 300), (257, 256)]
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "subject_golden.json")))


def ring(a, m, t=1):
    h, w = a.shape
    a[m:h - m, m:w - m] = 1
    a[m + t:h - m - t, m + t:w - m - t] = 0


def drawn(h, w):
    out = {"spiral": spiral(h, w)}
    a = np.zeros((h, w), np.uint8)
    for m in (10, 6, 2):                                    # innermost first: each larger ring is drawn around the ones inside
        b = np.zeros((h, w), np.uint8); ring(b, m); a |= b
    out["nested3"] = a
    a = np.zeros((h, w), np.uint8); ring(a, 0)
    b = np.zeros((h, w), np.uint8); ring(b, 5, 2); a |= b
    a[h // 2, w // 2] = 1
    out["ring_in_frame_ring"] = a
    a = np.zeros((h, w), np.uint8); a[3, 2:w - 2] = 1; a[3:h - 3, 2:w - 2:2] = 1
    out["comb"] = a
    a = np.zeros((h, w), np.uint8)
    for t in range(min(h, w)):
        a[t, t] = 1
        a[t, w - 1 - t] = 1
    for x in range(w - 1):
        a[h - 2 - (x & 1), x] = 1                           # zigzag: diagonal links only
    out["diagonals"] = a
    a = np.zeros((h, w), np.uint8); a[::3, ::3] = 1
    out["isolated"] = a
    return out


def check(engine, imgs, **kw):
    got = engine.external_contours(np.stack(imgs), **kw)
    for k, (g, img) in enumerate(zip(got, imgs)):
        want, _ = S.records(img, kw.get("min_twice_area", 0))
        assert g.tolist() == want.tolist(), k
    return got


@pytest.mark.parametrize("h,w", SHAPES)
def test_external_contours_on_drawn_images(engine, h, w):
    d = drawn(h, w)
    got = check(engine, list(d.values()))                   # one batch of 6 different images; 'isolated' exceeds the default room
    names = list(d)
    assert len(got[names.index("nested3")]) == 1 and len(got[names.index("ring_in_frame_ring")]) == 1
    assert len(got[names.index("spiral")]) == 1 and len(got[names.index("isolated")]) == ((h + 2) // 3) * ((w + 2) // 3) > 256


def test_external_contours_noise_batch_area_filter_and_recall(engine):
    rng = np.random.default_rng(11)
    h, w = 97, 131
    noise = (rng.random((h, w)) < 0.35).astype(np.uint8) * 255
    d = drawn(h, w)
    imgs = [noise, d["comb"], d["nested3"], (rng.random((h, w)) < 0.5).astype(np.uint8), d["diagonals"]]
    check(engine, imgs)
    check(engine, imgs, max_contours=1)                     # forces the second call
    check(engine, imgs, min_twice_area=12)
    # the same from device memory
    a = np.ascontiguousarray(np.stack(imgs))
    p = engine.dev_alloc(a.nbytes)
    try:
        engine.h2d(p, a)
        dev = engine.external_contours((p, len(imgs), h, w))
    finally:
        engine.dev_free(p)
    assert [g.tolist() for g in dev] == [S.records(i)[0].tolist() for i in imgs]


@pytest.mark.parametrize("h,w", SHAPES)
def test_subject_region_equals_restatement(engine, h, w):
    imgs = np.stack([S.scene(h, w, 20 + k, n, kind) for k, (n, kind) in
                     enumerate([(0, "disc"), (0, "bars"), (0, "gradient"), (0, "mixed"), (6, "mixed"), (25, "mixed")])])
    rec, edges, thr = engine.subject_contours(imgs, want_edges=True, want_thresholds=True)
    for k in range(len(imgs)):
        want, wthr, wedges = S.subject_records(imgs[k])
        assert tuple(thr[k]) == wthr, k
        assert np.array_equal(edges[k], wedges), k
        assert rec[k].tolist() == want.tolist(), k
    assert edges.any() and sum(len(r) for r in rec) > 3
    p = engine.dev_alloc(imgs.nbytes)
    try:
        engine.h2d(p, imgs)
        dev = engine.subject_contours((p, len(imgs), h, w))
    finally:
        engine.dev_free(p)
    assert [g.tolist() for g in dev] == [g.tolist() for g in rec]


def test_boxes_equal_the_golden_file(engine):
    from facet_amd.composition import CompositionAnalyzer
    for g in GOLDEN:
        img = S.scene(g["h"], g["w"], g["seed"], g["noise"], g["kind"])
        assert CompositionAnalyzer.detect_subject_region(img, engine=engine) == g["box"], g["seed"]
        assert CompositionAnalyzer.get_placement_data(None, g["w"], g["h"], None, img, engine) == g["placement"], g["seed"]


def test_degenerate_inputs(engine):
    for h, w in ((40, 50), (1, 1), (3, 3)):
        for v in (0, 255):
            rec, edges, thr = engine.subject_contours(np.full((2, h, w, 3), v, np.uint8), want_edges=True, want_thresholds=True)
            want = S.subject_records(np.full((h, w, 3), v, np.uint8))
            assert [len(r) for r in rec] == [0, 0] and not edges.any() and len(want[0]) == 0
            assert thr.tolist() == [list(want[1])] * 2 and (v != 0 or thr.tolist() == [[0, 0]] * 2)
    assert [r.tolist() for r in engine.external_contours(np.ones((1, 1, 1), np.uint8))] == [[[0, 0, 0, 0, 0, 0, 0, 0]]]
    assert [r.tolist() for r in engine.external_contours(np.ones((1, 3, 3), np.uint8))] == [S.records(np.ones((3, 3), np.uint8))[0].tolist()]
    assert [len(r) for r in engine.external_contours(np.zeros((2, 3, 3), np.uint8))] == [0, 0]
    nones = [g for g in GOLDEN if g["box"] is None and (g["h"], g["w"]) == (97, 131)]
    assert len(nones) == 2
    from facet_amd.composition import CompositionAnalyzer
    batch = np.stack([S.scene(g["h"], g["w"], g["seed"], g["noise"], g["kind"]) for g in nones])
    assert CompositionAnalyzer.detect_subject_region_batch(engine, batch) == [None, None]


def test_batch_scorer_option():
    """On a context of its own with no model loaded: comp_score is then the rule-based one (SAMP-Net's score, when that model is loaded,
    replaces it with or without the option, scorer.py:675-690), so both columns are the golden placement's."""
    from facet_amd import Engine
    from facet_amd.batch import BatchScorer
    gs = [g for g in GOLDEN if (g["h"], g["w"]) == (97, 131)]
    assert len(gs) >= 5
    rgb = np.stack([S.scene(g["h"], g["w"], g["seed"], g["noise"], g["kind"])[..., ::-1] for g in gs])
    e = Engine(0, arena_bytes=1 << 30)
    try:
        on = BatchScorer(e, subject_region=True).process_batch(rgb)
        off, today = BatchScorer(e, subject_region=False).process_batch(rgb), BatchScorer(e).process_batch(rgb)
    finally:
        e.close()
    for r, g in zip(on, gs):
        assert r["power_point_score"] == float(g["placement"]["power_point_score"]) and r["comp_score"] == round(g["placement"]["score"], 2)
    assert len({r["power_point_score"] for r in on}) > 2
    for a, b in zip(off, today):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], k
        assert a["power_point_score"] == 5.0 and a["comp_score"] == 7.0
