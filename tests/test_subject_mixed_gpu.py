"""GPU: fe_subject_region_mixed (Engine.subject_contours_mixed) - the subject-region contours of a list of images of mixed sizes in one
call. For every image the thresholds, the edge image and the contour records (with their order) must equal the restatement's
(tests/subject_ref.py) and fe_subject_region's for that image alone; integer work, so exact. Shapes as in tests/test_lines_mixed_gpu.py:
1 x 1, 3 x 3, 1 x 7, 16 x 16 and 17 x 31 (exact, and one over, a labelling tile), 33 x 47, 64 x 65, 97 x 131, 64 x 300, 257 x 256,
48 x 1100, and 64 x 96 twice, not as neighbours."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subject_ref as S                                   # noqa: E402

from facet_amd import EngineError                         # noqa: E402
from facet_amd._lib import EngineCapacityError            # noqa: E402
from facet_amd.composition import CompositionAnalyzer     # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 3), (1, 7), (64, 96), (16, 16), (17, 31), (33, 47), (64, 65), (97, 131), (64, 300), (64, 96), (257, 256), (48, 1100)]
KINDS = [(0, "disc"), (0, "bars"), (0, "gradient"), (0, "mixed"), (6, "mixed"), (25, "mixed")]
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "subject_golden.json")))


@pytest.fixture(scope="module")
def imgs():
    return [S.scene(h, w, 40 + k, *KINDS[k % 6]) for k, (h, w) in enumerate(SHAPES)]


@pytest.fixture(scope="module")
def want(imgs):
    """the restatement's (records, (lower, upper), edges) per image, computed once"""
    return [S.subject_records(im) for im in imgs]


def check(got, want):
    rec, edges, thr = got
    assert len(rec) == len(edges) == len(thr) == len(want)
    for k, (wrec, wthr, wedges) in enumerate(want):
        assert tuple(thr[k]) == wthr, k
        assert edges[k].shape == wedges.shape and np.array_equal(edges[k], wedges), k
        assert rec[k].dtype == np.int64 and rec[k].tolist() == wrec.tolist(), k


def test_records_thresholds_and_edges_equal_restatement_and_per_shape_call(engine, imgs, want):
    got = engine.subject_contours_mixed(imgs, want_edges=True, want_thresholds=True)
    check(got, want)
    assert sum(len(r) for r in got[0]) > 6 and sum(int(e.any()) for e in got[1]) >= 8      # not a comparison of empty lists
    for k, im in enumerate(imgs):
        r1, e1, t1 = engine.subject_contours(im[None], want_edges=True, want_thresholds=True)
        assert got[0][k].tolist() == r1[0].tolist() and np.array_equal(got[1][k], e1[0]) and got[2][k].tolist() == t1[0].tolist(), k
    plain = engine.subject_contours_mixed(imgs)
    assert [r.tolist() for r in plain] == [r.tolist() for r in got[0]]
    boxes = CompositionAnalyzer.detect_subject_region_mixed(engine, imgs)
    assert boxes == [CompositionAnalyzer.detect_subject_region(im, engine=engine) for im in imgs] and any(b is not None for b in boxes)


def test_rgb_order_on_reversed_channels(engine, imgs, want):
    check(engine.subject_contours_mixed([np.ascontiguousarray(im[..., ::-1]) for im in imgs], order='rgb', want_edges=True, want_thresholds=True), want)


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_resident_images_at_odd_byte_offsets(engine, imgs, want, order):
    src = imgs if order == "bgr" else [np.ascontiguousarray(im[..., ::-1]) for im in imgs]
    at, offs = 0, []
    for k, im in enumerate(src):      # back to back, each start moved to 1, 2 or 3 mod 4
        at += (1 + k % 3 - at) % 4
        offs.append(at)
        at += im.nbytes
    assert {o % 4 for o in offs} == {1, 2, 3}
    buf = np.zeros(at, np.uint8)
    for o, im in zip(offs, src):
        buf[o:o + im.nbytes] = im.ravel()
    d = engine.dev_alloc(at)
    try:
        engine.h2d(d, buf)
        got = engine.subject_contours_mixed(([d.value + o for o in offs], SHAPES), order=order, want_edges=True, want_thresholds=True)
    finally:
        engine.dev_free(d)
    check(got, want)


def test_several_chunks_give_the_same(imgs, want):
    from facet_amd import Engine
    e = Engine(0, arena_bytes=5 << 20)      # about 58 bytes per pixel staged: 257 x 256 alone takes 3.7 MiB, the list 12 MiB
    try:
        check(e.subject_contours_mixed(imgs, want_edges=True, want_thresholds=True), want)
        big = np.zeros((400, 400, 3), np.uint8)      # 9 MB of its own
        with pytest.raises(EngineCapacityError, match=r"image 1 \(400 x 400\) needs \d+ bytes of scratch, the arena holds 5242880"):
            e.subject_contours_mixed([imgs[3], big])
        check(e.subject_contours_mixed(imgs[:5], want_edges=True, want_thresholds=True), want[:5])
    finally:
        e.close()


def dots(h, w):
    """3 x 3 bright squares every 6 pixels on a dark field: one closed edge ring per square, 352 contours at 97 x 131"""
    a = np.full((h, w), 20, np.uint8)
    for dy in range(3):
        for dx in range(3):
            a[1 + dy::6, 1 + dx::6] = 230
    return np.repeat(a[..., None], 3, 2)


def test_more_contours_than_room_next_to_images_with_none(engine, imgs, want):
    many = dots(97, 131)
    wmany = S.subject_records(many)
    assert len(wmany[0]) > 256
    zeros, full = np.zeros((64, 96, 3), np.uint8), np.full((17, 31, 3), 255, np.uint8)
    lst = [zeros, many, full, imgs[8], np.zeros((1, 1, 3), np.uint8), np.full((3, 3, 3), 255, np.uint8), np.zeros((3, 3, 3), np.uint8),
           np.full((1, 1, 3), 255, np.uint8)]
    wlst = [S.subject_records(im) for im in lst[:3]] + [want[8]] + [S.subject_records(im) for im in lst[4:]]
    assert [len(w[0]) for w in wlst][:3] == [0, len(wmany[0]), 0] and all(len(w[0]) == 0 and not w[2].any() for w in wlst[4:])
    assert wlst[0][1] == (0, 0)
    check(engine.subject_contours_mixed(lst, want_edges=True, want_thresholds=True), wlst)      # default room 256: the binding runs again
    check(engine.subject_contours_mixed(lst, max_contours=1, want_edges=True, want_thresholds=True), wlst)
    # the call itself: exact counts, and the first `room` records in order
    import ctypes as C
    ptrs, hw, n, dev, keep = engine._img_list(lst)
    rec, cnt = np.full((n, 2, 8), -7, np.int64), np.zeros(n, np.int32)
    rc = engine.lib.fe_subject_region_mixed(engine.h, ptrs, hw.ctypes.data_as(C.POINTER(C.c_int32)), n, dev, 0, 2, rec.ctypes.data_as(C.c_void_p),
                                            cnt.ctypes.data_as(C.c_void_p), None, None)
    assert rc == 0 and cnt.tolist() == [len(w[0]) for w in wlst]
    for k, w in enumerate(wlst):
        m = min(2, len(w[0]))
        assert rec[k, :m].tolist() == w[0][:m].tolist() and (rec[k, m:] == -7).all(), k


def test_golden_boxes_as_one_mixed_list(engine):
    lst = [S.scene(g["h"], g["w"], g["seed"], g["noise"], g["kind"]) for g in GOLDEN]
    assert len({im.shape for im in lst}) >= 4
    assert CompositionAnalyzer.detect_subject_region_mixed(engine, lst) == [g["box"] for g in GOLDEN]
    rgb = [np.ascontiguousarray(im[..., ::-1]) for im in lst]
    assert CompositionAnalyzer.detect_subject_region_mixed(engine, rgb, order='rgb') == [g["box"] for g in GOLDEN]


def test_bad_arguments_raise_and_leave_the_engine_usable(engine, imgs, want):
    good = imgs[3]
    d = engine.dev_alloc(good.nbytes)
    try:
        engine.h2d(d, good)
        cases = [
            (dict(images=[]), r"null list|n <= 0"),
            (dict(images=[good, None, good]), r"image 1 is a null pointer"),
            (dict(images=([d.value, None], [(64, 96), (64, 96)])), r"image 1 is a null pointer"),
            (dict(images=([d.value, d.value], [(64, 96), (0, 96)])), r"image 1 is 0 x 96"),
            (dict(images=([d.value, d.value, d.value], [(64, 96), (64, 96), (64, -1)])), r"image 2 is 64 x -1"),
            (dict(images=([d.value, d.value], [(64, 96), (32768, 32768)])), r"image 1 is 32768 x 32768 .*2\^30"),
            (dict(images=[good], order=2), r"order 2"),
        ]
        for kw, msg in cases:
            with pytest.raises(EngineError, match=msg):
                engine.subject_contours_mixed(**kw)
            check(engine.subject_contours_mixed([good], want_edges=True, want_thresholds=True), want[3:4])      # the next good call still equals the restatement
    finally:
        engine.dev_free(d)
