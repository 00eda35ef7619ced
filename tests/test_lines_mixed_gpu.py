"""GPU: fe_leading_lines_mixed (Engine.leading_lines_mixed) - the leading lines of a list of images of mixed sizes in one call. For every
image the Canny edge image and the Hough segments must equal oracle/lines_ref.py's and fe_leading_lines's for that image alone (integer
work: exact). Shapes: 1 x 1 and 3 x 3; 1 x 7 (one row: borders on both sides of every pixel); 16 x 16 and 17 x 31 (exact, and one over, a
labelling tile); 33 x 47; 64 x 65 (one column past the Sobel tile); 97 x 131; 64 x 300; 257 x 256; 48 x 1100; 64 x 96 twice, not as
neighbours."""
import numpy as np
import pytest

from oracle import lines_ref as R
from facet_amd import EngineError
from facet_amd._lib import EngineCapacityError
from facet_amd.composition import CompositionAnalyzer

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 3), (1, 7), (64, 96), (16, 16), (17, 31), (33, 47), (64, 65), (97, 131), (64, 300), (64, 96), (257, 256), (48, 1100)]
NOISE = (0, 6, 25, 3)


def scene(h, w, seed, noise):
    """tests/test_lines_gpu.py's scene: bars, a diagonal band, a disc and graded noise."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), 50, np.int32)
    img[h // 5:h // 5 + 5, w // 10:w - w // 10] = (200, 180, 90)
    img[h // 8:h - h // 8, w // 3:w // 3 + 4] = (30, 220, 220)
    for t in range(min(h, w) - 30):
        img[12 + t, 8 + t:14 + t] = (240, 240, 240)
    yy, xx = np.mgrid[:h, :w]
    img[(yy - h * 0.7) ** 2 + (xx - w * 0.7) ** 2 < (min(h, w) * 0.15) ** 2] = (120, 40, 200)
    img += (xx[..., None] * 40 // w)
    img += rng.integers(-noise, noise + 1, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def imgs():
    return [scene(h, w, 30 + k, NOISE[k % 4]) for k, (h, w) in enumerate(SHAPES)]


@pytest.fixture(scope="module")
def want(imgs):
    """the oracle's (result dict, segments, edges) per image, computed once"""
    return [R.detect_leading_lines(im) for im in imgs]


def check(got_lines, got_edges, want):
    assert len(got_lines) == len(got_edges) == len(want)
    for k, (l, e, (_, wl, we)) in enumerate(zip(got_lines, got_edges, want)):
        assert e.shape == we.shape and np.array_equal(e, we), k
        assert l.dtype == np.int32 and l.tolist() == np.asarray(wl).reshape(-1, 4).tolist(), k


def test_edges_and_segments_equal_oracle_and_per_shape_call(engine, imgs, want):
    lines, edges = engine.leading_lines_mixed(imgs, want_edges=True)
    check(lines, edges, want)
    assert sum(len(l) for l in lines) >= 4 and sum(int(e.any()) for e in edges) >= 8      # not a comparison of empty lists
    for k, im in enumerate(imgs):
        l1, e1 = engine.leading_lines(im[None], want_edges=True)
        assert np.array_equal(edges[k], e1[0]) and lines[k].tolist() == l1[0].tolist(), k
    assert [len(l) for l in engine.leading_lines_mixed(imgs)] == [len(l) for l in lines]      # without the edges
    res = CompositionAnalyzer.detect_leading_lines_mixed(engine, imgs)
    assert res == [w[0] for w in want]


def test_rgb_order_on_reversed_channels(engine, imgs, want):
    lines, edges = engine.leading_lines_mixed([np.ascontiguousarray(im[..., ::-1]) for im in imgs], order='rgb', want_edges=True)
    check(lines, edges, want)


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
        lines, edges = engine.leading_lines_mixed(([d.value + o for o in offs], SHAPES), order=order, want_edges=True)
    finally:
        engine.dev_free(d)
    check(lines, edges, want)


def test_other_thresholds_and_room_for_one_line(engine, imgs):
    kw = dict(canny_low=20, canny_high=60, threshold=30, max_line_gap=3)
    lines, edges = engine.leading_lines_mixed(imgs, min_line_length=10, max_lines=1, want_edges=True, **kw)      # the binding runs again with room
    assert max(len(l) for l in lines) > 1
    for k, im in enumerate(imgs):
        ref_e = R.canny_u8(R.gaussian5_u8(R.bgr2gray(im)), 20, 60)
        assert np.array_equal(edges[k], ref_e), k
        assert lines[k].tolist() == np.asarray(R.hough_lines_p(ref_e, 30, 10, 3)).reshape(-1, 4).tolist(), k
    # one minimum length per image
    per = [3 + 2 * k for k in range(len(imgs))]
    got = engine.leading_lines_mixed(imgs, min_line_length=per, **kw)
    for k, im in enumerate(imgs):
        ref_e = R.canny_u8(R.gaussian5_u8(R.bgr2gray(im)), 20, 60)
        assert got[k].tolist() == np.asarray(R.hough_lines_p(ref_e, 30, per[k], 3)).reshape(-1, 4).tolist(), k


def test_several_chunks_give_the_same(imgs, want):
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 20)      # 8 bytes per pixel and 3 staged: 257 x 256 alone takes 0.7 MiB, the list 2.3 MiB
    try:
        lines, edges = e.leading_lines_mixed(imgs, want_edges=True)
        check(lines, edges, want)
        big = np.zeros((400, 400, 3), np.uint8)      # 1.76 MB of its own
        with pytest.raises(EngineCapacityError, match=r"image 1 \(400 x 400\) needs \d+ bytes of scratch, the arena holds 1048576"):
            e.leading_lines_mixed([imgs[3], big])
        check(*e.leading_lines_mixed(imgs[:5], want_edges=True), want[:5])
    finally:
        e.close()


def test_flat_images_have_no_edges_and_no_lines(engine):
    flat = [np.full((h, w, 3), v, np.uint8) for (h, w), v in zip([(40, 50), (1, 1), (17, 31), (3, 3)], (99, 0, 255, 7))]
    lines, edges = engine.leading_lines_mixed(flat, want_edges=True)
    assert not any(e.any() for e in edges) and all(len(l) == 0 for l in lines)
    assert CompositionAnalyzer.detect_leading_lines_mixed(engine, flat) == [{'leading_lines_score': 0, 'line_count': 0}] * 4


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
            (dict(images=[good], canny_low=-1), r"bad thresholds"),
            (dict(images=[good], canny_low=100, canny_high=50), r"bad thresholds"),
            (dict(images=[good], threshold=0), r"bad thresholds"),
            (dict(images=[good], max_line_gap=-1), r"bad thresholds"),
            (dict(images=[good, good], min_line_length=[3, -2]), r"image 1: min_line_length -2"),
        ]
        for kw, msg in cases:
            with pytest.raises(EngineError, match=msg):
                engine.leading_lines_mixed(**kw)
            lines, edges = engine.leading_lines_mixed([good], want_edges=True)      # the next good call still equals the oracle
            check(lines, edges, want[3:4])
    finally:
        engine.dev_free(d)
