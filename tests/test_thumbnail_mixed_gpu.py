"""GPU: thumbnails of images of mixed sizes in one engine call (fe_thumbnail_jpeg_mixed, Engine.thumbnail_jpeg_mixed,
facet_amd.thumbnail.thumbnails_mixed) against Pillow itself - `thumbnail((size, size), LANCZOS)` + `save("JPEG", quality)`, as
tests/test_thumbnail_gpu.py states it - and against fe_thumbnail_jpeg on every image alone. The 20 images of tests/mixed_index_cases.py
(what their plans cover is asserted by tests/test_thumb_mixed_host.py) with a saturated-noise image (the longest codes, many 0xFF bytes
to stuff) and a flat one beside them in the same call."""
import ctypes

import numpy as np
import pytest
from PIL import Image

from facet_amd._lib import FE_ERR_CAPACITY, FE_ERR_INVALID, EngineCapacityError, EngineError
from facet_amd.thumbnail import thumbnail_plan, thumbnails, thumbnails_mixed
from mixed_index_cases import ALL_SHAPES, CHUNK_ARENA, all_images, chunk_images
from test_thumbnail_gpu import saturated_noise
from test_thumbnail_host import pil_thumbnail

pytestmark = pytest.mark.gpu

CASES = [(64, 80), (640, 30)]      # (size, quality)


@pytest.fixture(scope="module")
def imgs():
    """The 20 shapes, then 96 x 64 saturated noise and a flat 96 x 64 image."""
    return all_images() + [saturated_noise(5, 96, 64), np.full((96, 64, 3), 77, np.uint8)]


@pytest.fixture(scope="module")
def pillow(imgs):
    """Pillow's bytes of every image for every case. Computed once, never changed."""
    return {c: tuple(pil_thumbnail(Image.fromarray(a), c[0], c[1]) for a in imgs) for c in CASES}


def _name(i):
    return ALL_SHAPES[i] if i < len(ALL_SHAPES) else ("noise", "flat")[i - len(ALL_SHAPES)]


@pytest.mark.parametrize("case", CASES, ids=["64_q80", "640_q30"])
def test_equals_pillow_and_the_per_image_call(engine, imgs, pillow, case):
    size, quality = case
    got = thumbnails_mixed(engine, imgs, size=size, quality=quality)
    assert len(got) == len(imgs) == 22
    for i, a in enumerate(imgs):
        assert got[i] == pillow[case][i], (_name(i), len(got[i]), len(pillow[case][i]))
        assert got[i] == thumbnails(engine, a[None], size, quality)[0], _name(i)
    assert got[20].count(b"\xff\x00") >= 5          # the noise image did exercise the byte stuffing


def test_bgr_order_and_permutation_and_one_image(engine, imgs, pillow):
    want = pillow[CASES[0]]
    assert thumbnails_mixed(engine, [np.ascontiguousarray(a[..., ::-1]) for a in imgs], size=64, order='bgr') == list(want)
    perm = [int(v) for v in np.random.default_rng(4).permutation(len(imgs))]
    assert thumbnails_mixed(engine, [imgs[i] for i in perm], size=64) == [want[i] for i in perm]
    for i in (0, 4, 15, 20):          # unchanged, reduced on both axes, the 2000 x 10 column, noise
        assert thumbnails_mixed(engine, [imgs[i]], size=64) == [want[i]]


@pytest.mark.parametrize("case", CASES, ids=["64_q80", "640_q30"])
def test_resident_images_at_odd_byte_offsets(engine, imgs, pillow, case):
    """The images in one allocation, each at an odd offset: sources that are encoded as they are included."""
    offs, at = [], 1
    for a in imgs:
        offs.append(at)
        at += a.nbytes + (2 if a.nbytes % 2 == 0 else 1)
    assert all(o % 2 == 1 for o in offs)
    buf = engine.dev_alloc(at)
    try:
        for a, o in zip(imgs, offs):
            engine.h2d(ctypes.c_void_p(buf.value + o), a)
        got = thumbnails_mixed(engine, ([buf.value + o for o in offs], [a.shape[:2] for a in imgs]), size=case[0], quality=case[1])
    finally:
        engine.dev_free(buf)
    assert got == list(pillow[case])


def test_several_chunks_give_the_same(engine):
    """A 1 MiB arena cuts the eleven images of tests/mixed_index_cases.py into chunks of 2, 3, 2, 2, 2 from the host and 5, 5, 1 resident
    (the figures are there): the bytes, and so the lengths, equal the default engine's."""
    from facet_amd import Engine
    arrs = chunk_images()
    want = thumbnails_mixed(engine, arrs, size=64)
    assert len(want) == len(arrs) and all(want)
    e = Engine(0, arena_bytes=CHUNK_ARENA)
    try:
        assert thumbnails_mixed(e, arrs, size=64) == want
        offs = np.concatenate([[0], np.cumsum([a.nbytes for a in arrs])])
        buf = e.dev_alloc(int(offs[-1]))
        try:
            for a, o in zip(arrs, offs):
                e.h2d(ctypes.c_void_p(buf.value + int(o)), a)
            assert thumbnails_mixed(e, ([buf.value + int(o) for o in offs[:-1]], [a.shape[:2] for a in arrs]), size=64) == want
        finally:
            e.dev_free(buf)
        assert thumbnails_mixed(e, arrs[:4], size=64) == want[:4]
    finally:
        e.close()


def test_capacity(engine, imgs, pillow):
    """One byte short of the largest thumbnail: the capacity error, minus the bytes needed for exactly the images that do not fit, every
    other row correct, and nothing stored behind a row's bytes or behind the last row."""
    want = pillow[CASES[0]]
    longest = max(len(b) for b in want)
    too_long = [i for i, b in enumerate(want) if len(b) == longest]
    cap = longest - 1
    plans = [thumbnail_plan(a.shape[1], a.shape[0], 64) for a in imgs]
    with pytest.raises(EngineCapacityError) as ei:
        engine.thumbnail_jpeg_mixed(imgs, plans, quality=80, cap=cap)
    assert ei.value.status == FE_ERR_CAPACITY and "more than" in str(ei.value)
    assert [i for i, l in enumerate(ei.value.lengths) if l < 0] == too_long
    assert all(ei.value.lengths[i] == -longest for i in too_long)
    assert [r for i, r in enumerate(ei.value.rows) if i not in too_long] == [b for i, b in enumerate(want) if i not in too_long]
    # the raw call into a buffer of 0xA5 with a guard band behind the last row
    n, guard = len(imgs), 4096
    ptrs, hw, _, dev, keep = engine._img_list(imgs)
    arr = engine.thumb_plans(plans, hw)
    out = np.full(n * cap + guard, 0xA5, np.uint8)
    lengths = np.zeros(n, np.int32)
    rc = engine.lib.fe_thumbnail_jpeg_mixed(engine.h, ptrs, hw.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, dev, 1, arr.ctypes.data_as(ctypes.c_void_p), 80,
                                            out.ctypes.data_as(ctypes.c_void_p), cap, lengths.ctypes.data_as(ctypes.c_void_p))
    assert rc == FE_ERR_CAPACITY
    assert (out[n * cap:] == 0xA5).all()
    for i in range(n):
        row = out[i * cap:(i + 1) * cap]
        used = int(lengths[i]) if lengths[i] > 0 else 0
        assert (i in too_long) == (used == 0)
        assert row[:used].tobytes() == (want[i] if used else b"") and (row[used:] == 0xA5).all(), _name(i)
    assert thumbnails_mixed(engine, imgs, size=64) == list(want)          # the context stays usable


def test_bad_arguments_name_the_image(engine, imgs):
    plans = [thumbnail_plan(a.shape[1], a.shape[0], 64) for a in imgs[:4]]
    with pytest.raises(EngineError, match=r"image 2\b") as ei:
        engine.thumbnail_jpeg_mixed((list(range(1, 5))[:2] + [None, 4], [a.shape[:2] for a in imgs[:4]]), plans)
    assert ei.value.status == FE_ERR_INVALID
    bad = list(plans)
    bad[2] = bad[2]._replace(reduce_box=(0, 0, 10 ** 6, 10), factors=(2, 2))          # a reduce box outside the image
    with pytest.raises(EngineError, match=r"image 2\b") as ei:
        engine.thumbnail_jpeg_mixed(imgs[:4], bad)
    assert ei.value.status == FE_ERR_INVALID
    with pytest.raises(EngineError, match=r"order 2\b"):
        engine.thumbnail_jpeg_mixed(imgs[:4], plans, order=2)
    with pytest.raises(EngineError, match=r"quality 0\b"):
        engine.thumbnail_jpeg_mixed(imgs[:4], plans, quality=0)
