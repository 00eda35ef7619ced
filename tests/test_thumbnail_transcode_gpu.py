"""GPU: stored JPEG thumbnails made smaller (fe_jpeg_thumbnail; the reference's export_viewer_db loops and _resize_thumbnail) against
Pillow byte for byte: `Image.open(f)`, `thumbnail((size, size), LANCZOS)`, `save(buf, "JPEG", quality=80)`. The sources are thumbnails
Pillow wrote; the sizes make draft() choose every scale, so the scale > 1 cases fail for any chain that decodes in full first."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from facet_amd import EngineError
from facet_amd.thumbnail import (downsize_thumbnails, draft_scale, pillow_resize_thumbnail, resize_thumbnail, resize_thumbnails,
                                 thumbnail_plan_jpeg)

pytestmark = pytest.mark.gpu

SOURCES = [(160, 107), (107, 160), (640, 427), (333, 500)]      # (w, h)
SIZES = [20, 40, 50, 64, 100, 320]


def photo(w, h, seed):
    """Smooth colour fields with hard edges and some noise: what a photo's thumbnail holds, and nothing a quality-80 file flattens."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.stack([127 + 120 * np.sin(x / (7 + 3 * k) + seed + k) * np.cos(y / (11 - 2 * k)) for k in range(3)], -1)
    a[h // 5:h // 2, w // 4:w // 2] = (250, 20, 90)
    a += rng.normal(0, 12, a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def stored(w, h, seed=0, **kw):
    buf = io.BytesIO()
    Image.fromarray(photo(w, h, seed)).save(buf, format="JPEG", quality=80, **kw)
    return buf.getvalue()


@pytest.fixture(scope="module")
def sources():
    return {(w, h): [stored(w, h, s) for s in range(3)] for (w, h) in SOURCES}


def test_every_scale_occurs():
    assert {draft_scale(w, h, s) for (w, h) in SOURCES for s in SIZES} == {1, 2, 4, 8}


@pytest.mark.parametrize("size", SIZES)
def test_resize_thumbnails_equals_pillow_byte_for_byte(engine, sources, size):
    for (w, h), blobs in sources.items():
        got = resize_thumbnails(engine, blobs, size)
        want = [pillow_resize_thumbnail(b, size) for b in blobs]
        assert got == want, (w, h, size, draft_scale(w, h, size))


def test_the_device_did_the_work(engine, sources):
    """The raw call on files of every scale: status 0 and Pillow's bytes, so resize_thumbnails above did not get them from its fallback."""
    for (w, h), blobs in sources.items():
        for size in (20, 50, 100):
            scale, plan = thumbnail_plan_jpeg(w, h, size)
            rows, status = engine.jpeg_thumbnail(blobs, scale, plan)
            assert not status.any() and rows == [pillow_resize_thumbnail(b, size) for b in blobs], (w, h, size)


def test_mixed_source_sizes_keep_their_order(engine, sources):
    blobs = [sources[s][k] for k in range(3) for s in SOURCES]
    want = [pillow_resize_thumbnail(b, 50) for b in blobs]
    assert resize_thumbnails(engine, blobs, 50) == want
    rows = [(i, b) for i, b in enumerate(blobs)] + [("none", None), ("junk", b"junk")]
    got = list(downsize_thumbnails(engine, rows, thumbnail_size=120))
    keep = [i for i, b in enumerate(blobs) if max(Image.open(io.BytesIO(b)).size) > 120]
    assert [k for _, k in got] == keep and [b for b, _ in got] == [pillow_resize_thumbnail(blobs[i], 120) for i in keep]
    small = sources[(160, 107)][0]
    assert resize_thumbnail(engine, small, 160) is small
    assert resize_thumbnail(engine, small, 64) == pillow_resize_thumbnail(small, 64)


def test_grayscale_cmyk_progressive_and_corrupt_files_come_back_with_pillows_bytes(engine, sources):
    rgb = photo(160, 107, 5)
    gray, cmyk = io.BytesIO(), io.BytesIO()
    Image.fromarray(rgb[..., 1]).save(gray, format="JPEG", quality=80)
    Image.fromarray(rgb).convert("CMYK").save(cmyk, format="JPEG", quality=80)
    good = sources[(160, 107)][1]
    cut = good[:len(good) * 2 // 3] + b"\xff\xd9"
    blobs = [good, gray.getvalue(), cmyk.getvalue(), stored(160, 107, 6, progressive=True), b"junk", stored(160, 107, 7, comment=b"kept"), cut]
    for size in (20, 50):
        for prog in (False, True):
            got = resize_thumbnails(engine, blobs, size, progressive=prog)
            for k, b in enumerate(blobs):
                try:
                    want = pillow_resize_thumbnail(b, size)
                except Exception:
                    want = None
                assert got[k] == want, (size, prog, k)
            assert got[4] is None and Image.open(io.BytesIO(got[1])).mode == "L"
    # the raw call reports what it did not take and leaves those rows empty, between two files it did
    scale, plan = thumbnail_plan_jpeg(160, 107, 40)
    rows, status = engine.jpeg_thumbnail([gray.getvalue(), good, cut, cmyk.getvalue(), good], scale, plan)
    assert status[1] == 0 and status[4] == 0 and status[2] < 0 and status[3] == 4
    assert rows[2] == b"" and rows[3] == b"" and rows[1] == rows[4] == pillow_resize_thumbnail(good, 40)


def test_a_row_too_small_for_its_output_gives_capacity(engine, sources):
    blobs = sources[(160, 107)][:2]
    scale, plan = thumbnail_plan_jpeg(160, 107, 64)
    want = [pillow_resize_thumbnail(b, 64) for b in blobs]
    cap = max(len(x) for x in want) - 1
    n, guard = len(blobs), 64
    buf = np.full((n * cap + guard,), 0xA5, np.uint8)
    lengths, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ptrs, lens = (C.c_char_p * n)(*blobs), (C.c_size_t * n)(*[len(b) for b in blobs])
    (ow, oh), (fx, fy) = plan.size, plan.factors
    rbox = np.asarray(plan.reduce_box if plan.reduce_box is not None else (0, 0, 0, 0), np.int32)
    box = np.asarray(plan.resize_box, np.float32)
    rc = engine.lib.fe_jpeg_thumbnail(engine.h, ptrs, lens, n, plan.src_h, plan.src_w, scale, 0, oh, ow, fx, fy, rbox.ctypes.data_as(C.c_void_p),
                                      box.ctypes.data_as(C.c_void_p), 0, 80, buf.ctypes.data_as(C.c_void_p), cap,
                                      lengths.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
    assert rc == -4 and b"more than" in engine.lib.fe_last_error(engine.h)           # FE_ERR_CAPACITY, as fe_thumbnail_jpeg
    assert not status.any() and np.all(buf[n * cap:] == 0xA5)
    for k in range(n):
        if len(want[k]) > cap:
            assert int(lengths[k]) == -len(want[k]) and np.all(buf[k * cap:(k + 1) * cap] == 0xA5)
        else:
            assert buf[k * cap:k * cap + int(lengths[k])].tobytes() == want[k]
    with pytest.raises(EngineError, match="more than"):
        engine.jpeg_thumbnail(blobs, scale, plan, cap=cap)
    assert engine.jpeg_thumbnail(blobs, scale, plan, cap=cap + 1)[0] == want          # exactly enough; the context is still usable
