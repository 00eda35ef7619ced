"""CPU: thumbnail_plan_jpeg against Pillow itself. For every shape and size of the grid the scale draft() chooses, the drafted size and
the final size equal what `Image.open(blob)` + `im.thumbnail((size, size), LANCZOS)` report, and carrying the plan out with Pillow's own
primitives (draft to the plan's scale, reduce with the plan's box, resize with the plan's box) gives that thumbnail's pixels. Plus the
host side of resize_thumbnail / downsize_thumbnails on the Pillow fallback. Every equality is exact."""
import functools
import io

import numpy as np
import pytest
from PIL import Image

from facet_amd.thumbnail import downsize_thumbnails, pillow_resize_thumbnail, resize_thumbnail, resize_thumbnails, thumbnail_plan, thumbnail_plan_jpeg

DIMS = [1, 2, 7, 8, 9, 16, 17, 33, 100, 427, 640, 641, 1999, 4000, 6000]
SIZES = [1, 16, 40, 64, 100, 160, 320, 640]
_TILE = np.random.default_rng(7).integers(0, 256, (64, 64, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=4)
def blob_of(w, h):
    """A small encoded file of that shape: tiled noise, so that every stage has something to get wrong."""
    a = np.tile(_TILE, (-(-h // 64), -(-w // 64), 1))[:h, :w]
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=50)
    return buf.getvalue()


def drafted(blob, scale):
    """The file opened and set to decode at 1/scale, as JpegImageFile.draft() sets it."""
    im = Image.open(io.BytesIO(blob))
    if scale != 1:
        w, h = im.size
        im._size = (-(-w // scale), -(-h // scale))
        im.tile = [im.tile[0]._replace(extents=(0, 0) + im.size)]
        im.decoderconfig = (scale, 0)
    return im


def carry_out(blob, scale, plan):
    im = drafted(blob, scale)
    assert im.size == (plan.src_w, plan.src_h)
    im.load()
    if plan.unchanged:
        return im
    if plan.factors != (1, 1):
        im = im.reduce(plan.factors, box=plan.reduce_box)
    return im.resize(plan.size, Image.LANCZOS, box=plan.resize_box)      # no reducing_gap: the plan has done that part


@pytest.mark.parametrize("w", DIMS)
def test_plan_equals_pillow_on_the_grid(w):
    seen_scales = set()
    for h in DIMS:
        blob = blob_of(w, h)
        for size in SIZES:
            scale, plan = thumbnail_plan_jpeg(w, h, size)
            im = Image.open(io.BytesIO(blob))
            im.thumbnail((size, size), Image.LANCZOS)
            want_scale = im.decoderconfig[0] if im.decoderconfig else 1
            assert scale == want_scale, (w, h, size)
            assert plan.size == im.size, (w, h, size)
            probe = Image.open(io.BytesIO(blob))
            if im.decoderconfig:      # thumbnail() drafted: the size draft() leaves
                probe.draft(None, (int(size * 2.0), int(size * 2.0)))
            assert (plan.src_w, plan.src_h) == probe.size, (w, h, size)
            got = carry_out(blob, scale, plan)
            assert got.size == im.size and got.mode == im.mode
            assert np.array_equal(np.asarray(got), np.asarray(im)), (w, h, size, scale, plan)
            seen_scales.add(scale)
    if w >= 640:
        assert seen_scales == {1, 2, 4, 8}


def test_draft_changes_the_pixels():
    """The table of the issue: at 640 x 427 the drafted thumbnails of size 100 and 40 differ from full decode + thumbnail, and those of
    320 and 160 (scale 1) do not. So the grid test can tell a plan without draft() from one with it."""
    blob = blob_of(640, 427)
    full = Image.fromarray(np.asarray(Image.open(io.BytesIO(blob))))          # the same pixels, but not from a JPEG file: no draft
    for size, want_scale in ((100, 2), (40, 4), (320, 1), (160, 1)):
        scale, plan = thumbnail_plan_jpeg(640, 427, size)
        assert scale == want_scale
        a = full.copy()
        a.thumbnail((size, size), Image.LANCZOS)
        b = carry_out(blob, scale, plan)
        assert a.size == b.size
        assert np.array_equal(np.asarray(a), np.asarray(b)) == (scale == 1), size
    assert thumbnail_plan_jpeg(640, 427, 100)[1].resize_box == (0.0, 0.0, 320.0, 213.5)
    assert thumbnail_plan_jpeg(640, 427, 40)[1].resize_box[2:] != (160.0, 106.75)      # reduced first: the box is in reduced pixels


def test_thumbnail_plan_is_unchanged():
    """thumbnail_plan keeps its results: spot values from before thumbnail_plan_jpeg shared its code."""
    p = thumbnail_plan(6000, 4000, 640)
    assert (p.size, p.factors, p.reduce_box, p.unchanged, p.tall) == ((640, 427), (4, 4), (0, 0, 6000, 4000), False, False)
    assert p.resize_box == (0.0, 0.0, 1500.0, 1000.0)
    p = thumbnail_plan(640, 427, 320)
    assert (p.size, p.factors, p.reduce_box, p.resize_box) == ((320, 214), (1, 1), None, (0.0, 0.0, 640.0, 427.0))
    assert thumbnail_plan(300, 200, 640).unchanged


# ---- resize_thumbnail / downsize_thumbnails on the fallback path ----------------------------------------------------------------------
class _FallbackEngine:
    """Reports every file unsupported, so everything must come from the Pillow recipe."""
    def jpeg_probe(self, blob, progressive=False):
        return dict(width=0, height=0, components=0, hsamp=1, vsamp=1, restart_interval=0, orientation=1, status=-1)

    def jpeg_thumbnail(self, *a, **k):
        raise AssertionError("nothing is decodable for this engine")


def test_resize_thumbnail_returns_the_same_object_when_it_fits():
    blob = blob_of(100, 33)
    eng = _FallbackEngine()
    assert resize_thumbnail(eng, blob, 100) is blob
    assert resize_thumbnail(eng, blob, 640) is blob
    got = resize_thumbnail(eng, blob, 99)
    assert got == pillow_resize_thumbnail(blob, 99) and Image.open(io.BytesIO(got)).size == (99, 33)
    with pytest.raises(Exception):
        resize_thumbnail(eng, b"not an image", 50)


def test_resize_thumbnails_keeps_order_and_gives_none_for_corrupt_files():
    blobs = [blob_of(640, 427), b"junk", blob_of(100, 33), blob_of(640, 427)[:300]]
    got = resize_thumbnails(_FallbackEngine(), blobs, 64)
    assert got[1] is None and got[3] is None
    assert got[0] == pillow_resize_thumbnail(blobs[0], 64) and got[2] == pillow_resize_thumbnail(blobs[2], 64)


def test_downsize_thumbnails_skips_small_and_corrupt_rows():
    rows = [("a", blob_of(640, 427)), ("b", blob_of(100, 33)), ("c", b"junk"), ("d", None), ("e", blob_of(640, 427)[:300]), (6, blob_of(427, 640))]
    got = list(downsize_thumbnails(_FallbackEngine(), rows, thumbnail_size=320))
    assert [k for _, k in got] == ["a", 6]
    assert got[0][0] == pillow_resize_thumbnail(rows[0][1], 320) and got[1][0] == pillow_resize_thumbnail(rows[5][1], 320)
    assert list(downsize_thumbnails(_FallbackEngine(), rows, thumbnail_size=640)) == []
