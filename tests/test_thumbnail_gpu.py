"""GPU: fe_reduce_u8 / fe_resize_u8_box / fe_jpeg_encode / fe_thumbnail_jpeg against Pillow itself (live) and against
tests/golden/thumbnail_golden.npz (the reference's own generate_photo_thumbnail, tests/golden/make_thumbnail_golden.py).
Every assertion is byte or pixel equality. If the live Pillow and the golden ever disagree, this Pillow build writes other bytes
than the one the golden was made with: test_thumbnail_host.py::test_golden_reproduces_from_its_generator says so first."""
import ctypes as C
import hashlib
import io
import os

import numpy as np
import pytest
from PIL import Image

from facet_amd import EngineError
from facet_amd.thumbnail import generate_photo_thumbnail, thumbnail_plan, thumbnails
from test_phash_host import GOLDEN, synth_image
from test_thumbnail_host import gold_gen, pil_thumbnail

pytestmark = pytest.mark.gpu


def pil_jpeg(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def saturated_noise(seed, h, w):
    """Noise with a white and a black band: rounding at both ends of the range."""
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[: h // 5] = 255
    a[h // 5: 2 * h // 5, ::3] = 0
    return a


# ---- reduce ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(29, 31), (64, 48)])
def test_reduce_equals_pillow(engine, h, w):
    img = saturated_noise(h * 100 + w, h, w)
    pil = Image.fromarray(img)
    for f in [(2, 2), (3, 3), (4, 4), (5, 5), (2, 3), (1, 4), (6, 1), (7, 7)]:
        for box in [(0, 0, w, h), (3, 2, w - 4, h - 1)]:
            want = np.asarray(pil.reduce(f, box))
            got = engine.reduce_u8(img[None], f, box)[0]
            assert got.shape == want.shape and np.array_equal(got, want), f"factor {f} box {box}: max diff {np.abs(got.astype(int) - want).max()}"
    assert np.array_equal(engine.reduce_u8(np.stack([img, img[::-1]]), 3)[1], np.asarray(Image.fromarray(img[::-1]).reduce(3)))      # batch, int factor


# ---- boxed resize ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,out,box", [
    ((234, 334), (112, 160), (0.0, 0.0, 1000 / 3, 700 / 3)),      # the plan of 1000 x 700 at size 160
    ((100, 120), (40, 50), (10.25, 3.5, 110.75, 97.125)),         # inset on every side
    ((64, 48), (64, 20), (0.0, 0.0, 47.5, 64.0)),                 # horizontal pass only
    ((64, 48), (90, 48), (0.0, 1.5, 48.0, 60.0)),                 # vertical pass only, enlarging
    ((37, 41), (37, 41), (0.5, 0.25, 40.5, 36.75)),               # same size, shifted box: both passes run
])
def test_resize_box_equals_pillow(engine, shape, out, box):
    imgs = np.stack([saturated_noise(7, *shape), synth_image(8, *shape)])
    got = engine.resize_u8_box(imgs, out[0], out[1], box)
    for i in range(2):
        want = np.asarray(Image.fromarray(imgs[i]).resize((out[1], out[0]), Image.LANCZOS, box))
        assert np.array_equal(got[i], want), f"{shape} -> {out} box {box}: max diff {np.abs(got[i].astype(int) - want).max()}"


def test_plain_resize_is_unchanged(engine):
    img = saturated_noise(9, 333, 517)
    for filt, pf in (("lanczos", Image.LANCZOS), ("bicubic", Image.BICUBIC)):
        want = np.asarray(Image.fromarray(img).resize((347, 224), pf))
        assert np.array_equal(engine.resize_u8(img[None], 224, 347, filt)[0], want)
        assert np.array_equal(engine.resize_u8_box(img[None], 224, 347, (0, 0, 517, 333), filt)[0], want)


# ---- encoder alone --------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (8, 8), (16, 16), (8, 17), (17, 8), (53, 37), (33, 48), (112, 160)]      # (h, w)


def contents(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    grad = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 3 % 256], -1).astype(np.uint8)
    if h > 4 and w > 4:
        grad[h // 3: h // 2, w // 4: w // 2] = (250, 10, 30)      # hard edges inside the gradient
    sparse = np.zeros((h, w, 3), np.uint8)
    sparse[3::16, 5::16] = 255                                     # one bright pixel per 16 x 16 tile: long zero runs, ZRL
    return {"constant": np.full((h, w, 3), (90, 160, 33), np.uint8), "gradient": grad,
            "noise": np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8), "sparse": sparse}


@pytest.mark.parametrize("h,w", SIZES)
def test_jpeg_equals_pillow(engine, h, w):
    for name, rgb in contents(h, w).items():
        for q in (80, 85, 30, 100, 1):
            want = pil_jpeg(rgb, q)
            got = engine.jpeg_encode(rgb[None], quality=q)[0]
            assert got == want, f"{name} {h}x{w} q{q}: {len(got)} bytes against {len(want)}"
        assert engine.jpeg_encode(np.ascontiguousarray(rgb[None, ..., ::-1]), quality=80, bgr=True)[0] == pil_jpeg(rgb, 80), name


def test_jpeg_header_and_stuffing(engine):
    rgb = contents(112, 160)["noise"]
    data = engine.jpeg_encode(rgb[None], quality=100)[0]
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9" and data[621:623] == b"?\x00"      # the 623-byte header ends with SOS's Se, Ah/Al
    scan = data[623:-2]
    assert scan.count(b"\xff\x00") > 0 and scan.count(b"\xff") == scan.count(b"\xff\x00")          # natural 0xFF bytes, every one stuffed
    assert data == pil_jpeg(rgb, 100)


def test_jpeg_batch_equals_single_calls(engine):
    c = contents(53, 37)
    batch = np.stack([c["noise"], c["gradient"], c["sparse"]])
    got = engine.jpeg_encode(batch, quality=80)
    assert got == [engine.jpeg_encode(batch[i:i + 1], quality=80)[0] for i in range(3)] == [pil_jpeg(batch[i], 80) for i in range(3)]
    d = engine.dev_alloc(batch.nbytes)
    try:
        engine.h2d(d, batch)
        assert engine.jpeg_encode((d, 3, 53, 37), quality=80) == got
    finally:
        engine.dev_free(d)


# ---- whole path -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "thumbnail_golden.npz"))


def test_thumbnail_equals_golden_and_pillow(engine, gold):
    for i, name in enumerate(gold["names"].tolist()):
        seed, h, w, size, quality, stored = (int(v) for v in gold["meta"][i])
        rgb = gold_gen.make_image(str(gold["kinds"][i]), seed, h, w)
        assert hashlib.sha1(rgb.tobytes()).hexdigest() == str(gold["input_sha1"][i]), f"{name}: the seeded generator gives other pixels than at golden time"
        got = thumbnails(engine, rgb[None], size=size, quality=quality)[0]
        live = pil_thumbnail(Image.fromarray(rgb), size, quality)
        print(f"[thumbnail] {name}: {len(got)} bytes, golden {int(gold['lengths'][i])}, live Pillow {len(live)}")
        assert len(got) == int(gold["lengths"][i]) and hashlib.sha256(got).hexdigest() == str(gold["sha256"][i]), name
        if stored:
            assert got == gold["jpeg_" + name].tobytes(), name
        assert got == live, name
        assert thumbnails(engine, np.ascontiguousarray(rgb[None, ..., ::-1]), size=size, quality=quality, bgr=True)[0] == got, name
        if h <= 300:
            assert generate_photo_thumbnail(engine, Image.fromarray(rgb), size=size, quality=quality) == got


@pytest.mark.parametrize("w,h,size", [(10, 2000, 640), (8, 4000, 300), (997, 13, 64), (200, 3000, 64)])
def test_thumbnail_of_strips(engine, w, h, size):
    """More than 100 times taller than wide (Image.resize runs the rows first), with and without a reduce; factors that differ per axis."""
    rgb = saturated_noise(w + h, h, w)
    assert thumbnails(engine, np.stack([rgb, rgb[::-1]]), size=size) == [pil_thumbnail(Image.fromarray(a), size) for a in (rgb, rgb[::-1])]


# ---- capacity -------------------------------------------------------------------------------------------------------------------
def test_small_capacity_is_an_error_and_writes_nothing_past_it(engine):
    rgb = contents(53, 37)["noise"]
    batch = np.ascontiguousarray(np.stack([rgb, contents(53, 37)["constant"]]))
    want = [pil_jpeg(batch[0], 80), pil_jpeg(batch[1], 80)]
    assert len(want[1]) < 700 < len(want[0]) <= engine.jpeg_bound(53, 37)
    for cap in (len(want[0]) - 1, 700, 623, 100):
        guard = 64
        buf = np.full((2 * cap + guard,), 0xA5, np.uint8)
        lengths = np.zeros(2, np.int32)
        rc = engine.lib.fe_jpeg_encode(engine.h, batch.ctypes.data_as(C.c_void_p), 2, 53, 37, 0, 0, 80, buf.ctypes.data_as(C.c_void_p), cap,
                                       lengths.ctypes.data_as(C.c_void_p))
        assert rc != 0 and b"more than" in engine.lib.fe_last_error(engine.h)
        assert int(lengths[0]) == -len(want[0])                                   # what it would have taken
        assert np.all(buf[:cap] == 0xA5) and np.all(buf[2 * cap:] == 0xA5)        # the row that does not fit and the guard are untouched
        if cap >= len(want[1]):
            assert int(lengths[1]) == len(want[1]) and buf[cap:cap + len(want[1])].tobytes() == want[1]
    with pytest.raises(EngineError, match="more than"):
        engine.jpeg_encode(batch, quality=80, cap=700)
    assert engine.jpeg_encode(batch, quality=80, cap=len(want[0])) == want       # exactly enough; the context is still usable


# ---- BatchScorer ----------------------------------------------------------------------------------------------------------------
def test_batch_scorer_thumbnail_column():
    """BatchScorer(thumbnails=True): 'thumbnail' equals the reference's function on the same pixels, every other key and value equals the
    thumbnails=False result, with and without a second context; the key is absent when the flag is off."""
    from facet_amd import Engine
    from facet_amd._lib import FE_MODEL_TOPIQ
    from facet_amd.batch import BatchScorer
    from facet_amd.weights import synthetic_state_dict
    imgs = np.stack([synth_image(31, 150, 210), synth_image(32, 150, 210)])
    e, e2 = Engine(0, arena_bytes=4 << 30), Engine(0, arena_bytes=2 << 30)
    try:
        e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 4))
        for aux in (None, e2):
            off = BatchScorer(e, aux_engine=aux).process_batch(imgs)
            on = BatchScorer(e, aux_engine=aux, thumbnails=True, thumbnail_size=96).process_batch(imgs)
            for i, (a, b) in enumerate(zip(off, on)):
                assert 'thumbnail' not in a and set(b) == set(a) | {'thumbnail'}
                assert isinstance(b['thumbnail'], bytes) and b['thumbnail'] == pil_thumbnail(Image.fromarray(imgs[i]), 96, 80)
                for k, v in a.items():
                    assert type(b[k]) is type(v) and (b[k] == v or (isinstance(v, float) and np.isnan(v) and np.isnan(b[k]))), k
        default = BatchScorer(e, thumbnails=True, phash=True).process_batch(imgs)      # 640: already small enough, encoded as it is
        assert [r['thumbnail'] for r in default] == [pil_jpeg(imgs[i], 80) for i in range(2)] and all('phash' in r for r in default)
        mixed = BatchScorer(e, thumbnails=True, thumbnail_size=96, thumbnail_quality=30).process_images([imgs[1], synth_image(33, 97, 131)])
        assert [r['thumbnail'] for r in mixed] == [pil_thumbnail(Image.fromarray(a), 96, 30) for a in (imgs[1], synth_image(33, 97, 131))]
    finally:
        e.close()
        e2.close()
