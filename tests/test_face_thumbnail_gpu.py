"""GPU: fe_face_thumbnails against the host FaceAnalyzer._crop_face_thumbnail on the same arrays - byte for byte, no tolerance.

Two BGR images of 320 x 256 (w x h) in one batch: the left half seeded noise (long codes, 0xFF stuffing), the right half a smooth
gradient with a saturated patch (EOB / ZRL runs, all-zero AC blocks). Boxes are given directly; CASES lists, for each, the plan it has
to produce, so what the cases cover is checked and not assumed. The fused (LDS) encoder takes outputs up to 128 x 128
(FE_FACE_THUMB_FUSED_SIDE); thumbnail_size 160 goes through the same kernel over arena scratch and has to give the oracle's bytes too."""
import ctypes as C

import numpy as np
import pytest

from facet_amd._lib import EngineCapacityError, EngineError, FE_ERR_CAPACITY
from facet_amd.face import FaceAnalyzer, face_thumbnail_plan, face_thumbnails

pytestmark = pytest.mark.gpu

H, W = 256, 320
FUSED_SIDE = 128      # include/facet_engine.h FE_FACE_THUMB_FUSED_SIDE


def make_images():
    rng = np.random.default_rng(31)
    imgs = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W // 2]
    for i in range(2):
        g = np.stack([(xx + yy // 2 + 40 * i) % 256, (2 * yy // 3 + 30) % 256, (255 - xx - 20 * i) % 256], axis=-1).astype(np.uint8)
        g[60:140, 50:130] = 255
        imgs[i, :, W // 2:] = g
    return imgs


# (box, padding, plan at thumbnail_size 128)
CASES = [
    ((100, 100, 130, 130), 0.3, (91, 91, 139, 139, 128, 128)),       # 30 px face: 48 px crop, upscaled by the one-tap path
    ((10, 10, 138, 138), 0.0, (10, 10, 138, 138, 128, 128)),         # exactly 128 x 128: both passes are the identity
    ((170, 20, 298, 117), 0.0, (170, 20, 298, 117, 128, 97)),        # 128 x 97: one pass is
    ((20, 100, 149, 228), 0.0, (20, 100, 149, 228, 128, 127)),       # 129 x 128: scale just above 1
    ((30, 40, 281, 239), 0.0, (30, 40, 281, 239, 128, 101)),         # 251 x 199: non-integer downscale, sides no multiple of 8
    ((0, 0, 320, 256), 0.0, (0, 0, 320, 256, 128, 102)),             # the whole image, across both kinds of content
    ((-20, 100, 40, 160), 0.3, (0, 82, 58, 178, 77, 128)),           # clipped left
    ((100, -30, 170, 50), 0.3, (79, 0, 191, 74, 128, 84)),           # top
    ((280, 90, 340, 170), 0.3, (262, 66, 320, 194, 58, 128)),        # right
    ((120, 200, 200, 290), 0.3, (96, 173, 224, 256, 128, 83)),       # bottom
    ((60, 120, 260, 128), 0.0, (60, 120, 260, 128, 128, 5)),         # thin: one partial MCU row
    ((60, 50, 260, 52), 0.0, (60, 50, 260, 52, 128, 1)),             # thin: a single output row
    ((150, 3, 153, 250), 0.0, (150, 3, 153, 250, 1, 128)),           # and a single output column
    ((400, 300, 450, 350), 0.3, None),                               # outside the image: no thumbnail
]


def oracle(img, box, padding, size, quality):
    fa = object.__new__(FaceAnalyzer)
    fa.thumbnail_size, fa.thumbnail_quality = size, quality
    return fa._crop_face_thumbnail(img, np.asarray(box), padding)


@pytest.fixture(scope="module")
def imgs():
    return make_images()


@pytest.fixture(scope="module")
def resident(engine, imgs):
    d = engine.dev_alloc(imgs.nbytes)
    engine.h2d(d, imgs)
    yield (d, 2, H, W)
    engine.dev_free(d)


def planned(size):
    """Every case on both images, interleaved in img_index; cases without a plan left out. -> (img, box, padding, plan) rows"""
    rows = []
    for k, (box, padding, _) in enumerate(CASES):
        plan = face_thumbnail_plan(box, H, W, size, padding)
        if plan is not None:
            rows += [(k % 2, box, padding, plan), (1 - k % 2, box, padding, plan)]
    return rows


def test_cases_cover_what_they_claim():
    for box, padding, want in CASES:
        assert face_thumbnail_plan(box, H, W, 128, padding) == want, box


@pytest.mark.parametrize("size,quality", [(128, 85), (128, 50), (128, 95), (64, 85), (160, 85)])
def test_bytes_equal_host_path(engine, imgs, resident, size, quality):
    assert size <= FUSED_SIDE or size == 160      # 160: above the fused encoder's limit
    rows = planned(size)
    # at 64 the two crops whose short output side is 1 at 128 scale to a side of 0: no plan, and no thumbnail on the host either
    dropped = [(box, padding) for box, padding, _ in CASES if face_thumbnail_plan(box, H, W, size, padding) is None]
    assert len(dropped) == (3 if size == 64 else 1) and len(rows) == 2 * (len(CASES) - len(dropped))
    assert all(oracle(imgs[i], box, padding, size, quality) is None for box, padding in dropped for i in range(2))
    idx, crops, sizes = [r[0] for r in rows], [r[3][:4] for r in rows], [r[3][4:] for r in rows]
    want = [oracle(imgs[i], box, padding, size, quality) for i, box, padding, _ in rows]
    assert all(w is not None and w[:2] == b"\xff\xd8" for w in want)
    got = engine.face_thumbnails(resident, idx, crops, sizes, quality)
    bad = [(k, rows[k][1], len(g), len(w)) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad
    assert engine.face_thumbnails(imgs, idx, crops, sizes, quality) == want      # host-array input: the same bytes


def test_direct_call_none_plans_and_empty(engine, imgs, resident):
    boxes = [[c[0] for c in CASES if c[1] == 0.3], [CASES[-1][0], CASES[0][0], CASES[-1][0]]]
    got = face_thumbnails(engine, resident, boxes, 128, 85)
    want = [[oracle(imgs[i], b, 0.3, 128, 85) for b in boxes[i]] for i in range(2)]
    assert got == want
    assert got[0][-1] is None and got[1][0] is None and got[1][2] is None and got[1][1] is not None
    assert face_thumbnails(engine, imgs, boxes, 128, 85) == want
    assert face_thumbnails(engine, resident, [[], []]) == [[], []]                       # m == 0
    assert face_thumbnails(engine, resident, [[CASES[-1][0]], []]) == [[None], []]       # nothing but faces without a plan
    assert engine.face_thumbnails(resident, [], np.zeros((0, 4)), np.zeros((0, 2))) == []
    lib = engine.lib
    assert lib.fe_face_thumbnails(engine.h, resident[0], 2, H, W, 1, 0, None, None, None, 85, None, 0, None) == 0


def test_bad_arguments_are_refused(engine, resident):
    for idx, crop, size in (([2], (0, 0, 10, 10), (8, 8)), ([0], (0, 0, W + 1, 10), (8, 8)), ([0], (5, 5, 5, 10), (8, 8)),
                            ([0], (0, 0, 10, 10), (0, 8)), ([0], (-1, 0, 10, 10), (8, 8)), ([0], (0, 0, 10, 10), (8, 9000))):
        with pytest.raises(EngineError) as err:
            engine.face_thumbnails(resident, idx, [crop], [size])
        assert not isinstance(err.value, EngineCapacityError)
    with pytest.raises(EngineError):
        engine.face_thumbnails(resident, [0], [(0, 0, 10, 10)], [(8, 8)], quality=0)
    assert len(engine.face_thumbnails(resident, [0], [(0, 0, 10, 10)], [(8, 8)])[0]) > 600      # the context stays usable


def test_capacity_one_byte_short(engine, imgs, resident):
    rows = planned(128)[:12]
    m = len(rows)
    idx = np.asarray([r[0] for r in rows], np.int32)
    crops = np.asarray([r[3][:4] for r in rows], np.int32)
    sizes = np.asarray([r[3][4:] for r in rows], np.int32)
    want = engine.face_thumbnails(resident, idx, crops, sizes, 85)
    lens = [len(b) for b in want]
    k = int(np.argmax(lens))
    cap = lens[k] - 1                                   # one byte short for face k
    assert all(n <= cap for j, n in enumerate(lens) if j != k) and sum(n == lens[k] for n in lens) == 1
    with pytest.raises(EngineCapacityError):
        engine.face_thumbnails(resident, idx, crops, sizes, 85, cap=cap)
    tail = 64
    out = np.full(m * cap + tail, 0xA5, np.uint8)
    lengths = np.zeros(m, np.int32)
    rc = engine.lib.fe_face_thumbnails(engine.h, resident[0], 2, H, W, 1, m, idx.ctypes.data_as(C.c_void_p), crops.ctypes.data_as(C.c_void_p),
                                       sizes.ctypes.data_as(C.c_void_p), 85, out.ctypes.data_as(C.c_void_p), cap, lengths.ctypes.data_as(C.c_void_p))
    assert rc == FE_ERR_CAPACITY
    assert lengths[k] == -lens[k]
    for j in range(m):
        row = out[j * cap:(j + 1) * cap]
        if j == k:
            assert (row == 0xA5).all()                  # its row is left alone
        else:
            assert lengths[j] == lens[j] and row[:lens[j]].tobytes() == want[j]
            assert (row[lens[j]:] == 0xA5).all()        # nothing behind a face's bytes
    assert (out[m * cap:] == 0xA5).all()                # nor past the last row
    assert engine.face_thumbnails(resident, idx, crops, sizes, 85) == want


def deep_equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(deep_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(deep_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


@pytest.fixture(scope="module")
def models():
    from standins import synthetic_onnx as S      # the stand-in graphs of test_face_gpu.py
    det, _ = S.scrfd_like(seed=12, size=320)
    lmk, _ = S.landmark_like(seed=13)
    rec, _ = S.arcface_iresnet(layers=(1, 1, 1, 1), seed=14)
    return {"det": det, "lmk": lmk, "rec": rec}


def make_analyzer(engine, models, gpu):
    fa = FaceAnalyzer(min_confidence=0.55, min_face_size=10, engine=engine, models=models, gpu_thumbnails=gpu)
    assert fa.available and fa.gpu_thumbnails == gpu
    fa.face_app.det_size, fa.face_app.max_candidates, fa.face_app.max_faces = (320, 320), 4096, 256
    return fa


def test_analyzer_option_gives_the_same_dicts(engine, models):
    photos = np.random.default_rng(10).integers(0, 256, (2, 320, 320, 3), dtype=np.uint8)      # test_face_gpu.py finds faces on these
    fa = make_analyzer(engine, models, False)
    want = fa.analyze_faces_batch(list(photos))
    details = [d for r in want for d in r["face_details"]]
    assert all(r["face_count"] > 0 for r in want) and details and all(d["thumbnail"][:2] == b"\xff\xd8" for d in details)
    fa.gpu_thumbnails = True
    assert deep_equal(fa.analyze_faces_batch(list(photos)), want)
    d = engine.dev_alloc(photos.nbytes)
    try:
        engine.h2d(d, photos)
        assert deep_equal(fa.analyze_faces_batch(None, resident=(d, 2, 320, 320)), want)      # no host pixels at all
    finally:
        engine.dev_free(d)
    single = fa.analyze_faces(photos[1])      # the single-image call keeps the host path
    assert [f["thumbnail"] for f in single["face_details"]] == [f["thumbnail"] for f in want[1]["face_details"]]
    fa.face_app.unload()


def test_process_files_same_records_without_the_download(models):
    import io
    from PIL import Image
    from facet_amd import Engine
    from facet_amd.batch import BatchScorer
    from facet_amd._lib import FE_MODEL_TOPIQ
    from facet_amd.weights import synthetic_state_dict
    engine = Engine(0, arena_bytes=2 << 30)      # its own context: the session's carries no models
    try:
        engine.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
        photos = np.random.default_rng(10).integers(0, 256, (4, 320, 320, 3), dtype=np.uint8)
        blobs = []
        for p in photos:
            buf = io.BytesIO()
            Image.fromarray(p).save(buf, "JPEG", quality=95, subsampling=0)
            blobs.append(buf.getvalue())
        sizes = []
        d2h = engine.d2h
        engine.d2h = lambda arr, dptr: (sizes.append(arr.nbytes), d2h(arr, dptr))[1]
        records = {}
        fa = make_analyzer(engine, models, False)
        for gpu in (False, True):
            sizes.clear()
            fa.gpu_thumbnails = gpu
            records[gpu] = BatchScorer(engine, face_analyzer=fa).process_files(blobs)
            assert (photos.nbytes in sizes) == (not gpu), sizes      # the batch comes down only for Pillow's crops
    finally:
        engine.close()
    thumbs = [d["thumbnail"] for r in records[False] for d in r["face_details"]]
    assert len(records[False]) == 4 and thumbs and all(t[:2] == b"\xff\xd8" for t in thumbs)
    assert deep_equal(records[True], records[False])
