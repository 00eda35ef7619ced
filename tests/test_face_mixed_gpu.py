"""GPU: the face path over images of mixed sizes in one engine call (fe_face_analyze_mixed and the calls beside it: Engine.face_analyze_mixed,
face_det_input_mixed, face_crops_run_mixed, roi_laplacian_mixed, face_thumbnails_mixed, face_cache_entries; FaceEngine.get_batch_mixed).

Images, thresholds and the seeds that keep every score and overlap 1e-3 away from its threshold: tests/face_mixed_cases.py (checked on the
CPU by tests/test_face_mixed_host.py). The integer pixel work (detector input, crops, ROI sums, thumbnails) must equal its reference bit
for bit. The records of face_analyze_mixed are compared with face_analyze of every image alone within the bounds tests/test_face_gpu.py
holds between the engine and its oracle: a graph's summation routes may depend on the batch it runs in, so equal bits are not required."""
import ctypes

import numpy as np
import pytest

import face_mixed_cases as FC
from conftest import assert_int_boxes_match
from facet_amd._lib import FE_ERR_INVALID, FE_FACE_FLOATS, FE_GRAPH_FACE_REC, EngineError
from facet_amd.face import FaceEngine, face_thumbnail_plan, face_thumbnails, face_thumbnails_mixed
from oracle import face_ref
from standins import synthetic_onnx as S

pytestmark = pytest.mark.gpu

MAX_FACES = 256


@pytest.fixture(scope="module")
def models():
    det, _ = S.scrfd_like(seed=12, size=320)
    lmk, _ = S.landmark_like(seed=13)
    rec, _ = S.arcface_iresnet(layers=(1, 1, 1, 1), seed=14)
    return {"det": det, "lmk": lmk, "rec": rec}


@pytest.fixture(scope="module")
def fe(engine, models):
    engine.set_microbatch(8)      # the session's engine keeps what the test before left
    f = FaceEngine(engine, models, det_size=FC.DET_SIZE, det_thresh=FC.DET_THRESH, nms_thresh=FC.NMS_THRESH, max_candidates=4096, max_faces=MAX_FACES)
    yield f
    f.unload()


@pytest.fixture(scope="module")
def imgs():
    return FC.images(FC.DETECT)


@pytest.fixture(scope="module")
def singles(engine, fe, imgs):
    """face_analyze of every image alone: (records [max_faces, 739], count). Computed once, never changed."""
    out = []
    for a in imgs:
        rec, counts, mask = engine.face_analyze(a[None], FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, MAX_FACES)
        assert mask == 7
        rec.setflags(write=False)
        out.append((rec[0], int(counts[0])))
    return out


class _Resident:
    """Images in one allocation, each at the first odd byte offset behind the one before."""
    def __init__(self, engine, arrs):
        self.engine = engine
        offs, at = [], 1
        for a in arrs:
            offs.append(at)
            at += a.nbytes
            at += 1 - at % 2
        self.buf = engine.dev_alloc(at)
        for a, o in zip(arrs, offs):
            engine.h2d(ctypes.c_void_p(self.buf.value + o), a)
        self.offsets = offs
        self.images = ([self.buf.value + o for o in offs], [a.shape[:2] for a in arrs])

    def __enter__(self):
        return self.images

    def __exit__(self, *exc):
        self.engine.dev_free(self.buf)


def _rgb(arrs):
    return [np.ascontiguousarray(a[..., ::-1]) for a in arrs]


def _compare(got, got_count, want, want_count, what):
    """The bounds of tests/test_face_gpu.py lines 65-67 and 88-89 between two records of one image."""
    assert got_count == want_count, f"{what}: {got_count} faces, {want_count} alone"
    k = min(want_count, MAX_FACES)
    if k == 0:
        return
    g, w = got[:k].astype(np.float64), want[:k].astype(np.float64)
    lm_bound = 1e-4 * max(1.0, np.abs(w[:, 15:227]).max())
    em_bound = 1e-4 * np.abs(w[:, 227:739]).max()
    d = np.abs(g - w)
    print(f"[face mixed] {what}: {k} faces, |score| {d[:, 4].max():.2e}, |box| {d[:, 0:4].max():.2e}, |kps| {d[:, 5:15].max():.2e}, "
          f"|lmk| {d[:, 15:227].max():.2e} (bound {lm_bound:.2e}), |emb| {d[:, 227:739].max():.2e} (bound {em_bound:.2e}), "
          f"bit-equal {np.array_equal(got[:k], want[:k])}")
    assert d[:, 4].max() < 1e-4, what
    assert d[:, 0:4].max() < 2e-2 and d[:, 5:15].max() < 2e-2, what
    assert_int_boxes_match(got[:k, 0:4], want[:k, 0:4])
    assert d[:, 15:227].max() < lm_bound, what
    assert d[:, 227:739].max() < em_bound, what
    assert not got[k:].any(), f"{what}: unused slots are not zero"


# ---- 1. detector input -------------------------------------------------------------------------------------------------------------
def _expected_det_input(img_bgr):
    h, w = img_bgr.shape[:2]
    det_h, det_w = FC.DET_SIZE
    F = np.float32      # SCRFD.detect's fit in fp32, as fe_face_analyze computes it (tests/test_face_mixed_host.py pins the planner to it)
    if F(h) / F(w) > F(det_h) / F(det_w):
        new_h, new_w = det_h, int(F(det_h) / (F(h) / F(w)))
    else:
        new_w, new_h = det_w, int(F(det_w) * (F(h) / F(w)))
    canvas = np.zeros((det_h, det_w, 3), np.uint8)
    canvas[:new_h, :new_w] = face_ref.cv_resize_linear_u8(img_bgr, new_h, new_w)
    out = np.zeros((det_h, det_w, 4), np.float32)
    out[..., :3] = (canvas[..., ::-1].astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 128)      # R, G, B as the graph takes them
    return out


def test_detector_input_bit_exact_from_host_bgr_and_resident_rgb(engine, imgs):
    want = np.stack([_expected_det_input(a) for a in imgs])
    pad = np.float32(-127.5 / 128)      # the two truncated fits, as the expected tensor must have them: 192 rows of 300 x 500, 240 columns of 400 x 300
    assert (want[3, 192:, :, :3] == pad).all() and (want[3, 191, :, :3] != pad).any() and (want[4, :, 240:, :3] == pad).all() and (want[4, :, 239, :3] != pad).any()
    got = engine.face_det_input_mixed(imgs, FC.DET_SIZE, order='bgr')
    for i in range(len(imgs)):
        assert np.array_equal(got[i], want[i]), f"host BGR: image {i} {imgs[i].shape[:2]}: {int((got[i] != want[i]).sum())} values differ"
    res = _Resident(engine, _rgb(imgs))
    assert all(o % 2 == 1 for o in res.offsets)
    with res as dev:
        got = engine.face_det_input_mixed(dev, FC.DET_SIZE, order='rgb')
    for i in range(len(imgs)):
        assert np.array_equal(got[i], want[i]), f"resident RGB: image {i} {imgs[i].shape[:2]}: {int((got[i] != want[i]).sum())} values differ"


# ---- 2. crops ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crop_case():
    rng = np.random.default_rng(5)
    arrs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((240, 320), (131, 97), (400, 300))]
    Ms, idx = [], []
    for f in range(10):      # as test_warp_affine_bit_exact
        ang, sc = rng.uniform(-0.6, 0.6), rng.uniform(0.3, 2.5)
        c, s = np.cos(ang) * sc, np.sin(ang) * sc
        Ms.append([[c, -s, rng.uniform(-80, 60)], [s, c, rng.uniform(-80, 60)]])     # some crops hang over the border
        idx.append(f % 3)
    return arrs, np.asarray(Ms, np.float64), idx


@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("size", [112, 192])
def test_crops_bit_exact(engine, crop_case, size, order):
    arrs, Ms, idx = crop_case
    src = arrs if order == 'bgr' else _rgb(arrs)
    _, crops = engine.face_crops_run_mixed(FE_GRAPH_FACE_REC, src, idx, Ms, size, 0.0, 1.0, out_dim=0, want_crops=True, order=order)
    for f in range(10):
        assert np.array_equal(crops[f], face_ref.warp_affine_u8(src[idx[f]], Ms[f], size)), (size, order, f)
    with _Resident(engine, src) as dev:
        _, again = engine.face_crops_run_mixed(FE_GRAPH_FACE_REC, dev, idx, Ms, size, 0.0, 1.0, out_dim=0, want_crops=True, order=order)
    assert np.array_equal(again, crops)


def test_fused_warp_feeds_the_graph_what_the_byte_crops_do(engine, fe, crop_case):
    """Without crops_out the warp writes the graph's fp32 input itself. The same ten crops through the same graph in the same batch: the
    embeddings of the fused route, of the byte route, of either byte order and of face_crops_run on a same-sized batch are the same bits
    (all four feed the graph the same numbers: an 8-bit value minus 127.5, times 1 / 127.5, is one fp32 operation each)."""
    arrs, Ms, idx = crop_case
    fused, _ = engine.face_crops_run_mixed(FE_GRAPH_FACE_REC, arrs, idx, Ms, 112, 127.5, 1 / 127.5, out_dim=512, order='bgr')
    bytes_, crops = engine.face_crops_run_mixed(FE_GRAPH_FACE_REC, arrs, idx, Ms, 112, 127.5, 1 / 127.5, out_dim=512, want_crops=True, order='bgr')
    rgb, _ = engine.face_crops_run_mixed(FE_GRAPH_FACE_REC, _rgb(arrs), idx, Ms, 112, 127.5, 1 / 127.5, out_dim=512, order='rgb')
    assert np.abs(fused).max() > 0 and crops is not None
    assert np.array_equal(fused, bytes_) and np.array_equal(fused, rgb)
    same = np.stack([arrs[0], arrs[0][::-1].copy(), arrs[0][:, ::-1].copy()])
    want, _ = engine.face_crops_run(FE_GRAPH_FACE_REC, same, idx, Ms, 112, 127.5, 1 / 127.5, out_dim=512)
    got, _ = engine.face_crops_run_mixed(FE_GRAPH_FACE_REC, list(same), idx, Ms, 112, 127.5, 1 / 127.5, out_dim=512, order='bgr')
    assert np.array_equal(got, want)


# ---- 3. ROI Laplacian ----------------------------------------------------------------------------------------------------------------
def test_roi_laplacian_equals_the_per_image_call(engine, imgs):
    rng = np.random.default_rng(21)
    rois, idx = [], []
    for i, a in enumerate(imgs):
        h, w = a.shape[:2]
        rois += [[0, 0, w, h], [0, 0, 1, 1], [w - 1, h - 1, w, h], [0, 0, w, 1], [0, 0, 1, h], [w - 1, 0, w, h], [0, h - 1, w, h]]      # whole, 1 x 1, 1 x k, borders
        idx += [i] * 7
        for _ in range(4):
            x1, y1 = int(rng.integers(0, w)), int(rng.integers(0, h))
            rois.append([x1, y1, int(rng.integers(x1 + 1, w + 1)), int(rng.integers(y1 + 1, h + 1))])
            idx.append(i)
    rois.append([3, 3, 3, 9]); idx.append(0)      # empty
    order = rng.permutation(len(rois))           # ROIs of one image are not neighbours
    rois, idx = [rois[k] for k in order], [idx[k] for k in order]
    want = np.zeros((len(rois), 4))
    for i, a in enumerate(imgs):
        mine = [k for k in range(len(rois)) if idx[k] == i]
        want[mine] = engine.roi_laplacian(a[None], [0] * len(mine), [rois[k] for k in mine])
    assert want[:, 3].max() == 640 * 640 and (want[:, 3] == 1).any() and (want[:, 3] == 0).sum() == 1
    got = engine.roi_laplacian_mixed(imgs, idx, rois, order='bgr')
    assert np.array_equal(got, want)
    with _Resident(engine, _rgb(imgs)) as dev:      # R,G,B read in place against the BGR call on the swapped copy
        got = engine.roi_laplacian_mixed(dev, idx, rois, order='rgb')
    assert np.array_equal(got, want)
    with pytest.raises(EngineError, match=r"roi 0 .* image 6"):      # checked against the ROI's own image (8 x 600)
        engine.roi_laplacian_mixed(imgs, [6], [[0, 0, 600, 9]])


# ---- 4. face_analyze_mixed against face_analyze of every image alone ------------------------------------------------------------------
def test_records_match_the_per_image_call(engine, fe, imgs, singles):
    assert all(c > 0 for _, c in singles), [c for _, c in singles]      # every image of item 1 yields detections (face_mixed_cases.py)
    rec, counts, mask = engine.face_analyze_mixed(imgs, FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, MAX_FACES, order='bgr')
    assert mask == 7 and rec.shape == (len(imgs), MAX_FACES, FE_FACE_FLOATS)
    for i, (want, c) in enumerate(singles):
        _compare(rec[i], int(counts[i]), want, c, f"host BGR image {i} {imgs[i].shape[:2]}")
    with _Resident(engine, _rgb(imgs)) as dev:
        rec2, counts2, _ = engine.face_analyze_mixed(dev, FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, MAX_FACES, order='rgb')
    # the same pixels through the same kernels in the same batches: host BGR and resident RGB are the same bits
    assert np.array_equal(counts2, counts) and np.array_equal(rec2, rec)
    faces = fe.get_batch_mixed(imgs)
    assert [len(f) for f in faces] == [c for _, c in singles]
    assert np.array_equal(faces[3][0].bbox, rec[3, 0, 0:4]) and np.array_equal(faces[3][0].embedding, rec[3, 0, 227:739])


# ---- 5. batching ------------------------------------------------------------------------------------------------------------------
def test_micro_batches_order_thresholds_and_capacity(engine, fe, imgs, singles):
    seven = [imgs[k] for k in (6, 0, 3, 1, 5, 2, 4)]      # not the order of the fixture: input order is kept
    want = [singles[k] for k in (6, 0, 3, 1, 5, 2, 4)]
    large, large_counts, _ = engine.face_analyze_mixed(seven, FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, MAX_FACES)
    engine.set_microbatch(1)      # micro-batches of 2: four of them, the last with one image
    try:
        small, small_counts, _ = engine.face_analyze_mixed(seven, FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, MAX_FACES)
    finally:
        engine.set_microbatch(8)
    for i in range(7):
        _compare(small[i], int(small_counts[i]), large[i], int(large_counts[i]), f"micro-batches of 2 against one of 7, image {i}")
        _compare(large[i], int(large_counts[i]), want[i][0], want[i][1], f"one micro-batch of 7, image {i}")
    none, none_counts, _ = engine.face_analyze_mixed(seven, FC.DET_SIZE, 0.999, FC.NMS_THRESH, MAX_FACES)      # above every score
    assert not none_counts.any() and not none.any()
    best, best_counts, _ = engine.face_analyze_mixed(seven, FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, 3)      # capacity below the detections
    assert np.array_equal(best_counts, large_counts) and best.shape == (7, 3, FE_FACE_FLOATS)
    for i in range(7):
        k = min(3, int(large_counts[i]))
        _compare(best[i], k, large[i, :3], k, f"max_faces 3, image {i}")
        assert not best[i, k:].any()


# ---- 6. face thumbnails ------------------------------------------------------------------------------------------------------------
def test_face_thumbnail_bytes_equal_the_per_image_call(engine):
    arrs = [FC.image(k) for k in (1, 3, 4)]      # 200 x 320, 300 x 500, 400 x 300
    boxes = [[(10.5, 20.2, 90.9, 130.0), (250, 150, 330, 210), (-5, -5, 40, 60)], [(100, 50, 400, 280), (3, 3, 9, 9)], [(20, 30, 280, 390), (0, 0, 0, 0)]]
    want = [face_thumbnails(engine, a[None], [b])[0] for a, b in zip(arrs, boxes)]
    assert sum(w is not None for ws in want for w in ws) >= 6 and want[2][1] is None
    assert face_thumbnail_plan(boxes[0][1], 200, 320) is not None      # a box that reaches past the right and bottom edge
    assert face_thumbnails_mixed(engine, arrs, boxes, order='bgr') == want
    with _Resident(engine, _rgb(arrs)) as dev:
        assert face_thumbnails_mixed(engine, dev, boxes, order='rgb') == want
    big = face_thumbnails(engine, arrs[1][None], [boxes[1][:1]], size=300)      # past the fused encoder's 128 x 128
    assert face_thumbnails_mixed(engine, arrs, [[], boxes[1][:1], []], size=300)[1] == big[0]


# ---- 7. the weight-table cache -------------------------------------------------------------------------------------------------------
def test_mixed_calls_cache_no_table_per_size(engine, fe):
    rng = np.random.default_rng(3)
    shapes = [(211 + 2 * k, 307 + 3 * k) for k in range(8)]      # eight sizes no other test uses
    arrs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    before = engine.face_cache_entries()
    engine.face_analyze_mixed(arrs, FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, 8)
    engine.face_det_input_mixed(arrs, FC.DET_SIZE)
    assert engine.face_cache_entries() == before
    for a in arrs[:3]:
        engine.face_analyze(a[None], FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, 8)
    assert engine.face_cache_entries() >= before + 3      # a column and a row table per new size; some may be shared


# ---- 8. bad arguments ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_invalid_and_launch_nothing(engine, fe, imgs, singles):
    good = list(imgs[:2]) + list(imgs[3:5])
    args = (FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, 8)

    def refused(match, call):
        with pytest.raises(EngineError, match=match) as ei:
            call()
        assert ei.value.status == FE_ERR_INVALID, ei.value

    engine.profile_enable(True)      # every layer of a graph that runs leaves a record
    try:
        zero = good[:2] + [np.zeros((0, 64, 3), np.uint8)] + good[2:]
        refused(r"image 2\b", lambda: engine.face_analyze_mixed(zero, *args))
        refused(r"image 2\b", lambda: engine.face_analyze_mixed(good[:2] + [np.zeros((5, 0, 3), np.uint8)] + good[2:], *args))
        refused(r"image 2\b", lambda: engine.face_analyze_mixed(good[:2] + [None] + good[2:], *args))
        flat = good[:3] + [np.zeros((2, 2000, 3), np.uint8)]      # new_h = int(320 * 2 / 2000) = 0
        refused(r"image 3\b.*empty detector input", lambda: engine.face_analyze_mixed(flat, *args))
        refused(r"image 3\b.*empty detector input", lambda: engine.face_det_input_mixed(flat, FC.DET_SIZE))
        refused(r"image 0\b.*empty detector input", lambda: engine.face_analyze_mixed([np.zeros((2000, 2, 3), np.uint8)], *args))
        refused(r"n <= 0", lambda: engine.face_analyze_mixed([], *args))
        refused(r"order 2\b", lambda: engine.face_analyze_mixed(good, *args, order=2))
        for det in ((320, 300), (16, 320), (0, 0)):
            refused(r"detector input %d x %d" % det, lambda det=det: engine.face_analyze_mixed(good, det, *args[1:]))
        refused(r"image 1\b", lambda: engine.roi_laplacian_mixed([good[0], None], [0], [[0, 0, 1, 1]]))
        refused(r"order 7\b", lambda: engine.roi_laplacian_mixed(good, [0], [[0, 0, 1, 1]], order=7))
        refused(r"image 2\b", lambda: engine.face_thumbnails_mixed(zero, [0], [[0, 0, 8, 8]], [[8, 8]]))
        refused(r"image 2\b", lambda: engine.face_crops_run_mixed(FE_GRAPH_FACE_REC, zero, [0], np.eye(2, 3)[None], 112, 0.0, 1.0, want_crops=True))
        # a null list, through the C interface itself
        hw = np.array([[8, 8]], np.int32)
        rec, cnt = np.zeros((1, 8, FE_FACE_FLOATS), np.float32), np.zeros(1, np.int32)
        rc = engine.lib.fe_face_analyze_mixed(engine.h, None, hw.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, 0, 0, 320, 320, 0.5, 0.4, 8,
                                              rec.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None)
        assert rc == FE_ERR_INVALID
        assert engine.profile_records() == []
        rec, counts, _ = engine.face_analyze_mixed(imgs[:2], FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, MAX_FACES)      # the context stays usable
        assert engine.profile_records() != []
    finally:
        engine.profile_enable(False)
    for i in range(2):
        _compare(rec[i], int(counts[i]), singles[i][0], singles[i][1], f"after the refused calls, image {i}")


def test_host_image_that_cannot_be_staged_is_a_capacity_error():
    """Host images are staged in a quarter of the arena: one that alone exceeds it is FE_ERR_CAPACITY by its index, before anything
    runs (no graph is loaded here); the same pixels resident need no staging and get as far as the missing detector graph."""
    from facet_amd import Engine
    from facet_amd._lib import EngineCapacityError
    e = Engine(0, arena_bytes=32 << 20)
    try:
        small, big = np.zeros((64, 64, 3), np.uint8), np.zeros((1700, 1700, 3), np.uint8)      # 8.3 MiB staged against 8 MiB of room
        with pytest.raises(EngineCapacityError, match=r"image 1\b"):
            e.face_analyze_mixed([small, big, small], FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, 8)
        with _Resident(e, [small, big]) as dev:
            with pytest.raises(EngineError) as ei:
                e.face_analyze_mixed(dev, FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH, 8)
        assert not isinstance(ei.value, EngineCapacityError) and ei.value.status != FE_ERR_INVALID
        with pytest.raises(EngineCapacityError, match=r"image 4\b"):      # the calls that stage the whole list: the fourth 8.3 MiB image passes 32 MiB
            e.roi_laplacian_mixed([small] + [big] * 4, [0], [[0, 0, 8, 8]])
    finally:
        e.close()
