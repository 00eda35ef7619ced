"""GPU: fe_jpeg_decode against Pillow, pixel for pixel (`ImageOps.exif_transpose(Image.open(f)).convert('RGB')`, the reference's
utils/image_loading.py:100-106). The files and the expectation are made at test time (tests/jpeg_cases.py); the same files pass the
sanitized host harness in test_jpeg_decode_host.py, which runs the very functions the kernels are built from."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as J

pytestmark = pytest.mark.gpu


def by_size(cases):
    """{(h, w): [(name, blob, pillow pixels)]} by decoded size."""
    out = {}
    for name, blob in cases:
        px = J.pillow_pixels(blob)
        out.setdefault(px.shape[:2], []).append((name, blob, px))
    return out


@pytest.fixture(scope="module")
def matrix_groups():
    return by_size(J.matrix())


def test_matrix_equals_pillow_host_destination(engine, matrix_groups):
    assert sum(len(g) for g in matrix_groups.values()) == 632
    for (h, w), group in matrix_groups.items():
        got, status = engine.jpeg_decode([b for _, b, _ in group], h, w)
        assert not status.any(), [(n, int(s)) for (n, _, _), s in zip(group, status) if s]
        bad = [n for k, (n, _, px) in enumerate(group) if not np.array_equal(got[k], px)]
        assert not bad, bad[:10]


def test_matrix_equals_pillow_device_destination_and_bgr(engine, matrix_groups):
    for (h, w), group in matrix_groups.items():
        dev, status = engine.jpeg_decode([b for _, b, _ in group], h, w, bgr=True, device=True)
        try:
            got = np.empty((len(group), h, w, 3), np.uint8)
            engine.d2h(got, dev[0])
        finally:
            engine.dev_free(dev[0])
        assert not status.any()
        bad = [n for k, (n, _, px) in enumerate(group) if not np.array_equal(got[k], px[..., ::-1])]
        assert not bad, bad[:10]


def test_one_call_mixes_quality_subsampling_tables_and_restarts(engine):
    h, w = 53, 37
    a = [J.content(k, h, w, 5) for k in ("noise", "gradient", "bands", "sparse")]
    blobs = [J.encode(a[0], quality=30, subsampling=2), J.encode(a[1], quality=95, subsampling=0, optimize=True),
             J.encode(a[2], quality=75, subsampling=1, restart_marker_blocks=1), J.encode(a[3], quality=100, subsampling=2, restart_marker_rows=1),
             J.encode(a[0][..., 0], quality=60, restart_marker_blocks=3), J.encode(a[1], quality=50, subsampling=1, optimize=True),
             J.encode(a[2], quality=85, subsampling=0, restart_marker_blocks=3), J.encode(a[0], quality=100, subsampling=2, optimize=True)]
    got, status = engine.jpeg_decode(blobs, h, w)
    assert not status.any()
    for k, b in enumerate(blobs):
        assert np.array_equal(got[k], J.pillow_pixels(b)), k


def test_orientations(engine):
    a = J.content("gradient", 20, 30)
    for s in (0, 1, 2):
        blobs = [J.encode(a, quality=90, subsampling=s, exif=J.exif_bytes(o, o % 2 == 0)) for o in range(1, 9)]
        flat, status = engine.jpeg_decode(blobs[:4], 20, 30)                 # 1 .. 4 keep the size
        assert not status.any()
        turned, status = engine.jpeg_decode(blobs[4:], 30, 20)               # 5 .. 8 exchange it
        assert not status.any()
        for k in range(4):
            assert np.array_equal(flat[k], J.pillow_pixels(blobs[k])), (s, k + 1)
            assert np.array_equal(turned[k], J.pillow_pixels(blobs[4 + k])), (s, k + 5)
        raw, status = engine.jpeg_decode(blobs, 20, 30, apply_orientation=False)
        assert not status.any()
        want = np.asarray(Image.open(io.BytesIO(blobs[0])).convert("RGB"))
        assert all(np.array_equal(raw[k], want) for k in range(8))
        mixed, status = engine.jpeg_decode(blobs, 20, 30)                    # the turned ones do not have this size
        assert status.tolist() == [0, 0, 0, 0, -5, -5, -5, -5]


def test_unsupported_files_get_their_code_and_keep_their_slot(engine):
    from facet_amd.image_loading import decode_jpegs
    h, w = 33, 17
    a = J.content("gradient", h, w)
    cmyk = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(cmyk, "JPEG")
    blobs = [J.encode(a, quality=80), J.encode(a, progressive=True), cmyk.getvalue(), J.encode(a, quality=40, subsampling=0)]
    n, per = len(blobs), h * w * 3
    guard = np.full((n + 2) * per, 0xA5, np.uint8)
    d = engine.dev_alloc(guard.nbytes)
    try:
        engine.h2d(d, guard)
        _, status = engine.jpeg_decode(blobs, h, w, device=type(d)(d.value + per))
        got = np.empty_like(guard)
        engine.d2h(got, d)
    finally:
        engine.dev_free(d)
    assert status.tolist() == [0, 1, 4, 0]
    got = got.reshape(n + 2, h, w, 3)
    assert (got[0] == 0xA5).all() and (got[-1] == 0xA5).all() and (got[2] == 0xA5).all() and (got[3] == 0xA5).all()
    assert np.array_equal(got[1], J.pillow_pixels(blobs[0])) and np.array_equal(got[4], J.pillow_pixels(blobs[3]))
    for px, b in zip(decode_jpegs(engine, blobs), blobs):
        assert np.array_equal(px, J.pillow_pixels(b))


def test_damaged_files_get_a_negative_status_and_neighbours_decode(engine):
    """The inputs of test_jpeg_decode_host.py::test_host_decode_damaged_files_end_with_a_status, which the sanitized host harness decodes
    without a report: this checks the statuses and the bounds the kernels were built with."""
    for src_h, src_w, tag in ((53, 37, "420"), (33, 17, "444rst"), (48, 64, "422opt"), (17, 33, "gray")):
        bad = [(n, b) for n, b in J.damaged() if n.startswith(tag + "-")]
        good = J.encode(J.content("gradient", src_h, src_w), quality=85, subsampling=2, restart_marker_blocks=2)
        blobs = [good] + [b for _, b in bad] + [good]
        n, per = len(blobs), src_h * src_w * 3
        guard = np.full((n + 2) * per, 0x5A, np.uint8)
        d = engine.dev_alloc(guard.nbytes)
        try:
            engine.h2d(d, guard)
            _, status = engine.jpeg_decode(blobs, src_h, src_w, device=type(d)(d.value + per))
            got = np.empty_like(guard)
            engine.d2h(got, d)
        finally:
            engine.dev_free(d)
        got = got.reshape(n + 2, src_h, src_w, 3)
        assert (got[0] == 0x5A).all() and (got[-1] == 0x5A).all()
        assert status[0] == 0 and status[-1] == 0
        assert np.array_equal(got[1], J.pillow_pixels(good)) and np.array_equal(got[n], J.pillow_pixels(good))
        for k, (name, blob) in enumerate(bad, start=1):
            assert status[k] <= 0, (name, int(status[k]))
            if "cut" in name:
                assert status[k] < 0, name
            if status[k] < 0:
                assert (got[1 + k] == 0x5A).all(), name
            else:
                assert np.array_equal(got[1 + k], J.pillow_pixels(blob)), name
        host, hstatus = engine.jpeg_decode(blobs, src_h, src_w)
        assert np.array_equal(hstatus, status) and all((host[k] == 0).all() for k in range(n) if status[k] != 0)


def test_process_files_equals_process_batch_on_pillows_decode():
    from facet_amd import Engine
    from facet_amd.batch import BatchScorer
    from facet_amd._lib import FE_MODEL_TOPIQ
    from facet_amd.weights import synthetic_state_dict
    engine = Engine(0, arena_bytes=2 << 30)      # its own context: the session's carries no models
    engine.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
    h, w = 96, 128
    imgs = [J.content(k, h, w, 9) for k in ("gradient", "noise", "bands", "sparse")]
    blobs = [J.encode(imgs[0], quality=85, subsampling=2), J.encode(imgs[1], quality=75, subsampling=1, restart_marker_rows=1),
             J.encode(imgs[2], quality=95, subsampling=0, optimize=True), J.encode(np.rot90(imgs[3]).copy(), quality=85, exif=J.exif_bytes(6))]
    scorer = BatchScorer(engine, phash=True)
    got = scorer.process_files(blobs)
    want = scorer.process_batch(np.stack([J.pillow_pixels(b) for b in blobs]))
    engine.close()
    assert len(got) == 4
    for g, r in zip(got, want):
        assert g.keys() == r.keys()
        for key in r:
            assert np.array_equal(g[key], r[key]) if isinstance(r[key], np.ndarray) else g[key] == r[key], key
