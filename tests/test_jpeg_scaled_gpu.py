"""GPU: fe_jpeg_decode_scaled against Pillow's drafted image, pixel for pixel: `im.draft(None, ...)` makes libjpeg decode at 1/2, 1/4 or
1/8, and `np.asarray(im.convert('RGB'))` is the expectation. Files and expectations are made at test time (tests/jpeg_scaled_cases.py);
the same files pass the sanitized host harness in test_jpeg_scaled_host.py, which runs the very functions the kernels are built from."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as J
import jpeg_scaled_cases as S

pytestmark = pytest.mark.gpu


def by_scaled_size(cases, transpose=False):
    """{(scale, h, w): [(name, blob, drafted pixels)]}"""
    out = {}
    for name, blob in cases:
        for scale in S.SCALES:
            px = S.pillow_scaled(blob, scale, transpose)
            out.setdefault((scale,) + px.shape[:2], []).append((name, blob, px))
    return out


@pytest.fixture(scope="module")
def matrix_groups():
    return by_scaled_size(S.files())


def test_matrix_equals_pillow_draft_host_destination(engine, matrix_groups):
    assert sum(len(g) for g in matrix_groups.values()) == 7 * 4 * 3 * 2 * 2 * 3
    for (scale, h, w), group in matrix_groups.items():
        got, status = engine.jpeg_decode([b for _, b, _ in group], h, w, scale=scale)
        assert not status.any(), [(n, scale, int(s)) for (n, _, _), s in zip(group, status) if s]
        bad = [n for k, (n, _, px) in enumerate(group) if not np.array_equal(got[k], px)]
        assert not bad, (scale, bad[:10])


def test_matrix_equals_pillow_draft_device_destination_and_bgr(engine, matrix_groups):
    for (scale, h, w), group in matrix_groups.items():
        dev, status = engine.jpeg_decode([b for _, b, _ in group], h, w, bgr=True, device=True, scale=scale)
        try:
            got = np.empty((len(group), h, w, 3), np.uint8)
            engine.d2h(got, dev[0])
        finally:
            engine.dev_free(dev[0])
        assert not status.any()
        bad = [n for k, (n, _, px) in enumerate(group) if not np.array_equal(got[k], px[..., ::-1])]
        assert not bad, (scale, bad[:10])


def test_progressive_subset_under_the_flag(engine):
    for (scale, h, w), group in by_scaled_size(S.progressive_files()).items():
        blobs = [b for _, b, _ in group]
        got, status = engine.jpeg_decode(blobs, h, w, progressive=True, scale=scale)
        assert not status.any()
        bad = [n for k, (n, _, px) in enumerate(group) if not np.array_equal(got[k], px)]
        assert not bad, (scale, bad[:10])
        _, status = engine.jpeg_decode(blobs, h, w, scale=scale)              # without the flag: left to the caller
        assert (status == 1).all()


def test_orientations_at_scale_2_on_an_odd_size(engine):
    a = J.content("gradient", 21, 31)
    for s in (0, 1, 2):
        blobs = [J.encode(a, quality=90, subsampling=s, exif=J.exif_bytes(o, o % 2 == 0)) for o in range(1, 9)]
        flat, status = engine.jpeg_decode(blobs[:4], 11, 16, scale=2)           # 1 .. 4 keep the scaled size
        assert not status.any()
        turned, status = engine.jpeg_decode(blobs[4:], 16, 11, scale=2)         # 5 .. 8 exchange it
        assert not status.any()
        for k in range(4):
            assert np.array_equal(flat[k], S.pillow_scaled(blobs[k], 2, transpose=True)), (s, k + 1)
            assert np.array_equal(turned[k], S.pillow_scaled(blobs[4 + k], 2, transpose=True)), (s, k + 5)
        raw, status = engine.jpeg_decode(blobs, 11, 16, apply_orientation=False, scale=2)
        assert not status.any()
        assert all(np.array_equal(raw[k], S.pillow_scaled(blobs[0], 2)) for k in range(8))
        _, status = engine.jpeg_decode(blobs, 11, 16, scale=2)                  # the turned ones do not have this size
        assert status.tolist() == [0, 0, 0, 0, -5, -5, -5, -5]


def test_scale_1_equals_the_existing_call(engine):
    h, w = 53, 37
    blobs = [b for n, b in J.matrix() if n.startswith("53x37")][:40]
    ptrs = (C.c_char_p * len(blobs))(*blobs)
    lens = (C.c_size_t * len(blobs))(*[len(x) for x in blobs])
    for kw in (dict(), dict(bgr=True), dict(apply_orientation=False)):
        a, sa = engine.jpeg_decode(blobs, h, w, **kw)
        status = np.zeros(len(blobs), np.int32)
        b = np.zeros_like(a)
        rc = engine.lib.fe_jpeg_decode_scaled(engine.h, ptrs, lens, len(blobs), h, w, 1, 1 if kw.get("bgr") else 0,
                                              1 if kw.get("apply_orientation", True) else 0, 0, 0, b.ctypes.data_as(C.c_void_p),
                                              status.ctypes.data_as(C.c_void_p))
        assert rc == 0 and np.array_equal(status, sa) and np.array_equal(a, b)


def test_one_call_mixes_sampling_kinds_and_qualities(engine):
    h, w = 53, 37
    a = [J.content(k, h, w, 5) for k in ("noise", "gradient", "bands", "sparse")]
    blobs = [J.encode(a[0], quality=30, subsampling=2), J.encode(a[1], quality=95, subsampling=0, optimize=True),
             J.encode(a[2], quality=75, subsampling=1, restart_marker_blocks=1), J.encode(a[3], quality=100, subsampling=2, restart_marker_rows=1),
             J.encode(a[0][..., 0], quality=60, restart_marker_blocks=3), J.encode(a[1], quality=50, subsampling=1, optimize=True),
             J.encode(a[2], quality=85, subsampling=0, restart_marker_blocks=3), J.encode(a[0], quality=100, subsampling=2, progressive=True)]
    for scale in S.SCALES:
        sh, sw = engine.jpeg_scaled_size(h, w, scale)
        got, status = engine.jpeg_decode(blobs, sh, sw, progressive=True, scale=scale)
        assert not status.any()
        for k, b in enumerate(blobs):
            assert np.array_equal(got[k], S.pillow_scaled(b, scale)), (scale, k)


def test_damaged_files_get_the_existing_statuses_and_keep_their_slot(engine):
    """The inputs of test_jpeg_scaled_host.py::test_host_scaled_damaged_files_end_with_a_status, which the sanitized harness decodes
    without a report. The status comes from the parser and the entropy stage, which do not know the scale: it equals the full decode's."""
    for src_h, src_w, tag in ((53, 37, "420"), (33, 17, "444rst"), (48, 64, "422opt"), (17, 33, "gray")):
        bad = [(n, b) for n, b in J.damaged() if n.startswith(tag + "-")]
        good = J.encode(J.content("gradient", src_h, src_w), quality=85, subsampling=2, restart_marker_blocks=2)
        blobs = [good] + [b for _, b in bad] + [good]
        _, full_status = engine.jpeg_decode(blobs, src_h, src_w)
        for scale in S.SCALES:
            h, w = S.scaled_size(src_h, src_w, scale)
            n, per = len(blobs), h * w * 3
            guard = np.full((n + 2) * per, 0x5A, np.uint8)
            d = engine.dev_alloc(guard.nbytes)
            try:
                engine.h2d(d, guard)
                _, status = engine.jpeg_decode(blobs, h, w, device=type(d)(d.value + per), scale=scale)
                got = np.empty_like(guard)
                engine.d2h(got, d)
            finally:
                engine.dev_free(d)
            got = got.reshape(n + 2, h, w, 3)
            assert (got[0] == 0x5A).all() and (got[-1] == 0x5A).all()
            assert status[0] == 0 and status[-1] == 0
            assert np.array_equal(got[1], S.pillow_scaled(good, scale)) and np.array_equal(got[n], S.pillow_scaled(good, scale))
            for k, (name, blob) in enumerate(bad, start=1):
                assert status[k] <= 0, (name, int(status[k]))
                if "cut" in name:
                    assert status[k] < 0, name
                if status[k] < 0:
                    assert (got[1 + k] == 0x5A).all(), name
            # a reduced transform reads fewer coefficients, so only FE_JPEG_BAD_COEFFICIENT (-6) may come or go with the scale
            assert all(a == b or -6 in (a, b) for a, b in zip(status.tolist(), full_status.tolist()))


def test_a_bad_scale_raises_without_launching(engine):
    blob = J.encode(J.content("noise", 16, 16))
    for scale in (0, 3, 5, 16, -1):
        with pytest.raises(ValueError):
            engine.jpeg_decode([blob], 16, 16, scale=scale)
        ptrs, lens = (C.c_char_p * 1)(blob), (C.c_size_t * 1)(len(blob))
        out, status = np.full((16, 16, 3), 0xA5, np.uint8), np.full(1, 77, np.int32)
        rc = engine.lib.fe_jpeg_decode_scaled(engine.h, ptrs, lens, 1, 16, 16, scale, 0, 1, 0, 0, out.ctypes.data_as(C.c_void_p),
                                              status.ctypes.data_as(C.c_void_p))
        assert rc == -1 and b"scale" in engine.lib.fe_last_error(engine.h)          # FE_ERR_INVALID
        assert (out == 0xA5).all() and status[0] == 77


def test_decode_jpegs_scaled_never_depends_on_which_side_decoded(engine):
    from facet_amd.image_loading import decode_jpegs
    a = J.content("gradient", 33, 17)
    cmyk = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(cmyk, "JPEG")
    blobs = [J.encode(a, quality=80), J.encode(a, progressive=True), cmyk.getvalue(), J.encode(a[..., 0], quality=40), b"junk",
             J.encode(J.content("noise", 53, 37), subsampling=1, exif=J.exif_bytes(6))]
    for scale in S.SCALES:
        for prog in (False, True):
            got = decode_jpegs(engine, blobs, progressive=prog, scale=scale)
            assert got[4] is None
            for k in (0, 1, 2, 3, 5):
                assert np.array_equal(got[k], S.pillow_scaled(blobs[k], scale, transpose=True)), (scale, prog, k)
