"""GPU: the decode entry points with FE_JPEG_FLAG_PARALLEL (parallel_entropy=True) against Pillow, pixel for pixel and byte for byte.
The files (tests/jpeg_parallel_cases.py) are the ones the sanitized host harness decodes in test_jpeg_parallel_host.py with the very
functions the kernels are built from. Nothing is compared with the call without the flag, except the statuses of damaged files, which
Pillow can only describe as an exception. Engine.jpeg_entropy_stats() proves which path ran: the segments and subsequences it reports
are counted again here from the files' bytes, and no honest file is decoded twice."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_parallel_cases as P
import jpeg_scaled_cases as S

pytestmark = pytest.mark.gpu

ZERO = dict(parallel_segments=0, subsequences=0, max_rounds=0, redone=0)


def decode_and_check(engine, blobs, **kw):
    """One call with the flag over files of one size: every slot equals Pillow, the stats equal the count from the bytes."""
    want = [J.pillow_pixels(b) for b in blobs]
    h, w = want[0].shape[:2]
    got, status = engine.jpeg_decode(blobs, h, w, parallel_entropy=True, **kw)
    stats = engine.jpeg_entropy_stats()
    assert not status.any(), status.tolist()
    for k in range(len(blobs)):
        assert np.array_equal(got[k], want[k]), k
    segs, subs = P.expected_stats(blobs)
    assert stats["redone"] == 0 and (stats["parallel_segments"], stats["subsequences"]) == (segs, subs), stats
    assert (stats["max_rounds"] > 0) == (segs > 0) and stats["max_rounds"] <= max([1] + [-(-(e - s) // P.SUB) for b in blobs for s, e in P.segments(b)])
    return stats


def test_single_blocks_take_the_serial_kernel(engine):
    for name, blob in P.single_block():
        assert decode_and_check(engine, [blob]) == ZERO, name


def test_long_blocks_flat_content_and_stuffed_cuts(engine):
    for name, blob in P.long_blocks() + P.flat() + [("stuffed", P.stuffed_file())]:
        stats = decode_and_check(engine, [blob])
        assert stats["parallel_segments"] == 1, name
        print(f"[parallel entropy] {name}: {stats['subsequences']} subsequences settled in {stats['max_rounds']} rounds")


def test_photo_matrix_one_call(engine):
    cases = P.photo_matrix()
    stats = decode_and_check(engine, [b for _, b in cases])                    # long, mixed and short segments in one chunk
    assert stats["parallel_segments"] > 100
    for name, blob in cases:
        one = decode_and_check(engine, [blob])
        if name.endswith("rst3") and ("4:4:4" in name or "gray" in name):      # every segment shorter than a subsequence
            assert one == ZERO, name
        else:
            assert one["parallel_segments"] > 0, name


def test_flag_off_reports_zero_stats(engine):
    blob = P.photo_matrix()[0][1]
    px = J.pillow_pixels(blob)
    engine.jpeg_decode([blob], *px.shape[:2], parallel_entropy=True)
    assert engine.jpeg_entropy_stats()["parallel_segments"] == 1
    got, status = engine.jpeg_decode([blob], *px.shape[:2])
    assert status[0] == 0 and np.array_equal(got[0], px) and engine.jpeg_entropy_stats() == ZERO


def test_orientations_bgr_and_device_destination(engine):
    a = P.photo(40, 56, 3)
    blobs = [J.encode(a, quality=90, subsampling=2, exif=J.exif_bytes(o, o % 2 == 0)) for o in range(1, 9)]
    assert P.expected_stats(blobs[:1])[0] == 1
    decode_and_check(engine, blobs[:4])                                        # 1 .. 4 keep the size
    decode_and_check(engine, blobs[4:])                                        # 5 .. 8 exchange it
    dev, status = engine.jpeg_decode(blobs[:4], 40, 56, bgr=True, device=True, parallel_entropy=True)
    try:
        got = np.empty((4, 40, 56, 3), np.uint8)
        engine.d2h(got, dev[0])
    finally:
        engine.dev_free(dev[0])
    assert not status.any() and engine.jpeg_entropy_stats()["parallel_segments"] == 4
    for k in range(4):
        assert np.array_equal(got[k], J.pillow_pixels(blobs[k])[..., ::-1]), k


def test_scaled_decode(engine):
    blob = J.encode(P.photo(427, 640, 5), quality=80)
    for scale in S.SCALES:
        want = S.pillow_scaled(blob, scale)
        got, status = engine.jpeg_decode([blob], *want.shape[:2], scale=scale, parallel_entropy=True)
        stats = engine.jpeg_entropy_stats()
        assert status[0] == 0 and np.array_equal(got[0], want), scale
        assert stats["redone"] == 0 and (stats["parallel_segments"], stats["subsequences"]) == P.expected_stats([blob])


@pytest.mark.parametrize("size", [320, 100])
def test_thumbnails_equal_pillows_bytes(engine, size):
    from facet_amd.thumbnail import pillow_resize_thumbnail, resize_thumbnails
    blobs = P.thumbnail_sources()
    got = resize_thumbnails(engine, blobs, size, parallel_entropy=True)
    stats = engine.jpeg_entropy_stats()                                        # of the last source size, two files
    for k, b in enumerate(blobs):
        assert got[k] == pillow_resize_thumbnail(b, size), k
    assert stats["redone"] == 0 and (stats["parallel_segments"], stats["subsequences"]) == P.expected_stats(blobs[2:])


def test_one_call_mixes_every_kind(engine):
    """A file without restart markers, one with a marker per MCU row, a complete progressive file (both flags) and a file of one-block
    segments in one fe_jpeg_decode_ex call. The files of one call share their output size, so the 8 x 8 file of the plan cannot sit in
    that call: a quality-5 file with a restart marker behind every MCU stands in for it there (every segment shorter than a
    subsequence), and the 8 x 8 file itself joins through decode_jpegs, which groups by size and makes one call per group."""
    h, w = 203, 157
    a = P.photo(h, w, 1)
    blobs = [P.photo_matrix()[0][1], J.encode(a, quality=80, subsampling=1, restart_marker_rows=1), J.encode(a, quality=80, subsampling=2, progressive=True),
             J.encode(a, quality=5, subsampling=2, restart_marker_blocks=1)]
    want = [J.pillow_pixels(b) for b in blobs]
    got, status = engine.jpeg_decode(blobs, h, w, progressive=True, parallel_entropy=True)
    stats = engine.jpeg_entropy_stats()
    assert not status.any()
    for k in range(4):
        assert np.array_equal(got[k], want[k]), k
    base = [blobs[0], blobs[1], blobs[3]]                                      # the progressive file's scans stay a lane per segment
    assert stats["redone"] == 0 and (stats["parallel_segments"], stats["subsequences"]) == P.expected_stats(base) and stats["parallel_segments"] > 1
    from facet_amd.image_loading import decode_jpegs
    blobs.append(P.single_block()[0][1])                                       # an 8 x 8 file has its own size: decode_jpegs groups by size
    for k, px in enumerate(decode_jpegs(engine, blobs, progressive=True, parallel_entropy=True)):
        assert np.array_equal(px, J.pillow_pixels(blobs[k])), k
    assert engine.jpeg_entropy_stats() == ZERO                                 # of the last group, the one-block file: the serial kernel


def test_damaged_files_get_the_serial_statuses_and_are_decoded_again(engine):
    """The inputs of test_jpeg_parallel_host.py::test_damaged_files_and_trailing_bytes_end_as_the_serial_decoder_does, which the
    sanitized harness decodes without a report. A baseline file is decoded again exactly when its entropy stage reports an error, and
    the status shows that as -2 (a bad code) or -3 (data that ends early) unless the transform stage also reports -6 for what such a
    decode left, which is the smaller number and wins, with and without the flag; an honest stream with wild coefficients gets -6 too.
    So the files whose status without the flag is -6 are left out of the call with the flag, and for the rest `redone` equals the
    number of files with a negative entropy status. What the parser refuses never reaches the device."""
    total_redone = 0
    for src_h, src_w, tag in ((53, 37, "420"), (33, 17, "444rst"), (48, 64, "422opt"), (17, 33, "gray")):
        bad = [(n, b) for n, b in J.damaged() if n.startswith(tag + "-")]
        good = J.encode(P.photo(src_h, src_w, 2), quality=85, subsampling=2)
        _, first_status = engine.jpeg_decode([b for _, b in bad], src_h, src_w)
        bad = [nb for nb, s in zip(bad, first_status) if s != -6]
        blobs = [good] + [b for _, b in bad] + [good]
        n, per = len(blobs), src_h * src_w * 3
        _, serial_status = engine.jpeg_decode(blobs, src_h, src_w)
        guard = np.full((n + 2) * per, 0x5A, np.uint8)
        d = engine.dev_alloc(guard.nbytes)
        try:
            engine.h2d(d, guard)
            _, status = engine.jpeg_decode(blobs, src_h, src_w, device=type(d)(d.value + per), parallel_entropy=True)
            stats = engine.jpeg_entropy_stats()
            got = np.empty_like(guard)
            engine.d2h(got, d)
        finally:
            engine.dev_free(d)
        got = got.reshape(n + 2, src_h, src_w, 3)
        assert np.array_equal(status, serial_status), (tag, status.tolist(), serial_status.tolist())
        assert (got[0] == 0x5A).all() and (got[-1] == 0x5A).all()
        assert status[0] == 0 and status[-1] == 0
        assert np.array_equal(got[1], J.pillow_pixels(good)) and np.array_equal(got[n], J.pillow_pixels(good))
        for k, (name, blob) in enumerate(bad, start=1):
            if status[k] < 0:
                assert (got[1 + k] == 0x5A).all(), name
            else:
                assert np.array_equal(got[1 + k], J.pillow_pixels(blob)), name
        entropy_bad = sum(1 for k, (name, blob) in enumerate(bad, start=1) if status[k] in (-2, -3) and engine.jpeg_probe(blob)["status"] == 0)
        print(f"[parallel entropy] damaged {tag}: statuses {status.tolist()}, redone {stats['redone']}, entropy errors {entropy_bad}")
        assert -6 not in status.tolist() and stats["redone"] == entropy_bad, (tag, stats, entropy_bad)
        total_redone += stats["redone"]
    assert total_redone >= 4


def test_trailing_bytes_are_ignored(engine):
    cases = P.extra_byte_files()
    for tag in ("420", "gray-flat", "444rstrow"):
        decode_and_check(engine, [b for n, b in cases if n.startswith(tag + "-extra")])


def test_unknown_flag_bits_are_refused_without_launching(engine):
    blob = P.photo_matrix()[0][1]
    ptrs, lens = (C.c_char_p * 1)(blob), (C.c_size_t * 1)(len(blob))
    out, status = np.full((203, 157, 3), 0xA5, np.uint8), np.full(1, 77, np.int32)
    rc = engine.lib.fe_jpeg_decode_ex(engine.h, ptrs, lens, 1, 203, 157, 0, 1, 0, 0x100 | 0x40, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
    assert rc != 0 and (out == 0xA5).all() and status[0] == 77
    info = (C.c_int32 * 10)()
    assert engine.lib.fe_jpeg_probe_ex(blob, len(blob), 0x100, info) == 0 and info[7] == 0 and info[0] == 157      # accepted and ignored
    assert engine.lib.fe_jpeg_probe_ex(blob, len(blob), 0x40, info) != 0


def test_process_files_gives_the_same_records():
    from facet_amd import Engine
    from facet_amd.batch import BatchScorer
    from facet_amd._lib import FE_MODEL_TOPIQ
    from facet_amd.weights import synthetic_state_dict
    engine = Engine(0, arena_bytes=2 << 30)      # its own context: the session's carries no models
    engine.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
    h, w = 96, 128
    imgs = [P.photo(h, w, 20 + k) for k in range(4)]
    blobs = [J.encode(imgs[0], quality=85, subsampling=2), J.encode(imgs[1], quality=75, subsampling=1, restart_marker_rows=1),
             J.encode(imgs[2], quality=95, subsampling=0, optimize=True), J.encode(np.rot90(imgs[3]).copy(), quality=85, exif=J.exif_bytes(6))]
    scorer = BatchScorer(engine, phash=True)
    want = scorer.process_files(blobs)
    got = scorer.process_files(blobs, parallel_entropy=True)
    stats = engine.jpeg_entropy_stats()
    engine.close()
    assert stats["parallel_segments"] > 0 and stats["redone"] == 0
    assert len(got) == 4
    for g, r in zip(got, want):
        assert g.keys() == r.keys()
        for key in r:
            assert np.array_equal(g[key], r[key]) if isinstance(r[key], np.ndarray) else g[key] == r[key], key
