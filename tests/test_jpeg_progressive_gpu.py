"""GPU: fe_jpeg_decode_ex with FE_JPEG_PROGRESSIVE against Pillow, pixel for pixel. The files (tests/jpeg_prog_cases.py) are the ones the
sanitized host harness of test_jpeg_progressive_host.py decodes with the very functions the scan kernel is built from."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as J
import jpeg_prog_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def groups():
    """{(h, w): [(name, blob, pillow pixels)]} by decoded size: the matrix and the eight orientations."""
    out = {}
    for name, blob in G.matrix() + [(f"orient{o}", b) for o, b in enumerate(G.oriented(), start=1)]:
        px = J.pillow_pixels(blob)
        out.setdefault(px.shape[:2], []).append((name, blob, px))
    return out


def test_matrix_equals_pillow_host_destination(engine, groups):
    assert sum(len(g) for g in groups.values()) == G.MATRIX_SIZE + 8
    for (h, w), group in groups.items():
        got, status = engine.jpeg_decode([b for _, b, _ in group], h, w, progressive=True)
        assert not status.any(), [(n, int(s)) for (n, _, _), s in zip(group, status) if s]
        bad = [n for k, (n, _, px) in enumerate(group) if not np.array_equal(got[k], px)]
        assert not bad, bad[:10]


def test_matrix_equals_pillow_device_destination_and_bgr(engine, groups):
    for (h, w), group in groups.items():
        dev, status = engine.jpeg_decode([b for _, b, _ in group], h, w, bgr=True, device=True, progressive=True)
        try:
            got = np.empty((len(group), h, w, 3), np.uint8)
            engine.d2h(got, dev[0])
        finally:
            engine.dev_free(dev[0])
        assert not status.any()
        bad = [n for k, (n, _, px) in enumerate(group) if not np.array_equal(got[k], px[..., ::-1])]
        assert not bad, bad[:10]


def test_end_of_band_run_over_16384_blocks(engine):
    blob = G.long_eobrun()
    got, status = engine.jpeg_decode([blob], 1024, 1024, progressive=True)
    assert status.tolist() == [0] and np.array_equal(got[0], J.pillow_pixels(blob))


def test_one_call_mixes_baseline_and_progressive(engine):
    h, w = 53, 37
    a = [J.content(k, h, w, 5) for k in ("noise", "gradient", "bands", "sparse")]
    blobs = [J.encode(a[0], quality=30, subsampling=2), G.encode(a[1], quality=95, subsampling=0),
             J.encode(a[2], quality=75, subsampling=1, restart_marker_blocks=1), G.encode(a[3], quality=100, subsampling=2, restart_marker_rows=1),
             G.encode(a[0][..., 0], quality=60, restart_marker_blocks=3), J.encode(a[1], quality=50, subsampling=1, optimize=True),
             G.encode(a[2], quality=85, subsampling=1, restart_marker_blocks=1), J.encode(a[0][..., 2], quality=90)]
    got, status = engine.jpeg_decode(blobs, h, w, progressive=True)
    assert not status.any()
    for k, b in enumerate(blobs):
        assert np.array_equal(got[k], J.pillow_pixels(b)), k
    got, status = engine.jpeg_decode(blobs, h, w)                          # without the flag the progressive ones keep status 1
    assert status.tolist() == [0, 1, 0, 1, 1, 0, 1, 0]
    for k in (0, 2, 5, 7):
        assert np.array_equal(got[k], J.pillow_pixels(blobs[k])), k
    for k in (1, 3, 4, 6):
        assert (got[k] == 0).all()


def test_damaged_files_get_a_status_and_neighbours_decode(engine):
    """The inputs of test_jpeg_progressive_host.py::test_host_decode_damaged_files_end_with_a_status, which the sanitized harness decodes
    without a report, between two good files in a device buffer with guard slots."""
    for tag, (src_h, src_w) in G.DAMAGED_SOURCES.items():
        bad = [(n, b) for n, b in G.damaged() if n.startswith(tag + "-")]
        good = G.encode(J.content("gradient", src_h, src_w), quality=85, subsampling=2, restart_marker_blocks=2)
        blobs = [good] + [b for _, b in bad] + [good]
        n, per = len(blobs), src_h * src_w * 3
        guard = np.full((n + 2) * per, 0x5A, np.uint8)
        d = engine.dev_alloc(guard.nbytes)
        try:
            engine.h2d(d, guard)
            _, status = engine.jpeg_decode(blobs, src_h, src_w, device=type(d)(d.value + per), progressive=True)
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
        host, hstatus = engine.jpeg_decode(blobs, src_h, src_w, progressive=True)
        assert np.array_equal(hstatus, status) and all((host[k] == 0).all() for k in range(n) if status[k] != 0)


def _mixed_list():
    h, w = 96, 128
    imgs = [J.content(k, h, w, 9) for k in ("gradient", "noise", "bands", "sparse")]
    src = G.encode(imgs[1], quality=75, subsampling=2)
    png = io.BytesIO()
    Image.fromarray(imgs[2]).save(png, "PNG")
    return [J.encode(imgs[0], quality=85, subsampling=2), G.encode(imgs[1], quality=75, subsampling=1, restart_marker_rows=1),
            G.cut_before_scan(src, 6), png.getvalue(), G.encode(np.rot90(imgs[3]).copy(), quality=85, exif=J.exif_bytes(6)), src]


def test_decode_jpegs_is_independent_of_the_flag(engine):
    from facet_amd.image_loading import decode_groups, decode_jpegs
    blobs = _mixed_list()
    off, on = decode_jpegs(engine, blobs), decode_jpegs(engine, blobs, progressive=True)
    for k, b in enumerate(blobs):
        want = J.pillow_pixels(b)
        assert np.array_equal(off[k], want) and np.array_equal(on[k], want), k
    assert decode_groups(engine, blobs)[1] == [1, 2, 3, 4, 5]              # only the baseline file is the engine's without the flag,
    assert decode_groups(engine, blobs, progressive=True)[1] == [2, 3]     # with it the incomplete progression and the PNG stay Pillow's


def test_process_files_is_independent_of_the_flag():
    from facet_amd import Engine
    from facet_amd.batch import BatchScorer
    from facet_amd._lib import FE_MODEL_TOPIQ
    from facet_amd.weights import synthetic_state_dict
    engine = Engine(0, arena_bytes=2 << 30)      # its own context: the session's carries no models
    engine.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
    blobs = _mixed_list()
    scorer = BatchScorer(engine, phash=True)
    on = scorer.process_files(blobs, progressive=True)
    off = scorer.process_files(blobs)
    engine.close()
    assert len(on) == len(off) == len(blobs)
    for g, r in zip(on, off):
        assert g.keys() == r.keys()
        for key in r:
            assert np.array_equal(g[key], r[key]) if isinstance(r[key], np.ndarray) else g[key] == r[key], key
