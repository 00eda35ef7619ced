"""CPU: the progressive side of the JPEG decoder's host code. fe_jpeg_probe_ex through the built library; the scan parser and the four
jdphuff.c scan procedures of jpeg_dec_core.h in a harness compiled under AddressSanitizer + UBSan, pixel for pixel against Pillow;
incomplete progressions are refused; damaged files end with a status and no sanitizer report; decode_jpegs(progressive=True) falls back
to Pillow in input order. Every equality is exact."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as J
import jpeg_prog_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def probe(blob, progressive=False):
    from facet_amd import Engine
    return Engine.jpeg_probe(blob, progressive=True) if progressive else Engine.jpeg_probe(blob)


# ---- fe_jpeg_probe_ex --------------------------------------------------------------------------------------------------------------
def test_probe_plain_is_1_and_flagged_is_0_with_size_and_scans():
    cases = G.matrix()
    assert len(cases) == G.MATRIX_SIZE
    for name, blob in cases + [("eobrun", G.long_eobrun())]:
        assert probe(blob)["status"] == 1, name
        p = probe(blob, True)
        im = Image.open(io.BytesIO(blob))
        gray = im.mode == "L"
        assert (p["status"], p["progressive"], p["width"], p["height"], p["components"]) == (0, 1, im.size[0], im.size[1], 1 if gray else 3), name
        assert p["scans"] == (6 if gray else 10), name
    for o, blob in enumerate(G.oriented(), start=1):
        assert probe(blob)["status"] == 1
        p = probe(blob, True)
        assert (p["status"], p["orientation"], p["width"], p["height"], p["scans"]) == (0, o, 30, 20, 10)


def test_probe_restart_interval_is_the_scans_own():
    """Pillow's restart_marker_rows writes DRI 3 in front of the interleaved scans and DRI 5 in front of the others of a 4:2:0 file 37
    pixels wide: the probe reports the first scan's, and the decode (below) needs each."""
    blob = G.encode(J.content("bands", 53, 37), quality=95, subsampling=2, restart_marker_rows=1)
    dri = [(blob[i + 4] << 8) | blob[i + 5] for i in range(len(blob) - 5) if blob[i:i + 4] == b"\xff\xdd\x00\x04"]
    assert dri[:4] == [3, 5, 3, 5]
    assert probe(blob, True)["restart_interval"] == 3


def test_flagged_probe_of_other_files_equals_the_plain_probe():
    a = J.content("gradient", 33, 17)
    cmyk = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(cmyk, "JPEG", progressive=True)
    blobs = [b for _, b in J.matrix()[::37]] + [J.encode(a, exif=J.exif_bytes(6)), J.encode(a[..., 0], restart_marker_blocks=2), b"", b"\xff\xd8\xff\xd9",
                                                 bytes(range(256)) * 4]
    for blob in blobs:
        p = probe(blob, True)
        assert (p.pop("progressive"), p.pop("scans")) == (0, 0)
        assert p == probe(blob)
    assert probe(cmyk.getvalue(), True)["status"] == 4      # progressive CMYK stays Pillow's


def test_incomplete_progressions_are_refused():
    """The file cut in front of the tables of scan k and closed with EOI is a valid JPEG file that Pillow decodes to other, smoothed
    pixels: the probe must not take it."""
    src = G.encode(J.content("gradient", 48, 64), quality=85, subsampling=2)
    want = J.pillow_pixels(src)
    n = len(G.scans(src))
    assert n == 10 and probe(src, True)["status"] == 0
    for k in range(1, n):
        blob = G.cut_before_scan(src, k)
        px = J.pillow_pixels(blob)
        assert px is not None and not np.array_equal(px, want), k
        p = probe(blob, True)
        assert p["status"] > 0 and p["scans"] == k, (k, p)
        assert probe(blob)["status"] == 1


def _sos_patched(blob, scan, offset_from_end, value):
    """blob with one byte of the SOS header of scan `scan` (0-based) replaced; offset_from_end: 3 Ss, 2 Se, 1 Ah/Al."""
    _, a, _ = G.scans(blob)[scan]
    x = bytearray(blob)
    x[a - offset_from_end] = value
    return bytes(x)


def test_scan_parameter_and_progression_rules():
    src = G.encode(J.content("noise", 17, 33), quality=75, subsampling=1)
    assert probe(_sos_patched(src, 0, 2, 5), True)["status"] < 0           # Ss = 0 with Se = 5
    assert probe(_sos_patched(src, 1, 2, 64), True)["status"] < 0          # Se = 64
    assert probe(_sos_patched(src, 1, 1, 0x0E), True)["status"] < 0        # Al = 14
    assert probe(_sos_patched(src, 5, 1, 0x31), True)["status"] < 0        # Ah = 3, Al = 1
    assert probe(_sos_patched(src, 1, 1, 0x01), True)["status"] > 0        # first AC scan at Al = 1, refined later from Ah = 2
    assert probe(_sos_patched(src, 5, 1, 0x10), True)["status"] > 0        # a refinement from Ah = 1 of coefficients left at 2
    tables, _, _ = G.scans(src)[1]
    dqt = src[src.index(b"\xff\xdb"):src.index(b"\xff\xdb") + 69]
    assert probe(src[:tables] + dqt + src[tables:], True)["status"] > 0    # DQT behind the first SOS
    sc = G.scans(src)
    assert probe(src[:-2] + src[sc[9][0]:sc[9][2]] + b"\xff\xd9", True)["status"] > 0      # the last scan twice: nothing is left to refine


# ---- the decode from jpeg_dec_core.h, sanitized ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("jpegprog") / "jpeg_prog_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "jpeg_prog_harness.cpp"), "-o", exe], check=True)
    return exe


def run_harness(exe, blobs, tmp, bgr=0, apply_orientation=1, flags=1):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("4i", len(blobs), bgr, apply_orientation, flags))
        for b in blobs:
            f.write(struct.pack("I", len(b)))
            f.write(b)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(fout, "rb").read()
    out, o = [], 0
    for _ in blobs:
        st, oh, ow = struct.unpack_from("3i", raw, o)
        o += 12
        px = None
        if st == 0:
            px = np.frombuffer(raw, np.uint8, oh * ow * 3, o).reshape(oh, ow, 3)
            o += oh * ow * 3
        out.append((st, px))
    assert o == len(raw)
    return out


def test_host_decode_equals_pillow_on_the_matrix(harness, tmp_path):
    cases = G.matrix()
    res = run_harness(harness, [b for _, b in cases], str(tmp_path))
    bad = [name for (name, blob), (st, px) in zip(cases, res) if st != 0 or not np.array_equal(px, J.pillow_pixels(blob))]
    assert not bad, bad[:20]
    plain = run_harness(harness, [b for _, b in cases[::9]], str(tmp_path), flags=0)
    assert all(st == 1 for st, _ in plain)


def test_host_decode_baseline_files_through_the_flagged_parser(harness, tmp_path):
    cases = J.matrix()[::5]
    res = run_harness(harness, [b for _, b in cases], str(tmp_path))
    bad = [name for (name, blob), (st, px) in zip(cases, res) if st != 0 or not np.array_equal(px, J.pillow_pixels(blob))]
    assert not bad, bad[:20]


def test_host_decode_orientations_and_bgr(harness, tmp_path):
    blobs = G.oriented()
    for (st, px), blob in zip(run_harness(harness, blobs, str(tmp_path)), blobs):
        assert st == 0 and np.array_equal(px, J.pillow_pixels(blob))
    for (st, px), blob in zip(run_harness(harness, blobs, str(tmp_path), bgr=1), blobs):
        assert st == 0 and np.array_equal(px, J.pillow_pixels(blob)[..., ::-1])
    for (st, px), blob in zip(run_harness(harness, blobs, str(tmp_path), bgr=1, apply_orientation=0), blobs):
        want = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))[..., ::-1]
        assert st == 0 and np.array_equal(px, want)


def test_host_decode_end_of_band_run_over_16384_blocks(harness, tmp_path):
    blob = G.long_eobrun()
    (st, px), = run_harness(harness, [blob], str(tmp_path))
    assert st == 0 and np.array_equal(px, J.pillow_pixels(blob))


def test_host_decode_incomplete_progressions_keep_their_positive_status(harness, tmp_path):
    src = G.encode(J.content("gradient", 48, 64), quality=85, subsampling=2)
    res = run_harness(harness, [G.cut_before_scan(src, k) for k in range(1, 10)], str(tmp_path))
    assert all(st > 0 for st, _ in res), [st for st, _ in res]


def test_host_decode_damaged_files_end_with_a_status(harness, tmp_path):
    cases = G.damaged()
    assert len(cases) == 3 * 4 * 12
    res = run_harness(harness, [b for _, b in cases], str(tmp_path))          # returncode 0: no sanitizer report
    for (name, blob), (st, px) in zip(cases, res):
        assert st <= 0, (name, st)
        if "cut" in name:
            assert st < 0, (name, st)
        if st == 0:                                                           # overwritten bytes that still form an honest stream
            assert np.array_equal(px, J.pillow_pixels(blob)), name


# ---- decode_jpegs ------------------------------------------------------------------------------------------------------------------
class _RefusingEngine:
    """Refuses every file, with or without the flag, so everything must come from Pillow."""
    def __init__(self):
        self.flagged = 0

    def jpeg_probe(self, blob, progressive=False):
        self.flagged += bool(progressive)
        return dict(width=0, height=0, components=0, hsamp=1, vsamp=1, restart_interval=0, orientation=1, status=8 if progressive else 1,
                    progressive=1, scans=0)

    def jpeg_decode(self, *a, **k):
        raise AssertionError("nothing is decodable for this engine")


def test_decode_jpegs_progressive_falls_back_to_pillow_in_input_order(tmp_path):
    from facet_amd.image_loading import decode_jpegs, load_image_from_path
    a, b = J.content("gradient", 20, 30), J.content("noise", 17, 33)
    png = io.BytesIO()
    Image.fromarray(b).save(png, "PNG")
    blobs = [G.encode(a, quality=80), png.getvalue(), G.encode(a, exif=J.exif_bytes(6)), b"not an image", G.encode(b[..., 0]), J.encode(b, quality=70)]
    eng = _RefusingEngine()
    got = decode_jpegs(eng, blobs, progressive=True)
    assert eng.flagged == len(blobs)                  # each status 1 was asked again with the flag
    assert got[3] is None
    for k in (0, 1, 2, 4, 5):
        assert np.array_equal(got[k], J.pillow_pixels(blobs[k])), k
    assert got[2].shape == (30, 20, 3)
    f = tmp_path / "x.jpg"
    f.write_bytes(blobs[2])
    pil, cv = load_image_from_path(_RefusingEngine(), f, progressive=True)
    assert pil.size == (20, 30) and np.array_equal(cv[..., ::-1], J.pillow_pixels(blobs[2]))
