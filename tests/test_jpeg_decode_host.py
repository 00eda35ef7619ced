"""CPU: the JPEG decoder's host side. fe_jpeg_probe through the built library; the whole decode from jpeg_dec_core.h's functions in a
harness compiled under AddressSanitizer + UBSan, pixel for pixel against Pillow; damaged files end with a status and no sanitizer
report; decode_jpegs falls back to Pillow in input order. Every equality is exact: baseline decoding is integer arithmetic."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def probe(blob):
    from facet_amd import Engine
    return Engine.jpeg_probe(blob)


# ---- fe_jpeg_probe -----------------------------------------------------------------------------------------------------------------
def test_probe_geometry():
    a = J.content("gradient", 53, 37)
    for sname, (hs, vs) in {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}.items():
        p = probe(J.encode(a, quality=80, subsampling=J.SUBSAMPLING[sname]))
        assert p == dict(width=37, height=53, components=3, hsamp=hs, vsamp=vs, restart_interval=0, orientation=1, status=0), sname
    p = probe(J.encode(a[..., 0], quality=80))
    assert (p["components"], p["hsamp"], p["vsamp"], p["status"]) == (1, 1, 1, 0)
    assert probe(J.encode(a, subsampling=2, restart_marker_blocks=3))["restart_interval"] == 3
    assert probe(J.encode(a, subsampling=2, restart_marker_rows=1))["restart_interval"] == 3          # ceil(37 / 16) MCUs per row
    assert probe(J.encode(a, subsampling=0, restart_marker_rows=2))["restart_interval"] == 10         # 2 x ceil(37 / 8)
    assert probe(J.encode(a, quality=90, optimize=True))["status"] == 0
    qt = [int(v) for v in np.linspace(300, 1000, 64)]                                                 # 16-bit DQT entries (SOF1)
    p = probe(J.encode(a, qtables=[qt, qt], subsampling=0))
    assert p["status"] == 0


@pytest.mark.parametrize("big_endian", [False, True])
def test_probe_orientations(big_endian):
    a = J.content("gradient", 20, 30)
    for o in range(1, 9):
        p = probe(J.encode(a, exif=J.exif_bytes(o, big_endian)))
        assert (p["orientation"], p["status"], p["width"], p["height"]) == (o, 0, 30, 20)
    assert probe(J.encode(a, exif=J.exif_bytes(9)))["orientation"] == 1          # no transpose for a value Pillow does not know


def _with_adobe_rgb(blob):
    """The same scan declared as RGB: an APP14 Adobe marker with transform 0 in place of the JFIF marker."""
    assert blob[2:4] == b"\xff\xe0"
    n = (blob[4] << 8) | blob[5]
    return blob[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + blob[4 + n:]


def _patched(blob, marker, offset, value):
    """blob with the byte `offset` bytes into the payload of the first `marker` segment replaced."""
    i = 2
    while True:
        assert blob[i] == 0xFF
        n = (blob[i + 2] << 8) | blob[i + 3]
        if blob[i + 1] == marker:
            x = bytearray(blob)
            x[i + 4 + offset] = value
            return bytes(x)
        i += 2 + n


def test_probe_unsupported_kinds_by_code():
    a = J.content("gradient", 33, 17)
    base = J.encode(a, quality=80, subsampling=0)
    assert probe(J.encode(a, progressive=True))["status"] == 1
    x = bytearray(base)
    x[base.index(b"\xff\xc0") + 1] = 0xC9                                             # SOF9: arithmetic coding
    assert probe(bytes(x))["status"] == 2
    assert probe(_patched(base, 0xC0, 0, 12))["status"] == 3                          # 12-bit precision
    buf = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(buf, "JPEG")
    assert probe(buf.getvalue())["status"] == 4
    assert probe(_with_adobe_rgb(base))["status"] == 5
    assert probe(_patched(base, 0xC0, 7, 0x12))["status"] == 6                        # luma 1x2: 4:4:0
    assert probe(_patched(base, 0xC0, 7, 0x41))["status"] == 6                        # luma 4x1: 4:1:1
    # a baseline file with one scan per component: the first scan names one component of three
    sos = base.index(b"\xff\xda")
    multi = base[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + base[sos + 14:]
    assert probe(multi)["status"] == 7
    for blob in (J.encode(a, progressive=True), buf.getvalue()):                      # a frame header was read: the size is reported
        assert (probe(blob)["width"], probe(blob)["height"]) == (17, 33)


def test_probe_garbage_and_empty():
    assert probe(b"")["status"] < 0
    assert probe(b"\xff")["status"] < 0
    assert probe(b"\xff\xd8")["status"] < 0
    assert probe(b"\xff\xd8\xff\xd9")["status"] < 0
    assert probe(bytes(range(256)) * 4)["status"] < 0
    buf = io.BytesIO()
    Image.fromarray(J.content("noise", 8, 8)).save(buf, "PNG")
    assert probe(buf.getvalue())["status"] == -1
    base = J.encode(J.content("noise", 16, 16))
    for cut in range(2, len(base) - 2, 7):                                           # every prefix is judged without reading past it
        assert probe(base[:cut])["status"] < 0, cut
    rng = np.random.default_rng(0)
    for _ in range(200):                                                             # header bytes overwritten: any status, no crash
        x = bytearray(base)
        for _ in range(3):
            x[int(rng.integers(2, J.entropy_span(base)[0]))] = int(rng.integers(0, 256))
        assert -6 <= probe(bytes(x))["status"] <= 8


# ---- the decode from jpeg_dec_core.h, sanitized ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("jpegdec") / "jpeg_decode_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "jpeg_decode_harness.cpp"), "-o", exe], check=True)
    return exe


def run_harness(exe, blobs, tmp, bgr=0, apply_orientation=1):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", len(blobs), bgr, apply_orientation))
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
    cases = J.matrix()
    assert len(cases) == 8 * 3 * 5 * 4 + 8 * (3 * 5 + 4)
    res = run_harness(harness, [b for _, b in cases], str(tmp_path))
    bad = [name for (name, blob), (st, px) in zip(cases, res) if st != 0 or not np.array_equal(px, J.pillow_pixels(blob))]
    assert not bad, bad[:20]


def test_host_decode_small_widths_long_codes_and_16bit_tables(harness, tmp_path):
    blobs = []
    for (h, w) in [(3, 2), (5, 3), (2, 4), (9, 5), (4, 6), (1, 17), (19, 1)]:      # chroma 1 .. 3 samples wide: replicated / filtered
        for s in (0, 1, 2):
            blobs.append(J.encode(J.content("noise", h, w, 2), quality=90, subsampling=s))
    qt = [int(v) for v in np.linspace(300, 1000, 64)]
    blobs.append(J.encode(J.content("gradient", 33, 17), qtables=[qt, qt], subsampling=2))
    blobs.append(J.encode(J.content("noise", 64, 64, 3), quality=100, subsampling=0, optimize=True))
    res = run_harness(harness, blobs, str(tmp_path))
    for k, (blob, (st, px)) in enumerate(zip(blobs, res)):
        assert st == 0 and np.array_equal(px, J.pillow_pixels(blob)), k


def test_host_decode_orientations_and_bgr(harness, tmp_path):
    a = J.content("gradient", 20, 30)
    blobs = [J.encode(a, quality=90, subsampling=s, exif=J.exif_bytes(o, be)) for o in range(1, 9) for s in (0, 2) for be in (False, True)]
    for (st, px), blob in zip(run_harness(harness, blobs, str(tmp_path)), blobs):
        assert st == 0 and np.array_equal(px, J.pillow_pixels(blob))
    for (st, px), blob in zip(run_harness(harness, blobs, str(tmp_path), bgr=1, apply_orientation=0), blobs):
        want = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))[..., ::-1]
        assert st == 0 and np.array_equal(px, want)


def test_host_decode_damaged_files_end_with_a_status(harness, tmp_path):
    cases = J.damaged()
    res = run_harness(harness, [b for _, b in cases], str(tmp_path))          # returncode 0: no sanitizer report
    for (name, blob), (st, px) in zip(cases, res):
        assert st <= 0, (name, st)
        if "cut" in name:
            assert st < 0, (name, st)
        if st == 0:                                                           # overwritten bytes that still form an honest stream
            assert np.array_equal(px, J.pillow_pixels(blob)), name


# ---- decode_jpegs ------------------------------------------------------------------------------------------------------------------
class _UnsupportedEngine:
    """Reports every file unsupported, so everything must come from Pillow."""
    def jpeg_probe(self, blob):
        return dict(width=0, height=0, components=0, hsamp=1, vsamp=1, restart_interval=0, orientation=1, status=1)

    def jpeg_decode(self, *a, **k):
        raise AssertionError("nothing is decodable for this engine")


def test_decode_jpegs_falls_back_to_pillow_in_input_order():
    from facet_amd.image_loading import decode_jpegs
    a, b = J.content("gradient", 20, 30), J.content("noise", 17, 33)
    png = io.BytesIO()
    Image.fromarray(b).save(png, "PNG")
    blobs = [J.encode(a, quality=80), png.getvalue(), J.encode(a, exif=J.exif_bytes(6)), b"not an image", J.encode(b[..., 0], progressive=True)]
    got = decode_jpegs(_UnsupportedEngine(), blobs)
    assert got[3] is None
    for k in (0, 1, 2, 4):
        assert np.array_equal(got[k], J.pillow_pixels(blobs[k])), k
    assert got[2].shape == (30, 20, 3) and np.array_equal(got[1], b)


def test_raw_suffix_is_refused(tmp_path):
    from facet_amd.image_loading import load_image_from_path, read_blob
    for name in ("a.CR2", "b.cr3"):
        with pytest.raises(ValueError):
            read_blob(str(tmp_path / name))
        with pytest.raises(ValueError):
            load_image_from_path(_UnsupportedEngine(), tmp_path / name)
    f = tmp_path / "x.jpg"
    f.write_bytes(J.encode(J.content("gradient", 20, 30), exif=J.exif_bytes(8)))
    pil, cv = load_image_from_path(_UnsupportedEngine(), f)
    assert pil.size == (20, 30) and np.array_equal(cv[..., ::-1], J.pillow_pixels(f.read_bytes()))
    assert load_image_from_path(_UnsupportedEngine(), tmp_path / "missing.jpg") == (None, None)
