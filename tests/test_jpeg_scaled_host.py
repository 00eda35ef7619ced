"""CPU: the scaled JPEG decode (libjpeg's 1/2, 1/4, 1/8, which Pillow's draft() asks for) from jpeg_dec_core.h's functions in a harness
compiled under AddressSanitizer + UBSan, pixel for pixel against Pillow's drafted image; damaged files end with a status and no
sanitizer report; fe_jpeg_scaled_size and the Pillow fallback of decode_jpegs(scale=...). Every equality is exact."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_scaled_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("jpegscaled") / "jpeg_scaled_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "jpeg_scaled_harness.cpp"), "-o", exe], check=True)
    return exe


def run_harness(exe, jobs, tmp, bgr=0, apply_orientation=1, flags=0):
    """jobs: [(scale, blob)] -> [(status, pixels | None)]"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("4i", len(jobs), bgr, apply_orientation, flags))
        for scale, b in jobs:
            f.write(struct.pack("iI", scale, len(b)))
            f.write(b)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(fout, "rb").read()
    out, o = [], 0
    for _ in jobs:
        st, oh, ow = struct.unpack_from("3i", raw, o)
        o += 12
        px = None
        if st == 0:
            px = np.frombuffer(raw, np.uint8, oh * ow * 3, o).reshape(oh, ow, 3)
            o += oh * ow * 3
        out.append((st, px))
    assert o == len(raw)
    return out


def test_host_scaled_decode_equals_pillow_draft_on_the_matrix(harness, tmp_path):
    cases = S.files()
    assert len(cases) == 7 * 4 * 3 * 2 * 2
    jobs = [(s, b) for _, b in cases for s in S.SCALES]
    names = [f"{n}/{s}" for n, _ in cases for s in S.SCALES]
    res = run_harness(harness, jobs, str(tmp_path))
    bad = [name for name, (s, b), (st, px) in zip(names, jobs, res) if st != 0 or not np.array_equal(px, S.pillow_scaled(b, s))]
    assert not bad, (len(bad), bad[:20])


def test_host_scaled_decode_differs_from_full_decode_then_reduce(harness, tmp_path):
    """The scaled transform is arithmetic of its own: box-reducing the full decode gives other pixels, so the matrix test tells them apart."""
    from PIL import Image
    blob = S.file_of(97, 131, "4:2:0", "noise", 95, False)
    (st, px), = run_harness(harness, [(2, blob)], str(tmp_path))
    reduced = np.asarray(Image.fromarray(J.pillow_pixels(blob)).reduce(2))
    assert st == 0 and px.shape == reduced.shape and not np.array_equal(px, reduced)


def test_host_scaled_progressive_subset(harness, tmp_path):
    cases = S.progressive_files()
    jobs = [(s, b) for _, b in cases for s in S.SCALES]
    names = [f"{n}/{s}" for n, _ in cases for s in S.SCALES]
    res = run_harness(harness, jobs, str(tmp_path), flags=1)
    bad = [name for name, (s, b), (st, px) in zip(names, jobs, res) if st != 0 or not np.array_equal(px, S.pillow_scaled(b, s))]
    assert not bad, (len(bad), bad[:20])
    assert all(st == 1 for st, _ in run_harness(harness, jobs[:6], str(tmp_path)))          # without the flag: left to the caller


def test_host_scale_1_is_the_unscaled_decode(harness, tmp_path):
    cases = [c for c in J.matrix() if c[0].startswith(("53x37", "7x9"))]
    res = run_harness(harness, [(1, b) for _, b in cases], str(tmp_path))
    for (name, blob), (st, px) in zip(cases, res):
        assert st == 0 and np.array_equal(px, J.pillow_pixels(blob)), name


def test_host_scaled_orientations_and_bgr(harness, tmp_path):
    a = J.content("gradient", 21, 30)
    blobs = [J.encode(a, quality=90, subsampling=s, exif=J.exif_bytes(o, be)) for o in range(1, 9) for s in (0, 1, 2) for be in (False, True)]
    for scale in S.SCALES:
        for (st, px), blob in zip(run_harness(harness, [(scale, b) for b in blobs], str(tmp_path)), blobs):
            assert st == 0 and np.array_equal(px, S.pillow_scaled(blob, scale, transpose=True))
        for (st, px), blob in zip(run_harness(harness, [(scale, b) for b in blobs], str(tmp_path), bgr=1, apply_orientation=0), blobs):
            assert st == 0 and np.array_equal(px, S.pillow_scaled(blob, scale)[..., ::-1])


def test_host_scaled_damaged_files_end_with_a_status(harness, tmp_path):
    """Truncated and bit-flipped files: a status, never a sanitizer report (returncode 0), at every scale."""
    cases = J.damaged()
    jobs = [(s, b) for _, b in cases for s in S.SCALES]
    res = run_harness(harness, jobs, str(tmp_path))
    for k, ((s, blob), (st, px)) in enumerate(zip(jobs, res)):
        name = cases[k // len(S.SCALES)][0]
        assert st <= 0, (name, s, st)
        if "cut" in name:
            assert st < 0, (name, s, st)
        if st == 0:                                                           # overwritten bytes that still form an honest stream
            want = S.pillow_scaled(blob, s)
            assert px.shape == want.shape, (name, s)


def test_scaled_size_helper():
    from facet_amd import Engine
    for (h, w) in S.SIZES + [(427, 640), (4000, 6000)]:
        for s in (1, 2, 4, 8):
            assert Engine.jpeg_scaled_size(h, w, s) == S.scaled_size(h, w, s)
    for bad in (0, 3, 16, -2):
        with pytest.raises(ValueError):
            Engine.jpeg_scaled_size(10, 10, bad)


class _UnsupportedEngine:
    """Reports every file unsupported, so everything must come from Pillow."""
    def jpeg_probe(self, blob, progressive=False):
        return dict(width=0, height=0, components=0, hsamp=1, vsamp=1, restart_interval=0, orientation=1, status=1)

    def jpeg_decode(self, *a, **k):
        raise AssertionError("nothing is decodable for this engine")


def test_decode_jpegs_scaled_falls_back_to_drafted_pillow():
    from facet_amd.image_loading import decode_jpegs
    blobs = [S.file_of(53, 37, "4:2:0", "noise", 95, False), S.file_of(17, 33, "gray", "gradient", 30, False),
             J.encode(J.content("gradient", 20, 30), exif=J.exif_bytes(6)), b"not an image"]
    for scale in (2, 4, 8):
        got = decode_jpegs(_UnsupportedEngine(), blobs, scale=scale)
        assert got[3] is None
        for k in range(3):
            assert np.array_equal(got[k], S.pillow_scaled(blobs[k], scale, transpose=True)), (scale, k)
    with pytest.raises(ValueError):
        decode_jpegs(_UnsupportedEngine(), blobs, scale=3)
