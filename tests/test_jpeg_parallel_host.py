"""CPU: the parallel entropy decode of jpeg_dec_core.h (self-synchronising Huffman decoding inside a segment), run with the lanes as
loops by a harness compiled under AddressSanitizer + UBSan, pixel for pixel against Pillow and against the serial decode of the same
harness run. Valid files never take the serial redo; damaged ones end with the serial decoder's status and no sanitizer report. Every
equality is exact."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_parallel_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("jpegpar") / "jpeg_parallel_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "jpeg_parallel_harness.cpp"), "-o", exe], check=True)
    return exe


def run_harness(exe, blobs, tmp, sub, bgr=0, apply_orientation=1):
    """[dict(parsed, status, px, serial_status, serial_px, rounds, redone, segments, subsequences)] per file; parsed: the parser took it."""
    fin, fout = os.path.join(tmp, f"in{sub}.bin"), os.path.join(tmp, f"out{sub}.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("4i", len(blobs), bgr, apply_orientation, sub))
        for b in blobs:
            f.write(struct.pack("I", len(b)))
            f.write(b)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(fout, "rb").read()
    out, o = [], 0
    for _ in blobs:
        st, oh, ow, sst, rounds, redone, segs, subs = struct.unpack_from("8i", raw, o)
        o += 32
        px = [None, None]
        for k, s in enumerate((st, sst)):
            if s == 0:
                px[k] = np.frombuffer(raw, np.uint8, oh * ow * 3, o).reshape(oh, ow, 3)
                o += oh * ow * 3
        out.append(dict(parsed=oh > 0, status=st, px=px[0], serial_status=sst, serial_px=px[1], rounds=rounds, redone=redone, segments=segs, subsequences=subs))
    assert o == len(raw)
    return out


def check_honest(cases, res, sub):
    bad = [name for (name, blob), r in zip(cases, res)
           if r["status"] != 0 or r["redone"] != 0 or not np.array_equal(r["px"], J.pillow_pixels(blob))]
    assert not bad, (sub, bad[:20])
    for (name, blob), r in zip(cases, res):
        assert (r["segments"], r["subsequences"]) == P.expected_stats([blob], sub), (sub, name)
        assert r["rounds"] <= max([-(-(e - s) // sub) for s, e in P.segments(blob)]), (sub, name)


@pytest.mark.parametrize("sub", [16, 32, 128])
def test_matrix_equals_pillow_and_never_falls_back(harness, tmp_path, sub):
    cases = J.matrix()
    res = run_harness(harness, [b for _, b in cases], str(tmp_path), sub)
    check_honest(cases, res, sub)
    assert sum(r["segments"] for r in res) > (400 if sub == 16 else 100)      # the path under test ran


@pytest.mark.parametrize("sub", [16, 128])
def test_gpu_cases_equal_pillow(harness, tmp_path, sub):
    cases = P.gpu_cases()
    res = run_harness(harness, [b for _, b in cases], str(tmp_path), sub)
    check_honest(cases, res, sub)
    for (name, _), r in zip(cases, res):
        print(f"[parallel entropy, S={sub}] {name}: {r['segments']} segments, {r['subsequences']} subsequences, {r['rounds']} rounds")
    if sub == P.SUB:
        by = {name: r for (name, _), r in zip(cases, res)}
        assert by["8x8-gray"]["segments"] == 0 and by["16x16-420"]["segments"] == 0
        assert by["photo-4:4:4-rst3"]["segments"] == 0 and by["photo-gray-rst3"]["segments"] == 0
        assert by["photo-4:2:0-rstrow"]["segments"] == 13 and by["stuffed"]["segments"] == 1
        # A lane that guessed the component wrong falls into step inside its own subsequence (sub_pass drops a bit or ends the block
        # where a wrong guess meets a code in no table or a run past 63), so a photo without restart markers settles in a few rounds,
        # not in one per subsequence: a block of these files is 10 to 20 times shorter than a subsequence. A quarter of the
        # subsequence count is far above what that needs and far below what giving up on such a pass costs (one round each).
        for name in ("photo-4:4:4", "photo-4:2:2", "photo-4:2:0", "photo-gray"):
            assert by[name]["segments"] == 1 and 4 * by[name]["rounds"] <= by[name]["subsequences"], (name, by[name]["rounds"], by[name]["subsequences"])


def test_orientations_and_bgr(harness, tmp_path):
    a = P.photo(40, 56, 3)
    blobs = [J.encode(a, quality=90, subsampling=2, exif=J.exif_bytes(o)) for o in range(1, 9)]
    for r, blob in zip(run_harness(harness, blobs, str(tmp_path), 16), blobs):
        assert r["status"] == 0 and r["redone"] == 0 and r["segments"] == 1 and np.array_equal(r["px"], J.pillow_pixels(blob))
    for r, blob in zip(run_harness(harness, blobs, str(tmp_path), 16, bgr=1, apply_orientation=0), blobs):
        assert r["status"] == 0 and np.array_equal(r["px"], J.pillow_pixels(blobs[0])[..., ::-1])


@pytest.mark.parametrize("sub", [16, 128])
def test_damaged_files_and_trailing_bytes_end_as_the_serial_decoder_does(harness, tmp_path, sub):
    cases = J.damaged() + P.extra_byte_files()
    res = run_harness(harness, [b for _, b in cases], str(tmp_path), sub)          # returncode 0: no sanitizer report
    redone = 0
    for (name, blob), r in zip(cases, res):
        assert r["status"] == r["serial_status"], (name, r["status"], r["serial_status"])
        assert r["status"] <= 0, name
        if r["status"] == 0:
            assert np.array_equal(r["px"], r["serial_px"]) and np.array_equal(r["px"], J.pillow_pixels(blob)), name
        if "extra" in name:
            assert r["status"] == 0 and r["redone"] == 0, name
        assert r["redone"] == (1 if r["status"] in (-2, -3) and r["parsed"] else 0), name      # decoded again exactly when the entropy stage refuses it
        redone += r["redone"]
    assert redone > 10                                                             # cut files reach step 4 and are decoded again


def test_random_small_images_equal_pillow(harness, tmp_path):
    cases = P.random_small(200)
    res = run_harness(harness, [b for _, b in cases], str(tmp_path), 16)
    check_honest(cases, res, 16)
    worst = max(zip(res, cases), key=lambda t: t[0]["rounds"])
    print(f"[parallel entropy, S=16] 200 random files, {sum(r['segments'] for r in res)} parallel segments, "
          f"largest round count {worst[0]['rounds']} ({worst[1][0]}, {worst[0]['subsequences']} subsequences)")
    assert sum(r["segments"] for r in res) >= 200
