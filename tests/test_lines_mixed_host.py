"""CPU: lines_host_stage_mixed (facet_amd/csrc/lines_host.cpp) - hysteresis and Hough over maps of mixed sizes, images taken largest
first from a shared cursor by up to 16 threads - equals lines_host_stage image by image. Built stand-alone with AddressSanitizer + UBSan
(tests/native/lines_mixed_harness.cpp does the comparison)."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 3), (1, 7), (16, 16), (17, 31), (33, 47), (64, 65), (97, 131), (64, 300), (37, 1), (120, 77), (64, 96), (2, 2), (64, 96)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("lines_mixed") / "lines_mixed_harness")
    src = os.path.join(ROOT, "facet_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-pthread",
                    "-I", src, os.path.join(ROOT, "tests", "native", "lines_mixed_harness.cpp"), os.path.join(src, "lines_host.cpp"), "-o", exe], check=True)
    return exe


def nms_like_map(rng, h, w, kind):
    """A 2 / 0 / 1 map as the NMS kernel writes it: noise of given densities plus straight and slanted chains."""
    m = np.ones((h, w), np.uint8)
    r = rng.random((h, w))
    dens = (0.02, 0.10, 0.35)[kind % 3]
    m[r < dens] = 0
    m[r < dens * 0.3] = 2
    for _ in range(4):
        if min(h, w) < 8:
            break
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        dy, dx = rng.uniform(-1, 1), rng.uniform(-1, 1)
        for t in range(int(rng.integers(5, max(h, w)))):
            y, x = int(round(y0 + dy * t)), int(round(x0 + dx * t))
            if 0 <= y < h and 0 <= x < w:
                m[y, x] = 2 if (t % 7 == 0) else 0
    return m


def run(exe, maps, thr, min_len, max_gap, max_lines, threads, tmp):
    fin = os.path.join(tmp, "in.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("5i", len(maps), thr, max_gap, max_lines, threads))
        f.write(np.array([m.shape for m in maps], np.int32).tobytes())
        f.write(np.asarray(min_len, np.int32).tobytes())
        for m in maps:
            f.write(np.ascontiguousarray(m, np.uint8).tobytes())
    r = subprocess.run([exe, fin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = re.match(r"images=(\d+) segments=(\d+) edge_pixels=(\d+)", r.stdout)
    assert got and int(got.group(1)) == len(maps), r.stdout
    return int(got.group(2)), int(got.group(3))


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_mixed_stage_equals_per_shape_stage(harness, tmp_path, threads):
    rng = np.random.default_rng(100 + threads)
    maps = [nms_like_map(rng, h, w, k) for k, (h, w) in enumerate(SHAPES)]
    min_len = [int(min(h, w) * 0.15) for h, w in SHAPES]
    segments, edge_pixels = run(harness, maps, 8, min_len, 3, 256, threads, str(tmp_path))
    assert segments > len(SHAPES) and edge_pixels > 0      # the comparison is not of empty lists


def test_mixed_stage_with_room_for_one_line(harness, tmp_path):
    rng = np.random.default_rng(9)
    maps = [nms_like_map(rng, h, w, 2) for h, w in SHAPES]
    segments, _ = run(harness, maps, 8, [4] * len(SHAPES), 3, 1, 16, str(tmp_path))      # counts go past the room: the rest must stay untouched
    assert segments > len(SHAPES)


def test_mixed_stage_per_image_min_length(harness, tmp_path):
    """the same map twice with two minimum lengths: each image takes its own"""
    rng = np.random.default_rng(3)
    m = nms_like_map(rng, 64, 96, 1)
    short, _ = run(harness, [m, m], 8, [0, 0], 3, 256, 3, str(tmp_path))
    mixed, _ = run(harness, [m, m], 8, [0, 60], 3, 256, 3, str(tmp_path))
    both_long, _ = run(harness, [m, m], 8, [60, 60], 3, 256, 3, str(tmp_path))
    assert short > mixed > both_long and 2 * mixed == short + both_long
