"""CPU: what the plans of the mixed-size calls share (facet_amd/csrc/mixed_list.h: the greedy cutter, the staged offsets, the Pillow
table pool), checked by tests/native/mixed_list_harness.cpp under AddressSanitizer + UBSan, and the arena chunks of the lists that the
chunking tests of tests/test_phash_mixed_gpu.py, test_thumbnail_mixed_gpu.py and test_stats_mixed_gpu.py send through a 1 MiB arena:
the counts worked out beside the lists in tests/mixed_index_cases.py and tests/mixed_cases.py are what the plans give, so those tests do
run several chunks, one of them of several images, with a shorter last one."""
import os
import shutil
import subprocess

import pytest

import mixed_cases
import mixed_index_cases
from facet_amd.thumbnail import thumbnail_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("mixed_list") / "mixed_list_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "facet_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "mixed_list_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    print(r.stdout.strip())
    return r.stdout


@pytest.mark.parametrize("seed", [1, 2])
def test_cutter_tiles_the_list_with_maximal_chunks_and_names_the_first_image_that_cannot_stand_alone(harness, seed):
    assert "cutter ok: 300 lists" in _run(harness, "cutter", seed, 300)


def test_staged_offsets_are_aligned_or_packed_and_stay_within_the_sum(harness):
    assert "offsets ok: 300 lists" in _run(harness, "offsets", 3, 300)


def test_pool_holds_the_slices_of_pil_resize_coeffs_one_per_key(harness):
    assert "pool ok: 11 tables" in _run(harness, "pool")          # nine keys that differ in one field each, the identity, a clamped box


def _cuts(out):
    line = out.strip().splitlines()[-1].split()
    assert line[0] == "cuts", out
    return [int(v) for v in line[1:]]


def _chunked(cuts, n):
    """At least three chunks that tile the list, several images in one of them, the last one shorter than the longest."""
    return sum(cuts) == n and len(cuts) >= 3 and max(cuts) > 1 and cuts[-1] < max(cuts)


def test_the_chunking_lists_are_cut_as_their_comments_say(harness, tmp_path):
    arena = mixed_index_cases.CHUNK_ARENA
    assert arena == mixed_cases.CHUNK_ARENA == 1 << 20
    shapes = mixed_index_cases.CHUNK_SHAPES
    flat = [v for s in shapes for v in s]
    host = _cuts(_run(harness, "cuts", "phash", arena, 1, 1, 1, *flat))
    assert host == [5, 5, 1] and _chunked(host, len(shapes))
    assert _cuts(_run(harness, "cuts", "phash", arena, 1, 0, 0, *flat)) == [5, 5, 1]          # the plain call
    assert _cuts(_run(harness, "cuts", "phash", arena, 0, 1, 1, *flat)) == [11]               # resident: rows and outputs only
    assert _run(harness, "cuts", "phash", arena, 1, 1, 1, 128, 128, 700, 700).split()[:2] == ["bad", "1"]

    src = str(tmp_path / "in.bin")
    arrs = mixed_index_cases.chunk_images()
    mixed_index_cases.write_harness_input(src, arrs, [thumbnail_plan(w, h, 64) for h, w in shapes])
    row = 96 * 208 * 2 + 625          # fe_jpeg_bound(64, 64), the default row: 96 blocks at their longest, every byte stuffed, header, EOI
    host = _cuts(_run(harness, "cuts", "thumb", arena, 1, row, src))
    assert host == [2, 3, 2, 2, 2] and _chunked(host, len(shapes))
    assert _cuts(_run(harness, "cuts", "thumb", arena, 0, row, src)) == [5, 5, 1]

    shapes = mixed_cases.STATS_CHUNK_SHAPES
    flat = [v for s in shapes for v in s]
    for staged in (1, 0):
        cuts = _cuts(_run(harness, "cuts", "stats", arena, staged, 262144, *flat))
        assert cuts == [5, 5, 1] and _chunked(cuts, len(shapes))
    assert _run(harness, "cuts", "stats", arena, 1, 262144, 96, 64, 33, 47, 600, 500).split()[:2] == ["bad", "2"]
