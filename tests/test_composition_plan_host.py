"""CPU: the plan of the mixed-size lines / subject calls (facet_amd/csrc/composition_mixed_plan.h - what fe_leading_lines_mixed and
fe_subject_region_mixed execute) checked by tests/native/composition_plan_harness.cpp under AddressSanitizer + UBSan, for both calls and
for device and host input. Input: a hand-made list with every side of 1, 15, 16, 17, 63, 64, 65 and the shapes of the GPU tests, seeded
random lists, and one 1200 x 800 image among small ones for the arena cases. Checked there: every image in exactly one chunk in order; all
regions 256-aligned, disjoint, inside the arena; the prefix tables against tile counts computed independently, and every grid walked block
by block the way the kernels bisect it covers every pixel exactly once. Here: an arena that holds exactly the large image makes three
chunks; one byte less and the image is reported by its index with what it needs; a list that needs several chunks gets several."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (1, 15, 16, 17, 63, 64, 65)
HAND = [(h, w) for h in SIDES for w in SIDES] + [(1, 7), (3, 3), (33, 47), (97, 131), (64, 300), (257, 256), (48, 1100), (64, 96), (5, 9), (64, 96)]
SMALL = [(1, 1), (17, 31), (64, 65), (3, 3)]
ARENA_LIST = SMALL + [(800, 1200)] + SMALL
BIG = len(SMALL)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("composition_plan") / "composition_plan_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "composition_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, staged, subject, arena, shapes):
    r = subprocess.run([harness, str(staged), str(subject), str(arena)] + [str(v) for hw in shapes for v in hw], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    return dict(kv.split("=") for kv in r.stdout.split())


CALLS = pytest.mark.parametrize("subject", [0, 1], ids=["lines", "subject"])
INPUTS = pytest.mark.parametrize("staged", [0, 1], ids=["device_input", "host_input"])


@CALLS
@INPUTS
def test_hand_made_list_in_one_chunk(harness, staged, subject):
    assert _run(harness, staged, subject, "big", HAND) == {"chunks": "1", "bad": "-1", "need": "0"}


@CALLS
@INPUTS
def test_seeded_random_lists(harness, staged, subject):
    rng = np.random.default_rng(11 + 2 * staged + subject)
    for _ in range(4):
        shapes = [(int(rng.integers(1, 200)), int(rng.integers(1, 200))) for _ in range(int(rng.integers(1, 40)))]
        assert _run(harness, staged, subject, "big", shapes)["bad"] == "-1"
        # an arena of three times the largest image alone: several chunks, every check again
        h, w = max(shapes, key=lambda s: s[0] * s[1])
        per_pixel = (8 + (55 if subject else 0) + 3 * staged)
        got = _run(harness, staged, subject, 3 * per_pixel * h * w + 65536, shapes)
        assert got["bad"] == "-1"
        if sum(a * b for a, b in shapes) > 6 * h * w:
            assert int(got["chunks"]) > 1


@CALLS
@INPUTS
def test_arena_that_fits_the_large_image_exactly_makes_three_chunks(harness, staged, subject):
    assert _run(harness, staged, subject, f"fit:{BIG}", ARENA_LIST) == {"chunks": "3", "bad": "-1", "need": "0"}


@CALLS
@INPUTS
def test_image_that_cannot_fit_is_reported_with_its_bytes(harness, staged, subject):
    fits = _run(harness, staged, subject, "fit:0", [ARENA_LIST[BIG]])
    assert fits["chunks"] == "1"
    got = _run(harness, staged, subject, f"short:{BIG}", ARENA_LIST)
    assert got["chunks"] == "0" and got["bad"] == str(BIG)
    # what it needs: at least its planes - 8 bytes per pixel for the lines, the subject's planes and lists on top, 3 more when staged
    npx = 800 * 1200
    assert int(got["need"]) >= npx * (8 + (46 if subject else 0) + 3 * staged)
    tiny = _run(harness, staged, subject, 8192, [(3, 3), (64, 96)])      # the 3 x 3 image fits (a region is at least 256 bytes), the next cannot
    assert tiny["chunks"] == "0" and tiny["bad"] == "1" and int(tiny["need"]) > 8192


def test_pixel_cap_cuts_chunks_but_lets_a_large_image_through_alone(harness):
    """fe_leading_lines_mixed caps a chunk's pixels by its host buffer: two 64 x 96 images fit the cap, a 400 x 400 one passes it alone"""
    shapes = [(64, 96)] * 5 + [(400, 400), (64, 96)]
    assert _run(harness, 0, 0, f"cap:{2 * 64 * 96}", shapes) == {"chunks": "5", "bad": "-1", "need": "0"}


def test_scratch_per_pixel_is_what_the_header_says(harness):
    """A 2 GiB arena takes one 6000 x 4000 photo in one chunk (both calls), 37 photos of 1024 x 1024 of the subject call in one chunk (about
    55 bytes per pixel) and 48 of them in two."""
    for subject in (0, 1):
        assert int(_run(harness, 0, subject, 2 << 30, [(4000, 6000)])["chunks"]) == 1
    assert int(_run(harness, 0, 1, 2 << 30, [(1024, 1024)] * 37)["chunks"]) == 1
    assert int(_run(harness, 0, 1, 2 << 30, [(1024, 1024)] * 48)["chunks"]) == 2
