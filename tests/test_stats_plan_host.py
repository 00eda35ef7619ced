"""CPU: the block plan of a mixed-size statistics call (facet_amd/csrc/stats_plan.h - what fe_image_stats_mixed executes) checked by
tests/native/stats_plan_harness.cpp under AddressSanitizer + UBSan. Input: the shapes of tests/mixed_cases.py, one 6000 x 4000 image, then
1 x 1, 1 x 7, 3 x 5 and 257 x 131, at segment sizes 4096 and 262 144, for device and for host input. Checked: every pixel of every image
lies in exactly one segment per hue half, every segment starts at a multiple of 4 pixels, every row lies in exactly one strip, gray planes
do not overlap, no chunk's scratch exceeds the arena; an arena that holds exactly the large image makes three chunks (the images before
it, the image, the images after it); one byte less and the image is reported by its index."""
import os
import shutil
import subprocess

import pytest

from mixed_cases import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = len(SHAPES)
LIST = list(SHAPES) + [(4000, 6000), (1, 1), (1, 7), (3, 5), (257, 131)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stats_plan") / "stats_plan_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "stats_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, staged, segment, arena, shapes=LIST):
    r = subprocess.run([harness, str(staged), str(segment), arena] + [str(v) for hw in shapes for v in hw], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    return r.stdout.split()


@pytest.mark.parametrize("segment", [4096, 262144])
@pytest.mark.parametrize("staged", [0, 1], ids=["device_input", "host_input"])
def test_plan_covers_every_pixel_and_row_once_and_fits_the_arena(harness, staged, segment):
    assert _run(harness, staged, segment, "big") == ["chunks=1", "bad=-1"]
    assert _run(harness, staged, segment, f"fit:{BIG}") == ["chunks=3", "bad=-1"]


@pytest.mark.parametrize("staged", [0, 1], ids=["device_input", "host_input"])
def test_image_that_cannot_fit_is_reported_by_index(harness, staged):
    assert _run(harness, staged, 262144, f"short:{BIG}") == ["chunks=0", f"bad={BIG}"]
    assert _run(harness, staged, 4096, "short:0") == ["chunks=0", "bad=0"]
