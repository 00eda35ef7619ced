"""CPU: the schedule of a mixed-size ensemble call (facet_amd/csrc/ensemble_plan.h: cut_mixed + build(Shape, cuts) - what
fe_ensemble_score_mixed executes) replayed by tests/native/mixed_plan_harness.cpp on simulated in-order queues, under AddressSanitizer +
UBSan. Inputs: all images of one shape, two shapes alternating, every image different, n = 1, 70 images in 3 shapes at micro-batch 16,
each under the model masks 7, 6 (TOPIQ deselected), 5 and 1. Checked by vector clocks: no cross-queue hazard; every image passes through
each selected model exactly once; the position map of the interleave returns the records to input order; a micro-batch holds one shape
whenever TOPIQ is on; for uniform input the operation list equals build(Shape) element by element."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("mixed_plan") / "mixed_plan_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "mixed_plan_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("overlap", [1, 0], ids=["two_lanes", "one_lane"])
@pytest.mark.parametrize("on_device", [1, 0], ids=["device_input", "host_input"])
def test_mixed_plans_are_hazard_free_complete_and_in_input_order(harness, on_device, overlap):
    r = subprocess.run([harness, "check", str(on_device), str(overlap)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    cases, masks, chunks = 7, 4, 2
    assert r.stdout.split() == [str(cases * masks * chunks * (4 if overlap else 1)), "plans", "ok"], r.stdout[-3000:]
