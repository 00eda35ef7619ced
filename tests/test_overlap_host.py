"""CPU: the two-lane schedule of the ensemble call (facet_amd/csrc/ensemble_plan.h - the header ensemble_run executes) replayed by
tests/native/ensemble_plan_harness.cpp on simulated in-order queues, under AddressSanitizer + UBSan. For n in {1, 2, 31, 32, 33, 45, 127,
128, 129, 256, 300} x micro-batch in {1, 8, 32, 64, 200} x SAMP chunk in {1, 27, 128} (model masks 7, 3, 5; one lane, and two lanes in each variant the plan has) it checks
by vector clocks that every image goes through every model once and lands at its own output offset, that any two operations on
different queues touching overlapping staging / result bytes are ordered unless both read, and that the join orders every side
operation before the interleave."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("overlap") / "ensemble_plan_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "ensemble_plan_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("on_device", [1, 0], ids=["device_input", "host_input"])
def test_every_plan_is_hazard_free_and_complete(harness, on_device):
    r = subprocess.run([harness, "check", str(on_device)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    assert r.stdout.split() == [str(11 * 5 * 3 * 3 * 5), "plans", "ok"], r.stdout[-3000:]
