"""CPU: the branch-free fp32 erf of the GELU epilogues (facet_amd/csrc/erf_core.h - the header the fp32 kernels call) compiled for the host
by tests/native/erf_harness.cpp under AddressSanitizer + UBSan and compared with erf() in double: every 64th fp32 bit pattern of both
signs, every pattern within 2^16 of the range threshold, zeros, infinities, NaN, the largest finite value and denormals. The harness
asserts an error of at most 2 ulp of the result (what tests/plain_ops_ref.act_eval budgets for erff), oddness bit for bit, |erf| <= 1,
a non-decreasing result along the sweep and exactly +-1 at and above 4.0; it prints the measured maximum (1.2541 ulp at x = 0.921938896,
just above the threshold, when this was written)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("erf") / "erf_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "facet_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "erf_harness.cpp"), "-o", exe], check=True)
    return exe


def test_fe_erf_against_double(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    m = re.search(r"max error ([0-9.]+) ulp", r.stdout)
    assert m and float(m.group(1)) <= 2.0, r.stdout
    assert r.stdout.rstrip().endswith("ok"), r.stdout
