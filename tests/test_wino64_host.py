"""CPU: the in-register Winograd F(2x2,3x3) kernel (facet_amd/csrc/kernels_wino64.hip) as a host model. tests/native/wino64_harness.cpp
runs the kernel's algorithm as loops over workgroups, waves and lanes on the index maps, transforms and U packing of
facet_amd/csrc/wino64_maps.h - the header the device code is compiled from - under AddressSanitizer + UBSan, and compares it with a
plain direct convolution. The inputs are small integers, so U holds quarters of integers, V integer sums, and every product and sum is
exact in fp32: the two results must be exactly equal."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("wino64") / "wino64_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "wino64_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (19, 23)])
@pytest.mark.parametrize("cin,cout", [(64, 64), (56, 40)])
def test_kernel_model_equals_direct_convolution(harness, cin, cout, hw):
    r = subprocess.run([harness, "3", str(cin), str(cout), str(hw[0]), str(hw[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    assert r.stdout.split()[0] == str(3 * cout * hw[0] * hw[1]) and " 0 differ" in r.stdout
