"""CPU: the per-sample arithmetic of the mixed-size 224 x 224 preprocessing (facet_amd/csrc/resize_mixed_core.h - the header the two
kernels of kernels_resize_mixed.hip call) run by tests/native/resize_mixed_harness.cpp under AddressSanitizer + UBSan, from the
descriptors and the table pool that MixedTables builds for the device. The crops of every shape of tests/mixed_cases.py, in both
modes, must be Pillow's bytes."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from mixed_cases import CLIP, SAMP, SHAPES, images, pillow_crop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("resize_mixed") / "resize_mixed_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "facet_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "resize_mixed_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("mode", [CLIP, SAMP], ids=["clip", "samp"])
def test_cpu_passes_give_pillows_bytes(harness, tmp_path, mode):
    imgs = images()
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(imgs)))
        for a in imgs:
            f.write(struct.pack("<ii", a.shape[0], a.shape[1]))
            f.write(a.tobytes())
    r = subprocess.run([harness, str(mode), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    crops = np.fromfile(dst, np.uint8).reshape(len(imgs), 224, 224, 3)
    for i, a in enumerate(imgs):
        want = pillow_crop(a, mode)
        assert np.array_equal(crops[i], want), (f"image {i} {SHAPES[i]}: {int((crops[i] != want).sum())} bytes differ, "
                                                f"max |d| {int(np.abs(crops[i].astype(int) - want.astype(int)).max())}")
