"""CPU: the per-sample arithmetic of the mixed-size thumbnails (facet_amd/csrc/thumb_mixed_core.h - the header the reduce and resize
kernels of fe_thumbnail_jpeg_mixed call) run by tests/native/thumb_mixed_harness.cpp under AddressSanitizer + UBSan, from the descriptors
and the table pool ThumbTables builds for the device. For every shape of tests/mixed_index_cases.py at sizes 64 and 640 the pixels must be
those of Pillow's `Image.thumbnail`, and the pool must hold one table per distinct (input size, box, output size). The table pool of
fe_phash_mixed (phash_mixed_plan.h) is checked through the same program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from facet_amd.thumbnail import thumbnail_plan
from mixed_index_cases import ALL_SHAPES, all_images, expected_tables, pil_thumbnail_pixels, write_harness_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("thumb_mixed") / "thumb_mixed_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "facet_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "thumb_mixed_harness.cpp"), "-o", exe], check=True)
    return exe


def test_the_plans_cover_what_the_cases_promise():
    p64 = {s: thumbnail_plan(s[1], s[0], 64) for s in ALL_SHAPES}
    assert [s for s in ALL_SHAPES if p64[s].unchanged] == [(33, 47), (32, 32), (31, 33), (1, 1), (1, 50), (50, 1)]      # encoded as they are
    assert {s: p64[s].factors for s in ALL_SHAPES if p64[s].factors != (1, 1)} == {
        (300, 260): (2, 2), (40, 400): (3, 3), (48, 1100): (8, 8), (257, 255): (1, 2), (2000, 10): (5, 15), (13, 997): (7, 6)}
    assert any(not p.unchanged and p.factors == (1, 1) for p in p64.values())      # resize only
    assert p64[(40, 400)].size == (64, 6) and p64[(13, 997)].size == (64, 1) and p64[(2000, 10)].size == (1, 64) and p64[(48, 1100)].size == (64, 3)
    # remainders: a last column, a last row and a corner that average fewer samples
    rem = [((p.reduce_box[2] - p.reduce_box[0]) % p.factors[0], (p.reduce_box[3] - p.reduce_box[1]) % p.factors[1]) for p in p64.values() if p.reduce_box]
    assert any(c and not r for c, r in rem) and any(r and not c for c, r in rem) and any(c and r for c, r in rem), rem
    assert not any(p.tall for p in p64.values())
    p640 = thumbnail_plan(10, 2000, 640)
    assert p640.tall and p640.size == (3, 640)
    assert thumbnail_plan(1100, 48, 640).size == (640, 28)
    assert ALL_SHAPES.count((64, 96)) == 2 and ALL_SHAPES.count((80, 80)) == 2


@pytest.mark.parametrize("size", [64, 640])
def test_cpu_stages_give_pillows_pixels_and_one_table_per_geometry(harness, tmp_path, size):
    imgs = all_images()
    plans = [thumbnail_plan(a.shape[1], a.shape[0], size) for a in imgs]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_harness_input(src, imgs, plans)
    r = subprocess.run([harness, "thumb", src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a sanitizer report ends the run with a status of its own
    got = np.fromfile(dst, np.uint8)
    at = 0
    for i, (a, p) in enumerate(zip(imgs, plans)):
        want = pil_thumbnail_pixels(a, size)
        assert want.shape[:2] == (p.size[1], p.size[0]), (i, ALL_SHAPES[i])
        mine = got[at:at + want.size].reshape(want.shape)
        at += want.size
        assert np.array_equal(mine, want), (f"image {i} {ALL_SHAPES[i]} size {size}: {int((mine != want).sum())} bytes differ, "
                                            f"max |d| {int(np.abs(mine.astype(int) - want.astype(int)).max())}")
    assert at == got.size
    keys = expected_tables(plans)
    tables = int(r.stdout.split("tables")[1].split()[0])
    assert tables == len(keys), (tables, len(keys))
    if size == 64:                # 64 x 96 and 80 x 80 occur twice and share their tables: one per geometry, not one per image
        twice = [p for a, p in zip(imgs, plans) if a.shape[:2] in ((64, 96), (80, 80))]
        assert len(twice) == 4 and 2 * len(expected_tables(twice)) == sum(len(expected_tables([p])) for p in twice)
        assert tables < sum(len(expected_tables([p])) for p in plans)


def test_phash_pool_identity_and_shared_sides(harness):
    shapes = [(32, 32), (32, 100), (100, 32), (64, 96), (96, 64), (64, 96), (1, 50)]
    r = subprocess.run([harness, "phash"] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    descs = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("desc")]
    sides = {}
    for l in lines:
        if l.startswith("side"):
            f = l.split()
            sides[int(f[1])] = dict(ksize=int(f[3]), first=(int(f[5]), int(f[6])), count=(int(f[8]), int(f[9])), sum=(int(f[11]), int(f[12])), tap=int(f[14]))
    assert len(descs) == len(shapes)
    assert int(lines[-1].split()[1]) == len({v for s in shapes for v in s}) == 6          # 32, 100, 64, 96, 1, 50: one table per side, not per image
    # a side of 32: one tap of exactly 1.0 at the sample itself
    assert sides[32] == dict(ksize=1, first=(0, 31), count=(1, 1), sum=(1 << 22, 1 << 22), tap=1 << 22)
    for s, v in sides.items():
        if s != 32:
            assert v["ksize"] > 1 or s == 1
            assert all(abs(t - (1 << 22)) <= v["ksize"] for t in v["sum"]), (s, v)      # normalised, each tap rounded once
    # shared sides share a table: (kh, bh, ksize_h) of an image equals (kv, bv, ksize_v) of one whose height is that width
    by_shape = dict(zip(shapes, descs))
    assert by_shape[(64, 96)][:3] == by_shape[(96, 64)][3:] and by_shape[(64, 96)][3:] == by_shape[(96, 64)][:3]
    assert by_shape[(32, 32)][:3] == by_shape[(32, 32)][3:] == by_shape[(32, 100)][3:] == by_shape[(100, 32)][:3]
    assert by_shape[(32, 100)][:3] == by_shape[(100, 32)][3:]
    assert descs[3] == descs[5]
