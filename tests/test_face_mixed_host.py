"""CPU: the plan of the mixed-size face calls (facet_amd/csrc/face_mixed_plan.h - what fe_face_analyze_mixed executes) checked by
tests/native/face_plan_harness.cpp under AddressSanitizer + UBSan, and against fe_face_analyze's own fit arithmetic restated in numpy
float32 (capi_face.hip; insightface SCRFD.detect): new_h, new_w, the resize route and the bits of det_scale for a sweep of sizes at
det_size 320 x 320 and 640 x 640 and a non-square 320 x 480 canvas. The harness itself checks the micro-batch cuts (never more than the
given bytes, 256-byte starts, no overlap, greedy) and the table pool (one table per distinct (source, target, clamp), read back whole)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# the float-truncation cases first, then every route: copy, exact 2x, tall, wide, upscale, extreme ratios (new_h or new_w of 0)
SWEEP = [(300, 500), (501, 333), (1, 1), (8, 600), (640, 640), (200, 320), (320, 320), (400, 300), (97, 131), (2, 2000), (2000, 2), (1280, 1280),
         (1024, 683), (683, 1024), (3, 7), (7, 3), (333, 501), (1000, 999), (999, 1000), (4000, 6000), (65535, 1), (479, 640), (640, 320), (213, 320)]


def _fit(h, w, det_h, det_w):
    """fe_face_analyze's arithmetic, operation by operation in float32."""
    im_ratio, model_ratio = F(h) / F(w), F(det_h) / F(det_w)
    if im_ratio > model_ratio:
        new_h = det_h
        new_w = int(F(new_h) / im_ratio)
    else:
        new_w = det_w
        new_h = int(F(new_w) * im_ratio)
    scale = F(new_h) / F(h) if new_h > 0 else F(0)
    mode = 2 if (h == new_h and w == new_w) else (1 if (h == 2 * new_h and w == 2 * new_w) else 0)
    return new_h, new_w, mode, int(np.asarray(scale, F).view(np.uint32)), int(new_h > 0 and new_w > 0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("face_plan") / "face_plan_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "face_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, det, max_images, staged, room, shapes):
    r = subprocess.run([harness, str(det[0]), str(det[1]), str(max_images), str(staged), str(room)] + [str(v) for hw in shapes for v in hw],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]          # a failed check or a sanitizer report ends the run with a status of its own
    imgs, cuts, bad = [], [], None
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "img":
            imgs.append((int(t[2]), int(t[3]), int(t[4]), int(t[5], 16), int(t[6])))
        elif t[0] == "cut":
            cuts.append((int(t[1]), int(t[2]), int(t[3])))
        elif t[0].startswith("bad="):
            bad = int(t[0][4:])
    return imgs, cuts, bad


@pytest.mark.parametrize("det", [(320, 320), (640, 640), (320, 480)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_descriptors_equal_the_per_shape_arithmetic(harness, det):
    imgs, cuts, bad = _run(harness, det, 16, 0, 0, SWEEP)
    assert bad == -1 and len(imgs) == len(SWEEP)
    for (h, w), got in zip(SWEEP, imgs):
        assert got == _fit(h, w, *det), (h, w)
    if det == (320, 320):      # what the GPU tests rely on
        by = dict(zip(SWEEP, imgs))
        assert by[(640, 640)][:3] == (320, 320, 1) and by[(200, 320)][:3] == (200, 320, 2) and by[(320, 320)][:3] == (320, 320, 2)
        assert by[(300, 500)][:3] == (192, 320, 0) and by[(400, 300)][:3] == (320, 240, 0) and by[(8, 600)][:3] == (4, 320, 0)
        assert by[(1, 1)][:3] == (320, 320, 0) and by[(2, 2000)][0] == 0 and by[(2, 2000)][4] == 0 and by[(2000, 2)][4] == 0
    assert cuts == [(0, 16, 0), (16, len(SWEEP), 0)]      # resident input: nothing is staged, only the image count cuts


def test_micro_batches_never_exceed_the_staging_room(harness):
    shapes = [(100, 100), (300, 500), (1, 1), (640, 640), (97, 131), (640, 640), (8, 600), (400, 300), (3, 5)]
    up = lambda h, w: -(-h * w * 3 // 256) * 256
    big = up(640, 640)
    for room in (big, big + 256, 2 * big + 1024, 1 << 30):
        for max_images in (1, 2, 16):
            imgs, cuts, bad = _run(harness, (320, 320), max_images, 1, room, shapes)
            assert bad == -1
            assert [c[0] for c in cuts] == [0] + [c[1] for c in cuts[:-1]] and cuts[-1][1] == len(shapes)
            for i0, i1, b in cuts:
                assert b == sum(up(*shapes[i]) for i in range(i0, i1)) <= room and 1 <= i1 - i0 <= max_images
    # exactly the large image's bytes: it is alone in its micro-batches
    _, cuts, _ = _run(harness, (320, 320), 16, 1, big, shapes)
    assert (3, 4, big) in cuts and (5, 6, big) in cuts


def test_image_that_cannot_fit_is_reported_by_index(harness):
    shapes = [(100, 100), (300, 500), (640, 640), (97, 131), (641, 640)]
    room = -(-640 * 640 * 3 // 256) * 256
    assert _run(harness, (320, 320), 16, 1, room, shapes)[2] == 4
    assert _run(harness, (320, 320), 16, 1, room - 1, shapes)[2] == 2
    assert _run(harness, (320, 320), 16, 1, 255, shapes)[2] == 0
    assert _run(harness, (320, 320), 16, 0, 255, shapes)[2] == -1      # resident images are read in place


def test_case_images_keep_their_margins():
    """What tests/face_mixed_cases.py says of its seeds, by the CPU oracle: every image yields detections, and no score and no overlap
    lies within 1e-3 of its threshold. NMS removes a candidate in at least one image, so the overlap rule is exercised."""
    from standins import synthetic_onnx as S
    import face_mixed_cases as FC
    det, _ = S.scrfd_like(seed=12, size=320)
    removed = 0
    for k in range(len(FC.CASES)):
        score_gap, overlap_gap, cand, kept = FC.margins(det, FC.image(k))
        print(f"[face cases] {k} {FC.CASES[k]}: score gap {score_gap:.2e}, overlap gap {overlap_gap:.2e}, {cand} candidates, {kept} kept")
        assert cand > 0 and kept > 0 and score_gap > 1e-3 and overlap_gap > 1e-3, k
        removed += cand - kept
    assert removed > 0
