"""Subject-region detection, the parts that need no GPU: the selection arithmetic against the reference's own function
(tests/golden/subject_golden.json), the unchanged placement call, the ABI symbols, and the border walk of contour_core.h under
AddressSanitizer + UBSan against the restatement (tests/subject_ref.py)."""
import ctypes
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subject_ref as S                                   # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "subject_golden.json")))


def test_subject_box_equals_the_reference_on_recorded_records():
    from facet_amd.batch import placement_data
    from facet_amd.composition import subject_box
    assert len(GOLDEN) >= 12 and sum(g["box"] is None for g in GOLDEN) >= 2
    for g in GOLDEN:
        assert subject_box(np.array(g["records"], np.int64).reshape(-1, 8), g["h"], g["w"]) == g["box"], g["seed"]
        assert placement_data(g["box"], g["w"], g["h"]) == g["placement"], g["seed"]


def test_whole_selection_from_pixels_equals_the_golden_file():
    from facet_amd.composition import subject_box
    for g in GOLDEN:
        rec, thr, _ = S.subject_records(S.scene(g["h"], g["w"], g["seed"], g["noise"], g["kind"]))
        assert list(thr) == g["thresholds"] and rec.tolist() == g["records"], g["seed"]
        assert subject_box(rec, g["h"], g["w"]) == g["box"], g["seed"]


def test_placement_without_image_is_unchanged_and_none_gives_none():
    from facet_amd.batch import placement_data
    from facet_amd.composition import CompositionAnalyzer
    host = json.load(open(os.path.join(ROOT, "tests", "golden", "host_golden.json")))["placement"]
    for p in host:
        cfg = None
        if p["weights"] != [2.0, 1.0]:
            wts = {"power_point_weight": p["weights"][0], "line_weight": p["weights"][1]}
            cfg = type("Cfg", (), {"get_composition_weights": lambda self, _w=wts: _w})()
        assert CompositionAnalyzer.get_placement_data(p["bbox"], p["w"], p["h"], cfg) == p["out"]
        assert CompositionAnalyzer.get_placement_data(p["bbox"], p["w"], p["h"], cfg, img_cv=None) == p["out"]
    assert CompositionAnalyzer.get_placement_data(None, 640, 480) == placement_data(None, 640, 480)
    assert CompositionAnalyzer.detect_subject_region(None) is None


def test_abi_symbols_exist():
    from facet_amd._lib import LIB_PATH, SIGNATURES
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("fe_external_contours", "fe_subject_region"):
        assert name in SIGNATURES and getattr(lib, name) is not None


# ---- the walk of contour_core.h, sanitized ----------------------------------------------------------------------------------------------
def drawn_cases():
    single = np.zeros((5, 7), np.uint8); single[2, 3] = 1
    curve = np.zeros((12, 15), np.uint8)
    for t in range(9):
        curve[2 + t, 3 + (t * 2) // 3] = 1                  # one pixel wide, open: area 0
    curve[10, 11:14] = 1
    frame_ring = np.zeros((9, 11), np.uint8); frame_ring[0, :] = frame_ring[-1, :] = 1; frame_ring[:, 0] = frame_ring[:, -1] = 1
    frame_ring[4, 5] = 1                                    # a pixel in its hole: not external
    ring2 = np.zeros((14, 16), np.uint8); ring2[2:12, 3:13] = 1; ring2[4:10, 5:11] = 0
    return {"single": single, "open_curve": curve, "frame_ring": frame_ring, "ring2": ring2, "spiral": spiral(23, 29)}


def spiral(h, w, gap=2):
    """A one-pixel-wide rectangular spiral: one component whose border runs along both of its sides."""
    a = np.zeros((h, w), np.uint8)
    t, b, l, r = 1, h - 2, 1, w - 2
    while t <= b and l <= r:
        a[t, l:r + 1] = 1
        a[t:b + 1, r] = 1
        if b - t >= gap:
            a[b, l + gap:r + 1] = 1
        if r - l >= 2 * gap and b - t >= 2 * gap:
            a[t + gap:b + 1, l + gap] = 1
        t, b, l, r = t + gap, b - gap, l + 2 * gap, r - gap
        if t <= b and l <= r:
            a[t, l - gap:l + 1] = 1
    return a


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("contour") / "contour_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "contour_harness.cpp"), "-o", exe], check=True)
    return exe


def run_harness(exe, images, tmp):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(images)))
        for a in images:
            f.write(struct.pack("ii", *a.shape))
            f.write(np.ascontiguousarray(a, np.uint8).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(fout, "rb").read()
    out, o = [], 0
    for _ in images:
        k = struct.unpack_from("i", raw, o)[0]
        o += 4
        out.append(np.frombuffer(raw, np.int64, k * 10, o).reshape(k, 10))
        o += k * 80
    assert o == len(raw)
    return out


def test_host_walk_equals_restatement_and_keeps_the_step_bound(harness, tmp_path):
    cases = drawn_cases()
    rng = np.random.default_rng(3)
    cases["noise"] = (rng.random((40, 53)) < 0.35).astype(np.uint8)
    got = run_harness(harness, list(cases.values()), str(tmp_path))
    for (name, img), g in zip(cases.items(), got):
        want, steps = S.records(img)
        assert g[:, :8].tolist() == want.tolist(), name
        assert g[:, 8].tolist() == steps and (g[:, 8] >= 0).all() and (g[:, 8] <= g[:, 9]).all(), name
        topo = S.topology_scipy(img)                        # second opinion: same components, same boxes, same external ones
        assert [t[:5] for t in topo if t[5]] == [(r[0], r[4], r[5], r[6], r[7]) for r in want.tolist()], name
    assert len(S.records(cases["single"])[0]) == 1 and S.records(cases["single"])[0][0, 1] == 0
    assert S.records(cases["open_curve"])[0][:, 1].tolist() == [0, 0]
    assert len(S.records(cases["frame_ring"])[0]) == 1 and len(S.topology_scipy(cases["frame_ring"])) == 2
    assert len(S.records(cases["spiral"])[0]) == 1
