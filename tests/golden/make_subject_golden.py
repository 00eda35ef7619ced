"""Generates tests/golden/subject_golden.json by RUNNING THE REFERENCE'S OWN CompositionAnalyzer.detect_subject_region and
get_placement_data(None, w, h, None, img) (analyzers/composition.py:16-93, 111-187) on small seeded scenes. cv2 is absent, so a module
named cv2 is put in sys.modules whose cvtColor / Canny / findContours / contourArea / moments / boundingRect are the restatements of
tests/subject_ref.py (the host_golden.json method); `cv2.saliency` does not exist on it, as in the opencv-python wheel the reference
installs, so strategy 2 ends in the reference's own `except AttributeError`. Nothing from the reference is copied: only the scene
parameters and what its code returned are stored, plus the restatement's records the boxes were chosen from.

    python tests/golden/make_subject_golden.py <path of the reference checkout>

Fails when the two best contour scores of a scene are closer than 1e-9 relative (the choice must not hang on rounding)."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import subject_ref as S                                   # noqa: E402

sys.path.insert(0, sys.argv[1])
cv2 = S.fake_cv2(types.ModuleType("cv2"))
sys.modules["cv2"] = cv2
from analyzers.composition import CompositionAnalyzer    # noqa: E402

SCENES = [  # h, w, seed, noise, kind
    (97, 131, 1, 0, "mixed"), (97, 131, 2, 6, "disc"), (97, 131, 3, 25, "mixed"), (97, 131, 4, 0, "flat"), (97, 131, 5, 0, "gradient"),
    (97, 131, 6, 6, "bars"), (200, 260, 7, 0, "disc"), (200, 260, 8, 6, "mixed"), (64, 300, 9, 0, "bars"), (64, 300, 10, 25, "mixed"),
    (257, 256, 11, 6, "mixed"), (257, 256, 12, 0, "gradient"),
]

out = []
for h, w, seed, noise, kind in SCENES:
    img = S.scene(h, w, seed, noise, kind)
    box = CompositionAnalyzer.detect_subject_region(img)
    placement = CompositionAnalyzer.get_placement_data(None, w, h, None, img)
    rec, thr, edges = S.subject_records(img)
    # the scores the reference's loop compared, recomputed through the same cv2 stand-ins, for the closeness test only
    contours, _ = cv2.findContours(edges, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)
    scores = []
    for c in contours:
        if not cv2.contourArea(c) > (h * w) * 0.0001:
            continue
        M = cv2.moments(c)
        if M["m00"] == 0:
            continue
        cx, cy = M["m10"] / M["m00"], M["m01"] / M["m00"]
        dist_x = min(abs(cx - t) for t in [w / 3, 2 * w / 3]) / w
        dist_y = min(abs(cy - t) for t in [h / 3, 2 * h / 3]) / h
        scores.append(cv2.contourArea(c) / (h * w) * (1 + max(0, 1 - (dist_x + dist_y))))
    scores.sort(reverse=True)
    if len(scores) >= 2 and scores[0] - scores[1] <= 1e-9 * scores[0]:
        raise SystemExit(f"scene {(h, w, seed, noise, kind)}: the two best scores {scores[:2]} are too close - choose another scene")
    assert (box is None) == (not scores)
    out.append({"h": h, "w": w, "seed": seed, "noise": noise, "kind": kind, "thresholds": list(thr), "records": rec.tolist(),
                "edge_pixels": int((edges != 0).sum()), "box": None if box is None else [int(v) for v in box],
                "placement": {k: float(v) for k, v in placement.items()}})
    print((h, w, seed, noise, kind), "thr", thr, "contours", len(contours), "valid", len(scores), "box", box)
assert sum(r["box"] is None for r in out) >= 2
path = os.path.join(HERE, "subject_golden.json")
json.dump(out, open(path, "w"))
print("wrote", path, os.path.getsize(path), "bytes")
