"""Mirror of the reference's `CompositionAnalyzer` (analyzers/composition.py) over the engine.

    CompositionAnalyzer.get_placement_data(bbox, w, h, config, img_cv)  rule-of-thirds placement (:111-187; facet_amd/batch.py)
    CompositionAnalyzer.detect_subject_region(img_cv)                 :16-93 - subject box of a photo without a face box
    CompositionAnalyzer.detect_subject_region_batch(engine, bgr_batch) the same for a whole batch in one engine call
    CompositionAnalyzer.detect_leading_lines(img_cv, cache=None)      :191-261 - one image
    CompositionAnalyzer.detect_leading_lines_batch(engine, bgr_batch) the same for a whole batch in one engine call
    CompositionAnalyzer.detect_subject_region_mixed / detect_leading_lines_mixed(engine, images, order=)
                                                                      the same for a list of images of any sizes, one engine call each
    CompositionAnalyzer.integrate_leading_lines(base, lines, faces)   :262-283

The reference runs cv2.GaussianBlur + cv2.Canny + cv2.HoughLinesP per image; here `fe_leading_lines` does the pixel scans on
the GPU and the sequential Hough stage on host threads (include/facet_engine.h). Scoring of the segments follows :231-256 with
the same numpy types (int32 coordinates, float64 arithmetic, numpy's round).

The subject region (median-threshold cv2.Canny + cv2.findContours(RETR_EXTERNAL) + contourArea / moments per image in the reference)
comes from `fe_subject_region`, which keeps every stage on the GPU and returns a few integer records per image; `subject_box` makes the
reference's choice among them in float64. The reference's second strategy (cv2.saliency spectral residual, :77-91) is not built: the
opencv-python wheel the reference installs has no `saliency` module, so that branch ends in its `except AttributeError` and the
function returns None - as this mirror does when strategy 1 finds nothing. Parity of the contour stage with cv2 itself is unpinned
(cv2 is not available offline); the selection arithmetic is pinned by tests/golden/subject_golden.json."""
import numpy as np

from . import default_engine
from .batch import placement_data


def score_lines(lines, h, w):
    """lines: int32 [k,4] as cv2.HoughLinesP returns them (k may be 0 = the reference's `lines is None`)."""
    if lines is None or len(lines) == 0:
        return {'leading_lines_score': 0, 'line_count': 0}
    seg = np.asarray(lines, dtype=np.int32).reshape(-1, 4)
    dx, dy = seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1]                # int32, as the reference's per-segment scalars
    length = np.sqrt(dx ** 2 + dy ** 2)
    with np.errstate(divide='ignore', invalid='ignore'):
        angle = np.where(dx != 0, np.abs(np.degrees(np.arctan(dy / dx))), 90.0)
    bonus = np.where((angle >= 15) & (angle <= 75), 1.5, 1.0)           # diagonals guide the eye (:244-247)
    terms = (length / np.sqrt(h ** 2 + w ** 2)) * 10 * bonus
    total_score = np.float64(sum(terms.tolist()))                       # left-to-right float64 sum, like the reference's loop
    score = min(10.0, total_score / max(1, len(seg)) * 2)
    return {'leading_lines_score': round(score, 2), 'line_count': len(lines)}


def subject_box(records, h, w):
    """The reference's choice among the contours (:40-75). records: int [k,8] = start_index, a00, a10, a01, x_min, y_min, x_max, y_max in
    cv2.findContours' order (Engine.subject_contours). -> [x1, y1, x2, y2] or None."""
    min_area = (h * w) * 0.0001
    thirds_x = [w / 3, 2 * w / 3]
    thirds_y = [h / 3, 2 * h / 3]
    best, best_score = None, 0
    for start, a00, a10, a01, x_min, y_min, x_max, y_max in np.asarray(records, dtype=np.int64).reshape(-1, 8).tolist():
        area = abs(a00) * 0.5                                   # cv2.contourArea
        if not area > min_area:
            continue
        sgn = -1 if a00 < 0 else 1                              # cv2.moments: m00 = a00 / 2, m10 = a10 / 6, m01 = a01 / 6, sign of a00
        m00, m10, m01 = sgn * a00 / 2, sgn * a10 / 6, sgn * a01 / 6
        if m00 == 0:
            continue
        cx = m10 / m00
        cy = m01 / m00
        area_score = area / (h * w)
        dist_x = min(abs(cx - t) for t in thirds_x) / w
        dist_y = min(abs(cy - t) for t in thirds_y) / h
        score = area_score * (1 + max(0, 1 - (dist_x + dist_y)))
        if score > best_score:
            best_score, best = score, [x_min, y_min, x_max + 1, y_max + 1]
    return best


class CompositionAnalyzer:
    @staticmethod
    def detect_subject_region_batch(engine, bgr_batch):
        """bgr_batch: uint8 [n,h,w,3] or a resident (device_ptr, n, h, w) -> one [x1, y1, x2, y2] or None per image."""
        if isinstance(bgr_batch, tuple):
            h, w = bgr_batch[2], bgr_batch[3]
        else:
            bgr_batch = np.ascontiguousarray(bgr_batch, dtype=np.uint8)
            h, w = bgr_batch.shape[1:3]
        return [subject_box(r, h, w) for r in engine.subject_contours(bgr_batch)]

    @staticmethod
    def _sizes(images):
        return [tuple(s) for s in images[1]] if isinstance(images, tuple) else [np.shape(a)[:2] for a in images]

    @staticmethod
    def detect_subject_region_mixed(engine, images, order='bgr'):
        """images: a list of uint8 [h,w,3] arrays of any sizes, or resident (device_pointers, sizes) -> one [x1, y1, x2, y2] or None per
        image, from one engine call (fe_subject_region_mixed)."""
        return [subject_box(r, h, w) for r, (h, w) in zip(engine.subject_contours_mixed(images, order=order), CompositionAnalyzer._sizes(images))]

    @staticmethod
    def detect_leading_lines_mixed(engine, images, order='bgr'):
        """images as above -> one {'leading_lines_score', 'line_count'} per image, from one engine call (fe_leading_lines_mixed)."""
        return [score_lines(l, h, w) for l, (h, w) in zip(engine.leading_lines_mixed(images, order=order), CompositionAnalyzer._sizes(images))]

    @staticmethod
    def detect_subject_region(img_cv, engine=None):
        """Strategy 1 of the reference (:32-75); None where the reference's saliency fallback is unavailable too (module docstring)."""
        if img_cv is None:
            return None
        engine = engine or default_engine()
        return CompositionAnalyzer.detect_subject_region_batch(engine, np.asarray(img_cv)[None])[0]

    @staticmethod
    def get_placement_data(bbox, img_w, img_h, config=None, img_cv=None, engine=None):
        if bbox is None and img_cv is not None:      # edge-based fallback for photos without faces (:125-126)
            bbox = CompositionAnalyzer.detect_subject_region(img_cv, engine)
        wts = config.get_composition_weights() if config is not None else {}
        return placement_data(bbox, img_w, img_h, wts.get('power_point_weight', 2.0), wts.get('line_weight', 1.0))

    @staticmethod
    def detect_leading_lines_batch(engine, bgr_batch):
        bgr = np.ascontiguousarray(bgr_batch, dtype=np.uint8)
        h, w = bgr.shape[1:3]
        return [score_lines(l, h, w) for l in engine.leading_lines(bgr)]

    @staticmethod
    def detect_leading_lines(img_cv, cache=None, engine=None):
        if img_cv is None:
            return {'leading_lines_score': 0, 'line_count': 0}
        engine = engine or default_engine()          # `cache` is accepted for signature parity; the engine computes its own gray
        return CompositionAnalyzer.detect_leading_lines_batch(engine, np.asarray(img_cv)[None])[0]

    @staticmethod
    def integrate_leading_lines(base_comp_score, leading_lines_score, has_faces):
        if has_faces:
            return base_comp_score
        return min(10.0, base_comp_score + min(2.0, leading_lines_score / 5.0))
