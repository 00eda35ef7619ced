"""CPU: face_thumbnail_plan is the slicing and sizing FaceAnalyzer._crop_face_thumbnail does, and that helper still returns the bytes
of its earlier body (Pillow BOX resize of the crop + Pillow JPEG) now that both share the plan. The GPU side is
test_face_thumbnail_gpu.py."""
import io

import numpy as np
import pytest
from PIL import Image

from facet_amd.face import FaceAnalyzer, face_thumbnail_plan


def analyzer(size=128, quality=85):
    fa = object.__new__(FaceAnalyzer)      # the helper reads only these two attributes; no engine, no models
    fa.thumbnail_size, fa.thumbnail_quality = size, quality
    return fa


def earlier_body(img_cv, bbox, size, quality, padding=0.3):
    """_crop_face_thumbnail as it stood before face_thumbnail_plan was factored out, word for word."""
    try:
        left, top, right, bottom = (int(v) for v in bbox)
        grow_x, grow_y = int((right - left) * padding), int((bottom - top) * padding)
        rows = slice(max(0, top - grow_y), min(img_cv.shape[0], bottom + grow_y))
        cols = slice(max(0, left - grow_x), min(img_cv.shape[1], right + grow_x))
        crop = img_cv[rows, cols]
        if crop.size == 0:
            return None
        factor = size / max(crop.shape[0], crop.shape[1])
        out_size = (int(crop.shape[1] * factor), int(crop.shape[0] * factor))
        thumb = Image.fromarray(np.ascontiguousarray(crop[:, :, ::-1])).resize(out_size, Image.BOX)
        out = io.BytesIO()
        thumb.save(out, format='JPEG', quality=int(quality))
        return out.getvalue(), rows, cols, out_size
    except Exception:
        return None


H, W = 240, 1100
BOXES = [
    (100, 60, 180, 150),            # inside
    (100.9, 60.2, 180.7, 150.99),   # floats truncate
    (-30, 80, 50, 160),             # over the left border
    (1050, 80, 1130, 160),          # right
    (500, -40, 580, 40),            # top
    (500, 200, 580, 280),           # bottom
    (-500, -400, 2000, 900),        # larger than the image
    (-60, -70, -30, -40),           # negative on both axes: numpy counts the upper bounds from the far edge
    (1300, 300, 1400, 380),         # fully outside -> None
    (1200, 50, 1300, 120),          # outside to the right only -> None
    (50, 100, 1050, 103),           # 1000 x 3 with padding 0 -> 128 x 0 -> None
    (10, 10, 10, 60),               # zero width
    (10, 10, 138, 138),             # exactly 128 x 128 with padding 0
    (float('nan'), 0, 10, 10),      # not a number -> None
]


@pytest.mark.parametrize("padding", [0.3, 0.0])
@pytest.mark.parametrize("size", [128, 64])
def test_plan_matches_the_helpers_slices_and_sizes(padding, size):
    img = np.zeros((H, W, 3), np.uint8)
    seen_none = seen_plan = 0
    for box in BOXES:
        plan = face_thumbnail_plan(box, H, W, size, padding)
        want = earlier_body(img, box, size, 85, padding)
        if want is None:
            assert plan is None, box
            seen_none += 1
            continue
        _, rows, cols, out_size = want
        y0, y1, _ = rows.indices(H)
        x0, x1, _ = cols.indices(W)
        assert plan == (x0, y0, x1, y1, out_size[0], out_size[1]), box
        assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H and min(out_size) >= 1 and max(out_size) <= size
        seen_plan += 1
    assert seen_none >= 4 and seen_plan >= 8


def test_plan_of_the_issue_examples():
    assert face_thumbnail_plan((50, 100, 1050, 103), H, W, 128, 0.0) is None          # 1000 x 3 -> 128 x 0: Pillow raises
    assert face_thumbnail_plan((1300, 300, 1400, 380), H, W) is None
    assert face_thumbnail_plan((100, 100, 130, 130), 256, 320) == (91, 91, 139, 139, 128, 128)      # 30 px face: 48 px crop, upscaled
    assert face_thumbnail_plan((0, 0, 320, 256), 256, 320, 128, 0.0) == (0, 0, 320, 256, 128, 102)


def test_helper_returns_the_bytes_of_its_earlier_body():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (200, 260, 3), dtype=np.uint8)
    img[:, 130:] = (np.arange(130)[None, :, None] + np.arange(200)[:, None, None] // 2).astype(np.uint8)
    for size, quality, box in ((128, 85, (40, 30, 150, 170)), (128, 50, (-20, 120, 90, 230)), (96, 95, (180, 10, 215, 44))):
        want = earlier_body(img, box, size, quality)
        got = analyzer(size, quality)._crop_face_thumbnail(img, np.asarray(box))
        assert want is not None and got == want[0]
    assert analyzer()._crop_face_thumbnail(img, (400, 300, 450, 350)) is None
