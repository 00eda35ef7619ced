"""CPU: the host side of the thumbnail feature.

* facet_amd.thumbnail.thumbnail_plan against Pillow itself over a sweep of (w, h, size): the output size of `Image.thumbnail`, the
  factors and the box `Image.thumbnail` hands to `Image.reduce` (recorded by wrapping the method), and the resize box, observed through
  the pixels: `im.reduce(f, box).resize(size, LANCZOS, box2)` with the planned values must equal `thumbnail`'s result.
* tests/golden/thumbnail_golden.npz (written by tests/golden/make_thumbnail_golden.py from the reference's own
  generate_photo_thumbnail) reproduces from its generator with the reference's four Pillow calls restated here."""
import hashlib
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

from facet_amd.thumbnail import thumbnail_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_thumbnail_golden as gold_gen  # noqa: E402

# (w, h, size)
SWEEP = [
    (1024, 1024, 640), (200, 136, 48), (1000, 700, 160), (4000, 3000, 640), (53, 37, 640),      # the sizes measured for the issue
    (640, 640, 640), (641, 640, 640), (640, 641, 640), (639, 300, 640),                         # at and around "already small enough"
    (1001, 333, 100), (333, 1001, 100), (997, 13, 64), (13, 997, 64), (2000, 30, 640),          # sides no multiple of the factor, strips
    (3000, 200, 64), (200, 3000, 64), (1500, 1000, 50), (90, 300, 64), (700, 500, 33),          # factors that differ per axis
    (10, 2000, 640), (8, 4000, 300), (5, 1200, 100), (3, 301, 64), (3, 300, 64),                # more than 100 times taller than wide
    (4000, 8, 300), (1, 1, 640), (1, 5000, 640), (5000, 1, 640), (257, 255, 17), (4096, 4095, 1),
]


def pil_thumbnail(pil_img, size=640, quality=80):
    """The reference's generate_photo_thumbnail (utils/image_transforms.py:46-50)."""
    thumb = pil_img.copy()
    thumb.thumbnail((size, size), Image.Resampling.LANCZOS)
    buf = io.BytesIO()
    thumb.save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def test_plan_of_the_issues_table():
    for (w, h, size), want in {(1024, 1024, 640): (640, 640), (200, 136, 48): (48, 33), (1000, 700, 160): (160, 112),
                               (4000, 3000, 640): (640, 480), (53, 37, 640): (53, 37)}.items():
        assert thumbnail_plan(w, h, size).size == want
    p = thumbnail_plan(1000, 700, 160)
    assert p.factors == (3, 3) and p.reduce_box == (0, 0, 1000, 700) and p.resize_box == (0.0, 0.0, 1000 / 3, 700 / 3) and not p.tall
    assert thumbnail_plan(53, 37, 640).unchanged and thumbnail_plan(640, 640, 640).unchanged and not thumbnail_plan(641, 640, 640).unchanged


@pytest.mark.parametrize("w,h,size", SWEEP)
def test_plan_equals_pillow(monkeypatch, w, h, size):
    rng = np.random.default_rng(w * 7919 + h * 31 + size)
    src = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    calls = []
    real_reduce = Image.Image.reduce

    def recording_reduce(self, factor, box=None):
        calls.append((tuple(factor) if isinstance(factor, (tuple, list)) else (factor, factor), box))
        return real_reduce(self, factor, box)

    monkeypatch.setattr(Image.Image, "reduce", recording_reduce)
    want = src.copy()
    want.thumbnail((size, size), Image.Resampling.LANCZOS)
    monkeypatch.undo()
    plan = thumbnail_plan(w, h, size)
    assert plan.size == want.size
    assert plan.unchanged == (want.size == (w, h))
    if plan.factors == (1, 1):
        assert calls == [] and plan.reduce_box is None
    else:
        assert calls == [(plan.factors, plan.reduce_box)]
    # the boxes, through the pixels
    im = src
    if plan.factors != (1, 1):
        im = im.reduce(plan.factors, plan.reduce_box)
    if not plan.unchanged:
        assert plan.tall == (im.size[1] > im.size[0] * 100 and plan.size[1] < im.size[1])
        if plan.tall:      # what Image.resize does with such an image, spelled out on the core object
            core = im.im.resize((im.size[0], plan.size[1]), Image.Resampling.LANCZOS, (0, plan.resize_box[1], im.size[0], plan.resize_box[3]))
            core = core.resize(plan.size, Image.Resampling.LANCZOS, (plan.resize_box[0], 0, plan.resize_box[2], plan.size[1]))
            im = im._new(core)
        else:
            im = im._new(im.im.resize(plan.size, Image.Resampling.LANCZOS, plan.resize_box))
    assert im.size == want.size and np.array_equal(np.asarray(im), np.asarray(want))


def test_golden_reproduces_from_its_generator():
    g = np.load(os.path.join(GOLDEN, "thumbnail_golden.npz"))
    again = gold_gen.generate(pil_thumbnail)
    assert sorted(again) == sorted(g.files)
    for k in g.files:
        assert np.array_equal(g[k], again[k]), f"{k}: this Pillow build writes other bytes than the one the golden was made with"
    for i, name in enumerate(g["names"].tolist()):
        if "jpeg_" + name in g.files:
            data = g["jpeg_" + name].tobytes()
            assert len(data) == int(g["lengths"][i]) and hashlib.sha256(data).hexdigest() == str(g["sha256"][i])
            assert Image.open(io.BytesIO(data)).size == thumbnail_plan(int(g["meta"][i][2]), int(g["meta"][i][1]), int(g["meta"][i][3])).size
