"""GPU: BatchScorer(mixed_sizes=True, detect_lines=True, subject_region=True) computes the line scores and the subject boxes of a chunk
with one fe_leading_lines_mixed and one fe_subject_region_mixed call on the resident RGB pixels - no per-shape fe_leading_lines /
fe_subject_region, no BGR copy - and returns the dicts of the per-shape path. Seeded stand-in weights, as tests/test_mixed_gpu.py loads
them."""
import contextlib
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subject_ref as S                                   # noqa: E402

from facet_amd._lib import FE_MODEL_TOPIQ                 # noqa: E402
from facet_amd.batch import BatchScorer                   # noqa: E402
from facet_amd.weights import synthetic_state_dict        # noqa: E402

pytestmark = pytest.mark.gpu

SIX = [(120, 160), (160, 120), (130, 130), (120, 160), (97, 131), (130, 130)]      # four shapes, two of them twice and not as neighbours
NAMES = ("leading_lines", "leading_lines_mixed", "subject_contours", "subject_contours_mixed", "swap_rb", "image_stats_mixed", "phash_mixed",
         "thumbnail_jpeg_mixed")


class _Calls:
    """Counts the calls of some Engine methods of one context (tests/test_batch_mixed_index_gpu.py's wrapper)."""
    def __init__(self, eng, names):
        self.eng, self.names, self.count = eng, names, {n: 0 for n in names}

    def __enter__(self):
        for n in self.names:
            real = getattr(self.eng, n)

            def spy(*a, _real=real, _n=n, **kw):
                self.count[_n] += 1
                return _real(*a, **kw)
            setattr(self.eng, n, spy)
        return self.count

    def __exit__(self, *exc):
        for n in self.names:
            delattr(self.eng, n)      # the instance attribute goes, the method of the class is back


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def lines_scene(h, w, seed, noise):
    """tests/test_lines_gpu.py's scene (BGR): bars, a diagonal band, a disc and graded noise - long straight edges"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), 50, np.int32)
    img[h // 5:h // 5 + 5, w // 10:w - w // 10] = (200, 180, 90)
    img[h // 8:h - h // 8, w // 3:w // 3 + 4] = (30, 220, 220)
    for t in range(min(h, w) - 30):
        img[12 + t, 8 + t:14 + t] = (240, 240, 240)
    yy, xx = np.mgrid[:h, :w]
    img[(yy - h * 0.7) ** 2 + (xx - w * 0.7) ** 2 < (min(h, w) * 0.15) ** 2] = (120, 40, 200)
    img += (xx[..., None] * 40 // w)
    img += rng.integers(-noise, noise + 1, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def photos():
    """RGB photos: three with long straight edges (lines found), three of tests/subject_ref.py's scenes (short bars and a disc: none)"""
    bgr = [lines_scene(*SIX[0], 60, 0), S.scene(*SIX[1], 61, 6, "bars"), lines_scene(*SIX[2], 62, 25), S.scene(*SIX[3], 63, 25, "mixed"),
           lines_scene(*SIX[4], 64, 0), S.scene(*SIX[5], 65, 0, "disc")]
    return [np.ascontiguousarray(im[..., ::-1]) for im in bgr]


@pytest.mark.parametrize("aux", [False, True], ids=["one_context", "aux_engine"])
def test_one_call_each_no_bgr_copy_and_the_same_dicts(aux):
    from facet_amd import Engine
    e = Engine(0, arena_bytes=2 << 30)
    e2 = Engine(0, arena_bytes=1 << 30) if aux else None
    try:
        e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
        arrs = photos()
        kw = dict(detect_lines=True, subject_region=True, thumbnails=True, phash=True, thumbnail_size=96)
        want = BatchScorer(e, **kw).process_images(arrs)
        with contextlib.ExitStack() as stack:
            main = stack.enter_context(_Calls(e, NAMES))
            side = stack.enter_context(_Calls(e2, NAMES)) if aux else main
            got = BatchScorer(e, mixed_sizes=True, aux_engine=e2, **kw).process_images(arrs)
        for c in {id(main): main, id(side): side}.values():
            assert c["leading_lines"] == 0 and c["subject_contours"] == 0 and c["swap_rb"] == 0, c
        assert side["leading_lines_mixed"] == 1 and side["subject_contours_mixed"] == 1 and side["image_stats_mixed"] == 1, side      # on the aux context when there is one
        if aux:
            assert main["leading_lines_mixed"] == 0 and main["subject_contours_mixed"] == 0, main
        assert len(got) == len(want) == 6
        for i, (g, r) in enumerate(zip(got, want)):
            assert g.keys() == r.keys() and 'leading_lines_score' in r and 'power_point_score' in r and 'comp_score' in r, i
            assert (g['image_height'], g['image_width']) == SIX[i]
            for key in r:
                if key in ('aesthetic', 'quality_score'):      # TOPIQ on a mixed call against a uniform batch: tests/test_mixed_gpu.py
                    assert g[key] == pytest.approx(r[key], abs=0.011), (i, key)
                else:
                    assert _same(g[key], r[key]), (i, key)
        for key in ('leading_lines_score', 'power_point_score', 'comp_score'):      # not a comparison of constants
            assert len({r[key] for r in want}) > 1, key
        # scores passed in win over detection, as on the per-shape path: no lines call at all
        given = [float(i) for i in range(6)]
        with _Calls(e2 if aux else e, NAMES) as c:
            res = BatchScorer(e, mixed_sizes=True, aux_engine=e2, **kw).process_images(arrs, leading_lines=given)
        assert c["leading_lines_mixed"] == 0 and c["subject_contours_mixed"] == 1 and [r['leading_lines_score'] for r in res] == given
    finally:
        e.close()
        if e2 is not None:
            e2.close()
