"""GPU: BatchScorer(mixed_sizes=True, phash=True, thumbnails=True) computes the `phash` and `thumbnail` columns of a chunk with one
fe_phash_mixed and one fe_thumbnail_jpeg_mixed call on the resident RGB pixels - no per-shape fe_phash / fe_thumbnail_jpeg, no BGR copy -
and returns the dicts of the per-shape path. Seeded stand-in weights, as tests/test_mixed_gpu.py loads them."""
import contextlib
import math

import numpy as np
import pytest

from facet_amd._lib import FE_MODEL_TOPIQ
from facet_amd.batch import BatchScorer
from facet_amd.weights import synthetic_state_dict
from mixed_cases import images

pytestmark = pytest.mark.gpu

SIX = [(64, 96), (96, 64), (80, 80), (64, 96), (33, 47), (80, 80)]      # four shapes, two of them twice and not as neighbours
NAMES = ("phash", "phash_mixed", "thumbnail_jpeg", "thumbnail_jpeg_mixed", "swap_rb", "image_stats_mixed")


class _Calls:
    """Counts the calls of some Engine methods of one context (tests/test_stats_mixed_gpu.py's wrapper)."""
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


@pytest.mark.parametrize("aux", [False, True], ids=["one_context", "aux_engine"])
def test_one_call_each_no_bgr_copy_and_the_same_dicts(aux):
    from facet_amd import Engine
    e = Engine(0, arena_bytes=2 << 30)
    e2 = Engine(0, arena_bytes=1 << 30) if aux else None
    try:
        e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
        arrs = images(shapes=SIX)
        kw = dict(phash=True, thumbnails=True, thumbnail_size=96)
        want = BatchScorer(e, **kw).process_images(arrs)
        with contextlib.ExitStack() as stack:
            main = stack.enter_context(_Calls(e, NAMES))
            side = stack.enter_context(_Calls(e2, NAMES)) if aux else main
            got = BatchScorer(e, mixed_sizes=True, aux_engine=e2, **kw).process_images(arrs)
        for c in {id(main): main, id(side): side}.values():
            assert c["phash"] == 0 and c["thumbnail_jpeg"] == 0 and c["swap_rb"] == 0, c
        assert side["phash_mixed"] == 1 and side["thumbnail_jpeg_mixed"] == 1 and side["image_stats_mixed"] == 1, side      # on the aux context when there is one
        assert len(got) == len(want) == 6
        for i, (g, r) in enumerate(zip(got, want)):
            assert g.keys() == r.keys() and 'phash' in r and 'thumbnail' in r, i
            assert (g['image_height'], g['image_width']) == SIX[i]
            for key in r:
                if key in ('aesthetic', 'quality_score'):      # TOPIQ on a mixed call against a uniform batch: tests/test_mixed_gpu.py
                    assert g[key] == pytest.approx(r[key], abs=0.011), (i, key)
                else:
                    assert _same(g[key], r[key]), (i, key)
            assert isinstance(g['thumbnail'], bytes) and g['thumbnail'][:2] == b"\xff\xd8" and len(g['phash']) == 16
        assert len({r['phash'] for r in want}) > 1 and len({r['thumbnail'] for r in want}) == 6
    finally:
        e.close()
        if e2 is not None:
            e2.close()
