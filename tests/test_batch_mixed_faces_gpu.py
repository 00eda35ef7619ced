"""GPU: BatchScorer(mixed_sizes=True) with a face analyzer computes the face dicts of a whole chunk of mixed sizes with one
fe_face_analyze_mixed call, one fe_roi_laplacian_mixed call (and one fe_face_thumbnails_mixed call with gpu_thumbnails) on the resident
RGB pixels - no per-shape face call, no BGR copy - and returns the dicts of mixed_sizes=False.

Ten images of eight shapes from tests/face_mixed_cases.py (BATCH; the scorer takes them as RGB, the detector sees their B,G,R twins, which
are the arrays whose threshold margins tests/test_face_mixed_host.py checks). Float face fields are held to the bounds of
tests/test_face_mixed_gpu.py: the graphs may sum in another order in another batch."""
import contextlib

import numpy as np
import pytest

import face_mixed_cases as FC
from facet_amd._lib import FE_MODEL_TOPIQ
from facet_amd.batch import BatchScorer
from facet_amd.face import FaceAnalyzer
from facet_amd.weights import synthetic_state_dict
from standins import synthetic_onnx as S

pytestmark = pytest.mark.gpu

FACE_FLOAT_KEYS = ('face_sharpness', 'raw_eye_sharpness', 'isolation_bonus', 'face_confidence', '_isolation_bonus_raw')


class _Calls:
    """Counts the calls of some Engine methods of one context (tests/test_stats_mixed_gpu.py)."""
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


def _analyzer(engine, gpu_thumbnails):
    det, _ = S.scrfd_like(seed=12, size=320)
    lmk, _ = S.landmark_like(seed=13)
    rec, _ = S.arcface_iresnet(layers=(1, 1, 1, 1), seed=14)
    fa = FaceAnalyzer(min_confidence=FC.DET_THRESH, min_face_size=10, engine=engine, models={"det": det, "lmk": lmk, "rec": rec},
                      gpu_thumbnails=gpu_thumbnails)
    assert fa.available
    fa.face_app.det_size, fa.face_app.det_thresh, fa.face_app.nms_thresh = FC.DET_SIZE, FC.DET_THRESH, FC.NMS_THRESH
    fa.face_app.max_candidates, fa.face_app.max_faces = 4096, 256
    return fa


def _close(a, b, rel):
    return abs(a - b) <= rel * abs(b)


def _same_dicts(got, want):
    assert len(got) == len(want)
    worst = 0.0
    for i, (g, r) in enumerate(zip(got, want)):
        assert g.keys() == r.keys(), i
        for key in r:
            if key in ('aesthetic', 'quality_score'):      # TOPIQ on a mixed call against a uniform batch: tests/test_mixed_gpu.py
                assert g[key] == pytest.approx(r[key], abs=0.011), (i, key)
            elif key in FACE_FLOAT_KEYS:
                worst = max(worst, abs(g[key] - r[key]) / abs(r[key]) if r[key] else abs(g[key]))
                assert _close(g[key], r[key], 1e-6), (i, key, g[key], r[key])
            elif key == '_face_bbox':
                assert (g[key] is None) == (r[key] is None) and (r[key] is None or np.array_equal(g[key], r[key])), (i, key)
            elif key == 'face_details':
                assert len(g[key]) == len(r[key]), i
                for fg, fr in zip(g[key], r[key]):
                    assert fg.keys() == fr.keys() and fg['index'] == fr['index'] and fg['bbox'] == fr['bbox'], i
                    assert abs(fg['confidence'] - fr['confidence']) < 1e-4, i
                    eg, er = np.frombuffer(fg['embedding'], np.float32), np.frombuffer(fr['embedding'], np.float32)
                    assert np.abs(eg - er).max() < 1e-4 * np.abs(er).max(), i
                    lg, lr = np.frombuffer(fg['landmark_2d_106'], np.float32), np.frombuffer(fr['landmark_2d_106'], np.float32)
                    assert np.abs(lg - lr).max() < 1e-4 * max(1.0, np.abs(lr).max()), i
                    assert fr['thumbnail'] is not None and fr['thumbnail'][:2] == b"\xff\xd8"
                    assert fg['thumbnail'] == fr['thumbnail'], i      # Pillow's bytes on either path, or the engine's on both
            else:
                if isinstance(r[key], float) and np.isnan(r[key]):
                    assert np.isnan(g[key]), (i, key)
                else:
                    assert g[key] == r[key], (i, key)
    print(f"[batch mixed faces] worst relative difference of a float face field: {worst:.2e}")


@pytest.mark.parametrize("aux", [False, True], ids=["one_context", "aux_engine"])
def test_one_face_call_per_chunk_and_the_same_dicts(aux):
    from facet_amd import Engine
    e = Engine(0, arena_bytes=4 << 30)
    e2 = Engine(0, arena_bytes=2 << 30) if aux else None
    try:
        e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
        face_eng = e2 if aux else e
        arrs = [np.ascontiguousarray(a[..., ::-1]) for a in FC.images(FC.BATCH)]
        assert len(arrs) == 10 and len({a.shape for a in arrs}) == 8
        names = ("face_analyze", "face_analyze_mixed", "roi_laplacian", "roi_laplacian_mixed", "face_thumbnails", "face_thumbnails_mixed", "swap_rb", "d2h")
        for gpu_thumbnails in (False, True):
            fa = _analyzer(face_eng, gpu_thumbnails)
            want = BatchScorer(e, face_analyzer=fa, aux_engine=e2).process_images(arrs)
            # the stand-in detector's boxes mostly have a negative width; by the CPU oracle six of them pass min_face_size, in four images
            assert sum(r['face_count'] for r in want) >= 5 and sum(r['face_count'] > 0 for r in want) >= 3 and all('face_details' in r for r in want)
            with contextlib.ExitStack() as stack:
                main = stack.enter_context(_Calls(e, names))
                side = stack.enter_context(_Calls(e2, names)) if aux else main
                got = BatchScorer(e, face_analyzer=fa, mixed_sizes=True, aux_engine=e2).process_images(arrs)
            # one face call and one ROI call for the ten images of eight shapes, on the analyzer's context; none per shape; no BGR copy
            assert side["face_analyze_mixed"] == 1 and side["roi_laplacian_mixed"] == 1, (main, side)
            assert main["face_analyze"] == 0 and side["face_analyze"] == 0 and main["roi_laplacian"] == 0 and side["roi_laplacian"] == 0
            assert main["swap_rb"] == 0 and side["swap_rb"] == 0
            assert side["face_thumbnails_mixed"] == (1 if gpu_thumbnails else 0) and side["face_thumbnails"] == 0 and main["face_thumbnails"] == 0
            if gpu_thumbnails:      # the thumbnails are cut on the engine: no pixels come back to the host
                assert main["d2h"] == 0 and side["d2h"] == 0
            _same_dicts(got, want)
            fa.face_app.unload()
    finally:
        e.close()
        if e2 is not None:
            e2.close()
