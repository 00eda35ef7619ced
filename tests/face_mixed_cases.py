"""Images of mixed sizes for the mixed-size face tests, with the stand-in graphs of tests/test_face_gpu.py at det_size 320 x 320.

DETECT: the shapes (h, w) that reach every route of the detector-input kernel at det_size 320: (640, 640) the exact-2x box average;
(200, 320) and (320, 320) a copy; (300, 500) wide with a truncated new_h (192); (400, 300) the tall branch; (97, 131) an upscale;
(8, 600) a new_h of 4; (1, 1). BATCH: ten images of eight shapes the whole ensemble takes as well (BatchScorer), among them two shapes
twice with different pixels.

Every image is uniform noise from its own seed. The seeds were chosen so that, by oracle.face_ref.scrfd_detect on the CPU with
S.scrfd_like(seed=12, size=320), no candidate score lies within 1e-3 of DET_THRESH and no overlap NMS looks at lies within 1e-3 of
NMS_THRESH (seeds 0 .. 79 were tried in order per image; `margins` is the check, tests/test_face_mixed_host.py runs it). GPU and CPU
detector outputs differ by about 1e-5, so a face count can then differ between two engine routes only through a real fault. The stand-in
detector's scores crowd around 0.5, where no seed of 80 gave that margin; 0.56 is the lowest threshold tried at which seeds exist."""
import numpy as np

DET_SIZE = (320, 320)
DET_THRESH, NMS_THRESH = 0.56, 0.4
# (h, w), seed
CASES = [((640, 640), 42), ((200, 320), 20), ((320, 320), 7), ((300, 500), 1), ((400, 300), 5), ((97, 131), 0), ((8, 600), 0), ((1, 1), 0),
         ((64, 96), 3), ((40, 400), 0), ((200, 320), 5), ((320, 320), 7)]
DETECT = list(range(8))
BATCH = [0, 1, 2, 3, 4, 5, 8, 9, 10, 11]


def image(k):
    """Case k as a BGR uint8 [h, w, 3] array."""
    (h, w), seed = CASES[k]
    return np.random.default_rng(1000 * seed + k).integers(0, 256, (h, w, 3), dtype=np.uint8)


def images(which=DETECT):
    return [image(k) for k in which]


def margins(det_onnx, img):
    """(distance of the nearest candidate score to DET_THRESH, distance of the nearest overlap NMS computes to NMS_THRESH, candidates at
    or above DET_THRESH, faces kept) of a BGR image, by oracle.face_ref.scrfd_detect. 1.0 where there is nothing to compare."""
    from oracle import face_ref
    seen = {}
    real = face_ref.nms

    def spy(dets, thresh):
        seen['dets'] = dets.copy()
        return []

    face_ref.nms = spy
    try:
        face_ref.scrfd_detect(det_onnx, img, DET_SIZE, DET_THRESH - 2e-3, NMS_THRESH)
    finally:
        face_ref.nms = real
    s = seen['dets'][:, 4]
    d = seen['dets'][s >= DET_THRESH]
    x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = d[:, 4].argsort()[::-1]
    near, kept = 1.0, 0
    while order.size > 0:      # the loop of face_ref.nms
        i, rest = order[0], order[1:]
        kept += 1
        w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
        h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
        ovr = w * h / (areas[i] + areas[rest] - w * h)
        if ovr.size:
            near = min(near, float(np.abs(ovr - NMS_THRESH).min()))
        order = rest[ovr <= NMS_THRESH]
    return (float(np.abs(s - DET_THRESH).min()) if s.size else 1.0), near, int(d.shape[0]), kept
