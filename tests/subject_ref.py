"""CPU restatement of subject-region detection - TEST INFRASTRUCTURE ONLY (never imported by facet_amd/).

What reference analyzers/composition.py:16-75 asks OpenCV for, in plain Python / numpy:
    gray = cv2.cvtColor(img, COLOR_BGR2GRAY); med = np.median(gray); edges = cv2.Canny(gray, int(max(0, .5 med)), int(min(255, 1.5 med)))
    contours, _ = cv2.findContours(edges, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE); cv2.contourArea / cv2.moments / cv2.boundingRect
Canny is oracle.lines_ref.canny_u8 (imported). findContours is Suzuki & Abe's raster scan with border marking (algorithm 1): every
outer and hole border is followed and numbered, each gets its parent border, and RETR_EXTERNAL keeps the outer borders whose parent is
the frame. That is a different route from facet_amd/csrc/kernels_contours.hip (component labelling + a frame test on the background),
so agreement checks both. scipy.ndimage gives a second opinion on the topology (`topology_scipy`).
[DEP-KNOWLEDGE] cv2 is not installed: parity with cv2 itself is unpinned."""
import numpy as np
from scipy import ndimage

from oracle.lines_ref import canny_u8
from oracle.technical_ref import bgr2gray

FIELDS = 8
# (di, dj) by direction 0 = E, 1 = NE, 2 = N, ... counter-clockwise on the screen (rows grow downwards)
N8 = [(0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1)]


def scene(h, w, seed, noise, kind="mixed"):
    """Seeded BGR test scenes: a filled disc, bars, a gradient and graded noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    img = np.full((h, w, 3), 60, np.int32)
    if kind == "flat":
        return np.full((h, w, 3), 117, np.uint8)
    if kind == "gradient":                       # smooth ramp: the ramp itself stays far below the thresholds
        img = np.stack([40 + xx * 60 // w, 50 + yy * 50 // h, 45 + (xx + yy) * 40 // (h + w)], -1).astype(np.int32)
        img[xx > w * 0.55] += 90                     # one step from top to bottom: a one-pixel-wide open edge curve, area 0
        return np.clip(img, 0, 255).astype(np.uint8)
    if kind in ("mixed", "disc"):
        cy, cx, r = h * (0.35 + 0.3 * rng.random()), w * (0.3 + 0.4 * rng.random()), min(h, w) * (0.12 + 0.1 * rng.random())
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = (200, 170, 90)
    if kind in ("mixed", "bars"):
        img[h // 6:h // 6 + max(3, h // 12), w // 10:w - w // 8] = (30, 210, 220)
        img[h // 2:h - h // 7, w - w // 4:w - w // 4 + max(3, w // 14)] = (230, 60, 40)
    img += (xx[..., None] * 30 // w)
    if noise:
        img += rng.integers(-noise, noise + 1, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def median_thresholds(gray):
    med = np.median(gray)
    return int(max(0, 0.5 * med)), int(min(255, 1.5 * med))


def _follow(f, i, j, start_dir, nbd):
    """Suzuki & Abe steps 3.1-3.5 on the padded int image f; returns the border's pixels [(x, y), ...] in padded coordinates."""
    first = None
    for k in range(1, 9):                                   # 3.1: clockwise from the start neighbour
        d = (start_dir - k) % 8
        if f[i + N8[d][0], j + N8[d][1]] != 0:
            first = d
            break
    if first is None:
        f[i, j] = -nbd
        return [(j, i)]
    i1, j1 = i + N8[first][0], j + N8[first][1]
    i3, j3, d2 = i, j, first                                # d2: direction from (i3, j3) to (i2, j2)
    pts = []
    while True:
        east_zero = False
        for k in range(1, 9):                               # 3.3: counter-clockwise, starting after (i2, j2)
            d = (d2 + k) % 8
            if f[i3 + N8[d][0], j3 + N8[d][1]] != 0:
                break
            if d == 0:
                east_zero = True
        i4, j4 = i3 + N8[d][0], j3 + N8[d][1]
        if east_zero:                                       # 3.4
            f[i3, j3] = -nbd
        elif f[i3, j3] == 1:
            f[i3, j3] = nbd
        pts.append((j3, i3))
        if (i4, j4) == (i, j) and (i3, j3) == (i1, j1):     # 3.5
            return pts
        d2 = (d + 4) % 8
        i3, j3 = i4, j4


def find_external_contours(binary):
    """-> list of int arrays [k,2] (x, y): the full chains of the outer borders whose parent is the frame, the one found last first."""
    b = np.asarray(binary) != 0
    h, w = b.shape
    f = np.zeros((h + 2, w + 2), np.int64)
    f[1:-1, 1:-1] = b
    nbd = 1
    is_hole = {1: True}                                     # the frame counts as a hole border
    parent = {1: 0}
    found = []
    for i in range(1, h + 1):
        lnbd = 1
        row = f[i]
        for j in np.nonzero(row)[0]:                        # zero pixels start nothing and do not change lnbd
            v = f[i, j]
            outer = v == 1 and f[i, j - 1] == 0
            hole = (not outer) and v >= 1 and f[i, j + 1] == 0
            if outer or hole:
                nbd += 1
                if hole and v > 1:
                    lnbd = int(v)
                is_hole[nbd] = hole
                parent[nbd] = lnbd if is_hole[lnbd] != hole else parent[lnbd]
                pts = _follow(f, i, j, 4 if outer else 0, nbd)
                if outer and parent[nbd] == 1:
                    found.append(np.array(pts, np.int64) - 1)
            if f[i, j] != 1:
                lnbd = abs(int(f[i, j]))
    return found[::-1]


def approx_simple(pts):
    """CHAIN_APPROX_SIMPLE: keep the points where the chain changes direction (and the first one)."""
    n = len(pts)
    if n <= 2:
        return pts
    step = np.roll(pts, -1, 0) - pts
    keep = np.any(step != np.roll(step, 1, 0), axis=1)
    keep[0] = True
    return pts[keep]


def green_sums(pts):
    a00 = a10 = a01 = 0
    n = len(pts)
    for k in range(n):
        px, py = int(pts[k][0]), int(pts[k][1])
        qx, qy = int(pts[(k + 1) % n][0]), int(pts[(k + 1) % n][1])
        d = px * qy - qx * py
        a00 += d
        a10 += d * (px + qx)
        a01 += d * (py + qy)
    return a00, a10, a01


def records(binary, min_twice_area=0):
    """The records fe_external_contours returns for one image: int64 [k, 8], and the step count of every reported border."""
    w = np.asarray(binary).shape[1]
    out, steps = [], []
    for c in find_external_contours(binary):
        a00, a10, a01 = green_sums(c)
        assert (a00, a10, a01) == green_sums(approx_simple(c))
        if abs(a00) < min_twice_area:
            continue
        out.append([int(c[0][1]) * w + int(c[0][0]), a00, a10, a01, int(c[:, 0].min()), int(c[:, 1].min()), int(c[:, 0].max()), int(c[:, 1].max())])
        steps.append(0 if len(c) == 1 else len(c))
    return np.array(out, np.int64).reshape(-1, FIELDS), steps


def topology_scipy(binary):
    """Second opinion: (first pixel index, x_min, y_min, x_max, y_max, external) of every 8-connected component, by descending first
    pixel. External = not inside the filled holes of the other components."""
    b = np.asarray(binary) != 0
    w = b.shape[1]
    lab, k = ndimage.label(b, structure=np.ones((3, 3), int))
    out = []
    for c, sl in enumerate(ndimage.find_objects(lab), 1):
        comp = lab == c
        inside = ndimage.binary_fill_holes(b & ~comp)
        out.append((int(np.flatnonzero(comp)[0]), sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1, not bool((inside & comp).any())))
    return sorted(out, reverse=True)


def subject_records(bgr):
    """One image through the restated pipeline -> (records int64 [k,8], (lower, upper), edges uint8 [h,w])."""
    gray = bgr2gray(bgr)
    h, w = gray.shape
    lo, hi = median_thresholds(gray)
    edges = canny_u8(gray, lo, hi)
    rec, _ = records(edges, (h * w + 4999) // 5000)
    return rec, (lo, hi), edges


# ---- the cv2 calls of detect_subject_region, for running the reference's own function (tests/golden/make_subject_golden.py) ----------
def fake_cv2(module):
    module.COLOR_BGR2GRAY, module.RETR_EXTERNAL, module.CHAIN_APPROX_SIMPLE = 6, 0, 2
    module.error = type("error", (Exception,), {})
    module.cvtColor = lambda img, code: bgr2gray(img)
    module.Canny = lambda g, lo, hi: canny_u8(g, lo, hi)
    module.findContours = lambda e, mode, method: (tuple(approx_simple(c).astype(np.int32)[:, None, :] for c in find_external_contours(e)), None)

    def contour_area(c):
        return abs(green_sums(np.asarray(c).reshape(-1, 2))[0]) * 0.5

    def moments(c):
        a00, a10, a01 = green_sums(np.asarray(c).reshape(-1, 2))
        sgn = -1 if a00 < 0 else 1
        return {"m00": sgn * a00 / 2, "m10": sgn * a10 / 6, "m01": sgn * a01 / 6}

    def bounding_rect(c):
        p = np.asarray(c).reshape(-1, 2)
        return int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max() - p[:, 0].min() + 1), int(p[:, 1].max() - p[:, 1].min() + 1)

    module.contourArea, module.moments, module.boundingRect = contour_area, moments, bounding_rect
    return module
