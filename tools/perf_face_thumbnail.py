"""fe_face_thumbnails rates (profiles/face_thumbnail_perf.txt).
usage: perf_face_thumbnail.py [call] [step]      (no argument: both parts)
  call: 256 x 1024x1024 resident BGR images, 2 face boxes per image with sides of 40 .. 600 px (log-uniform, some over a border),
        thumbnail_size 128, quality 85: median of 10 calls (min, max) of facet_amd.face.face_thumbnails - plans, one engine call, bytes
        copied back - for photo-like and for noise content; the same call on boxes whose crop already has the output size (both resample
        passes are the identity: what is left is the encoder and the copies); and the host path of the parent commit
        (FaceAnalyzer._crop_face_thumbnail before the plan was factored out: slice, Pillow BOX resize, Pillow JPEG) on the same boxes,
        one process alone and 16 side by side. A per-kernel split comes from
        `rocprofv3 --kernel-trace --stats -- python tools/perf_face_thumbnail.py call`.
  step: BatchScorer.process_files (five models; statistics and faces on a second context) on 64 JPEG files of 1024x1024 with the
        stand-in face graphs, gpu_thumbnails off / on; the faces found and their thumbnails are counted."""
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facet_amd import Engine          # noqa: E402
from facet_amd.face import FaceAnalyzer, face_thumbnail_plan, face_thumbnails          # noqa: E402

parts = set(sys.argv[1:]) or {"call", "step"}
N, HW, SIZE, QUALITY = 256, 1024, 128, 85


def stats_ms(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def photo_like(seed, hw):
    """Smooth colour waves plus sensor-like noise: compresses like a photograph (tools/perf_thumbnail.py)."""
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, 1.0, hw)[:, None]
    x = np.linspace(0.0, 1.0, hw)[None, :]
    img = np.empty((hw, hw, 3), np.float64)
    for c in range(3):
        acc = np.full((hw, hw), 128.0 + rng.uniform(-30.0, 30.0))
        for _ in range(4):
            fy, fx = rng.uniform(0.3, 3.5, 2)
            acc = acc + rng.uniform(15.0, 45.0) * np.sin(2.0 * np.pi * (fy * y + fx * x) + rng.uniform(0.0, 2.0 * np.pi))
        img[..., c] = acc + rng.normal(0.0, 6.0, (hw, hw))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def face_boxes(seed, n):
    """2 boxes per image: sides 40 .. 600 px log-uniform, aspect 0.75 .. 1.33, centres anywhere (so some hang over a border)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        boxes = []
        for _ in range(2):
            side = float(np.exp(rng.uniform(np.log(40.0), np.log(600.0))))
            bw, bh = side * rng.uniform(0.75, 1.0), side * rng.uniform(0.75, 1.0)
            cx, cy = rng.uniform(0.1 * HW, 0.9 * HW, 2)
            boxes.append((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2))
        out.append(boxes)
    return out


def parent_host_path(img_cv, bbox, padding=0.3):
    """FaceAnalyzer._crop_face_thumbnail of the parent commit (thumbnail_size 128, thumbnail_quality 85)."""
    from PIL import Image
    left, top, right, bottom = (int(v) for v in bbox)
    grow_x, grow_y = int((right - left) * padding), int((bottom - top) * padding)
    crop = img_cv[slice(max(0, top - grow_y), min(img_cv.shape[0], bottom + grow_y)), slice(max(0, left - grow_x), min(img_cv.shape[1], right + grow_x))]
    if crop.size == 0:
        return None
    factor = SIZE / max(crop.shape[0], crop.shape[1])
    thumb = Image.fromarray(np.ascontiguousarray(crop[:, :, ::-1])).resize((int(crop.shape[1] * factor), int(crop.shape[0] * factor)), Image.BOX)
    out = io.BytesIO()
    thumb.save(out, format='JPEG', quality=QUALITY)
    return out.getvalue()


def cpu_host_path(seed, images=8):
    """One worker of the CPU leg: the 2 * `images` faces of `images` photo-like images, serially as FaceAnalyzer._post does."""
    base = photo_like(seed % 8, HW)[..., ::-1]
    boxes = face_boxes(1000 + seed, images)
    t0 = time.perf_counter()
    for i in range(images):
        img = np.roll(base, 37 * i, axis=1)
        for b in boxes[i]:
            parent_host_path(img, b)
    return time.perf_counter() - t0


if "call" in parts:
    # the CPU leg first: its 16 worker processes are forked before this process opens the GPU
    import multiprocessing as mp
    cpu_host_path(0)
    one = cpu_host_path(0) / 16
    with mp.get_context("fork").Pool(16) as pool:
        pool.map(cpu_host_path, range(16), chunksize=1)          # warm the workers
        secs = pool.map(cpu_host_path, range(100, 116), chunksize=1)     # 16 loops side by side, each timing itself
    print(f"host path of the parent commit (slice + Pillow BOX + Pillow JPEG; np.roll of the image included): {one * 1e3:.3f} ms/face with one process alone "
          f"({1 / one:.0f} faces/s); 16 processes side by side, 16 faces each: slowest loop {max(secs):.3f} s = {max(secs) / 256 * 1e3:.3f} ms/face over the 16 CPUs "
          f"({256 / max(secs):.0f} faces/s)", flush=True)
    e = Engine(0, arena_bytes=8 << 30)
    boxes = face_boxes(7, N)
    plans = [face_thumbnail_plan(b, HW, HW, SIZE) for bs in boxes for b in bs]
    sides = sorted(max(p[2] - p[0], p[3] - p[1]) for p in plans if p)
    print(f"{N} x {HW}x{HW}, {len(plans)} boxes, {sum(p is not None for p in plans)} with a plan; crop long edge min {sides[0]}, median {sides[len(sides) // 2]}, "
          f"max {sides[-1]} px; {sum(s < SIZE for s in sides)} upscaled", flush=True)
    same = [[(100 + 3 * (i % 200), 50 + i % 300, 228 + 3 * (i % 200), 178 + i % 300), (600, 700 - i % 100, 728, 828 - i % 100)] for i in range(N)]
    base = [photo_like(s, HW)[..., ::-1] for s in range(8)]
    for label, imgs in (("photo-like", np.stack([base[i % 8] for i in range(N)])), ("noise", np.random.default_rng(1).integers(0, 256, (N, HW, HW, 3), dtype=np.uint8))):
        d = e.dev_alloc(imgs.nbytes)
        e.h2d(d, imgs)
        dev = (d, N, HW, HW)
        out = face_thumbnails(e, dev, boxes, SIZE, QUALITY)
        blobs = [b for row in out for b in row if b is not None]
        check = [(i, j) for i in range(0, N, 37) for j in range(2)]
        assert all(out[i][j] == parent_host_path(imgs[i], boxes[i][j]) for i, j in check), "bytes differ from the host path"
        med, lo, hi = stats_ms(lambda: face_thumbnails(e, dev, boxes, SIZE, QUALITY))
        print(f"face_thumbnails {label:10s}: median {med:7.2f} ms (min {lo:.2f}, max {hi:.2f}) for {len(blobs)} faces, {sum(map(len, blobs)) / 1e6:.2f} MB of JPEG copied "
              f"back = {med * 1e3 / len(blobs):6.1f} us/face, {len(blobs) / med * 1e3:7.0f} faces/s ({len(check)} faces compared with the host path: equal)", flush=True)
        t0 = time.perf_counter()
        for _ in range(20):
            [face_thumbnail_plan(b, HW, HW, SIZE) for bs in boxes for b in bs]
        t_plan = (time.perf_counter() - t0) / 20 * 1e3
        med2, lo2, hi2 = stats_ms(lambda: face_thumbnails(e, dev, same, SIZE, QUALITY, padding=0.0))
        print(f"   stages {label:10s}: plans in Python {t_plan:.2f} ms; crops of 128x128 (identity resample: encoder + copies) median {med2:.2f} ms (min {lo2:.2f}, max {hi2:.2f}); "
              f"resample of the spread above = the rest, about {med - t_plan - med2:.2f} ms", flush=True)
        e.dev_free(d)
    e.close()

if "step" in parts:
    from PIL import Image
    from standins import synthetic_onnx as S
    from facet_amd._lib import FE_MODEL_TOPIQ, FE_MODEL_CLIP, FE_MODEL_AESTHETIC, FE_MODEL_SAMP, FE_MODEL_U2NETP
    from facet_amd.batch import BatchScorer
    from facet_amd.weights import synthetic_state_dict
    e, e2 = Engine(0, arena_bytes=72 << 30), Engine(0, arena_bytes=8 << 30)
    for mid, name in ((FE_MODEL_TOPIQ, "topiq"), (FE_MODEL_CLIP, "clip"), (FE_MODEL_AESTHETIC, "aesthetic"), (FE_MODEL_U2NETP, "u2netp"), (FE_MODEL_SAMP, "samp_net")):
        e.load_weights(mid, synthetic_state_dict(name, 4))
    e.set_microbatch(32)
    n = 64
    models = {"det": S.scrfd_like(seed=12, size=640)[0], "lmk": S.landmark_like(seed=13)[0], "rec": S.arcface_iresnet(layers=(1, 1, 1, 1), seed=14)[0]}
    fa = FaceAnalyzer(min_confidence=0.55, min_face_size=30, engine=e2, models=models)
    fa.face_app.max_faces = 2      # the bench's shape: 2 faces per image
    base = [photo_like(s, HW) for s in range(8)]
    files = []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(np.roll(base[i % 8], 53 * i, axis=1)).save(buf, "JPEG", quality=92)
        files.append(buf.getvalue())
    scorer = BatchScorer(e, aux_engine=e2, face_analyzer=fa)
    times, recs = {False: [], True: []}, {}
    for flag in (False, True):
        fa.gpu_thumbnails = flag
        scorer.process_files(files[:8])
    for _ in range(5):
        for flag in (False, True):
            fa.gpu_thumbnails = flag
            t0 = time.perf_counter()
            recs[flag] = scorer.process_files(files)
            times[flag].append((time.perf_counter() - t0) * 1e3)
    thumbs = {flag: [d['thumbnail'] for r in recs[flag] for d in r['face_details']] for flag in recs}
    assert thumbs[True] == thumbs[False], "thumbnails differ between the two paths"
    off, on = float(np.median(times[False])), float(np.median(times[True]))
    print(f"BatchScorer.process_files step (aux context), {n} JPEG files of {HW}x{HW}, stand-in face graphs, {len(thumbs[True])} faces accepted "
          f"({sum(t is not None for t in thumbs[True])} thumbnails, equal on both paths): gpu_thumbnails off {off:.1f} ms ({n / off * 1e3:.1f} images/s), on {on:.1f} ms "
          f"({n / on * 1e3:.1f} images/s), difference {on - off:+.1f} ms; runs off {[round(t) for t in times[False]]} on {[round(t) for t in times[True]]}", flush=True)
    e2.close()
    e.close()
