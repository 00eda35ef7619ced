"""fe_thumbnail_jpeg rates (profiles/thumbnail_perf.txt).
usage: perf_thumbnail.py [thumb] [step]      (no argument: both parts)
  thumb: 256 x 1024x1024 -> 640x640 at quality 80 on a resident batch, bytes copied back included: median of 10 calls (min, max) for
         photo-like and for noise content; the encoder alone on the resident 640x640 batch (the difference is reduce + resize; a per-kernel
         split comes from `rocprofv3 --kernel-trace --stats -- python tools/perf_thumbnail.py thumb`); and the reference's function
         (Pillow) on the CPU, one process alone and 16 side by side
  step:  BatchScorer.process_batch (five models + statistics on a second context), 64 x 1024x1024, thumbnails off / on"""
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facet_amd import Engine          # noqa: E402
from facet_amd.thumbnail import thumbnail_plan, thumbnails          # noqa: E402

HBM_PEAK = 8.0e12                     # MI355X, bytes/s
parts = set(sys.argv[1:]) or {"thumb", "step"}


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
    """Smooth colour waves plus sensor-like noise: compresses like a photograph (about 30 KB at 640 x 640, quality 80)."""
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


def cpu_reference(seed, count=8):
    """One worker of the CPU leg: `count` images through the reference's generate_photo_thumbnail (utils/image_transforms.py:46-50)."""
    from PIL import Image
    base = photo_like(seed, 1024)
    pils = [Image.fromarray(np.roll(base, 37 * i, axis=1)) for i in range(count)]
    t0 = time.perf_counter()
    for im in pils:
        thumb = im.copy()
        thumb.thumbnail((640, 640), Image.Resampling.LANCZOS)
        buf = io.BytesIO()
        thumb.save(buf, format="JPEG", quality=80)
    return time.perf_counter() - t0


if "thumb" in parts:
    # the CPU leg first: its 16 worker processes are forked before this process opens the GPU
    import multiprocessing as mp
    one = cpu_reference(0) / 8
    with mp.get_context("fork").Pool(16) as pool:
        pool.map(cpu_reference, range(16), chunksize=1)          # warm the workers
        secs = pool.map(cpu_reference, range(100, 116), chunksize=1)     # 16 loops side by side, each timing itself
    print(f"reference function (Pillow) on the CPU: {one * 1e3:.2f} ms/image with one process alone ({1 / one:.0f} images/s); 16 processes side by side, "
          f"8 images each: slowest loop {max(secs):.3f} s = {max(secs) / 128 * 1e3:.3f} ms/image over the 16 CPUs ({128 / max(secs):.0f} images/s)", flush=True)
    e = Engine(0, arena_bytes=8 << 30)
    n, hw = 256, 1024
    plan = thumbnail_plan(hw, hw, 640)
    print(f"plan of {hw}x{hw} at 640: size {plan.size}, factors {plan.factors}, resize box {plan.resize_box}", flush=True)
    base = [photo_like(s, hw) for s in range(8)]
    for label, imgs in (("photo-like", np.stack([base[i % 8] for i in range(n)])), ("noise", np.random.default_rng(1).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8))):
        d = e.dev_alloc(imgs.nbytes)
        e.h2d(d, imgs)
        out = thumbnails(e, (d, n, hw, hw))
        total = sum(len(b) for b in out)
        med, lo, hi = stats_ms(lambda: thumbnails(e, (d, n, hw, hw)))
        print(f"fe_thumbnail_jpeg {label:10s}: median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f}) for {n} x {hw}x{hw} -> 640x640 q80, D2H of {total / 1e6:.1f} MB of JPEG "
              f"included = {med * 1e3 / n:7.1f} us/image, {n / med * 1e3:7.0f} images/s; source bytes at {imgs.nbytes / med * 1e3 / 1e9:6.1f} GB/s = "
              f"{imgs.nbytes / med * 1e3 / HBM_PEAK * 100:4.1f} % of {HBM_PEAK / 1e12:.0f} TB/s", flush=True)
        e.dev_free(d)
        # the encoder alone: the same thumbnails' pixels, resident
        from PIL import Image
        px = np.stack([np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in out[:8]])
        px = np.ascontiguousarray(np.stack([px[i % 8] for i in range(n)])) if label == "photo-like" else np.random.default_rng(2).integers(0, 256, (n, 640, 640, 3), dtype=np.uint8)
        d2 = e.dev_alloc(px.nbytes)
        e.h2d(d2, px)
        enc = e.jpeg_encode((d2, n, 640, 640))
        med2, lo2, hi2 = stats_ms(lambda: e.jpeg_encode((d2, n, 640, 640)))
        print(f"fe_jpeg_encode    {label:10s}: median {med2:8.2f} ms (min {lo2:.2f}, max {hi2:.2f}) for {n} x 640x640, {sum(len(b) for b in enc) / 1e6:.1f} MB of JPEG copied back "
              f"= {med2 * 1e3 / n:7.1f} us/image" + (f"; reduce + resize = the rest of the call above, about {med - med2:.2f} ms" if label == "photo-like" else
                                                  " (fresh 640x640 noise, which codes longer than resized noise: not the same bytes as above)"), flush=True)
        e.dev_free(d2)
    e.close()

if "step" in parts:
    from facet_amd._lib import FE_MODEL_TOPIQ, FE_MODEL_CLIP, FE_MODEL_AESTHETIC, FE_MODEL_SAMP, FE_MODEL_U2NETP
    from facet_amd.batch import BatchScorer
    from facet_amd.weights import synthetic_state_dict, synthetic_images
    e, e2 = Engine(0, arena_bytes=72 << 30), Engine(0, arena_bytes=8 << 30)
    for mid, name in ((FE_MODEL_TOPIQ, "topiq"), (FE_MODEL_CLIP, "clip"), (FE_MODEL_AESTHETIC, "aesthetic"), (FE_MODEL_U2NETP, "u2netp"), (FE_MODEL_SAMP, "samp_net")):
        e.load_weights(mid, synthetic_state_dict(name, 4))
    e.set_microbatch(32)
    n, hw = 64, 1024
    imgs = synthetic_images(6, n, hw, hw)
    scorers = {False: BatchScorer(e, aux_engine=e2), True: BatchScorer(e, aux_engine=e2, thumbnails=True)}
    for s in scorers.values():
        s.process_batch(imgs[:8])
    times = {False: [], True: []}
    for _ in range(5):
        for flag, s in scorers.items():
            t0 = time.perf_counter()
            s.process_batch(imgs)
            times[flag].append((time.perf_counter() - t0) * 1e3)
    off, on = float(np.median(times[False])), float(np.median(times[True]))
    print(f"BatchScorer step (aux context), {n} x {hw}x{hw}: thumbnails off {off:.1f} ms ({n / off * 1e3:.1f} images/s), on {on:.1f} ms "
          f"({n / on * 1e3:.1f} images/s), difference {on - off:+.1f} ms; runs off {[round(t) for t in times[False]]} on {[round(t) for t in times[True]]}", flush=True)
    e2.close()
    e.close()
