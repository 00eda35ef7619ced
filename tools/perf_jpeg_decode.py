"""fe_jpeg_decode rates (profiles/jpeg_decode_perf.txt).
usage: perf_jpeg_decode.py
  256 x 1024x1024 photo-like files at quality 85, 4:2:0 and 4:2:2, without restart markers and with one per MCU row, and the same
  sources saved with progressive=True (decoded with FE_JPEG_PROGRESSIVE: one entropy pass per scan); every baseline configuration a
  second time with parallel_entropy=True (FE_JPEG_FLAG_PARALLEL: a lane per 128-byte subsequence); the files are in host memory, the
  pixels stay on the device. Per configuration: median of 7 calls (min, max), images/s, and from one profiled call the
  time of each stage (host parse, the upload, entropy, IDCT, colour). Before the GPU is opened: Pillow's decode of the same files on this
  host, one process alone and 16 side by side; afterwards the upload of the decoded pixels, which the CPU route also pays."""
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facet_amd import Engine          # noqa: E402

N, HW, QUALITY = 256, 1024, 85
CONFIGS = [("4:2:0", 2, False, False), ("4:2:0 rst/row", 2, True, False), ("4:2:2", 1, False, False), ("4:2:2 rst/row", 1, True, False),
           ("prog 4:2:0", 2, False, True), ("prog 4:2:0 rst/row", 2, True, True), ("prog 4:2:2", 1, False, True), ("prog 4:2:2 rst/row", 1, True, True)]


def photo_like(seed, hw):
    """Smooth colour waves plus sensor-like noise: compresses like a photograph."""
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


def make_files(subsampling, restart, progressive):
    """8 distinct files, repeated to N (each is decoded on its own; only the encode time is saved)."""
    from PIL import Image
    out = []
    for s in range(8):
        buf = io.BytesIO()
        kw = {"restart_marker_rows": 1} if restart else {}
        if progressive:
            kw["progressive"] = True
        Image.fromarray(photo_like(s, HW)).save(buf, "JPEG", quality=QUALITY, subsampling=subsampling, **kw)
        out.append(buf.getvalue())
    return [out[i % 8] for i in range(N)]


def pillow_decode(blobs):
    from PIL import Image, ImageOps
    t0 = time.perf_counter()
    for b in blobs:
        np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(b))).convert("RGB"))
    return time.perf_counter() - t0


def stats_ms(fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


if __name__ == "__main__":
    import multiprocessing as mp
    files = {label: make_files(s, r, p) for label, s, r, p in CONFIGS}
    # the CPU leg first: its 16 worker processes are forked before this process opens the GPU
    with mp.get_context("fork").Pool(16) as pool:
        for label, blobs in files.items():
            one = pillow_decode(blobs[:16]) / 16
            pool.map(pillow_decode, [blobs[:4]] * 16, chunksize=1)
            secs = pool.map(pillow_decode, [blobs[16 * k:16 * k + 16] for k in range(16)], chunksize=1)      # 16 loops side by side
            print(f"Pillow {label:18s}: {np.mean([len(b) for b in blobs]) / 1e3:6.1f} KB/file; one process alone {one * 1e3:6.2f} ms/image "
                  f"({1 / one:5.0f} images/s); 16 processes side by side, 16 images each: slowest loop {max(secs):.3f} s = "
                  f"{N / max(secs):6.0f} images/s", flush=True)
    e = Engine(0, arena_bytes=8 << 30)
    d = e.dev_alloc(N * HW * HW * 3)
    rounds = 0
    for label, blobs in files.items():
        # a baseline configuration a second time with FE_JPEG_FLAG_PARALLEL; the scans of a progressive file stay a lane per segment
        for par in ((False,) if label.startswith("prog") else (False, True)):
            kw = {"progressive": True} if label.startswith("prog") else ({"parallel_entropy": True} if par else {})
            name = label + (" parallel" if par else "")
            _, status = e.jpeg_decode(blobs, HW, HW, device=d, **kw)
            assert not status.any(), status
            med, lo, hi = stats_ms(lambda: e.jpeg_decode(blobs, HW, HW, device=d, **kw))
            print(f"fe_jpeg_decode {name:22s}: median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f}) for {N} x {HW}x{HW} q{QUALITY}, files in host memory, "
                  f"pixels left on the device = {med * 1e3 / N:7.1f} us/image, {N / med * 1e3:7.0f} images/s", flush=True)
            e.profile_enable(True)
            e.jpeg_decode(blobs, HW, HW, device=d, **kw)
            recs = e.profile_records()
            e.profile_enable(False)
            print("    stages of one call: " + "; ".join(f"{r['name'].split(': ')[1]} {r['ms']:.2f} ms" for r in recs), flush=True)
            if par:
                st = e.jpeg_entropy_stats()
                rounds = max(rounds, st["max_rounds"])
                print(f"    parallel entropy: {st['parallel_segments']} segments, {st['subsequences']} subsequences, most rounds of a segment "
                      f"{st['max_rounds']}, images decoded again {st['redone']}", flush=True)
    print(f"parallel entropy: most rounds of any segment over all configurations {rounds}", flush=True)
    px = np.random.default_rng(0).integers(0, 256, (N, HW, HW, 3), dtype=np.uint8)
    med, lo, hi = stats_ms(lambda: e.h2d(d, px))
    print(f"upload of {N} decoded images ({px.nbytes / 1e6:.0f} MB, pageable host memory): median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}) = "
          f"{px.nbytes / med / 1e6:.1f} GB/s, {N / med * 1e3:.0f} images/s", flush=True)
    e.dev_free(d)
    e.close()
