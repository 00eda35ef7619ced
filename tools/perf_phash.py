"""fe_phash / fe_hamming_pairs rates (profiles/phash_perf.txt).
usage: perf_phash.py [phash] [hamming] [step]      (no argument: all three parts)
  phash:   fe_phash on a resident 256 x 1024x1024 batch, median of 20 calls, against fe_image_stats on the same batch in the same run
           and the PIL + scipy restatement of imagehash.phash on the CPU, one process alone and 16 side by side
  hamming: fe_hamming_pairs on random hashes, distance 6, n = 100k and 1M (n is cut so that the step stays under a minute), against the
           reference's numpy loop (utils/duplicate.py:94-119, restated) at n = 20k
  step:    BatchScorer.process_batch (five models + statistics on a second context), 64 x 1024x1024, phash off / on"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facet_amd import Engine          # noqa: E402

HBM_PEAK = 8.0e12                     # MI355X, bytes/s
parts = set(sys.argv[1:]) or {"phash", "hamming", "step"}


def median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def cpu_restatement(seed, count=8):
    """One worker of the CPU leg: `count` images through the PIL + scipy restatement of imagehash.phash; returns its seconds."""
    import scipy.fftpack
    from PIL import Image
    imgs = np.random.default_rng(seed).integers(0, 256, (count, 1024, 1024, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    for im in imgs:
        small = np.asarray(Image.fromarray(im, "RGB").convert("L").resize((32, 32), Image.Resampling.LANCZOS))
        lo_ = scipy.fftpack.dct(scipy.fftpack.dct(small, axis=0), axis=1)[:8, :8]
        _ = lo_ > np.median(lo_)
    return time.perf_counter() - t0


if "phash" in parts:
    # the CPU leg first: its 16 worker processes are forked before this process opens the GPU
    try:
        import multiprocessing as mp
        import scipy.fftpack          # noqa: F401
        one = cpu_restatement(0) / 8
        with mp.get_context("fork").Pool(16) as pool:
            pool.map(cpu_restatement, range(16), chunksize=1)          # warm the workers
            secs = pool.map(cpu_restatement, range(100, 116), chunksize=1)     # 16 loops side by side, each timing itself
        print(f"PIL + scipy restatement: {one * 1e3:.2f} ms/image with one process alone; 16 processes side by side, 8 images each: "
              f"slowest loop {max(secs):.3f} s = {max(secs) / 128 * 1e3:.3f} ms/image over the 16 CPUs ({128 / max(secs):.0f} images/s)", flush=True)
    except ImportError as ex:
        print("PIL + scipy restatement not timed:", ex)
    e = Engine(0, arena_bytes=8 << 30)
    n, hw = 256, 1024
    imgs = np.random.default_rng(1).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    d = e.dev_alloc(imgs.nbytes)
    e.h2d(d, imgs)
    dev = (d, n, hw, hw)
    nbytes = imgs.nbytes
    for label, fn in (("fe_phash (RGB bytes)", lambda: e.phash(dev)), ("fe_phash (bgr=1)", lambda: e.phash(dev, bgr=True)),
                      ("fe_image_stats", lambda: e.image_stats(dev))):
        med, lo, hi = median_ms(fn)
        print(f"{label:22s}: median {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}) for {n} x {hw}x{hw} = {med * 1e3 / n:7.2f} us/image, "
              f"{nbytes / med * 1e3 / 1e9:7.1f} GB/s of source bytes = {nbytes / med * 1e3 / HBM_PEAK * 100:5.1f} % of {HBM_PEAK / 1e12:.0f} TB/s", flush=True)
    e.dev_free(d)
    e.close()

if "hamming" in parts:
    e = Engine(0, arena_bytes=2 << 30)
    rng = np.random.default_rng(2)
    rate = None
    for n in (100_000, 1_000_000):
        if rate is not None and n * (n - 1) / 2 / rate > 45.0:
            n = int((2 * 45.0 * rate) ** 0.5)
        h = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
        h[n // 2] = h[7]                                   # one certain hit
        e.hamming_pairs(h[:4096], 6)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            pairs = e.hamming_pairs(h, 6)
            ts.append(time.perf_counter() - t0)
        dt = float(np.median(ts))
        rate = n * (n - 1) / 2 / dt
        print(f"fe_hamming_pairs n = {n}: median of 5 {dt * 1e3:9.1f} ms (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f}), {len(pairs)} pairs found, {rate:.3e} pairs compared / s", flush=True)
    e.close()
    table = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)
    n = 20_000
    h = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
    t0 = time.perf_counter()
    found = 0
    for i in range(n - 1):                                 # the shape of utils/duplicate.py:94-119: one row against the rest, eight byte passes
        x = np.bitwise_xor(h[i], h[i + 1:])
        dist = np.zeros(len(x), dtype=np.int32)
        for b in range(8):
            dist += table[((x >> np.uint64(b * 8)) & np.uint64(0xFF)).astype(np.int32)]
        found += int(np.count_nonzero(dist <= 6))
    dt = time.perf_counter() - t0
    print(f"numpy loop of the reference n = {n}: {dt:7.2f} s, {found} pairs, {n * (n - 1) / 2 / dt:.3e} pairs compared / s", flush=True)

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
    scorers = {False: BatchScorer(e, aux_engine=e2), True: BatchScorer(e, aux_engine=e2, phash=True)}
    for s in scorers.values():
        s.process_batch(imgs[:8])
    times = {False: [], True: []}
    for _ in range(5):
        for flag, s in scorers.items():
            t0 = time.perf_counter()
            s.process_batch(imgs)
            times[flag].append((time.perf_counter() - t0) * 1e3)
    off, on = float(np.median(times[False])), float(np.median(times[True]))
    print(f"BatchScorer step (aux context), {n} x {hw}x{hw}: phash off {off:.1f} ms ({n / off * 1e3:.1f} images/s), on {on:.1f} ms "
          f"({n / on * 1e3:.1f} images/s), difference {on - off:+.1f} ms; runs off {[round(t) for t in times[False]]} on {[round(t) for t in times[True]]}", flush=True)
    e2.close()
    e.close()
