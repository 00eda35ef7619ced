"""fe_jpeg_thumbnail rates (profiles/thumbnail_transcode_perf.txt): stored thumbnails made smaller, JPEG bytes in, JPEG bytes out.
usage: perf_thumbnail_transcode.py [out.txt]
  512 thumbnails as Pillow writes them (256 of 640x427 and 256 of 427x640, photo-like, quality 80) to the sizes 320, 160 (draft() keeps
  scale 1) and 100 (scale 2). Per size: resize_thumbnails over all 512 (two fe_jpeg_thumbnail calls, grouping and the Python bytes
  objects included), median of 7 (min, max), and from one profiled call per source shape the time of each stage (host parse, upload,
  entropy, IDCT, colour, then reduce / resize / encode as one remainder), first with the lane-per-segment entropy stage and then with
  parallel_entropy=True (FE_JPEG_FLAG_PARALLEL), whose rows carry that name. Before the GPU is opened: the reference's Pillow recipe on this
  host, one process alone and 16 side by side. The table goes to stdout and, when a path is given, into that file as well."""
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facet_amd import Engine                                                                                  # noqa: E402
from facet_amd.thumbnail import draft_scale, pillow_resize_thumbnail, resize_thumbnails, thumbnail_plan_jpeg    # noqa: E402

N, QUALITY, TARGETS = 512, 80, (320, 160, 100)
SHAPES = ((640, 427), (427, 640))      # (w, h)


def photo_like(seed, w, h):
    """Smooth colour waves plus sensor-like noise: compresses like a photograph."""
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, 1.0, h)[:, None]
    x = np.linspace(0.0, 1.0, w)[None, :]
    img = np.empty((h, w, 3), np.float64)
    for c in range(3):
        acc = np.full((h, w), 128.0 + rng.uniform(-30.0, 30.0))
        for _ in range(4):
            fy, fx = rng.uniform(0.3, 3.5, 2)
            acc = acc + rng.uniform(15.0, 45.0) * np.sin(2.0 * np.pi * (fy * y + fx * x) + rng.uniform(0.0, 2.0 * np.pi))
        img[..., c] = acc + rng.normal(0.0, 6.0, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def make_files():
    """16 distinct files per shape, repeated to N / 2 each and interleaved, as rows of a `photos` table would come."""
    from PIL import Image
    per = {}
    for (w, h) in SHAPES:
        per[(w, h)] = []
        for s in range(16):
            buf = io.BytesIO()
            Image.fromarray(photo_like(s, w, h)).save(buf, format="JPEG", quality=QUALITY)
            per[(w, h)].append(buf.getvalue())
    return [per[SHAPES[i % 2]][(i // 2) % 16] for i in range(N)]


def pillow_loop(job):
    blobs, size = job
    t0 = time.perf_counter()
    for b in blobs:
        pillow_resize_thumbnail(b, size)
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
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    files = make_files()
    say(f"{N} stored thumbnails, {N // 2} of 640x427 and {N // 2} of 427x640, quality {QUALITY}, {np.mean([len(b) for b in files]) / 1e3:.1f} KB/file")
    # the CPU leg first: its 16 worker processes are forked before this process opens the GPU
    with mp.get_context("fork").Pool(16) as pool:
        for size in TARGETS:
            one = pillow_loop((files[:32], size)) / 32
            pool.map(pillow_loop, [(files[:4], size)] * 16, chunksize=1)
            secs = pool.map(pillow_loop, [(files[32 * k:32 * k + 32], size) for k in range(16)], chunksize=1)      # 16 loops side by side
            say(f"Pillow -> {size:3d} (draft scale {draft_scale(640, 427, size)}): one process alone {one * 1e3:6.2f} ms/file ({1 / one:5.0f} files/s); "
                f"16 processes side by side, 32 files each: slowest loop {max(secs):.3f} s = {N / max(secs):6.0f} files/s")
    e = Engine(0, arena_bytes=4 << 30)
    for par in (False, True):            # the lane-per-segment entropy stage, then FE_JPEG_FLAG_PARALLEL: one lane per 128-byte subsequence
        kw, tag = (dict(parallel_entropy=True), " parallel_entropy") if par else ({}, "")
        rounds = redone = 0
        for size in TARGETS:
            got = resize_thumbnails(e, files, size, **kw)
            assert got[:4] == [pillow_resize_thumbnail(b, size) for b in files[:4]], "not Pillow's bytes"
            med, lo, hi = stats_ms(lambda: resize_thumbnails(e, files, size, **kw))
            say(f"resize_thumbnails{tag} -> {size:3d} (draft scale {draft_scale(640, 427, size)}): median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f}) for {N} files, "
                f"{sum(len(b) for b in got) / 1e6:.2f} MB of JPEG back = {med * 1e3 / N:7.1f} us/file, {N / med * 1e3:7.0f} files/s")
            for (w, h) in SHAPES:
                group = [b for i, b in enumerate(files) if SHAPES[i % 2] == (w, h)]
                scale, plan = thumbnail_plan_jpeg(w, h, size)
                t0 = time.perf_counter()
                e.jpeg_thumbnail(group, scale, plan, **kw)
                plain = (time.perf_counter() - t0) * 1e3
                e.profile_enable(True)
                e.jpeg_thumbnail(group, scale, plan, **kw)
                recs = e.profile_records()
                e.profile_enable(False)
                st = e.jpeg_entropy_stats()
                rounds, redone = max(rounds, st['max_rounds']), redone + st['redone']
                dec = [r for r in recs if r["name"].startswith("jpeg_decode")]
                say(f"    fe_jpeg_thumbnail{tag} {w}x{h} -> {plan.size[0]}x{plan.size[1]}, {len(group)} files, one call {plain:.2f} ms; decode stages: "
                    + "; ".join(f"{r['name'].split(': ')[1]} {r['ms']:.2f} ms" for r in dec)
                    + f"; reduce + resize + encode + copies back: the remaining {plain - sum(r['ms'] for r in dec):.2f} ms")
        if par:
            say(f"parallel_entropy: {st['parallel_segments']} segments / {st['subsequences']} subsequences in the last call, "
                f"most rounds of any segment in the profiled calls {rounds}, images decoded again by the serial kernel {redone}")
    e.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("python tools/perf_thumbnail_transcode.py        (MI355X, one GPU; wall-clock per call on the host, 2 warm-up calls, median of 7 with min / max)\n\n")
            f.write("\n".join(lines) + "\n")
