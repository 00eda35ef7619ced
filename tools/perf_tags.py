"""Tag selection rates (profiles/tags_perf.txt).
usage: perf_tags.py [--out FILE] [--n A,B] [--no-batch]      (default FILE: profiles/tags_perf.txt; every line is also printed; default
                                                             library sizes 100000,1000000)

  libraries: n stored embeddings (unit rows: the normalised sum of 1 - 4 prompt rows plus noise; sizes above the first repeat the
             first library's rows, which changes no timing), the shipped grouping of 61 tags / 239 prompts
             (tests/golden/tags_golden.json), threshold 0.22, max_tags 5
  engine:    Engine.tag_select on the host matrix (upload, GEMM on the cached text rows, selection, ids / scores / counts back), on the
             same matrix resident in device memory, and CLIPTagger.select_batch from the list of stored blobs (the first size only:
             the blobs are joined on the host first) to the lists of names
  baselines: the existing CLIPTagger.get_tags_batch (GEMM on the device, the [n, 239] matrix back, the selection in Python) on
             100 000 rows and the per-row CLIPTagger.get_tags_from_embedding loop, which is what the reference's library passes
             run (photos.py:613-623, tag_existing.py:51-58), on 10 000 rows
  batch:     one BatchScorer.process_batch step of 256 images of 384 x 384 (TOPIQ, CLIP + aesthetic, U2-Net-P + SAMP-Net, statistics,
             tags; no faces) with gpu_tag_select off and on, alternating in one session
Each figure is the median of 5 calls after a warm-up call, with the fastest and the slowest."""
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from facet_amd import Engine                   # noqa: E402
from facet_amd.tagger import CLIPTagger        # noqa: E402

out_path = os.path.join(ROOT, "profiles", "tags_perf.txt")
if "--out" in sys.argv:
    out_path = sys.argv[sys.argv.index("--out") + 1]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
out_file = open(out_path, "w")
SIZES = [int(v) for v in sys.argv[sys.argv.index("--n") + 1].split(",")] if "--n" in sys.argv else [100_000, 1_000_000]
THRESHOLD, MAX_TAGS, D = 0.22, 5, 768


def say(line):
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()


def timed(fn, reps=5):
    fn()                                       # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    m, lo, hi = t
    unit, k = ("ms", 1e3) if m < 1.0 else ("s", 1.0)
    return f"{m * k:.2f} {unit} (fastest {lo * k:.2f}, slowest {hi * k:.2f})"


def library(rng, text, n):
    emb = np.empty((n, D), np.float32)
    for i0 in range(0, n, 16384):
        m = min(16384, n - i0)
        pick = rng.integers(0, len(text), (m, 4))
        use = rng.integers(1, 5, m)[:, None] > np.arange(4)[None, :]
        rows = np.einsum("mk,mkd->md", use.astype(np.float32), text[pick])
        noise = rng.standard_normal((m, D)).astype(np.float32)
        rows += noise / np.linalg.norm(noise, axis=1, keepdims=True) * rng.uniform(2.5, 4.5, (m, 1)).astype(np.float32)
        emb[i0:i0 + m] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    return emb


g = json.load(open(os.path.join(ROOT, "tests", "golden", "tags_golden.json")))
vocab = {t: [f"{t} {k}" for k in range(s)] for t, s in zip(g["tags"], g["sizes"])}
tg = CLIPTagger(config=types.SimpleNamespace(get_tag_vocabulary=lambda: vocab, get_art_tags=lambda: set(g["art_tags"])))
names, _ = tg.prompts()
rng = np.random.default_rng(11)
tg.set_text_embeddings(names, rng.standard_normal((len(names), D)))
e = Engine(0, arena_bytes=8 << 30)
tg.use_engine(e)
say(f"tag selection: {len(vocab)} tags / {len(names)} prompts, d = {D}, threshold {THRESHOLD}, max_tags {MAX_TAGS}; median of 5 calls after a warm-up")

base = library(rng, tg.text_embeddings, SIZES[0])
for k, n in enumerate(SIZES):
    emb = base if k == 0 else np.ascontiguousarray(np.resize(base, (n, D)))
    t_host = timed(lambda: e.tag_select(emb, THRESHOLD, MAX_TAGS))
    ids, _, counts = e.tag_select(emb, THRESHOLD, MAX_TAGS)
    d_emb = e.dev_alloc(emb.nbytes)
    try:
        e.h2d(d_emb, emb)
        t_dev = timed(lambda: e.tag_select((d_emb, n, D), THRESHOLD, MAX_TAGS))
        same = all(np.array_equal(a, b) for a, b in zip(e.tag_select((d_emb, n, D), THRESHOLD, MAX_TAGS), e.tag_select(emb, THRESHOLD, MAX_TAGS)))
    finally:
        e.dev_free(d_emb)
    say(f"{n} embeddings: Engine.tag_select host matrix {fmt(t_host)} = {n / t_host[0]:.3g} rows/s | resident {fmt(t_dev)} = {n / t_dev[0]:.3g} rows/s"
        f" | {counts.mean():.2f} tags per row, resident == host: {same}")
    if k == 0:
        blobs = [row.tobytes() for row in emb]
        t_blobs = timed(lambda: tg.select_batch(blobs, THRESHOLD, MAX_TAGS))
        say(f"{n} blobs: CLIPTagger.select_batch (join, engine call, names) {fmt(t_blobs)} = {n / t_blobs[0]:.3g} rows/s")
        m = min(n, 100_000)
        t_old = timed(lambda: tg.get_tags_batch(emb[:m], e, THRESHOLD, MAX_TAGS))
        say(f"{m} rows: CLIPTagger.get_tags_batch (device GEMM, selection in Python) {fmt(t_old)} = {m / t_old[0]:.3g} rows/s")
        m = min(n, 10_000)
        t_row = timed(lambda: [tg.get_tags_from_embedding(b, THRESHOLD, MAX_TAGS) for b in blobs[:m]])
        say(f"{m} rows: per-row CLIPTagger.get_tags_from_embedding loop (host) {fmt(t_row)} = {m / t_row[0]:.3g} rows/s")
        agree = tg.select_batch(blobs[:m], THRESHOLD, MAX_TAGS) == [tg.get_tags_from_embedding(b, THRESHOLD, MAX_TAGS) for b in blobs[:m]]
        say(f"{m} rows: select_batch == the per-row loop: {agree} (float32 similarities of two summation orders; a row may differ only where a decision is within 1e-5)")
        del blobs
    del emb
del base
e.close()

if "--no-batch" not in sys.argv:
    from facet_amd._lib import FE_MODEL_TOPIQ, FE_MODEL_CLIP, FE_MODEL_AESTHETIC, FE_MODEL_SAMP, FE_MODEL_U2NETP
    from facet_amd.batch import BatchScorer
    from facet_amd.weights import synthetic_state_dict, synthetic_images
    e = Engine(0, arena_bytes=24 << 30)
    for mid, name in ((FE_MODEL_TOPIQ, "topiq"), (FE_MODEL_CLIP, "clip"), (FE_MODEL_AESTHETIC, "aesthetic"), (FE_MODEL_U2NETP, "u2netp"), (FE_MODEL_SAMP, "samp_net")):
        e.load_weights(mid, synthetic_state_dict(name, 4))
    imgs = synthetic_images(6, 256, 384, 384)
    off = BatchScorer(e, tagger=tg, tag_threshold=THRESHOLD, max_tags=MAX_TAGS)
    on = BatchScorer(e, tagger=tg, tag_threshold=THRESHOLD, max_tags=MAX_TAGS, gpu_tag_select=True)
    off.process_batch(imgs[:8]), on.process_batch(imgs[:8])
    off.process_batch(imgs), on.process_batch(imgs)
    t = {"off": [], "on": []}
    for _ in range(5):
        for label, bs in (("off", off), ("on", on)):
            t0 = time.perf_counter()
            bs.process_batch(imgs)
            t[label].append(time.perf_counter() - t0)
    for label in ("off", "on"):
        say(f"BatchScorer.process_batch, 256 x 384x384, gpu_tag_select {label}: {fmt((statistics.median(t[label]), min(t[label]), max(t[label])))}")
    e.close()
out_file.close()
