"""Times the similarity sweeps (fe_similar_topk / fe_similar_pairs) on one GPU and writes profiles/similar_perf.txt.

    python tools/perf_similar.py [--sizes 10000,100000] [--d 768] [--out profiles/similar_perf.txt]

Per library size n (rows resident on the device, metadata for every factor): nq = 1, 64 and n queries, k = 32. A sweep is
2 nq n d FLOP; one query is a read of n d 4 bytes. nq = n is put next to Engine.core_distances(x, 32) at the same n and d in the
same run (the same tile core with a top-k epilogue), nq = 1 next to the HBM rate, and everything next to a numpy restatement of
the reference's per-candidate loop on this host (thread count printed). Each figure: 2 warm-up calls, then the minimum and the
median of `--reps` timed calls (wall time of the call, host bookkeeping included)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TFLOPS, HBM_GBS = 157.3, 8000.0          # fp32 matrix peak and HBM3E rate of one MI355X (vendor figures; a plain copy reaches about 6300 GB/s)


def library(n, d, seed=0):
    from facet_amd._lib import FE_SIM_NO_DATE, SimRows
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((n, d)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    date = (1_600_000_000 + rng.integers(0, 900 * 86400, n)).astype(np.int64)
    date[rng.random(n) < 0.05] = FE_SIM_NO_DATE
    agg = rng.uniform(1, 10, n).astype(np.float32)
    counts = rng.choice([0, 0, 1, 2, 3], n)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    owner = np.repeat(np.arange(n), counts)
    nth = np.arange(off[-1]) - np.repeat(off[:-1], counts)
    ids = (rng.integers(0, 130, n)[owner] + 130 * nth).astype(np.int32)      # ascending and unique within a row
    return SimRows(emb, np.ones(n, np.uint8), date, agg, off, ids, normalise=False)


def timed(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts))


def reference_loop_ms(rows, nq_sample=1):
    """The reference's loop restated with numpy: per candidate one float32 dot, two norms, the three other factors in Python."""
    n = rows.n
    emb = rows.emb
    t0 = time.perf_counter()
    for q in range(nq_sample):
        out = []
        for c in range(n):
            if c == q:
                continue
            cos = float(np.dot(emb[q], emb[c]) / (np.linalg.norm(emb[q]) * np.linalg.norm(emb[c]) + 1e-10))
            total = 0.4 * (cos + 1) / 2
            a = set(rows.person_ids[rows.person_off[q]:rows.person_off[q + 1]].tolist())
            b = set(rows.person_ids[rows.person_off[c]:rows.person_off[c + 1]].tolist())
            if a and b:
                total += 0.3 * len(a & b) / max(len(a), len(b))
            days = abs((int(rows.date[q]) - int(rows.date[c])) // 86400)
            total += 0.2 * (1.0 if days == 0 else 0.5 if days <= 7 else 0.2 if days <= 30 else max(0, 1 - days / 365))
            total += 0.1 * max(0, 1 - abs(float(rows.aggregate[q]) - float(rows.aggregate[c])) / 10)
            out.append((round(total, 4), c))
        out.sort(key=lambda x: x[0], reverse=True)
    return (time.perf_counter() - t0) * 1e3 / nq_sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similar_perf.txt"))
    a = ap.parse_args()
    from facet_amd import Engine
    eng = Engine(0, arena_bytes=1 << 30)
    d = a.d
    lines = [f"Similarity sweeps on one MI355X (python tools/perf_similar.py --sizes {a.sizes} --d {d}), k = 32, default weights, every factor's",
             f"metadata present, library resident on the device. min / median of {a.reps} calls after 2 warm-ups; wall time of the call.",
             f"Vendor figures used for the ratios: fp32 matrix peak {PEAK_TFLOPS:.0f} TFLOP/s, HBM {HBM_GBS:.0f} GB/s.", ""]
    for n in [int(s) for s in a.sizes.split(",")]:
        rows = library(n, d)
        dev = eng.upload_sim_rows(rows)
        lines.append(f"n = {n}")
        for nq in (1, 64, n):
            q = dev if nq == n else type(rows)(rows.emb[:nq], rows.has_emb[:nq], rows.date[:nq], rows.aggregate[:nq], rows.person_off[:nq + 1],
                                               rows.person_ids[:rows.person_off[nq]], normalise=False)
            qs = np.arange(nq, dtype=np.int32)
            lo, med = timed(lambda: eng.similar_topk(q, dev, 32, q_self=qs), a.reps)
            flop, byts = 2.0 * nq * n * d, 4.0 * n * d
            lines.append(f"  topk  nq = {nq:6d}: {lo:9.3f} / {med:9.3f} ms   {flop / lo / 1e9:8.2f} TFLOP/s ({flop / lo / 1e9 / PEAK_TFLOPS:.2f} of peak)"
                         f"   {byts / lo / 1e6:8.1f} GB/s of C ({byts / lo / 1e6 / HBM_GBS:.2f} of HBM)")
        thr = np.full(1, 0.62, np.float32)
        lo, med = timed(lambda: eng.similar_pairs(dev, dev, thr, cosine=True, upper=True), a.reps)
        lines.append(f"  pairs nq = {n:6d} (cosine, upper, thr 0.62): {lo:9.3f} / {med:9.3f} ms   {1.0 * n * n * d / lo / 1e9:8.2f} TFLOP/s on the half that is formed")
        import torch
        x = torch.from_numpy(rows.emb).cuda()
        lo, med = timed(lambda: eng.core_distances((x.data_ptr(), n, d), 32, normalise=False), a.reps)
        lines.append(f"  core_distances(x, 32), the same tile core:  {lo:9.3f} / {med:9.3f} ms   {2.0 * n * n * d / lo / 1e9:8.2f} TFLOP/s")
        sample = min(n, 20000)
        sub = type(rows)(rows.emb[:sample], rows.has_emb[:sample], rows.date[:sample], rows.aggregate[:sample], rows.person_off[:sample + 1],
                         rows.person_ids[:rows.person_off[sample]], normalise=False)
        ms = reference_loop_ms(sub) * n / sample
        lines.append(f"  numpy restatement of the reference loop, one query: {ms:9.1f} ms (measured on {sample} candidates, scaled to n; "
                     f"{os.environ.get('OMP_NUM_THREADS', '?')} threads allowed, the loop itself is single-threaded Python)")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
