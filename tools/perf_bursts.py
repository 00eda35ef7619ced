"""fe_burst_links rates (profiles/bursts_perf.txt).
usage: perf_bursts.py [--out FILE] [--n A,B]      (default FILE: profiles/bursts_perf.txt; every line is also printed; default sizes
                                                 100000,1000000 - the first is also the size of the one-timestamp libraries)

  libraries: synthetic, time-sorted: sessions of 1 - 40 photos 0 - 2 s apart (hashes a few bits around the session's centre, 0 - 2
             persons per photo), sessions 30 s - 2 h apart; 100k and 1M photos, under the shipped settings (70 % / 0.8 min / 0.4 s ->
             19 / 48 s / 0 s) and under the fallbacks (88 % / 60 min / 5 s -> 7 / 3600 s / 5 s)
  worst band: 100k photos with one identical timestamp and unrelated hashes, at 95 % / 60 min / 5 s (3 / 3600 s / 5 s): every row has
             every earlier row in reach and none is alike (random hashes are about 32 bits apart, 2 thr = 6), so all n (n - 1) / 2 pairs
             are tested; under the fallbacks (2 thr = 14) a few rows in a thousand find a partner by chance and stop early; under the
             shipped settings the library is one burst: rapid_s = 0 joins photos of one second up to 38 bits apart
  long burst: the same timestamps, every hash 7 bits from the one before: the reference's walk is quadratic on it
  baseline:  the host restatement below - the reference's walk (each photo against the members of the open burst, oldest first) over
             integers, the dates parsed ONCE, which is kinder than the reference's two strptime calls per comparison - at sizes where it
             ends within a minute
Each engine figure is the median of 5 calls of Engine.burst_links (upload of the arrays, the kernel, the links back) after a warm-up
call; group_bursts (the O(n) host part) is timed beside it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from facet_amd import Engine                                  # noqa: E402
from facet_amd.bursts import burst_settings, group_bursts     # noqa: E402

SHIPPED = {"similarity_threshold_percent": 70, "time_window_minutes": 0.8, "rapid_burst_seconds": 0.4}

out_path = os.path.join(ROOT, "profiles", "bursts_perf.txt")
if "--out" in sys.argv:
    out_path = sys.argv[sys.argv.index("--out") + 1]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
out_file = open(out_path, "w")
SIZES = [int(v) for v in sys.argv[sys.argv.index("--n") + 1].split(",")] if "--n" in sys.argv else [100_000, 1_000_000]


def say(line):
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()


def library(seed, n):
    rng = np.random.default_rng(seed)
    length = rng.integers(1, 41, n)                            # more sessions than needed
    first = np.cumsum(length) - length
    first = first[first < n]
    new_session = np.zeros(n, bool)
    new_session[first] = True
    gap = np.where(new_session, rng.integers(30, 7200, n), rng.integers(0, 3, n))
    times = 1_600_000_000 + np.cumsum(gap).astype(np.int64)
    session = np.cumsum(new_session) - 1
    centre = rng.integers(0, 2 ** 63, int(session[-1]) + 1, dtype=np.uint64)
    hashes = centre[session]
    for _ in range(4):                                         # up to four flipped bits per photo
        hashes = hashes ^ np.where(rng.random(n) < 0.6, np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64), np.uint64(0))
    count = rng.integers(0, 3, n)
    off = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    a, b = rng.integers(0, 6, n), rng.integers(6, 12, n)      # ascending and distinct within a row
    ids = np.stack([a, b], axis=1)[np.arange(2)[None, :] < count[:, None]].astype(np.int32)
    return hashes, times, np.full(n, 3, np.uint8), off, ids


def host_walk(hashes, times, off, ids, aggregates, thr, window_s, rapid_s):
    """The reference's loop with the dates parsed once -> is_burst_lead."""
    h, t = hashes.tolist(), times.tolist()
    persons = [frozenset(ids[off[i]:off[i + 1]].tolist()) for i in range(len(h))]
    lead = [0] * len(h)
    start = 0

    def close(a, b):
        best = a
        for k in range(a + 1, b):
            if aggregates[k] > aggregates[best]:
                best = k
        lead[best] = 1

    for i in range(1, len(h)):
        joined = False
        for j in range(start, i):
            d = abs(t[i] - t[j])
            if d <= rapid_s and (not persons[i] or not persons[j] or persons[i] & persons[j]) and bin(h[i] ^ h[j]).count("1") <= 2 * thr:
                joined = True
                break
            if d <= window_s and bin(h[i] ^ h[j]).count("1") <= thr:
                joined = True
                break
        if not joined:
            close(start, i)
            start = i
    close(start, len(h))
    return lead


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, float(np.median(ts)), min(ts), max(ts)


def band_pairs(times, reach):
    """Rows in reach on the old side, summed: the most pair tests the kernel can make (it stops at the first chunk with a match)."""
    lo = np.searchsorted(times, times - reach, side="left")
    return int((np.arange(len(times)) - lo).sum())


e = Engine(0, arena_bytes=1 << 30)
say("fe_burst_links on an MI355X: Engine.burst_links = upload of times / flags / bounds / person lists, one wave per photo, links back")
for n in SIZES:
    hashes, times, flags, off, ids = library(n, n)
    aggregates = np.random.default_rng(n + 1).uniform(0, 10, n).round(2).tolist()
    d = e.dev_alloc(hashes.nbytes)
    e.h2d(d, hashes)
    for label, cfg in (("shipped 19 / 48 s / 0 s", SHIPPED), ("fallback 7 / 3600 s / 5 s", None)):
        thr, window_s, rapid_s = burst_settings(cfg)
        links, med, lo_, hi_ = timed(lambda: e.burst_links(hashes, times, flags, thr, window_s, rapid_s, off, ids))
        links_dev, med_dev, _, _ = timed(lambda: e.burst_links((d, n), times, flags, thr, window_s, rapid_s, off, ids))
        assert np.array_equal(links, links_dev)
        t0 = time.perf_counter()
        burst_id, lead = group_bursts(links, aggregates)
        t_group = time.perf_counter() - t0
        say(f"n = {n:8d}, {label:26s}: median of 5 {med * 1e3:9.2f} ms (min {lo_ * 1e3:.2f}, max {hi_ * 1e3:.2f}), resident hashes {med_dev * 1e3:9.2f} ms, "
            f"{n / med:.3e} photos/s; {band_pairs(times, max(window_s, rapid_s))} pairs in reach, {burst_id[-1]} bursts, {int((links >= 0).sum())} rows linked; "
            f"group_bursts on the host {t_group * 1e3:8.1f} ms")
        if n == SIZES[0]:
            t0 = time.perf_counter()
            want = host_walk(hashes, times, off, ids, aggregates, thr, window_s, rapid_s)
            dt = time.perf_counter() - t0
            say(f"             host restatement (dates parsed once), same library and settings: {dt:8.2f} s = {n / dt:.3e} photos/s; is_burst_lead "
                f"{'equal' if want == lead else 'DIFFERENT'}")
    e.dev_free(d)

n = SIZES[0]
rng = np.random.default_rng(5)
hashes = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
times, flags = np.full(n, 1_600_000_000, np.int64), np.full(n, 3, np.uint8)
off, ids = np.zeros(n + 1, np.int32), np.zeros(0, np.int32)
for label, cfg in (("95 % / 60 min / 5 s", {"similarity_threshold_percent": 95}), ("fallback", None)):
    thr, window_s, rapid_s = burst_settings(cfg)
    links, med, lo_, hi_ = timed(lambda: e.burst_links(hashes, times, flags, thr, window_s, rapid_s))
    linked = int((links >= 0).sum())
    say(f"worst band n = {n}, one timestamp, {label:18s}: median of 5 {med * 1e3:9.2f} ms (min {lo_ * 1e3:.2f}, max {hi_ * 1e3:.2f}), {linked} rows linked"
        + (f", {n * (n - 1) / 2 / med:.3e} pairs tested / s" if linked == 0 else " (so not every pair was tested)"))
# one long burst (a timelapse): one timestamp, every hash 7 bits from the one before, so a row is alike to the last few rows only. The
# engine finds the neighbour in its first chunk; the reference's walk starts at the OLDEST member of the open burst and is quadratic.
thr, window_s, rapid_s = burst_settings(None)
drift = np.zeros(n, np.uint64)
drift[0] = hashes[0]
for i in range(1, n):
    v = int(drift[i - 1])
    for b in rng.choice(64, size=7, replace=False):
        v ^= 1 << int(b)
    drift[i] = v
links, med, lo_, hi_ = timed(lambda: e.burst_links(drift, times, flags, thr, window_s, rapid_s))
burst_id, lead = group_bursts(links, [1.0] * n)
say(f"one long burst n = {n}, one timestamp, fallback: median of 5 {med * 1e3:9.2f} ms (min {lo_ * 1e3:.2f}, max {hi_ * 1e3:.2f}), {burst_id[-1]} bursts")
e.close()
for m in (min(n, 2000), min(n, 4000)):
    t0 = time.perf_counter()
    want = host_walk(drift[:m], times[:m], off[:m + 1], ids, [1.0] * m, thr, window_s, rapid_s)
    dt = time.perf_counter() - t0
    say(f"             host restatement on its first {m} photos: {dt:8.2f} s, {sum(want)} bursts, is_burst_lead {'equal' if want == lead[:m] else 'DIFFERENT'}")
out_file.close()
