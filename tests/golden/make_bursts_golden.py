"""Generates tests/golden/bursts_golden.json by RUNNING THE REFERENCE'S OWN `process_bursts` (processing/scorer.py:1880-1986) on
scratch SQLite files (tables `photos` and `faces`) with a configuration copy per case. The libraries are made up HERE (seeded);
nothing of the reference is stored, only our inputs and the `is_burst_lead` column its code wrote.

    python tests/golden/make_bursts_golden.py /path/to/reference

Per case the file holds the whole table in insertion order - [date_taken, aggregate, phash, persons, is_burst_lead] per photo - the
`burst_detection` block of its configuration (null: the block is absent and the reference's fallbacks apply) and `order`: the photos
with a hash in the order the reference's own SELECT returned them.

Every scenario below states which leads it expects and why; the generator asserts them on the reference's output, so each item of the
edge list is known to decide at least one lead. Scenarios of one case are days apart and share no bursts.
"""
import contextlib
import io
import json
import os
import sqlite3
import sys
import tempfile
from datetime import datetime, timedelta

import numpy as np

sys.dont_write_bytecode = True

FMT = "%Y:%m:%d %H:%M:%S"
A6, B6, C6 = 0x3F, 0x3F00, 0x3F0000            # three disjoint sets of six bits: one is "alike" at 90 % (distance 6), two are not (12)
UP6 = 0x3F << 40                               # six bits of the upper word


def hx(v):
    return format(int(v) & (2 ** 64 - 1), "016x")


def rand64(rng):
    return int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))


def flip(rng, v, bits):
    for b in rng.choice(64, size=bits, replace=False):
        v ^= 1 << int(b)
    return v


class Lib:
    """Photos in insertion order, scenarios days apart, and what the reference must answer."""

    def __init__(self, start=datetime(2021, 3, 4, 10, 0, 0)):
        self.rows, self.expect, self.base = [], [], start

    def at(self, seconds):
        return (self.base + timedelta(seconds=seconds)).strftime(FMT)

    def add(self, date, phash, aggregate, persons=(), lead=None, why=""):
        self.rows.append([date, aggregate, phash, sorted(persons)])
        if lead is not None:
            self.expect.append((len(self.rows) - 1, lead, why))
        return len(self.rows) - 1

    def next_scenario(self):
        self.base += timedelta(days=3)


# settings of the edge libraries: 90 % -> distance 6
BANDS = {"similarity_threshold_percent": 90, "time_window_minutes": 10, "rapid_burst_seconds": 0}
RAPID = {"similarity_threshold_percent": 90, "time_window_minutes": 1, "rapid_burst_seconds": 5}


def lib_bands(rng):
    """BANDS settings, every photo in its own second, so only the slow rule acts. O (hash P, score 9), then fillers one second apart
    (P ^ A6: alike to O and to each other, 12 bits from X), then X (P ^ B6: alike to O only, score 0.5).
      join: X is 600 s after O - O is the very last row of X's band of k predecessors and the only match: X joins, no lead.
      miss: X is 601 s after O - O sits at lo(X) - 1 behind a band of k fillers and must not count: X leads a burst of its own."""
    L = Lib()
    for k in (1, 63, 64, 65, 129):
        p = rand64(rng)
        L.add(L.at(0), hx(p), 9.0, lead=1, why=f"band {k} join: O leads")
        for f in range(k - 1):
            L.add(L.at(1 + f), hx(p ^ A6), 1.0, lead=0)
        L.add(L.at(600), hx(p ^ B6), 0.5, lead=0, why=f"band {k}: the match is the last row of the band")
        L.next_scenario()
    for k in (0, 1, 63, 64, 65, 129):
        p = rand64(rng)
        L.add(L.at(0), hx(p), 9.0, lead=1)
        for f in range(k):
            L.add(L.at(1 + f), hx(p ^ A6), 1.0, lead=0)
        L.add(L.at(601), hx(p ^ B6), 0.5, lead=1, why=f"band {k}: the row at lo - 1 does not count")
        L.next_scenario()
    # the largest match decides: A (P), B (P ^ A6 ^ B6: 12 bits from A, opens the burst), fillers alike to B only, X (P ^ A6) alike to A
    # (before the open burst) and to B (its start)
    for fillers in (0, 70):
        p = rand64(rng)
        L.add(L.at(0), hx(p), 5.0, lead=1, why="A alone")
        L.add(L.at(1), hx(p ^ A6 ^ B6), 7.0, lead=1, why="B leads the burst X joins")
        for f in range(fillers):
            L.add(L.at(2 + f), hx(p ^ A6 ^ B6 ^ C6), 1.0, lead=0)
        L.add(L.at(100), hx(p ^ A6), 0.5, lead=0, why="X matches below and at the start of the open burst: the largest match counts")
        L.next_scenario()
    # hashes that differ in the upper word only
    p = rand64(rng)
    L.add(L.at(0), hx(p), 9.0, lead=1)
    L.add(L.at(1), hx(p ^ UP6), 1.0, lead=0, why="six upper bits: alike")
    L.add(L.at(2), hx(p ^ UP6 ^ (0x7F << 50)), 1.0, lead=1, why="seven more upper bits, equal lower word: not alike")
    L.add(L.at(3), hx(p ^ UP6 ^ (0x7F << 50) ^ (0xFFFFFFFF << 32)), 0.5, lead=1, why="the whole upper word differs")
    L.next_scenario()
    # rows without a hash ('' : distance 999) and without a date break a burst; a NULL hash takes no part at all
    p = rand64(rng)
    L.add(L.at(0), hx(p), 9.0, lead=1)
    L.add(L.at(1), None, 8.0, lead=1, why="NULL hash: standalone, and invisible between its neighbours")
    L.add(L.at(2), hx(p), 1.0, lead=0, why="joins across the NULL-hash photo")
    L.add(L.at(3), "", 1.0, lead=1, why="empty hash string: alike to nothing")
    L.add(L.at(4), hx(p), 1.0, lead=1, why="the empty hash closed the burst; the match lies before its start")
    L.next_scenario()
    return L


def lib_dates(rng):
    """BANDS settings but a window of 40 s (rows below override it): unparsable and out-of-order dates inside a band."""
    L = Lib()
    p = rand64(rng)
    day = L.base.strftime("%Y:%m:%d")
    # strings in byte order; the parsed time of the last two is EARLIER than all before them ('9:59:50' sorts after '10:..')
    L.add(f"{day} 10:00:00", hx(p), 9.0, lead=1, why="O")
    L.add(f"{day} 10:00:30", hx(p ^ B6), 1.0, lead=0, why="Y: alike to O, 30 s")
    L.add(f"{day} 10:00:38", hx(p ^ A6), 1.0, lead=0, why="Y': alike to O, 38 s")
    L.add(f"{day} 9:59:50", hx(p ^ B6), 1.0, lead=0, why="Z: out of order (10 s before O), alike to O and Y")
    L.add(f"{day} 9:59:55", hx(p ^ A6), 0.5, lead=0, why="W: matches O only (5 s); Y' has its hash but is 43 s in its future")
    L.next_scenario()
    p = rand64(rng)
    day = L.base.strftime("%Y:%m:%d")
    L.add(f"{day} 10:00:00", hx(p), 9.0, lead=1)
    L.add(f"{day} 10:00:05", hx(p), 1.0, lead=0)
    L.add(f"{day} 10:00:0x", hx(p), 8.0, lead=1, why="unparsable in the middle of a band: closes the burst")
    L.add(f"{day} 10:00:10", hx(p), 1.0, lead=1, why="its matches lie before the unparsable row")
    L.add(f"{day} 10:00:12", hx(p), 0.5, lead=0)
    L.add(f"{day} 10:00:61", hx(p), 0.25, lead=1, why="second 61")
    L.add(f"{day} 24:00:00", hx(p), 0.25, lead=1, why="hour 24")
    L.next_scenario()
    # no date at all: NULL and '' sort first
    p = rand64(rng)
    L.add(None, hx(p), 3.0, lead=1, why="NULL date")
    L.add("", hx(p), 3.0, lead=1, why="empty date")
    L.add("0000:00:00 00:00:00", hx(p), 3.0, lead=1, why="the camera's null date")
    # 2^32 seconds apart: low words 5 s apart
    p = rand64(rng)
    t0 = datetime(1900, 1, 1, 0, 0, 0)
    L.add(t0.strftime(FMT), hx(p), 9.0, lead=1)
    L.add((t0 + timedelta(seconds=5)).strftime(FMT), hx(p), 1.0, lead=0)
    L.add((t0 + timedelta(seconds=2 ** 32 + 7)).strftime(FMT), hx(p), 0.5, lead=1, why="2^32 + 7 s after the first photo")
    t1 = datetime(9999, 12, 31, 23, 59, 50)
    L.add(t1.strftime(FMT), hx(p), 0.5, lead=1, why="the last year strptime accepts")
    L.add((t1 + timedelta(seconds=9)).strftime(FMT), hx(p), 0.25, lead=0)
    L.add("0001:01:01 00:00:00", hx(p), 0.5, lead=1, why="the first year")
    return L


DATES = {"similarity_threshold_percent": 90, "time_window_minutes": 40 / 60, "rapid_burst_seconds": 0}


def lib_rapid(rng):
    """RAPID settings (distance 6 / 12, window 60 s, rapid 5 s). Pairs 2 s apart and 10 bits apart: only the rapid rule can join them,
    so the person test decides."""
    L = Lib()

    def pair(pa, pb, joins, why, dist_mask=0x3FF, gap=2):
        p = rand64(rng)
        L.add(L.at(0), hx(p), 9.0, persons=pa, lead=1)
        L.add(L.at(gap), hx(p ^ dist_mask), 1.0, persons=pb, lead=0 if joins else 1, why=why)
        L.next_scenario()

    pair((), (), True, "no persons on either side")
    pair((1, 2), (), True, "one side without persons")
    pair((), (3,), True, "the other side without persons")
    pair((1, 2), (3, 4), False, "disjoint persons")
    pair((1, 2, 9), (3, 4, 9), True, "lists that overlap in their last element only")
    pair((9,), (1, 2, 9), True, "one id against the last of three")
    pair(tuple(range(1, 41)), tuple(range(41, 81)), False, "40 disjoint ids each")
    pair(tuple(range(1, 40)) + (100,), tuple(range(41, 80)) + (100,), True, "40 ids each, the last one shared")
    pair((1, 2), (3, 4), True, "disjoint persons but 6 bits: the slow rule", dist_mask=0x3F)
    pair((), (), False, "13 bits: beyond 2 thr", dist_mask=0x1FFF)
    pair((), (), True, "exactly rapid_s apart", gap=5)
    pair((), (), False, "one second past rapid_s", gap=6)
    return L


# rapid_s > window_s: window 3 s, rapid 10 s - the search must reach back 10 s
RAPID_WIDE = {"similarity_threshold_percent": 90, "time_window_minutes": 0.05, "rapid_burst_seconds": 10}
# rapid_s = 0: photos of one second only
RAPID_ZERO = {"similarity_threshold_percent": 90, "time_window_minutes": 1, "rapid_burst_seconds": 0}


def lib_rapid_wide(rng):
    L = Lib()
    p = rand64(rng)
    L.add(L.at(0), hx(p), 9.0, persons=(1,), lead=1)
    L.add(L.at(8), hx(p ^ 0x3FF), 1.0, persons=(1,), lead=0, why="8 s > window 3 s, inside rapid 10 s, shared person")
    L.add(L.at(16), hx(p ^ 0x3FF), 1.0, persons=(2,), lead=1, why="8 s but no shared person, and outside the window for the slow rule")
    L.add(L.at(19), hx(p ^ 0x3FF), 0.5, persons=(3,), lead=0, why="3 s: the slow rule needs no person")
    L.add(L.at(30), hx(p ^ 0x3FF), 0.5, persons=(3,), lead=1, why="11 s: past both")
    L.next_scenario()
    return L


def lib_rapid_zero(rng):
    L = Lib()
    p = rand64(rng)
    L.add(L.at(0), hx(p), 9.0, lead=1)
    L.add(L.at(0), hx(p ^ 0x3FF), 1.0, lead=0, why="same second, 10 bits: rapid rule with rapid_s = 0")
    L.add(L.at(1), hx(p ^ 0xFFC00), 1.0, lead=1, why="one second later, 10 / 20 bits from the two before")
    L.next_scenario()
    return L


def lib_thr(rng):
    """One library under 100 % (thr 0), 0 % (thr 64) and 110 % (thr -6), window 60 s, rapid 5 s."""
    L = Lib()
    p = rand64(rng)
    L.add(L.at(0), hx(p), 9.0)
    L.add(L.at(1), hx(p), 1.0)                       # identical
    L.add(L.at(2), hx(p ^ 1), 1.0)                   # one bit
    L.add(L.at(3), hx(p ^ (2 ** 64 - 1)), 1.0)       # 64 bits
    L.add(L.at(4), "", 1.0)                          # no hash: 999
    L.add(L.at(5), hx(p), 0.5)
    L.add(L.at(200), hx(p), 0.5)                     # outside the window
    return L


THR_EXPECT = {100: [1, 0, 1, 1, 1, 1, 1], 0: [1, 0, 0, 0, 1, 1, 1], 110: [1, 1, 1, 1, 1, 1, 1]}


def lib_two(rng):
    L = Lib()
    p = rand64(rng)
    L.add(L.at(0), hx(p), 1.0, lead=0)
    L.add(L.at(1), hx(p), 2.0, lead=1, why="n = 2: one burst, the second photo scores higher")
    return L


def lib_one(rng):
    L = Lib()
    L.add(L.at(0), hx(rand64(rng)), None, lead=1, why="n = 1")
    return L


def lib_long(rng):
    """One sequence of 150 alike photos, 80 of them within one second (a sports run), under the shipped settings; ties and missing
    aggregates decide the lead."""
    L = Lib()
    p = rand64(rng)
    t = 0
    for k in range(150):
        if not 30 <= k < 110:
            t += 1
        agg = [None, 0.0, 7.25, 7.25, 3.0][k % 5]
        L.add(L.at(t), hx(flip(rng, p, int(rng.integers(0, 4)))), agg, persons=(1,) if k % 3 == 0 else ())
    return L


def lib_planted(rng, n=320):
    """Sessions of 1-9 alike photos seconds apart, some with persons, some rows without hash or date; inserted in shuffled order with
    DISTINCT date strings (the order check of the host test runs on this case)."""
    rows, t, used = [], datetime(2022, 7, 1, 8, 0, 0), set()
    while len(rows) < n:
        centre = rand64(rng)
        t += timedelta(seconds=int(rng.integers(30, 4000)))
        who = [(), (1,), (1, 2), (3,)][int(rng.integers(0, 4))]
        for _ in range(int(rng.integers(1, 10))):
            t += timedelta(seconds=int(rng.integers(1, 9)))
            date = t.strftime(FMT) + ["", "", ".50", "+01:00"][int(rng.integers(0, 4))]
            roll = rng.random()
            if roll < 0.03:
                date = date[:17] + "xx"
            elif roll < 0.05:
                date = date.replace(":", "-", 2)
            assert date not in used
            used.add(date)
            h = hx(flip(rng, centre, int(rng.integers(0, 9))))
            roll = rng.random()
            if roll < 0.03:
                h = None
            elif roll < 0.05:
                h = ""
            persons = who if rng.random() < 0.8 else [(), (7,)][int(rng.integers(0, 2))]
            rows.append([date, [float(np.round(rng.uniform(0, 10), 2)), None, 5.0, 0.0][int(rng.integers(0, 4))], h, sorted(persons)])
    rows.append([None, 4.0, hx(rand64(rng)), []])      # a single NULL date (the strings stay distinct)
    L = Lib()
    L.rows = [rows[i] for i in rng.permutation(len(rows))]
    return L


def run_reference(process_bursts, rows, settings):
    with tempfile.TemporaryDirectory() as d:
        db, cfg = os.path.join(d, "photos.db"), os.path.join(d, "scoring_config.json")
        config = {"categories": []}
        if settings is not None:
            config["burst_detection"] = settings
        json.dump(config, open(cfg, "w"))
        paths = [f"/p/{i:06d}.jpg" for i in range(len(rows))]
        with sqlite3.connect(db) as conn:
            conn.execute("CREATE TABLE photos (path TEXT PRIMARY KEY, date_taken TEXT, aggregate REAL, phash TEXT, is_burst_lead INTEGER DEFAULT 0)")
            conn.execute("CREATE TABLE faces (id INTEGER PRIMARY KEY AUTOINCREMENT, photo_path TEXT, person_id INTEGER)")
            conn.executemany("INSERT INTO photos (path, date_taken, aggregate, phash) VALUES (?, ?, ?, ?)",
                             [(paths[i], r[0], r[1], r[2]) for i, r in enumerate(rows)])
            faces = [(paths[i], p) for i, r in enumerate(rows) for p in r[3]]
            faces += [(paths[i], None) for i in range(0, len(rows), 7) if faces]     # faces nobody was identified on
            conn.executemany("INSERT INTO faces (photo_path, person_id) VALUES (?, ?)", faces)
            conn.commit()
        with contextlib.redirect_stdout(io.StringIO()):
            process_bursts(db, cfg)
        with sqlite3.connect(db) as conn:
            order = [paths.index(r[0]) for r in conn.execute("SELECT path, date_taken, aggregate, phash FROM photos WHERE phash IS NOT NULL ORDER BY date_taken")]
            lead = dict(conn.execute("SELECT path, is_burst_lead FROM photos"))
    return order, [int(lead[p]) for p in paths]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from processing.scorer import process_bursts            # noqa: E402
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bursts_ref                                        # the plain restatement: used for the non-triviality counts only

    rng = np.random.default_rng(20240917)
    shipped = {"similarity_threshold_percent": 70, "time_window_minutes": 0.8, "rapid_burst_seconds": 0.4}
    planted, long_run, thr_lib = lib_planted(rng), lib_long(rng), lib_thr(rng)
    cases = [("one", lib_one(rng), None), ("two", lib_two(rng), None), ("bands", lib_bands(rng), BANDS), ("dates", lib_dates(rng), DATES),
             ("rapid", lib_rapid(rng), RAPID), ("rapid_wide", lib_rapid_wide(rng), RAPID_WIDE), ("rapid_zero", lib_rapid_zero(rng), RAPID_ZERO),
             ("long_shipped", long_run, shipped), ("long_fallback", long_run, None),
             ("planted_fallback", planted, None), ("planted_shipped", planted, shipped),
             ("planted_85_2_3", planted, {"similarity_threshold_percent": 85, "time_window_minutes": 2, "rapid_burst_seconds": 3})]
    for pct, want in THR_EXPECT.items():
        lib = Lib()
        lib.rows = thr_lib.rows
        lib.expect = [(i, w, f"{pct} %") for i, w in enumerate(want)]
        cases.append((f"thr_{pct}", lib, {"similarity_threshold_percent": pct, "time_window_minutes": 1, "rapid_burst_seconds": 5}))

    out, big, longest, longest_second = {"cases": []}, 0, 0, 0
    for name, lib, settings in cases:
        order, lead = run_reference(process_bursts, lib.rows, settings)
        for row, want, why in lib.expect:
            assert lead[row] == want, (name, row, lib.rows[row], "expected", want, why)
        # the order the reference read the rows in is NULL first, then byte order, ties in insertion order
        keyed = sorted((i for i, r in enumerate(lib.rows) if r[2] is not None),
                       key=lambda i: (0, b"") if lib.rows[i][0] is None else (1, lib.rows[i][0].encode()))
        assert keyed == order, name
        sizes = bursts_ref.burst_sizes_from_rows([lib.rows[i] for i in order], settings)
        assert sum(sizes) == len(order) and len(sizes) == sum(lead[i] for i in order), name
        big += sum(1 for s in sizes if s >= 3)
        if name.startswith("long") and max(sizes) >= longest:
            longest = max(sizes)
            dates = [lib.rows[i][0] for i in order]
            longest_second = max(dates.count(d) for d in set(dates))
        out["cases"].append({"name": name, "settings": settings, "order": order, "table": [r + [lead[i]] for i, r in enumerate(lib.rows)]})
        print(f"{name:>18}: {len(lib.rows):4d} photos, {len(order):4d} with a hash, {len(sizes):4d} bursts (largest {max(sizes)}), "
              f"{len(lib.expect)} leads asserted")
    assert big >= 10, big
    assert longest >= 130 and longest_second >= 70, (longest, longest_second)
    assert len(set(r[0] for r in planted.rows)) == len(planted.rows)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bursts_golden.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
