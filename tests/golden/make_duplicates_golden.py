"""Generates tests/golden/duplicates_golden.json by RUNNING THE REFERENCE'S OWN `detect_duplicates` (utils/duplicate.py:44-169) in
the build container on a scratch SQLite file with a minimal v4 configuration. The hashes and aggregates are made up HERE
(seeded); nothing of the reference is stored, only our inputs and the `duplicate_group_id` / `is_duplicate_lead` columns its
code wrote. Rows are given paths that sort in input order (the reference reads them `ORDER BY path`); rows without a hash are
stored too (phash null) - the reference leaves them out of the comparison and so must the caller of find_duplicates.

    python tests/golden/make_duplicates_golden.py
"""
import contextlib
import io
import json
import os
import sqlite3
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
from utils.duplicate import detect_duplicates            # noqa: E402


def hx(v):
    return format(int(v) & (2 ** 64 - 1), "016x")


def flip(rng, v, bits):
    for b in rng.choice(64, size=bits, replace=False):
        v ^= 1 << int(b)
    return v


def rand64(rng):
    return int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))


def case_none(rng):
    return [(hx(rand64(rng)), float(rng.uniform(0, 10))) for _ in range(40)]


def case_chain(rng):
    """A~B, B~C, A!~C at the 90 % threshold (distance <= 6): B = A + 5 bits, C = B + 5 other bits -> A..C differ in 10."""
    rows = []
    for _ in range(6):
        a = rand64(rng)
        bits = rng.choice(64, size=10, replace=False)
        b, c = a, a
        for k in bits[:5]:
            b ^= 1 << int(k)
        c = b
        for k in bits[5:]:
            c ^= 1 << int(k)
        trio = [a, b, c]
        rng.shuffle(trio)
        rows += [(hx(v), float(rng.uniform(0, 10))) for v in trio]
        rows.append((hx(rand64(rng)), float(rng.uniform(0, 10))))
    return rows


def case_ties(rng):
    """Equal aggregates inside a group, a NULL aggregate, a zero, rows without a hash, exact copies and leading zeros."""
    a, b, c = rand64(rng), rand64(rng), rand64(rng) >> 20
    return [(hx(a), 7.5), (None, 9.9), (hx(flip(rng, a, 2)), 7.5), (hx(b), None), (hx(flip(rng, b, 1)), 0.0), (hx(flip(rng, b, 3)), None),
            (hx(c), 3.25), (None, None), (hx(c), 3.25), (hx(c), 3.0), (hx(flip(rng, a, 1)), 7.5), (hx(rand64(rng)), 8.0),
            (hx(0), 1.0), (hx(1), 2.0), (hx(2 ** 64 - 1), 5.0)]


def case_planted(rng):
    """About 300 rows: 40 clusters of 2-7 members within a few bits of a centre, the rest random; shuffled."""
    rows = []
    for _ in range(40):
        centre = rand64(rng)
        for _ in range(int(rng.integers(2, 8))):
            rows.append((hx(flip(rng, centre, int(rng.integers(0, 5)))), [float(rng.uniform(0, 10)), None, 5.0][int(rng.integers(0, 3))]))
    while len(rows) < 300:
        rows.append((hx(rand64(rng)) if rng.random() > 0.05 else None, float(rng.uniform(0, 10))))
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def run_reference(rows, similarity):
    with tempfile.TemporaryDirectory() as d:
        db, cfg = os.path.join(d, "photos.db"), os.path.join(d, "scoring_config.json")
        json.dump({"categories": [], "duplicate_detection": {"similarity_threshold_percent": similarity}}, open(cfg, "w"))
        with sqlite3.connect(db) as conn:
            conn.execute("CREATE TABLE photos (path TEXT PRIMARY KEY, phash TEXT, aggregate REAL, duplicate_group_id INTEGER, "
                         "is_duplicate_lead INTEGER DEFAULT 0)")
            conn.executemany("INSERT INTO photos (path, phash, aggregate) VALUES (?, ?, ?)",
                             [(f"/p/{i:06d}.jpg", h, a) for i, (h, a) in enumerate(rows)])
            conn.commit()
        with contextlib.redirect_stdout(io.StringIO()) as log:
            detect_duplicates(db, cfg)
        with sqlite3.connect(db) as conn:
            got = conn.execute("SELECT duplicate_group_id, is_duplicate_lead FROM photos ORDER BY path").fetchall()
    return [g for g, _ in got], [int(l or 0) for _, l in got], log.getvalue().splitlines()[0]


def main():
    rng = np.random.default_rng(20240607)
    inputs = {"none": case_none(rng), "chain": case_chain(rng), "ties": case_ties(rng), "planted": case_planted(rng)}
    out = {"cases": [], "max_distance": {}}
    for name, rows in inputs.items():
        for sim in (100, 95, 90, 80):
            gid, lead, first = run_reference(rows, sim)
            out["max_distance"][str(sim)] = int(first.split("<= ")[1].rstrip(")"))       # the value the reference printed
            out["cases"].append({"name": name, "similarity": sim, "phash": [h for h, _ in rows], "aggregate": [a for _, a in rows],
                                 "group_id": gid, "is_lead": lead})
            print(f"{name:>8} @ {sim:3d} %: {len(rows)} rows, {len(set(g for g in gid if g is not None))} groups, {sum(lead)} leads | {first}")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "duplicates_golden.json")
    json.dump(out, open(path, "w"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
