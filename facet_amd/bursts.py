"""Burst detection over stored hashes: the mirror of the reference's `process_bursts` (processing/scorer.py:1880-1986), without the
database.

The reference walks the photos in `date_taken` order with one open burst: a photo joins it when it is "similar" to ANY member (taken
close together and alike by perceptual hash, :1943-1968), otherwise the burst is closed, its best-scoring member becomes
`is_burst_lead = 1`, and the photo opens the next one. That loop parses two date strings per comparison and is quadratic in the length
of a burst. The open burst is always the contiguous run [s, i-1] of the ordered rows, so "similar to any member" is `L(i) >= s`, where
L(i) is the largest j < i that passes the pair test. L does not depend on s: it is one engine call (`fe_burst_links`, one wave per
photo on the GPU); the recurrence over it and the choice of the lead are the O(n) loop of `group_bursts` below. The pair search has
no host version in this package: without a GPU context it is an error, as everywhere else.

`utils/burst.py::IncrementalBurstProcessor` is another algorithm (several open bursts, no hash test in its rapid rule, pruning) that
nothing in the reference calls; it is not mirrored.
"""
import math
import re
from datetime import datetime

import numpy as np

from ._lib import FE_BURST_HAS_DATE, FE_BURST_HAS_HASH

_CANONICAL = re.compile(r"[0-9]{4}:[0-9]{2}:[0-9]{2} [0-9]{2}:[0-9]{2}:[0-9]{2}", re.ASCII)


def _seconds(dt):
    return (dt.toordinal() * 24 + dt.hour) * 3600 + dt.minute * 60 + dt.second


def parse_date(s):
    """A `date_taken` value -> whole seconds (since the day before 0001-01-01; only differences are used), or None where the reference's
    `parse_date` gives None (scorer.py:1925-1931): `datetime.strptime(s[:19], '%Y:%m:%d %H:%M:%S')`, anything that raises ValueError
    or TypeError being "no date". The canonical form, 19 ASCII characters with all fields zero-padded, skips strptime: the same
    fields go to the same constructor, which refuses what strptime refuses there (year 0, month 13, 30 February, hour 24, second 60)."""
    if not s:
        return None
    try:
        head = s[:19]
        if isinstance(head, str) and _CANONICAL.fullmatch(head):
            return _seconds(datetime(int(head[0:4]), int(head[5:7]), int(head[8:10]), int(head[11:13]), int(head[14:16]), int(head[17:19])))
        return _seconds(datetime.strptime(head, "%Y:%m:%d %H:%M:%S"))
    except (ValueError, TypeError):
        return None


def burst_settings(cfg_dict=None):
    """The `burst_detection` block of the scoring configuration (None: the fallbacks 88 / 60 / 5 of scorer.py:1885-1887) ->
    (thr, window_s, rapid_s) as integers. thr = int(64 * (1 - percent / 100)) as the reference computes it; the two time limits are
    compared with whole-second differences (`d <= time_window_minutes * 60`, `d <= rapid_burst_seconds`), so the floor of the
    reference's own float expression decides the same pairs: 0.8 * 60 -> 48, 0.4 -> 0."""
    cfg = cfg_dict or {}
    percent = cfg.get("similarity_threshold_percent", 88)
    minutes = cfg.get("time_window_minutes", 60)
    rapid = cfg.get("rapid_burst_seconds", 5)
    return int(64 * (1 - percent / 100)), math.floor(minutes * 60), math.floor(rapid)


def burst_order(date_strings):
    """Row order of the reference's `ORDER BY date_taken`: NULL first, then text in byte order (SQLite's BINARY collation compares
    the UTF-8 bytes), equal values in input order. A column that also holds numbers or blobs follows SQLite's storage classes: numbers
    before text, blobs after. -> list of row indices."""
    def key(i):
        s = date_strings[i]
        if s is None:
            return (0, 0)
        if isinstance(s, str):
            return (2, s.encode("utf-8", "surrogatepass"))
        if isinstance(s, (bytes, bytearray, memoryview)):
            return (3, bytes(s))
        return (1, s)
    return sorted(range(len(date_strings)), key=key)


def group_bursts(links, aggregates):
    """links: per ordered row the largest earlier row it is similar to, or -1 (Engine.burst_links); aggregates: the rows' scores (None
    allowed). -> (burst_id, is_burst_lead): bursts numbered from 1 in row order - a row that joins nothing is a burst of one, and the
    reference marks it as a lead too - and 1 on the first member with the largest `aggregate or 0` of each (scorer.py:1970-1984)."""
    n = len(links)
    if len(aggregates) != n:
        raise ValueError(f"{n} links but {len(aggregates)} aggregates")
    burst_id, is_lead = [0] * n, [0] * n
    start, number, lead, lead_score = 0, 0, 0, 0
    for i, link in enumerate(np.asarray(links, dtype=np.int64).tolist()):
        score = aggregates[i] or 0
        if i > 0 and link >= start:
            if score > lead_score:           # strictly: among equals the earliest row stays the lead
                lead, lead_score = i, score
        else:
            if i > 0:
                is_lead[lead] = 1
            start, lead, lead_score = i, i, score
            number += 1
        burst_id[i] = number
    if n:
        is_lead[lead] = 1
    return burst_id, is_lead


def _hash_value(h):
    v = int(h, 16)
    if not 0 <= v < 1 << 64:
        raise ValueError(f"phash {h!r} does not fit 64 bits")
    return v


def burst_rows(phashes, date_taken, person_ids=None):
    """Ordered rows -> the arrays of Engine.burst_links: (hashes uint64, times int64, flags uint8, person_off, person_ids). An empty
    hash string is "no hash" (the reference's distance 999), an unparsable date "no date". person_ids: per row an iterable of
    identified persons (any hashable values) or None; they are numbered densely and each row's list is sorted and distinct."""
    n = len(phashes)
    hashes, times, flags = np.zeros(n, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.uint8)
    for i in range(n):
        if phashes[i]:
            hashes[i] = _hash_value(phashes[i])
            flags[i] |= FE_BURST_HAS_HASH
        t = parse_date(date_taken[i])
        if t is not None:
            times[i] = t
            flags[i] |= FE_BURST_HAS_DATE
    if person_ids is None:
        return hashes, times, flags, None, None
    dense, off, ids = {}, [0], []
    for row in person_ids:
        ids.extend(sorted({dense.setdefault(p, len(dense)) for p in (row or ()) if p is not None}))
        off.append(len(ids))
    return hashes, times, flags, np.array(off, np.int32), np.array(ids, np.int32)


def find_bursts(engine, phashes, date_taken, aggregates, person_ids=None, **settings):
    """phashes / date_taken / aggregates (/ person_ids: per row the identified persons of its faces, or None): the photos' columns in
    the caller's order. settings: the keys of the `burst_detection` block. -> (burst_id, is_burst_lead) per row, as `process_bursts`
    writes the column: rows whose phash is None take no part and get (None, 1); the others are put in the reference's order
    (burst_order), linked on the GPU and grouped."""
    n = len(phashes)
    if len(date_taken) != n or len(aggregates) != n or (person_ids is not None and len(person_ids) != n):
        raise ValueError("find_bursts: the columns differ in length")
    unknown = set(settings) - {"similarity_threshold_percent", "time_window_minutes", "rapid_burst_seconds"}
    if unknown:
        raise TypeError(f"find_bursts: unknown settings {sorted(unknown)}")
    thr, window_s, rapid_s = burst_settings(settings)
    burst_id, is_lead = [None] * n, [1] * n
    rows = [i for i in range(n) if phashes[i] is not None]
    rows = [rows[k] for k in burst_order([date_taken[i] for i in rows])]
    if not rows:
        return burst_id, is_lead
    hashes, times, flags, off, ids = burst_rows([phashes[i] for i in rows], [date_taken[i] for i in rows],
                                                None if person_ids is None else [person_ids[i] for i in rows])
    links = engine.burst_links(hashes, times, flags, thr, window_s, rapid_s, off, ids)
    gid, lead = group_bursts(links, [aggregates[i] for i in rows])
    for k, i in enumerate(rows):
        burst_id[i], is_lead[i] = gid[k], lead[k]
    return burst_id, is_lead
