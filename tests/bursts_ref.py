"""Brute-force restatement of the pair test of the reference's `process_bursts` (processing/scorer.py:1919-1968) in plain Python:
L(i) = the largest j < i that row i is similar to, or -1, over ALL earlier rows - no band, no early exit. Two forms: from the raw
columns (strptime on the strings, the configuration's float values compared as they are) and from the integer arrays that
Engine.burst_links takes. Shared by the host and GPU tests and by tests/golden/make_bursts_golden.py (burst sizes only)."""
from datetime import datetime

NO_HASH = 999
HAS_HASH, HAS_DATE = 1, 2


def _parse(s):
    if not s:
        return None
    try:
        return datetime.strptime(s[:19], "%Y:%m:%d %H:%M:%S")
    except (ValueError, TypeError):
        return None


def _settings(settings):
    s = settings or {}
    return s.get("similarity_threshold_percent", 88), s.get("time_window_minutes", 60), s.get("rapid_burst_seconds", 5)


def links_from_rows(rows, settings):
    """rows: [date_taken, aggregate, phash, persons, ...] per photo in the reference's order (phash not None); settings: the
    `burst_detection` block or None."""
    percent, minutes, rapid = _settings(settings)
    thr = int(64 * (1 - percent / 100))
    dates = [_parse(r[0]) for r in rows]
    hashes = [int(r[2], 16) if r[2] else None for r in rows]
    persons = [set(r[3]) for r in rows]
    links = []
    for i in range(len(rows)):
        link = -1
        if dates[i] is not None:
            for j in range(i - 1, -1, -1):
                if dates[j] is None:
                    continue
                d = abs((dates[i] - dates[j]).total_seconds())
                dist = NO_HASH if hashes[i] is None or hashes[j] is None else bin(hashes[i] ^ hashes[j]).count("1")
                share = not persons[i] or not persons[j] or bool(persons[i] & persons[j])
                if (d <= rapid and share and dist <= thr * 2) or (d <= minutes * 60 and dist <= thr):
                    link = j
                    break
        links.append(link)
    return links


def links_from_arrays(hashes, times, flags, thr, window_s, rapid_s, person_off=None, person_ids=None):
    """The same over the arrays of Engine.burst_links (Python integers throughout: nothing wraps)."""
    h, t, f = [int(v) for v in hashes], [int(v) for v in times], [int(v) for v in flags]
    persons = None
    if person_off is not None:
        off, ids = [int(v) for v in person_off], [int(v) for v in person_ids]
        persons = [set(ids[off[i]:off[i + 1]]) for i in range(len(h))]
    links = []
    for i in range(len(h)):
        link = -1
        if f[i] & HAS_DATE:
            for j in range(i - 1, -1, -1):
                if not f[j] & HAS_DATE:
                    continue
                d = abs(t[i] - t[j])
                if d > window_s and d > rapid_s:
                    continue
                dist = bin(h[i] ^ h[j]).count("1") if f[i] & f[j] & HAS_HASH else NO_HASH
                share = persons is None or not persons[i] or not persons[j] or bool(persons[i] & persons[j])
                if (d <= rapid_s and share and dist <= thr * 2) or (d <= window_s and dist <= thr):
                    link = j
                    break
        links.append(link)
    return links


def burst_sizes(links):
    """The reference's walk over the links: row i joins the open burst [s, i-1] when links[i] >= s. -> the bursts' lengths in order."""
    sizes, start = [], 0
    for i, link in enumerate(links):
        if i > 0 and link >= start:
            sizes[-1] += 1
        else:
            sizes.append(1)
            start = i
    return sizes


def burst_sizes_from_rows(rows, settings):
    return burst_sizes(links_from_rows(rows, settings))
