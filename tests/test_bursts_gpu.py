"""fe_burst_links on the GPU: exactly the brute force of tests/bursts_ref.py (every earlier row tried, no band, no early exit) on every
case of tests/golden/bursts_golden.json and on seeded random libraries, and `find_bursts` against the `is_burst_lead` column that the
reference's own process_bursts wrote (tests/golden/make_bursts_golden.py lists the edges the cases decide: bands of 0, 1, 63, 64, 65
and 129 predecessors, a match in the last row of the band and one just below it, the largest of several matches, unparsable and
out-of-order dates, upper-word hashes, thr 0 / 64 / negative, rapid_s above window_s and 0, the person lists, rows without hash or date).
The array-level cases below add what no date string can express: rows in any order, times 2^32 and 2^61 apart, distances of 999.
Links are integers: every comparison is for equality."""
import numpy as np
import pytest

import bursts_ref
from facet_amd import EngineError
from facet_amd._lib import FE_ERR_INVALID
from facet_amd.bursts import burst_rows, burst_settings, find_bursts
from test_bursts_host import case_names, columns, golden_cases

pytestmark = pytest.mark.gpu


def links_resident(engine, hashes, *rest):
    d = engine.dev_alloc(hashes.nbytes)
    try:
        engine.h2d(d, hashes)
        return engine.burst_links((d, len(hashes)), *rest)
    finally:
        engine.dev_free(d)


@pytest.mark.parametrize("name", case_names())
def test_links_equal_the_brute_force_on_the_golden_cases(engine, name):
    case = golden_cases()[name]
    rows = case["rows"]
    persons = [r[3] for r in rows]
    hashes, times, flags, off, ids = burst_rows([r[2] for r in rows], [r[0] for r in rows], persons if any(persons) else None)
    rest = (times, flags, *burst_settings(case["settings"]), off, ids)
    got = engine.burst_links(hashes, *rest)
    assert got.dtype == np.int32 and got.tolist() == case["links"]
    if len(rows) >= 2:
        assert np.array_equal(links_resident(engine, hashes, *rest), got)


@pytest.mark.parametrize("name", case_names())
def test_find_bursts_equals_the_references_column(engine, name):
    phash, dates, aggregates, persons, want = columns(golden_cases()[name])
    burst_id, lead = find_bursts(engine, phash, dates, aggregates, persons, **(golden_cases()[name]["settings"] or {}))
    assert lead == want
    assert [b is None for b in burst_id] == [h is None for h in phash]


def random_library(rng, n, with_persons):
    """Arrays of Engine.burst_links. Times: a dense walk (0 - 3 s steps, so bands run over several chunks of 64), a tenth of the rows
    moved out of order, a few shifted by +-2^32 (low words stay close) and two at the ends of the accepted range; hashes: families a
    few bits around a centre, some members differing in the upper word only, some exact copies of a row up to 90 back; 5 % of the rows without a date, 5 % without a hash."""
    times = 10 ** 9 + np.cumsum(rng.integers(0, 4, n)).astype(np.int64)
    moved = rng.random(n) < 0.1
    times[moved] = rng.permutation(times[moved])
    shifted = rng.random(n) < 0.03
    times[shifted] += rng.choice([-2 ** 32, 2 ** 32], int(shifted.sum()))
    if n >= 8:
        times[rng.integers(0, n)] = 2 ** 61
        times[rng.integers(0, n)] = -2 ** 61
    centres = [int(rng.integers(0, 2 ** 63)) * 2 + 1 for _ in range(4)]
    hashes = np.zeros(n, np.uint64)
    for i in range(n):
        v = centres[int(rng.integers(0, 4))]
        for b in rng.choice(64, size=int(rng.integers(0, 9)), replace=False):
            v ^= 1 << int(b)
        if rng.random() < 0.1:
            v ^= int(rng.integers(0, 2 ** 32)) << 32
        if i and rng.random() < 0.15:                      # exact copies of an earlier row: the matches of thr = 0
            v = int(hashes[rng.integers(max(0, i - 90), i)])
        hashes[i] = v
    flags = np.full(n, 3, np.uint8)
    flags[rng.random(n) < 0.05] &= 1
    flags[rng.random(n) < 0.05] &= 2
    if not with_persons:
        return hashes, times, flags, None, None
    off, ids = [0], []
    for i in range(n):
        roll = rng.random()
        k = 0 if roll < 0.3 else (40 if roll > 0.97 else int(rng.integers(1, 5)))
        ids += sorted(rng.choice(60 if k == 40 else 8, size=k, replace=False).tolist())
        off.append(len(ids))
    return hashes, times, flags, np.array(off, np.int32), np.array(ids, np.int32)


# (thr, window_s, rapid_s): the fallbacks, the shipped settings, rapid above the window, rapid 0 with a tight distance, thr 0, thr 64
# (2 thr = 128: still below 999), a negative thr with a wide window, and limits that reach across the 2^32 shifts
SETTINGS = [(7, 3600, 5), (19, 48, 0), (6, 3, 10), (2, 60, 0), (0, 20, 2), (64, 4, 1), (-6, 3600, 5), (9, 2 ** 32 + 10, 2 ** 33)]


@pytest.mark.parametrize("n,with_persons", [(2, True), (3, False), (64, True), (65, False), (66, True), (130, True), (700, True), (700, False), (1500, True)])
def test_links_equal_the_brute_force_on_random_libraries(engine, n, with_persons):
    rng = np.random.default_rng(1000 + n + int(with_persons))
    lib = random_library(rng, n, with_persons)
    hashes, times, flags, off, ids = lib
    picks = SETTINGS if n <= 130 else [SETTINGS[k] for k in ((0, 2, 7) if n == 700 else (1, 2))]
    for thr, window_s, rapid_s in picks:
        want = bursts_ref.links_from_arrays(hashes, times, flags, thr, window_s, rapid_s, off, ids)
        got = engine.burst_links(hashes, times, flags, thr, window_s, rapid_s, off, ids)
        print(f"[bursts] n {n} persons {with_persons} settings {(thr, window_s, rapid_s)}: {sum(1 for v in want if v >= 0)} rows linked, "
              f"farthest link {max((i - v for i, v in enumerate(want) if v >= 0), default=0)} rows back")
        assert got.tolist() == want, (n, thr, window_s, rapid_s)
    thr, window_s, rapid_s = picks[-1]
    assert np.array_equal(links_resident(engine, hashes, times, flags, thr, window_s, rapid_s, off, ids), got)


@pytest.mark.parametrize("n", [2, 64, 65, 66, 129, 130, 193, 257])
def test_one_timestamp_and_the_only_match_in_row_zero(engine, n):
    """The worst band: every row has every earlier row in reach. Row 0 is the only one alike to the last row, so the wave walks all of
    its chunks and the match is the last lane it looks at; the rows between are alike to each other (they link to their neighbour)."""
    p = 0x0123456789ABCDEF
    hashes = np.full(n, p ^ 0xFFF, np.uint64)
    hashes[0], hashes[n - 1] = p, p ^ (0x3F << 50)
    times, flags = np.full(n, 1_700_000_000, np.int64), np.full(n, 3, np.uint8)
    got = engine.burst_links(hashes, times, flags, 6, 60, 0)             # 2 thr = 12: the rows between are exactly 12 bits from row 0
    assert got.tolist() == bursts_ref.links_from_arrays(hashes, times, flags, 6, 60, 0)
    assert got[n - 1] == 0 and (n < 3 or got[1] == 0)
    got = engine.burst_links(hashes, times, flags, 6, 60, -1)            # without the rapid rule they are not alike to row 0
    assert got.tolist() == bursts_ref.links_from_arrays(hashes, times, flags, 6, 60, -1)
    assert got[n - 1] == 0 and (n < 3 or got[1] == -1)


def test_times_stay_64_bit_and_rows_may_come_in_any_order(engine):
    """Row 1 is out of order and 2^32 - 3 s older than row 0: it is inside row 2's band (the band's lower end comes from the prefix
    maximum) and its low word is 8 s from row 2's, but it is not a match; row 0 is."""
    t = 1_700_000_000
    times = np.array([t, t - 2 ** 32 + 3, t + 5, t + 2 ** 32 + 6, t + 7, 2 ** 61, -2 ** 61, t + 8], np.int64)
    hashes = np.full(8, 0xF0F0F0F0F0F0F0F0, np.uint64)
    flags = np.full(8, 3, np.uint8)
    got = engine.burst_links(hashes, times, flags, 0, 10, 0)
    assert got.tolist() == [-1, -1, 0, -1, 2, -1, -1, 4] == bursts_ref.links_from_arrays(hashes, times, flags, 0, 10, 0)
    # a reach of 2^62 s covers all of them: every row links to the one before it
    assert engine.burst_links(hashes, times, flags, 0, 2 ** 62, 0).tolist() == [-1, 0, 1, 2, 3, 4, 5, 6]
    assert engine.burst_links(hashes, times, flags, 0, 2 ** 70, -2 ** 70).tolist() == [-1, 0, 1, 2, 3, 4, 5, 6]   # clamped, not wrapped


def test_distance_999_and_settings_that_let_nothing_pass(engine):
    hashes = np.array([5, 5, 5, 5], np.uint64)
    times = np.array([100, 101, 102, 103], np.int64)
    flags = np.array([3, 2, 3, 3], np.uint8)                              # row 1 has no hash
    for thr, want in ((64, [-1, -1, 0, 2]), (998, [-1, -1, 0, 2]), (999, [-1, 0, 1, 2]), (500, [-1, -1, 0, 2]), (2 ** 31 - 1, [-1, 0, 1, 2])):
        assert engine.burst_links(hashes, times, flags, thr, 60, -1).tolist() == want == bursts_ref.links_from_arrays(hashes, times, flags, thr, 60, -1), thr
    assert engine.burst_links(hashes, times, flags, 500, 60, 5).tolist() == [-1, 0, 1, 2]        # 2 thr = 1000 admits 999 by the rapid rule
    assert engine.burst_links(hashes, times, flags, -1, 60, 5).tolist() == [-1] * 4
    assert engine.burst_links(hashes, times, flags, -2 ** 31, 60, 5).tolist() == [-1] * 4
    assert engine.burst_links(hashes, times, flags, 64, -1, -5).tolist() == [-1] * 4
    assert engine.burst_links(hashes, times, np.array([3, 3, 1, 3], np.uint8), 64, 60, 5).tolist() == [-1, 0, -1, 1]   # row 2 has no date


def test_small_n_and_bad_arguments_launch_nothing(engine):
    empty = engine.burst_links(np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint8), 7, 3600, 5)
    assert empty.shape == (0,) and empty.dtype == np.int32
    assert engine.burst_links(np.array([9], np.uint64), np.array([4], np.int64), np.array([3], np.uint8), 7, 3600, 5).tolist() == [-1]
    h, t, f = np.array([1, 1, 1], np.uint64), np.array([5, 6, 7], np.int64), np.array([3, 3, 3], np.uint8)
    good_off, good_ids = np.array([0, 2, 2, 3], np.int32), np.array([1, 4, 4], np.int32)
    assert engine.burst_links(h, t, f, 7, 60, 5, good_off, good_ids).tolist() == [-1, 0, 1]
    assert engine.burst_links(h, t, f, 7, 60, 5, np.zeros(4, np.int32), np.zeros(0, np.int32)).tolist() == [-1, 0, 1]   # all lists empty
    bad = [((h, t, np.array([3, 4, 3], np.uint8), 7, 60, 5), "flags"),
           ((h, np.array([5, 2 ** 61 + 1, 7], np.int64), f, 7, 60, 5), "times"),
           ((h, t, f, 7, 60, 5, np.array([0, 2, 1, 3], np.int32), good_ids), "person_off"),
           ((h, t, f, 7, 60, 5, np.array([0, 2, 2, 4], np.int32), good_ids), "person_off"),
           ((h, t, f, 7, 60, 5, np.array([-1, 2, 2, 3], np.int32), good_ids), "person_off"),
           ((h, t, f, 7, 60, 5, np.array([0, 1000, 1000, 3], np.int32), good_ids), "person_off"),
           ((h, t, f, 7, 60, 5, good_off, np.array([4, 1, 4], np.int32)), "ascending"),
           ((h, t, f, 7, 60, 5, good_off, np.array([4, 4, 4], np.int32)), "ascending")]
    for args, word in bad:
        with pytest.raises(EngineError, match=word) as e:
            engine.burst_links(*args)
        assert e.value.status == FE_ERR_INVALID and "fe_burst_links" in str(e.value)
    # a time out of range on a row WITHOUT a date is not read
    assert engine.burst_links(h, np.array([5, 2 ** 62, 7], np.int64), np.array([3, 1, 3], np.uint8), 7, 60, 5).tolist() == [-1, -1, 0]
    assert engine.lib.fe_burst_links(engine.h, None, 0, None, None, 3, None, None, 0, 7, 60, 5, None) == FE_ERR_INVALID
    assert engine.lib.fe_burst_links(engine.h, None, 0, None, None, -1, None, None, 0, 7, 60, 5, None) == FE_ERR_INVALID
    assert engine.burst_links(h, t, f, 7, 60, 5).tolist() == [-1, 0, 1]                          # the context stays usable
    with pytest.raises(ValueError):
        engine.burst_links(h, t[:2], f, 7, 60, 5)
    with pytest.raises(ValueError):
        engine.burst_links(h, t, f, 7, 60, 5, good_off, None)
