"""facet_amd/bursts.py on the CPU against tests/golden/bursts_golden.json: the `is_burst_lead` column that the reference's own
`process_bursts` wrote for seeded libraries (tests/golden/make_bursts_golden.py; the generator asserts, scenario by scenario, which
lead each edge decides). The link search itself runs on the GPU (tests/test_bursts_gpu.py); here the brute force of
tests/bursts_ref.py stands in for it, so what is checked is the reformulation - `link[i] >= start of the open burst` - the lead
choice, the date parser, the settings and the row order."""
import json
import os
from datetime import datetime

import numpy as np
import pytest

import bursts_ref
from facet_amd.bursts import burst_order, burst_rows, burst_settings, find_bursts, group_bursts, parse_date

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_cache = {}


def golden_cases():
    """The recorded cases, each with its ordered rows and their brute-force links (computed once per session, never changed)."""
    if not _cache:
        for case in json.load(open(os.path.join(GOLDEN, "bursts_golden.json")))["cases"]:
            case["rows"] = [case["table"][i] for i in case["order"]]
            case["links"] = bursts_ref.links_from_rows(case["rows"], case["settings"])
            _cache[case["name"]] = case
    return _cache


def case_names():
    return [c["name"] for c in json.load(open(os.path.join(GOLDEN, "bursts_golden.json")))["cases"]]


class BruteForceEngine:
    """Engine.burst_links by the plain restatement (the host tests have no GPU)."""

    def burst_links(self, hashes, times, flags, thr, window_s, rapid_s, person_off=None, person_ids=None):
        return np.array(bursts_ref.links_from_arrays(hashes, times, flags, thr, window_s, rapid_s, person_off, person_ids), np.int32)


def columns(case):
    table = case["table"]
    persons = [r[3] for r in table]
    return [r[2] for r in table], [r[0] for r in table], [r[1] for r in table], persons if any(persons) else None, [r[4] for r in table]


@pytest.mark.parametrize("name", case_names())
def test_group_bursts_over_brute_force_links_reproduces_the_reference(name):
    case = golden_cases()[name]
    burst_id, lead = group_bursts(case["links"], [r[1] for r in case["rows"]])
    assert lead == [r[4] for r in case["rows"]]
    sizes = bursts_ref.burst_sizes(case["links"])
    assert burst_id == [k + 1 for k, s in enumerate(sizes) for _ in range(s)]
    assert sum(lead) == len(sizes)                                     # one lead per burst, bursts of one included


@pytest.mark.parametrize("name", case_names())
def test_arrays_and_floored_settings_give_the_links_of_the_raw_columns(name):
    """burst_rows + burst_settings (parsed once, floored) lose nothing against strptime per pair and the float settings."""
    case = golden_cases()[name]
    rows = case["rows"]
    persons = [r[3] for r in rows]
    arrays = burst_rows([r[2] for r in rows], [r[0] for r in rows], persons if any(persons) else None)
    assert bursts_ref.links_from_arrays(*arrays[:3], *burst_settings(case["settings"]), *arrays[3:]) == case["links"]


@pytest.mark.parametrize("name", case_names())
def test_find_bursts_in_the_callers_order(name):
    case = golden_cases()[name]
    phash, dates, aggregates, persons, want = columns(case)
    burst_id, lead = find_bursts(BruteForceEngine(), phash, dates, aggregates, persons, **(case["settings"] or {}))
    assert lead == want
    assert [b is None for b in burst_id] == [h is None for h in phash]
    assert all(l == 1 for l, h in zip(lead, phash) if h is None)


def test_burst_order_is_the_references_order_by():
    case = golden_cases()["planted_fallback"]
    dates = [r[0] for r in case["table"] if r[2] is not None]
    assert len(set(dates)) == len(dates)                               # distinct strings: the order is fully determined
    index = [i for i, r in enumerate(case["table"]) if r[2] is not None]
    assert [index[k] for k in burst_order(dates)] == case["order"]
    # equal strings keep the input order, None comes first, then bytes: 'é' (0xC3 0xA9) after 'z'
    assert burst_order(["b", None, "a", "b", "", "é", "z", None]) == [1, 7, 4, 2, 0, 3, 6, 5]


def test_burst_settings():
    assert burst_settings() == (7, 3600, 5) and burst_settings({}) == (7, 3600, 5)          # int(64 * (1 - 0.88)) = int(7.68)
    assert burst_settings({"similarity_threshold_percent": 70, "time_window_minutes": 0.8, "rapid_burst_seconds": 0.4}) == (19, 48, 0)
    assert burst_settings({"similarity_threshold_percent": 85, "time_window_minutes": 2, "rapid_burst_seconds": 3}) == (9, 120, 3)
    assert burst_settings({"similarity_threshold_percent": 90})[0] == 6                      # 64 * (1 - 0.9) = 6.3999...
    assert burst_settings({"similarity_threshold_percent": 100})[0] == 0 and burst_settings({"similarity_threshold_percent": 0})[0] == 64
    assert burst_settings({"similarity_threshold_percent": 110})[0] == -6                    # int() truncates towards zero
    assert burst_settings({"time_window_minutes": 123 / 60})[1] == 122 and 123 / 60 * 60 < 123  # 122.99999999999999: 123 s apart is outside
    assert burst_settings({"rapid_burst_seconds": -0.5})[2] == -1                            # d <= -0.5 never holds, nor does d <= -1
    for case in golden_cases().values():                                                     # the settings every golden case ran under
        percent, minutes, rapid = bursts_ref._settings(case["settings"])
        thr, window_s, rapid_s = burst_settings(case["settings"])
        assert thr == int(64 * (1 - percent / 100))
        for d in range(0, 4000):
            assert (d <= minutes * 60) == (d <= window_s) and (d <= rapid) == (d <= rapid_s)


MALFORMED = [None, "", 0, 5, b"2021:03:04 10:00:00", "2021:03:04 10:00:00", "2021:03:04 10:00:00+02:00", "2021:03:04 10:00:00.50", "2021:03:04 10:00:00Z",
             "2021:03:04 10:00:0", "2021:03:04 10:00", "2021:3:4 1:2:3", "2021:03:04 9:59:50", "2021:03:04  9:59:50", " 2021:03:04 10:00:00",
             "2021-03-04 10:00:00", "2021:03:04T10:00:00", "2021:03:04 10:00:0x", "2021:03:04 10:00:61", "2021:03:04 10:00:60", "2021:03:04 24:00:00",
             "2021:03:04 23:60:00", "2021:13:04 10:00:00", "2021:00:04 10:00:00", "2021:02:29 10:00:00", "2020:02:29 10:00:00", "2021:02:30 10:00:00",
             "2021:04:31 10:00:00", "0000:00:00 00:00:00", "0000:01:01 00:00:00", "0001:01:01 00:00:00", "9999:12:31 23:59:59", "1900:01:01 00:00:00",
             "    :  :     :  :  ", "2021:03:04 10:00:00 trailing words", "２０２１:03:04 10:00:00", "2021:03:04 10:00:0٣", "+021:03:04 10:00:00",
             "2021:03:04 10:00:-1", "20 1:03:04 10:00:00", "2021:03:04\t10:00:00", "2021:03:04 10:00:00\n", "2021:03:04 10:00:0\n", "not a date"]


def reference_parse(s):
    if not s:
        return None
    try:
        return datetime.strptime(s[:19], "%Y:%m:%d %H:%M:%S")
    except (ValueError, TypeError):
        return None


def test_parse_date_equals_strptime_on_malformed_dates():
    epoch = datetime(1, 1, 1)
    parsed = 0
    dates = MALFORMED + [r[0] for case in golden_cases().values() for r in case["table"]]
    for s in dates:
        want = reference_parse(s)
        got = parse_date(s)
        if want is None:
            assert got is None, s
        else:
            parsed += 1
            assert isinstance(got, int) and got - parse_date("0001:01:01 00:00:00") == int((want - epoch).total_seconds()), s
    assert parsed >= 100 and parse_date("9999:12:31 23:59:59") - parse_date("0001:01:01 00:00:00") > 2 ** 38


def test_hashes_must_fit_64_bits():
    with pytest.raises(ValueError):
        burst_rows(["1" + "0" * 16], ["2021:03:04 10:00:00"])
    with pytest.raises(ValueError):
        burst_rows(["-1"], ["2021:03:04 10:00:00"])
    with pytest.raises(ValueError):
        burst_rows(["xyz"], ["2021:03:04 10:00:00"])
    hashes, times, flags, off, ids = burst_rows(["ffffffffffffffff", "", "0"], ["2021:03:04 10:00:00", None, "x"], [[5, 3, 5, None], None, ["a"]])
    assert hashes.tolist() == [2 ** 64 - 1, 0, 0] and flags.tolist() == [3, 0, 1]
    assert off.tolist() == [0, 2, 2, 3] and ids.tolist() == [0, 1, 2]
