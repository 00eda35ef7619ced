"""fe_phash / fe_hamming_pairs on the GPU against tests/golden/phash_golden.npz (PIL + scipy restatement of imagehash.phash, made
by tests/golden/make_phash_golden.py) and tests/golden/duplicates_golden.json (the reference's own detect_duplicates).

Stage by stage: the 32x32 gray image must equal PIL's byte for byte for every size (row starts at every byte offset: widths 17,
47, 131, 683; skipped passes: 32 x 100, 100 x 32, 32 x 32; upscaling: 20 x 17, 31 x 47; 193 and 565 taps: 1024, 3000), the 8x8 DCT
block within 1e-6, the hashes as 16-digit strings. The tie band (a coefficient within 1e-6 of the median is decided by the DCT
routine's rounding) is empty for every non-constant recorded image - the generator asserts it - so whole hashes are compared.
The pair search must return exactly the brute-force list, order included."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from facet_amd.batch import BatchScorer
from facet_amd.duplicates import find_duplicates, max_hamming_distance
from facet_amd.phash import from_hex, phash_batch, to_hex
from test_phash_host import GOLDEN, TIE_BAND, golden_images, hamming_pairs_bruteforce, synth_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "phash_golden.npz"))


def test_every_stage_equals_the_golden_for_every_size(engine, gold):
    want_hex = to_hex(gold["hashes"])
    for i, name, rgb, constant in golden_images(gold):
        hashes, small, lo = engine.phash(rgb[None], want_small=True, want_dct=True)
        assert small.shape == (1, 32, 32) and lo.shape == (1, 8, 8)
        diff = int(np.abs(small[0].astype(int) - gold["small"][i].astype(int)).max())
        err = float(np.abs(lo[0] - gold["lo"][i]).max())
        print(f"[phash] {name:>18}: small max diff {diff}, lo max err {err:.3e}, margin {float(gold['margins'][i]):.4g}, {to_hex(hashes)[0]}")
        assert np.array_equal(small[0], gold["small"][i]), name
        if name.startswith("black"):
            assert int(hashes[0]) == 0 and np.all(lo[0] == 0.0)
        elif constant:                     # every coefficient but DC is rounding noise around the median: only the DC bit is defined
            assert int(hashes[0]) >> 63 == 1, name
            assert abs(lo[0, 0, 0] - gold["lo"][i][0, 0]) < TIE_BAND
        else:
            assert err < TIE_BAND, (name, err)
            assert to_hex(hashes)[0] == want_hex[i], name
        assert np.array_equal(engine.phash(rgb[None]), hashes)                       # the plain call: hashes only


def test_bgr_and_device_resident_input_give_the_same_hashes(engine, gold):
    names = gold["names"].tolist()
    for h, w, seeds in ((97, 131, (11, 12)), (33, 500, (11, 12)), (1024, 683, (25, 26)), (20, 17, (11, 12))):
        idx = [names.index(f"{h}x{w}_s{s}") for s in seeds]
        rgb = np.stack([synth_image(s, h, w) for s in seeds])
        want = gold["hashes"][idx]
        assert np.array_equal(engine.phash(rgb), want)
        assert np.array_equal(engine.phash(np.ascontiguousarray(rgb[..., ::-1]), bgr=True), want)
        assert phash_batch(engine, rgb) == to_hex(want)
        # resident input, once at the allocation's start and once at an odd byte offset (row starts then walk through every alignment)
        for off in (0, 1, 3):
            d = engine.dev_alloc(rgb.nbytes + 16)
            try:
                p = C.c_void_p(d.value + off)
                engine.h2d(p, rgb)
                got, small, _ = engine.phash((p, len(seeds), h, w), want_small=True)
                assert np.array_equal(small, gold["small"][idx]), (h, w, off)
                assert np.array_equal(got, want), (h, w, off)
            finally:
                engine.dev_free(d)


def test_single_image_and_batch_of_257(engine, gold):
    h, w, s0 = (int(v) for v in gold["batch257"])
    imgs = np.stack([synth_image(s0 + i, h, w) for i in range(257)])
    got = engine.phash(imgs)
    assert got.dtype == np.uint64 and got.shape == (257,)
    assert to_hex(got) == to_hex(gold["batch257_hashes"])
    assert np.array_equal(engine.phash(imgs[200:201]), gold["batch257_hashes"][200:201])      # n = 1
    assert np.array_equal(engine.phash(np.ascontiguousarray(imgs[..., ::-1]), bgr=True), gold["batch257_hashes"])


def planted_hashes(rng, n):
    """Random 64-bit hashes with clusters of near copies (0..12 bits off a centre) planted at random positions."""
    h = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    for _ in range(max(0, n // 12)):
        centre = h[int(rng.integers(0, n))]
        for k in rng.integers(0, n, size=int(rng.integers(1, 5))):
            v = int(centre)
            for b in rng.choice(64, size=int(rng.integers(0, 13)), replace=False):
                v ^= 1 << int(b)
            h[k] = np.uint64(v)
    return h


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000, 5000])
def test_hamming_pairs_equal_brute_force(engine, n):
    rng = np.random.default_rng(100 + n)
    h = planted_hashes(rng, n)
    if n == 2:
        h[1] = h[0] ^ np.uint64(0b111111)             # 6 bits apart
    for maxd in (0, 6, 12):
        want = hamming_pairs_bruteforce(h, maxd)
        got = engine.hamming_pairs(h, maxd)
        print(f"[hamming] n {n} distance {maxd}: {len(want)} pairs")
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (n, maxd)
    if n >= 2:                                         # resident hashes
        d = engine.dev_alloc(h.nbytes)
        try:
            engine.h2d(d, h)
            assert np.array_equal(engine.hamming_pairs((d, n), 6), hamming_pairs_bruteforce(h, 6))
        finally:
            engine.dev_free(d)
    if n == 2:
        assert len(engine.hamming_pairs(h, 6)) == 1 and len(engine.hamming_pairs(h, 5)) == 0


def test_hamming_distance_64_is_every_pair(engine):
    h = planted_hashes(np.random.default_rng(7), 300)
    got = engine.hamming_pairs(h, 64)                  # 44850 pairs > the first attempt's room: grown once inside
    i, j = np.triu_indices(300, 1)
    assert np.array_equal(got, np.stack([i, j], axis=1).astype(np.int32))
    assert np.array_equal(engine.hamming_pairs(h, 64, max_pairs=10), got)


def test_overflow_reports_the_exact_count_and_writes_nothing_past_the_buffer(engine):
    """The guard after the host array checks the copy-out. The kernel's own `at < cap` check is pinned by the exact count: on the
    device the hit counter sits directly behind the pair buffer and a canary word behind that (fe_hamming_pairs), so a store past the
    capacity would corrupt the count this test compares, or trip the canary and fail the call."""
    h = planted_hashes(np.random.default_rng(8), 300)
    total = 300 * 299 // 2
    for room in (0, 1, 1000, total - 1):
        guard = 4096
        buf = np.full((room + guard, 2), 0x5A5A5A5A, np.int32)
        count = C.c_int64(-1)
        rc = engine.lib.fe_hamming_pairs(engine.h, h.ctypes.data_as(C.c_void_p), 300, 0, 64, room, buf.ctypes.data_as(C.c_void_p) if room else None,
                                         C.byref(count))
        assert rc == 0 and count.value == total, (room, rc, count.value)
        assert np.all(buf[room:] == 0x5A5A5A5A), room
    buf = np.full((total + 64, 2), 0x5A5A5A5A, np.int32)      # exactly enough room: filled, sorted, guard untouched
    count = C.c_int64(-1)
    assert engine.lib.fe_hamming_pairs(engine.h, h.ctypes.data_as(C.c_void_p), 300, 0, 64, total, buf.ctypes.data_as(C.c_void_p), C.byref(count)) == 0
    i, j = np.triu_indices(300, 1)
    assert count.value == total and np.array_equal(buf[:total], np.stack([i, j], axis=1)) and np.all(buf[total:] == 0x5A5A5A5A)
    # a sparse case: 1000 hashes at distance 6, room for fewer pairs than there are
    h = planted_hashes(np.random.default_rng(9), 1000)
    want = hamming_pairs_bruteforce(h, 6)
    assert len(want) > 8
    buf = np.full((8 + 64, 2), 0x5A5A5A5A, np.int32)
    assert engine.lib.fe_hamming_pairs(engine.h, h.ctypes.data_as(C.c_void_p), 1000, 0, 6, 8, buf.ctypes.data_as(C.c_void_p), C.byref(count)) == 0
    assert count.value == len(want) and np.all(buf[8:] == 0x5A5A5A5A)
    assert np.array_equal(engine.hamming_pairs(h, 6, max_pairs=8), want)


def test_batch_scorer_phash_column(gold):
    """BatchScorer(phash=True): the 'phash' values equal the golden, every other key and value equals the phash=False result, with
    and without a second context; the key is absent when the flag is off."""
    from facet_amd import Engine
    from facet_amd._lib import FE_MODEL_TOPIQ
    from facet_amd.weights import synthetic_state_dict
    names = gold["names"].tolist()
    idx = [names.index("512x512_s21"), names.index("512x512_s22")]
    imgs = np.stack([synth_image(21, 512, 512), synth_image(22, 512, 512)])
    want = [to_hex(gold["hashes"])[i] for i in idx]
    e, e2 = Engine(0, arena_bytes=6 << 30), Engine(0, arena_bytes=2 << 30)
    try:
        e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 4))
        for aux in (None, e2):
            off = BatchScorer(e, aux_engine=aux).process_batch(imgs)
            on = BatchScorer(e, aux_engine=aux, phash=True).process_batch(imgs)
            assert [r['phash'] for r in on] == want
            for a, b in zip(off, on):
                assert 'phash' not in a
                assert set(b) == set(a) | {'phash'}
                for k, v in a.items():
                    assert type(b[k]) is type(v) and (b[k] == v or (isinstance(v, float) and np.isnan(v) and np.isnan(b[k]))), k
        mixed = BatchScorer(e, phash=True).process_images([imgs[1], synth_image(11, 97, 131), imgs[0]])       # passes through the ragged path
        assert [r['phash'] for r in mixed] == [want[1], to_hex(gold["hashes"])[names.index("97x131_s11")], want[0]]
    finally:
        e.close()
        e2.close()


def test_find_duplicates_equals_the_reference_end_to_end(engine):
    gold = json.load(open(os.path.join(GOLDEN, "duplicates_golden.json")))
    for case in gold["cases"]:
        keep = [i for i, h in enumerate(case["phash"]) if h is not None]
        gid, lead = find_duplicates(engine, [case["phash"][i] for i in keep], [case["aggregate"][i] for i in keep], case["similarity"])
        assert gid == [case["group_id"][i] for i in keep] and lead == [case["is_lead"][i] for i in keep], (case["name"], case["similarity"])
        assert max_hamming_distance(case["similarity"]) == gold["max_distance"][str(case["similarity"])]
    assert find_duplicates(engine, [], [], 90) == ([], [])
    assert from_hex(["00000000000000ff"])[0] == 255
