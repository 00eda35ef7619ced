"""CPU: the host side of the perceptual-hash / duplicate-detection feature.

* tests/golden/phash_golden.npz reproduces from PIL (gray + two-pass LANCZOS) and, where scipy is importable, from
  scipy.fftpack.dct - the restatement of `imagehash.phash` that tests/golden/make_phash_golden.py documents (imagehash itself is
  not installed: parity with the package is unpinned).
* facet_amd.phash.to_hex / from_hex, facet_amd.duplicates.max_hamming_distance / group_duplicates against
  tests/golden/duplicates_golden.json, which holds what the reference's own `detect_duplicates` wrote for made-up rows. The
  pairs come from a brute-force numpy search inside this file (the package has no host pair search on purpose)."""
import hashlib
import json
import os

import numpy as np
import pytest

from facet_amd.duplicates import group_duplicates, max_hamming_distance
from facet_amd.phash import from_hex, to_hex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIE_BAND = 1e-6


def synth_image(seed, h, w):
    """tests/golden/make_phash_golden.py::synth_image, repeated."""
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, 1.0, h)[:, None]
    x = np.linspace(0.0, 1.0, w)[None, :]
    img = np.empty((h, w, 3), np.float64)
    for c in range(3):
        acc = np.full((h, w), 128.0 + rng.uniform(-30.0, 30.0))
        for _ in range(4):
            fy, fx = rng.uniform(0.3, 3.5, 2)
            ph = rng.uniform(0.0, 2.0 * np.pi)
            amp = rng.uniform(15.0, 45.0)
            acc = acc + amp * np.sin(2.0 * np.pi * (fy * y + fx * x) + ph)
        img[..., c] = acc + rng.normal(0.0, 6.0, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def golden_images(g, only_stored=False):
    """(index, name, rgb, constant) for every recorded image; the large ones are regenerated from their seed."""
    for i, name in enumerate(g["names"].tolist()):
        seed, h, w, stored, constant = (int(v) for v in g["meta"][i])
        if stored:
            rgb = g["img_" + name]
        elif only_stored:
            continue
        else:
            rgb = synth_image(seed, h, w)
            assert hashlib.sha1(rgb.tobytes()).hexdigest() == str(g["sha1"][i]), f"{name}: the seeded generator gives other pixels than at golden time"
        yield i, name, rgb, bool(constant)


def hamming_pairs_bruteforce(hashes, maxd):
    """Every i < j with popcount(h[i] ^ h[j]) <= maxd, ascending (i, j): int32 [k,2]."""
    h = np.asarray(hashes, np.uint64)
    out = []
    for i in range(len(h) - 1):
        x = np.bitwise_xor(h[i], h[i + 1:])
        d = np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)
        js = np.nonzero(d <= maxd)[0] + i + 1
        out.append(np.stack([np.full(js.shape, i), js], axis=1))
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 2), np.int32)


def test_golden_small_and_gray_reproduce_from_pil():
    from PIL import Image
    g = np.load(os.path.join(GOLDEN, "phash_golden.npz"))
    assert float(g["tie_band"]) == TIE_BAND
    for i, name, rgb, _ in golden_images(g):
        im = Image.fromarray(rgb, "RGB").convert("L")
        r, gg, b = (rgb[..., k].astype(np.int64) for k in range(3))
        assert np.array_equal(np.asarray(im), ((r * 19595 + gg * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)), name
        small = np.asarray(im.resize((32, 32), Image.Resampling.LANCZOS))
        assert np.array_equal(small, g["small"][i]), name


def test_golden_dct_and_hash_reproduce_from_a_direct_sum():
    """lo from a direct fp64 sum over the recorded 32x32 image; the hash from lo. No recorded non-constant image has a bit inside
    the tie band, so this route must give the recorded hash too."""
    g = np.load(os.path.join(GOLDEN, "phash_golden.npz"))
    n = np.arange(32)
    cosv = np.cos(np.pi * np.arange(8)[:, None] * (2 * n[None, :] + 1) / 64.0)
    meta = g["meta"]
    for i, name in enumerate(g["names"].tolist()):
        small = g["small"][i].astype(np.float64)
        lo = 4.0 * cosv @ small @ cosv.T
        assert np.abs(lo - g["lo"][i]).max() < TIE_BAND, name
        med = np.median(g["lo"][i])
        assert float(np.abs(g["lo"][i] - med).min()) == float(g["margins"][i])
        if not meta[i][4]:
            assert g["margins"][i] > TIE_BAND
            bits = (lo > np.median(lo)).flatten()
            assert int("".join(str(int(b)) for b in bits), 2) == int(g["hashes"][i]), name
    assert int(g["hashes"][g["names"].tolist().index("black_64x48")]) == 0
    assert g["batch257_hashes"].shape == (257,)


def test_golden_dct_reproduces_from_scipy():
    """The recorded lo is scipy.fftpack.dct over axis 0, then axis 1, of the recorded 32x32 image (skipped where scipy is absent)."""
    fftpack = pytest.importorskip("scipy.fftpack", reason="scipy is not importable: the scipy route of the golden is not re-run")
    g = np.load(os.path.join(GOLDEN, "phash_golden.npz"))
    for i, name in enumerate(g["names"].tolist()):
        d = fftpack.dct(fftpack.dct(g["small"][i], axis=0), axis=1)[:8, :8]
        assert np.array_equal(d, g["lo"][i]), name


def test_hex_round_trip():
    v = np.array([0, 1, 0x00000000ffffffff, 0x8000000000000000, 0xffffffffffffffff, 0x0123456789abcdef, 0x000f000000000000], np.uint64)
    s = to_hex(v)
    assert s == ["0000000000000000", "0000000000000001", "00000000ffffffff", "8000000000000000", "ffffffffffffffff", "0123456789abcdef",
                 "000f000000000000"]
    assert all(len(x) == 16 and x == x.lower() for x in s)
    back = from_hex(s)
    assert back.dtype == np.uint64 and np.array_equal(back, v)
    assert np.array_equal(from_hex(["F", "00ff"]), np.array([15, 255], np.uint64))       # what int(s, 16) accepts
    g = np.load(os.path.join(GOLDEN, "phash_golden.npz"))
    assert to_hex(g["hashes"])[g["names"].tolist().index("const_50x70")] == "8000000000000000"


def test_max_hamming_distance_matches_what_the_reference_printed():
    gold = json.load(open(os.path.join(GOLDEN, "duplicates_golden.json")))
    assert gold["max_distance"] == {"100": 0, "95": 3, "90": 6, "80": 12}
    for pct, d in gold["max_distance"].items():
        assert max_hamming_distance(int(pct)) == d
    assert max_hamming_distance(90) == 6 and max_hamming_distance(95) == 3 and max_hamming_distance(90.0) == 6


def test_group_duplicates_equals_the_reference_on_every_case():
    gold = json.load(open(os.path.join(GOLDEN, "duplicates_golden.json")))
    assert len(gold["cases"]) == 16
    for case in gold["cases"]:
        keep = [i for i, h in enumerate(case["phash"]) if h is not None]           # the reference's WHERE phash IS NOT NULL
        hashes = from_hex([case["phash"][i] for i in keep])
        pairs = hamming_pairs_bruteforce(hashes, max_hamming_distance(case["similarity"]))
        gid, lead = group_duplicates(len(keep), pairs, [case["aggregate"][i] for i in keep])
        want_gid, want_lead = [case["group_id"][i] for i in keep], [case["is_lead"][i] for i in keep]
        assert gid == want_gid and lead == want_lead, (case["name"], case["similarity"])
        for i, h in enumerate(case["phash"]):                                     # rows without a hash stay unmarked there too
            if h is None:
                assert case["group_id"][i] is None and case["is_lead"][i] == 0
    # no pairs: nothing is marked
    gid, lead = group_duplicates(3, np.zeros((0, 2), np.int32), [1.0, None, 2.0])
    assert gid == [None, None, None] and lead == [0, 0, 0]
