"""JPEG files for the tests of the parallel entropy decode (test_jpeg_parallel_host.py, test_jpeg_parallel_gpu.py), made with jpeg_cases'
helpers at test time: each is the smallest file at which one mechanism of the self-synchronising decoder can fail. SUB is the device's
subsequence size; the host harness sweeps others."""
import functools

import numpy as np

import jpeg_cases as J

SUB = 128
STUFFED_SEED = 95       # found by stuffed_seed_search(); stuffed_file() asserts what it was searched for


def photo(h, w, seed=0):
    """Photo-like content: smooth colour fields, a few hard edges and fine texture of varying strength, so that blocks differ in length."""
    rng = np.random.default_rng(seed * 7919 + h * 131 + w)
    gh, gw = h // 24 + 2, w // 24 + 2
    coarse = rng.integers(0, 256, (gh, gw, 3)).astype(np.float64)
    y, x = np.linspace(0, gh - 1.001, h), np.linspace(0, gw - 1.001, w)
    y0, x0 = y.astype(int), x.astype(int)
    fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
    a = (coarse[y0][:, x0] * (1 - fy) * (1 - fx) + coarse[y0 + 1][:, x0] * fy * (1 - fx) + coarse[y0][:, x0 + 1] * (1 - fy) * fx +
         coarse[y0 + 1][:, x0 + 1] * fy * fx)
    strength = np.abs(np.sin(np.arange(w) / 17.0))[None, :, None] * 10
    a = a + rng.normal(0, 1, (h, w, 3)) * strength
    a[h // 5:h // 3, w // 4:w // 2] = (250, 250, 245)
    a[h // 2:h // 2 + 3, :] = 10
    return np.clip(a, 0, 255).astype(np.uint8)


def segments(blob):
    """[(first, last + 1)] of the entropy-coded segments of a single-scan file: its entropy data cut at the restart markers."""
    a, b = J.entropy_span(blob)
    out, start, i = [], a, a
    while i < b - 1:
        if blob[i] == 0xFF and 0xD0 <= blob[i + 1] <= 0xD7:
            out.append((start, i))
            start = i = i + 2
        else:
            i += 2 if blob[i] == 0xFF else 1
    out.append((start, b))
    return out


def expected_stats(blobs, sub=SUB):
    """(segments that take the parallel path, their subsequences) over baseline files: a segment of at least two subsequences does."""
    counts = [-(-(e - s) // sub) for blob in blobs for s, e in segments(blob)]
    return sum(1 for c in counts if c >= 2), sum(c for c in counts if c >= 2)


def _stuffed_cuts(blob, sub=SUB):
    """Residues mod sub (from the segment's start) of the 0xFF bytes of a file without restart markers."""
    a, b = J.entropy_span(blob)
    return {(i - a) % sub for i in range(a, b - 1) if blob[i] == 0xFF and blob[i + 1] == 0x00}


def _stuffed_candidate(seed):
    return J.encode(J.content("noise", 64, 64, seed), quality=97, subsampling=0)


def stuffed_seed_search(limit=2000):
    for seed in range(limit):
        r = _stuffed_cuts(_stuffed_candidate(seed))
        if SUB - 1 in r and 0 in r:
            return seed
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def stuffed_file():
    """Noise whose entropy data has an FF 00 pair at an offset = SUB - 1 (mod SUB): a cut lands on the stuffed zero; and one at an
    offset = 0: a subsequence begins with the 0xFF."""
    blob = _stuffed_candidate(STUFFED_SEED)
    r = _stuffed_cuts(blob)
    assert SUB - 1 in r and 0 in r
    return blob


def single_block():
    return [("8x8-gray", J.encode(J.content("noise", 8, 8)[..., 0], quality=75)), ("16x16-420", J.encode(J.content("gradient", 16, 16), quality=75, subsampling=2))]


def long_blocks():
    return [("64x64-noise-q100-444-opt", J.encode(J.content("noise", 64, 64, 3), quality=100, subsampling=0, optimize=True))]


def flat():
    return [("256x256-constant-q30-420", J.encode(J.content("constant", 256, 256), quality=30, subsampling=2)),
            ("256x256-gradient-q30-420", J.encode(J.content("gradient", 256, 256), quality=30, subsampling=2))]


@functools.lru_cache(maxsize=None)
def photo_matrix():
    """203 x 157 at quality 80 in every sampling: no restart markers; one restart interval per MCU row (segments of a few subsequences);
    one every 3 MCUs (all segments shorter than a subsequence)."""
    a = photo(203, 157, 1)
    out = []
    for sname in ("4:4:4", "4:2:2", "4:2:0", "gray"):
        src, kw = (a[..., 1], {}) if sname == "gray" else (a, dict(subsampling=J.SUBSAMPLING[sname]))
        out.append((f"photo-{sname}", J.encode(src, quality=80, **kw)))
        out.append((f"photo-{sname}-rstrow", J.encode(src, quality=80, restart_marker_rows=1, **kw)))
        out.append((f"photo-{sname}-rst3", J.encode(src, quality=80, restart_marker_blocks=3, **kw)))
    return out


def gpu_cases():
    """[(name, blob)]: the honest files of test_jpeg_parallel_gpu.py, which the host harness decodes first."""
    return single_block() + long_blocks() + flat() + list(photo_matrix()) + [("stuffed", stuffed_file())]


def with_extra_bytes(blob, n, seed=0):
    """blob with n bytes that are no marker put in front of its EOI: data behind the last MCU, which a decoder ignores."""
    assert blob[-2:] == b"\xff\xd9"
    rng = np.random.default_rng(seed * 1000 + n)
    return blob[:-2] + bytes(int(v) for v in rng.integers(0, 255, n)) + b"\xff\xd9"


EXTRA = [1, 2, 3, 15, 16, 17, 127, 128, 129, 255, 256, 300]


def extra_byte_files():
    srcs = [("420", J.encode(J.content("noise", 53, 37), quality=75, subsampling=2)), ("gray-flat", J.encode(J.content("constant", 64, 64)[..., 0], quality=30)),
            ("444rstrow", J.encode(J.content("bands", 33, 17), quality=95, subsampling=0, restart_marker_rows=1))]
    return [(f"{name}-extra{n}", with_extra_bytes(blob, n, k)) for k, (name, blob) in enumerate(srcs) for n in EXTRA]


def random_small(count=200, seed=2024):
    """[(name, blob)]: seeded random small images over every encoder setting the decoder distinguishes."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        h, w = int(rng.integers(8, 97)), int(rng.integers(8, 97))
        kind = J.CONTENTS[int(rng.integers(0, len(J.CONTENTS)))] if rng.random() < 0.6 else "photo"
        a = photo(h, w, k) if kind == "photo" else J.content(kind, h, w, k)
        kw = dict(quality=int(rng.integers(5, 101)), optimize=bool(rng.integers(0, 2)))
        sampling = int(rng.integers(0, 4))
        if sampling == 3:
            a = a[..., 0]
        else:
            kw["subsampling"] = sampling
        rst = int(rng.integers(0, 4))
        if rst == 1:
            kw["restart_marker_rows"] = int(rng.integers(1, 4))
        elif rst == 2:
            kw["restart_marker_blocks"] = int(rng.integers(1, 40))
        out.append((f"rand{k}-{h}x{w}-{kind}-s{sampling}-q{kw['quality']}-o{int(kw['optimize'])}-r{rst}", J.encode(a, **kw)))
    return out


def thumbnail_sources():
    """Four stored thumbnails as the product writes them (`save("JPEG", quality=80)`, no restart markers): 640 x 427 and 427 x 640."""
    return [J.encode(photo(427, 640, 11), quality=80), J.encode(photo(427, 640, 12), quality=80),
            J.encode(photo(640, 427, 13), quality=80), J.encode(photo(640, 427, 14), quality=80)]
