"""Progressive JPEG files for test_jpeg_progressive_host.py and test_jpeg_progressive_gpu.py, made with Pillow at test time
(`Image.save(progressive=True)`: libjpeg's default script, 10 scans for colour and 6 for gray, a fresh DHT in front of every Huffman scan).
What they must decode to is jpeg_cases.pillow_pixels, as for the baseline files."""
import functools

import numpy as np

import jpeg_cases as J

QUALITIES = [30, 95]
SMALL = [(3, 2), (5, 3), (2, 4), (9, 5), (4, 6), (1, 17), (19, 1)]      # chroma 1 .. 3 samples wide, as in the baseline host test


def encode(arr, **kw):
    return J.encode(arr, progressive=True, **kw)


@functools.lru_cache(maxsize=None)
def matrix():
    """[(name, blob)]: sizes x subsampling x contents x qualities, grayscale, restart intervals (in blocks and in rows: the interval then
    differs between the interleaved and the one-component scans), the small widths, and one file with more than 64 segments in a scan."""
    out = []
    for (h, w) in J.SIZES:
        for sname, s in J.SUBSAMPLING.items():
            for kind in J.CONTENTS:
                for q in QUALITIES:
                    out.append((f"{h}x{w}-{sname}-{kind}-q{q}", encode(J.content(kind, h, w), quality=q, subsampling=s)))
            a = J.content("noise", h, w, 1)
            for rb in (1, 3):
                out.append((f"{h}x{w}-{sname}-rst{rb}", encode(a, quality=75, subsampling=s, restart_marker_blocks=rb)))
            out.append((f"{h}x{w}-{sname}-rstrow", encode(J.content("bands", h, w), quality=95, subsampling=s, restart_marker_rows=1)))
        for kind in ("gradient", "noise"):
            out.append((f"{h}x{w}-gray-{kind}", encode(J.content(kind, h, w)[..., 1], quality=75)))
    for (h, w) in SMALL:
        for sname, s in J.SUBSAMPLING.items():
            out.append((f"{h}x{w}-{sname}-small", encode(J.content("noise", h, w, 2), quality=90, subsampling=s)))
    out.append(("72x88-4:4:4-rst1", encode(J.content("noise", 72, 88, 4), quality=75, subsampling=0, restart_marker_blocks=1)))      # 99 segments
    return out


MATRIX_SIZE = 8 * (3 * (5 * 2 + 3) + 2) + 7 * 3 + 1


def oriented():
    """All eight orientations on one 20 x 30 image."""
    a = J.content("gradient", 20, 30)
    return [encode(a, quality=90, subsampling=(0, 2)[o % 2], exif=J.exif_bytes(o, o > 4)) for o in range(1, 9)]


@functools.lru_cache(maxsize=None)
def long_eobrun():
    """1024 x 1024 constant gray: every AC scan is one end-of-band run over all 16384 blocks, the 14-bit form."""
    return encode(np.full((1024, 1024), 77, np.uint8), quality=75)


def scans(blob):
    """[(tables, first, last + 1)] per scan, in file order: where the marker segments in front of its SOS begin (the DHT / DRI written for
    it), and its entropy-coded bytes."""
    out, i, tables = [], 2, None
    while i < len(blob):
        assert blob[i] == 0xFF
        m = blob[i + 1]
        if m == 0xD9:
            break
        n = (blob[i + 2] << 8) | blob[i + 3]
        if m != 0xDA:
            if tables is None and out:      # the first segment behind the previous scan
                tables = i
            i += 2 + n
            continue
        a = j = i + 2 + n
        while not (blob[j] == 0xFF and blob[j + 1] != 0 and not 0xD0 <= blob[j + 1] <= 0xD7):
            j += 1
        out.append((tables if tables is not None else i, a, j))
        tables, i = None, j
    return out


def cut_before_scan(blob, k):
    """The file up to the tables of scan k (0-based), closed with EOI: scans 0 .. k - 1 are whole, the progression stops short."""
    return blob[:scans(blob)[k][0]] + b"\xff\xd9"


def truncated(blob, scan, fraction, with_eoi):
    """jpeg_cases.truncated inside the entropy data of scan `scan` (1-based)."""
    _, a, b = scans(blob)[scan - 1]
    return blob[:a + int((b - a) * fraction)] + (b"\xff\xd9" if with_eoi else b"")


def overwritten(blob, scan, seed):
    """jpeg_cases.overwritten inside the entropy data of scan `scan` (1-based)."""
    _, a, b = scans(blob)[scan - 1]
    rng = np.random.default_rng(seed)
    x = bytearray(blob)
    for _ in range(max(1, (b - a) // 40)):
        x[int(rng.integers(a, b))] = int(rng.integers(0, 256))
    return bytes(x)


DAMAGED_SOURCES = {"420": (53, 37), "444rst": (33, 17), "422rstrow": (48, 64)}      # name: (h, w)


@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, blob)]: three files cut at 25 / 50 / 75 % of the entropy data of scans 1, 2, 6 and 10 (as they are, and with an EOI marker
    behind the cut) and with bytes overwritten inside it."""
    srcs = [("420", encode(J.content("noise", 53, 37), quality=75, subsampling=2)),
            ("444rst", encode(J.content("bands", 33, 17), quality=95, subsampling=0, restart_marker_blocks=3)),
            ("422rstrow", encode(J.content("gradient", 48, 64), quality=95, subsampling=1, restart_marker_rows=1))]
    out = []
    for name, blob in srcs:
        assert len(scans(blob)) == 10
        for sc in (1, 2, 6, 10):
            for fr in (0.25, 0.5, 0.75):
                out.append((f"{name}-s{sc}-cut{fr}", truncated(blob, sc, fr, False)))
                out.append((f"{name}-s{sc}-cut{fr}-eoi", truncated(blob, sc, fr, True)))
            for seed in range(6):
                out.append((f"{name}-s{sc}-over{seed}", overwritten(blob, sc, seed)))
    return out
