"""JPEG files for the decoder tests (test_jpeg_decode_host.py, test_jpeg_decode_gpu.py), made with Pillow at test time, and what
Pillow decodes them to: `ImageOps.exif_transpose(Image.open(f)).convert('RGB')`, the reference's load_image_from_path recipe."""
import functools
import io

import numpy as np
from PIL import Image, ImageOps

SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (33, 17), (53, 37), (48, 64)]      # (h, w)
SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
CONTENTS = ["constant", "gradient", "noise", "sparse", "bands"]
QUALITIES = [30, 75, 95, 100]


def content(kind, h, w, seed=0):
    rng = np.random.default_rng(seed * 1000 + h * 131 + w)
    if kind == "constant":
        return np.broadcast_to(np.array([200, 90, 30], np.uint8), (h, w, 3)).copy()
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], -1).astype(np.uint8)
        a[h // 4:h // 2 + 1, w // 3:w // 2 + 1] = (255, 0, 128)      # a hard-edged patch
        return a
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "sparse":      # one bright pixel per 16 x 16 tile: long zero runs, EOB / ZRL
        a = np.full((h, w, 3), 16, np.uint8)
        a[5::16, 7::16] = 255
        return a
    if kind == "bands":       # noise with saturated bands: the IDCT overshoots 0 .. 255
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        a[:, w // 4:w // 2] = 255
        a[h // 2:h // 2 + max(h // 4, 1), :] = 0
        return a
    raise ValueError(kind)


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_pixels(blob):
    """The reference's pixels, or None where it gives up on the file."""
    try:
        im = Image.open(io.BytesIO(blob))
        im = ImageOps.exif_transpose(im)
        return np.asarray(im.convert("RGB"))
    except Exception:
        return None


def exif_bytes(orientation, big_endian=False):
    ex = Image.Exif()
    ex[0x0112] = orientation
    b = ex.tobytes()
    if big_endian:      # the same one-entry IFD written by hand in Motorola order
        b = b"Exif\0\0MM\0\x2a\0\0\0\x08\0\x01\x01\x12\0\x03\0\0\0\x01" + bytes([0, orientation]) + b"\0\0\0\0\0\0"
    return b


@functools.lru_cache(maxsize=None)
def matrix():
    """[(name, blob)]: sizes x subsampling x contents x qualities, then the variants: optimised tables, restart intervals, grayscale."""
    out = []
    for (h, w) in SIZES:
        for sname, s in SUBSAMPLING.items():
            for kind in CONTENTS:
                for q in QUALITIES:
                    out.append((f"{h}x{w}-{sname}-{kind}-q{q}", encode(content(kind, h, w), quality=q, subsampling=s)))
    for (h, w) in SIZES:
        for sname, s in SUBSAMPLING.items():
            a = content("noise", h, w, 1)
            out.append((f"{h}x{w}-{sname}-opt-q100", encode(a, quality=100, subsampling=s, optimize=True)))
            out.append((f"{h}x{w}-{sname}-opt-q75", encode(content("gradient", h, w), quality=75, subsampling=s, optimize=True)))
            for rb in (1, 3):
                out.append((f"{h}x{w}-{sname}-rst{rb}", encode(a, quality=75, subsampling=s, restart_marker_blocks=rb)))
            out.append((f"{h}x{w}-{sname}-rstrow", encode(content("bands", h, w), quality=95, subsampling=s, restart_marker_rows=1)))
        for kind in ("gradient", "noise"):
            g = content(kind, h, w)[..., 1]
            out.append((f"{h}x{w}-gray-{kind}", encode(g, quality=75)))
            out.append((f"{h}x{w}-gray-{kind}-rst", encode(g, quality=95, restart_marker_blocks=2, optimize=True)))
    return out


def entropy_span(blob):
    """(first, last + 1) byte of the entropy-coded data of a single-scan file: behind the SOS header, up to the EOI marker."""
    i = 2
    while True:
        assert blob[i] == 0xFF
        m = blob[i + 1]
        n = (blob[i + 2] << 8) | blob[i + 3]
        if m == 0xDA:
            return i + 2 + n, len(blob) - 2
        i += 2 + n


def truncated(blob, fraction, with_eoi):
    a, b = entropy_span(blob)
    cut = a + int((b - a) * fraction)
    return blob[:cut] + (b"\xff\xd9" if with_eoi else b"")


def overwritten(blob, seed):
    a, b = entropy_span(blob)
    rng = np.random.default_rng(seed)
    x = bytearray(blob)
    for _ in range(max(1, (b - a) // 40)):
        x[int(rng.integers(a, b))] = int(rng.integers(0, 256))
    return bytes(x)


def damaged():
    """[(name, blob)]: files cut at 25 / 50 / 75 % of their entropy data (as they are, and with an EOI marker put behind the cut so that
    only the entropy decoder can notice) and files with bytes overwritten inside it."""
    out = []
    srcs = [("420", encode(content("noise", 53, 37), quality=75, subsampling=2)),
            ("444rst", encode(content("bands", 33, 17), quality=95, subsampling=0, restart_marker_blocks=3)),
            ("422opt", encode(content("gradient", 48, 64), quality=95, subsampling=1, optimize=True)),
            ("gray", encode(content("noise", 17, 33)[..., 0], quality=75))]
    for name, blob in srcs:
        for fr in (0.25, 0.5, 0.75):
            out.append((f"{name}-cut{fr}", truncated(blob, fr, False)))
            out.append((f"{name}-cut{fr}-eoi", truncated(blob, fr, True)))
        for seed in range(6):
            out.append((f"{name}-over{seed}", overwritten(blob, seed)))
    return out
