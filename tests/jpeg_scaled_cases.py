"""JPEG files for the scaled-decode tests (test_jpeg_scaled_host.py, test_jpeg_scaled_gpu.py), made with jpeg_cases' helpers at test
time, and what Pillow decodes them to after `JpegImageFile.draft()` chose a scale: libjpeg's 1/2, 1/4 and 1/8 decode."""
import functools
import io

import numpy as np
from PIL import Image, ImageOps

import jpeg_cases as J

# partial MCUs, planes narrower than 3 samples (where fancy upsampling switches off) and ceil rounding of the output size all occur here
SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (17, 33), (53, 37), (97, 131)]      # (h, w)
SCALES = [2, 4, 8]
CONTENTS = ["noise", "gradient", "sparse"]
QUALITIES = [30, 95]
SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "gray"]


def drafted(blob, scale, transpose=False):
    """Pillow's image of the file decoded at 1/scale: draft() with the requested size that makes it choose exactly that scale."""
    im = Image.open(io.BytesIO(blob))
    w, h = im.size
    if scale > 1:
        im.draft(None, (max(w // scale, 1), max(h // scale, 1)))
        got = im.decoderconfig[0] if im.decoderconfig else 1
        if got != scale:      # images smaller than the scale: draft() would settle for less, so set what it sets
            im.decoderconfig = (scale, 0)
            im._size = ((w + scale - 1) // scale, (h + scale - 1) // scale)
            im.tile = [im.tile[0]._replace(extents=(0, 0) + im.size)]
    if transpose:
        im = ImageOps.exif_transpose(im)
    return im


def pillow_scaled(blob, scale, transpose=False):
    return np.asarray(drafted(blob, scale, transpose).convert("RGB"))


def file_of(h, w, sname, kind, q, rst, progressive=False):
    a = J.content(kind, h, w)
    kw = dict(quality=q)
    if rst:
        kw["restart_marker_blocks"] = 2
    if progressive:
        kw["progressive"] = True
    if sname == "gray":
        return J.encode(a[..., 1], **kw)
    return J.encode(a, subsampling=J.SUBSAMPLING[sname], **kw)


@functools.lru_cache(maxsize=None)
def files():
    """[(name, blob)]: sizes x samplings x contents x qualities x with / without restart markers."""
    return [(f"{h}x{w}-{s}-{k}-q{q}{'-rst' if r else ''}", file_of(h, w, s, k, q, r))
            for (h, w) in SIZES for s in SAMPLINGS for k in CONTENTS for q in QUALITIES for r in (False, True)]


@functools.lru_cache(maxsize=None)
def progressive_files():
    """The progressive subset: every size and sampling, noise at quality 95, with restart markers on the odd sizes."""
    return [(f"{h}x{w}-{s}-prog", file_of(h, w, s, "noise", 95, (h * w) % 2 == 1, progressive=True)) for (h, w) in SIZES for s in SAMPLINGS]


def scaled_size(h, w, scale):
    return -(-h // scale), -(-w // scale)
