"""Photo thumbnails: what the reference stores per photo in the `thumbnail` column,

    thumb = pil_img.copy(); thumb.thumbnail((640, 640), Image.Resampling.LANCZOS); thumb.save(buf, format="JPEG", quality=80)

(utils/image_transforms.py:32-50 `generate_photo_thumbnail`; processing/scorer.py:1611-1617, :1680-1686), computed on the resident
batch by `fe_thumbnail_jpeg`: Pillow's integer box reduce, its LANCZOS resize with a fractional source box and a baseline JPEG
encoder that writes libjpeg's bytes. The geometry - which size, which reduce factors, which boxes - is decided here on the host,
exactly as Pillow's `Image.thumbnail` / `Image.resize(reducing_gap=2.0)` decide it (PIL/Image.py); `draft()` only acts on images
that come from a JPEG file and is not restated.
"""
import math
from collections import namedtuple

import numpy as np

# size: (ow, oh) of the thumbnail. factors: (fx, fy) of `Image.reduce` ((1, 1): none). reduce_box: the integer source box of the reduce
# or None. resize_box: the box of the LANCZOS resize in pixels of the (reduced) image, as Python floats. tall: the (reduced) image is
# more than 100 times taller than wide and shrinks vertically, where Image.resize runs the vertical pass first. unchanged: the image is
# already small enough and is encoded as it is.
ThumbnailPlan = namedtuple("ThumbnailPlan", "src_w src_h size factors reduce_box resize_box tall unchanged")

LANCZOS_SUPPORT = 3.0      # PIL.Image._filters_support[LANCZOS]
REDUCING_GAP = 2.0         # Image.thumbnail's default


def _thumbnail_size(w, h, size):
    """Image.thumbnail's preserve_aspect_ratio(): (x, y), or None when the image already fits."""
    x = y = math.floor(size)

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    if x >= w and y >= h:
        return None
    aspect = w / h
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def thumbnail_plan(w, h, size=640):
    """The steps of `Image.thumbnail((size, size), LANCZOS)` on a w x h image that does not come from a JPEG file."""
    w, h = int(w), int(h)
    final = _thumbnail_size(w, h, size)
    if final is None or final == (w, h):
        return ThumbnailPlan(w, h, (w, h), (1, 1), None, (0.0, 0.0, float(w), float(h)), False, True)
    box = (0, 0, w, h)
    # Image.resize(final, LANCZOS, box=None, reducing_gap=2.0)
    fx = int((box[2] - box[0]) / final[0] / REDUCING_GAP) or 1
    fy = int((box[3] - box[1]) / final[1] / REDUCING_GAP) or 1
    reduce_box = None
    cur_w, cur_h = w, h
    if fx > 1 or fy > 1:
        # Image._get_safe_box: the box grown by the pixels the filter may read
        support = LANCZOS_SUPPORT - 0.5
        sx = support * ((box[2] - box[0]) / final[0])
        sy = support * ((box[3] - box[1]) / final[1])
        reduce_box = (max(0, int(box[0] - sx)), max(0, int(box[1] - sy)), min(w, math.ceil(box[2] + sx)), min(h, math.ceil(box[3] + sy)))
        cur_w = -(-(reduce_box[2] - reduce_box[0]) // fx)
        cur_h = -(-(reduce_box[3] - reduce_box[1]) // fy)
        box = ((box[0] - reduce_box[0]) / fx, (box[1] - reduce_box[1]) / fy, (box[2] - reduce_box[0]) / fx, (box[3] - reduce_box[1]) / fy)
    tall = cur_h > cur_w * 100 and final[1] < cur_h
    return ThumbnailPlan(w, h, final, (fx, fy), reduce_box, tuple(float(v) for v in box), tall, False)


def thumbnails(engine, images, size=640, quality=80, bgr=False):
    """uint8 [n,h,w,3] images (host array, or the `(ptr, n, h, w)` tuple of a resident batch; bgr=True when its bytes are B,G,R) ->
    list of bytes, the reference's generate_photo_thumbnail(pil_img, size, quality) of every image."""
    if isinstance(images, tuple):
        _, _, h, w = images
    else:
        images = np.ascontiguousarray(images, dtype=np.uint8)
        _, h, w, _ = images.shape
    return engine.thumbnail_jpeg(images, thumbnail_plan(w, h, size), quality=quality, bgr=bgr)


def generate_photo_thumbnail(engine, pil_img, size=640, quality=80):
    """The reference's signature plus the engine: PIL image -> JPEG bytes. Modes other than RGB are converted first, which the
    reference does when it loads a photo."""
    rgb = np.asarray(pil_img if pil_img.mode == "RGB" else pil_img.convert("RGB"), dtype=np.uint8)
    return thumbnails(engine, rgb[None], size=size, quality=quality)[0]
