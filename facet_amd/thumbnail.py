"""Photo thumbnails: what the reference stores per photo in the `thumbnail` column,

    thumb = pil_img.copy(); thumb.thumbnail((640, 640), Image.Resampling.LANCZOS); thumb.save(buf, format="JPEG", quality=80)

(utils/image_transforms.py:32-50 `generate_photo_thumbnail`; processing/scorer.py:1611-1617, :1680-1686), computed on the resident
batch by `fe_thumbnail_jpeg`: Pillow's integer box reduce, its LANCZOS resize with a fractional source box and a baseline JPEG
encoder that writes libjpeg's bytes. The geometry - which size, which reduce factors, which boxes - is decided here on the host,
exactly as Pillow's `Image.thumbnail` / `Image.resize(reducing_gap=2.0)` decide it (PIL/Image.py). `draft()` only acts on images
that come from a JPEG file, which a resident batch does not: `thumbnail_plan` leaves it out, `thumbnail_plan_jpeg` restates it.

Stored thumbnails made smaller, which is the case where the image does come from a JPEG file: the reference's viewer export
(db/maintenance.py:182-272 `export_viewer_db`, both loops) and its thumbnail route (api/routers/thumbnails.py:54-64 `_resize_thumbnail`) run

    img = Image.open(BytesIO(blob)); img.thumbnail((size, size), Image.LANCZOS); img.save(buf, format='JPEG', quality=80)

and there `Image.thumbnail` first calls `JpegImageFile.draft()`, which makes libjpeg decode at 1/2, 1/4 or 1/8 size. `fe_jpeg_thumbnail`
chains that scaled decode with reduce, resize and encode on the device; `resize_thumbnail`, `resize_thumbnails` and `downsize_thumbnails`
are the reference's functions on top of it, with every file the GPU path does not take sent through the Pillow recipe above.
"""
import io
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


def _unchanged_plan(w, h):
    return ThumbnailPlan(w, h, (w, h), (1, 1), None, (0.0, 0.0, float(w), float(h)), False, True)


def thumbnail_plan(w, h, size=640):
    """The steps of `Image.thumbnail((size, size), LANCZOS)` on a w x h image that does not come from a JPEG file."""
    w, h = int(w), int(h)
    final = _thumbnail_size(w, h, size)
    if final is None or final == (w, h):
        return _unchanged_plan(w, h)
    return _resize_plan(w, h, final, (0, 0, w, h))


def _resize_plan(w, h, final, box):
    """Image.resize(final, LANCZOS, box=box, reducing_gap=2.0) on a w x h image whose size is not `final`."""
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


def draft_scale(w, h, size):
    """The scale `JpegImageFile.draft(None, (int(size * 2.0), int(size * 2.0)))` chooses for a w x h file: 8, 4, 2 or 1."""
    req = int(size * REDUCING_GAP)
    scale = min(w // req, h // req)
    for s in (8, 4, 2, 1):
        if scale >= s:
            return s
    return 1


def thumbnail_plan_jpeg(w, h, size):
    """The steps of `Image.thumbnail((size, size), LANCZOS)` on a w x h image that comes from a JPEG file -> (scale, ThumbnailPlan).
    scale: what draft() makes libjpeg decode at; the plan is stated on that ceil(w / scale) x ceil(h / scale) image. The final size comes
    from the file's own size; draft() hands resize() the fractional box (0, 0, w / scale, h / scale), which goes into the reduce factors,
    the safe box and the resize box; an image whose scaled size is already the final size is not resized at all; one that already fits is
    not even drafted."""
    w, h = int(w), int(h)
    final = _thumbnail_size(w, h, size)
    if final is None:
        return 1, _unchanged_plan(w, h)
    scale = draft_scale(w, h, size)
    sw, sh = -(-w // scale), -(-h // scale)
    if (sw, sh) == final:                                      # Image.thumbnail's `self.size != final_size`
        return scale, _unchanged_plan(sw, sh)
    # Image.resize's early `return self.copy()` needs size == final, which the test above has just excluded: the resize always runs
    return scale, _resize_plan(sw, sh, final, (0, 0, w / scale, h / scale))


def thumbnails(engine, images, size=640, quality=80, bgr=False):
    """uint8 [n,h,w,3] images (host array, or the `(ptr, n, h, w)` tuple of a resident batch; bgr=True when its bytes are B,G,R) ->
    list of bytes, the reference's generate_photo_thumbnail(pil_img, size, quality) of every image."""
    if isinstance(images, tuple):
        _, _, h, w = images
    else:
        images = np.ascontiguousarray(images, dtype=np.uint8)
        _, h, w, _ = images.shape
    return engine.thumbnail_jpeg(images, thumbnail_plan(w, h, size), quality=quality, bgr=bgr)


def thumbnails_mixed(engine, images, size=640, quality=80, order='rgb'):
    """Images that each have their own size (a list of uint8 [h,w,3] arrays, or `(device_pointers, sizes)` for resident images; order:
    'rgb' or 'bgr' bytes) -> list of bytes, the reference's generate_photo_thumbnail(pil_img, size, quality) of every image, from one
    `fe_thumbnail_jpeg_mixed` call with one `thumbnail_plan` per image."""
    sizes = images[1] if isinstance(images, tuple) else [np.asarray(a).shape[:2] for a in images]
    return engine.thumbnail_jpeg_mixed(images, [thumbnail_plan(w, h, size) for h, w in sizes], quality=quality, order=order)


def generate_photo_thumbnail(engine, pil_img, size=640, quality=80):
    """The reference's signature plus the engine: PIL image -> JPEG bytes. Modes other than RGB are converted first, which the
    reference does when it loads a photo."""
    rgb = np.asarray(pil_img if pil_img.mode == "RGB" else pil_img.convert("RGB"), dtype=np.uint8)
    return thumbnails(engine, rgb[None], size=size, quality=quality)[0]


# ---- stored JPEG thumbnails made smaller ------------------------------------------------------------------------------------------
def pillow_resize_thumbnail(blob, size, quality=80):
    """The reference's recipe on one file: Image.open, thumbnail((size, size), LANCZOS), save JPEG. Raises what Pillow raises."""
    from PIL import Image
    img = Image.open(io.BytesIO(blob))
    img.thumbnail((size, size), Image.LANCZOS)
    buf = io.BytesIO()
    img.save(buf, format='JPEG', quality=quality)
    return buf.getvalue()


def _has_comment(blob):
    """A COM segment in front of the first scan: Pillow's save carries it over from im.info, the device encoder writes none."""
    i, n = 2, len(blob)
    while i + 4 <= n and blob[i] == 0xFF:
        m = blob[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xFE:
            return True
        if m == 0xDA or m == 0xD9:
            return False
        i += 2 + ((blob[i + 2] << 8) | blob[i + 3])
    return False


def _probe(engine, blob, progressive):
    info = engine.jpeg_probe(blob)
    if progressive and info['status'] == 1:
        info = engine.jpeg_probe(blob, progressive=True)
    return info


def resize_thumbnails(engine, blobs, size, quality=80, progressive=False, parallel_entropy=False):
    """JPEG files (bytes) -> list of bytes in input order: `Image.open(f)`, `thumbnail((size, size), LANCZOS)`, `save(buf, "JPEG",
    quality=quality)` of each, byte for byte, None where Pillow raises. Three-component files the decoder takes are grouped by source
    size and go through fe_jpeg_thumbnail; everything else - grayscale (Pillow keeps mode L and writes a one-component file), CMYK,
    progressive files without progressive=True, files with a comment segment (Pillow copies it), corrupt files - goes through that same
    Pillow recipe, so the bytes never depend on which side did the work. Unlike resize_thumbnail, a file that already fits is encoded
    again, as Pillow's three calls would. parallel_entropy: Engine.jpeg_thumbnail's, for the files the engine takes; the bytes are the same."""
    blobs = [bytes(b) for b in blobs]
    out = [None] * len(blobs)
    groups, rest = {}, []
    for i, b in enumerate(blobs):
        info = _probe(engine, b, progressive)
        if info['status'] != 0 or info['components'] != 3 or _has_comment(b):
            rest.append(i)
        else:
            groups.setdefault((info['width'], info['height']), []).append(i)
    for (w, h), idx in groups.items():
        scale, plan = thumbnail_plan_jpeg(w, h, size)
        flag = dict(parallel_entropy=True) if parallel_entropy else {}
        rows, status = engine.jpeg_thumbnail([blobs[i] for i in idx], scale, plan, quality=quality, progressive=progressive, **flag)
        for k, i in enumerate(idx):
            if status[k] == 0:
                out[i] = rows[k]
            else:
                rest.append(i)                                 # rare: a stream only the entropy decoder finds corrupt
    for i in rest:
        try:
            out[i] = pillow_resize_thumbnail(blobs[i], size, quality)
        except Exception:
            out[i] = None
    return out


def _jpeg_size(engine, blob):
    """(w, h) as `Image.open(blob).size` gives it: from the probe, and from Pillow where the probe read no frame header."""
    info = engine.jpeg_probe(blob)
    if info['width'] > 0 and info['height'] > 0 and info['status'] >= 0:
        return info['width'], info['height']
    from PIL import Image
    return Image.open(io.BytesIO(blob)).size


def resize_thumbnail(engine, thumbnail_bytes, size, parallel_entropy=False):
    """The reference's `_resize_thumbnail(thumbnail_bytes, size)` (api/routers/thumbnails.py:54-64) plus the engine: the same bytes
    object when the image is already small enough, else its JPEG at quality 80 with the longer side `size`. Raises where Pillow raises."""
    if max(_jpeg_size(engine, thumbnail_bytes)) <= size:
        return thumbnail_bytes
    got = resize_thumbnails(engine, [thumbnail_bytes], size, parallel_entropy=parallel_entropy)[0]
    return got if got is not None else pillow_resize_thumbnail(thumbnail_bytes, size)      # raises Pillow's error


def downsize_thumbnails(engine, rows, thumbnail_size=320, parallel_entropy=False):
    """The body of both loops of the reference's export_viewer_db (db/maintenance.py:182-272) without the database: rows = (key, blob)
    pairs -> yields (new_bytes, key), in input order, for the rows whose image is larger than thumbnail_size; a None blob and a row
    Pillow cannot read are skipped silently."""
    todo = []
    for key, blob in rows:
        if blob is None:
            continue
        try:
            if max(_jpeg_size(engine, bytes(blob))) > thumbnail_size:
                todo.append((key, bytes(blob)))
        except Exception:
            pass      # skip corrupt thumbnails
    for (key, _), new in zip(todo, resize_thumbnails(engine, [b for _, b in todo], thumbnail_size, parallel_entropy=parallel_entropy)):
        if new is not None:
            yield new, key
