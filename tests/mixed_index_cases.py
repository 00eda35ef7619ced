"""The images of the mixed-size pHash and thumbnail tests (host and GPU): tests/mixed_cases.py's shapes plus ten that reach the
remaining paths of `thumbnail_plan` and of the pHash tables.

At size 64 the plans cover: unchanged (33 x 47, 32 x 32, 31 x 33); resize only; reduce on one axis and on both with column, row and
corner remainders (300 x 260 -> factors (2, 2); 40 x 400 -> (3, 3); 48 x 1100 -> (8, 8); 257 x 255 -> (1, 2); 2000 x 10 -> (5, 15);
13 x 997 -> (7, 6)); outputs of one pixel on an axis (64 x 1, 1 x 64, 64 x 3); 64 x 96 and 80 x 80 twice, not as neighbours. At size 640,
2000 x 10 is the `tall` plan (3 x 640) and 48 x 1100 gives 640 x 28. test_thumb_mixed_host.py asserts all of this. For pHash, 32 x 32,
32 x 100 and 100 x 32 have the identity table on one or both axes, and the three images with a one-pixel side tie with their median."""
import struct

import numpy as np
from PIL import Image

from mixed_cases import SHAPES, images

EXTRA = [(32, 32), (32, 100), (100, 32), (31, 33), (257, 255), (2000, 10), (13, 997), (1, 1), (1, 50), (50, 1)]
ALL_SHAPES = list(SHAPES) + EXTRA      # (h, w)


def all_images():
    return images(shapes=ALL_SHAPES)


# The list of the chunking tests: eleven images of about 200 KB, which an engine with a 1 MiB arena cannot take at once. From the host
# fe_phash_mixed has room for 985 856 bytes beside its 60 672-byte pool and an image needs its staged pixels (to 256 bytes) plus 32 h +
# 1608 with both extra outputs: 207 208, 207 176, 188 232, 207 208, 54 856 (864 680; the next, 206 376, would pass the room), then five
# more (914 408), then one - chunks of 5, 5, 1; resident there is nothing to stage and one chunk takes all. fe_thumbnail_jpeg_mixed at
# size 64 has a budget of 7/8 MiB less its 42 700-byte pool and an image needs two rows of fe_jpeg_bound(64, 64) = 40 561 bytes, its
# staged pixels and its scratch, 160 833 (128 x 128) to 431 681 bytes (255 x 257) in all - chunks of 2, 3, 2, 2, 2, and 5, 5, 1 resident.
# tests/test_mixed_list_host.py asserts the counts.
CHUNK_SHAPES = [(257, 256), (256, 257), (200, 300), (257, 256), (128, 128), (255, 257), (240, 250), (257, 256), (100, 333), (256, 256), (257, 255)]
CHUNK_ARENA = 1 << 20


def chunk_images():
    return images(seed=19, shapes=CHUNK_SHAPES)


def pil_thumbnail_pixels(a, size):
    """uint8 [oh, ow, 3]: `Image.fromarray(a).copy().thumbnail((size, size), LANCZOS)`."""
    im = Image.fromarray(a).copy()
    im.thumbnail((size, size), Image.Resampling.LANCZOS)
    return np.asarray(im, dtype=np.uint8)


def write_harness_input(path, arrs, plans):
    """tests/native/thumb_mixed_harness.cpp's input: fe_thumb_plan's fields behind every image's size, then its pixels."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(arrs)))
        for a, p in zip(arrs, plans):
            rb = p.reduce_box if p.reduce_box is not None else (0, 0, 0, 0)
            f.write(struct.pack("<10i", a.shape[0], a.shape[1], p.size[1], p.size[0], p.factors[0], p.factors[1], *rb))
            f.write(np.asarray(p.resize_box, dtype="<f4").tobytes())
            f.write(struct.pack("<i", 1 if p.tall else 0))
            f.write(np.ascontiguousarray(a).tobytes())


def expected_tables(plans):
    """The distinct (input size, box start, box end, output size) of every pass the plans run: what the pool must hold."""
    keys = set()
    for p in plans:
        if p.unchanged:
            continue
        rw, rh = p.src_w, p.src_h
        if p.reduce_box is not None:
            rw = -(-(p.reduce_box[2] - p.reduce_box[0]) // p.factors[0])
            rh = -(-(p.reduce_box[3] - p.reduce_box[1]) // p.factors[1])
        b = [float(np.float32(v)) for v in p.resize_box]
        ow, oh = p.size
        if ow != rw or b[0] != 0.0 or b[2] != float(rw):
            keys.add((rw, b[0], b[2], ow))
        if oh != rh or b[1] != 0.0 or b[3] != float(rh):
            keys.add((rh, b[1], b[3], oh))
    return keys
