"""Images of mixed sizes for the mixed-size tests (host and GPU), and Pillow's own 224 x 224 crops of them.

Shapes (h, w), the smallest at which the geometry can go wrong: 33 x 47 odd and enlarged on both axes (filter scale clamped to 1);
64 x 96 and 96 x 64 the same pixel count transposed; 80 x 80; 300 x 260 reduced on both axes; 40 x 400 (CLIP resizes to 224 x 2240, the
centre crop lies far from the edge); 224 x 224 (no SAMP pass runs: the crop-only path); 48 x 1100 (long edge over 1024: TOPIQ's LANCZOS
cap). 64 x 96 and 80 x 80 appear twice, so their groups have members that are not neighbours in the list."""
import numpy as np
from PIL import Image

SHAPES = [(33, 47), (64, 96), (96, 64), (80, 80), (300, 260), (40, 400), (224, 224), (48, 1100), (64, 96), (80, 80)]
CLIP, SAMP = 0, 1

# The list of the statistics chunking test: with a 1 MiB arena the 184 320-byte hue-saturation histogram of every image (plus 3 184 bytes
# of accumulators and record, its gray plane and, from the host, its pixels) lets five of these into a chunk (the first five take about
# 1 044 000 bytes from the host; a sixth histogram would pass 1 048 576) - chunks of 5, 5, 1, resident too.
# tests/test_mixed_list_host.py asserts the counts.
STATS_CHUNK_SHAPES = [(96, 64), (64, 96), (80, 80), (96, 64), (33, 47), (100, 60), (96, 64), (64, 96), (1, 7), (96, 65), (80, 80)]
CHUNK_ARENA = 1 << 20


def images(seed=7, shapes=SHAPES):
    """Smooth structure plus noise, so that neither the filters nor the models see a flat field."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w) in enumerate(shapes):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        base = np.stack([127 + 100 * np.sin(xx / (5.0 + k) + c) * np.cos(yy / (7.0 + c)) for c in range(3)], axis=-1)
        out.append(np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def pillow_crop(img, mode):
    """uint8 [224, 224, 3]: _clip_pre / _samp_pre of tests/test_ensemble_gpu.py before their float conversion."""
    if mode == SAMP:
        return np.asarray(Image.fromarray(img).resize((224, 224), Image.BILINEAR), dtype=np.uint8)
    h, w = img.shape[:2]
    ow, oh = (224, int(224 * h / w)) if w <= h else (int(224 * w / h), 224)
    pil = Image.fromarray(img).resize((ow, oh), Image.BICUBIC)
    top, left = int(round((oh - 224) / 2.0)), int(round((ow - 224) / 2.0))
    return np.asarray(pil.crop((left, top, left + 224, top + 224)), dtype=np.uint8)
