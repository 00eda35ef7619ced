"""Generates tests/golden/thumbnail_golden.npz: what the reference's own `generate_photo_thumbnail` (utils/image_transforms.py:32-50;
its imports are lazy and need only Pillow) returns for seeded synthetic images.

Inputs are not stored: tests regenerate them from (kind, seed, h, w) - `synth_image` is tests/test_phash_host.py's, `noise` is
numpy's default_rng(seed).integers(0, 256). The JPEG bytes are stored for the small cases; for the two 1024 x 1024 cases (9600
blocks per thumbnail) only the length and the SHA-256, noise at 640 x 640 encodes to hundreds of KB.

    python tests/golden/make_thumbnail_golden.py <path to a checkout of the reference>      (or FACET_REFERENCE=<path>)
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from test_phash_host import synth_image  # noqa: E402

# name, kind, seed, h, w, size, quality, bytes stored
CASES = [
    ("136x200_s48", "synth", 21, 136, 200, 48, 80, True),        # plain resize, no reduce
    ("700x1000_s160", "synth", 22, 700, 1000, 160, 80, True),    # 3 x 3 reduce, fractional resize box
    ("37x53_s640", "synth", 23, 37, 53, 640, 80, True),          # already small enough: encoded as it is
    ("300x90_s64_q85", "synth", 24, 300, 90, 64, 85, True),      # portrait, factors (1, 2), another quality
    ("1024x1024_noise", "noise", 25, 1024, 1024, 640, 80, False),
    ("1024x1024_photo", "synth", 26, 1024, 1024, 640, 80, False),
]


def make_image(kind, seed, h, w):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return synth_image(seed, h, w)


def reference_function(root):
    spec = importlib.util.spec_from_file_location("ref_image_transforms", os.path.join(root, "utils", "image_transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.generate_photo_thumbnail


def generate(fn):
    from PIL import Image
    out = {"names": np.array([c[0] for c in CASES]), "kinds": np.array([c[1] for c in CASES]),
           "meta": np.array([[c[2], c[3], c[4], c[5], c[6], int(c[7])] for c in CASES], np.int64)}
    lengths, digests, in_sha1 = [], [], []
    for name, kind, seed, h, w, size, quality, stored in CASES:
        rgb = make_image(kind, seed, h, w)
        data = fn(Image.fromarray(rgb), size=size, quality=quality)
        lengths.append(len(data))
        digests.append(hashlib.sha256(data).hexdigest())
        in_sha1.append(hashlib.sha1(rgb.tobytes()).hexdigest())
        if stored:
            out["jpeg_" + name] = np.frombuffer(data, np.uint8)
    out["lengths"] = np.array(lengths, np.int64)
    out["sha256"] = np.array(digests)
    out["input_sha1"] = np.array(in_sha1)
    return out


if __name__ == "__main__":
    import PIL
    from PIL import features
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FACET_REFERENCE")
    if not root:
        sys.exit(__doc__)
    g = generate(reference_function(root))
    path = os.path.join(HERE, "thumbnail_golden.npz")
    np.savez_compressed(path, **g)
    print(f"Pillow {PIL.__version__}, libjpeg-turbo {features.version('libjpeg_turbo')}: {path}, {os.path.getsize(path)} bytes")
    for n, l in zip(g["names"], g["lengths"]):
        print(f"  {n}: {l} bytes")
