"""Generates tests/golden/phash_golden.npz: `imagehash.phash(image)` (hash_size 8, highfreq_factor 4) restated stage by stage with
PIL + scipy - imagehash itself is not installed, so parity with the package is unpinned; its source is four lines:

    image = image.convert('L').resize((32, 32), Image.Resampling.LANCZOS)
    dct = scipy.fftpack.dct(scipy.fftpack.dct(numpy.asarray(image), axis=0), axis=1)
    lo = dct[:8, :8];  bits = lo > numpy.median(lo)            # str(): the row-major bits as a binary number, 16 hex digits

on seeded photo-like images made up HERE (low-frequency sinusoids per channel plus noise, numpy only). Recorded per image: the
32x32 `small`, the 8x8 `lo`, the hash and the smallest |lo - median|. Inputs up to 200 x 300 are stored; the larger ones are
regenerated in the tests from (seed, h, w) by `synth_image`, which tests/test_phash_host.py / test_phash_gpu.py repeat (their
sha1 is stored, so a generator that drifted is told apart from a wrong kernel).

The tie band: a bit whose coefficient lies within TIE_BAND = 1e-6 of the median is decided by the rounding of the DCT routine
(the reference's own bit follows pocketfft's butterflies; a direct fp64 sum of 1024 terms of magnitude <= 5.3e5 differs from it
by about 3e-11). This script asserts that NO recorded image except the two constant ones has a bit inside the band, so the
tests compare whole hashes.

    python tests/golden/make_phash_golden.py
"""
import hashlib
import os

import numpy as np
import scipy.fftpack
from PIL import Image

TIE_BAND = 1e-6
# (name, seed, h, w, stored)
CASES = [(f"{h}x{w}_s{seed}", seed, h, w, True)
         for (h, w) in ((32, 32), (32, 100), (100, 32), (20, 17), (31, 47), (97, 131), (33, 500)) for seed in (11, 12)]
CASES += [("200x300_s13", 13, 200, 300, True)]
CASES += [(f"{h}x{w}_s{seed}", seed, h, w, False)
          for (h, w), seeds in (((512, 512), (21, 22)), ((768, 1024), (23, 24)), ((1024, 683), (25, 26)), ((1024, 1024), (27, 28)),
                                ((2000, 3000), (29,))) for seed in seeds]
BATCH257 = (97, 131, 1000)          # h, w, first seed: 257 images, hashes only


def synth_image(seed, h, w):
    """Seeded photo-like RGB image: four low-frequency sinusoids per channel plus Gaussian noise."""
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


def phash_stages(rgb):
    """-> (small uint8 [32,32], lo float64 [8,8], hash int, margin float)."""
    small = np.asarray(Image.fromarray(rgb, "RGB").convert("L").resize((32, 32), Image.Resampling.LANCZOS))
    dct = scipy.fftpack.dct(scipy.fftpack.dct(small, axis=0), axis=1)
    lo = dct[:8, :8]
    med = np.median(lo)
    bits = (lo > med).flatten()
    return small, lo.astype(np.float64), int("".join(str(int(b)) for b in bits), 2), float(np.abs(lo - med).min())


def main():
    out = {"tie_band": np.float64(TIE_BAND)}
    names, meta, small, lo, hashes, margins, sha = [], [], [], [], [], [], []

    def record(name, seed, h, w, stored, rgb, constant):
        s, l, hv, m = phash_stages(rgb)
        assert constant or m > TIE_BAND, (name, m)
        names.append(name); meta.append((seed, h, w, int(stored), int(constant)))
        small.append(s); lo.append(l); hashes.append(hv); margins.append(m); sha.append(hashlib.sha1(rgb.tobytes()).hexdigest())
        if stored:
            out["img_" + name] = rgb
        print(f"{name:>18}  {hv:016x}  margin {m:.4g}")

    for name, seed, h, w, stored in CASES:
        record(name, seed, h, w, stored, synth_image(seed, h, w), False)
    record("black_64x48", 0, 64, 48, True, np.zeros((64, 48, 3), np.uint8), True)
    const = np.empty((50, 70, 3), np.uint8)
    const[...] = (200, 100, 50)
    record("const_50x70", 0, 50, 70, True, const, True)
    h, w, s0 = BATCH257
    b = [phash_stages(synth_image(s0 + i, h, w)) for i in range(257)]
    assert min(x[3] for x in b) > TIE_BAND
    out.update(names=np.array(names), meta=np.array(meta, np.int64), small=np.stack(small), lo=np.stack(lo),
               hashes=np.array(hashes, np.uint64), margins=np.array(margins), sha1=np.array(sha),
               batch257=np.array(BATCH257, np.int64), batch257_hashes=np.array([x[2] for x in b], np.uint64))
    print("smallest margin of a non-constant image:", min(m for m, mt in zip(margins, meta) if not mt[4]), "| batch of 257:", min(x[3] for x in b))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "phash_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
