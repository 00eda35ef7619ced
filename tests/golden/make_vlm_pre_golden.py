"""Golden vectors for the VLM tagger's image preprocessing (fe_vlm_preprocess_rgb) from transformers' own Qwen2-VL image processor.

models/vlm_tagger.py hands PIL images to `processor(text=..., images=..., padding=True)` (:245-259, :346-360); its image half is
Qwen2VLImageProcessor, which without torchvision is Qwen2VLImageProcessorPil: convert to RGB, smart_resize to multiples of 28, PIL bicubic
resample, rescale by 1/255, normalise by the CLIP mean / std, patchify into rows of 3 x 2 x 14 x 14. This script runs that class on six
seeded images - the round-to-28 path, the min_pixels upscale, the max_pixels downscale (a small max_pixels), a portrait image, an RGBA and
an L-mode image - and stores the input images (uint8, with their PIL mode), each case's max_pixels, pixel_values and image_grid_thw.
Run in the build container:
    python tests/golden/make_vlm_pre_golden.py
"""
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vlm_pre_golden.npz")
MAX_DEFAULT = 28 * 28 * 1280
# (name, height, width, mode, max_pixels)
CASES = [("round28", 100, 130, "RGB", MAX_DEFAULT), ("min_up", 30, 40, "RGB", MAX_DEFAULT), ("max_down", 200, 170, "RGB", 28 * 28 * 12),
         ("portrait", 120, 60, "RGB", MAX_DEFAULT), ("rgba", 64, 90, "RGBA", MAX_DEFAULT), ("gray", 70, 50, "L", MAX_DEFAULT)]


def image(seed, h, w, mode):
    """A smooth field plus noise (the bicubic taps see both), uint8."""
    rng = np.random.default_rng(seed)
    ch = {"RGB": 3, "RGBA": 4, "L": 1}[mode]
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = np.stack([np.sin(3 * xx + k) * np.cos(2 * yy - k) for k in range(ch)], -1) * 100 + 128
    a = np.clip(base + rng.normal(0, 30, (h, w, ch)), 0, 255).astype(np.uint8)
    return a[..., 0] if ch == 1 else a


def main():
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil
    out = {"names": np.array([c[0] for c in CASES]), "modes": np.array([c[3] for c in CASES]),
           "max_pixels": np.array([c[4] for c in CASES], np.int64), "min_pixels": np.int64(56 * 56)}
    for i, (name, h, w, mode, mx) in enumerate(CASES):
        a = image(100 + i, h, w, mode)
        proc = Qwen2VLImageProcessorPil(min_pixels=56 * 56, max_pixels=mx)
        r = proc(images=[Image.fromarray(a, mode)], return_tensors="np")
        out[f"image_{i}"] = a
        out[f"pixel_values_{i}"] = np.asarray(r["pixel_values"], np.float32)
        out[f"grid_thw_{i}"] = np.asarray(r["image_grid_thw"], np.int32)
        print(name, a.shape, mode, "->", out[f"grid_thw_{i}"].tolist(), out[f"pixel_values_{i}"].shape)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
