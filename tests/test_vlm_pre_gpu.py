"""GPU: the VLM tagger's image preprocessing (fe_vlm_preprocess_rgb) and the vision tower fed from it (fe_vlm_encode_preprocessed).

tests/golden/make_vlm_pre_golden.py ran transformers' Qwen2-VL image processor (PIL backend) on six images - round to 28, min_pixels
upscale, max_pixels downscale, portrait, RGBA, L mode. The GPU's pixel_values must be bit-identical to it (and to the live processor
when transformers imports), and the vision tower on the rows left on the device must give exactly the embeddings of fe_vlm_encode_images
on the processor's fp32 rows (the patch embedding converts both to the same bf16).
"""
import os

import numpy as np
import pytest
from PIL import Image

from facet_amd._lib import FE_MODEL_VLM
from facet_amd.vlm_tagger import smart_resize, to_rgb, vision_indices, IMAGE_MEAN, IMAGE_STD
from facet_amd.weights import synthetic_state_dict, VLM_TINY

pytestmark = pytest.mark.gpu
P = np.load(os.path.join(os.path.dirname(__file__), "golden", "vlm_pre_golden.npz"))
N = len(P["names"])


@pytest.fixture(scope="module")
def vlm():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=4 << 30)
    e.vlm_configure(n_heads=VLM_TINY["heads"], n_kv_heads=VLM_TINY["kv_heads"], head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24))
    e.vlm_vision_configure(2, [1])
    e.load_weights(FE_MODEL_VLM, synthetic_state_dict("qwen2_5_vl_tiny", 16))
    yield e
    e.close()


def _case(i):
    rgb = to_rgb(Image.fromarray(P[f"image_{i}"], str(P["modes"][i])))
    return rgb, smart_resize(rgb.shape[0], rgb.shape[1], 28, int(P["min_pixels"]), int(P["max_pixels"][i]))


@pytest.mark.parametrize("i", range(N))
def test_pixel_values_bit_identical_to_the_processor(vlm, i):
    rgb, size = _case(i)
    g = P[f"grid_thw_{i}"][0]
    assert (size[0] // 14, size[1] // 14) == (g[1], g[2])
    pv = vlm.vlm_preprocess_rgb([rgb], [size], IMAGE_MEAN, IMAGE_STD, want_pixel_values=True)
    want = P[f"pixel_values_{i}"]
    assert pv.shape == want.shape
    assert np.array_equal(pv.view(np.uint32), want.view(np.uint32)), f"{P['names'][i]}: {int((pv != want).sum())} values differ"


def test_images_of_different_sizes_in_one_call(vlm):
    cases = [_case(i) for i in range(N)]
    pv = vlm.vlm_preprocess_rgb([c[0] for c in cases], [c[1] for c in cases], IMAGE_MEAN, IMAGE_STD, want_pixel_values=True)
    want = np.concatenate([P[f"pixel_values_{i}"] for i in range(N)])
    assert np.array_equal(pv.view(np.uint32), want.view(np.uint32))


def test_pixel_values_against_the_live_processor_when_importable(vlm):
    try:
        from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil
    except Exception:
        return          # the golden above pins the same values
    rng = np.random.default_rng(44)
    imgs = [Image.fromarray(rng.integers(0, 256, (97, 211, 3), dtype=np.uint8)), Image.fromarray(rng.integers(0, 256, (300, 41), dtype=np.uint8), "L")]
    r = Qwen2VLImageProcessorPil()(images=imgs, return_tensors="np")
    rgb = [to_rgb(im) for im in imgs]
    pv = vlm.vlm_preprocess_rgb(rgb, [smart_resize(a.shape[0], a.shape[1]) for a in rgb], IMAGE_MEAN, IMAGE_STD, want_pixel_values=True)
    assert np.array_equal(pv.view(np.uint32), np.asarray(r["pixel_values"], np.float32).view(np.uint32))


def test_encode_preprocessed_equals_encode_images_on_the_processor_rows(vlm):
    cases = [_case(i) for i in range(N)]
    grid = np.concatenate([P[f"grid_thw_{i}"] for i in range(N)])
    idx = vision_indices(grid)
    args = (idx["patch_pos_hw"], idx["window_index"], idx["cu_window_seqlens"], idx["cu_seqlens"])
    ref = vlm.vlm_encode_images(np.concatenate([P[f"pixel_values_{i}"] for i in range(N)]), *args)
    vlm.vlm_preprocess_rgb([c[0] for c in cases], [c[1] for c in cases], IMAGE_MEAN, IMAGE_STD)
    got = vlm.vlm_encode_preprocessed(*args)
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
