"""CPU: the Qwen3-VL tagger's host arithmetic against tests/golden/vlm3_golden.npz (transformers' Qwen3VLForConditionalGeneration and
Qwen2VLImageProcessorPil with 16-pixel patches, tests/golden/make_vlm3_golden.py): the tower's index arrays (vision_inputs_qwen3), the
processor's size choice at factor 32, the decoder-input M-RoPE position ids (rope_index), VLMTagger(qwen3).prepare_inputs on the photo
batch, and the interleaved frequency -> position-component map against a numpy restatement of apply_interleaved_mrope."""
import os

import numpy as np
from facet_amd.vlm_tagger import (VLMTagger, interleaved_mrope_components, rope_index, smart_resize, vision_inputs_qwen3, MIN_PIXELS_QWEN3,
                                  MAX_PIXELS_QWEN3, QWEN3_VL_2B, IMAGE_MEAN_QWEN3, IMAGE_STD_QWEN3)

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "vlm3_golden.npz"))
IMG = int(G["image_token_id"])


def test_vision_inputs_equal_transformers_vision_utils():
    v = vision_inputs_qwen3(G["vis_grid_thw"], 8)
    assert np.array_equal(v["patch_pos_hw"], G["vis_patch_pos_hw"])
    assert np.array_equal(v["interp_idx"], G["vis_interp_idx"])
    assert v["interp_w"].dtype == np.float32 and np.array_equal(v["interp_w"], G["vis_interp_w"])
    assert np.array_equal(v["cu_seqlens"], G["vis_cu_seqlens"])


def test_interpolation_weights_sum_to_one_and_hit_the_corners():
    v = vision_inputs_qwen3([[1, 30, 48]], 48)
    assert np.allclose(v["interp_w"].sum(1), 1.0, atol=1e-6)
    # align_corners=True: the first and last patch take exactly the first and last table row
    first = np.flatnonzero((v["patch_pos_hw"] == [0, 0]).all(1))[0]
    last = np.flatnonzero((v["patch_pos_hw"] == [29, 47]).all(1))[0]
    assert v["interp_w"][first].max() == 1.0 and v["interp_idx"][first][np.argmax(v["interp_w"][first])] == 0
    assert v["interp_idx"][last][np.argmax(v["interp_w"][last])] == 48 * 48 - 1


def test_smart_resize_factor_32_and_the_reference_max_pixels():
    assert (MIN_PIXELS_QWEN3, MAX_PIXELS_QWEN3) == (65536, 512 * 28 * 28)
    assert smart_resize(900, 1400, 32, MIN_PIXELS_QWEN3, MAX_PIXELS_QWEN3) == (480, 768)      # grid [1, 30, 48]
    for (oh, ow), g in zip([smart_resize(a.shape[0], a.shape[1], 32, int(G["photo_min_pixels"]), int(G["photo_max_pixels"]))
                            for a in (G[f"photo_{i}"] for i in range(3))], G["photo_grid_thw"]):
        assert (oh // 16, ow // 16) == (int(g[1]), int(g[2]))


def test_rope_index_equals_the_decoder_input_positions():
    pos, _ = rope_index(G["input_ids"], G["vis_grid_thw"], IMG)
    assert np.array_equal(pos, G["position_ids"])
    pos, _ = rope_index(G["batch_input_ids"], G["batch_grid_thw"], IMG, attention_mask=G["batch_attention_mask"])
    assert np.array_equal(pos, G["batch_position_ids"])


def test_prepare_inputs_equals_the_processor_batch():
    from standins import vlm_tokenizer as T
    from PIL import Image
    tg = VLMTagger({"model_path": "Qwen/Qwen3-VL-2B-Instruct", "min_pixels": int(G["photo_min_pixels"]), "max_pixels": int(G["photo_max_pixels"])},
                   encode=T.encode, decode=T.decode, special_tokens=T.TOKENS)
    assert tg.family == "qwen3" and tg.batch_size == 4
    photos = [G[f"photo_{i}"] for i in range(3)]
    x = tg.prepare_inputs([Image.fromarray(a, "RGBA" if a.shape[2] == 4 else "RGB") for a in photos])
    assert np.array_equal(x["grid_thw"], G["photo_grid_thw"])
    assert np.array_equal(x["input_ids"], G["photo_input_ids"])
    assert np.array_equal(x["attention_mask"], G["photo_attention_mask"])
    assert np.array_equal(x["position_ids"], G["photo_position_ids"])
    assert x["image_rows"].size == int((G["photo_grid_thw"].prod(1) // 4).sum())


def test_interleaved_section_map_equals_transformers():
    """interleaved_mrope_components (the rule vlm3_qk_rope_cache_kernel applies per frequency lane) against the map transformers' own
    apply_interleaved_mrope produced for the golden's sections; the kernel itself is pinned by the GPU logit tests."""
    assert np.array_equal(interleaved_mrope_components(tuple(int(v) for v in G["mrope_section"])), G["mrope_component_map"])


def test_qwen3_defaults():
    assert QWEN3_VL_2B["mrope_section"] == (24, 20, 20) and QWEN3_VL_2B["n_heads"] // QWEN3_VL_2B["n_kv_heads"] == 2
    assert IMAGE_MEAN_QWEN3 == IMAGE_STD_QWEN3 == (0.5, 0.5, 0.5)
