"""CPU: the host half of the VLM tagger's photo path (facet_amd/vlm_tagger.py) - smart_resize, the masked rope_index, the chat text with
its placeholder expansion and left padding, and tag_batch's sub-batching and out-of-memory fallback against a fake engine."""
import math
import os

import numpy as np
import pytest

from facet_amd._lib import EngineCapacityError, EngineError, left_padding
from facet_amd.vlm_tagger import (VLMTagger, chat_text, expand_image_pads, left_pad, rope_index, smart_resize, to_rgb, IMAGE_MEAN, IMAGE_STD)
from standins import vlm_tokenizer as T

HERE = os.path.dirname(os.path.abspath(__file__))


def _hf_smart_resize():
    try:
        from transformers.models.qwen2_vl.image_processing_qwen2_vl import smart_resize as f
        return f
    except Exception:
        return None


def test_smart_resize_matches_transformers_over_a_size_sweep():
    ref = _hf_smart_resize()
    # the three paths by hand (transformers' function restated): round to 28, min_pixels upscale, max_pixels downscale
    assert smart_resize(100, 130) == (112, 140)
    assert smart_resize(30, 40) == (56, 84)
    assert smart_resize(200, 170, max_pixels=28 * 28 * 12) == (84, 84)
    sizes = [(h, w) for h in (1, 7, 28, 29, 55, 56, 100, 333, 1000, 1080, 4000) for w in (3, 28, 41, 224, 640, 1920, 3000, 6000)]
    for h, w in sizes:
        for mx in (28 * 28 * 1280, 28 * 28 * 40, 12845056):
            if max(h, w) / min(h, w) > 200:
                with pytest.raises(ValueError):
                    smart_resize(h, w, max_pixels=mx)
                if ref is not None:
                    with pytest.raises(ValueError):
                        ref(h, w, max_pixels=mx)
                continue
            got = smart_resize(h, w, max_pixels=mx)
            assert got[0] % 28 == 0 and got[1] % 28 == 0
            if ref is not None:
                assert got == tuple(ref(h, w, max_pixels=mx)), (h, w, mx)


def test_numpy_restatement_of_the_gpu_preprocessing_equals_the_golden():
    """What fe_vlm_preprocess_rgb computes (lut gather + patch order), in numpy on PIL's bicubic resample: the golden's bits."""
    from PIL import Image
    z = np.load(os.path.join(HERE, "golden", "vlm_pre_golden.npz"))
    m32, s32 = np.array(IMAGE_MEAN, np.float32), np.array(IMAGE_STD, np.float32)
    lut = np.stack([((np.arange(256) * (1 / 255)).astype(np.float32) - m32[c]) / s32[c] for c in range(3)])
    for i in range(len(z["names"])):
        rgb = to_rgb(Image.fromarray(z[f"image_{i}"], str(z["modes"][i])))
        oh, ow = smart_resize(rgb.shape[0], rgb.shape[1], 28, int(z["min_pixels"]), int(z["max_pixels"][i]))
        v = lut[np.arange(3), np.asarray(Image.fromarray(rgb).resize((ow, oh), Image.BICUBIC))]
        gh, gw = oh // 14, ow // 14
        p = v.transpose(2, 0, 1).reshape(3, gh // 2, 2, 14, gw // 2, 2, 14).transpose(1, 4, 2, 5, 0, 3, 6)
        p = np.broadcast_to(p[:, :, :, :, :, None], p.shape[:5] + (2, 14, 14)).reshape(gh * gw, 1176)
        assert np.array_equal(p.view(np.uint32), z[f"pixel_values_{i}"].view(np.uint32)), z["names"][i]


def test_masked_rope_index_equals_the_golden_positions():
    z = np.load(os.path.join(HERE, "golden", "vlm_ragged_golden.npz"))
    pos, nxt = rope_index(z["input_ids"], z["grid_thw"], int(z["image_token_id"]), attention_mask=z["attention_mask"])
    assert np.array_equal(pos, z["position_ids"])
    am = z["attention_mask"].astype(bool)
    for b in range(pos.shape[1]):
        assert nxt[b] == pos[:, b, am[b]].max() + 1
        assert (pos[:, b, ~am[b]] == 0).all()
    # without a mask: unchanged, and a row's positions do not depend on its padding
    p0, n0 = rope_index(z["input_ids"][:1], z["grid_thw"][:1], int(z["image_token_id"]))
    assert np.array_equal(p0, pos[:, :1]) and n0[0] == nxt[0]


def test_chat_text_expansion_left_padding_and_image_rows():
    t = VLMTagger({"model_path": "Qwen/Qwen2.5-VL-7B-Instruct"}, encode=T.encode, decode=T.decode, special_tokens=T.TOKENS)
    text = chat_text("Tags:")
    assert text.count("<|image_pad|>") == 1 and text.endswith("<|im_start|>assistant\n")
    assert "<|vision_start|><|image_pad|><|vision_end|>Tags:<|im_end|>" in text
    assert expand_image_pads(text, [[1, 4, 6]]).count("<|image_pad|>") == 6
    with pytest.raises(ValueError):
        expand_image_pads(text, [[1, 4, 6], [1, 2, 2]])
    ids, am = left_pad([[5, 6, 7], [8]], 99)
    assert ids.tolist() == [[5, 6, 7], [99, 99, 8]] and am.tolist() == [[1, 1, 1], [0, 0, 1]]
    imgs = [np.zeros((60, 80, 3), np.uint8), np.zeros((120, 100, 3), np.uint8), np.zeros((40, 150, 3), np.uint8)]
    x = t.prepare_inputs(imgs)
    assert x["grid_thw"].tolist() == [[1, 4, 6], [1, 8, 8], [1, 2, 10]]
    n_img = [6, 16, 5]
    pad = (x["attention_mask"] == 0).sum(1)
    assert pad.tolist() == [10, 0, 11]
    L = x["input_ids"].shape[1]
    for b in range(3):
        row = x["input_ids"][b]
        assert (row[:pad[b]] == T.TOKENS["pad_token_id"]).all()
        assert row[pad[b]:].tolist() == T.encode(expand_image_pads(chat_text(t._build_prompt()), [x["grid_thw"][b]]))
        mine = x["image_rows"][(x["image_rows"] // L) == b] % L
        assert len(mine) == n_img[b] and (row[mine] == T.TOKENS["image_token_id"]).all() and (mine >= pad[b]).all()
    assert np.array_equal(x["position_ids"], rope_index(x["input_ids"], x["grid_thw"], 2000, attention_mask=x["attention_mask"])[0])


def test_left_padding_only():
    assert left_padding([[0, 0, 1, 1], [1, 1, 1, 1]]).tolist() == [2, 0]
    for bad in ([[1, 1, 0]], [[0, 1, 0, 1]], [[0, 0, 0]], [[2, 1]]):
        with pytest.raises(ValueError):
            left_padding(bad)


def test_to_rgb_modes():
    from PIL import Image
    rgba = np.random.default_rng(0).integers(0, 256, (5, 7, 4), dtype=np.uint8)
    assert np.array_equal(to_rgb(Image.fromarray(rgba, "RGBA")), rgba[..., :3])
    g = np.arange(35, dtype=np.uint8).reshape(5, 7)
    assert np.array_equal(to_rgb(Image.fromarray(g, "L")), np.repeat(g[..., None], 3, 2))
    p = Image.fromarray(g, "L").convert("P")
    assert np.array_equal(to_rgb(p), np.asarray(p.convert("RGB")))


class FakeTagger(VLMTagger):
    """generate_from_images replaced: every image is an int; a batch holding a value in `oom_batch` raises EngineCapacityError, a single
    image in `oom_single` too, and `boom` raises another error."""

    def __init__(self, batch_size, oom_batch=(), oom_single=(), boom=()):
        super().__init__({"model_path": "Qwen/Qwen2.5-VL-7B-Instruct", "vlm_batch_size": batch_size}, decode=lambda ids: ",".join(f"t{i}" for i in ids),
                         special_tokens=dict(eos_token_ids=(999,)))
        self.model = object()
        self.calls = []
        self.oom_batch, self.oom_single, self.boom = set(oom_batch), set(oom_single), set(boom)

    def generate_from_images(self, images, max_new_tokens=None, prompt=None):
        self.calls.append(list(images))
        if set(images) & self.boom:
            raise EngineError("something else")
        if (len(images) > 1 and set(images) & self.oom_batch) or (len(images) == 1 and images[0] in self.oom_single):
            raise EngineCapacityError("arena exhausted")
        return np.array([[im, im + 100, 999, 5] for im in images])


def test_tag_batch_sub_batches_keep_order():
    t = FakeTagger(3)
    got = t.tag_batch(list(range(1, 8)))
    assert got == [[f"t{i}", f"t{i + 100}"] for i in range(1, 8)]          # cut at the first EOS id
    assert [len(c) for c in t.calls] == [3, 3, 1]


def test_tag_batch_falls_back_to_single_images_on_capacity_errors():
    t = FakeTagger(3, oom_batch={2}, oom_single={3})
    got = t.tag_batch([1, 2, 3, 4, 5])
    assert got == [["t1", "t101"], ["t2", "t102"], [], ["t4", "t104"], ["t5", "t105"]]
    assert [len(c) for c in t.calls] == [3, 1, 1, 1, 2]


def test_tag_batch_propagates_other_errors():
    with pytest.raises(EngineError, match="something else"):
        FakeTagger(2, boom={3}).tag_batch([1, 2, 3, 4])
    t = FakeTagger(2, oom_batch={1}, boom={2})
    with pytest.raises(EngineError, match="something else"):
        t.tag_batch([1, 2])
    assert not issubclass(EngineError, EngineCapacityError)
