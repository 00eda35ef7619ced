"""CPU: the host side of the Qwen2-VL composition analyzer. COMPOSITION_PROMPT and _parse_response against results recorded from the
reference's own class (tests/golden/vlm_composition_host_golden.json, make_vlm_composition_host_golden.py); rope_index and the tower's
index arrays against tests/golden/vlm2_golden.npz (transformers' Qwen2VLForConditionalGeneration / Qwen2VLImageProcessorPil,
make_vlm2_golden.py); prepare_inputs on the photo batch; the ModelManager's composition-model methods per profile."""
import json
import os

import numpy as np
import pytest

from facet_amd.model_manager import ModelManager
from facet_amd.vlm_composition import (MAX_PIXELS_QWEN2, MIN_PIXELS_QWEN2, QWEN2_VL_2B, Qwen2VLProcessor, VLMCompositionAnalyzer,
                                       create_composition_analyzer)
from facet_amd.vlm_tagger import rope_index, vision_inputs_qwen2
from facet_amd.weights import synthetic_state_dict

HERE = os.path.dirname(__file__)
G = np.load(os.path.join(HERE, "golden", "vlm2_golden.npz"))
H = json.load(open(os.path.join(HERE, "golden", "vlm_composition_host_golden.json")))
IMG = int(G["image_token_id"])


def _analyzer(**kw):
    from standins import vlm_tokenizer as T
    proc = Qwen2VLProcessor(T.encode, T.decode, int(G["photo_min_pixels"]), int(G["photo_max_pixels"]), special_tokens=T.TOKENS)
    return VLMCompositionAnalyzer({"model": None, "processor": proc}, **kw)


def test_prompt_and_defaults_equal_the_reference():
    assert VLMCompositionAnalyzer.COMPOSITION_PROMPT == H["prompt"]
    a = _analyzer()
    assert a.max_tokens == H["max_tokens"] == 256 and a.device == "cuda" and a.batch_size == 8
    assert (MIN_PIXELS_QWEN2, MAX_PIXELS_QWEN2) == (3136, 1003520)
    assert QWEN2_VL_2B["n_heads"] // QWEN2_VL_2B["n_kv_heads"] == 6 and QWEN2_VL_2B["mrope_section"] == (16, 24, 24)


@pytest.mark.parametrize("case", H["cases"], ids=[str(i) for i in range(len(H["cases"]))])
def test_parse_response_equals_the_reference(case):
    got = _analyzer()._parse_response(case["response"])
    assert got == case["result"], (case["response"], got, case["result"])
    assert type(got["composition_score"]) is float


def test_recorded_cases_cover_the_parse_branches():
    scores = [c["result"]["composition_score"] for c in H["cases"]]
    assert len(H["cases"]) >= 20 and 0.0 in scores and 10.0 in scores and 7.5 in scores and 5.0 in scores
    seen = set().union(*[set(c["result"]["elements"]) for c in H["cases"]])
    assert seen == {"rule_of_thirds", "leading_lines", "symmetry", "balance", "depth", "framing", "negative_space"}
    assert any(c["response"] == "" for c in H["cases"])


def test_rope_index_equals_the_decoder_input_positions():
    pos, _ = rope_index(G["input_ids"], G["vis_grid_thw"], IMG)
    assert np.array_equal(pos, G["position_ids"])
    pos, _ = rope_index(G["short_input_ids"], G["short_grid_thw"], IMG)
    assert np.array_equal(pos, G["short_position_ids"])
    pos, _ = rope_index(G["batch_input_ids"], G["batch_grid_thw"], IMG, attention_mask=G["batch_attention_mask"])
    assert np.array_equal(pos, G["batch_position_ids"])


def test_vision_inputs_block_major_positions_and_one_segment_per_image():
    v = vision_inputs_qwen2(G["vis_grid_thw"])
    assert v["cu_seqlens"].tolist() == [0, 120, 156] and v["patch_pos_hw"].shape == (156, 2)
    assert v["patch_pos_hw"][:6].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [0, 2], [0, 3]]
    assert v["patch_pos_hw"][120:124].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]] and v["patch_pos_hw"][-1].tolist() == [5, 5]


def test_prepare_inputs_equals_the_processor_batch():
    """Independent of the project: the grids (the processor's size choice), and the position ids (transformers' get_rope_index on the
    fixture's ids). NOT independent: photo_input_ids / photo_attention_mask, which the golden script builds with the project's own
    chat_text, expand_image_pads, left_pad and COMPOSITION_PROMPT (the chat template ships inside the checkpoint, unpinned offline) - those
    two asserts only hold the fixture and the code in step, as in the Qwen3 golden."""
    from PIL import Image
    a = _analyzer()
    photos = [G[f"photo_{i}"] for i in range(3)]
    x = a.prepare_inputs([Image.fromarray(p, "RGBA" if p.shape[2] == 4 else "RGB") for p in photos])
    assert np.array_equal(x["grid_thw"], G["photo_grid_thw"])
    assert np.array_equal(x["input_ids"], G["photo_input_ids"])
    assert np.array_equal(x["attention_mask"], G["photo_attention_mask"])
    assert np.array_equal(x["position_ids"], G["photo_position_ids"])


class _Cfg:
    def __init__(self, mc):
        self.mc = mc

    def get_model_config(self):
        return self.mc


PROFILES = {"legacy": {"composition_model": "samp-net"}, "8gb": {"composition_model": "samp-net"}, "16gb": {"composition_model": "samp-net"},
            "24gb": {"composition_model": "qwen2-vl-2b"}}


@pytest.mark.parametrize("profile,want", [("legacy", False), ("8gb", False), ("16gb", False), ("24gb", True)])
def test_model_manager_answers_per_profile(profile, want):
    for table in (PROFILES, None):      # the config's own table, or the reference's defaults without one
        mc = {"vram_profile": profile}
        if table:
            mc["profiles"] = table
        mm = ModelManager(_Cfg(mc), engine=object())
        assert mm.is_using_qwen_composition() is want
        if not want:
            assert mm.load_composition_model() is None
            assert create_composition_analyzer(mm) is None


def test_composition_model_without_a_checkpoint_is_a_load_failure_not_a_download(capsys):
    mm = ModelManager(_Cfg({"vram_profile": "24gb", "profiles": PROFILES, "qwen2_vl": {"max_new_tokens": 256}}), engine=object())
    assert mm.load_composition_model() is None and create_composition_analyzer(mm) is None
    assert "no checkpoint" in capsys.readouterr().out
    with pytest.raises(FileNotFoundError, match="no checkpoint"):
        mm._create("qwen2_vl")
    with pytest.raises(KeyError):
        mm._create("ram_plus")


def test_weight_specs_tie_the_head_at_2b():
    sd = synthetic_state_dict("qwen2_vl_tiny", 1)
    assert "lm_head.weight" not in sd and "model.visual.blocks.0.mlp.fc1.bias" in sd and "model.visual.merger.ln_q.bias" in sd
    assert sd["model.language_model.layers.0.self_attn.q_proj.weight"].shape == (768, 768)
    assert sd["model.language_model.layers.0.self_attn.k_proj.weight"].shape == (128, 768)
    assert "lm_head.weight" in synthetic_state_dict("qwen2_vl_tiny_untied", 1)
