"""Drop-in for reference models/vlm_composition.py `VLMCompositionAnalyzer` (the 24gb profile's composition model, Qwen2-VL-2B) on the
engine: photo -> smart_resize / GPU preprocessing -> Qwen2-VL vision tower -> decoder prefill -> greedy decode that stops at EOS ->
`SCORE:` / `EXPLANATION:` parse. Same constructor, `analyze_composition`, `batch_analyze`, `_parse_response` and
`create_composition_analyzer`; RuleBasedCompositionAnalyzer (legacy profile, cv2 Canny / HoughLinesP) is not mirrored.

`model_dict['model']` is the engine-backed handle ModelManager.load_composition_model returns (Qwen2VLModel: `.engine` with the checkpoint
committed); `model_dict['processor']` is a Qwen2VLProcessor: the caller's tokenizer (`encode` chat text -> ids, `decode` ids -> text with
special tokens skipped) and the image processor's pixel limits. The batch form is a facet_amd extension: the reference loops over photos,
here each sub-batch of `vlm_batch_size` photos is one left-padded batch with one stop-at-EOS decode loop.
Parity: tests/test_vlm2_host.py (prompt and parse against recorded results of the reference class), tests/test_vlm2_gpu.py.
"""
import re
from typing import Any, Dict, List, Optional

import numpy as np

from ._lib import EngineCapacityError, FE_MODEL_VLM
from .vlm_tagger import (IMAGE_MEAN, IMAGE_STD, QWEN2_5_VL_TOKENS, chat_text, expand_image_pads, left_pad, rope_index, smart_resize, to_rgb,
                         vision_inputs_qwen2)

# [DEP-KNOWLEDGE: Qwen2-VL-2B-Instruct config.json - confirm against the checkpoint] geometry for Engine.vlm2_configure
QWEN2_VL_2B = dict(n_heads=12, n_kv_heads=2, head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24), vis_heads=16)
# Qwen2VLImageProcessorPil() defaults (size shortest_edge / longest_edge); the checkpoint's preprocessor_config.json may set a larger maximum
# [DEP-KNOWLEDGE, not checkable offline]
MIN_PIXELS_QWEN2, MAX_PIXELS_QWEN2 = 56 * 56, 28 * 28 * 1280

_ELEMENT_WORDS = (("rule_of_thirds", ("rule of thirds", "thirds")), ("leading_lines", ("leading line",)), ("symmetry", ("symmetr",)),
                  ("balance", ("balance",)), ("depth", ("depth", "layer")), ("framing", ("fram",)), ("negative_space", ("negative space",)))


class Qwen2VLProcessor:
    """What the analyzer needs of `AutoProcessor.from_pretrained(...)`: the tokenizer stays the caller's (ids in and out, as in VLMTagger),
    the image half is the engine's. special_tokens overrides the Qwen2-VL ids (the same as Qwen2.5-VL's)."""

    def __init__(self, encode, decode, min_pixels: int = MIN_PIXELS_QWEN2, max_pixels: int = MAX_PIXELS_QWEN2, special_tokens=None):
        self.encode, self.decode = encode, decode
        self.min_pixels, self.max_pixels = int(min_pixels), int(max_pixels)
        self.tokens = dict(QWEN2_5_VL_TOKENS, **(special_tokens or {}))


class Qwen2VLModel:
    """The engine-backed stand-in for the loaded `Qwen2VLForConditionalGeneration`: holds the state dict on the host and commits it to
    the engine (`to`) or drops the device copy (`cpu`), the two moves ModelManager makes between passes."""

    def __init__(self, engine, state_dict, geometry=None, weight_format="bf16", kv_format="bf16"):
        self.engine, self.state_dict, self.geometry = engine, state_dict, dict(geometry or QWEN2_VL_2B)
        if weight_format not in ("bf16", "fp8"):
            raise ValueError(f"weight_format {weight_format!r}: 'bf16' or 'fp8'")
        self.weight_format = weight_format      # "fp8": the decoder's Linear weights as e4m3 rows (Engine.vlm_weight_format)
        if kv_format not in ("bf16", "fp8", "bf16_e4m3"):
            raise ValueError(f"kv_format {kv_format!r}: 'bf16', 'fp8' or 'bf16_e4m3'")
        self.kv_format = kv_format              # "fp8": the decoder's KV cache as e4m3 rows (Engine.vlm_kv_format)
        self.loaded = False

    def to(self, device=None):
        if not self.loaded:
            self.engine.vlm2_configure(**self.geometry)
            self.engine.vlm_weight_format(self.weight_format)
            self.engine.vlm_kv_format(self.kv_format)
            self.engine.load_weights(FE_MODEL_VLM, self.state_dict)
            self.loaded = True
        return self

    def cpu(self):
        if self.loaded:
            self.engine.unload(FE_MODEL_VLM)
            self.loaded = False
        return self


class VLMCompositionAnalyzer:
    COMPOSITION_PROMPT = ("Analyze this photograph's composition. Rate the overall composition quality from 1 to 10 and briefly explain why.\n"
                          "\n"
                          "Consider these elements:\n"
                          "- Rule of thirds / subject placement\n"
                          "- Leading lines\n"
                          "- Balance and symmetry\n"
                          "- Depth and layering\n"
                          "- Framing\n"
                          "- Negative space usage\n"
                          "\n"
                          "Format your response as:\n"
                          "SCORE: [number 1-10]\n"
                          "EXPLANATION: [1-2 sentences explaining the score]")

    def __init__(self, model_dict: Dict[str, Any], device: str = 'cuda', max_tokens: int = 256, vlm_batch_size: int = 8):
        self.model = model_dict['model']
        self.processor = model_dict['processor']
        self.device = device
        self.max_tokens = max_tokens
        self.batch_size = int(vlm_batch_size)
        self.engine = getattr(self.model, 'engine', self.model)

    # -- generation ---------------------------------------------------------------------------------------------------------------------
    def prepare_inputs(self, images):
        """What `processor(text=[chat text] * n, images=images, padding=True)` yields, the pixel work left to the GPU (VLMTagger.prepare_inputs
        for this family: 14-pixel patches, the Qwen2.5 chat text)."""
        p = self.processor
        rgb = [to_rgb(im) for im in images]
        sizes = [smart_resize(a.shape[0], a.shape[1], 28, p.min_pixels, p.max_pixels) for a in rgb]
        grid = np.array([[1, oh // 14, ow // 14] for oh, ow in sizes], np.int64)
        text = chat_text(self.COMPOSITION_PROMPT, "qwen2_5")
        ids, am = left_pad([list(p.encode(expand_image_pads(text, g[None]))) for g in grid], p.tokens["pad_token_id"])
        img = p.tokens["image_token_id"]
        pos, _ = rope_index(ids, grid, img, attention_mask=am)
        image_rows = np.flatnonzero(((ids == img) & (am == 1)).reshape(-1)).astype(np.int32)
        return dict(rgb=rgb, sizes=sizes, grid_thw=grid, input_ids=ids, attention_mask=am, position_ids=pos, image_rows=image_rows)

    def generate_from_images(self, images, max_new_tokens: Optional[int] = None):
        """Greedy ids int [n, max_new_tokens] for a list of photos as one left-padded batch; the decode loop ends once every row has
        emitted EOS (rows are padded with their EOS id from there)."""
        x = self.prepare_inputs(images)
        n_new = int(max_new_tokens or self.max_tokens)
        if x["input_ids"].shape[1] + n_new > 8192:      # the engine's KV cache ends there: no point in running the tower first
            raise EngineCapacityError(f"a prompt of {x['input_ids'].shape[1]} positions and {n_new} new tokens do not fit the engine's 8192 "
                                      "(lower the processor's max_pixels)")
        e = self.engine
        e.vlm_preprocess_rgb(x["rgb"], x["sizes"], IMAGE_MEAN, IMAGE_STD)
        v = vision_inputs_qwen2(x["grid_thw"])
        e.vlm2_encode_images(None, v["patch_pos_hw"], v["cu_seqlens"], want_embeds=False)
        return e.vlm_generate(x["input_ids"], n_new, position_ids=x["position_ids"],
                              eos_token_ids=self.processor.tokens["eos_token_ids"], image_rows=x["image_rows"], attention_mask=x["attention_mask"],
                              stop_at_eos=True)

    def _texts(self, generated_ids) -> List[str]:
        eos = [int(t) for t in self.processor.tokens["eos_token_ids"]]
        out = []
        for row in np.asarray(generated_ids):
            hit = np.flatnonzero(np.isin(row, eos))
            out.append(self.processor.decode([int(t) for t in row[:hit[0] if hit.size else len(row)]]))
        return out

    # -- the reference's surface ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _failure(e) -> Dict[str, Any]:
        return {'composition_score': 5.0, 'explanation': f"Analysis error: {str(e)}", 'elements': {}}

    def analyze_composition(self, image) -> Dict[str, Any]:
        """-> {'composition_score': float in [0, 10], 'explanation': str, 'elements': {name: True}}; any failure (a photo whose prompt
        exceeds the engine's 8192 positions included) comes back as the reference's failure dict, score 5.0."""
        try:
            return self._parse_response(self._texts(self.generate_from_images([image]))[0])
        except Exception as e:
            print(f"VLM composition analysis error: {e}")
            return self._failure(e)

    def _parse_response(self, response: str) -> Dict[str, Any]:
        result = {'composition_score': 5.0, 'explanation': response.strip(), 'elements': {}}
        try:
            m = re.search(r'SCORE:\s*(\d+(?:\.\d+)?)', response, re.IGNORECASE)
            if m:
                result['composition_score'] = max(0.0, min(10.0, float(m.group(1))))
            m = re.search(r'EXPLANATION:\s*(.+?)(?:\n|$)', response, re.IGNORECASE | re.DOTALL)
            if m:
                result['explanation'] = m.group(1).strip()
            low = response.lower()
            result['elements'] = {name: True for name, words in _ELEMENT_WORDS if any(w in low for w in words)}
        except Exception as e:
            print(f"Response parsing error: {e}")
        return result

    def batch_analyze(self, images) -> List[Dict[str, Any]]:
        """One result per photo, in order, each equal to that photo's own analyze_composition: sub-batches of vlm_batch_size as one
        left-padded batch each; a sub-batch that does not fit the engine, or fails in any other way, is retried one photo at a time (as
        VLMTagger.tag_batch does on a capacity error), so a failure comes back as that photo's failure dict."""
        results: List[Dict[str, Any]] = []
        for i in range(0, len(images), self.batch_size):
            sub = list(images[i:i + self.batch_size])
            if len(sub) == 1:
                results.append(self.analyze_composition(sub[0]))
                continue
            try:
                results.extend(self._parse_response(t) for t in self._texts(self.generate_from_images(sub)))
            except Exception:      # did not fit (EngineCapacityError) or failed otherwise: each photo's own analyze_composition decides
                results.extend(self.analyze_composition(im) for im in sub)
        return results


def create_composition_analyzer(model_manager) -> Optional[VLMCompositionAnalyzer]:
    """The analyzer when the active profile's composition model is Qwen2-VL and it loads, else None (the reference's rule-based analyzer of
    the legacy profile is not served here)."""
    if model_manager.is_using_qwen_composition():
        model_dict = model_manager.load_composition_model()
        if model_dict and 'model' in model_dict:
            settings = getattr(model_manager, 'model_settings', {}) or {}
            return VLMCompositionAnalyzer(model_dict, model_manager.device, settings.get('qwen2_vl', {}).get('max_new_tokens', 256))
    return None
