"""Host-side mirror of the reference's VLM tagger (models/vlm_tagger.py) over the engine's Qwen2.5-VL text decoder.

SURVEY 8(f)-4 / BASELINE configs[4]: the vision tower and the text decoder run in the engine (`fe_vlm_encode_images`, `fe_vlm_prefill_images`,
`fe_vlm_generate`: greedy, bf16 as the reference loads the model, models/vlm_tagger.py:155-184); what stays here is what the reference also
does on the host - the prompt built from the tag vocabulary (:88-148), the index arithmetic transformers derives from `image_grid_thw`
(window order, segment bounds, M-RoPE position ids: `vision_indices`, `rope_index`), the generate loop's bookkeeping and the parsing of the
generated text into vocabulary tags (:446-495). The photo path (`tag_image` / `tag_batch`, :202-308 / :327-368) restates the processor:
smart_resize and the grids on the host, the resample / rescale / normalise / patchify on the GPU (`fe_vlm_preprocess_rgb`, matching
transformers' PIL backend bit for bit), the chat text and its <|image_pad|> expansion here, left padding of the batch in the engine
(`fe_vlm_prefill_images_padded`). The tokenizer stays the caller's (`encode` / `decode` callables of the checkpoint's processor, exactly as
the CLIP text tower takes token ids, facet_amd/tagger.py); `generate_with_images` still takes the processor's own tensors. The scored half
(`tag_image_with_scores` / `get_tags_with_scores`, :497-626) takes the greedy tokens' log-probs from the engine's selection pass
(`Engine.vlm_generate(return_logprobs=True)`) and splits them into tags here (`tag_confidences`).
"""
import math
from typing import Any, Dict, Iterable, List, Optional, Sequence

import numpy as np

from ._lib import FE_MODEL_VLM, EngineCapacityError

QWEN2_5_VL_7B = dict(n_heads=28, n_kv_heads=4, head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24))

# [DEP-KNOWLEDGE: Qwen2.5-VL-7B-Instruct tokenizer_config / generation_config] special-token ids of the checkpoint's tokenizer; parameters of
# VLMTagger (special_tokens=...), so a checkpoint with other ids only passes its own
QWEN2_5_VL_TOKENS = dict(image_token_id=151655, vision_start_token_id=151652, vision_end_token_id=151653, pad_token_id=151643,
                         eos_token_ids=(151645, 151643))
# [DEP-KNOWLEDGE: transformers Qwen2VLImageProcessor defaults] OPENAI_CLIP_MEAN / OPENAI_CLIP_STD, min / max pixels of smart_resize
IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)
MIN_PIXELS, MAX_PIXELS = 56 * 56, 28 * 28 * 1280
# [DEP-KNOWLEDGE: Qwen2.5-VL chat template - parity unpinned: the template ships inside the checkpoint (tokenizer_config.json /
# chat_template.json), not available offline] apply_chat_template(messages = [user: image, text], add_generation_prompt=True) restated
CHAT_TEMPLATE = ("<|im_start|>system\nYou are a helpful assistant.<|im_end|>\n"
                 "<|im_start|>user\n<|vision_start|><|image_pad|><|vision_end|>{prompt}<|im_end|>\n"
                 "<|im_start|>assistant\n")
IMAGE_PAD = "<|image_pad|>"

# Qwen3-VL (transformers Qwen3VLForConditionalGeneration; the reference's 8gb / 16gb profiles tag with qwen3-vl-2b)
# [DEP-KNOWLEDGE: Qwen3-VL-2B-Instruct config.json - confirm against the checkpoint] decoder geometry for Engine.vlm3_configure
QWEN3_VL_2B = dict(n_heads=16, n_kv_heads=8, head_dim=128, rope_theta=5e6, rms_eps=1e-6, mrope_section=(24, 20, 20), vis_heads=16,
                   deepstack_indexes=(5, 11, 17))
# [DEP-KNOWLEDGE: Qwen3-VL tokenizer] the same special-token ids as Qwen2.5-VL's
QWEN3_VL_TOKENS = dict(QWEN2_5_VL_TOKENS)
# [DEP-KNOWLEDGE: Qwen3-VL preprocessor_config] mean / std 0.5, 16-pixel patches merged 2 x 2 (smart_resize factor 32), shortest_edge
# 65536 = min_pixels; the reference passes max_pixels = model_config.get('max_pixels', 512*28*28) to the processor (vlm_tagger.py:178-181)
IMAGE_MEAN_QWEN3 = (0.5, 0.5, 0.5)
IMAGE_STD_QWEN3 = (0.5, 0.5, 0.5)
MIN_PIXELS_QWEN3, MAX_PIXELS_QWEN3 = 65536, 512 * 28 * 28
# [DEP-KNOWLEDGE: Qwen3-VL chat template - parity unpinned like CHAT_TEMPLATE; no default system turn] apply_chat_template(messages =
# [user: image, text], add_generation_prompt=True) restated
CHAT_TEMPLATE_QWEN3 = ("<|im_start|>user\n<|vision_start|><|image_pad|><|vision_end|>{prompt}<|im_end|>\n"
                       "<|im_start|>assistant\n")


def smart_resize(height: int, width: int, factor: int = 28, min_pixels: int = MIN_PIXELS, max_pixels: int = MAX_PIXELS):
    """transformers.models.qwen2_vl.image_processing_qwen2_vl.smart_resize restated: both sides multiples of `factor`, the pixel count within
    [min_pixels, max_pixels], the aspect ratio kept as closely as possible. -> (height, width)."""
    if max(height, width) / min(height, width) > 200:
        raise ValueError(f"absolute aspect ratio must be smaller than 200, got {max(height, width) / min(height, width)}")
    h_bar = round(height / factor) * factor
    w_bar = round(width / factor) * factor
    if h_bar * w_bar > max_pixels:
        beta = math.sqrt((height * width) / max_pixels)
        h_bar = max(factor, math.floor(height / beta / factor) * factor)
        w_bar = max(factor, math.floor(width / beta / factor) * factor)
    elif h_bar * w_bar < min_pixels:
        beta = math.sqrt(min_pixels / (height * width))
        h_bar = math.ceil(height * beta / factor) * factor
        w_bar = math.ceil(width * beta / factor) * factor
    return h_bar, w_bar


def to_rgb(image) -> np.ndarray:
    """A PIL image (or an HWC uint8 array) -> uint8 RGB [h, w, 3], as the processor's convert_to_rgb does in transformers 5: any mode other
    than RGB goes through `image.convert("RGB")` (RGBA drops its alpha; transformers 4.x composited RGBA on white first - unpinned)."""
    if isinstance(image, np.ndarray):
        a = image if image.ndim == 3 else np.repeat(image[..., None], 3, axis=2)
        if a.dtype != np.uint8 or a.shape[2] != 3:
            raise ValueError(f"expected uint8 RGB [h, w, 3], got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a)
    if image.mode != "RGB":
        image = image.convert("RGB")
    return np.asarray(image, dtype=np.uint8)


def chat_text(prompt: str, family: str = "qwen2_5") -> str:
    """The chat-formatted text of one photo + prompt (CHAT_TEMPLATE, or CHAT_TEMPLATE_QWEN3 for family "qwen3"), one <|image_pad|>
    placeholder before expansion."""
    return (CHAT_TEMPLATE_QWEN3 if family == "qwen3" else CHAT_TEMPLATE).format(prompt=prompt)


def expand_image_pads(text: str, grids, merge_size: int = 2, image_pad: str = IMAGE_PAD) -> str:
    """The processor's text-level expansion: the i-th <|image_pad|> becomes t * h * w / merge^2 copies for grid i."""
    parts = text.split(image_pad)
    grids = np.asarray(grids, np.int64).reshape(-1, 3)
    if len(parts) - 1 != len(grids):
        raise ValueError(f"{len(parts) - 1} image placeholders for {len(grids)} images")
    out = [parts[0]]
    for g, rest in zip(grids, parts[1:]):
        out.append(image_pad * int(g[0] * g[1] * g[2] // merge_size ** 2))
        out.append(rest)
    return "".join(out)


def left_pad(id_rows: Sequence[Sequence[int]], pad_token_id: int):
    """Token-id rows of different lengths -> (input_ids int32 [n, L], attention_mask int32 [n, L]), padded on the LEFT (the processor's
    padding=True with padding_side='left', the only side on which batched greedy generation of a decoder-only model is defined)."""
    L = max(len(r) for r in id_rows)
    ids = np.full((len(id_rows), L), int(pad_token_id), np.int32)
    am = np.zeros((len(id_rows), L), np.int32)
    for b, r in enumerate(id_rows):
        if len(r):
            ids[b, L - len(r):] = np.asarray(r, np.int32)
            am[b, L - len(r):] = 1
    return ids, am


def vision_indices(grid_thw, spatial_merge_size: int = 2, window_size: int = 112, patch_size: int = 14):
    """The index arrays of the vision tower for images of `grid_thw` [n_images, 3] (t, h, w in patches): numpy restatement of
    transformers.vision_utils.get_vision_position_ids / get_vision_window_index / get_vision_cu_seqlens (what
    Qwen2_5_VisionTransformerPretrainedModel.forward derives from image_grid_thw). Returns a dict for Engine.vlm_encode_images:
    patch_pos_hw [n, 2] (row, column of every patch, in WINDOW order), window_index [n / m^2] (raster merge-block index at each
    window-order slot), cu_window_seqlens, cu_seqlens (segment bounds in patches)."""
    grid = np.asarray(grid_thw, dtype=np.int64).reshape(-1, 3)
    m, unit = spatial_merge_size, spatial_merge_size ** 2
    win = window_size // spatial_merge_size // patch_size          # window side in merge blocks (4)
    pos, widx, cu_win, cu_full, base = [], [], [0], [0], 0
    for t, h, w in grid:
        hh, ww = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        blk = lambda a: a.reshape(h // m, m, w // m, m).transpose(0, 2, 1, 3).reshape(-1)      # block-major over the m x m merge blocks
        pos.append(np.tile(np.stack([blk(hh), blk(ww)], -1), (t, 1)))
        gh, gw = h // m, w // m
        idx = np.arange(t * gh * gw).reshape(t, gh, gw)
        ph, pw = win - gh % win, win - gw % win                    # (a full extra window of padding when the side divides: as transformers)
        nh, nw = (gh + ph) // win, (gw + pw) // win
        padded = np.pad(idx, ((0, 0), (0, ph), (0, pw)), constant_values=-100)
        padded = padded.reshape(t, nh, win, nw, win).transpose(0, 1, 3, 2, 4).reshape(t, nh * nw, win, win)
        seqlens = (padded != -100).sum((2, 3)).reshape(-1)
        flat = padded.reshape(-1)
        widx.append(flat[flat != -100] + base)
        cu_win.extend((np.cumsum(seqlens) * unit + cu_win[-1]).tolist())
        base += t * gh * gw
        for _ in range(t):                                         # full attention: one segment per frame
            cu_full.append(cu_full[-1] + h * w)
    window_index = np.concatenate(widx).astype(np.int32)
    cu_win = np.asarray(cu_win, np.int32)
    cu_win = cu_win[np.concatenate([[True], np.diff(cu_win) != 0])]          # unique_consecutive: drops the empty padded windows
    pos = np.concatenate(pos, 0)                                             # raster (block-major) order
    n = pos.shape[0]
    pos_w = pos.reshape(n // unit, unit, 2)[window_index].reshape(n, 2)      # rows regrouped window by window, like the hidden states
    return {"patch_pos_hw": pos_w.astype(np.int32), "window_index": window_index, "cu_window_seqlens": cu_win,
            "cu_seqlens": np.asarray(cu_full, np.int32)}


def vision_inputs_qwen3(grid_thw, num_grid_per_side: int, spatial_merge_size: int = 2):
    """The index arrays of Qwen3-VL's vision tower for images of `grid_thw` [n_images, 3]: numpy restatement of transformers.vision_utils
    get_vision_position_ids (rows / columns in 2x2-block-major order), get_vision_interpolation_indices_and_weights(mode="bilinear",
    align_corners=True) into the num_grid_per_side^2 position table (fp32 arithmetic as torch's), and get_vision_cu_seqlens (one segment
    per frame). Returns a dict for Engine.vlm3_encode_images: patch_pos_hw [n, 2] int32, interp_idx [n, 4] int64, interp_w [n, 4] float32,
    cu_seqlens int32."""
    grid = np.asarray(grid_thw, dtype=np.int64).reshape(-1, 3)
    m, side = spatial_merge_size, int(num_grid_per_side)
    f32 = np.float32
    pos, idx, wts, cu = [], [], [], [0]
    for t, h, w in grid:
        t, h, w = int(t), int(h), int(w)
        hh, ww = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        blk = lambda a: a.reshape(h // m, m, w // m, m).transpose(0, 2, 1, 3).reshape(-1)      # block-major over the m x m merge blocks
        row, col = blk(hh), blk(ww)
        pos.append(np.tile(np.stack([row, col], -1), (t, 1)))

        def axis(index, size):
            src = index.astype(f32) * f32(side - 1) / f32(max(size - 1, 1))
            fl = np.floor(src)
            taps = np.clip(fl.astype(np.int64)[:, None] + np.arange(2), 0, side - 1)
            dist = np.abs((src[:, None] - fl[:, None]) - np.arange(2).astype(f32))
            return taps, np.maximum(f32(1) - dist, f32(0)).astype(f32)

        ht, hw_ = axis(row, h)
        wt, ww_ = axis(col, w)
        idx.append(np.tile((ht[:, :, None] * side + wt[:, None, :]).reshape(-1, 4), (t, 1)))
        wts.append(np.tile((hw_[:, :, None] * ww_[:, None, :]).reshape(-1, 4).astype(f32), (t, 1)))
        for _ in range(t):
            cu.append(cu[-1] + h * w)
    return {"patch_pos_hw": np.concatenate(pos, 0).astype(np.int32), "interp_idx": np.concatenate(idx, 0).astype(np.int64),
            "interp_w": np.concatenate(wts, 0).astype(np.float32), "cu_seqlens": np.asarray(cu, np.int32)}


def vision_inputs_qwen2(grid_thw, spatial_merge_size: int = 2):
    """The index arrays of Qwen2-VL's vision tower (no windows, no position table) for images of `grid_thw` [n_images, 3]: rows / columns
    of every patch in 2x2-block-major order (transformers.vision_utils.get_vision_position_ids) and one attention segment per frame
    (get_vision_cu_seqlens). Returns a dict for Engine.vlm2_encode_images: patch_pos_hw [n, 2] int32, cu_seqlens int32."""
    grid = np.asarray(grid_thw, dtype=np.int64).reshape(-1, 3)
    m = spatial_merge_size
    pos, cu = [], [0]
    for t, h, w in grid:
        t, h, w = int(t), int(h), int(w)
        hh, ww = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        blk = lambda a: a.reshape(h // m, m, w // m, m).transpose(0, 2, 1, 3).reshape(-1)      # block-major over the m x m merge blocks
        pos.append(np.tile(np.stack([blk(hh), blk(ww)], -1), (t, 1)))
        for _ in range(t):
            cu.append(cu[-1] + h * w)
    return {"patch_pos_hw": np.concatenate(pos, 0).astype(np.int32), "cu_seqlens": np.asarray(cu, np.int32)}


def interleaved_mrope_components(mrope_section=(24, 20, 20), n_freq: int = 64):
    """Which position component (0 temporal, 1 height, 2 width) each rotary frequency of Qwen3-VL's interleaved M-RoPE takes
    (Qwen3VLTextRotaryEmbedding.apply_interleaved_mrope): j % 3 == 1 and j < 3 s_h -> height, j % 3 == 2 and j < 3 s_w -> width, else
    temporal. The engine's rotary kernel applies the same rule."""
    j = np.arange(n_freq)
    out = np.zeros(n_freq, np.int32)
    out[(j % 3 == 1) & (j < 3 * mrope_section[1])] = 1
    out[(j % 3 == 2) & (j < 3 * mrope_section[2])] = 2
    return out


def rope_index(input_ids, grid_thw, image_token_id: int, spatial_merge_size: int = 2, attention_mask=None):
    """M-RoPE position ids [3, n_seq, len] of prompts with image placeholders: numpy restatement of Qwen2_5_VLModel.get_rope_index for
    still images (what the reference's processor + generate compute): text tokens count up on all three axes; a run of <|image_pad|>
    tokens takes (start, start + row, start + column) over its merged grid, and the next text token continues at start + max(rows,
    columns). With attention_mask, only the unmasked tokens of a row are counted (from 0) and masked positions keep 0, as transformers
    does. Returns (position_ids, next_position [n_seq] = the position of the first generated token: the row's maximum + 1)."""
    ids = np.asarray(input_ids)
    grids = iter(np.asarray(grid_thw, dtype=np.int64).reshape(-1, 3))
    out = np.zeros((3,) + ids.shape, np.int32)
    nxt = np.zeros(ids.shape[0], np.int32)
    keep = np.ones(ids.shape, bool) if attention_mask is None else np.asarray(attention_mask).astype(bool)
    assert keep.shape == ids.shape, (keep.shape, ids.shape)
    for b, full_row in enumerate(ids):
        row = full_row[keep[b]]
        cur, i, cols = 0, 0, []
        while i < len(row):
            if row[i] == image_token_id:
                t, h, w = next(grids)
                gh, gw = int(h) // spatial_merge_size, int(w) // spatial_merge_size
                n = int(t) * gh * gw
                if not (row[i:i + n] == image_token_id).all():
                    raise ValueError("a run of image placeholder tokens does not match its grid")
                hh, ww = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
                tt = np.repeat(np.arange(int(t)), gh * gw)
                cols.append(np.stack([tt + cur, np.tile(hh.reshape(-1), int(t)) + cur, np.tile(ww.reshape(-1), int(t)) + cur]))
                cur += max(gh, gw)
                i += n
            else:
                cols.append(np.full((3, 1), cur))
                cur += 1
                i += 1
        p = np.concatenate(cols, 1)
        out[:, b, keep[b]] = p
        nxt[b] = p.max() + 1
    return out, nxt


def edit_distance(a: str, b: str) -> int:
    """Levenshtein distance (insert / delete / substitute, unit costs) by a rolling row of the DP table."""
    if not a:
        return len(b)
    if not b:
        return len(a)
    row = np.arange(len(b) + 1)
    for i, ca in enumerate(a, 1):
        diag, row[0] = row[0], i
        for j, cb in enumerate(b, 1):
            diag, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, diag + (ca != cb))
    return int(row[-1])


def tag_confidences(token_ids: Sequence[int], logprobs: Sequence[float], tags: Sequence[str], token_text) -> Dict[str, float]:
    """Per-tag confidences of one generated row, as the reference's tag_image_with_scores computes them (models/vlm_tagger.py:590-618):
    token_ids / logprobs are the generated tokens up to and including the first EOS (HF stops there at batch 1 and that step is in
    `outputs.scores`), tags the `_parse_tags` result of the row's decoded text, token_text(id) the text of one token. The log-probs are
    split into segments at tokens whose text contains ',' - such a token closes a non-empty segment and is dropped, but is appended to an
    empty one (a leading or repeated comma). Tag i takes segment i BY INDEX (even where _parse_tags dropped or merged pieces): confidence
    clamp(exp(mean log-prob), 0, 1), 1.0 when there is no such segment. token_text is the caller's `decode([id])`, which skips special
    tokens (""), where the reference decodes them with skip_special_tokens=False into their literal text; neither contains a comma, so the
    segments are the same."""
    segments: List[List[float]] = []
    cur: List[float] = []
    for tid, lp in zip(token_ids, logprobs):
        if "," in token_text(int(tid)) and cur:
            segments.append(cur)
            cur = []
        else:
            cur.append(float(lp))
    if cur:
        segments.append(cur)
    out: Dict[str, float] = {}
    for i, tag in enumerate(tags):
        if i < len(segments) and segments[i]:
            out[tag] = max(0.0, min(1.0, math.exp(sum(segments[i]) / len(segments[i]))))
        else:
            out[tag] = 1.0
    return out


class VLMTagger:
    """Same constructor and public surface as the reference class (models/vlm_tagger.py:45-87): `model_config` (model_path,
    vlm_batch_size, max_new_tokens, ...), optional `scoring_config` for the tag vocabulary. `engine` is the facet_amd Engine the decoder
    lives in; `decode` / `encode` are the tokenizer callables of the checkpoint's processor (ids -> text with special tokens skipped,
    chat-formatted text -> ids); `special_tokens` overrides QWEN2_5_VL_TOKENS (image / vision / pad / EOS ids)."""

    def __init__(self, model_config: Dict[str, Any], scoring_config=None, engine=None, decode=None, encode=None, special_tokens=None):
        self.model_config = model_config
        self.scoring_config = scoring_config
        self.engine = engine
        self.decode, self.encode = decode, encode
        self.model = None
        self.device = "cuda"
        path = model_config.get("model_path", "")
        self.family = "qwen3" if ("Qwen3" in path or "qwen3" in path) else "qwen2_5"
        self.tokens = dict(QWEN3_VL_TOKENS if self.family == "qwen3" else QWEN2_5_VL_TOKENS, **(special_tokens or {}))
        self.batch_size = model_config.get("vlm_batch_size", 4 if self.family == "qwen3" else 2)
        self.valid_tags = set(scoring_config.get_tag_vocabulary().keys()) if scoring_config else set()
        # "bf16" (the reference's dtype) or "fp8": the decoder's Linear weights as e4m3 rows (Engine.vlm_weight_format)
        self.weight_format = model_config.get("weight_format", "bf16")
        if self.weight_format not in ("bf16", "fp8"):
            raise ValueError(f"weight_format {self.weight_format!r}: 'bf16' or 'fp8'")
        # "bf16", "fp8" (the decoder's KV cache as e4m3 rows read by the decode attention) or "bf16_e4m3" (Engine.vlm_kv_format)
        self.kv_format = model_config.get("kv_format", "bf16")
        if self.kv_format not in ("bf16", "fp8", "bf16_e4m3"):
            raise ValueError(f"kv_format {self.kv_format!r}: 'bf16', 'fp8' or 'bf16_e4m3'")
        self._prompt = None

    # -- lifecycle (ModelManager calls load / unload around a pass) ------------------------------------------------------------------
    def load(self, state_dict=None, geometry=None):
        """Commits a Qwen2_5_VLForConditionalGeneration state dict (name -> array) to the engine. geometry: fe_vlm_configure's
        arguments (default Qwen2.5-VL-7B-Instruct)."""
        if self.model is not None:
            return
        if state_dict is None:
            raise FileNotFoundError("no checkpoint: pass the model's state dict (the reference downloads it with from_pretrained, "
                                    "models/vlm_tagger.py:170-176; there is no network here)")
        self.engine.vlm_weight_format(self.weight_format)      # read by the commit below
        self.engine.vlm_kv_format(self.kv_format)              # read by every prefill
        if self.family == "qwen3":      # Qwen3VLForConditionalGeneration: geometry = Engine.vlm3_configure's arguments (default Qwen3-VL-2B)
            self.engine.vlm3_configure(**dict(geometry or QWEN3_VL_2B))
            self.engine.load_weights(FE_MODEL_VLM, state_dict)
            self.model = self.engine
            return
        geometry = dict(geometry or QWEN2_5_VL_7B)
        vis = {k: geometry.pop(k) for k in ("vis_heads", "fullatt_block_indexes") if k in geometry}
        self.engine.vlm_configure(**geometry)
        self.engine.vlm_vision_configure(vis.get("vis_heads", 16), vis.get("fullatt_block_indexes", (7, 15, 23, 31)))
        self.engine.load_weights(FE_MODEL_VLM, state_dict)      # model.language_model.*, lm_head.weight and (when present) model.visual.*
        self.model = self.engine

    def unload(self):
        if self.model is not None:
            self.engine.unload(FE_MODEL_VLM)
            self.model = None

    # -- prompt (reference :88-148) -----------------------------------------------------------------------------------------------------
    def _build_prompt(self) -> str:
        if self._prompt is None:
            self._prompt = self._fallback_prompt() if not self.scoring_config else self._vocabulary_prompt()
        return self._prompt

    def _vocabulary_prompt(self) -> str:
        out = ["Analyze this photo and provide semantic tags.", "",
               "Return ONLY a comma-separated list of relevant tags from this exact list:"]
        seen = set()
        for cat in self.scoring_config.get_categories():
            names = [n for n in (cat.get("tags", {}) or {}) if n not in seen]
            if names:
                seen.update(names)
                out.append(f"- {cat['name'].replace('_', ' ').title()}: {', '.join(names)}")
        extra = [n for n in (self.scoring_config.config.get("standalone_tags", {}) or {}) if n not in seen]
        if extra:
            out.append(f"- Other: {', '.join(extra)}")
        out += ["", "Tags:"]
        return "\n".join(out)

    @staticmethod
    def _fallback_prompt() -> str:
        return ("Analyze this photo and provide semantic tags.\n\n"
                "Return ONLY a comma-separated list of relevant tags from these categories:\n"
                "- Scene: landscape, portrait, street, architecture, macro, wildlife, aerial, concert, night, astro, food, sports, travel, "
                "fashion, urban\n"
                "- Subject: person, animal, building, nature, water, sky, mountain, beach, forest, flower, vehicle\n"
                "- Style: black_and_white, silhouette, long_exposure, dramatic, minimalist, vintage, cinematic, abstract\n"
                "- Mood: dramatic, peaceful, energetic, intimate, moody\n\nTags:")

    # -- generation ---------------------------------------------------------------------------------------------------------------------
    def generate_with_images(self, input_ids, pixel_values, image_grid_thw, image_token_id: int, max_new_tokens: Optional[int] = None,
                             eos_token_ids: Iterable[int] = ()):
        """`self.model.generate(**processor(text=..., images=...), max_new_tokens=..., do_sample=False)` (reference :245-259, :346-360) on the
        processor's tensors: input_ids int [n, len] with the <|image_pad|> runs in place, pixel_values [n_patches, 1176], image_grid_thw
        [n_images, 3]. The vision tower encodes all images of the batch in one call, their embeddings replace the placeholder rows, the
        decoder prefills with the M-RoPE positions of get_rope_index and decodes greedily. -> int [n, max_new_tokens]."""
        if self.model is None:
            raise RuntimeError("VLMTagger.load() first")
        ids = np.asarray(input_ids)
        idx = vision_indices(image_grid_thw)
        self.engine.vlm_encode_images(pixel_values, idx["patch_pos_hw"], idx["window_index"], idx["cu_window_seqlens"], idx["cu_seqlens"], want_embeds=False)
        pos, _ = rope_index(ids, image_grid_thw, image_token_id)
        rows = np.flatnonzero(ids.reshape(-1) == image_token_id).astype(np.int32)
        n_new = int(max_new_tokens or self.model_config.get("max_new_tokens", 100))
        return self.engine.vlm_generate(ids, n_new, position_ids=pos, eos_token_ids=eos_token_ids, image_rows=rows)

    def generate_ids(self, input_ids, max_new_tokens: Optional[int] = None, position_ids=None, eos_token_ids: Iterable[int] = ()):
        """Greedy continuation of a batch of equally long prompts: int [n, len] -> int [n, max_new_tokens] (the slice
        `output_ids[:, input_len:]` the reference takes, :262-265 / :363)."""
        if self.model is None:
            raise RuntimeError("VLMTagger.load() first")
        n_new = int(max_new_tokens or self.model_config.get("max_new_tokens", 100))
        return self.engine.vlm_generate(np.asarray(input_ids), n_new, position_ids=position_ids, eos_token_ids=eos_token_ids)

    # -- photos in (reference :202-308 tag_image / tag_batch, :327-368 _batch_qwen2_5) -----------------------------------------------------
    def prepare_inputs(self, images, prompt: Optional[str] = None):
        """What `processor(text=[chat text] * n, images=images, padding=True)` yields, with the pixel work left to the GPU: -> dict of
        rgb (uint8 arrays), sizes (smart_resize targets), grid_thw [n, 3], input_ids / attention_mask int32 [n, L] (left-padded),
        position_ids [3, n, L] and image_rows (flat indices of the <|image_pad|> tokens, in order)."""
        if self.encode is None:
            raise RuntimeError("no tokenizer: pass encode= (the checkpoint's processor.tokenizer.encode)")
        rgb = [to_rgb(im) for im in images]
        q3 = self.family == "qwen3"
        lo = int(self.model_config.get("min_pixels", MIN_PIXELS_QWEN3 if q3 else MIN_PIXELS))
        hi = int(self.model_config.get("max_pixels", MAX_PIXELS_QWEN3 if q3 else MAX_PIXELS))
        patch = 16 if q3 else 14
        sizes = [smart_resize(a.shape[0], a.shape[1], 2 * patch, lo, hi) for a in rgb]
        grid = np.array([[1, oh // patch, ow // patch] for oh, ow in sizes], np.int64)
        text = chat_text(self._build_prompt() if prompt is None else prompt, self.family)
        rows = [list(self.encode(expand_image_pads(text, g[None]))) for g in grid]
        ids, am = left_pad(rows, self.tokens["pad_token_id"])
        img = self.tokens["image_token_id"]
        pos, _ = rope_index(ids, grid, img, attention_mask=am)
        image_rows = np.flatnonzero(((ids == img) & (am == 1)).reshape(-1)).astype(np.int32)
        return dict(rgb=rgb, sizes=sizes, grid_thw=grid, input_ids=ids, attention_mask=am, position_ids=pos, image_rows=image_rows)

    def generate_from_images(self, images, max_new_tokens: Optional[int] = None, prompt: Optional[str] = None, return_logprobs: bool = False):
        """Greedy generation for a list of photos (any sizes): preprocessing and the vision tower on the GPU from uint8 pixels, one
        left-padded batch through the decoder. -> int [n, max_new_tokens] or, with return_logprobs, (ids, log-probs float32 [n,
        max_new_tokens], NaN after a row's first EOS). An EngineCapacityError means the batch did not fit."""
        if self.model is None:
            raise RuntimeError("VLMTagger.load() first")
        x = self.prepare_inputs(images, prompt)
        if self.family == "qwen3":
            self.engine.vlm_preprocess_rgb(x["rgb"], x["sizes"], IMAGE_MEAN_QWEN3, IMAGE_STD_QWEN3)
            side = self.engine.vlm_vision_dims()["pos_side"]
            if side <= 0:
                raise ValueError("the committed tower's position table is not a square grid")
            v = vision_inputs_qwen3(x["grid_thw"], side)
            self.engine.vlm3_encode_images(None, v["patch_pos_hw"], v["interp_idx"], v["interp_w"], v["cu_seqlens"], want_embeds=False)
        else:
            self.engine.vlm_preprocess_rgb(x["rgb"], x["sizes"], IMAGE_MEAN, IMAGE_STD)
            idx = vision_indices(x["grid_thw"])
            self.engine.vlm_encode_preprocessed(idx["patch_pos_hw"], idx["window_index"], idx["cu_window_seqlens"], idx["cu_seqlens"], want_embeds=False)
        n_new = int(max_new_tokens or self.model_config.get("max_new_tokens", 100))
        return self.engine.vlm_generate(x["input_ids"], n_new, position_ids=x["position_ids"], eos_token_ids=self.tokens["eos_token_ids"],
                                        image_rows=x["image_rows"], attention_mask=x["attention_mask"], return_logprobs=return_logprobs)

    def _texts(self, generated_ids) -> List[str]:
        """Each row cut at its first EOS id, then the tokenizer's decode."""
        if self.decode is None:
            raise RuntimeError("no tokenizer: pass decode= (processor.decode of the checkpoint, skip_special_tokens=True)")
        eos = [int(e) for e in self.tokens["eos_token_ids"]]
        out = []
        for row in np.asarray(generated_ids):
            hit = np.flatnonzero(np.isin(row, eos))
            out.append(self.decode([int(t) for t in row[:hit[0] if hit.size else len(row)]]))
        return out

    def tag_image(self, image, max_tags: int = 5) -> List[str]:
        """Tags of one photo (PIL image of any mode and size)."""
        return self._parse_tags(self._texts(self.generate_from_images([image]))[0], max_tags)

    def _tag_sub_batch(self, images, max_tags: int) -> List[List[str]]:
        if len(images) == 1:
            return [self.tag_image(images[0], max_tags)]
        return [self._parse_tags(t, max_tags) for t in self._texts(self.generate_from_images(images))]

    def tag_batch(self, images, max_tags: int = 5) -> List[List[str]]:
        """Tags of every photo, in order: sub-batches of vlm_batch_size as one left-padded batch each; a sub-batch that does not fit the
        engine (EngineCapacityError, the engine's out-of-memory) is retried one image at a time, and an image that still does not fit
        gets [] (reference :297-306). Every other error propagates."""
        results: List[List[str]] = []
        for i in range(0, len(images), self.batch_size):
            sub = images[i:i + self.batch_size]
            try:
                results.extend(self._tag_sub_batch(sub, max_tags))
            except EngineCapacityError:
                for im in sub:
                    try:
                        results.append(self.tag_image(im, max_tags))
                    except EngineCapacityError:
                        results.append([])
        return results

    # -- confidence scores (reference :497-626) -----------------------------------------------------------------------------------------
    def _scored_tags(self, ids_row, lp_row, max_tags: int) -> Dict[str, float]:
        """One generated row and its log-probs -> {tag: confidence}: the row up to and including its first EOS, its text, _parse_tags,
        tag_confidences."""
        if self.decode is None:
            raise RuntimeError("no tokenizer: pass decode= (processor.decode of the checkpoint, skip_special_tokens=True)")
        ids_row = np.asarray(ids_row)
        hit = np.flatnonzero(np.isin(ids_row, [int(e) for e in self.tokens["eos_token_ids"]]))
        n = int(hit[0]) + 1 if hit.size else len(ids_row)
        gen = [int(t) for t in ids_row[:n]]
        tags = self._parse_tags(self.decode(gen), max_tags)
        if not tags:
            return {}
        return tag_confidences(gen, [float(v) for v in np.asarray(lp_row)[:n]], tags, lambda t: self.decode([t]))

    def tag_image_with_scores(self, image, max_tags: int = 5) -> Dict[str, float]:
        """Tags of one photo with confidences in [0, 1]: exp of the mean log-probability of each tag's tokens (the greedy tokens'
        log-probs come from the decoder's selection pass on the device; see tag_confidences for the split into tags)."""
        ids, lps = self.generate_from_images([image], return_logprobs=True)
        return self._scored_tags(ids[0], lps[0], max_tags)

    def get_tags_with_scores(self, image, threshold: float = 0.0) -> Dict[str, float]:
        """tag_image_with_scores with its default max_tags; a threshold > 0 keeps the tags whose confidence is >= threshold."""
        scores = self.tag_image_with_scores(image)
        if threshold > 0:
            scores = {tag: conf for tag, conf in scores.items() if conf >= threshold}
        return scores

    def tag_batch_with_scores(self, images, max_tags: int = 5) -> List[Dict[str, float]]:
        """facet_amd extension (the reference scores one photo at a time): tag_image_with_scores for every photo, in order, with
        sub-batches of vlm_batch_size run as one left-padded batch each. A row has the tags tag_image_with_scores gives that photo alone;
        its confidences agree to within the batch's rounding of the logits. A sub-batch that does not fit the engine (EngineCapacityError)
        is retried one image at a time, and an image that still does not fit gets {} (as tag_batch)."""
        results: List[Dict[str, float]] = []
        for i in range(0, len(images), self.batch_size):
            sub = images[i:i + self.batch_size]
            try:
                if len(sub) == 1:
                    results.append(self.tag_image_with_scores(sub[0], max_tags))
                else:
                    ids, lps = self.generate_from_images(sub, return_logprobs=True)
                    results.extend(self._scored_tags(r, lp, max_tags) for r, lp in zip(ids, lps))
            except EngineCapacityError:
                for im in sub:
                    try:
                        results.append(self.tag_image_with_scores(im, max_tags))
                    except EngineCapacityError:
                        results.append({})
        return results

    def tags_from_ids(self, generated_ids, max_tags: int = 5) -> List[List[str]]:
        """Generated ids -> text (the checkpoint's tokenizer) -> vocabulary tags."""
        if self.decode is None:
            raise RuntimeError("no tokenizer: pass decode= (processor.batch_decode of the checkpoint)")
        return [self._parse_tags(self.decode(row), max_tags) for row in np.asarray(generated_ids)]

    # -- parsing (reference :446-495) ---------------------------------------------------------------------------------------------------
    def _parse_tags(self, text: str, max_tags: int) -> List[str]:
        text = text.strip()
        for lead in ("Tags:", "tags:", "Here are the tags:", "The tags are:"):      # applied in this order, each at most once
            if text.startswith(lead):
                text = text[len(lead):].strip()
        found: List[str] = []
        for piece in text.split(","):
            tag = piece.strip().lower().lstrip("0123456789.-) ").strip("\"'")
            if ":" in tag:                                  # a category the model echoed ("art: painting")
                tag = tag.split(":", 1)[1].strip()
            tag = tag.replace(" ", "_")
            if len(tag) <= 1:
                continue
            if self.valid_tags and tag not in self.valid_tags:
                best, best_d = None, 3                      # accept a vocabulary tag within edit distance 2; first best in set order
                for cand in self.valid_tags:
                    d = edit_distance(tag, cand)
                    if d < best_d:
                        best, best_d = cand, d
                if best is not None:
                    tag = best
            if tag not in found:
                found.append(tag)
        return found[:max_tags]
