"""Golden vectors for the VLM tagger's PADDED batches (fe_vlm_prefill_images_padded) from the reference's own model class.

models/vlm_tagger.py:327-368 tags a sub-batch of photos with `processor(text=texts, images=images, padding=True)` and `generate(**inputs,
do_sample=False)`: photos of different sizes give prompts of different lengths, padded on the left, with the attention mask passed to
generate. This script builds Qwen2_5_VLForConditionalGeneration as make_vlm_vision_golden.py does (reduced config, seeded `qwen2_5_vl_tiny`
weights) and runs a left-padded batch of three prompts whose images have different grids; the pads are 0, > 32 and > 128 tokens (a whole
32-key prefill tile, a whole 128-key decode chunk). Stored: input_ids, attention_mask, the M-RoPE position ids transformers computed
(captured at the decoder's input), the greedy ids of the planted-read-out checkpoint, and the greedy ids and per-step logits of the
unplanted one (the GPU test teacher-forces those ids). A second batch goes in as PHOTOS: three PIL images of different sizes and modes
through transformers' Qwen2-VL image processor (PIL backend), the tagger's chat text with the stand-in tokenizer of standins/vlm_tokenizer.py
(the checkpoint's tokenizer is not available offline), left-padded; its planted greedy ids are what VLMTagger.tag_batch must reproduce.
Run in the build container:
    python tests/golden/make_vlm_ragged_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_vlm_vision_golden import IMG, VSTART, VEND, VIS_HEADS, FULLATT, build  # noqa: E402
from facet_amd.weights import synthetic_state_dict  # noqa: E402

OUT = os.path.join(HERE, "vlm_ragged_golden.npz")
PAD_ID = 0


def prompts(rng, grid):
    """Three prompts: text, <|vision_start|>, the image's placeholders, <|vision_end|>, text - of very different lengths."""
    text_len = [(30, 160), (12, 90), (6, 20)]
    rows = []
    for (a, b), g in zip(text_len, grid):
        n = int(g[0] * g[1] * g[2] // 4)
        rows.append(list(rng.integers(10, 1990, a)) + [VSTART] + [IMG] * n + [VEND] + list(rng.integers(10, 1990, b)))
    L = max(len(r) for r in rows)
    ids = np.full((3, L), PAD_ID, np.int64)
    am = np.zeros((3, L), np.int64)
    for i, r in enumerate(rows):
        ids[i, L - len(r):] = r
        am[i, L - len(r):] = 1
    return ids, am


def run(m, ids, am, pv, grid, new, pad_id=PAD_ID):
    got = {}

    def grab(mod, args, kwargs):
        if kwargs.get("position_ids") is not None and "pos" not in got:
            got["pos"] = kwargs["position_ids"].clone()
    hook = m.model.language_model.register_forward_pre_hook(grab, with_kwargs=True)
    with torch.no_grad():
        out = m.generate(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(am), pixel_values=torch.from_numpy(pv),
                         image_grid_thw=torch.from_numpy(grid), mm_token_type_ids=torch.from_numpy((ids == IMG).astype(np.int32)), max_new_tokens=new,
                         do_sample=False, output_logits=True, return_dict_in_generate=True, pad_token_id=pad_id, eos_token_id=None)
    hook.remove()
    pos = got["pos"]
    pos = pos[-3:] if pos.shape[0] == 4 else pos
    return out.sequences[:, ids.shape[1]:].numpy().astype(np.int32), torch.stack(out.logits, 1).float().numpy(), pos.numpy().astype(np.int32)


def main():
    seed, NEW = 16, 12
    grid = np.array([[1, 10, 12], [1, 6, 8], [1, 4, 4]], np.int64)
    n_patches = int((grid[:, 0] * grid[:, 1] * grid[:, 2]).sum())
    pv = np.random.default_rng(9).normal(0, 1, (n_patches, 1176)).astype(np.float32)
    ids, am = prompts(np.random.default_rng(3), grid)
    pad = (am == 0).sum(1)
    print("len", ids.shape[1], "pads", pad.tolist())
    assert pad.min() == 0 and (pad > 32).any() and (pad > 128).any()
    toks_p, _, pos = run(build(seed), ids, am, pv, grid, NEW)
    m = build(seed)
    sd = synthetic_state_dict("qwen2_5_vl_tiny", seed)            # the unplanted read-out
    m.load_state_dict({k: torch.from_numpy(v).to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    toks_u, logits_u, pos_u = run(m, ids, am, pv, grid, NEW)
    assert np.array_equal(pos, pos_u)
    print("planted tokens", toks_p.tolist())
    print("unplanted logits |max|", float(np.abs(logits_u).max()))
    # photos: processor pixel values, the tagger's chat text, stand-in token ids
    from PIL import Image
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil
    from facet_amd.vlm_tagger import VLMTagger, chat_text, expand_image_pads, left_pad
    from standins import vlm_tokenizer as T
    rng = np.random.default_rng(21)
    photos = [rng.integers(0, 256, (60, 80, 3), dtype=np.uint8), rng.integers(0, 256, (120, 100, 3), dtype=np.uint8),
              rng.integers(0, 256, (40, 150, 4), dtype=np.uint8)]
    pil = [Image.fromarray(a, "RGBA" if a.shape[2] == 4 else "RGB") for a in photos]
    r = Qwen2VLImageProcessorPil()(images=pil, return_tensors="np")
    ppv, pgrid = np.asarray(r["pixel_values"], np.float32), np.asarray(r["image_grid_thw"], np.int64)
    text = chat_text(VLMTagger._fallback_prompt())
    pids, pam = left_pad([T.encode(expand_image_pads(text, g[None])) for g in pgrid], T.TOKENS["pad_token_id"])
    pids, pam = pids.astype(np.int64), pam.astype(np.int64)
    print("photo grids", pgrid.tolist(), "len", pids.shape[1], "pads", (pam == 0).sum(1).tolist())
    toks_photo, _, _ = run(build(seed), pids, pam, ppv, pgrid, NEW, T.TOKENS["pad_token_id"])
    photo_arrays = {f"photo_{i}": a for i, a in enumerate(photos)}
    np.savez_compressed(OUT, **photo_arrays, photo_grid_thw=pgrid.astype(np.int32), photo_tokens=toks_photo, photo_input_ids=pids.astype(np.int32),
                        seed_w=seed, grid_thw=grid.astype(np.int32), pixel_seed=9, input_ids=ids.astype(np.int32), attention_mask=am.astype(np.int32),
                        position_ids=pos, tokens_planted=toks_p, tokens_unplanted=toks_u, logits_unplanted=logits_u.astype(np.float32),
                        vis_heads=np.int32(VIS_HEADS), fullatt=np.asarray(FULLATT, np.int32), image_token_id=np.int32(IMG), pad_token_id=np.int32(PAD_ID),
                        vision_start_token_id=np.int32(VSTART), vision_end_token_id=np.int32(VEND))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
