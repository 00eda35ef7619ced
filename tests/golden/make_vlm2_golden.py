"""Golden vectors for the Qwen2-VL composition analyzer (the 24gb profile's qwen2-vl-2b) from the reference's own model class.

models/model_manager.py:96-125 loads `Qwen2VLForConditionalGeneration`; models/vlm_composition.py runs `generate(**inputs, max_new_tokens=256,
do_sample=False)` on one chat prompt per photo. This script builds that class from a reduced config - decoder: 4 layers, hidden 768, 6
heads over 1 KV head of 128 (the GQA group of 6 of the 2B checkpoint), inter 1408, sectioned M-RoPE [16, 24, 24]; vision tower: 4 blocks of
2 heads x 80, mlp_ratio 4, quick_gelu, 14-pixel patches - with the seeded `qwen2_vl_tiny` weights of facet_amd/weights.py. The planted
read-out of make_vlm3_golden.py (lm_head = a permutation of the embeddings / 16) gives greedy ids with wide margins; the unplanted
checkpoint is TIED (no lm_head.weight) and gives the per-step logits. Stored:
  - the tower on grids 10 x 12 and 6 x 6: merged embeddings, with their sdpa-vs-eager spread;
  - one image prompt: decoder-input position ids, planted greedy ids, tied per-step logits and their teacher-forced sdpa-vs-eager spread;
  - a short image prompt (16 rows: the decoder's split-K prefill route) with its tied per-step logits, greedy ids and spread;
  - a left-padded 3-prompt batch (pads 0, > 32, > 128): position ids, planted ids, tied ids, logits and spread;
  - a photo batch: three PIL images of different sizes and modes through Qwen2VLImageProcessorPil (small min / max pixels), the composition
    chat text with the stand-in tokenizer (standins/vlm_tokenizer.py), left-padded; its pixel_values and planted greedy ids.
Reproducible across x86 hosts: torch's CPU kernels are pinned to their portable forms (ATEN_CPU_CAPABILITY=default, oneDNN off) before torch
loads, so no AVX-512 / AMX bf16 kernel decides a rounding; one thread.
    python tests/golden/make_vlm2_golden.py
"""
import os
import sys

os.environ["ATEN_CPU_CAPABILITY"] = "default"
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.backends.mkldnn.enabled = False
torch.set_num_threads(1)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from facet_amd.weights import synthetic_state_dict, VLM2_TINY, VLM2_VISION_TINY  # noqa: E402

OUT = os.path.join(HERE, "vlm2_golden.npz")
IMG, VSTART, VEND, PAD_ID = 2000, 2002, 2003, 0
VIS_HEADS, MROPE = 2, [16, 24, 24]
PHOTO_MIN_PIXELS, PHOTO_MAX_PIXELS = 56 * 56, 112 * 112
PD = 1176


def planted(seed):
    sd = synthetic_state_dict("qwen2_vl_tiny_untied", seed)
    perm = np.random.default_rng([seed, 77]).permutation(VLM2_TINY["vocab"])
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    return sd


def build(seed, attn="sdpa", plant=True):
    from transformers import Qwen2VLForConditionalGeneration, Qwen2VLConfig
    c, v = VLM2_TINY, VLM2_VISION_TINY
    cfg = Qwen2VLConfig(
        text_config=dict(hidden_size=c["hidden"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"], num_key_value_heads=c["kv_heads"],
                         intermediate_size=c["inter"], vocab_size=c["vocab"], rms_norm_eps=1e-6, max_position_embeddings=4096,
                         rope_parameters={"rope_theta": 1000000.0, "rope_type": "default", "mrope_section": MROPE}),
        vision_config=dict(depth=v["depth"], embed_dim=v["hidden"], hidden_size=v["out_hidden"], mlp_ratio=v["inter"] // v["hidden"], num_heads=VIS_HEADS,
                           patch_size=14, spatial_merge_size=2, temporal_patch_size=2, hidden_act="quick_gelu"),
        image_token_id=IMG, video_token_id=2001, vision_start_token_id=VSTART, vision_end_token_id=VEND, tie_word_embeddings=not plant)
    assert c["hidden"] // c["heads"] == 128
    cfg._attn_implementation = attn
    cfg.vision_config._attn_implementation = attn
    cfg.text_config._attn_implementation = attn
    m = Qwen2VLForConditionalGeneration(cfg).eval()
    sd = planted(seed) if plant else synthetic_state_dict("qwen2_vl_tiny", seed)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(val) for k, val in sd.items()}, strict=False)
    assert not unexpected, unexpected[:4]
    assert all(k == "lm_head.weight" for k in missing) and (plant or missing), missing[:4]
    m = m.to(torch.bfloat16)
    if not plant:
        assert m.lm_head.weight.data_ptr() == m.model.language_model.embed_tokens.weight.data_ptr()
    return m


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


def forced_spread(seed, ids, am, pv, grid, toks):
    """The reference's own implementation spread on teacher-forced logits: one forward pass of the prompt + the forced ids through the tied
    checkpoint with sdpa and with eager attention, max |difference| over the positions that predict the generated tokens."""
    n = toks.shape[1]
    full = np.concatenate([ids, toks[:, :-1].astype(ids.dtype)], 1)
    fam = np.concatenate([am, np.ones((ids.shape[0], n - 1), am.dtype)], 1)
    lg = []
    for attn in ("sdpa", "eager"):
        m = build(seed, attn, plant=False)
        with torch.no_grad():
            o = m(input_ids=torch.from_numpy(full), attention_mask=torch.from_numpy(fam), pixel_values=torch.from_numpy(pv), image_grid_thw=torch.from_numpy(grid),
                  mm_token_type_ids=torch.from_numpy((full == IMG).astype(np.int32)))
        lg.append(o.logits[:, -n:].float().numpy())
    return np.float32(np.abs(lg[0] - lg[1]).max())


def padded_prompts(rng, grid):
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


def main():
    torch.manual_seed(0)
    seed, NEW, BATCH_NEW = 16, 12, 25
    out = {}
    # -- the tower on two images (grids 10 x 12 and 6 x 6 patches) -------------------------------------------------------------------------
    grid = np.array([[1, 10, 12], [1, 6, 6]], np.int64)
    n_patches = int((grid[:, 0] * grid[:, 1] * grid[:, 2]).sum())
    pv = np.random.default_rng(5).normal(0, 1, (n_patches, PD)).astype(np.float32)
    g_t = torch.from_numpy(grid)
    vis = {}
    for attn in ("sdpa", "eager"):
        m = build(seed, attn)
        with torch.no_grad():
            vis[attn] = m.model.visual(torch.from_numpy(pv).to(torch.bfloat16), grid_thw=g_t).pooler_output.float().numpy()
    e_s, e_e = vis["sdpa"], vis["eager"]
    out.update(vis_grid_thw=grid.astype(np.int32), vis_pixel_seed=np.int32(5), embeds=e_s, spread_embeds=np.float32(np.abs(e_s - e_e).max()))
    print(f"embeds {e_s.shape} |max| {np.abs(e_s).max():.3f} spread {out['spread_embeds']:.4f}")
    # -- one image prompt ------------------------------------------------------------------------------------------------------------------
    n_img = [int(g[1] * g[2] // 4) for g in grid]
    ids = np.array([[5, 6, VSTART] + [IMG] * n_img[0] + [VEND, 7, 8, 9, VSTART] + [IMG] * n_img[1] + [VEND, 11, 12]], np.int64)
    am = np.ones_like(ids)
    tp, lp, pos = run(build(seed), ids, am, pv, grid, NEW)
    tp_e, _, _ = run(build(seed, "eager"), ids, am, pv, grid, NEW)
    assert np.array_equal(tp, tp_e)
    top2 = np.sort(lp, -1)[..., -2:]
    print("planted", tp.tolist(), "margin min", float((top2[..., 1] - top2[..., 0]).min()))
    tu, lu, _ = run(build(seed, plant=False), ids, am, pv, grid, NEW)
    top2 = np.sort(lu, -1)[..., -2:]
    print("tied |max|", float(np.abs(lu).max()), "margin min", float((top2[..., 1] - top2[..., 0]).min()))
    out.update(input_ids=ids.astype(np.int32), position_ids=pos, tokens_planted=tp, tokens_unplanted=tu, logits_unplanted=lu.astype(np.float32),
               spread_logits=forced_spread(seed, ids, am, pv, grid, tu))
    # -- a short prompt: 16 rows take the decoder's split-K prefill route ---------------------------------------------------------------------
    sgrid = np.array([[1, 4, 4]], np.int64)
    spv = np.random.default_rng(11).normal(0, 1, (16, PD)).astype(np.float32)
    sids = np.array([[5, 6, 7, VSTART] + [IMG] * 4 + [VEND, 8, 9, 10, 11, 12, 13, 14]], np.int64)
    assert sids.shape[1] == 16
    stu, slu, spos = run(build(seed, plant=False), sids, np.ones_like(sids), spv, sgrid, NEW)
    out.update(short_grid_thw=sgrid.astype(np.int32), short_pixel_seed=np.int32(11), short_input_ids=sids.astype(np.int32), short_position_ids=spos,
               short_tokens_unplanted=stu, short_logits_unplanted=slu.astype(np.float32),
               spread_short_logits=forced_spread(seed, sids, np.ones_like(sids), spv, sgrid, stu))
    # -- a left-padded batch of three single-image prompts (25 planted ids: tests/test_vlm_until_gpu.py stops inside them) -----------------
    bgrid = np.array([[1, 10, 12], [1, 6, 8], [1, 4, 4]], np.int64)
    bn = int((bgrid[:, 0] * bgrid[:, 1] * bgrid[:, 2]).sum())
    bpv = np.random.default_rng(9).normal(0, 1, (bn, PD)).astype(np.float32)
    bids, bam = padded_prompts(np.random.default_rng(3), bgrid)
    pad = (bam == 0).sum(1)
    assert pad.min() == 0 and (pad > 32).any() and (pad > 128).any(), pad
    btp, blp, bpos = run(build(seed), bids, bam, bpv, bgrid, BATCH_NEW)
    top2 = np.sort(blp, -1)[..., -2:]
    print("batch planted margin min", float((top2[..., 1] - top2[..., 0]).min()))
    # the stop test's condition: with the ids rows 0 / 1 / 2 emit at decode steps 3 / 6 / 9 as EOS ids, every row's first hit is <= step 12
    steps = btp[:, 1:]
    eos = [int(steps[0, 3]), int(steps[1, 6]), int(steps[2, 9])]
    first = [int(np.flatnonzero(np.isin(np.concatenate([btp[b, :1], steps[b]]), eos))[0]) - 1 for b in range(3)]
    print("until: eos", eos, "first hits (decode step)", first)
    assert max(first) <= 12 and max(first) >= 4, first
    btu, blu, bpos_u = run(build(seed, plant=False), bids, bam, bpv, bgrid, NEW)
    assert np.array_equal(bpos, bpos_u)
    spread_batch = forced_spread(seed, bids, bam, bpv, bgrid, btu)
    print("batch pads", pad.tolist(), "planted", btp.tolist())
    out.update(batch_grid_thw=bgrid.astype(np.int32), batch_pixel_seed=np.int32(9), batch_input_ids=bids.astype(np.int32), batch_attention_mask=bam.astype(np.int32),
               batch_position_ids=bpos, batch_tokens_planted=btp, batch_tokens_unplanted=btu, batch_logits_unplanted=blu.astype(np.float32),
               spread_batch_logits=spread_batch)
    # -- photos --------------------------------------------------------------------------------------------------------------------------------
    from PIL import Image
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil
    from facet_amd.vlm_tagger import chat_text, expand_image_pads, left_pad
    from facet_amd.vlm_composition import VLMCompositionAnalyzer
    from standins import vlm_tokenizer as T
    rng = np.random.default_rng(21)
    photos = [rng.integers(0, 256, (60, 80, 3), dtype=np.uint8), rng.integers(0, 256, (120, 100, 3), dtype=np.uint8),
              rng.integers(0, 256, (40, 150, 4), dtype=np.uint8)]
    pil = [Image.fromarray(a, "RGBA" if a.shape[2] == 4 else "RGB") for a in photos]
    proc = Qwen2VLImageProcessorPil(size={"shortest_edge": PHOTO_MIN_PIXELS, "longest_edge": PHOTO_MAX_PIXELS})
    r = proc(images=pil, return_tensors="np")
    ppv, pgrid = np.asarray(r["pixel_values"], np.float32), np.asarray(r["image_grid_thw"], np.int64)
    assert ppv.shape[1] == PD, ppv.shape
    text = chat_text(VLMCompositionAnalyzer.COMPOSITION_PROMPT, "qwen2_5")
    pids, pam = left_pad([T.encode(expand_image_pads(text, g[None])) for g in pgrid], T.TOKENS["pad_token_id"])
    pids, pam = pids.astype(np.int64), pam.astype(np.int64)
    print("photo grids", pgrid.tolist(), "len", pids.shape[1], "pads", (pam == 0).sum(1).tolist())
    ptoks, plp, ppos = run(build(seed), pids, pam, ppv, pgrid, NEW, T.TOKENS["pad_token_id"])
    top2 = np.sort(plp, -1)[..., -2:]
    print("photo planted margin min", float((top2[..., 1] - top2[..., 0]).min()))
    out.update({f"photo_{i}": a for i, a in enumerate(photos)})
    out.update(photo_grid_thw=pgrid.astype(np.int32), photo_pixel_values=ppv, photo_input_ids=pids.astype(np.int32), photo_attention_mask=pam.astype(np.int32),
               photo_position_ids=ppos, photo_tokens=ptoks, photo_min_pixels=np.int32(PHOTO_MIN_PIXELS), photo_max_pixels=np.int32(PHOTO_MAX_PIXELS))
    print("teacher-forced sdpa-vs-eager spread: single", out["spread_logits"], "short", out["spread_short_logits"], "batch", out["spread_batch_logits"])
    out.update(seed_w=np.int32(seed), vis_heads=np.int32(VIS_HEADS), mrope_section=np.asarray(MROPE, np.int32), image_token_id=np.int32(IMG),
               pad_token_id=np.int32(PAD_ID))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
