"""GPU: the Qwen2-VL composition analyzer (fe_vlm2_configure, fe_vlm2_encode_images, the Qwen2.5 decoder with a tied head at GQA group 6
behind fe_vlm_prefill_images(_padded) / fe_vlm_generate) against tests/golden/vlm2_golden.npz - transformers'
Qwen2VLForConditionalGeneration at a reduced config (tests/golden/make_vlm2_golden.py). Reads only tests/golden/.

  * vision tower: merged embeddings within 3x the reference's own sdpa-vs-eager spread (floor 0.03); an fc1 bias set to zero changes them
    (the QuickGELU branch is live);
  * planted checkpoint: greedy ids identical for one image prompt, a left-padded 3-prompt batch (pads 0 / 106 / 190) and the photos;
  * tied checkpoint (no lm_head.weight, and the torch form that keeps it), teacher-forced: every step's logits within max(0.0625, twice the
    reference's own sdpa-vs-eager spread on the same logits) for the image prompt, a 16-row prompt (split-K prefill route) and the batch;
  * every padded row equals its alone run; fe_vlm_preprocess_rgb rows equal the processor's bit for bit;
  * analyze_composition / batch_analyze on the photos return the dict the host parse gives for the decoded planted ids; a photo whose
    prompt exceeds the engine's positions returns the failure dict;
  * loading Qwen2.5-VL after Qwen2-VL restores its golden's ids.
"""
import os

import numpy as np
import pytest
from PIL import Image

from facet_amd._lib import FE_MODEL_VLM
from facet_amd.vlm_composition import Qwen2VLModel, Qwen2VLProcessor, VLMCompositionAnalyzer
from facet_amd.vlm_tagger import IMAGE_MEAN, IMAGE_STD, rope_index, vision_inputs_qwen2
from facet_amd.weights import synthetic_state_dict, VLM2_TINY

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
G = np.load(os.path.join(HERE, "golden", "vlm2_golden.npz"))
IMG = int(G["image_token_id"])
TOL = 0.0625
SEED = int(G["seed_w"])
GEOM = dict(n_heads=VLM2_TINY["heads"], n_kv_heads=VLM2_TINY["kv_heads"], head_dim=128, rope_theta=1e6, rms_eps=1e-6,
            mrope_section=tuple(int(v) for v in G["mrope_section"]), vis_heads=int(G["vis_heads"]))


def _planted():
    sd = synthetic_state_dict("qwen2_vl_tiny_untied", SEED)
    perm = np.random.default_rng([SEED, 77]).permutation(VLM2_TINY["vocab"])
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    return sd


def _tied():
    sd = synthetic_state_dict("qwen2_vl_tiny", SEED)
    assert "lm_head.weight" not in sd
    return sd


@pytest.fixture()
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=4 << 30)
    e.vlm2_configure(**GEOM)
    yield e
    e.close()


def _pixels(grid, seed):
    n = int((grid[:, 0] * grid[:, 1] * grid[:, 2]).sum())
    return np.random.default_rng(seed).normal(0, 1, (n, 1176)).astype(np.float32)


def _encode(e, pv, grid, want=False):
    v = vision_inputs_qwen2(grid)
    return e.vlm2_encode_images(pv, v["patch_pos_hw"], v["cu_seqlens"], want_embeds=want)


def _single(e):
    grid = G["vis_grid_thw"]
    _encode(e, _pixels(grid, int(G["vis_pixel_seed"])), grid)
    ids = G["input_ids"]
    pos, _ = rope_index(ids, grid, IMG)
    return ids, pos, np.flatnonzero(ids.reshape(-1) == IMG).astype(np.int32)


def test_vision_tower_embeddings_within_the_reference_spread_and_quick_gelu_is_live(eng):
    eng.load_weights(FE_MODEL_VLM, _planted())
    assert eng.vlm_vision_dims() == {"patch": 14, "patch_dim": 1176, "n_deepstack": 0, "pos_side": 0}
    grid = G["vis_grid_thw"]
    pv = _pixels(grid, int(G["vis_pixel_seed"]))
    emb = _encode(eng, pv, grid, want=True)
    assert np.isfinite(emb).all() and emb.shape == G["embeds"].shape
    bound = max(3 * float(G["spread_embeds"]), 0.03)
    err = np.abs(emb - G["embeds"]).max()
    print("embedding error", err, "bound", bound)
    assert err <= bound, (err, bound)
    # fc1's bias shifts the argument of the activation: zeroing it must move the embeddings (a dropped activation input would not). The
    # reference class itself moves by 0.164 (max) for these weights; 0.03 is the project's floor for a difference that is not rounding
    # (two bf16 ulps at the embeddings' scale, the floor of `bound` above)
    eng.unload(FE_MODEL_VLM)
    sd = _planted()
    for i in range(4):
        sd[f"model.visual.blocks.{i}.mlp.fc1.bias"][:] = 0
    eng.vlm2_configure(**GEOM)
    eng.load_weights(FE_MODEL_VLM, sd)
    zeroed = _encode(eng, pv, grid, want=True)
    assert np.abs(zeroed - emb).max() > 0.03, np.abs(zeroed - emb).max()


def test_planted_greedy_ids_identical_one_image_prompt(eng):
    eng.load_weights(FE_MODEL_VLM, _planted())
    ids, pos, rows = _single(eng)
    assert np.array_equal(pos, G["position_ids"])
    want = G["tokens_planted"]
    got = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows)
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("keep_head", [False, True])
def test_tied_checkpoint_teacher_forced_logits_within_tolerance(eng, keep_head):
    sd = _tied()
    if keep_head:      # a torch state dict keeps the shared tensor under both names
        sd["lm_head.weight"] = sd["model.language_model.embed_tokens.weight"].copy()
    eng.load_weights(FE_MODEL_VLM, sd)
    ids, pos, rows = _single(eng)
    want = G["logits_unplanted"]
    _, lg = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows, want_logits=True, forced_tokens=G["tokens_unplanted"])
    assert np.isfinite(lg).all()
    bound = max(TOL, 2 * float(G["spread_logits"]))
    err = np.abs(lg - want).max()
    print("logit error", err, "bound", bound)
    assert err <= bound, (err, bound)


def test_short_prompt_split_k_route_logits(eng):
    eng.load_weights(FE_MODEL_VLM, _tied())
    grid = G["short_grid_thw"]
    _encode(eng, _pixels(grid, int(G["short_pixel_seed"])), grid)
    ids = G["short_input_ids"]
    pos, _ = rope_index(ids, grid, IMG)
    assert np.array_equal(pos, G["short_position_ids"]) and ids.size <= 32
    want = G["short_logits_unplanted"]
    _, lg = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=np.flatnonzero(ids.reshape(-1) == IMG).astype(np.int32),
                             want_logits=True, forced_tokens=G["short_tokens_unplanted"])
    assert np.isfinite(lg).all()
    bound = max(TOL, 2 * float(G["spread_short_logits"]))
    print("short logit error", np.abs(lg - want).max(), "bound", bound)
    assert np.abs(lg - want).max() <= bound, (np.abs(lg - want).max(-1), bound)


def _batch(e, order):
    """Prompts `order` (indices into the golden batch) as one left-padded batch, their images encoded in that order."""
    grid_all, ids_all, am_all = G["batch_grid_thw"], G["batch_input_ids"], G["batch_attention_mask"]
    pv_all = _pixels(grid_all, int(G["batch_pixel_seed"]))
    off = np.concatenate([[0], np.cumsum(grid_all.prod(1))])
    rows_ = [ids_all[i][am_all[i] == 1] for i in order]
    L = max(len(r) for r in rows_)
    ids = np.zeros((len(order), L), np.int32)
    am = np.zeros((len(order), L), np.int32)
    for b, r in enumerate(rows_):
        ids[b, L - len(r):] = r
        am[b, L - len(r):] = 1
    grid = grid_all[list(order)]
    _encode(e, np.concatenate([pv_all[off[i]:off[i + 1]] for i in order]), grid)
    pos, _ = rope_index(ids, grid, IMG, attention_mask=am)
    image_rows = np.flatnonzero(((ids == IMG) & (am == 1)).reshape(-1)).astype(np.int32)
    return ids, am, pos, image_rows


def test_padded_batch_planted_greedy_ids_identical(eng):
    eng.load_weights(FE_MODEL_VLM, _planted())
    ids, am, pos, rows = _batch(eng, [0, 1, 2])
    assert np.array_equal(ids, G["batch_input_ids"]) and np.array_equal(pos, G["batch_position_ids"])
    want = G["batch_tokens_planted"]
    got = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows, attention_mask=am)
    assert np.array_equal(got, want), (got, want)


def test_padded_batch_tied_teacher_forced_logits(eng):
    eng.load_weights(FE_MODEL_VLM, _tied())
    ids, am, pos, rows = _batch(eng, [0, 1, 2])
    want = G["batch_logits_unplanted"]
    _, lg = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows, attention_mask=am, want_logits=True,
                             forced_tokens=G["batch_tokens_unplanted"])
    assert np.isfinite(lg).all()
    err = np.abs(lg - want).max(-1)      # [sequence, step]
    bound = max(TOL, 2 * float(G["spread_batch_logits"]))
    print("batch logit error", err.max(), "bound", bound)
    assert err.max() <= bound, (err, bound)


@pytest.mark.parametrize("order", [[2, 0], [0, 1, 2], [1, 2, 0, 2, 1]])
def test_each_padded_row_equals_its_alone_run(eng, order):
    eng.load_weights(FE_MODEL_VLM, _planted())
    n_new = 8
    alone = {}
    for i in sorted(set(order)):
        ids, am, pos, rows = _batch(eng, [i])
        alone[i] = eng.vlm_generate(ids, n_new, position_ids=pos, image_rows=rows)[0]
    ids, am, pos, rows = _batch(eng, order)
    got = eng.vlm_generate(ids, n_new, position_ids=pos, image_rows=rows, attention_mask=am)
    for b, i in enumerate(order):
        assert np.array_equal(got[b], alone[i]), (order, b, got[b], alone[i])


def _photos():
    return [Image.fromarray(G[f"photo_{i}"], "RGBA" if G[f"photo_{i}"].shape[2] == 4 else "RGB") for i in range(3)]


def _analyzer(e, max_pixels=None, load=True):
    from standins import vlm_tokenizer as T
    proc = Qwen2VLProcessor(T.encode, T.decode, int(G["photo_min_pixels"]), int(max_pixels or G["photo_max_pixels"]), special_tokens=T.TOKENS)
    model = Qwen2VLModel(e, _planted(), GEOM)
    if load:
        model.to("cuda")
    return VLMCompositionAnalyzer({"model": model, "processor": proc}, max_tokens=G["photo_tokens"].shape[1], vlm_batch_size=4)


def test_preprocess_rgb_rows_equal_the_processor(eng):
    a = _analyzer(eng)
    x = a.prepare_inputs(_photos())
    pv = eng.vlm_preprocess_rgb(x["rgb"], x["sizes"], IMAGE_MEAN, IMAGE_STD, want_pixel_values=True)
    want = G["photo_pixel_values"]
    assert pv.shape == want.shape == (want.shape[0], 1176)
    assert np.array_equal(pv.view(np.uint32), want.view(np.uint32)), np.abs(pv - want).max()


def test_analyze_and_batch_analyze_on_photos_return_the_reference_parse(eng):
    a = _analyzer(eng)
    photos = _photos()
    ids = a.generate_from_images(photos)
    eos = a.processor.tokens["eos_token_ids"]
    want_ids = G["photo_tokens"].copy()
    for row in want_ids:      # the stop-at-EOS loop pads a finished row with its EOS id, as generate does
        hit = np.flatnonzero(np.isin(row, eos))
        if hit.size:
            row[hit[0]:] = row[hit[0]]
    assert np.array_equal(ids, want_ids), (ids, want_ids)
    want = [a._parse_response(t) for t in a._texts(G["photo_tokens"])]
    assert all(set(w) == {"composition_score", "explanation", "elements"} for w in want)
    assert a.batch_analyze(photos) == want
    assert [a.analyze_composition(p) for p in photos[:2]] == want[:2]


def test_over_capacity_photo_returns_the_failure_dict(eng):
    a = _analyzer(eng, max_pixels=28 * 28 * 16384, load=False)      # 2800 x 3360 -> 200 x 240 patches -> 12000 image tokens > 8192 positions
    big = Image.fromarray(np.zeros((2800, 3360, 3), np.uint8))
    r = a.analyze_composition(big)
    assert r["composition_score"] == 5.0 and r["elements"] == {} and r["explanation"].startswith("Analysis error: ") and "8192" in r["explanation"]
    assert a.batch_analyze([big, big]) == [r, r]


def test_qwen2_5_after_qwen2_restores_its_golden_ids(eng):
    from facet_amd.weights import VLM_TINY
    eng.load_weights(FE_MODEL_VLM, _planted())
    ids, pos, rows = _single(eng)
    assert np.array_equal(eng.vlm_generate(ids, 4, position_ids=pos, image_rows=rows), G["tokens_planted"][:, :4])
    eng.unload(FE_MODEL_VLM)
    g = np.load(os.path.join(HERE, "golden", "vlm_golden.npz"))
    eng.vlm_configure(n_heads=VLM_TINY["heads"], n_kv_heads=VLM_TINY["kv_heads"], head_dim=128, rope_theta=float(g["rope_theta"]),
                      rms_eps=float(g["rms_eps"]), mrope_section=[int(v) for v in g["mrope_section"]])
    seed = int(g["seed_w"])
    sd = synthetic_state_dict("qwen2_5_vl_text_tiny", seed)      # the planted checkpoint of tests/test_vlm_gpu.py
    perm = np.random.default_rng([seed, 77]).permutation(VLM_TINY["vocab"])
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    eng.load_weights(FE_MODEL_VLM, sd)
    want = g["tokens"]
    got = eng.vlm_generate(g["prompts"], want.shape[1])
    assert np.array_equal(got, want), (got, want)
