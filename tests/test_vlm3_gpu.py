"""GPU: the Qwen3-VL tagger (fe_vlm3_configure, fe_vlm3_encode_images, the Qwen3 decoder behind fe_vlm_prefill_images(_padded) /
fe_vlm_generate) against tests/golden/vlm3_golden.npz - transformers' Qwen3VLForConditionalGeneration at a reduced config
(tests/golden/make_vlm3_golden.py). Reads only tests/golden/; transformers is not imported.

  * vision tower: merged embeddings and every DeepStack feature block within 3x the reference's own sdpa-vs-eager spread (floor 0.03);
  * planted checkpoint: greedy ids identical for one image prompt and for a left-padded 3-prompt batch (pads 0 / 106 / 190);
  * tied unplanted checkpoint (no lm_head.weight), teacher-forced: every step's logits within 0.0625 for one image prompt; for a 16-row
    prompt (the split-K prefill route) and the padded batch within 0.0625 or twice the reference's own sdpa-vs-eager spread on the same
    teacher-forced logits, whichever is larger (stored by the generator: 0.082 and 0.080 there, above 0.0625 at this reduced config);
  * every padded row equals its alone-run at 2 sequences (graph replay) and 3 / 5 (stream launches);
  * the DeepStack injection is live on both prefill routes: zeroed features change the logits;
  * VLMTagger(qwen3).tag_batch on three PIL photos returns the tags the reference's ids decode to, and the GPU patch rows of 16-pixel
    patches equal the processor's pixel_values within one bf16 ulp; no NaN anywhere.
"""
import os

import numpy as np
import pytest
from PIL import Image

from facet_amd._lib import FE_MODEL_VLM
from facet_amd.vlm_tagger import VLMTagger, rope_index, vision_inputs_qwen3
from facet_amd.weights import synthetic_state_dict, VLM3_TINY

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "vlm3_golden.npz"))
IMG = int(G["image_token_id"])
TOL = 0.0625
SEED = int(G["seed_w"])
GEOM = dict(n_heads=VLM3_TINY["heads"], n_kv_heads=VLM3_TINY["kv_heads"], head_dim=128, rope_theta=5e6, rms_eps=1e-6,
            mrope_section=tuple(int(v) for v in G["mrope_section"]), vis_heads=int(G["vis_heads"]),
            deepstack_indexes=tuple(int(v) for v in G["deepstack_indexes"]))
N_DS = len(GEOM["deepstack_indexes"])


def _planted():
    sd = synthetic_state_dict("qwen3_vl_tiny_untied", SEED)
    perm = np.random.default_rng([SEED, 77]).permutation(VLM3_TINY["vocab"])
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    return sd


def _tied():
    sd = synthetic_state_dict("qwen3_vl_tiny", SEED)
    assert "lm_head.weight" not in sd
    return sd


@pytest.fixture()
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=4 << 30)
    e.vlm3_configure(**GEOM)
    yield e
    e.close()


def _pixels(grid, seed):
    n = int((grid[:, 0] * grid[:, 1] * grid[:, 2]).sum())
    return np.random.default_rng(seed).normal(0, 1, (n, 1536)).astype(np.float32)


def _encode(e, pv, grid, want=False):
    v = vision_inputs_qwen3(grid, 8)
    return e.vlm3_encode_images(pv, v["patch_pos_hw"], v["interp_idx"], v["interp_w"], v["cu_seqlens"], want_embeds=want, want_deepstack=want)


def _single(e):
    grid = G["vis_grid_thw"]
    _encode(e, _pixels(grid, int(G["vis_pixel_seed"])), grid)
    ids = G["input_ids"]
    pos, _ = rope_index(ids, grid, IMG)
    rows = np.flatnonzero(ids.reshape(-1) == IMG).astype(np.int32)
    return ids, pos, rows


def test_vision_tower_embeddings_and_deepstack_within_the_reference_spread(eng):
    eng.load_weights(FE_MODEL_VLM, _planted())
    grid = G["vis_grid_thw"]
    emb, ds = _encode(eng, _pixels(grid, int(G["vis_pixel_seed"])), grid, want=True)
    assert np.isfinite(emb).all() and np.isfinite(ds).all()
    bound = max(3 * float(G["spread_embeds"]), 0.03)
    assert np.abs(emb - G["embeds"]).max() <= bound, (np.abs(emb - G["embeds"]).max(), bound)
    assert ds.shape == G["deepstack"].shape
    for k in range(N_DS):
        bk = max(3 * float(G["spread_deepstack"][k]), 0.03)
        assert np.abs(ds[k] - G["deepstack"][k]).max() <= bk, (k, np.abs(ds[k] - G["deepstack"][k]).max(), bk)


def test_planted_greedy_ids_identical_one_image_prompt(eng):
    eng.load_weights(FE_MODEL_VLM, _planted())
    ids, pos, rows = _single(eng)
    want = G["tokens_planted"]
    got = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows)
    assert np.array_equal(got, want), (got, want)


def test_tied_checkpoint_teacher_forced_logits_within_tolerance(eng):
    eng.load_weights(FE_MODEL_VLM, _tied())
    ids, pos, rows = _single(eng)
    want = G["logits_unplanted"]
    toks, lg = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows, want_logits=True, forced_tokens=G["tokens_unplanted"])
    assert np.isfinite(lg).all()
    err = np.abs(lg - want).max()
    assert err <= TOL, err


def test_zeroed_deepstack_features_change_the_logits(eng):
    eng.load_weights(FE_MODEL_VLM, _tied())
    ids, pos, rows = _single(eng)
    _, base = eng.vlm_prefill(ids, pos, want_logits=True, image_rows=rows)
    eng.unload(FE_MODEL_VLM)
    sd = _tied()
    for k in range(N_DS):      # DeepStack mergers whose output is zero: the features added to the image rows vanish
        sd[f"model.visual.deepstack_merger_list.{k}.linear_fc2.weight"][:] = 0
        sd[f"model.visual.deepstack_merger_list.{k}.linear_fc2.bias"][:] = 0
    eng.vlm3_configure(**GEOM)
    eng.load_weights(FE_MODEL_VLM, sd)
    ids, pos, rows = _single(eng)
    _, zeroed = eng.vlm_prefill(ids, pos, want_logits=True, image_rows=rows)
    assert np.isfinite(base).all() and np.isfinite(zeroed).all()
    assert np.abs(base - zeroed).max() > 0.1, np.abs(base - zeroed).max()
    assert np.abs(base - G["logits_unplanted"][:, 0]).max() <= TOL


def _short(e):
    grid = G["short_grid_thw"]
    _encode(e, _pixels(grid, int(G["short_pixel_seed"])), grid)
    ids = G["short_input_ids"]
    pos, _ = rope_index(ids, grid, IMG)
    assert np.array_equal(pos, G["short_position_ids"])
    return ids, pos, np.flatnonzero(ids.reshape(-1) == IMG).astype(np.int32)


def test_short_prompt_split_k_route_logits_and_live_deepstack(eng):
    """16 rows: the prefill takes the split-K route, whose finishing pass adds the DeepStack features (vlm_finish_add_rmsnorm_kernel)."""
    eng.load_weights(FE_MODEL_VLM, _tied())
    ids, pos, rows = _short(eng)
    assert ids.size <= 32
    want = G["short_logits_unplanted"]
    _, lg = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows, want_logits=True, forced_tokens=G["short_tokens_unplanted"])
    assert np.isfinite(lg).all()
    bound = max(TOL, 2 * float(G["spread_short_logits"]))
    assert np.abs(lg - want).max() <= bound, (np.abs(lg - want).max(-1), bound)
    eng.unload(FE_MODEL_VLM)
    sd = _tied()
    for k in range(N_DS):
        sd[f"model.visual.deepstack_merger_list.{k}.linear_fc2.weight"][:] = 0
        sd[f"model.visual.deepstack_merger_list.{k}.linear_fc2.bias"][:] = 0
    eng.vlm3_configure(**GEOM)
    eng.load_weights(FE_MODEL_VLM, sd)
    ids, pos, rows = _short(eng)
    _, zeroed = eng.vlm_prefill(ids, pos, want_logits=True, image_rows=rows)
    assert np.abs(zeroed - want[:, 0]).max() > 0.1, np.abs(zeroed - want[:, 0]).max()


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


def _tagger(e):
    from standins import vlm_tokenizer as T
    tg = VLMTagger({"model_path": "Qwen/Qwen3-VL-2B-Instruct", "max_new_tokens": G["photo_tokens"].shape[1], "vlm_batch_size": 4,
                    "min_pixels": int(G["photo_min_pixels"]), "max_pixels": int(G["photo_max_pixels"])}, engine=e, encode=T.encode, decode=T.decode,
                   special_tokens=T.TOKENS)
    tg.load(_planted(), geometry=GEOM)
    return tg, T


def test_preprocess_rgb_rows_for_16_pixel_patches_equal_the_processor(eng):
    tg, _ = _tagger(eng)
    photos = [G[f"photo_{i}"] for i in range(3)]
    x = tg.prepare_inputs([Image.fromarray(a, "RGBA" if a.shape[2] == 4 else "RGB") for a in photos])
    pv = eng.vlm_preprocess_rgb(x["rgb"], x["sizes"], (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), want_pixel_values=True)
    want = G["photo_pixel_values"]
    assert pv.shape == want.shape == (want.shape[0], 1536)
    ulp = np.maximum(np.abs(want), 2.0 ** -126) * 2.0 ** -7
    assert (np.abs(pv - want) <= ulp).all(), np.abs(pv - want).max()


def test_tag_batch_on_photos_returns_the_reference_tags(eng):
    tg, T = _tagger(eng)
    photos = [Image.fromarray(G[f"photo_{i}"], "RGBA" if G[f"photo_{i}"].shape[2] == 4 else "RGB") for i in range(3)]
    ids = tg.generate_from_images(photos)
    assert np.array_equal(ids, G["photo_tokens"]), (ids, G["photo_tokens"])
    want = [tg._parse_tags(t, 5) for t in tg._texts(G["photo_tokens"])]
    assert tg.tag_batch(photos) == want
