"""GPU: left-padded batches through the VLM decoder (fe_vlm_prefill_images_padded, then fe_vlm_decode_step / fe_vlm_generate with the
padding kept), against tests/golden/make_vlm_ragged_golden.py - transformers' Qwen2_5_VLForConditionalGeneration running `generate` on a
left-padded batch with its attention mask, the call models/vlm_tagger.py:327-368 makes for photos of different sizes.

  * planted checkpoint: the greedy ids of a 3-prompt image batch (pads 0 / 106 / 190: whole 32-key prefill tiles and a whole 128-key
    decode chunk of padding) are identical to the reference's;
  * unplanted checkpoint, teacher-forced with the reference's ids: every step's logits within 0.0625 (test_vlm_gpu.py's tolerance);
  * every row of a padded batch generates what that sequence generates alone, for 2 sequences (graph replay) and 3 / 5 (stream launches);
    the pad token id changes nothing; no NaN anywhere;
  * VLMTagger.tag_batch on three PIL photos of different sizes returns the tags the reference's ids decode to.
"""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from facet_amd._lib import FE_MODEL_VLM
from facet_amd.vlm_tagger import VLMTagger, rope_index, vision_indices
from facet_amd.weights import synthetic_state_dict, VLM_TINY

pytestmark = pytest.mark.gpu
R = np.load(os.path.join(os.path.dirname(__file__), "golden", "vlm_ragged_golden.npz"))
IMG = int(R["image_token_id"])
TOL = 0.0625


def _planted(name, seed):
    sd = synthetic_state_dict(name, seed)
    perm = np.random.default_rng([seed, 77]).permutation(VLM_TINY["vocab"])
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    return sd


@pytest.fixture()
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=6 << 30)
    e.vlm_configure(n_heads=VLM_TINY["heads"], n_kv_heads=VLM_TINY["kv_heads"], head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24))
    e.vlm_vision_configure(int(R["vis_heads"]), [int(v) for v in R["fullatt"]])
    yield e
    e.close()


def _image_batch(e):
    grid = R["grid_thw"]
    n_patches = int((grid[:, 0] * grid[:, 1] * grid[:, 2]).sum())
    pv = np.random.default_rng(int(R["pixel_seed"])).normal(0, 1, (n_patches, 1176)).astype(np.float32)
    idx = vision_indices(grid)
    e.vlm_encode_images(pv, idx["patch_pos_hw"], idx["window_index"], idx["cu_window_seqlens"], idx["cu_seqlens"], want_embeds=False)
    ids, am = R["input_ids"], R["attention_mask"]
    pos, _ = rope_index(ids, grid, IMG, attention_mask=am)
    assert np.array_equal(pos, R["position_ids"])
    rows = np.flatnonzero(((ids == IMG) & (am == 1)).reshape(-1)).astype(np.int32)
    return ids, am, pos, rows


def test_padded_image_batch_greedy_ids_identical_to_the_reference(eng):
    eng.load_weights(FE_MODEL_VLM, _planted("qwen2_5_vl_tiny", int(R["seed_w"])))
    ids, am, pos, rows = _image_batch(eng)
    n = R["tokens_planted"].shape[1]
    toks = eng.vlm_generate(ids, n, position_ids=pos, image_rows=rows, attention_mask=am)          # device-resident loop (stream path: 3 rows)
    assert np.array_equal(toks, R["tokens_planted"]), (toks, R["tokens_planted"])
    toks2, logits = eng.vlm_generate(ids, n, position_ids=pos, image_rows=rows, attention_mask=am, want_logits=True)      # stepwise path
    assert np.array_equal(toks2, R["tokens_planted"]) and np.isfinite(logits).all()


def test_padded_image_batch_teacher_forced_logits(eng):
    eng.load_weights(FE_MODEL_VLM, synthetic_state_dict("qwen2_5_vl_tiny", int(R["seed_w"])))
    ids, am, pos, rows = _image_batch(eng)
    want = R["logits_unplanted"]
    _, logits = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows, attention_mask=am, want_logits=True,
                                 forced_tokens=R["tokens_unplanted"])
    assert np.isfinite(logits).all()
    err = np.abs(logits - want).max()
    print(f"[vlm padded] teacher-forced logits max |diff| {err:.4f} (|max| {np.abs(want).max():.2f})")
    assert err <= TOL


def _text_batch(lengths, seed, pad_id):
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(10, 1990, n).astype(np.int32) for n in lengths]
    L = max(lengths)
    ids = np.full((len(seqs), L), pad_id, np.int32)
    am = np.zeros((len(seqs), L), np.int32)
    for b, s in enumerate(seqs):
        ids[b, L - len(s):] = s
        am[b, L - len(s):] = 1
    pos, _ = rope_index(ids, np.zeros((0, 3)), -1, attention_mask=am)
    return seqs, ids, am, pos


# pads cross 32-key prefill tiles and a 128-key decode chunk: B = 2 replays a captured decode graph, B = 3 and 5 launch on the stream
BATCHES = {2: [170, 31], 3: [40, 175, 140], 5: [150, 40, 175, 3, 100]}


@pytest.mark.parametrize("B", sorted(BATCHES))
def test_each_row_generates_what_it_generates_alone(eng, B):
    eng.load_weights(FE_MODEL_VLM, _planted("qwen2_5_vl_text_tiny", 11))
    seqs, ids, am, pos = _text_batch(BATCHES[B], B, 0)
    new = 10
    toks = eng.vlm_generate(ids, new, position_ids=pos, attention_mask=am)
    for b, s in enumerate(seqs):
        alone = eng.vlm_generate(s[None], new)
        assert np.array_equal(toks[b], alone[0]), (B, b, toks[b], alone[0])


@pytest.mark.parametrize("B", sorted(BATCHES))
def test_each_row_logits_match_the_sequence_alone(eng, B):
    eng.load_weights(FE_MODEL_VLM, synthetic_state_dict("qwen2_5_vl_text_tiny", 12))
    seqs, ids, am, pos = _text_batch(BATCHES[B], 10 + B, 0)
    new = 6
    forced = np.random.default_rng(B).integers(10, 1990, (B, new)).astype(np.int32)
    _, lg = eng.vlm_generate(ids, new, position_ids=pos, attention_mask=am, want_logits=True, forced_tokens=forced)
    assert np.isfinite(lg).all()
    for b, s in enumerate(seqs):
        _, la = eng.vlm_generate(s[None], new, want_logits=True, forced_tokens=forced[b:b + 1])
        err = np.abs(lg[b] - la[0]).max()
        assert err <= TOL, (B, b, float(err))
    # the pad token id is never looked at by a live row: another id gives the same bits
    _, ids2, am2, pos2 = _text_batch(BATCHES[B], 10 + B, 1234)
    _, lg2 = eng.vlm_generate(ids2, new, position_ids=pos2, attention_mask=am2, want_logits=True, forced_tokens=forced)
    assert np.array_equal(lg, lg2)


def test_right_padding_is_rejected(eng):
    eng.load_weights(FE_MODEL_VLM, synthetic_state_dict("qwen2_5_vl_text_tiny", 12))
    am = np.array([[1, 1, 1, 0], [1, 1, 1, 1]], np.int32)
    with pytest.raises(ValueError):
        eng.vlm_generate(np.ones((2, 4), np.int32), 2, position_ids=np.zeros((3, 2, 4), np.int32), attention_mask=am)


def test_a_prompt_longer_than_the_cache_is_a_capacity_error_by_number(eng):
    """fe_vlm_prefill_images_padded with one position more than max_seq: refused by the entry point's own check, whose text carries one
    of the strings the padded path reports as FE_ERR_CAPACITY (-4) and not as FE_ERR_RUNTIME; nothing is launched or written."""
    eng.load_weights(FE_MODEL_VLM, synthetic_state_dict("qwen2_5_vl_text_tiny", 12))
    n_seq, L = 2, 5
    i32p = C.POINTER(C.c_int32)
    ids, pos, pad = np.ones((n_seq, L), np.int32), np.zeros((3, n_seq, L), np.int32), np.zeros(n_seq, np.int32)
    nxt = np.full(n_seq, -7, np.int32)
    rc = eng.lib.fe_vlm_prefill_images_padded(eng.h, ids.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), n_seq, L, L - 1, pad.ctypes.data_as(i32p),
                                              None, 0, nxt.ctypes.data_as(i32p), None)
    assert rc == -4 and b"max_seq <= 8192" in eng.lib.fe_last_error(eng.h)
    assert (nxt == -7).all()


def test_tag_batch_on_photos_of_different_sizes(eng):
    from standins import vlm_tokenizer as T
    eng.load_weights(FE_MODEL_VLM, _planted("qwen2_5_vl_tiny", int(R["seed_w"])))
    photos = [R[f"photo_{i}"] for i in range(3)]
    pil = [Image.fromarray(a, "RGBA" if a.shape[2] == 4 else "RGB") for a in photos]
    n = R["photo_tokens"].shape[1]
    t = VLMTagger({"model_path": "Qwen/Qwen2.5-VL-7B-Instruct", "max_new_tokens": n, "vlm_batch_size": 3}, engine=eng, encode=T.encode,
                  decode=T.decode, special_tokens=T.TOKENS)
    t.model = eng
    x = t.prepare_inputs(pil)
    assert np.array_equal(x["input_ids"], R["photo_input_ids"]) and np.array_equal(x["grid_thw"], R["photo_grid_thw"])
    assert np.array_equal(t.generate_from_images(pil), R["photo_tokens"])
    want = [t._parse_tags(s, 5) for s in t._texts(R["photo_tokens"])]
    assert t.tag_batch(pil) == want
    assert t.tag_image(pil[1]) == t.tag_batch([pil[1]])[0]
