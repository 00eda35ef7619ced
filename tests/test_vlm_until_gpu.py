"""GPU: greedy decode that stops (fe_vlm_generate_until) against the full device loop (fe_vlm_generate / fe_vlm_generate_scored) on the
planted Qwen2-VL tiny checkpoint (the left-padded 3-row batch of tests/golden/vlm2_golden.npz; max_steps 24, poll 4), and once on the
Qwen3-VL tiny checkpoint.

The EOS ids are the ids rows 0 / 1 / 2 emitted at decode steps 3 / 6 / 9 of the full run. The expectation is computed here by the stated
rule: a row is finished from its first hit of ANY of the ids (an earlier hit of another row's id counts, the prefill's token included);
its tail holds that id, its log-probs are NaN after the hit; the loop ends at the first multiple of `poll` steps by which every row has
finished; rows of the output past that hold each sequence's EOS id."""
import os

import numpy as np
import pytest

from facet_amd._lib import FE_MODEL_VLM
from facet_amd.vlm_tagger import rope_index, vision_inputs_qwen2, vision_inputs_qwen3
from facet_amd.weights import synthetic_state_dict, VLM2_TINY, VLM3_TINY

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
MAX_STEPS, POLL = 24, 4


def _planted(name, tiny, seed):
    sd = synthetic_state_dict(name, seed)
    perm = np.random.default_rng([seed, 77]).permutation(tiny["vocab"])
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    return sd


def _prefill(e, G, encode, order=(0, 1, 2)):
    """Rows `order` of the golden's padded batch, left-padded among themselves and prefilled; -> (first tokens [n], positions of the first
    decode step [3, n])."""
    grid_all, ids_all, am_all = G["batch_grid_thw"], G["batch_input_ids"], G["batch_attention_mask"]
    pv_all = np.random.default_rng(int(G["batch_pixel_seed"])).normal(0, 1, (int(grid_all.prod(1).sum()), 1176 if encode is _enc2 else 1536)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(grid_all.prod(1))])
    rows_ = [ids_all[i][am_all[i] == 1] for i in order]
    L = max(len(r) for r in rows_)
    ids, am = np.zeros((len(order), L), np.int32), np.zeros((len(order), L), np.int32)
    for b, r in enumerate(rows_):
        ids[b, L - len(r):] = r
        am[b, L - len(r):] = 1
    grid = grid_all[list(order)]
    encode(e, np.concatenate([pv_all[off[i]:off[i + 1]] for i in order]), grid)
    img = int(G["image_token_id"])
    pos, nxt = rope_index(ids, grid, img, attention_mask=am)
    if tuple(order) == (0, 1, 2):
        assert np.array_equal(pos, G["batch_position_ids"])
    rows = np.flatnonzero(((ids == img) & (am == 1)).reshape(-1)).astype(np.int32)
    first = e.vlm_prefill(ids, pos, max_seq=L + MAX_STEPS + 1, image_rows=rows, pad=(am == 0).sum(1))
    return first, np.broadcast_to(nxt.astype(np.int32), (3, len(order))).copy(), L


def _enc2(e, pv, grid):
    v = vision_inputs_qwen2(grid)
    e.vlm2_encode_images(pv, v["patch_pos_hw"], v["cu_seqlens"], want_embeds=False)


def _enc3(e, pv, grid):
    v = vision_inputs_qwen3(grid, 8)
    e.vlm3_encode_images(pv, v["patch_pos_hw"], v["interp_idx"], v["interp_w"], v["cu_seqlens"], want_embeds=False)


def _full(e, G, encode, order=(0, 1, 2)):
    """The full run: (first tokens, decode-step tokens [24, n], their log-probs [24, n]) of fe_vlm_generate_scored, ids checked against fe_vlm_generate."""
    import ctypes as C
    n = len(order)
    first, pos, _ = _prefill(e, G, encode, order)
    plain = np.empty((MAX_STEPS, n), np.int32)
    e._ck(e.lib.fe_vlm_generate(e.h, first.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.POINTER(C.c_int32)), n, MAX_STEPS,
                                plain.ctypes.data_as(C.POINTER(C.c_int32))))
    first2, pos2, _ = _prefill(e, G, encode, order)
    assert np.array_equal(first, first2)
    toks = np.empty((MAX_STEPS, n), np.int32)
    lps = np.empty((MAX_STEPS, n), np.float32)
    e._ck(e.lib.fe_vlm_generate_scored(e.h, first2.ctypes.data_as(C.POINTER(C.c_int32)), pos2.ctypes.data_as(C.POINTER(C.c_int32)), n, MAX_STEPS,
                                       toks.ctypes.data_as(C.POINTER(C.c_int32)), lps.ctypes.data_as(C.POINTER(C.c_float))))
    assert np.array_equal(plain, toks) and np.isfinite(lps).all()
    return first, toks, lps


def _expect(first, toks, lps, eos):
    """The stated rule on the host -> (tokens, log-probs, first-hit step per row (-1: the prefill's token; None: never), steps_run)."""
    want_t, want_l, hits = toks.copy(), lps.copy(), []
    for b in range(toks.shape[1]):
        if first[b] in eos:
            hits.append(-1)
            want_t[:, b] = first[b]
            want_l[:, b] = np.nan
            continue
        hit = np.flatnonzero(np.isin(toks[:, b], eos))
        hits.append(int(hit[0]) if hit.size else None)
        if hit.size:
            want_t[hit[0]:, b] = toks[hit[0], b]
            want_l[hit[0] + 1:, b] = np.nan
    if any(h is None for h in hits):
        ran = MAX_STEPS
    else:
        ran = min(MAX_STEPS, max(POLL, -(-(max(hits) + 1) // POLL) * POLL))
    return want_t, want_l, hits, ran


def _check(e, G, encode, first, toks, lps, eos, early, order=(0, 1, 2)):
    want_t, want_l, hits, ran = _expect(first, toks, lps, eos)
    if early:
        # the condition that makes the test mean something: the latest first hit is at step <= 12, so the loop really ends early
        assert all(h is not None for h in hits) and max(hits) <= 12, hits
        assert ran == -(-(max(hits) + 1) // POLL) * POLL and ran < MAX_STEPS, (hits, ran)
    else:
        assert ran == MAX_STEPS and np.array_equal(want_t, toks)
    f, pos, L = _prefill(e, G, encode, order)
    got_t, got_l, got_ran = e.vlm_generate_until(f, pos, MAX_STEPS, eos, poll=POLL, return_logprobs=True)
    assert got_ran == ran, (got_ran, ran, hits)
    assert np.array_equal(got_t, want_t), (got_t.T, want_t.T)
    assert np.array_equal(np.isnan(got_l), np.isnan(want_l)), (np.isnan(got_l).T, hits)
    assert np.array_equal(got_l[~np.isnan(want_l)], want_l[~np.isnan(want_l)])
    assert e.vlm_dims()["cur_len"] == L + ran
    f, pos, L = _prefill(e, G, encode, order)      # without log-probs: the plain selection kernels, same ids and step count
    got_t2, none, got_ran2 = e.vlm_generate_until(f, pos, MAX_STEPS, eos, poll=POLL)
    assert none is None and got_ran2 == ran and np.array_equal(got_t2, want_t)
    return hits, ran


@pytest.fixture()
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=4 << 30)
    yield e
    e.close()


def _qwen2(e):
    G = np.load(os.path.join(HERE, "golden", "vlm2_golden.npz"))
    e.vlm2_configure(n_heads=VLM2_TINY["heads"], n_kv_heads=VLM2_TINY["kv_heads"], head_dim=128, rope_theta=1e6, rms_eps=1e-6,
                     mrope_section=tuple(int(v) for v in G["mrope_section"]), vis_heads=int(G["vis_heads"]))
    e.load_weights(FE_MODEL_VLM, _planted("qwen2_vl_tiny_untied", VLM2_TINY, int(G["seed_w"])))
    return G


def test_stops_early_with_the_full_runs_ids_and_logprobs(eng):
    G = _qwen2(eng)
    first, toks, lps = _full(eng, G, _enc2)
    assert np.array_equal(np.concatenate([first[:, None], toks.T], 1), G["batch_tokens_planted"])      # the reference's own ids
    eos = [int(toks[3, 0]), int(toks[6, 1]), int(toks[9, 2])]
    hits, ran = _check(eng, G, _enc2, first, toks, lps, eos, early=True)
    print("eos", eos, "first hits", hits, "steps_run", ran)


@pytest.mark.parametrize("order", [(1,), (2, 0)])
def test_stops_between_graph_replays_with_one_and_two_rows(eng, order):
    """Up to 2 sequences replay the captured step graph (3 take stream launches): the stop is a host decision between replays, the device
    counters advance inside the graph. One row is what analyze_composition on a single photo runs."""
    G = _qwen2(eng)
    first, toks, lps = _full(eng, G, _enc2, order)
    eos = [int(toks[6, 0])] + ([int(toks[9, 1])] if len(order) > 1 else [])
    hits, ran = _check(eng, G, _enc2, first, toks, lps, eos, early=True, order=order)
    assert max(hits) <= 9 and ran <= 12
    never = next(t for t in range(10, 2000) if t not in toks and t not in first)
    _check(eng, G, _enc2, first, toks, lps, [never], early=False, order=order)


def test_an_id_never_emitted_runs_every_step(eng):
    G = _qwen2(eng)
    first, toks, lps = _full(eng, G, _enc2)
    never = next(t for t in range(10, 2000) if t not in toks and t not in first)
    _check(eng, G, _enc2, first, toks, lps, [never], early=False)


def test_engine_vlm_generate_stop_at_eos_equals_the_default_path(eng):
    G = _qwen2(eng)
    ids, am, pos = G["batch_input_ids"], G["batch_attention_mask"], G["batch_position_ids"]
    img = int(G["image_token_id"])
    rows = np.flatnonzero(((ids == img) & (am == 1)).reshape(-1)).astype(np.int32)
    pv = np.random.default_rng(int(G["batch_pixel_seed"])).normal(0, 1, (int(G["batch_grid_thw"].prod(1).sum()), 1176)).astype(np.float32)
    want = G["batch_tokens_planted"]
    eos = [int(want[0, 4]), int(want[1, 7]), int(want[2, 10])]
    out = {}
    for stop in (False, True):
        _enc2(eng, pv, G["batch_grid_thw"])
        out[stop] = eng.vlm_generate(ids, want.shape[1], position_ids=pos, image_rows=rows, attention_mask=am, eos_token_ids=eos, return_logprobs=True,
                                     stop_at_eos=stop, poll=POLL)
    assert np.array_equal(out[True][0], out[False][0])
    assert np.array_equal(out[True][1], out[False][1], equal_nan=True)
    assert eng.vlm_dims()["cur_len"] < ids.shape[1] + want.shape[1] - 1


def test_the_same_on_the_qwen3_tiny_checkpoint(eng):
    G = np.load(os.path.join(HERE, "golden", "vlm3_golden.npz"))
    eng.vlm3_configure(n_heads=VLM3_TINY["heads"], n_kv_heads=VLM3_TINY["kv_heads"], head_dim=128, rope_theta=5e6, rms_eps=1e-6,
                       mrope_section=tuple(int(v) for v in G["mrope_section"]), vis_heads=int(G["vis_heads"]),
                       deepstack_indexes=tuple(int(v) for v in G["deepstack_indexes"]))
    eng.load_weights(FE_MODEL_VLM, _planted("qwen3_vl_tiny_untied", VLM3_TINY, int(G["seed_w"])))
    first, toks, lps = _full(eng, G, _enc3)
    eos = [int(toks[3, 0]), int(toks[6, 1]), int(toks[9, 2])]
    _check(eng, G, _enc3, first, toks, lps, eos, early=True)
