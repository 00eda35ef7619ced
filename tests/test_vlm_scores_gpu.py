"""GPU: confidence scores of the VLM tagger - the log-probability of every greedy token, taken by the decoder's selection kernels in the
pass that picks the token (fe_op_vlm_select, fe_vlm_generate_scored, fe_vlm_last_logprobs) - up to VLMTagger.tag_image_with_scores /
get_tags_with_scores / tag_batch_with_scores, against tests/golden/vlm_scores_golden.npz (tests/golden/make_vlm_scores_golden.py: the
reference's own classes and its own tag_image_with_scores).

  * kernel: at vocab 152064 / 151936 / 2048 and 1 / 3 / 32 / 65 rows, on N(0, 10^2) logits, a spike, all-equal rows, ties at the top,
    +-3e4 magnitudes and -inf entries: ids equal np.argmax of the bf16-rounded rows (first index on ties), log-probs within 1e-5 of a
    float64 log_softmax;
  * engine: vlm_generate(return_logprobs=True) picks the same ids as vlm_generate at 1 / 2 sequences (graph replay), 3 / 5 / 32 / 40
    (stream launches; GEMV, 32-row GEMM and wide GEMM projections) and for a left-padded batch; its log-probs are within 1e-5 of the
    float64 log_softmax of the engine's own logits at those ids; NaN after a row's EOS;
  * reference, both families: identical greedy ids through the EOS; per-step log-probs within 2 max_i |d logit_i| + 1e-5 of the golden
    (log-softmax is 2-Lipschitz in the max norm, so the bound follows the logit error) and under 0.5 (planted) / 0.125 (unplanted,
    teacher-forced); tag_image_with_scores: the same tags in the same order, |log conf - log conf_ref| within that bound;
    get_tags_with_scores: the reference's tag set at every threshold that is not within the bound of a confidence;
  * tag_batch_with_scores on three photos of mixed size: each row has the tags tag_image_with_scores gives that photo alone, confidences
    within the same bound (measured against the two runs' own logits).
"""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from facet_amd._lib import FE_MODEL_VLM
from facet_amd.vlm_tagger import VLMTagger, rope_index
from facet_amd.weights import synthetic_state_dict, VLM_TINY, VLM3_TINY

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
S = np.load(os.path.join(GOLDEN, "vlm_scores_golden.npz"))
SEED = int(S["seed_w"])
NEW = int(S["max_new_tokens"])
# the reduced geometries of make_vlm_vision_golden.py / make_vlm3_golden.py
GEOM = {"qwen2_5": dict(n_heads=VLM_TINY["heads"], n_kv_heads=VLM_TINY["kv_heads"], head_dim=128, rope_theta=1e6, rms_eps=1e-6,
                        mrope_section=(16, 24, 24), vis_heads=2, fullatt_block_indexes=(1,)),
        "qwen3": dict(n_heads=VLM3_TINY["heads"], n_kv_heads=VLM3_TINY["kv_heads"], head_dim=128, rope_theta=5e6, rms_eps=1e-6,
                      mrope_section=(24, 20, 20), vis_heads=2, deepstack_indexes=(0, 2, 3))}
PATH = {"qwen2_5": "Qwen/Qwen2.5-VL-7B-Instruct", "qwen3": "Qwen/Qwen3-VL-2B-Instruct"}


def _lsm64(logits):
    x = np.asarray(logits, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


@pytest.fixture()
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=6 << 30)
    yield e
    e.close()


# -- 1. the selection kernels ------------------------------------------------------------------------------------------------------------
def _rows(rows, vocab, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((rows, vocab), np.float32)
    for r in range(rows):
        kind = r % 6
        if kind == 0:
            x[r] = rng.normal(0, 10, vocab)
        elif kind == 1:                                    # one spike: log-prob ~ 0
            x[r] = rng.normal(0, 1, vocab)
            x[r, rng.integers(vocab)] = 200.0
        elif kind == 2:                                    # all equal: -log V
            x[r] = 1.5
        elif kind == 3:                                    # ties at the top (the first index wins)
            x[r] = rng.normal(0, 3, vocab)
            x[r, rng.choice(vocab, 4, replace=False)] = 40.0
        elif kind == 4:                                    # large magnitudes
            x[r] = rng.uniform(-3e4, 3e4, vocab)
        else:                                              # -inf entries
            x[r] = rng.normal(0, 10, vocab)
            x[r, rng.random(vocab) < 0.4] = -np.inf
    return x


@pytest.mark.parametrize("vocab", [152064, 151936, 2048])
@pytest.mark.parametrize("rows", [1, 3, 32, 65])
def test_select_kernel_ids_and_logprobs(eng, vocab, rows):
    x = _rows(rows, vocab, vocab + rows)
    ids, lp = eng.select(x)
    xb = _bf16(x)
    want_ids = np.argmax(xb, axis=1)
    assert np.array_equal(ids, want_ids), (np.flatnonzero(ids != want_ids)[:4], ids[:8], want_ids[:8])
    want = _lsm64(xb)[np.arange(rows), want_ids]
    err = np.abs(lp.astype(np.float64) - want)
    assert np.isfinite(lp).all() and err.max() <= 1e-5, (float(err.max()), int(err.argmax()), lp[:6], want[:6])
    for r in range(rows):
        if r % 6 == 2:
            assert abs(lp[r] + math.log(vocab)) <= 1e-5 and ids[r] == 0
        if r % 6 == 3:
            assert ids[r] == np.flatnonzero(xb[r] == xb[r].max())[0]


def test_select_kernel_every_row_kind_at_one_row(eng):
    """rows = 1 above only sees the N(0, 10^2) kind: every kind alone."""
    x = _rows(6, 152064, 3)
    for r in range(6):
        ids, lp = eng.select(x[r:r + 1])
        xb = _bf16(x[r:r + 1])
        assert ids[0] == np.argmax(xb[0])
        assert abs(float(lp[0]) - _lsm64(xb)[0, ids[0]]) <= 1e-5, r


# -- 2. the engine's generate paths ----------------------------------------------------------------------------------------------------
def _text_model(e, div=64.0):
    """qwen2_5_vl_text_tiny with a planted read-out of moderate margins (lm_head = permuted embeddings / div): log-probs well away from 0."""
    e.vlm_configure(n_heads=VLM_TINY["heads"], n_kv_heads=VLM_TINY["kv_heads"], head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24))
    sd = synthetic_state_dict("qwen2_5_vl_text_tiny", 11)
    perm = np.random.default_rng([11, 77]).permutation(VLM_TINY["vocab"])
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / div).astype(np.float32)
    e.load_weights(FE_MODEL_VLM, sd)


def _check_scored(ids, logits, lps, eos):
    """lps: NaN exactly after each row's first EOS; elsewhere within 1e-5 of the float64 log_softmax of the logits at the ids."""
    ref = _lsm64(logits)
    n, T = ids.shape
    for b in range(n):
        hit = np.flatnonzero(np.isin(ids[b], eos))
        end = int(hit[0]) + 1 if hit.size else T
        assert np.isnan(lps[b, end:]).all() and np.isfinite(lps[b, :end]).all(), (b, lps[b])
        want = ref[b, np.arange(end), ids[b, :end]]
        err = np.abs(lps[b, :end].astype(np.float64) - want).max()
        assert err <= 1e-5, (b, float(err))


@pytest.mark.parametrize("B", [1, 2, 3, 5, 32, 40])
def test_generate_scored_ids_equal_and_logprobs_match_own_logits(eng, B):
    _text_model(eng)
    rng = np.random.default_rng(B)
    ids = rng.integers(10, 1990, (B, 24)).astype(np.int32)
    new = 10
    plain = eng.vlm_generate(ids, new)
    eos = [int(plain[0, 4])]                     # row 0 stops at step 4 (at the latest); rows that never emit it run to the end
    plain = eng.vlm_generate(ids, new, eos_token_ids=eos)
    got, lps = eng.vlm_generate(ids, new, eos_token_ids=eos, return_logprobs=True)
    assert np.array_equal(got, plain)
    sw, logits, lps_sw = eng.vlm_generate(ids, new, eos_token_ids=eos, want_logits=True, return_logprobs=True)
    assert np.array_equal(sw, plain)
    _check_scored(got, logits, lps, eos)
    _check_scored(sw, logits, lps_sw, eos)
    assert np.isnan(lps[0, 5:]).all() and np.nanmax(lps) <= 0
    print(f"[vlm scores] B={B}: log-probs {np.nanmin(lps):.3f} .. {np.nanmax(lps):.3g}, product vs stepwise max |diff| "
          f"{np.nanmax(np.abs(lps - lps_sw)):.2e}")


def test_generate_scored_left_padded_batch(eng):
    _text_model(eng)
    rng = np.random.default_rng(7)
    lengths = [150, 40, 175]
    L = max(lengths)
    ids = np.zeros((3, L), np.int32)
    am = np.zeros((3, L), np.int32)
    for b, n in enumerate(lengths):
        ids[b, L - n:] = rng.integers(10, 1990, n)
        am[b, L - n:] = 1
    pos, _ = rope_index(ids, np.zeros((0, 3)), -1, attention_mask=am)
    plain = eng.vlm_generate(ids, 8, position_ids=pos, attention_mask=am)
    got, lps = eng.vlm_generate(ids, 8, position_ids=pos, attention_mask=am, return_logprobs=True)
    assert np.array_equal(got, plain)
    _, logits, _ = eng.vlm_generate(ids, 8, position_ids=pos, attention_mask=am, want_logits=True, return_logprobs=True)
    _check_scored(got, logits, lps, [])


# -- 3. against the reference class ------------------------------------------------------------------------------------------------------
def _state(family, plant):
    if family == "qwen3":
        sd = synthetic_state_dict("qwen3_vl_tiny_untied" if plant else "qwen3_vl_tiny", SEED)
        vocab = VLM3_TINY["vocab"]
    else:
        sd = synthetic_state_dict("qwen2_5_vl_tiny", SEED)
        vocab = VLM_TINY["vocab"]
    if plant:
        perm = np.random.default_rng([SEED, 77]).permutation(vocab)
        sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    return sd


def _tagger(e, family, plant=True, batch=2):
    from standins import vlm_tokenizer as T
    eos = int(S[f"{family}_eos"])
    cfg = {"model_path": PATH[family], "max_new_tokens": NEW, "vlm_batch_size": batch}
    if family == "qwen3":
        cfg.update(min_pixels=int(S["photo_min_pixels"]), max_pixels=int(S["photo_max_pixels"]))
    tg = VLMTagger(cfg, engine=e, encode=T.encode, decode=lambda ids: T.decode([t for t in ids if int(t) != eos]),
                   special_tokens=dict(T.TOKENS, eos_token_ids=(eos,)))
    tg.load(_state(family, plant), geometry=GEOM[family])
    return tg


class _Extra:
    """Engine.vlm_generate with extra keyword arguments (want_logits, forced_tokens) while inside: the tagger's own photo path, observed."""

    def __init__(self, e, **extra):
        self.e, self.extra = e, extra

    def __enter__(self):
        orig = type(self.e).vlm_generate
        self.e.vlm_generate = lambda *a, **k: orig(self.e, *a, **dict(k, **self.extra))
        return self

    def __exit__(self, *exc):
        del self.e.vlm_generate


def _photo(family):
    return Image.fromarray(S[f"{family}_photo"], "RGB")


@pytest.mark.parametrize("family", ["qwen2_5", "qwen3"])
def test_planted_ids_logprobs_and_tag_scores_against_the_reference(eng, family):
    tg = _tagger(eng, family)
    pil = _photo(family)
    want_ids, want_lp, scores = S[f"{family}_ids"], S[f"{family}_logprobs"].astype(np.float64), S[f"{family}_scores"]
    n = len(want_ids)
    assert tg.prepare_inputs([pil])["input_ids"].tolist() == S[f"{family}_input_ids"].tolist()
    ids, lps = tg.generate_from_images([pil], return_logprobs=True)                  # the product path
    assert np.array_equal(ids[0, :n], want_ids), (ids[0], want_ids)
    assert (ids[0, n:] == want_ids[-1]).all() and np.isnan(lps[0, n:]).all()
    with _Extra(eng, want_logits=True):
        ids_w, logits, _ = tg.generate_from_images([pil], return_logprobs=True)
    assert np.array_equal(ids_w, ids)
    bound = 2 * np.abs(logits[0, :n] - scores).max(-1) + 1e-5                        # per step
    err = np.abs(lps[0, :n].astype(np.float64) - want_lp)
    print(f"[vlm scores {family}] log-prob |diff| max {err.max():.2e}, bound {bound.min():.3f} .. {bound.max():.3f}")
    assert (err <= bound).all() and err.max() < 0.5, (err, bound)
    # the tagger's dict methods against the reference's own tag_image_with_scores
    got = tg.tag_image_with_scores(pil)
    ref = dict(zip([str(t) for t in S[f"{family}_tags"]], S[f"{family}_confidences"].tolist()))
    assert list(got) == list(ref), (got, ref)
    B = float(bound.max())
    for k, v in ref.items():
        assert abs(math.log(got[k]) - math.log(v)) <= B, (k, got[k], v, B)
    checked = 0
    for th in (0.0, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95, 0.99, 0.9999, 1.0):
        if th > 0 and any(abs(math.log(th) - math.log(v)) <= B for v in ref.values()):
            continue                                  # a confidence within the bound of the threshold: either side is right
        want = {k for k, v in ref.items() if th <= 0 or v >= th}
        assert set(tg.get_tags_with_scores(pil, threshold=th)) == want, (th, got, ref)
        checked += 1
    assert checked >= 3


@pytest.mark.parametrize("family", ["qwen2_5", "qwen3"])
def test_unplanted_teacher_forced_logprobs_against_the_reference(eng, family):
    tg = _tagger(eng, family, plant=False)
    forced = S[f"{family}_unplanted_ids"][None]
    want_logits = S[f"{family}_unplanted_logits"]
    with _Extra(eng, want_logits=True, forced_tokens=forced):
        _, logits, lps = tg.generate_from_images([_photo(family)], return_logprobs=True)
    want = _lsm64(want_logits).max(-1)                  # the golden's log-prob of its own greedy id (the row maximum)
    bound = 2 * np.abs(logits[0] - want_logits).max(-1) + 1e-5
    err = np.abs(lps[0].astype(np.float64) - want)
    print(f"[vlm scores {family} unplanted] log-prob |diff| max {err.max():.2e}, bound max {bound.max():.3f}")
    assert np.isfinite(lps).all() and (err <= bound).all() and err.max() < 0.125, (err, bound)


# -- 4. the batch extension --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["qwen2_5", "qwen3"])
def test_tag_batch_with_scores_rows_equal_the_photo_alone(eng, family):
    g = np.load(os.path.join(GOLDEN, "vlm_ragged_golden.npz" if family == "qwen2_5" else "vlm3_golden.npz"))
    pil = [Image.fromarray(g[f"photo_{i}"], "RGBA" if g[f"photo_{i}"].shape[2] == 4 else "RGB") for i in range(3)]
    tg = _tagger(eng, family, batch=3)
    got = tg.tag_batch_with_scores(pil)
    alone = [tg.tag_image_with_scores(p) for p in pil]
    with _Extra(eng, want_logits=True):
        ids_b, lg_b, _ = tg.generate_from_images(pil, return_logprobs=True)
        rows = [tg.generate_from_images([p], return_logprobs=True) for p in pil]
    spread = []
    for i in range(3):
        assert list(got[i]) == list(alone[i]), (i, got[i], alone[i])
        assert np.array_equal(ids_b[i], rows[i][0][0])
        eos = np.flatnonzero(ids_b[i] == int(S[f"{family}_eos"]))
        end = int(eos[0]) + 1 if eos.size else NEW
        B = 2 * float(np.abs(lg_b[i, :end] - rows[i][1][0, :end]).max()) + 1e-5
        for k in got[i]:
            d = abs(math.log(got[i][k]) - math.log(alone[i][k]))
            assert d <= B, (i, k, d, B)
            spread.append(d)
    print(f"[vlm scores {family}] tag_batch_with_scores vs alone: |log conf| spread max {max(spread, default=0):.2e}, tags {[len(r) for r in got]}")
