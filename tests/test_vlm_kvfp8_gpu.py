"""GPU: the e4m3 KV cache of the VLM decoders (Engine.vlm_kv_format("fp8"): every cache row - the 128 values of one sequence, KV head
and position, K and V separately - as OCP e4m3 codes with one power-of-two scale, facet_amd/csrc/fp8_core.h, read by the decode
attention kernel; "bf16_e4m3": the same values in a bf16 cache).

Every dequantised value is exactly a bf16 value, so the fp8-cache engine is the bf16 engine whose cache rows were replaced by
dequantize(quantize(row)) (numpy: facet_amd.weights). Below, A is an engine under "fp8", B one under "bf16_e4m3" and C one under
"bf16", loaded with the same state dict. A prefill attends to its own unquantised K / V, so A's prefill is C's bit for bit and its cache
the image of C's; A against B is the same arithmetic on other storage; the decode kernel alone is tested against float64 on the
dequantised rows with the bound derived in tests/test_attention_gpu.py; an independent implementation (transformers' class over a
quantising cache, tests/golden/make_vlm_kvfp8_golden.py) gives the token ids.
"""
import os

import numpy as np
import pytest

from facet_amd._lib import FE_MODEL_VLM
from facet_amd.vlm_tagger import rope_index
from facet_amd.weights import (synthetic_state_dict, qwen2_5_vl_text_spec, qwen3_vl_text_spec, VLM_TINY, VLM2_TINY, VLM3_TINY, quantize_e4m3_rows,
                               dequantize_e4m3_rows)

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "vlm_kvfp8_golden.npz"))
GEOM = dict(head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24))


def _dq(w):
    w = np.asarray(w, np.float32)
    return dequantize_e4m3_rows(*quantize_e4m3_rows(w.reshape(-1, w.shape[-1]))).reshape(w.shape)


def _bf16(w):
    u = np.ascontiguousarray(w, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> 16) & 1)) & np.uint32(0xFFFF0000)).view(np.float32)


def _planted(seed, name="qwen2_5_vl_text_tiny", vocab=VLM_TINY["vocab"]):          # as tests/test_vlm_gpu.py
    sd = synthetic_state_dict(name, seed)
    perm = np.random.default_rng([seed, 77]).permutation(vocab)
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    return sd


def _margin(lg):
    t2 = np.sort(lg, -1)[..., -2:]
    return t2[..., 1] - t2[..., 0]


@pytest.fixture(scope="module")
def planted7():
    return _planted(7)


@pytest.fixture()
def engines():
    from facet_amd import Engine
    made = []

    def make(kv, cfg=VLM_TINY, configure=None, weights="bf16"):
        e = Engine(0, arena_bytes=4 << 30)
        made.append(e)
        if configure:
            configure(e)
        else:
            e.vlm_configure(n_heads=cfg["heads"], n_kv_heads=cfg["kv_heads"], **GEOM)
        e.vlm_weight_format(weights)
        e.vlm_kv_format(kv)
        return e
    yield make
    for e in made:
        e.close()


def _padded_batch(lengths, seed):
    rng = np.random.default_rng(seed)
    L = max(lengths)
    ids, am = np.zeros((len(lengths), L), np.int32), np.zeros((len(lengths), L), np.int32)
    for b, n in enumerate(lengths):
        ids[b, L - n:] = rng.integers(10, 1990, n)
        am[b, L - n:] = 1
    pos, _ = rope_index(ids, np.zeros((0, 3)), -1, attention_mask=am)
    return ids, am, pos


# ---- 1. bytes ----------------------------------------------------------------------------------------------------------------------------
def test_kv_info_reports_the_bytes(engines, planted7):
    c = VLM_TINY
    a, b = engines("fp8"), engines("bf16")
    for e in (a, b):
        e.load_weights(FE_MODEL_VLM, planted7)
    ia, ib = a.vlm_kv_info(), b.vlm_kv_info()
    assert ia == dict(format="fp8", bytes_per_token=c["layers"] * c["kv_heads"] * 2 * 132, allocated_bytes=0, max_seq=0)
    assert ib == dict(format="bf16", bytes_per_token=c["layers"] * c["kv_heads"] * 512, allocated_bytes=0, max_seq=0)
    p = np.random.default_rng(1).integers(0, 2048, (3, 21)).astype(np.int32)
    for e in (a, b):
        e.vlm_prefill(p, max_seq=40)
    ia, ib = a.vlm_kv_info(), b.vlm_kv_info()
    print(f"[vlm kv fp8] kv info fp8 {ia}, bf16 {ib}: ratio {ia['bytes_per_token'] / ib['bytes_per_token']:.4f}")
    assert ia["max_seq"] == 40 and ib["max_seq"] == 40
    assert ia["allocated_bytes"] == 3 * 40 * ia["bytes_per_token"] and ib["allocated_bytes"] == 3 * 40 * ib["bytes_per_token"]


# ---- 2. the prefill is untouched; the cache is the image of the bf16 cache ------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["3x21", "left-padded"])
def test_prefill_is_the_bf16_prefill_and_the_cache_its_image(engines, planted7, padded):
    a, c = engines("fp8"), engines("bf16")
    for e in (a, c):
        e.load_weights(FE_MODEL_VLM, planted7)
    if padded:
        ids, am, pos = _padded_batch([21, 9, 14], 3)
        pad = (am == 0).sum(1)
        kw = dict(position_ids=pos, pad=pad.astype(np.int32))
    else:
        ids, pad, kw = np.random.default_rng(2).integers(0, 2048, (3, 21)).astype(np.int32), np.zeros(3, int), {}
    ta, la = a.vlm_prefill(ids, want_logits=True, **kw)
    tc, lc = c.vlm_prefill(ids, want_logits=True, **kw)
    assert np.array_equal(la.view(np.uint32), lc.view(np.uint32)) and np.array_equal(ta, tc)
    moved = 0
    for layer in range(VLM_TINY["layers"]):
        for b in range(3):
            for h in range(VLM_TINY["kv_heads"]):
                (ka, va), (kc, vc) = a.vlm_kv_rows(layer, b, h), c.vlm_kv_rows(layer, b, h)
                assert ka.shape == (21, 128)
                live = slice(int(pad[b]), 21)
                assert np.array_equal(ka[live], _dq(kc[live])) and np.array_equal(va[live], _dq(vc[live])), (layer, b, h)
                moved += int((ka[live] != kc[live]).sum())
    assert moved > 0          # (the format is at work: the image is not the identity)


# ---- 3. the fused decode append ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
def test_decode_append_writes_the_image_of_the_row(engines, planted7, B):
    """Layer 0's K / V of a new token depend only on the token and its position, identical in A and C: its row in A's cache must be the
    image of C's row - through fe_vlm_decode_step (position by value) and through the device-resident loop (position from device
    memory; a captured graph at 1 sequence)."""
    a, c = engines("fp8"), engines("bf16")
    for e in (a, c):
        e.load_weights(FE_MODEL_VLM, planted7)
    L, new = 21, 5
    p = np.random.default_rng(3 + B).integers(0, 2048, (B, L)).astype(np.int32)
    for stepwise in (True, False):
        if stepwise:
            ta, _ = a.vlm_generate(p, 2, want_logits=True)
            tc, _ = c.vlm_generate(p, 2, want_logits=True)
            rows = 1
        else:
            ta, tc = a.vlm_generate(p, new), c.vlm_generate(p, new)
            rows = new - 1
        assert np.array_equal(ta, tc)
        assert a.vlm_dims()["cur_len"] == L + rows
        for b in range(B):
            for h in range(VLM_TINY["kv_heads"]):
                (ka, va), (kc, vc) = a.vlm_kv_rows(0, b, h, L, rows), c.vlm_kv_rows(0, b, h, L, rows)
                assert np.array_equal(ka, _dq(kc)) and np.array_equal(va, _dq(vc)), (stepwise, b, h)
                assert (ka != kc).any()


# ---- 4. the decode kernel alone against float64 ---------------------------------------------------------------------------------------------
# Bound (tests/test_attention_gpu.py, the bf16 row, restated): with Vmax = max|v| over the values the kernel reads (here: the dequantised V)
# and R = the largest spread of visible scores in a row (asserted <= 24),
#     |o - ref| <= 4 * 2^-9 * Vmax + 4 (4 + R) 2^-23 * Vmax
# 2^-9: one rounding of P to bf16 and one of the output, margin 2 each; R 2^-24: __expf's argument error; 4: fp32 accumulation; leading 4:
# margin. Codes times a power of two are exact, so the e4m3 kernel has the bf16 kernel's roundings and no other; the same cases run under
# "bf16" against float64 on the bf16 values with the same bound.
NKV, NSEQ = 2, 2


def _attn_bound(R, vmax):
    return 4.0 * 2.0 ** -9 * vmax + 4.0 * (4.0 + R) * 2.0 ** -23 * vmax


def _attn_inputs(seed, Gq, Lk, jstar, scaled):
    """Random q / k / v (scores ~ N(0, 1) after the kernel's 1 / sqrt(128)) plus, per sequence b, one key jstar[b] every query scores 12
    above its random score (tests/test_attention_gpu.py's planted spike: a unit vector u per KV head, q and k made orthogonal to it
    first). Plain cases: v[j*] = 50. `scaled` cases (Lk >= 8) exercise the per-row scales: v[j*] is a random row times 2^10 (so the output
    is about that row), one other K row is 2^10 s with s in {+-1/2, +-1}^128 - exact in e4m3 - and q orthogonal to s (a moderate score),
    and one further row is zero in K and V."""
    rng = np.random.default_rng(seed)
    nh = NKV * Gq
    q = rng.normal(0, 1, (NSEQ, NKV, Gq, 128))
    k = rng.normal(0, 1, (NSEQ, NKV, Lk, 128))
    v = rng.normal(0, 1, (NSEQ, NKV, Lk, 128))
    u = rng.normal(0, 1, (NKV, 128))
    s = rng.choice([-1.0, -0.5, 0.5, 1.0], (NKV, 128))
    if scaled:
        u -= (u * s).sum(-1, keepdims=True) / (s * s).sum(-1, keepdims=True) * s
        q -= (q * s[None, :, None]).sum(-1, keepdims=True) / (s * s).sum(-1)[None, :, None, None] * s[None, :, None]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q -= (q * u[None, :, None]).sum(-1, keepdims=True) * u[None, :, None]
    k -= (k * u[None, :, None]).sum(-1, keepdims=True) * u[None, :, None]
    ab = np.sqrt(12.0 * np.sqrt(128.0))
    q += ab * u[None, :, None]
    for b in range(NSEQ):
        k[b, :, jstar[b]] += ab * u
        v[b, :, jstar[b]] = 50.0
        if scaled:
            others = [j for j in range(Lk - 1, -1, -1) if j != jstar[b]]
            jk, jz = others[1], others[3]
            v[b, :, jstar[b]] = rng.normal(0, 1, (NKV, 128)) * 1024.0
            k[b, :, jk] = 1024.0 * s
            k[b, :, jz] = 0.0
            v[b, :, jz] = 0.0
    return q.reshape(NSEQ, nh, 128), k, v


def _attn_reference(q, k, v, pad):
    """float64 softmax(q k^T / sqrt(128)) v per head over keys pad[b] .. Lk - 1; returns (o [B, nh, 128], R)."""
    B, nh, _ = q.shape
    Gq = nh // NKV
    qh = np.asarray(q, np.float64).reshape(B, NKV, Gq, 128)
    s = np.einsum("bhgd,bhkd->bhgk", qh, np.asarray(k, np.float64)) / np.sqrt(128.0)
    dead = np.arange(k.shape[2])[None, :] < np.asarray(pad)[:, None]          # [B, Lk]
    s = np.where(dead[:, None, None, :], -np.inf, s)
    hi = s.max(-1, keepdims=True)
    R = float((hi[..., 0] - np.where(np.isinf(s), np.inf, s).min(-1)).max())
    p = np.exp(s - hi)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhgk,bhkd->bhgd", p, np.asarray(v, np.float64)).reshape(B, nh, 128), R


def _attn_geometries():
    out = []
    for Lk in (1, 127, 128, 129, 300):
        for pad in (0, 5, 130):
            if pad >= Lk:
                continue
            pads = (pad, pad // 2)          # per sequence
            # the spike at the first live key, at each chunk boundary inside the live keys, at the last key
            spots = sorted({pad, Lk - 1} | {j for j in (127, 128, 255, 256) if pad <= j < Lk})
            for j in spots:
                out.append((Lk, pads, (j, max(j, pads[1]))))
    return out


@pytest.fixture(scope="module")
def attn_engine():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 30)
    yield e
    e.close()


@pytest.mark.parametrize("kv", ["fp8", "bf16"])
@pytest.mark.parametrize("Gq", [1, 2, 3, 4, 5, 6, 7, 8])          # every instantiation the host dispatches
def test_decode_attention_kernel_against_float64(attn_engine, Gq, kv):
    e = attn_engine
    image = _dq if kv == "fp8" else _bf16
    worst = (0.0, None)
    n = 0
    for Lk, pads, jstar in _attn_geometries():
        for scaled in ((False, True) if Lk >= 8 else (False,)):
            q, k, v = _attn_inputs(1000 * Lk + 10 * jstar[0] + Gq + (500000 if scaled else 0), Gq, Lk, jstar, scaled)
            qi, ki, vi = _bf16(q), image(k), image(v)
            ref, R = _attn_reference(qi, ki, vi, pads)
            vmax = float(np.abs(vi).max())
            assert R <= 24.0, f"input spread {R:.1f}: the derived bound assumes R <= 24"
            # the spike decides the output (plain cases: about 50 in every dimension)
            assert scaled or ref.min() > 40.0
            tol = _attn_bound(R, vmax)
            for from_dev in (False, True):
                out, kimg, vimg = e.vlm_decode_attention(q, k, v, pad=pads, kv_format=kv, len_from_device=from_dev)
                assert np.array_equal(kimg, ki) and np.array_equal(vimg, vi), (Lk, pads, jstar, scaled, from_dev)
                err = float(np.abs(out - ref).max())
                n += 1
                if err / tol > worst[0]:
                    worst = (err / tol, (Lk, pads, jstar, scaled, from_dev, err, tol, R, vmax))
                assert err <= tol, f"{kv} G={Gq} Lk={Lk} pad={pads} spike={jstar} scaled={scaled} len_from_device={from_dev}: |o - ref| {err:.3e} > bound {tol:.3e} (R {R:.1f}, Vmax {vmax:.1f})"
    print(f"[vlm decode attention {kv} G={Gq}] {n} launches, worst |o - ref| / bound {worst[0]:.3f} at (Lk, pads, spike, scaled, len_from_device, err, bound, R, Vmax) = {worst[1]}")


# ---- 5. A ("fp8") against B ("bf16_e4m3"): the same arithmetic on other storage ---------------------------------------------------------------
def _a_against_b(a, b, p, steps=6, **kw):
    ta, la = a.vlm_generate(p, steps, want_logits=True, **kw)
    tb, lb = b.vlm_generate(p, steps, want_logits=True, **kw)
    d = float(np.abs(la - lb).max())
    print(f"[vlm kv fp8 A/B] {p.shape[0]} sequences: max |logit diff| {d:.4f} (scale {np.abs(lb).max():.1f}, B's smallest margin {_margin(lb).min():.2f})")
    assert np.array_equal(ta, tb), p.shape
    assert d <= 0.125, (p.shape, d)          # the bound of test_decode_kernels_agree_across_batch_sizes (tests/test_vlm_gpu.py)
    assert np.array_equal(a.vlm_generate(p, steps, **kw), tb), p.shape          # device-resident loop
    assert np.array_equal(b.vlm_generate(p, steps, **kw), tb), p.shape
    return tb


def test_fp8_cache_against_the_bf16_cache_of_the_same_values(engines, planted7):
    a, b = engines("fp8"), engines("bf16_e4m3")
    for e in (a, b):
        e.load_weights(FE_MODEL_VLM, planted7)
    rng = np.random.default_rng(12)
    for B in (1, 2, 3, 5, 8, 32):
        _a_against_b(a, b, rng.integers(0, 2048, (B, 21)).astype(np.int32))
    # a left-padded batch (pads inside the first decode chunk)
    ids, am, pos = _padded_batch([21, 9, 14], 5)
    tb = _a_against_b(a, b, ids, position_ids=pos, attention_mask=am)
    # the loop that stops at EOS: the third token of row 0 as the EOS id
    eos = [int(tb[0, 2])]
    ua = a.vlm_generate(ids, 6, position_ids=pos, attention_mask=am, eos_token_ids=eos, stop_at_eos=True, poll=1)
    ub = b.vlm_generate(ids, 6, position_ids=pos, attention_mask=am, eos_token_ids=eos, stop_at_eos=True, poll=1)
    assert np.array_equal(ua, ub) and (ua[0, 2:] == eos[0]).all()


def _tied_planted3():          # tests/test_vlm_fp8_gpu.py: a tied Qwen3-VL text checkpoint with a decisive read-out
    sd = synthetic_state_dict(None, 11, spec=qwen3_vl_text_spec(**VLM3_TINY, tied=True))
    E = "model.language_model.embed_tokens.weight"
    sd[E] = np.random.default_rng([11, 78]).standard_normal(sd[E].shape).astype(np.float32)
    sd["model.language_model.norm.weight"] = (sd["model.language_model.norm.weight"] / 16).astype(np.float32)
    return sd


def test_fp8_cache_qwen3_family(engines):
    """G = 2, the one-wave-per-head rope kernel with q / k norms"""
    conf = lambda e: e.vlm3_configure(n_heads=VLM3_TINY["heads"], n_kv_heads=VLM3_TINY["kv_heads"], head_dim=128, rope_theta=5e6, rms_eps=1e-6,
                                      mrope_section=(24, 20, 20), vis_heads=2, deepstack_indexes=())
    sd = _tied_planted3()
    a, b, c = engines("fp8", configure=conf), engines("bf16_e4m3", configure=conf), engines("bf16", configure=conf)
    for e in (a, b, c):
        e.load_weights(FE_MODEL_VLM, sd)
    for B in (2, 5):
        p = np.random.default_rng(12).integers(0, 2000, (B, 21)).astype(np.int32)
        _a_against_b(a, b, p)
        c.vlm_generate(p, 6)
        for h in range(VLM3_TINY["kv_heads"]):          # layer 0's rows, prompt and appended: the image of the bf16 engine's
            (ka, va), (kc, vc) = a.vlm_kv_rows(0, B - 1, h), c.vlm_kv_rows(0, B - 1, h)
            assert ka.shape == (26, 128) and np.array_equal(ka[:21], _dq(kc[:21])) and np.array_equal(va[:21], _dq(vc[:21]))


def test_fp8_cache_qwen2_family(engines):
    """G = 6 over one KV head (the Qwen2-VL tiny configuration)"""
    conf = lambda e: e.vlm2_configure(n_heads=VLM2_TINY["heads"], n_kv_heads=VLM2_TINY["kv_heads"], head_dim=128, rope_theta=1e6, rms_eps=1e-6,
                                      mrope_section=(16, 24, 24), vis_heads=2)
    sd = _planted(5, "qwen2_vl_tiny_untied", VLM2_TINY["vocab"])
    a, b = engines("fp8", configure=conf), engines("bf16_e4m3", configure=conf)
    for e in (a, b):
        e.load_weights(FE_MODEL_VLM, sd)
    for B in (2, 5):
        _a_against_b(a, b, np.random.default_rng(13).integers(0, 2000, (B, 21)).astype(np.int32))


def test_fp8_cache_with_fp8_weights(engines, planted7):
    a, b = engines("fp8", weights="fp8"), engines("bf16_e4m3", weights="fp8")
    for e in (a, b):
        e.load_weights(FE_MODEL_VLM, planted7)
    assert a.vlm_weight_info()["format"] == "fp8" and a.vlm_kv_info()["format"] == "fp8"
    for B in (2, 8):
        _a_against_b(a, b, np.random.default_rng(14).integers(0, 2048, (B, 21)).astype(np.int32))


# ---- 6. 7B geometry, one layer ---------------------------------------------------------------------------------------------------------------
def test_7b_geometry_one_layer(engines):
    """28 heads over 4 KV heads (G = 7), hidden 3584, 150-token prompts (two key chunks). A teacher-forced on B's tokens; every logit within
    max|B logits| * 2^-6 and ids equal wherever B's top-2 margin exceeds twice that: the rule of test_shapes_where_a_kernel_can_go_wrong
    (tests/test_vlm_fp8_gpu.py)."""
    cfg = dict(hidden=3584, layers=1, heads=28, kv_heads=4, inter=18944, vocab=4096)
    sd = synthetic_state_dict(None, 21, spec=qwen2_5_vl_text_spec(**cfg))
    a, b = engines("fp8", cfg), engines("bf16_e4m3", cfg)
    for e in (a, b):
        e.load_weights(FE_MODEL_VLM, sd)
    for B in (2, 8):
        p = np.random.default_rng(9).integers(0, cfg["vocab"], (B, 150)).astype(np.int32)
        tb, lb = b.vlm_generate(p, 4, want_logits=True)
        ta, la = a.vlm_generate(p, 4, want_logits=True, forced_tokens=tb)
        tol = float(np.abs(lb).max()) * 2.0 ** -6
        d = float(np.abs(la - lb).max())
        decisive = _margin(lb) > 2 * tol
        print(f"[vlm kv fp8: 7B width, 1 layer] {B} sequences: max |logit diff| {d:.4f} of scale {np.abs(lb).max():.2f} (tol {tol:.4f}); argmax equal on "
              f"{int(((ta == tb) & decisive).sum())} of {int(decisive.sum())} decisive steps")
        assert d <= tol, (B, d, tol)
        assert ((ta == tb) | ~decisive).all(), B


# ---- 7. against the golden of transformers' class over a quantising cache ------------------------------------------------------------------
def test_greedy_ids_of_the_independent_implementation(engines):
    """The 40 token ids of both prompts; logits of the first and last step and every step's winning logit within 0.25, the tolerances
    tests/test_vlm_gpu.py applies to vlm_golden.npz."""
    a = engines("fp8")
    a.load_weights(FE_MODEL_VLM, _planted(int(G["seed_w"])))
    toks, logits = a.vlm_generate(G["prompts"], G["tokens"].shape[1], want_logits=True)
    err0, err1 = np.abs(logits[:, 0] - G["logits_step0"]).max(), np.abs(logits[:, -1] - G["logits_last"]).max()
    print(f"[vlm kv fp8 golden] tokens equal: {np.array_equal(toks, G['tokens'])}; logits |diff| step 0 {err0:.4f}, last step {err1:.4f} "
          f"(scale {np.abs(G['logits_step0']).max():.1f}, reference top-2 margin >= {G['margin'].min():.2f})")
    assert np.array_equal(toks, G["tokens"])
    assert err0 <= 0.25 and err1 <= 0.25
    assert np.abs(logits.max(-1) - G["top_logit"]).max() <= 0.25
    assert np.array_equal(a.vlm_generate(G["prompts"], G["tokens"].shape[1]), G["tokens"])          # device-resident loop (captured graph)


# ---- 8. what the format costs ------------------------------------------------------------------------------------------------------------------
def test_against_the_bf16_cache(engines, planted7):
    """Reported, not bounded - the difference is the property of the format - except that the ids of the planted checkpoint must be
    identical. A against C on the same state dict."""
    a, c = engines("fp8"), engines("bf16")
    for e in (a, c):
        e.load_weights(FE_MODEL_VLM, planted7)
    p = np.random.default_rng(12).integers(0, 2048, (4, 21)).astype(np.int32)
    ta, la = a.vlm_generate(p, 12, want_logits=True)
    tc, lc = c.vlm_generate(p, 12, want_logits=True)
    d = np.abs(la - lc)
    print(f"[vlm fp8 KV cache against the bf16 cache] ids equal on {int((ta == tc).sum())} of {ta.size}; |logit diff| max {d.max():.4f}, mean {d.mean():.5f} "
          f"(logit scale {np.abs(lc).max():.1f}, bf16 engine's smallest top-2 margin {_margin(lc).min():.2f})")
    assert np.array_equal(la[:, 0], lc[:, 0])          # the prefill
    assert np.array_equal(ta, tc)


# ---- 9. state ---------------------------------------------------------------------------------------------------------------------------------
def test_format_is_state_of_the_context(engines, planted7):
    from facet_amd import EngineError
    e, fresh = engines("bf16"), engines("bf16")
    for x in (e, fresh):
        x.load_weights(FE_MODEL_VLM, planted7)
    p = np.random.default_rng(5).integers(0, 2048, (3, 21)).astype(np.int32)
    with pytest.raises(ValueError, match="int4"):
        e.vlm_kv_format("int4")
    with pytest.raises(EngineError, match="kv_format"):          # the C entry point refuses an unknown code and keeps the state
        e._ck(e.lib.fe_vlm_set_kv_format(e.h, 7))
    assert e.vlm_kv_info()["format"] == "bf16"
    first = e.vlm_prefill(p, max_seq=40)
    bytes_bf16 = e.vlm_kv_info()["allocated_bytes"]
    e.vlm_kv_format("bf16")          # the same format: the cache stays
    e.vlm_decode_step(first, np.full((3, 3), 21, np.int32))
    e.vlm_kv_format("fp8")          # another: the cache is gone
    assert e.vlm_kv_info() == dict(format="fp8", bytes_per_token=VLM_TINY["layers"] * VLM_TINY["kv_heads"] * 264, allocated_bytes=0, max_seq=0)
    with pytest.raises(EngineError, match="call fe_vlm_prefill"):
        e.vlm_decode_step(first, np.full((3, 3), 21, np.int32))
    with pytest.raises(EngineError, match="call fe_vlm_prefill"):
        e.vlm_generate_until(first, np.full((3, 3), 21, np.int32), 2, [0])
    with pytest.raises(EngineError, match="call fe_vlm_prefill"):
        e.vlm_kv_rows(0, 0, 0, 0, 1)
    e.vlm_prefill(p, max_seq=40)
    assert e.vlm_kv_info()["allocated_bytes"] * 512 == bytes_bf16 * 264 and e.vlm_kv_info()["max_seq"] == 40
    t8 = e.vlm_generate(p, 4)
    # back to bf16: the bits of an engine that never left it
    e.vlm_kv_format("bf16")
    t0, l0 = e.vlm_generate(p, 4, want_logits=True)
    t1, l1 = fresh.vlm_generate(p, 4, want_logits=True)
    assert np.array_equal(t0, t1) and np.array_equal(l0.view(np.uint32), l1.view(np.uint32))
    assert np.array_equal(e.vlm_generate(p, 4), fresh.vlm_generate(p, 4)) and np.array_equal(t8, t0)
    for layer in (0, VLM_TINY["layers"] - 1):
        (k0, v0), (k1, v1) = e.vlm_kv_rows(layer, 2, 1), fresh.vlm_kv_rows(layer, 2, 1)
        assert np.array_equal(k0, k1) and np.array_equal(v0, v1)
