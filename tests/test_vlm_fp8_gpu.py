"""GPU: e4m3 weights of the VLM decoders (Engine.vlm_weight_format("fp8"): the decode projections stream codes with one power-of-two
scale per output row, facet_amd/csrc/fp8_core.h).

Every dequantised weight is exactly a bf16 value, so the quantised engine is the bf16 engine on other weights, and it is tested against
the bf16 engine - which tests/test_vlm_gpu.py pins to transformers' classes. Below, `A` is an engine under "fp8" loaded with a state
dict `sd`; `B` is a bf16 engine loaded with `sd'` = sd with every quantised matrix (q, k, v, o, gate, up, down of every layer, lm_head)
replaced by dequantize(quantize(w)) in numpy (facet_amd.weights). q, k and v are replaced one by one, which gives the rows of the fused
matrix. A against B then differs only by the summation order of the same products, bounded as the existing decode tests bound it; where
A goes through its bf16 scratch (more than 32 rows) it runs B's kernels on B's bits and must equal it bit for bit.
"""
import numpy as np
import pytest

from facet_amd._lib import FE_MODEL_VLM
from facet_amd.weights import (synthetic_state_dict, qwen2_5_vl_text_spec, qwen3_vl_text_spec, VLM_TINY, VLM3_TINY, quantize_e4m3_rows,
                               dequantize_e4m3_rows)

pytestmark = pytest.mark.gpu

QUANTISED = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "gate_proj.weight", "up_proj.weight", "down_proj.weight")
GEOM = dict(head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24))


def _dq(w):
    return dequantize_e4m3_rows(*quantize_e4m3_rows(w))


def _primed(sd):
    """sd' of the module docstring"""
    return {k: _dq(v) if (k.startswith("model.language_model.layers.") and k.endswith(QUANTISED)) or k == "lm_head.weight" else v for k, v in sd.items()}


def _planted(seed):          # as tests/test_vlm_gpu.py
    sd = synthetic_state_dict("qwen2_5_vl_text_tiny", seed)
    perm = np.random.default_rng([seed, 77]).permutation(VLM_TINY["vocab"])
    sd["lm_head.weight"] = (sd["model.language_model.embed_tokens.weight"][perm] / 16.0).astype(np.float32)
    return sd


@pytest.fixture(scope="module")
def planted7():
    sd = _planted(7)
    return sd, _primed(sd)


@pytest.fixture()
def engines():
    from facet_amd import Engine
    made = []

    def make(fmt, cfg=VLM_TINY, configure=None):
        e = Engine(0, arena_bytes=4 << 30)
        made.append(e)
        if configure:
            configure(e)
        else:
            e.vlm_configure(n_heads=cfg["heads"], n_kv_heads=cfg["kv_heads"], **GEOM)
        e.vlm_weight_format(fmt)
        return e
    yield make
    for e in made:
        e.close()


def _text_spec_hd128(hidden, layers, heads, kv_heads, inter, vocab):
    """qwen2_5_vl_text_spec with the head width fixed at 128 (the spec helper derives it as hidden / heads, which geometry (b) below, 4
    heads over a 576-wide stream, does not satisfy; the engine itself only needs head_dim 128)."""
    spec = []
    for name, shape, kind in qwen2_5_vl_text_spec(hidden=heads * 128, layers=layers, heads=heads, kv_heads=kv_heads, inter=inter, vocab=vocab):
        if name.endswith("o_proj.weight"):
            shape = (hidden, heads * 128)
        elif len(shape) == 2:
            shape = (shape[0], hidden) if not name.endswith("down_proj.weight") else (hidden, inter)
        elif name.endswith("norm.weight") or name.endswith("layernorm.weight"):
            shape = (hidden,)
        spec.append((name, shape, kind))
    return spec


def _margin(lg):
    t2 = np.sort(lg, -1)[..., -2:]
    return t2[..., 1] - t2[..., 0]


def test_weight_info_reports_half_the_bytes(engines, planted7):
    sd, _ = planted7
    a, b = engines("fp8"), engines("bf16")
    a.load_weights(FE_MODEL_VLM, sd)
    b.load_weights(FE_MODEL_VLM, sd)
    ia, ib = a.vlm_weight_info(), b.vlm_weight_info()
    c = VLM_TINY
    rows = c["layers"] * ((c["heads"] + 2 * c["kv_heads"]) * 128 + 2 * c["hidden"] + 2 * c["inter"]) + c["vocab"]
    elems = c["layers"] * ((c["heads"] + 2 * c["kv_heads"]) * 128 * c["hidden"] + c["heads"] * 128 * c["hidden"] + 3 * c["inter"] * c["hidden"]) + c["vocab"] * c["hidden"]
    print(f"[vlm fp8] weight info fp8 {ia}, bf16 {ib}")
    assert ia["format"] == "fp8" and ib["format"] == "bf16"
    assert ib["weight_bytes"] == 2 * elems and 2 * ia["weight_bytes"] == ib["weight_bytes"]          # every K here is a multiple of 64: no row padding
    assert ia["quantized_rows"] == rows and ia["scale_bytes"] == 4 * rows
    assert ib["quantized_rows"] == 0 and ib["scale_bytes"] == 0


def test_dequantise_route_is_the_bf16_engine_bit_for_bit(engines, planted7):
    """40 prompts of 5 tokens: 200 rows in the prefill, 40 in every decode step and at the lm_head - all above the 32 rows the e4m3 kernels
    take, so every projection of A is its bf16 scratch through the shared GEMM. Equal bits also pin the device's reading of the codes to OCP
    e4m3fn with the specified scales (the fnuz reading would halve every weight)."""
    sd, sdp = planted7
    a, b = engines("fp8"), engines("bf16")
    a.load_weights(FE_MODEL_VLM, sd)
    b.load_weights(FE_MODEL_VLM, sdp)
    p = np.random.default_rng(31).integers(0, 2048, (40, 5)).astype(np.int32)
    ta, la = a.vlm_generate(p, 4, want_logits=True)          # the prefill and 3 decode steps
    tb, lb = b.vlm_generate(p, 4, want_logits=True)
    print(f"[vlm fp8] dequantise route: max |logit diff| {np.abs(la - lb).max()}, ids equal {np.array_equal(ta, tb)}")
    assert la.shape == (40, 4, 2048)
    assert np.array_equal(la, lb) and np.array_equal(ta, tb)


def test_streaming_kernels_against_the_bf16_engine(engines, planted7):
    """The e4m3 GEMV (1 .. 3 rows; 4 rows where K is no multiple of 128) and the e4m3 matrix-core GEMM with its fused finishing passes
    (4 .. 32 rows, the paired gate|up launch included), stepwise and in the device-resident loop (captured graph at 1 and 2 sequences).
    Planted read-out (the transformers class on sd' has a smallest top-2 margin of 9.9 here), so ids are identical at every step; logits
    within 0.125, the bound test_decode_kernels_agree_across_batch_sizes uses for different summation orders of the same products."""
    sd, sdp = planted7
    a, b = engines("fp8"), engines("bf16")
    a.load_weights(FE_MODEL_VLM, sd)
    b.load_weights(FE_MODEL_VLM, sdp)
    rng = np.random.default_rng(12)
    for B in (1, 2, 3, 4, 5, 8, 32):
        p = rng.integers(0, 2048, (B, 21)).astype(np.int32)
        ta, la = a.vlm_generate(p, 6, want_logits=True)
        tb, lb = b.vlm_generate(p, 6, want_logits=True)
        d = float(np.abs(la - lb).max())
        print(f"[vlm fp8] streaming kernels, {B} sequences: max |logit diff| {d:.4f} (scale {np.abs(lb).max():.1f}, B's smallest margin {_margin(lb).min():.2f})")
        assert np.array_equal(ta, tb), B
        assert d <= 0.125, (B, d)
        assert np.array_equal(a.vlm_generate(p, 6), tb), B          # device-resident loop, same kernels


@pytest.mark.parametrize("name,cfg,Bs,L", [
    ("7B width, 1 layer", dict(hidden=3584, layers=1, heads=28, kv_heads=4, inter=18944, vocab=4096), (2, 8), 150),
    ("K and N tails", dict(hidden=576, layers=2, heads=4, kv_heads=2, inter=1344, vocab=1001), (3, 6), 19),
])
def test_shapes_where_a_kernel_can_go_wrong(engines, name, cfg, Bs, L):
    """(a) the 7B projections (K = 3584 and 18944: several trips of every K loop, the K split of the GEMM, 28 query heads over 4 KV heads);
    (b) K % 128 = 64 for the q|k|v, gate, up, down and lm_head projections (the GEMM's condition fails: GEMV at 3 rows, bf16 scratch at 6)
    with an odd column count at the head (the geometry as asked for: the bf16 engine takes it; only the spec helper of facet_amd.weights
    does not, see _text_spec_hd128). A teacher-forced on B's tokens; every logit within max|B logits| * 2^-6, the rule of
    test_live_against_transformers_when_importable, and ids equal wherever B's top-2 margin exceeds twice that."""
    sd = synthetic_state_dict(None, 21, spec=_text_spec_hd128(**cfg))
    a, b = engines("fp8", cfg), engines("bf16", cfg)
    a.load_weights(FE_MODEL_VLM, sd)
    b.load_weights(FE_MODEL_VLM, _primed(sd))
    for B in Bs:
        p = np.random.default_rng(9).integers(0, cfg["vocab"], (B, L)).astype(np.int32)
        tb, lb = b.vlm_generate(p, 4, want_logits=True)
        ta, la = a.vlm_generate(p, 4, want_logits=True, forced_tokens=tb)
        tol = float(np.abs(lb).max()) * 2.0 ** -6
        d = float(np.abs(la - lb).max())
        decisive = _margin(lb) > 2 * tol
        print(f"[vlm fp8: {name}] {B} sequences: max |logit diff| {d:.4f} of scale {np.abs(lb).max():.2f} (tol {tol:.4f}); argmax equal on "
              f"{int(((ta == tb) & decisive).sum())} of {int(decisive.sum())} decisive steps")
        assert d <= tol, (B, d, tol)
        assert ((ta == tb) | ~decisive).all(), B


def test_against_the_unquantised_model(engines, planted7):
    """What the format costs, reported: A under fp8 against the bf16 engine on the SAME state dict. The ids must be identical (on the CPU,
    transformers' class gave 48 of 48 ids, max |logit diff| 0.43 at a logit scale of 22, margins >= 9.9); the difference itself is printed,
    not bounded - it is the property of the format, not a defect."""
    sd, _ = planted7
    a, b = engines("fp8"), engines("bf16")
    a.load_weights(FE_MODEL_VLM, sd)
    b.load_weights(FE_MODEL_VLM, sd)
    p = np.random.default_rng(12).integers(0, 2048, (4, 21)).astype(np.int32)
    ta, la = a.vlm_generate(p, 12, want_logits=True)
    tb, lb = b.vlm_generate(p, 12, want_logits=True)
    d = np.abs(la - lb)
    print(f"[vlm fp8 against bf16 weights] ids equal on {int((ta == tb).sum())} of {ta.size}; |logit diff| max {d.max():.4f}, mean {d.mean():.5f} "
          f"(logit scale {np.abs(lb).max():.1f}, bf16 engine's smallest top-2 margin {_margin(lb).min():.2f})")
    assert np.array_equal(ta, tb)


def _tied_planted():
    """A tied Qwen3-VL text checkpoint whose read-out is decisive: unit-scale embeddings (the residual stream keeps its token's direction) and
    the final norm's weight / 16 (logit scale ~10). The random tied checkpoint leaves top-2 margins under 0.1; on this one transformers'
    class, loaded with B's weights on the CPU, has margins >= 3.9 over the steps below."""
    sd = synthetic_state_dict(None, 11, spec=qwen3_vl_text_spec(**VLM3_TINY, tied=True))
    E = "model.language_model.embed_tokens.weight"
    sd[E] = np.random.default_rng([11, 78]).standard_normal(sd[E].shape).astype(np.float32)
    sd["model.language_model.norm.weight"] = (sd["model.language_model.norm.weight"] / 16).astype(np.float32)
    assert "lm_head.weight" not in sd
    return sd


def test_tied_head_keeps_the_bf16_embedding_rows(engines):
    """A: tied, under fp8. B: untied, lm_head = the dequantised table, embed_tokens the ORIGINAL table, projections dequantised. Had A
    looked its embeddings up in the quantised copy, its inputs would be off by up to 2^-4 relative and the logits far outside 0.125."""
    sd = _tied_planted()
    sdp = _primed(sd)
    sdp["lm_head.weight"] = _dq(sd["model.language_model.embed_tokens.weight"])
    conf = lambda e: e.vlm3_configure(n_heads=VLM3_TINY["heads"], n_kv_heads=VLM3_TINY["kv_heads"], head_dim=128, rope_theta=5e6, rms_eps=1e-6,
                                      mrope_section=(24, 20, 20), vis_heads=2, deepstack_indexes=())
    a, b = engines("fp8", configure=conf), engines("bf16", configure=conf)
    a.load_weights(FE_MODEL_VLM, sd)
    b.load_weights(FE_MODEL_VLM, sdp)
    assert a.vlm_weight_info()["quantized_rows"] == b.vlm_weight_info()["quantized_rows"] + sum(v.shape[0] for k, v in sdp.items() if k.endswith(QUANTISED) or k == "lm_head.weight")
    for B in (2, 8):
        p = np.random.default_rng(12).integers(0, 2000, (B, 21)).astype(np.int32)
        ta, la = a.vlm_generate(p, 6, want_logits=True)
        tb, lb = b.vlm_generate(p, 6, want_logits=True)
        d = float(np.abs(la - lb).max())
        print(f"[vlm fp8 tied] {B} sequences: max |logit diff| {d:.4f} (scale {np.abs(lb).max():.1f}, B's smallest margin {_margin(lb).min():.2f})")
        assert np.array_equal(ta, tb) and d <= 0.125, (B, d)
        assert np.array_equal(a.vlm_generate(p, 6), tb), B


def test_format_is_per_commit_state(engines, planted7):
    sd, _ = planted7
    e, fresh = engines("fp8"), engines("bf16")
    p = np.random.default_rng(5).integers(0, 2048, (3, 21)).astype(np.int32)
    e.load_weights(FE_MODEL_VLM, sd)
    assert e.vlm_weight_info()["format"] == "fp8"
    e.vlm_generate(p, 4)
    e.vlm_weight_format("bf16")
    assert e.vlm_weight_info()["format"] == "fp8"          # read by the NEXT commit
    e.load_weights(FE_MODEL_VLM, sd)
    assert e.vlm_weight_info()["format"] == "bf16"
    fresh.load_weights(FE_MODEL_VLM, sd)
    t0, l0 = e.vlm_generate(p, 4, want_logits=True)
    t1, l1 = fresh.vlm_generate(p, 4, want_logits=True)
    assert np.array_equal(t0, t1) and np.array_equal(l0, l1)
    assert np.array_equal(e.vlm_generate(p, 4), fresh.vlm_generate(p, 4))
    e.unload(FE_MODEL_VLM)
    from facet_amd import EngineError
    with pytest.raises(EngineError, match="not loaded"):
        e.vlm_weight_info()


def test_refusals_leave_nothing_loaded(engines, planted7):
    from facet_amd import EngineError
    sd, _ = planted7
    e = engines("fp8")
    bad = dict(sd)
    name = "model.language_model.layers.1.mlp.down_proj.weight"
    bad[name] = sd[name].copy()
    bad[name][37, 5] = np.nan
    with pytest.raises(EngineError, match=r"layers\.1\.mlp\.down_proj\.weight.*NaN"):
        e.load_weights(FE_MODEL_VLM, bad)
    assert not e.loaded(FE_MODEL_VLM)
    bad = dict(sd)
    name = "model.language_model.layers.2.self_attn.k_proj.weight"
    bad[name] = sd[name].copy()
    bad[name][0, 0] = np.inf
    with pytest.raises(EngineError, match=r"layers\.2\.self_attn\.k_proj\.weight.*Inf"):
        e.load_weights(FE_MODEL_VLM, bad)
    assert not e.loaded(FE_MODEL_VLM)
    with pytest.raises(ValueError, match="int4"):
        e.vlm_weight_format("int4")
    with pytest.raises(EngineError, match="weight_format"):          # the C entry point refuses it too
        e._ck(e.lib.fe_vlm_set_weight_format(e.h, 7))
    assert not e.loaded(FE_MODEL_VLM)
    e.load_weights(FE_MODEL_VLM, sd)          # the refused value changed nothing: still fp8
    assert e.loaded(FE_MODEL_VLM) and e.vlm_weight_info()["format"] == "fp8"
