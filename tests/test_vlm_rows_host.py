"""CPU: the test hooks of the VLM decoders' row passes (fe_op_vlm_rope_cache, fe_op_vlm_rows, fe_op_vlm_vis_rope) are exported, declared,
documented and bound; every case tests/test_vlm_rows_gpu.py runs stays under the fragile-share cap, computed from the reference alone;
the emulations of tests/vlm_rows_ref.py agree with their own float64 guards; and the comparison can fail: modelled faults, applied in
numpy to the reference's outputs (no kernel and no project code is altered), are rejected on cases of the GPU list while the unfaulted
outputs are accepted."""
import ctypes
import os
import re

import numpy as np
import pytest

import vlm_rows_ref as R
from facet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF0 = dict(cosf=0, sinf=0, rsqrtf=0, expf=0)


@pytest.mark.parametrize("name, n_args, method", [("fe_op_vlm_rope_cache", 25, "vlm_rope_cache"), ("fe_op_vlm_rows", 17, "vlm_rows"),
                                                  ("fe_op_vlm_vis_rope", 10, "vlm_vis_rope")])
def test_new_symbols_are_exported_declared_documented_and_bound(name, n_args, method):
    lib = ctypes.CDLL(os.path.join(ROOT, "facet_amd", "libfacet_engine.so"))
    header = open(os.path.join(ROOT, "include", "facet_engine.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(lib, name)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header)
    assert decl and len(decl.group(1).split(",")) == n_args          # the header's parameter count
    assert name in doc and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert callable(getattr(_lib.Engine, method))


def test_route_and_family_tables():
    assert _lib.Engine.VLM_ROWS_ROUTES == {r: i for i, r in enumerate(R.ROW_ROUTES)}
    assert _lib.Engine.VLM_ROPE_FAMILIES == {"qwen2_5": 0, "qwen3": 1}
    assert R.FILL == 0xA5 and set(R.KV_FORMATS) == set(_lib.VLM_KV_FORMATS)


def test_the_helpers_are_the_only_launch_sites():
    """Each of these kernels is launched from one host function, which vlm_forward and the hooks call."""
    src = "".join(open(os.path.join(ROOT, "facet_amd", "csrc", f)).read() for f in ("model_vlm.hip", "model_vlm_vision.hip", "model_vlm_ln_vision.hip", "capi_ops.hip",
                                                                                  "capi_vlm.hip"))
    launch = lambda kernel, text: len(re.findall(r"hipLaunchKernelGGL\(\(?%s" % re.escape(kernel), text))
    for kernel, sites in (("vlm_rope_cache_kernel<", 1), ("vlm3_qk_rope_cache_kernel<", 1), ("vlm_rmsnorm_kernel,", 1), ("vlm_add_kernel,", 1),
                          ("vlm_silu_mul_kernel,", 1), ("vlm_add_rmsnorm_kernel<", 2), ("vlm_vis_rope_kernel<", 2), ("vlm_attn_decode_gqa_kernel<", 2),
                          ("vlm_gemv_kernel<", 1)):
        assert launch(kernel, src) == sites, kernel
    assert "_e4m3_kernel" not in src          # one decode attention and one GEMV kernel name, whatever the storage
    # the decode attention (one launch per cache storage) and the GEMV are launched inside their host functions and nowhere else
    attn = src[src.index("void vlm_decode_attention("):src.index("void vlm_prefill_attention(")]
    gemv = src[src.index("static void vlm_gemv("):src.index("vlm_gemm32_kernel(")]
    assert launch("vlm_attn_decode_gqa_kernel<GG, uint8_t>", attn) == 1 and launch("vlm_attn_decode_gqa_kernel<GG, bf16>", attn) == 1
    assert launch("vlm_gemv_kernel<MR, TO, WT>", gemv) == 1
    fwd = src[src.index("void vlm_forward("):src.index("void vlm_select(")]
    assert "hipLaunchKernelGGL(vlm_finish_add_rmsnorm_kernel" not in fwd and fwd.count("vlm_few_rows_rmsnorm(") == 2 and "vlm_rope_cache(c, rope" in fwd


# ---- the arithmetic of the reference module itself -----------------------------------------------------------------------------------
def test_bf16_and_ulp_helpers():
    v = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, -0.0, np.inf, 3.0e38], np.float32)
    assert np.array_equal(R.bf16(v)[:4], np.array([1.0, 1.0 + 2.0 ** -6, 1.0, -0.0], np.float32))          # ties to even
    assert np.signbit(R.bf16(v)[3]) and np.isinf(R.bf16(v)[4]) and np.isnan(R.bf16(np.float32(np.nan)))
    assert np.array_equal(R.from_bits16(R.bits16(R.bf16(v))), R.bf16(v))
    one = np.float32(1)
    assert R.ulps(one, 2) == one + np.float32(2.0 ** -22) and R.ulps(one, -2) == one - np.float32(2.0 ** -23) and np.isinf(R.ulps(np.float32(np.inf), -1))
    # the variants bracket the centre, are exact where the function is, and leave an overflow alone
    a = np.array([0.0, 1.0, 89.0, 4000.0], np.float32)
    for fn in ("cosf", "sinf", "expf"):
        lo, mid, hi = (R.dev(fn, a, o) for o in (-1, 0, 1))
        assert lo[0] == mid[0] == hi[0] and (lo[1:] <= mid[1:]).all() and (mid[1:] <= hi[1:]).all()
        assert fn != "expf" or (np.isinf(lo[2:]).all() and np.isinf(hi[2:]).all())
        assert (hi[1:2].view(np.uint32).astype(np.int64) - lo[1:2].view(np.uint32).astype(np.int64) == 2 * R.K[fn]).all()
    assert R.dev("rsqrtf", np.float32(np.inf), -1) == 0 and R.dev("rsqrtf", np.float32(4), 0) == 0.5
    assert R.half_ulp_bf16(1.0) == 2.0 ** -8 and R.half_ulp_bf16(255.5) == 0.5 and R.half_ulp_bf16(0.0) == 0.0


def test_reductions_on_exact_rows():
    """Integer rows: every order of additions is exact, so both reduction orders give the plain sum of squares."""
    rng = np.random.default_rng(0)
    for d in (8, 252, 260, 4352):
        v = rng.integers(-7, 8, (3, d)).astype(np.float32)
        want = (v.astype(np.float64) ** 2).sum(1)
        assert want.max() < 2 ** 24
        assert np.array_equal(R.sumsq_wave(v), want) and np.array_equal(R.sumsq_few_rows(v), want)
    # random rows: the two orders are different roundings of the same sum
    v = R.bf16(rng.normal(0, 1, (64, 4352)))
    a, b, want = R.sumsq_wave(v), R.sumsq_few_rows(v), (v.astype(np.float64) ** 2).sum(1)
    assert (a != b).any() and np.abs(a - want).max() < 2.0 ** -18 * want.max() and np.abs(b - want).max() < 2.0 ** -18 * want.max()


def test_component_maps():
    from facet_amd.vlm_tagger import interleaved_mrope_components
    assert np.array_equal(R.components("qwen3", (20, 20)), interleaved_mrope_components((24, 20, 20)))
    assert np.array_equal(R.components("qwen3", (12, 17)), interleaved_mrope_components((35, 12, 17)))
    assert np.array_equal(R.components("qwen2_5", (16, 24)), np.repeat([0, 1, 2], [16, 24, 24]))
    assert np.array_equal(R.components("qwen2_5", (8, 8)), np.repeat([0, 1, 2], [8, 8, 48]))


def test_small_grids_make_three_trips_with_a_partial_last_one():
    cases = list(R.rope_cases().values()) + list(R.rows_cases().values()) + list(R.vis_cases().values())
    assert sum(c["small_grid"] is not None for c in cases) > len(cases) // 2
    for c in R.rope_cases().values():
        n = c["B"] * c["L"] * (c["nh"] + 2 * c["nkv"]) * 64
        per = c["small_grid"] * 256
        assert -(-n // per) >= 3 and n % per != 0 and per % 64 == 0, c["id"]
    for c in R.rows_cases().values():
        if c["rows"] == 65 and c["route"] not in ("few_rows_rmsnorm",):          # more rows than the capped launch has waves
            assert c["small_grid"] is not None and (c["route"] in ("add", "silu_mul") or c["small_grid"] * 4 < c["rows"]), c["id"]


def test_case_lists_cover_what_the_issue_names():
    rc = R.rope_cases()
    for family in ("qwen2_5", "qwen3"):
        for geom in R.GEOMETRIES:
            for form in R.FORMS:
                assert "%s-%dq%dkv-%s-random-s%dx%d" % ((family,) + geom + (form,) + R.SECTIONS[family][0]) in rc
        assert {c["sections"] for c in rc.values() if c["family"] == family} == set(R.SECTIONS[family])
    assert R.SECTIONS["qwen2_5"] == ((16, 24), (8, 8)) and 3 * 12 != 3 * 17 and 3 * 17 < 64
    assert any((c["nh"] + 2 * c["nkv"]) % 2 for c in rc.values())
    f = R.FORMS
    assert f["staged"][:4] == (3, 5, 0, 5) and f["prefill"][:4] == (3, 5, 0, 23) and f["cont"][:3] == (3, 4, 11) and f["decode"][:3] == (5, 1, 37)
    assert f["decode_dev"][4] and f["cont"][5] == ("bf16",) and f["decode"][5] == R.KV_FORMATS
    assert (np.asarray([c["pos"].max() for c in rc.values()]) < 4096).all()
    rows = R.rows_cases().values()
    for route in ("rmsnorm", "add_rmsnorm", "add_rmsnorm_no_w", "add_rmsnorm_ds"):
        got = {(c["rows"], c["d"]) for c in rows if c["route"] == route and c["kind"] == "random" and c["ldx"] == c["d"]}
        assert got == {(r, d) for r in R.ROW_ROWS for d in R.ROW_D}
        assert {c["eps"] for c in rows if c["route"] == route} == {1e-6, 1e-5}
    assert {(c["rows"], c["d"], c["eps"]) for c in rows if c["route"] == "few_rows_rmsnorm" and c["kind"] == "random"} == \
        {(r, d, e) for r in (1, 64) for d in (512, 4352) for e in (1e-6, 1e-5)}
    ds = [c for c in rows if c["route"] == "add_rmsnorm_ds" and c["rows"] == 65][0]["slot"]
    assert (ds == -1).any() and (ds >= 0).any() and (np.bincount(ds[ds >= 0]) > 1).any()
    silu = [c for c in rows if c["route"] == "silu_mul"]
    assert {c["alias"] for c in silu} == {False, True} and any(c["rows"] * c["d"] == 4 for c in silu) and any((c["rows"] * c["d"] // 4) % 2 for c in silu)
    big = [c for c in silu if c["rows"] == 65][0]["x"]
    assert (big < -88.73).any() and (big >= 40).any() and (big == 0).any()
    assert {(c["hd"], c["heads"], c["rows"], c["kind"]) for c in R.vis_cases().values()} == \
        {(hd, h, r, k) for hd in (64, 80) for h in (1, 3) for r in (1, 70) for k in ("random", "zero")}


# ---- the fragile-share cap, for every case the GPU test runs ----------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(R.rope_cases()))
def test_fragile_share_rope(case_id):
    c, e = R.rope_cases()[case_id], R.rope_expect(case_id)
    for fmt in c["formats"]:
        assert e.fragile_share(fmt) <= R.FRAGILE_CAP, (case_id, fmt, e.fragile_share(fmt))
    if c["kind"] == "zero" and c["family"] == "qwen2_5":          # cosf(0) = 1, sinf(0) = 0: the kernel moves bits
        x = c["qkv"].reshape(-1, c["nh"] + 2 * c["nkv"], 128)
        assert e.q.n_fragile == e.krows.n_fragile == 0
        assert np.array_equal(R.bits16(e.q.center), R.bits16(x[:, :c["nh"]])) and np.array_equal(R.bits16(e.krows.center), R.bits16(x[:, c["nh"]:c["nh"] + c["nkv"]]))
    # the unfaulted model of the outputs passes its own check, and the guard accepts it
    for fmt in c["formats"]:
        assert e.check(fmt, *e.model_outputs(fmt)) == [], (case_id, fmt)
    (rq, rk, _), (bq, bk) = R.guard_rope(c)
    assert R.worst(e.q.center, rq, bq) <= 1.0 and R.worst(e.krows.center, rk, bk) <= 1.0


@pytest.mark.parametrize("case_id", list(R.rows_cases()))
def test_fragile_share_rows(case_id):
    c = R.rows_cases()[case_id]
    ex, en = R.rows_expect(case_id)
    out_x = None if ex is None else ex.center
    out_n = None if en is None else np.pad(en.center, ((0, 0), (0, c["ldy"] - c["d"])), constant_values=768)
    bad, share = R.rows_check(case_id, out_x, out_n)
    assert bad == [] and share <= R.FRAGILE_CAP, (case_id, bad, share)
    assert R.rows_guard(case_id, out_x, out_n) <= 1.0
    if c["route"] in ("add", "add_rmsnorm_no_w"):
        assert share == 0


@pytest.mark.parametrize("case_id", list(R.vis_cases()))
def test_fragile_share_vision_rope(case_id):
    c = R.vis_cases()[case_id]
    q, k = R.vis_expect(case_id)
    share = (q.n_fragile + k.n_fragile) / (q.center.size + k.center.size)
    assert share <= R.FRAGILE_CAP and (c["kind"] != "zero" or share == 0)
    if c["kind"] == "zero":
        x = c["qkv"].reshape(c["rows"], 3, -1)
        assert np.array_equal(q.center, x[:, 0]) and np.array_equal(k.center, x[:, 1])
    (rq, rk), (bq, bk) = R.guard_vis_rope(c)
    assert R.worst(q.center, rq, bq) <= 1.0 and R.worst(k.center, rk, bk) <= 1.0


# ---- the checks can fail ----------------------------------------------------------------------------------------------------------------
ROPE_FAULTS = {          # fault -> (format, cases): rejected on at least one of them
    "section": ("bf16", ["qwen2_5-4q2kv-prefill-random-s16x24", "qwen3-4q2kv-prefill-random-s20x20", "qwen2_5-4q2kv-decode-random-s8x8"]),
    "swap_hw": ("bf16", ["qwen2_5-7q1kv-prefill-random-s16x24", "qwen3-7q1kv-prefill-random-s20x20", "qwen3-4q2kv-decode-random-s12x17"]),
    "routing": ("bf16", ["qwen2_5-3q1kv-decode-random-s16x24", "qwen3-3q1kv-decode-random-s20x20"]),
    "freq_partner": ("bf16", ["qwen2_5-3q1kv-cont-random-s16x24", "qwen3-3q1kv-cont-random-s20x20"]),
    "start": ("bf16", ["qwen2_5-4q2kv-prefill-random-s16x24", "qwen3-7q1kv-cont-random-s20x20"]),
    "row_L": ("bf16", ["qwen2_5-4q2kv-prefill-random-s16x24", "qwen3-3q1kv-cont-random-s20x20"]),
    "cos_unrounded": ("bf16", ["qwen2_5-4q2kv-staged-random-s16x24", "qwen3-4q2kv-staged-random-s20x20"]),
    "product_unrounded": ("bf16", ["qwen2_5-7q1kv-staged-random-s16x24", "qwen3-7q1kv-staged-random-s20x20"]),
    "qn_kn": ("bf16", ["qwen3-4q2kv-decode-random-s20x20", "qwen3-3q1kv-prefill-random-s20x20"]),
    "neighbour_scale": ("fp8", ["qwen2_5-4q2kv-decode-random-s16x24", "qwen3-4q2kv-decode_dev-random-s20x20", "qwen2_5-4q2kv-decode-special-s16x24"]),
    "v_with_k_scale": ("fp8", ["qwen2_5-7q1kv-decode-random-s16x24", "qwen3-3q1kv-decode-random-s20x20", "qwen3-4q2kv-decode-special-s20x20"]),
}


@pytest.mark.parametrize("fault", list(ROPE_FAULTS))
def test_planted_rope_faults_are_rejected(fault):
    fmt, cases = ROPE_FAULTS[fault]
    rejected = []
    for case_id in cases:
        e = R.rope_expect(case_id)
        assert e.check(fmt, *e.model_outputs(fmt)) == [], case_id
        bad = e.check(fmt, *e.model_outputs(fmt, fault))
        if bad:
            rejected.append(case_id)
            # which output notices: the routing and rounding faults show in q and K, the placement faults in the caches
            if fault in ("start", "row_L", "neighbour_scale", "v_with_k_scale"):
                assert not any(b.startswith("q:") for b in bad), bad
            else:
                assert any(b.startswith("q:") for b in bad) and any(b.startswith("k cache") for b in bad), bad
    assert len(rejected) == len(cases), (fault, rejected)
    if fault in ("neighbour_scale", "v_with_k_scale"):          # the same faults under the image format
        e = R.rope_expect(cases[0])
        assert e.check("bf16_e4m3", *e.model_outputs("bf16_e4m3")) == [] and e.check("bf16_e4m3", *e.model_outputs("bf16_e4m3", fault))


def test_a_text_prompt_would_hide_the_routing_faults():
    """Why the cases draw the three components independently: with equal components every routing fault returns the correct bits."""
    c = dict(R.rope_cases()["qwen3-4q2kv-prefill-random-s20x20"])
    c["pos"] = np.broadcast_to(c["pos"][:1], c["pos"].shape).copy()
    want = R.emu_rope(c, OFF0)
    for fault in ("section", "swap_hw", "routing"):
        assert all(np.array_equal(a, b) for a, b in zip(R.emu_rope(c, OFF0, fault), want))


ROWS_FAULTS = {
    "ds_minus1_as_0": ["add_rmsnorm_ds-3x260-random-eps1e-06", "add_rmsnorm_ds-65x1536-random-eps1e-06"],
    "sum_unrounded": ["add_rmsnorm-3x260-random-eps1e-06", "add_rmsnorm-65x3584-random-eps1e-05"],
    "silu_unrounded": ["silu_mul-3x260-random-eps1e-06", "silu_mul-65x1536-random-eps1e-06-alias"],
}


@pytest.mark.parametrize("fault", list(ROWS_FAULTS))
def test_planted_row_faults_are_rejected(fault):
    for case_id in ROWS_FAULTS[fault]:
        c = R.rows_cases()[case_id]
        ox, on = R.rows_emulate(c, OFF0, fault)
        bad, _ = R.rows_check(case_id, ox, on)
        assert bad, (fault, case_id)
        assert R.rows_check(case_id, *R.rows_emulate(c, OFF0))[0] == []


def test_one_ulp_and_misplaced_results_are_rejected():
    """The comparison itself: one bf16 ulp on one firm element, a neighbour's row."""
    case_id = "rmsnorm-65x3584-random-eps1e-05"
    c = R.rows_cases()[case_id]
    _, n = R.rows_emulate(c, OFF0)
    i = tuple(np.argwhere(R.rows_expect(case_id)[1].firm & (n != 0))[7])
    off = n.copy()
    off[i] = R.from_bits16(R.bits16(np.array([n[i]])) + np.uint16(1))[0]
    assert R.rows_check(case_id, None, off)[0] and R.rows_check(case_id, None, np.roll(n, 1, 0))[0]
    assert R.rows_check(case_id, None, n)[0] == []
