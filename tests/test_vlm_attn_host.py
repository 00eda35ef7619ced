"""CPU: the test hooks of the Qwen-VL attention tile (fe_op_vlm_vis_attention, fe_op_vlm_prefill_attention) are exported, declared,
documented and bound; each of the two kernels has one launch site; every case tests/test_vlm_attn_gpu.py runs satisfies what its bound
assumes, computed from the reference alone (tests/vlm_attn_ref.py); the case list covers what it was built to cover; and the comparison
can fail: modelled faults, applied in numpy to the reference's mask or indexing (no kernel and no project code is altered), miss the
bound on named cases of the GPU list while the unfaulted reference, rounded to bf16, passes on the same cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import vlm_attn_ref as A
from facet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name, n_args, method", [("fe_op_vlm_vis_attention", 10, "vlm_vis_attention"), ("fe_op_vlm_prefill_attention", 12, "vlm_prefill_attention")])
def test_new_symbols_are_exported_declared_documented_and_bound(name, n_args, method):
    lib = ctypes.CDLL(os.path.join(ROOT, "facet_amd", "libfacet_engine.so"))
    header = open(os.path.join(ROOT, "include", "facet_engine.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(lib, name)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header)
    assert decl and len(decl.group(1).split(",")) == n_args          # the header's parameter count
    assert name in doc and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert callable(getattr(_lib.Engine, method))


def test_each_kernel_has_one_launch_site():
    """vlm_vis_attention and vlm_prefill_attention are the only functions that launch the two kernels; vlm_forward and the hooks call them."""
    csrc = os.path.join(ROOT, "facet_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if re.fullmatch(r"model_vlm.*\.hip", f)) + ["capi_ops.hip", "capi_vlm.hip"]
    assert "model_vlm.hip" in files and "model_vlm_vision.hip" in files and "model_vlm_ln_vision.hip" in files
    src = {f: open(os.path.join(csrc, f)).read() for f in files}
    text = "".join(src.values())
    assert len(re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*vlm_attn_prefill_kernel\b", text)) == 1
    # the vision kernel: one site, a launch per instantiated wave count
    sites = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*vlm_vis_attn_kernel<HD, (\d)>", text)
    assert sorted(sites) == ["2", "4"] and text.count("vlm_vis_attn_kernel<") == 2
    body = src["model_vlm_vision.hip"]
    launch = body[body.index("static void vis_attention_launch("):body.index("void vlm_vis_attention(")]
    assert launch.count("hipLaunchKernelGGL") == 2 and body.count("vis_attention_launch<") == 2
    m = src["model_vlm.hip"]
    fwd = m[m.index("void vlm_forward("):m.index("void vlm_select(")]
    assert "vlm_prefill_attention(" in fwd and "hipLaunchKernelGGL(vlm_attn_prefill_kernel" not in fwd and "VlmAttnParams" not in fwd
    helper = m[m.index("void vlm_prefill_attention("):m.index("// ---- the launches of the row passes")]
    assert "hipLaunchKernelGGL(vlm_attn_prefill_kernel" in helper
    hooks = src["capi_ops.hip"]
    assert "vlm_prefill_attention(C," in hooks and "vlm_vis_attention(C," in hooks and "vlm_prefill_attention(" in open(os.path.join(csrc, "engine.h")).read()


def test_the_reference_on_hand_made_inputs():
    """The reference itself, on inputs whose answer is known without it."""
    # vision: two segments of constant v rows -> each row returns its segment's constant whatever the scores are
    rng = np.random.default_rng(0)
    cu = np.array([0, 3, 8], np.int32)
    q, k = A.bf16(rng.normal(0, 1, (8, 2 * 64))), A.bf16(rng.normal(0, 1, (8, 2 * 64)))
    v = np.repeat(np.array([2.0, -3.0]), [3, 5])[:, None] * np.ones((1, 128))
    o, R, S = A.vis_reference(q, k, v, cu, 64, 2)
    assert np.allclose(o, v, atol=1e-12) and 0 < R <= 2 * S
    # prefill: one key visible -> its v row; a pad row -> zeros; the KV head of head h is h // (nh / nkv)
    q = A.bf16(rng.normal(0, 1, (2, 3, 4 * 128)))
    k, v = A.bf16(rng.normal(0, 1, (2, 2, 5, 128))), A.bf16(rng.normal(0, 1, (2, 2, 5, 128)))
    o, _, _ = A.prefill_reference(q, k, v, 4, 2, 2, np.array([2, 3]))
    o = o.reshape(2, 3, 4, 128)
    assert np.array_equal(o[0, 0, 0], v[0, 0, 2]) and np.array_equal(o[0, 0, 3], v[0, 1, 2]) and np.array_equal(o[0, 0, 1], v[0, 0, 2])
    assert (o[1, 0] == 0).all() and np.array_equal(o[1, 1, 2], v[1, 1, 3])
    # two visible keys: the softmax by hand
    s = (q[1, 2].reshape(4, 128).astype(np.float64)[1] * k[1, 0, 3:5].astype(np.float64)).sum(-1) * A.scale_of(128)
    p = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
    assert np.allclose(o[1, 2, 1], p @ v[1, 0, 3:5].astype(np.float64), atol=1e-12)
    assert A.scale_of(64) == 0.125 and abs(A.scale_of(80) - 80 ** -0.5) < 2.0 ** -27


def test_case_list_covers_what_it_names():
    cs = A.cases()
    vis = [c for c in cs.values() if c["kernel"] == "vis"]
    pre = [c for c in cs.values() if c["kernel"] == "prefill"]
    assert A.VIS_LISTS == {"short": (1, 31, 32, 33, 63, 64, 4), "mixed": (65, 4, 128, 97, 1, 129), "long257": (257,), "long300": (300, 64)}
    for family in ("random", "exact"):
        assert {(c["list"], c["hd"], c["heads"]) for c in vis if c["family"] == family} == {(n, hd, h) for n in A.VIS_LISTS for hd in (64, 80) for h in (1, 3)}
    # launches: NW = 2 with one query block, NW = 4 with two and three; the key tile counts of the short list use both buffer parities
    assert max(A.VIS_LISTS["short"]) == 64 and [-(-n // 32) for n in A.VIS_LISTS["short"]] == [1, 1, 1, 2, 2, 2, 1]
    assert -(-max(A.VIS_LISTS["mixed"]) // 128) == 2 and min(A.VIS_LISTS["mixed"]) <= 128 - 1 and 97 % 32 == 1
    assert [-(-n // 32) for n in (257, 300)] == [9, 10] and -(-257 // 128) == -(-300 // 128) == 3
    assert (32 * 80 // 8) % 128 != 0 and (32 * 80 // 8) % 256 != 0 and (32 * 64 // 8) % 128 == 0 and (32 * 64 // 8) % 256 == 0
    # spikes: keys 0, 31, 32 and the last of a segment on every list that has them; first and last keys next to a neighbour segment
    sp = {(c["list"], c["hd"]): set() for c in vis if c["family"] == "spike"}
    for c in vis:
        if c["family"] == "spike":
            seg, key = c["spike"]
            n = c["lens"][seg]
            assert 0 <= key < n
            sp[(c["list"], c["hd"])] |= {"first" if key == 0 else "", "last" if key == n - 1 else "", "k%d" % key if key in (31, 32) else "",
                                         "first-after-a-segment" if key == 0 and seg > 0 else "", "last-before-a-segment" if key == n - 1 and seg + 1 < len(c["lens"]) else ""}
    for hd in (64, 80):
        for name in ("short", "mixed", "long300"):
            assert sp[(name, hd)] >= {"first", "last", "k31", "k32", "first-after-a-segment", "last-before-a-segment"}, (name, hd, sp[(name, hd)])
        assert "last" in sp[("long257", hd)]
    assert {c["heads"] for c in vis if c["family"] == "spike"} == {1, 3}
    # prefill
    for family in ("random", "exact"):
        mine = [c for c in pre if c["family"] == family]
        assert {c["Lq"] for c in mine if (c["nh"], c["nkv"]) == (4, 2)} == set(A.PREFILL_LQ) == {2, 31, 32, 33, 64, 65, 127, 128, 129, 257, 300}
        assert {(c["nh"], c["nkv"]) for c in mine} == {(4, 2), (3, 1), (7, 1)}
        for heads in ((3, 1), (7, 1)):
            assert len({c["Lq"] for c in mine if (c["nh"], c["nkv"]) == heads}) >= 3 and {c["qpos0"] for c in mine if (c["nh"], c["nkv"]) == heads} == {0, 11, 133}
        assert {c["qpos0"] for c in mine} == {0, 11, 133}
        assert {c["max_seq"] - c["qpos0"] - c["Lq"] for c in mine} == {0, 37}
        assert {c["pad"] for c in mine} == {(0, 0), (0, 1), (5, 37), (32, 33), (64, 0), (130, 0)}
        assert {c["Lq"] for c in mine if c["pad"] == (130, 0)} == {257}
        for Lq in A.PREFILL_LQ:          # every length both at the start and in a continued prefill
            assert len({c["qpos0"] for c in mine if c["Lq"] == Lq and c["nh"] == 4}) >= 2
    for c in pre:
        assert max(c["pad"]) < c["qpos0"] + c["Lq"] <= c["max_seq"] <= 8192 and c["nh"] % c["nkv"] == 0
    # (130, 0) at qpos0 0: the first workgroup's 128 queries are all padding and its key loop is empty (kt0 == nt), kt0 odd: parity shifted
    assert 130 // 32 == -(-min(257, 128) // 32) == 4 and (130 // 32) % 2 == 0 and (37 // 32) % 2 == 1 and (33 // 32) % 2 == 1
    # qpos0 11: the first workgroup's kend = 11 + 128 lies inside a tile; 133: past a whole 128-key block
    assert (11 + 128) % 32 != 0 and 133 > 128
    spikes = [c for c in pre if c["family"] == "spike"]
    kinds = set()
    for c in spikes:
        Lk = c["qpos0"] + c["Lq"]
        for b in range(2):
            j, p = c["spike"][b], c["pad"][b]
            assert 0 <= j < Lk
            kinds |= {"k%d" % j if j in (0, 31, 32) else "", "last" if j == Lk - 1 else "", "pad-1" if p and j == p - 1 else "", "pad" if p and j == p else ""}
    assert kinds >= {"k0", "k31", "k32", "last", "pad-1", "pad"} and {(c["nh"], c["nkv"]) for c in spikes} == {(4, 2), (3, 1), (7, 1)}
    assert {c["qpos0"] for c in spikes} == {0, 11, 133}
    # the budget: roughly 150 launches, one per case
    assert 120 <= len(cs) <= 175, len(cs)


@pytest.mark.parametrize("case_id", list(A.cases()))
def test_case_premises(case_id):
    """R and S under the cap, the spike decides the output where it is visible and nowhere else, the exact counts are what the bound
    assumes - and the reference rounded to bf16 (what a correct kernel may return at best) passes its own comparison."""
    assert A.premises(case_id) == []
    ref, R, S, vmax = A.expect(case_id)
    c = A.cases()[case_id]
    assert R <= A.R_CAP and S <= A.R_CAP
    assert vmax == 1.0 if c["family"] == "exact" else vmax == 50.0 if c["family"] == "spike" else 2.0 < vmax < 8.0
    bad, ratio = A.compare(case_id, A.model_output(case_id))
    assert bad == [] and ratio < (1.0 if c["family"] == "exact" else 0.5 + 1e-9), (bad, ratio)          # one rounding of the two the bound has
    if c["kernel"] == "prefill" and A.pad_rows(case_id).any():
        assert (ref[A.pad_rows(case_id)] == 0).all()


def test_the_bound_is_the_derived_formula():
    cid = "vis-random-mixed-hd80-h3"
    ref, R, S, vmax = A.expect(cid)
    assert 6.0 < R < 12.0                                                     # "a spread of about 8"
    assert A.bound(cid) == 4 * 2.0 ** -9 * vmax + 4 * (4 + R + S) * 2.0 ** -23 * vmax
    assert A.bound(cid) < 1.0015 * (4 * 2.0 ** -9 * vmax + 4 * (4 + R) * 2.0 ** -23 * vmax)          # the scale's term: under 0.15 %
    cid = "prefill-exact-4q2kv-L2-p0-x0-pad0_0"
    assert np.array_equal(A.bound(cid), 2.0 ** -8 * np.abs(A.expect(cid)[0]))


# ---- the comparison can fail ---------------------------------------------------------------------------------------------------------------
FAULTS = {          # fault -> cases of the GPU list on each of which it must miss the bound
    "causal_one_late": ["prefill-exact-4q2kv-L2-p0-x0-pad0_0", "prefill-exact-4q2kv-L129-p133-x0-pad0_1", "prefill-random-4q2kv-L64-p11-x0-pad32_33",
                        "prefill-spike-4q2kv-L65-p0-x37-pad0_0-j31_32", "prefill-exact-7q1kv-L300-p11-x37-pad0_1"],
    "causal_one_early": ["prefill-exact-4q2kv-L2-p0-x0-pad0_0", "prefill-exact-4q2kv-L129-p133-x0-pad0_1", "prefill-random-4q2kv-L64-p11-x0-pad32_33",
                         "prefill-spike-4q2kv-L65-p0-x37-pad0_0-j31_32", "prefill-exact-3q1kv-L2-p0-x0-pad0_0"],
    "qpos0_ignored": ["prefill-exact-4q2kv-L2-p11-x37-pad0_1", "prefill-random-4q2kv-L32-p133-x0-pad64_0", "prefill-spike-4q2kv-L33-p133-x0-pad32_33-j165_133",
                      "prefill-exact-7q1kv-L300-p11-x37-pad0_1"],
    "pad_minus_1_visible": ["prefill-exact-4q2kv-L31-p11-x0-pad5_37", "prefill-random-4q2kv-L64-p11-x0-pad32_33", "prefill-spike-4q2kv-L129-p11-x37-pad5_37-j4_36",
                            "prefill-spike-4q2kv-L257-p0-x0-pad130_0-j129_0", "prefill-spike-4q2kv-L2-p0-x0-pad0_1-j0_0"],
    "pad_rows_not_zeroed": ["prefill-exact-4q2kv-L257-p0-x0-pad32_33", "prefill-random-4q2kv-L257-p0-x0-pad130_0", "prefill-exact-4q2kv-L257-p11-x37-pad130_0"],
    "kv_head_modulo": ["prefill-random-4q2kv-L2-p0-x0-pad0_0", "prefill-random-4q2kv-L300-p133-x37-pad0_1", "prefill-spike-4q2kv-L65-p0-x0-pad0_0-j0_0"],
    "seg_last_key_dropped": ["vis-exact-short-hd64-h1", "vis-exact-mixed-hd80-h3", "vis-exact-long257-hd80-h1", "vis-random-short-hd80-h3",
                             "vis-spike-short-hd64-h3-s3k32", "vis-spike-long300-hd80-h3-s0k299"],
    "prev_seg_last_key_visible": ["vis-exact-short-hd80-h1", "vis-exact-mixed-hd64-h3", "vis-exact-long300-hd64-h1", "vis-spike-mixed-hd64-h3-s3k96",
                                  "vis-spike-long300-hd80-h1-s0k299"],
    "last_partial_tile_dropped": ["vis-exact-short-hd64-h3", "vis-exact-mixed-hd80-h1", "vis-exact-long257-hd64-h3", "vis-random-long300-hd80-h1",
                                  "vis-spike-long257-hd80-h3-s0k256", "vis-spike-mixed-hd64-h1-s3k96"],
    "v_from_k_third": ["vis-random-short-hd64-h1", "vis-exact-mixed-hd80-h3", "vis-spike-long300-hd64-h3-s1k0"],
    "hd80_tail_unwritten": ["vis-random-short-hd80-h1", "vis-exact-mixed-hd80-h3", "vis-random-long257-hd80-h3", "vis-spike-short-hd80-h3-s5k63"],
}


def test_every_required_fault_is_modelled():
    assert set(FAULTS) == set(A.VIS_FAULTS) | set(A.PREFILL_FAULTS) and len(FAULTS) == 11
    for fault, ids in FAULTS.items():
        kernel = "vis" if fault in A.VIS_FAULTS else "prefill"
        assert len(ids) >= 3 and all(A.cases()[i]["kernel"] == kernel for i in ids), fault


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_faults_miss_the_bound(fault):
    for case_id in FAULTS[fault]:
        ok, ratio = A.compare(case_id, A.model_output(case_id))
        assert ok == [] and ratio < 1.0, (fault, case_id, ok)
        bad, ratio = A.compare(case_id, A.model_output(case_id, fault))
        assert bad and (ratio > 1.0 or fault == "pad_rows_not_zeroed"), (fault, case_id, ratio)


def test_reverting_one_mask_condition_fails_a_gpu_case():
    """The kernels' mask conditions, each moved by one, written as the fault it is: `key > qpos` -> `key > qpos + 1` (one late) or
    `key >= qpos` (one early); `key < padb` -> `key < padb - 1`; `key >= len` -> `key >= len - 1`. The exact family catches each of them
    on EVERY case where the moved edge exists, by a margin that does not depend on the data: a count changes by one."""
    for fault, needs in (("causal_one_late", lambda c: True), ("causal_one_early", lambda c: True), ("pad_minus_1_visible", lambda c: max(c["pad"]) > 0),
                         ("qpos0_ignored", lambda c: c["qpos0"] > 0)):
        for cid in A.case_ids("prefill", "exact"):
            if needs(A.cases()[cid]):
                bad, ratio = A.compare(cid, A.model_output(cid, fault))
                assert bad and ratio > 1.0, (fault, cid)
    for fault in ("seg_last_key_dropped", "prev_seg_last_key_visible", "last_partial_tile_dropped"):
        for cid in A.case_ids("vis", "exact"):
            if fault == "prev_seg_last_key_visible" and len(A.cases()[cid]["lens"]) == 1:
                continue
            bad, ratio = A.compare(cid, A.model_output(cid, fault))
            assert bad and ratio > 1.0, (fault, cid)

