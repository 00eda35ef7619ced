"""GPU: the two kernels of the Qwen-VL attention tile (facet_amd/csrc/vlm_attn_tile.h), each launched alone through the one function that
launches it - vlm_vis_attn_kernel<HD, NW> by fe_op_vlm_vis_attention / vlm_vis_attention, vlm_attn_prefill_kernel by
fe_op_vlm_prefill_attention / vlm_prefill_attention - against the float64 reference of tests/vlm_attn_ref.py on inputs already rounded to
bf16. Its docstring has the three input families (random, planted spike, exact count), the derivation of the bounds and the case list with
the branch each shape takes; tests/test_vlm_attn_host.py shows on the CPU that every case meets what its bound assumes and that a
modelled fault of each mask condition misses the bound.

  random, spike   |o - ref| <= 4 * 2^-9 * Vmax + 4 (4 + R + S) * 2^-23 * Vmax, R and S <= 24
  exact           |o - ref| <= 2^-8 |ref|, zeros exactly zero
  always          no NaN (the cache rows behind the keys are NaN), no 768 (the outputs' fill), prefill pad rows exactly 0.0

One launch per case; every test prints its worst err / bound."""
import numpy as np
import pytest

import vlm_attn_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 30)
    yield e
    e.close()


def run(eng, case_id):
    c, x = A.cases()[case_id], A.inputs(case_id)
    if c["kernel"] == "vis":
        return eng.vlm_vis_attention(x["q"], x["k"], x["v"], x["cu"], c["hd"], c["heads"])
    return eng.vlm_prefill_attention(x["q"], x["k"], x["v"], c["nh"], c["nkv"], qpos0=c["qpos0"], max_seq=c["max_seq"], pad=x["pad"])


def check(eng, case_id):
    assert A.premises(case_id) == []
    _, R, S, vmax = A.expect(case_id)
    bad, ratio = A.compare(case_id, run(eng, case_id))
    print("[vlm_attn] %s: worst err / bound %.3f (R %.1f, S %.1f, Vmax %.1f)" % (case_id, ratio, R, S, vmax))
    assert bad == [], bad
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("case_id", A.case_ids("vis", "random"))
def test_vis_random(eng, case_id):
    check(eng, case_id)


@pytest.mark.parametrize("case_id", A.case_ids("vis", "spike"))
def test_vis_spike(eng, case_id):
    check(eng, case_id)


@pytest.mark.parametrize("case_id", A.case_ids("vis", "exact"))
def test_vis_exact_count(eng, case_id):
    check(eng, case_id)


@pytest.mark.parametrize("case_id", A.case_ids("prefill", "random"))
def test_prefill_random(eng, case_id):
    check(eng, case_id)


@pytest.mark.parametrize("case_id", A.case_ids("prefill", "spike"))
def test_prefill_spike(eng, case_id):
    check(eng, case_id)


@pytest.mark.parametrize("case_id", A.case_ids("prefill", "exact"))
def test_prefill_exact_count(eng, case_id):
    check(eng, case_id)


def test_argument_checks(eng):
    """What the hooks refuse before any launch - a head size the kernel is not built for, a segment list that does not describe the rows,
    a group that does not divide, a cache shorter than the keys, padding that leaves no key - and the context stays usable."""
    from facet_amd import EngineError
    cid = "vis-random-short-hd64-h1"
    x = A.inputs(cid)
    wide = np.zeros((x["q"].shape[0], 72), np.float32)
    with pytest.raises(EngineError):
        eng.vlm_vis_attention(wide, wide, wide, x["cu"], 72, 1)
    with pytest.raises(EngineError):
        eng.vlm_vis_attention(x["q"], x["k"], x["v"], x["cu"], 64, 1, max_seg=63)
    with pytest.raises(EngineError):
        eng.vlm_vis_attention(x["q"], x["k"], x["v"], x["cu"], 64, 1, max_seg=128)
    cu = x["cu"].copy()
    cu[3] = cu[2]          # an empty segment
    with pytest.raises(EngineError):
        eng.vlm_vis_attention(x["q"], x["k"], x["v"], cu, 64, 1, max_seg=64)
    cu = x["cu"].copy()
    cu[0] = 1
    with pytest.raises(EngineError):
        eng.vlm_vis_attention(x["q"], x["k"], x["v"], cu, 64, 1, max_seg=64)
    pid = "prefill-random-4q2kv-L33-p11-x37-pad5_37"
    c, p = A.cases()[pid], A.inputs(pid)
    Lk = c["qpos0"] + c["Lq"]
    with pytest.raises(EngineError):
        eng.vlm_prefill_attention(p["q"], p["k"], p["v"], 4, 2, qpos0=11, max_seq=Lk - 1, pad=p["pad"])
    with pytest.raises(EngineError):
        eng.vlm_prefill_attention(p["q"], p["k"], p["v"], 4, 2, qpos0=11, max_seq=8193, pad=p["pad"])
    with pytest.raises(EngineError):
        eng.vlm_prefill_attention(p["q"], p["k"], p["v"], 4, 2, qpos0=11, pad=[0, Lk])
    with pytest.raises(EngineError):
        eng.vlm_prefill_attention(p["q"], p["k"], p["v"], 4, 2, qpos0=11, pad=[-1, 0])
    with pytest.raises(EngineError):
        eng.vlm_prefill_attention(p["q"], np.concatenate([p["k"], p["k"][:, :1]], 1), np.concatenate([p["v"], p["v"][:, :1]], 1), 4, 3, qpos0=11, pad=p["pad"])
    for case_id in (cid, pid):          # the context is still usable
        bad, ratio = A.compare(case_id, run(eng, case_id))
        assert bad == [] and ratio <= 1.0
