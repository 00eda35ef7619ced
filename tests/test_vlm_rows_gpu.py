"""The VLM decoders' rotary + cache-append kernels, row kernels and the vision rotary kernel, each launched alone through the function
vlm_forward launches it with (fe_op_vlm_rope_cache / fe_op_vlm_rows / fe_op_vlm_vis_rope), against the float32 emulations of
tests/vlm_rows_ref.py (its docstring has the arithmetic, the variants of the four device functions and the two rules).

Every case is checked twice:
  * the exact check: a FIRM element (one whose bits do not depend on the +-K ulp variants of cosf / sinf / rsqrtf / expf) equals the
    emulation bit for bit - np.array_equal on bf16 bit patterns, e4m3 code bytes and scale bits; a FRAGILE element lies between its
    smallest and largest variant; an e4m3 row with a fragile element equals the quantisation of one of its variant rows. Every cache row
    and scale outside [start, start + L) keeps the fill pattern. At most 2% of a case's elements are fragile (asserted here from the
    reference, and for every case on the CPU by tests/test_vlm_rows_host.py).
  * the float64 guard, against a mistake in the emulation: the plain formula in float64 with a bound summed from the listed roundings.
Each test prints its fragile share and the guard's worst err / bound. Every case runs under the launch of production (max_blocks 0)
and, where the work has at least four workgroups, under a capped launch that makes three or more trips of the grid-stride loop with a
partial last one; both must give the same bits.

Cases (tests/vlm_rows_ref.py: rope_cases, rows_cases, vis_cases), the smallest shapes at which these kernels can go wrong:
  * rope, both families x (nh, nkv) = (4, 2), (7, 1), (3, 1: an odd head count) x the launch forms of vlm_forward: the staged prefill
    (max_seq == L), a prefill into a longer cache, a prefill that continues a cache (start 11), a decode step at start 37 with the start
    by value and from device memory; the e4m3 formats in the decode forms (their prefills are staged through the bf16 kernel), bf16 in all.
    Positions: three independent components below 4096, or all zero (cosf(0), sinf(0) exact: Qwen2.5 must return the input bits).
    Sections: production's and a second split per family. E4M3 edge rows: all-zero rows, one huge value among tiny ones, an Inf.
  * rows: d = 8 (one lane), 252 (ragged last trip), 256 (one trip), 260 (one trip + one lane), 1536, 3584 x rows 1, 3, 65 for rmsnorm and
    the three add_rmsnorm forms (DS: slots -1 and >= 0 mixed, one repeated), eps 1e-6 and 1e-5, padded strides, integer rows whose sums
    are exact in any order; the few-rows form at rows 1 and 64, d 512 and 4352; add; silu_mul out of place and over the gate, with
    gates below -88.73, gates >= 40, zeros, one quad and odd quad counts.
  * vision rope: hd 64 and 80 x heads 1 and 3 x rows 1 and 70, independent row / column positions, and zero positions."""
import numpy as np
import pytest

import vlm_rows_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 30)
    yield e
    e.close()


def _grids(c):
    return [0] + ([c["small_grid"]] if c["small_grid"] else [])


def run_rope(eng, case_id):
    """-> (failures, {format: fragile share}, worst err / bound of the guard)."""
    c, e = R.rope_cases()[case_id], R.rope_expect(case_id)
    (rq, rk, rv), (bq, bk) = R.guard_rope(c)
    bad, shares, w = [], {}, 0.0
    qw = dict(qn=c["qn"], kn=c["kn"], eps=c["eps"]) if c["family"] == "qwen3" else {}
    for fmt in c["formats"]:
        shares[fmt] = e.fragile_share(fmt)
        for mb in _grids(c):
            q, k, v, ks, vs = eng.vlm_rope_cache(c["qkv"], c["pos"], c["inv_freq"], c["nh"], c["nkv"], c["B"], c["L"], c["sections"], family=c["family"],
                                                 start=c["start"], start_from_device=c["start_from_device"], max_seq=c["max_seq"], kv_format=fmt, max_blocks=mb,
                                                 fill=R.FILL, **qw)
            bad += ["%s, max_blocks %d: %s" % (fmt, mb, b) for b in e.check(fmt, q, k, v, ks, vs)]
            # the guard: the rows as a reader of the cache sees them
            w = max(w, R.worst(q.reshape(rq.shape), rq, bq))
            for raw, sc, ref, bound in ((k, ks, rk, bk), (v, vs, rv, np.zeros_like(rv))):
                got = raw[e.b, :, e.p]
                if fmt == "fp8":
                    from facet_amd.weights import dequantize_e4m3_rows
                    got = dequantize_e4m3_rows(got.reshape(-1, 128), np.log2(sc[e.b, :, e.p].reshape(-1)).astype(np.int32)).reshape(ref.shape)
                else:
                    got = R.from_bits16(got)
                with np.errstate(invalid="ignore"):
                    fin = np.isfinite(ref).all(-1, keepdims=True) & np.isfinite(bound).all(-1, keepdims=True)
                    full = bound + R.TINY + (R.e4m3_step(np.where(fin, ref, 0.0)) + 2.0 ** -4 * bound if fmt != "bf16" else 0.0)
                w = max(w, R.worst(got, np.where(fin, ref, np.nan), full))
    return bad, shares, w


def run_rows(eng, case_id):
    c = R.rows_cases()[case_id]
    bad, share, w = [], 0.0, 0.0
    for mb in _grids(c):
        out = eng.vlm_rows(c["route"], np.pad(c["x"], ((0, 0), (0, c["ldx"] - c["d"]))), y=c.get("y"), w=c.get("w"), slot=c.get("slot"), ds=c.get("ds"), eps=c["eps"],
                           d=c["d"], ldy=c["ldy"], alias=c["alias"], max_blocks=mb)
        ox, on = (None, out) if c["route"] == "rmsnorm" else (out if isinstance(out, tuple) else (out, None))
        b, share = R.rows_check(case_id, ox, on)
        bad += ["max_blocks %d: %s" % (mb, t) for t in b]
        w = max(w, R.rows_guard(case_id, ox, on))
    return bad, share, w


def run_vis(eng, case_id):
    c = R.vis_cases()[case_id]
    eq, ek = R.vis_expect(case_id)
    (rq, rk), (bq, bk) = R.guard_vis_rope(c)
    bad, w = [], 0.0
    for mb in _grids(c):
        q, k = eng.vlm_vis_rope(c["qkv"], c["pos"], c["inv_freq"], c["hd"], c["heads"], max_blocks=mb)
        bad += ["max_blocks %d: %s" % (mb, t) for t in R.compare(q, eq, "q") + R.compare(k, ek, "k")]
        w = max(w, R.worst(q, rq, bq), R.worst(k, rk, bk))
    return bad, (eq.n_fragile + ek.n_fragile) / (eq.center.size + ek.center.size), w


@pytest.mark.parametrize("case_id", list(R.rope_cases()))
def test_rope_cache(eng, case_id):
    bad, shares, w = run_rope(eng, case_id)
    print("[vlm_rows] rope %s: fragile share %s, guard worst err / bound %.3f" % (case_id, ", ".join("%s %.4f" % kv for kv in shares.items()), w))
    assert max(shares.values()) <= R.FRAGILE_CAP, shares
    assert bad == [], bad[:6]
    assert w <= 1.0, w


@pytest.mark.parametrize("case_id", list(R.rows_cases()))
def test_rows(eng, case_id):
    bad, share, w = run_rows(eng, case_id)
    print("[vlm_rows] %s: fragile share %.4f, guard worst err / bound %.3f" % (case_id, share, w))
    assert share <= R.FRAGILE_CAP, share
    assert bad == [], bad[:6]
    assert w <= 1.0, w


@pytest.mark.parametrize("case_id", list(R.vis_cases()))
def test_vis_rope(eng, case_id):
    bad, share, w = run_vis(eng, case_id)
    print("[vlm_rows] vision rope %s: fragile share %.4f, guard worst err / bound %.3f" % (case_id, share, w))
    assert share <= R.FRAGILE_CAP, share
    assert bad == [], bad[:6]
    assert w <= 1.0, w


def test_launch_checks(eng):
    """What the launch functions refuse: a width that is no multiple of 4, rows past the cache, the few-rows form beyond 64 rows."""
    from facet_amd import EngineError
    c = R.rope_cases()["qwen2_5-3q1kv-cont-random-s16x24"]
    with pytest.raises(EngineError):
        eng.vlm_rope_cache(c["qkv"], c["pos"], c["inv_freq"], 3, 1, c["B"], c["L"], c["sections"], start=c["max_seq"] - c["L"] + 1, max_seq=c["max_seq"])
    x = np.ones((65, 8), np.float32)
    with pytest.raises(EngineError):
        eng.vlm_rows("few_rows_rmsnorm", x, w=np.ones(8, np.float32))
    with pytest.raises(EngineError):
        eng.vlm_rows("rmsnorm", np.ones((2, 6), np.float32), w=np.ones(6, np.float32))
