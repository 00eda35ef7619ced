"""GPU: the fused head_dim-64 attention kernels and the wiring around them, op by op against float64.

Two hooks of the C ABI are under test. `Engine.attention` (fe_op_attention) launches one kernel alone on caller q / k / v: the fp32
kernel (kernels_attn.hip), the bf16 / f16 kernel (kernels_attn_bf16.hip) or the split-f16 kernel (kernels_attn_split.hip).
`Engine.mha` (fe_op_mha) runs build_mha + mha_forward (engine.hip) with nn.MultiheadAttention's parameters. The reference is always
numpy / torch float64 on inputs ALREADY rounded to the element type (fp32 for the split form), so only the kernels' own arithmetic is
measured. d_model = 128 (two heads) and B = 2 throughout: batch, head and V^T-row offsets are all non-trivial.

Which case runs what (Lq picks the launch: 4 waves when roundup128(Lq) * 100 <= roundup64(Lq) * 108, i.e. Lq = 97, 128, 900 here):
  * 2-wave launch of the fp32 / bf16 / f16 kernels: test_shape_sweep with Lq in {1, 32, 33, 64, 65, 129, 257}
  * 4-wave launch of the same:                       test_shape_sweep with Lq in {97 (a wave with ONE valid query), 128, 900 (8 workgroups,
                                                     ragged last)}
  * split kernel (always 4 waves):                   every `split` case of test_shape_sweep / test_planted_spike / test_exact_mean
  * nt == 1 (no prefetch, one tile):                 Lk in {1, 31, 32};  nt = 2: {33, 63, 64};  nt = 3: {65, 96};  nt = 9: 257 - both
                                                     buffer parities; last tiles with 1 (Lk 1, 33, 65, 257), 31 and 32 visible keys
  * 2-byte causal branch:                            test_causal[bf16-*] / [f16-*], test_planted_spike[*-causal-*], test_exact_mean causal
  * ragged pad_store group of the V^T GEMM:          test_mha_out_of_range_isolation (Lk = 33, 37, 77 under bf16 / f16) and
                                                     test_mha_wiring cross (64, 37)
  * head_dim-32 unfused route (raw_gemm + softmax_rows_pad): test_mha_head_dim_32_unfused

Tolerances of the kernel tests (derived, not fitted). Vmax = max|v| + max|bv|, R = the largest spread of visible scores in a row
(asserted <= 24; about 8 for the random cases, about 16 with the planted spike):
  fp32    |o - ref| <= 4 (4 + R) 2^-23 Vmax      R: __expf's argument error |x| 2^-24; 4: fp32 accumulation; leading 4: margin
  bf16    4 * 2^-9  * Vmax + the fp32 term       one rounding of P and one of the output, margin 2 each
  f16     4 * 2^-12 * Vmax + the fp32 term
  split   4 * 2^-21 * Vmax + the fp32 term       2^-21: the pair precision of hi + lo
Tolerances of the wiring tests: see test_mha_wiring.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, H, HD = 2, 2, 64
D = H * HD
FORMS = ["fp32", "bf16", "f16", "split"]
UNIT = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12, "split": 2.0 ** -21}


@pytest.fixture(scope="module")
def engines():
    from facet_amd import Engine
    es = {p: Engine(0, arena_bytes=1 << 30, precision=p) for p in ("f32", "bf16", "f16")}
    yield {"fp32": es["f32"], "bf16": es["bf16"], "f16": es["f16"], "split": es["f16"]}
    for e in es.values():
        e.close()


def _round(a, form):
    """fp32 values rounded to the element type the kernel of `form` receives (the split kernel receives fp32, as a pair)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if form == "bf16":
        t = t.bfloat16().float()
    elif form == "f16":
        t = t.half().float()
    return t.numpy()


def _heads(a):
    return np.asarray(a, np.float64).reshape(a.shape[0], a.shape[1], H, HD).transpose(0, 2, 1, 3)


def _reference(q, k, v, bv, causal):
    """float64 softmax(q k^T) v + bv per (batch, head); returns (o [B, Lq, D], R)."""
    s = _heads(q) @ _heads(k).transpose(0, 1, 3, 2)                  # [B, H, Lq, Lk]
    if causal:
        i, j = np.indices(s.shape[-2:])
        s = np.where(j > i, -np.inf, s)
    hi = s.max(-1, keepdims=True)
    spread = float((hi[..., 0] - np.where(np.isinf(s), np.inf, s).min(-1)).max())
    p = np.exp(s - hi)
    p /= p.sum(-1, keepdims=True)
    o = (p @ _heads(v)).transpose(0, 2, 1, 3).reshape(q.shape[0], q.shape[1], D) + np.asarray(bv, np.float64)
    return o, spread


def _bound(form, R, vmax):
    f32 = 4.0 * (4.0 + R) * 2.0 ** -23 * vmax
    return f32 if form == "fp32" else 4.0 * UNIT[form] * vmax + f32


def _random_inputs(seed, Lq, Lk):
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 1, (B, Lq, D)) / np.sqrt(8.0)
    k = rng.normal(0, 1, (B, Lk, D)) / np.sqrt(8.0)
    v = rng.normal(0, 1, (B, Lk, D))
    bv = rng.normal(0, 0.5, D)
    return q, k, v, bv


def _spike_inputs(seed, Lq, Lk, jstar):
    """Random data plus one key every query scores a.b = 12 above its random score, with v[j*] = 50: where j* is visible the output
    is about 50, so a masked-in, masked-out or mis-indexed key moves the result by O(1) instead of O(1 / Lk). u is a unit vector per
    head; the random q and k are made orthogonal to it first, so the planted components add exactly 12 to the scores of j* and
    nothing to the others (R stays near 12 + the random spread)."""
    q, k, v, bv = _random_inputs(seed, Lq, Lk)
    rng = np.random.default_rng(seed + 1)
    u = rng.normal(0, 1, (H, HD))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for x in (q, k):
        xh = x.reshape(B, -1, H, HD)
        xh -= (xh * u).sum(-1, keepdims=True) * u
    a = b = np.sqrt(12.0)
    q += b * u.reshape(1, 1, D)
    k[:, jstar] += a * u.reshape(D)
    v[:, jstar] = 50.0
    return q, k, v, bv


_REF = {}


def _case(key, make, form, causal):
    """(rounded inputs, float64 reference, R) of one case; computed once per rounding and shared (fp32 and split share theirs)."""
    rounding = form if form in ("bf16", "f16") else "fp32"
    ck = (key, rounding, causal)
    if ck not in _REF:
        q, k, v, bv = make()
        q, k, v = _round(q, rounding), _round(k, rounding), _round(v, rounding)
        bv = np.asarray(bv, np.float32)      # the V bias stays fp32 in every form
        ref, R = _reference(q, k, v, bv, causal)
        for a in (q, k, v, bv, ref):
            a.setflags(write=False)
        _REF[ck] = (q, k, v, bv, ref, R)
    return _REF[ck]


def _check(engines, form, case, causal=False):
    q, k, v, bv, ref, R = case
    assert R <= 24.0, f"input spread {R:.1f}: the derived bound assumes R <= 24"
    got = engines[form].attention(q, k, v, bv, causal=causal, form=1 if form == "split" else 0)
    assert got.shape == ref.shape and np.isfinite(got).all()
    vmax = float(np.abs(v).max() + np.abs(bv).max())
    err, tol = float(np.abs(got - ref).max()), _bound(form, R, vmax)
    print(f"[attention {form}{' causal' if causal else ''} Lq={q.shape[1]} Lk={k.shape[1]}] worst |o - ref| {err:.3e} bound {tol:.3e} "
          f"ratio {err / tol:.3f} (R {R:.1f}, Vmax {vmax:.1f})")
    assert err <= tol, f"{form}: worst |o - ref| {err:.3e} > bound {tol:.3e} (R {R:.2f}, Vmax {vmax:.2f}) at {np.unravel_index(np.abs(got - ref).argmax(), ref.shape)}"


# (Lq, Lk): every Lq of {1, 32, 33, 64, 65, 97, 128, 129, 257, 900} and every Lk of {1, 31, 32, 33, 63, 64, 65, 96, 257} at least once,
# Lq != Lk in both directions, the models' own (257, 257)
SWEEP = [(1, 1), (1, 64), (1, 257), (32, 31), (32, 32), (33, 1), (33, 33), (64, 63), (64, 64), (64, 257), (65, 32), (65, 65), (97, 33),
         (97, 96), (128, 31), (128, 64), (128, 257), (129, 65), (129, 96), (257, 1), (257, 63), (257, 257), (900, 33), (900, 96), (900, 257)]


@pytest.mark.parametrize("shape", SWEEP, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", FORMS)
def test_shape_sweep(engines, form, shape):
    Lq, Lk = shape
    _check(engines, form, _case(("sweep", shape), lambda: _random_inputs(1000 * Lq + Lk, Lq, Lk), form, False))


@pytest.mark.parametrize("L", [1, 33, 77, 129])
@pytest.mark.parametrize("form", ["fp32", "bf16", "f16"])
def test_causal(engines, form, L):
    """Key j is visible to query i only if j <= i (the reference masks j > i). For bf16 / f16 this is the only direct execution of the
    causal branch: the CLIP text tower, its one caller in the models, is fp32."""
    _check(engines, form, _case(("causal", L), lambda: _random_inputs(7 + L, L, L), form, True), causal=True)


def _jstars(Lk):
    return [0, 31, 32, Lk - 1]


SPIKES = [(Lq, Lk, j, False) for Lq, Lk in ((65, 65), (128, 257)) for j in _jstars(Lk)] + [(65, 65, j, True) for j in _jstars(65)]


# every form on every spike; the split kernel has no causal mask (test_bad_forms_are_errors)
SPIKE_RUNS = [(f, s) for s in SPIKES for f in FORMS if not (s[3] and f == "split")]


@pytest.mark.parametrize("form,spike", SPIKE_RUNS, ids=lambda a: a if isinstance(a, str) else f"{a[0]}x{a[1]}-{'causal' if a[3] else 'full'}-j{a[2]}")
def test_planted_spike(engines, form, spike):
    """One key at j* (first of a tile, last of a tile, last key) carries softmax weight ~1 and v = 50. Same derived bounds as the
    sweep: a slipped key misses them by four orders of magnitude in fp32. Causal: queries i < j* must not see the spike."""
    Lq, Lk, jstar, causal = spike
    case = _case(("spike", Lq, Lk, jstar), lambda: _spike_inputs(31 * Lk + jstar, Lq, Lk, jstar), form, causal)
    ref = case[4]
    seen = ref[:, jstar:] if causal else ref
    assert seen.min() > 40.0 and (not causal or jstar == 0 or np.abs(ref[:, :jstar]).max() < 10.0)      # the spike decides the output
    _check(engines, form, case, causal=causal)


EXACT_RUNS = [(f, Lk, c) for c in (False, True) for Lk in (32, 64) for f in FORMS if not (c and f == "split")]


@pytest.mark.parametrize("form,Lk,causal", EXACT_RUNS, ids=lambda a: a if isinstance(a, str) else ("causal" if a is True else "full" if a is False else str(a)))
def test_exact_mean(engines, form, Lk, causal):
    """q = 0: every visible score is 0, every probability exp(0) = 1 and the output is the mean of the visible v rows. Integer v in
    [-8, 8]: the sum is exact in fp32 and sum / Lk (a power of two) is exact too and representable in bf16 / f16, so the result must
    be EQUAL - a mis-indexed or dropped key gives another rational. Causal: rows i with i + 1 a power of two (the divisor)."""
    rng = np.random.default_rng(100 + Lk)
    Lq = Lk if causal else (65 if Lk == 32 else 128)      # 2-wave and 4-wave launches
    q = np.zeros((B, Lq, D), np.float32)
    k = _round(rng.normal(0, 1, (B, Lk, D)), form)
    v = rng.integers(-8, 9, (B, Lk, D)).astype(np.float32)
    got = engines[form].attention(q, k, v, None, causal=causal, form=1 if form == "split" else 0)
    if causal:
        rows = [i for i in range(Lq) if (i + 1) & i == 0]
        want = np.stack([v[:, :i + 1].astype(np.float64).mean(1) for i in rows], 1)
        got = got[:, rows]
    else:
        want = np.broadcast_to(v.astype(np.float64).mean(1, keepdims=True), (B, Lq, D))
    assert np.array_equal(_round(want, "bf16").astype(np.float64), want), "the expected means must be representable in bf16"
    assert np.array_equal(got, want), f"{form}: {int((got != want).sum())} of {want.size} differ, worst {np.abs(got - want).max():.3e}"


def test_bad_forms_are_errors(engines):
    """The split form is f16-only and has no causal mask: both must come back as the engine's error, never reach a launch."""
    from facet_amd import EngineError
    q, k, v, bv = (np.asarray(a, np.float32) for a in _random_inputs(3, 33, 33))
    with pytest.raises(EngineError, match="no causal mask"):
        engines["f16"].attention(q, k, v, bv, causal=True, form=1)
    for p in ("fp32", "bf16"):
        with pytest.raises(EngineError, match="set f16 precision"):
            engines[p].attention(q, k, v, bv, form=1)
    assert np.isfinite(engines["f16"].attention(q, k, v, bv, form=1)).all()      # the context is still usable


# ---- the wiring: build_mha + mha_forward ------------------------------------------------------------------------------------------
def _mha_params(rng, d, form):
    w_in = _round(rng.normal(0, 1, (3 * d, d)) / np.sqrt(d), form)
    b_in = rng.normal(0, 0.2, 3 * d).astype(np.float32)
    w_out = _round(rng.normal(0, 1, (d, d)) / np.sqrt(d), form)
    b_out = rng.normal(0, 0.2, d).astype(np.float32)
    return w_in, b_in, w_out, b_out


def _mha_reference(x_q, x_kv, heads, params, res, causal):
    """float64 torch.nn.functional.multi_head_attention_forward (need_weights=False, additive causal mask) + res; [B, L, d] in / out."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    w_in, b_in, w_out, b_out = (t(a) for a in params)
    xq, xkv = t(x_q).transpose(0, 1), t(x_kv).transpose(0, 1)
    mask = None
    if causal:
        mask = torch.full((x_q.shape[1], x_kv.shape[1]), -np.inf, dtype=torch.float64).triu(1)
    y, _ = F.multi_head_attention_forward(xq, xkv, xkv, x_q.shape[2], heads, w_in, b_in, None, None, False, 0.0, w_out, b_out,
                                          training=False, need_weights=False, attn_mask=mask)
    y = y.transpose(0, 1).numpy()
    return y if res is None else y + np.asarray(res, np.float64)


def _mha_tol(form, ref):
    """4 x the per-contraction bound of the existing suites (4 = q/k projection, V projection, attention, out-projection):
    f16 2^-11 |ref| + 2e-4 max|ref| (test_f16_gpu.py, `tol = 2.0 ** -11 * np.abs(ref) + ... 2e-4 ... * np.abs(ref).max()`),
    bf16 2^-8 |ref| + 1e-3 max|ref| (test_bf16_gpu.py, `tol = 2.0 ** -8 * np.abs(ref) + 1e-3 * np.abs(ref).max()`),
    fp32 2e-4 max|ref| (test_ops_gpu.py, RTOL = 2e-4 in `_close`, applied to fe_op_conv2d)."""
    m = np.abs(ref).max()
    if form == "fp32":
        return np.full(ref.shape, 4 * 2e-4 * m)
    if form == "f16":
        return 4 * (2.0 ** -11 * np.abs(ref) + 2e-4 * m)
    return 4 * (2.0 ** -8 * np.abs(ref) + 1e-3 * m)


def _mha_check(tag, form, got, ref):
    assert got.shape == ref.shape and np.isfinite(got).all()
    excess = np.abs(got - ref) / _mha_tol(form, ref)
    print(f"[mha {form} {tag}] worst |y - ref| {np.abs(got - ref).max():.3e} (max|ref| {np.abs(ref).max():.3e}), worst err / tol {excess.max():.3f}")
    assert excess.max() <= 1.0, f"{form} {tag}: {int((excess > 1).sum())} of {ref.size} outside tolerance, worst err / tol {excess.max():.3f}, worst |y - ref| {np.abs(got - ref).max():.3e}"


MHA_CASES = [("self33", 33, 33, False), ("self129", 129, 129, False), ("cross64x37", 64, 37, False), ("causal77", 77, 77, True)]


@pytest.mark.parametrize("case", MHA_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("form", ["fp32", "bf16", "f16"])
def test_mha_wiring(engines, form, case):
    """fe_op_mha against float64 multi_head_attention_forward on the rounded inputs and weights (biases stay fp32 in the engine), with a
    residual: the projection scale fold, the V^T GEMM (ragged pad_store group at Lk = 33, 37, 77), the Lp != Lk memset, the kernel,
    the out-projection. Tolerance: _mha_tol."""
    tag, Lq, Lk, causal = case
    rng = np.random.default_rng(Lq * 1000 + Lk)
    params = _mha_params(rng, D, form)
    x_q = _round(rng.normal(0, 1, (B, Lq, D)), form)
    x_kv = x_q if Lq == Lk else _round(rng.normal(0, 1, (B, Lk, D)), form)
    res = _round(rng.normal(0, 1, (B, Lq, D)), form)
    got = engines[form].mha(x_q, x_kv, H, *params, res=res, causal=causal)
    _mha_check(tag, form, got, _mha_reference(x_q, x_kv, H, params, res, causal))


@pytest.mark.parametrize("Lk", [33, 37, 77])
@pytest.mark.parametrize("form", ["fp32", "bf16", "f16"])
def test_mha_out_of_range_isolation(engines, form, Lk):
    """Batch 1's key / value tokens are 200 x batch 0's. Batch 0's output must match the reference of batch 0 ALONE: a key row read
    across the batch boundary, or a V^T padding column holding the GEMM's out-of-range columns (Lk is no multiple of 8: under
    bf16 / f16 the last 8-column store group is ragged), would carry batch 1's magnitude into it."""
    Lq = 40
    rng = np.random.default_rng(500 + Lk)
    params = _mha_params(rng, D, form)
    x_q = _round(rng.normal(0, 1, (B, Lq, D)), form)
    x_kv = _round(rng.normal(0, 1, (B, Lk, D)) * np.array([1.0, 200.0]).reshape(B, 1, 1), form)
    res = _round(rng.normal(0, 1, (B, Lq, D)), form)
    got = engines[form].mha(x_q, x_kv, H, *params, res=res)
    assert np.isfinite(got).all()
    _mha_check(f"batch 0 alone, Lk={Lk}", form, got[:1], _mha_reference(x_q[:1], x_kv[:1], H, params, res[:1], False))


def test_mha_head_dim_32_unfused(engines):
    """d = 64 with 2 heads: head_dim 32 has no fused kernel, fp32 takes the raw_gemm + softmax_rows_pad route. Same fp32 tolerance."""
    rng = np.random.default_rng(64)
    params = _mha_params(rng, 64, "fp32")
    x_q = _round(rng.normal(0, 1, (B, 40, 64)), "fp32")
    x_kv = _round(rng.normal(0, 1, (B, 37, 64)), "fp32")
    res = _round(rng.normal(0, 1, (B, 40, 64)), "fp32")
    got = engines["fp32"].mha(x_q, x_kv, 2, *params, res=res)
    _mha_check("head_dim 32", "fp32", got, _mha_reference(x_q, x_kv, 2, params, res, False))


def test_mha_head_dim_32_unsupported_forms_are_errors(engines):
    """Causal and 2-byte attention exist only as the fused kernel: with head_dim 32 both must return the engine's error string."""
    from facet_amd import EngineError
    rng = np.random.default_rng(65)
    params = _mha_params(rng, 64, "fp32")
    x = _round(rng.normal(0, 1, (B, 33, 64)), "fp32")
    with pytest.raises(EngineError, match="causal attention needs the fused kernel"):
        engines["fp32"].mha(x, x, 2, *params, causal=True)
    for form in ("bf16", "f16"):
        with pytest.raises(EngineError, match="needs head_dim 64"):
            engines[form].mha(x, x, 2, *params)
