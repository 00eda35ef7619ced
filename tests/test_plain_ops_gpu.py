"""GPU: every pooling, resampling, row and small-GEMM kernel of kernels_misc.hip launched alone (fe_op_plane / fe_op_rowpass /
fe_op_gemm_skinny) per element type and per route of its launch function, against the float64 references of tests/plain_ops_ref.py on
inputs as rounded to the element type. The hooks do not depend on the context's precision: one fp32 engine serves every case.

Every check asserts the output shape, the values inside the view, and - bit for bit - that everything outside it (the other channels of
the output tensor, the columns past d of a row) still holds the fill value. Inputs outside the view hold a poison (3e4), so a read of a
neighbouring channel or column shows in the values.

Tolerances (derived term by term in the docstring of tests/plain_ops_ref.py; tests/test_plain_ops_host.py holds them to the project's
ceilings). Exact where the operation is: a maximum of stored values, a conversion, a sum of small integers. Otherwise
|got - ref64| <= A + ulp_E(ref64) / 2 (1 + 2^-10) elementwise, A the fp32 arithmetic bound of the operation, the second term the one store
rounding to a 2-byte type:
  bilinear          A = 8 u sum|w v| + coordinate error x steepest local slope
  adaptive avgpool  A = (window + 1) u sum|x| / window
  LayerNorm         A = |g| rstd e_mean + |y - b| (e_rstd + 3 u) + u |y|, e_mean and e_rstd from chains of ceil(d / 64) + 6 additions
  softmax           A = p u (|x - max| + E_p|x - max| + ceil(d / 64) + 17); every row sums to 1 within d u + sum A
  skinny GEMM       A = L_act ((ceil(K / 256) + 10) u sum|x w| |scale| + u |z scale| + u |v|) + the activation's own evaluation error
  layernorm_split   |hi - ref| <= A + ulp_f16(ref) / 2 (1 + 2^-10);  |hi + lo - ref| <= A + max(2^-11 ulp_f16(hi), 2^-25): lo is the f16
                    rounding of a remainder of at most ulp_f16(hi) / 2, and a remainder below 2^-14 is an f16 subnormal, spaced 2^-24
  add_rows_bcast    A = u |ref| (one fp32 addition)
Each test prints its worst err / bound per route and type before it asserts (recorded in DESIGN.md)."""
import numpy as np
import pytest

import plain_ops_ref as R

pytestmark = pytest.mark.gpu

ELEMS = ("f32", "bf16", "f16")
FILL = -7.0          # representable in every type
POISON = 3e4         # finite in f16


@pytest.fixture(scope="module")
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 30)
    yield e
    e.close()


Worst, _rng = R.Worst, R.case_rng


# ---- planes ----------------------------------------------------------------------------------------------------------------------------
def _views(c):
    """(name, ctot_in, c0_in, ctot_out, c0_out): dense; a window at a multiple of every vector in a wider tensor; at 4 elements (16 bytes in
    fp32, 8 in the 2-byte types: below maxpool3's alignment); at odd offsets with odd strides (every vector form must fall to the scalar one)."""
    c8 = (c + 7) // 8 * 8
    return [("dense", c, 0, c, 0), ("wide", 24 + c8, 16, 32 + c8, 16), ("off4", c8 + 8, 4, c8 + 16, 4), ("odd", c + 5, 1, c + 6, 3)]


def _plane(w, key, eng, route, x, elem, view, want, bound=None, **kw):
    """Runs one plane case and checks shape, view and surroundings; want [n, c, ho, wo] (bound None: exact)."""
    name, ci, c0i, co, c0o = view
    c = x.shape[1]
    got = eng.plane(route, x, elem=elem, ctot_in=ci, c0_in=c0i, ctot_out=co, c0_out=c0o, poison=POISON, fill=FILL, ho=want.shape[2], wo=want.shape[3], **kw)
    assert got.shape == (x.shape[0], co) + want.shape[2:], (got.shape, want.shape)
    inside = got[:, c0o:c0o + c]
    outside = np.delete(got, np.s_[c0o:c0o + c], axis=1)
    what = f"{route} {x.shape} {name} {kw}"
    w.exact(key, what + " outside the view", outside, np.full_like(outside, FILL))
    if bound is None:
        w.exact(key, what, inside.astype(np.float64), want)
    else:
        w.close(key, what, inside, want, bound)


def _grid(rng, shape, lo, hi):
    """Multiples of 1/32 with at most 7 significant bits: the same values in fp32, bf16 and f16, with many ties."""
    return rng.integers(lo, hi + 1, shape).astype(np.float64) / 32.0


POOLS = [(3, 2, 1, False), (2, 2, 0, True), (3, 1, 1, False)]
POOL_SIZES = [(1, 1), (2, 3), (7, 9), (15, 15), (14, 14), (37, 41)]


@pytest.mark.parametrize("elem", ELEMS)
def test_maxpool(eng, elem):
    """maxpool3_kernel<T> (k = 3, channels and strides multiples of 16 bytes, aligned base), maxpool_kernel<T, 4> and <T, 1>, by the view.
    Exact in every type. Values are ties-rich multiples of 1/32; one plane set is entirely negative (a maximum initialised with 0, or a
    padded tap read as 0, shows)."""
    w = Worst(f"maxpool {elem}")
    for k, s, p, ceil in POOLS:
        for hw in POOL_SIZES:
            for c in (4, 8, 12, 16, 3, 5):
                rng = _rng("maxpool", k, s, hw, c)
                for sign, x in (("mixed", _grid(rng, (2, c) + hw, -127, 127)), ("negative", _grid(rng, (2, c) + hw, -127, -1))):
                    if sign == "negative" and c not in (8, 5):
                        continue
                    want = R.maxpool(x, k, s, p, ceil)
                    for view in _views(c):
                        _plane(w, f"k{k}s{s}", eng, "maxpool", x, elem, view, want, k=k, stride=s, pad=p, ceil_mode=ceil)
    w.report()


def test_maxpool_f16_extremes(eng):
    """Values at and near +-65504 in f16 (pack and unpack of the 8-wide form must not lose or saturate them)."""
    w = Worst("maxpool f16 extremes")
    vals = np.array([65504.0, -65504.0, 65472.0, -65472.0, 6.1e-5, -6.1e-5, 0.0, 2.0 ** -24])
    x = R.rnd(_rng("extremes").choice(vals, (1, 8, 7, 9)), "f16")
    for k, s, p, ceil in POOLS:
        for view in _views(8):
            _plane(w, f"k{k}s{s}", eng, "maxpool", x, "f16", view, R.maxpool(x, k, s, p, ceil), k=k, stride=s, pad=p, ceil_mode=ceil)
    w.report()


def test_maxpool_second_grid_trip(eng):
    """n ho wo c / VEC above 2048 x 256 threads: the grid-stride loops of maxpool3_kernel and maxpool_kernel make a second, partial trip."""
    w = Worst("maxpool second trip")
    x = _grid(_rng("trip"), (1, 16, 371, 371), -127, 127)
    assert x.size // 4 > 2048 * 256
    want = R.maxpool(x, 3, 1, 1)
    _plane(w, "maxpool3", eng, "maxpool", x, "f32", _views(16)[0], want, k=3, stride=1, pad=1)
    _plane(w, "scalar", eng, "maxpool", x, "f32", ("odd", 17, 1, 17, 1), want, k=3, stride=1, pad=1)
    w.report()


RESIZE = [((4, 4), (8, 8)), ((8, 8), (4, 4)), ((7, 9), (10, 13)), ((1, 1), (7, 7)), ((7, 7), (1, 1)), ((5, 9), (11, 4))]
AVG = RESIZE + [((9, 8), (3, 2)), ((10, 9), (2, 1)), ((5, 5), (5, 5)), ((7, 10), (3, 4))]      # window lengths 1, 3, 4, 5, 9 and ragged ones


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("route", ["bilinear", "adaptive_avgpool"])
def test_resample(eng, route, elem):
    """bilinear_kernel / bilinear_vec4_kernel and adaptive_avgpool_kernel / adaptive_avgpool_vec4_kernel (c % 4 == 0, strides % 4 == 0 and
    an 8- / 16-byte base pick the 4-wide form), in every type and view."""
    w = Worst(f"{route} {elem}")
    fn = R.bilinear if route == "bilinear" else R.adaptive_avgpool
    for hw, out in (RESIZE if route == "bilinear" else AVG):
        for c in (1, 3, 4, 8, 12):
            x = R.rnd(_rng(route, hw, out, c).standard_normal((2, c) + hw), elem)
            ref, A = fn(x, *out)
            for view in _views(c):
                _plane(w, "vec4" if c % 4 == 0 and view[0] != "odd" else "scalar", eng, route, x, elem, view, ref, A + R.store(ref, elem))
    w.report()


@pytest.mark.parametrize("elem", ELEMS)
def test_resample_exact_integers(eng, elem):
    """Bilinear at 2x of integers 0 .. 15 is (9 a + 3 b + 3 c + d) / 16 < 256 / 16: 8 significant bits, exact in every type; a mean over 2 x 2
    or 4 x 4 windows of them (sum <= 240, a power-of-two count) too."""
    w = Worst(f"exact resample {elem}")
    for c in (4, 5):
        x = _rng("ints", c).integers(0, 16, (2, c, 8, 12)).astype(np.float64)
        for view in _views(c):
            _plane(w, "bilinear", eng, "bilinear", x, elem, view, R.bilinear(x, 16, 24)[0])
            _plane(w, "avg2", eng, "adaptive_avgpool", x, elem, view, R.adaptive_avgpool(x, 4, 6)[0])
            _plane(w, "avg4", eng, "adaptive_avgpool", x, elem, view, R.adaptive_avgpool(x, 2, 3)[0])
    w.report()


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
def _padded(x, ld, pad_value):
    out = np.full((x.shape[0], ld), pad_value, np.float64)
    out[:, :x.shape[1]] = x
    return out


def _rows_check(w, key, what, got, d, want, bound, fill=FILL):
    assert got.shape[0] == want.shape[0] and got.shape[1] >= d, (got.shape, want.shape)
    w.exact(key, what + " columns past d", got[:, d:], np.full_like(got[:, d:], fill))
    if bound is None:
        w.exact(key, what, got[:, :d].astype(np.float64), want)
    else:
        w.close(key, what, got[:, :d], want, bound)


def _ln_rows(rng, rows, d):
    """Row kinds: unit normal; 1000 + N(0, 1) (a one-pass variance cancels); constant; one outlier of 1e4."""
    x = rng.standard_normal((rows, d))
    kinds = {1: [0], 3: [1, 2, 3], 5: [0, 1, 2, 3, 0]}.get(rows, [0, 1, 2, 3])
    for r in range(rows):
        kind = kinds[r % len(kinds)]
        if kind == 1:
            x[r] += 1000.0
        elif kind == 2:
            x[r] = 0.375
        elif kind == 3:
            x[r, (7 * r + d // 2) % d] = 1e4
    return x


LN_PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("f32", "bf16"), ("f32", "f16")]
LN_GENERIC, LN_REG, LN_WIDE = (1, 63, 64, 65, 255), (256, 512, 768, 1024), (1152, 1280, 4608)


@pytest.mark.parametrize("pair", LN_PAIRS, ids="-".join)
def test_layernorm(eng, pair):
    """layernorm_reg_kernel<.., 1 | 2 | 3 | 4> (d = 256 .. 1024, everything aligned) and layernorm_kernel (any other d, or a stride, a base or
    g / b that is not aligned: forced here for each register width, and the result must agree with the register kernel's), rows 1, 3, 5
    and 8200 (more rows than the 8192 waves of a capped grid) x eps 1e-5, 1e-6. Input columns past d hold the poison."""
    ti, to = pair
    w = Worst(f"layernorm {ti}->{to}")

    def run(x, g, b, eps, d, key, **kw):
        ldx = kw.pop("ldx", d)
        ref, A = R.layernorm(x, g, b, eps)
        got = eng.rowpass("layernorm", _padded(x, ldx, POISON), d=d, elem_in=ti, elem_out=to, g=g, b=b, eps=eps, fill=FILL, **kw)
        bound = A + R.store(ref, to)
        _rows_check(w, key, f"d {d} rows {x.shape[0]} eps {eps} {kw}", got, d, ref, bound)
        return got[:, :d].astype(np.float64), bound

    for d in LN_GENERIC + LN_REG + LN_WIDE:
        rng = _rng("ln", d)
        g, b = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)
        key = "reg" if d in LN_REG else "generic"
        for eps in (1e-5, 1e-6):
            for rows in (1, 3, 5):
                x = R.rnd(_ln_rows(rng, rows, d), ti)
                run(x, g, b, eps, d, key, ldy=d + 4 if rows == 3 else d)
        if d in LN_REG:
            x = R.rnd(_ln_rows(rng, 5, d), ti)
            base, bound = run(x, g, b, 1e-5, d, "reg")
            for form in (dict(ldx=d + 2), dict(off_x=1, off_y=0), dict(off_gb=1)):
                other, _ = run(x, g, b, 1e-5, d, "forced generic", **form)
                w.close("reg vs generic", f"d {d} {form}", other, base, bound if to == "f32" else 2 * bound)      # (two roundings of one value may be neighbours)
        if d == 256:
            x = R.rnd(_ln_rows(rng, 8200, d), ti)
            run(x, g, b, 1e-5, d, "reg")
            run(x, g, b, 1e-5, d, "forced generic", off_gb=1)
    w.report()


def test_layernorm_f16_saturates(eng):
    """f32 -> f16 with g = 1e5: results past the f16 range come out as exactly +-65504, never Inf (stf(f16*) clamps), in both kernels."""
    rng = _rng("sat")
    x = rng.standard_normal((3, 256))
    g, b = np.full(256, 1e5, np.float32), np.zeros(256, np.float32)
    ref, _ = R.layernorm(R.rnd(x, "f32"), g, b, 1e-5)
    big = np.abs(ref) > 65504 * 1.01
    assert big.sum() > 100
    for kw in (dict(), dict(off_gb=1)):
        got = eng.rowpass("layernorm", x, elem_in="f32", elem_out="f16", g=g, b=b, eps=1e-5, **kw)
        assert np.isfinite(got).all() and np.array_equal(got[big], np.sign(ref[big]) * 65504.0)


def test_layernorm_split_and_split_hi_lo(eng):
    """layernorm_split_kernel<1 .. 4> (fp32 row -> f16 hi | lo) and split_hi_lo_kernel."""
    w = Worst("split")
    for d in LN_REG:
        rng = _rng("split", d)
        g, b = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)
        x = R.rnd(_ln_rows(rng, 5, d), "f32")
        ref, A = R.layernorm(x, g, b, 1e-5)
        for ldy in (2 * d, 2 * d + 8):
            got = eng.rowpass("layernorm_split", x, elem_in="f32", elem_out="f16", g=g, b=b, eps=1e-5, ldy=ldy, fill=FILL).astype(np.float64)
            assert got.shape == (5, ldy)
            w.exact("layernorm_split", f"d {d} ldy {ldy} columns past 2 d", got[:, 2 * d:], np.full((5, ldy - 2 * d), FILL))
            hi, lo = got[:, :d], got[:, d:2 * d]
            w.close("layernorm_split hi", f"d {d}", hi, ref, A + R.store(ref, "f16"))
            w.close("layernorm_split hi + lo", f"d {d}", hi + lo, ref, A + np.maximum(2.0 ** -11 * R.ulp(hi, "f16"), 2.0 ** -25))
        # split_hi_lo: both halves exactly, from the input (x - hi is exact in fp32)
        x = R.rnd(rng.standard_normal((7, d)) * 10.0 ** rng.integers(-6, 5, (7, d)), "f32")
        x[0, :4] = [0.0, 65504.0, 1e5, -1e5]
        got = eng.rowpass("split_hi_lo", x, elem_in="f32", elem_out="f16").astype(np.float64)
        hi, lo = R.split_pair(x)
        w.exact("split_hi_lo", f"d {d} hi", got[:, :d], hi)
        w.exact("split_hi_lo", f"d {d} lo", got[:, d:], lo)
    w.report()


@pytest.mark.parametrize("elem", ELEMS)
def test_add_rows_bcast(eng, elem):
    """add_rows_bcast_kernel<T>: row r += pos[r % L], rows = 3 L + 1, in place on strided rows."""
    w = Worst(f"add_rows_bcast {elem}")
    for d, L in ((5, 4), (64, 3), (260, 2)):
        rng = _rng("bcast", d)
        rows = 3 * L + 1
        x, pos = R.rnd(rng.standard_normal((rows, d)), elem), R.rnd(rng.standard_normal((L, d)), "f32")
        ref = x + pos[np.arange(rows) % L]
        for ld, off in ((d, 0), (d + 3, 1)):
            got = eng.rowpass("add_rows_bcast", _padded(x, ld, FILL), d=d, elem_in=elem, g=pos, off_x=off, off_gb=off)
            _rows_check(w, "add", f"d {d} ld {ld}", got, d, ref, R.U * np.abs(ref) + R.store(ref, elem))
    w.report()


def test_convert(eng):
    """convert_kernel in its four directions: exact roundings (ties to even, f16 saturating), exact widenings."""
    w = Worst("convert")
    rng = _rng("convert")
    x = rng.standard_normal((9, 130)) * 10.0 ** rng.integers(-5, 5, (9, 130))
    x[0, :8] = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0, 7e4, -7e4, 0.0]
    for e in ("bf16", "f16"):
        w.exact(f"f32->{e}", "", eng.rowpass("convert", x, elem_in="f32", elem_out=e).astype(np.float64), R.rnd(x, e))
        w.exact(f"{e}->f32", "", eng.rowpass("convert", x, elem_in=e, elem_out="f32").astype(np.float64), R.rnd(x, e))
    w.report()


def _sm_rows(rng, rows, d):
    """Row kinds: normal; all equal; one value 80 above the rest; all at -1e4; wide normal."""
    x = rng.standard_normal((rows, d))
    for r in range(rows):
        kind = (r + (0 if rows > 1 else 0)) % 5
        if kind == 1:
            x[r] = 0.25
        elif kind == 2:
            x[r, (3 * r + d // 2) % d] += 80.0
        elif kind == 3:
            x[r] = -1e4
        elif kind == 4:
            x[r] *= 3.0
    return R.rnd(x, "f32")


def _softmax_case(w, eng, route, key, rows, d, ld, off=0):
    x = _sm_rows(_rng(route, rows, d, ld), rows, d)
    ref, A = R.softmax(x)
    got = eng.rowpass(route, _padded(x, ld, FILL), d=d, off_x=off)
    what = f"{route} rows {rows} d {d} ld {ld} off {off}"
    _rows_check(w, key, what, got, d, ref, A, fill=0.0 if route == "softmax_rows_pad" else FILL)
    w.close(key + " row sums", what, got[:, :d].astype(np.float64).sum(axis=1), np.ones(rows), d * R.U + A.sum(axis=1))


def test_softmax_rows(eng):
    """softmax_rows_kernel: columns >= d keep what they held."""
    w = Worst("softmax_rows")
    for d in (1, 5, 64, 65, 1000):
        for ld in (d, d + 3):
            for rows in (1, 5):
                _softmax_case(w, eng, "softmax_rows", "generic", rows, d, ld)
    w.report()


def test_softmax_rows_pad(eng):
    """launch_softmax_rows_pad: softmax_rows_pad_reg_kernel<2> (ld <= 512), <8> (ld <= 2048) and the scalar kernel (longer, ld % 4 != 0, or
    a base that is not 16-byte aligned); columns d .. ld - 1 must come out exactly 0 (the V^T GEMM reads them)."""
    w = Worst("softmax_rows_pad")
    for key, shapes in (("reg2", [(4, 1), (8, 5), (32, 17), (512, 512), (512, 481)]), ("reg8", [(516, 513), (2048, 2047)]), ("scalar", [(2052, 2049), (30, 29)])):
        for ld, d in shapes:
            for rows in (1, 5):
                _softmax_case(w, eng, "softmax_rows_pad", key, rows, d, ld)
    _softmax_case(w, eng, "softmax_rows_pad", "scalar", 5, 17, 32, off=1)
    _softmax_case(w, eng, "softmax_rows_pad", "scalar", 5, 513, 516, off=1)
    _softmax_case(w, eng, "softmax_rows_pad", "reg2", 8200, 17, 32)
    w.report()


def test_uninstantiated_types_are_errors(eng):
    """Only the instantiated pairs and triples are accepted: anything else is an error of the hook, never another kernel."""
    from facet_amd import EngineError
    x, g = np.zeros((2, 256), np.float32), np.ones(256, np.float32)
    with pytest.raises(EngineError, match="no LayerNorm"):
        eng.rowpass("layernorm", x, elem_in="bf16", elem_out="f32", g=g, b=g)
    with pytest.raises(EngineError, match="no conversion"):
        eng.rowpass("convert", x, elem_in="bf16", elem_out="f16")
    with pytest.raises(EngineError, match="fp32"):
        eng.rowpass("softmax_rows", x, elem_in="f16")
    with pytest.raises(EngineError, match="no kernel"):
        eng.gemm_skinny(x, x, 256, types=("f32", "f32", "bf16"))


# ---- skinny GEMM -------------------------------------------------------------------------------------------------------------------------
TRIPLES = [("f32", "f32", "f32"), ("bf16", "bf16", "bf16"), ("bf16", "bf16", "f32"), ("f16", "f16", "f16"), ("f16", "f16", "f32"), ("f32", "bf16", "f32"),
           ("f32", "f16", "f32")]
ACTS = [None, "relu", "gelu", "sigmoid", "softplus", "quickgelu"]


@pytest.mark.parametrize("types", TRIPLES, ids="-".join)
def test_gemm_skinny(eng, types):
    """gemm_skinny_kernel<8 | 32, TI, TW, TO>: M on both sides of the MR split (8 / 9), K below, at and above one 256-wide trip of a wave,
    ragged last blocks of 4 columns, padded strides everywhere, scale / shift present and absent, every activation of fe_apply_act."""
    ti, tw, to = types
    w = Worst("gemm_skinny " + "-".join(types))
    i = 0
    for M in (1, 8, 9, 32):
        for K in (4, 252, 256, 260, 1028):
            for N in (1, 5, 67):
                rng = _rng("gemm", M, K, N)
                x, wt = R.rnd(rng.standard_normal((M, K + 4)), ti), R.rnd(rng.standard_normal((N, K + 8)) / np.sqrt(K), tw)
                x[:, K:], wt[:, K:] = POISON, POISON
                act, affine = ACTS[i % 6], (i // 6) % 2 == 0
                i += 1
                sc, sh = (rng.uniform(0.5, 1.5, N).astype(np.float32), rng.standard_normal(N).astype(np.float32)) if affine else (None, None)
                z, mag, chain = R.gemm(x, wt, K)
                ref, A = R.epilogue(z, mag, chain, sc, sh, act)
                got = eng.gemm_skinny(x, wt, K, types=types, scale=sc, shift=sh, act=act, ldy=N + 3, fill=FILL)
                _rows_check(w, f"MR{8 if M <= 8 else 32}", f"M {M} K {K} N {N} act {act} affine {affine}", got, N, ref, A + R.store(ref, to))
    # integers: |sum| <= 252 is exact in fp32 and in both 2-byte output types
    rng = _rng("gemm ints")
    x, wt = rng.integers(-1, 2, (9, 252)).astype(np.float64), rng.integers(-1, 2, (5, 252)).astype(np.float64)
    got = eng.gemm_skinny(x, wt, 252, types=types, ldy=8, fill=FILL)
    _rows_check(w, "integers", "M 9 K 252 N 5", got, 5, x @ wt.T, None)
    w.report()
