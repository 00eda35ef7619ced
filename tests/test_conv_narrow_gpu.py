"""GPU: the narrow-output convolutions (Cout <= 4) through Engine.conv2d, per route, against the float64 convolution of
tests/plain_ops_ref.py on operands as rounded to the context's element type.

Routes (launch_conv in kernels_conv.hip, conv_forward in engine.hip):
  fp32 narrow    conv_narrow_kernel<1> (Cout 1) and <4> (Cout 2 .. 4): any 1 x 1 with Cout <= 4, and Cout <= 4 with Cin % 16 != 0. The <4>
                 form keeps four accumulators whatever Cout is; those past Cout read the last weight row again (the packed weights hold
                 exactly Cout rows), which the Cin = 1024 case runs with a long row.
  fp32 taps      Cout <= 2, 3 x 3, Cin % 16 == 0, stride 1, no residual: a 1 x 1 convolution to KH KW Cout per-tap partial sums on the
                 matrix cores, then tap_gather_kernel<float> adds the neighbours' partials.
  2-byte taps    the same in bf16 / f16 (tap_gather_kernel<E>): every partial sum is ROUNDED to the element type before the sum, which no
                 other convolution route does.
  2-byte control Cout <= 2 with stride 2 or a residual: the ordinary 2-byte kernel, held to the contraction tolerance of
                 tests/test_bf16_gpu.py / tests/test_f16_gpu.py.

Tolerance of every route but the control: |got - ref64| <= A + ulp_E(ref64) / 2 (1 + 2^-10), with
  A = L_act ((chain + 6) u sum|x w| |scale| + u |z scale| + u |v|) + the activation's evaluation error (+ u |v| per residual sum),
  chain = KH KW ceil(Cin / 64) + 8 for the narrow kernel (a lane's serial accumulations, the 4-term dot product, 4 shuffle steps),
  chain = Cin + KH KW for the tap routes (the matrix cores' K chain, then the gather's sum),
and for the 2-byte tap route  + L_act |scale| sum_taps ulp_E(z_t) / 2 (1 + 2^-10)  for the roundings of the per-tap partials z_t.
Each test prints its worst err / bound per route before it asserts (recorded in DESIGN.md)."""
import numpy as np
import pytest

import plain_ops_ref as R

pytestmark = pytest.mark.gpu

Worst, _rng = R.Worst, R.case_rng

ACTS = [None, "relu", "gelu", "sigmoid", "softplus", "quickgelu"]


def _engine(precision):
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 30, precision=precision)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng32():
    yield from _engine("f32")


@pytest.fixture(scope="module")
def eng_bf16():
    yield from _engine("bf16")


@pytest.fixture(scope="module")
def eng_f16():
    yield from _engine("f16")


def _case(eng, elem, n, cin, hw, cout, k, stride, dil, act, affine=True, res=None, tap_rounding=False, chain=None, integers=0):
    """-> (got, ref, bound): one convolution on the engine and its float64 reference. res: None, "before" or "after" the activation."""
    rng = _rng(elem, n, cin, hw, cout, k, stride, dil, act, res)
    pad = dil * (k // 2)
    if integers:
        x = rng.integers(-integers, integers + 1, (n, cin) + hw).astype(np.float64)
        w = rng.integers(-integers, integers + 1, (cout, cin, k, k)).astype(np.float64)
    else:
        x, w = R.rnd(rng.standard_normal((n, cin) + hw), elem), R.rnd(rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k), elem)
    z, mag, taps = R.conv2d(x, w, stride, pad, dil)
    sc, sh = (rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.2, cout).astype(np.float32)) if affine else (None, None)
    r = None if res is None else R.rnd(rng.standard_normal(z.shape), elem)
    bc = lambda v: None if v is None else v.astype(np.float64).reshape(1, -1, 1, 1)
    ref, A = R.epilogue(z, mag, chain, bc(sc), bc(sh), act, r, res == "after")
    if tap_rounding:
        A = A + R.LIPSCHITZ[act] * (1.0 if sc is None else np.abs(bc(sc))) * R.store(taps, elem).sum(axis=0)
    got = eng.conv2d(x, w, scale=sc, shift=sh, res=r, res_after_act=res == "after", stride=stride, pad=pad, dil=dil, act=act)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return got, ref, A + R.store(ref, elem)


def test_fp32_narrow_kernel(eng32):
    """conv_narrow_kernel<4> at Cout 2, 3, 4 (and <1> beside it): 1 x 1 with Cin 8, 64 and 1024 (rows of 4 KiB: the accumulators past
    Cout must not read behind the last one), 3 x 3 with Cin % 16 != 0 at stride 2, dilation 2, M % 4 != 0, residual before and after the
    activation, every activation."""
    w = Worst("fp32 narrow conv")
    i = 0
    for cout in (1, 2, 3, 4):
        for cin in (8, 64, 1024):
            for hw in ((5, 7), (1, 1)):
                got, ref, bound = _case(eng32, "f32", 2 if hw == (5, 7) else 3, cin, hw, cout, 1, 1, 1, ACTS[i % 6], affine=i % 2 == 0, chain=-(-cin // 64) + 8)
                w.close(f"1x1 CO{1 if cout == 1 else 4}", f"cout {cout} cin {cin} {hw}", got, ref, bound)
                i += 1
    for cout in (1, 2, 3):
        for cin in (24, 40):
            for stride, dil, hw in ((1, 1, (7, 9)), (2, 1, (9, 11)), (1, 2, (5, 7)), (2, 2, (11, 6))):
                for res in (None, "before", "after"):
                    got, ref, bound = _case(eng32, "f32", 1, cin, hw, cout, 3, stride, dil, ACTS[i % 6], affine=i % 3 != 0, res=res, chain=9 * -(-cin // 64) + 8)
                    w.close(f"3x3 CO{1 if cout == 1 else 4}", f"cout {cout} cin {cin} {hw} s{stride} d{dil} res {res} act {ACTS[i % 6]}", got, ref, bound)
                    i += 1
    # integers: exact in any order
    for cout, cin, k in ((3, 24, 3), (2, 8, 1), (4, 1024, 1)):
        got, ref, _ = _case(eng32, "f32", 2, cin, (6, 5), cout, k, 1, 1, None, affine=False, chain=1, integers=3)
        w.exact("integers", f"cout {cout} cin {cin} k {k}", got.astype(np.float64), ref)
    w.report()


def test_fp32_tap_route(eng32):
    """Cout 1, 2 x Cin 16, 64, 3 x 3 with dilation 1 and 2 on odd sizes: per-tap partials + tap_gather_kernel<float>."""
    w = Worst("fp32 tap route")
    i = 0
    for cout in (1, 2):
        for cin in (16, 64):
            for dil in (1, 2):
                for hw in ((7, 9), (13, 5)):
                    got, ref, bound = _case(eng32, "f32", 2, cin, hw, cout, 3, 1, dil, ACTS[i % 6], affine=i % 2 == 0, chain=cin + 9)
                    w.close("taps", f"cout {cout} cin {cin} {hw} d{dil} act {ACTS[i % 6]}", got, ref, bound)
                    i += 1
    got, ref, _ = _case(eng32, "f32", 2, 16, (6, 5), 2, 3, 1, 1, None, affine=False, chain=1, integers=3)
    w.exact("integers", "cout 2 cin 16", got.astype(np.float64), ref)
    w.report()


@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_two_byte_tap_route(elem, request):
    """Cout 1, 2 x Cin 16, 32, 64, 3 x 3 with dilation 1 and 2, act none / relu / sigmoid: the 2-byte 1 x 1 convolution to per-tap partials
    rounded to the element type + tap_gather_kernel<E>, with the partials' roundings in the bound."""
    eng = request.getfixturevalue("eng_" + elem)
    w = Worst(f"{elem} tap route")
    i = 0
    for cout in (1, 2):
        for cin in (16, 32, 64):
            for dil in (1, 2):
                for act in (None, "relu", "sigmoid"):
                    got, ref, bound = _case(eng, elem, 2, cin, (7, 9) if i % 2 else (12, 5), cout, 3, 1, dil, act, affine=i % 2 == 0, tap_rounding=True, chain=cin + 9)
                    w.close("taps", f"cout {cout} cin {cin} d{dil} act {act}", got, ref, bound)
                    i += 1
    got, ref, _ = _case(eng, elem, 2, 16, (6, 5), 2, 3, 1, 1, None, affine=False, chain=1, integers=1)
    w.exact("integers", "cout 2 cin 16", got.astype(np.float64), ref)
    w.report()


@pytest.mark.parametrize("elem", ["bf16", "f16"])
def test_two_byte_control(elem, request):
    """Cout 1, 2 with stride 2 or a residual do not take the tap route (engine.hip): the ordinary 2-byte kernel, at the tolerance the
    2-byte contractions already have (exact products, fp32 sums, one rounding of the result)."""
    eng = request.getfixturevalue("eng_" + elem)
    rel, floor = (2.0 ** -8, 1e-3) if elem == "bf16" else (2.0 ** -11, 2e-4)
    worst, fails = 0.0, []
    for cout in (1, 2):
        for cin in (16, 64):
            for stride, res in ((2, None), (1, "before"), (2, "after")):
                for act in (None, "relu"):
                    got, ref, _ = _case(eng, elem, 2, cin, (9, 11), cout, 3, stride, 1, act, res=res, chain=1)
                    ratio = float((np.abs(got - ref) / (rel * np.abs(ref) + floor * np.abs(ref).max())).max())
                    worst = max(worst, ratio)
                    if not ratio <= 1.0:
                        fails.append((cout, cin, stride, res, act, ratio))
    got, ref, _ = _case(eng, elem, 2, 16, (6, 5), 2, 3, 2, 1, None, affine=False, chain=1, integers=1)
    print(f"\n{elem} control: worst err / tolerance {worst:.3f}")
    assert np.array_equal(got, ref) and not fails, fails
