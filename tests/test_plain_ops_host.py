"""CPU: the float64 references of tests/plain_ops_ref.py are the operations torch.nn.functional defines (pinned here in float64 on
shapes with odd sizes, ragged windows and every pooling mode the models use), and their error bounds are finite, positive and - on
well-conditioned data - no looser than what the project already grants the same operations: 1e-5 max|ref| for LayerNorm, bilinear and
the average pool, 2e-4 max|ref| for contractions (tests/test_ops_gpu.py). For a 2-byte output the fp32 arithmetic bound A must stay
below a tenth of the store's rounding term; A is absolute (it does not shrink with an element that happens to be near zero), so it is
compared with the rounding term at the scale of the output, ulp_E(max|ref|) / 2."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plain_ops_ref as R

T64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))


def _x(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape)


POOLS = [(k, s, p, ceil, hw) for k, s, p, ceil in [(3, 2, 1, False), (2, 2, 0, True), (3, 1, 1, False), (3, 2, 0, True)]
         for hw in [(1, 1), (2, 3), (7, 9), (15, 15), (14, 14), (37, 41)] if min(hw) + 2 * p >= k]      # (torch rejects a window larger than the padded input)


@pytest.mark.parametrize("k,s,p,ceil,hw", POOLS)
def test_maxpool_is_torch(k, s, p, ceil, hw):
    x = _x((2, 3) + hw) - 5.0      # all negative: padding must not win
    want = F.max_pool2d(T64(x), k, s, p, ceil_mode=ceil).numpy()
    got = R.maxpool(x, k, s, p, ceil)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("hw,out", [((4, 4), (8, 8)), ((8, 8), (4, 4)), ((7, 9), (10, 13)), ((1, 1), (7, 7)), ((7, 7), (1, 1)), ((5, 9), (11, 4)),
                                    ((16, 12), (5, 7))])
def test_bilinear_is_torch(hw, out):
    x = _x((2, 3) + hw, 1)
    want = F.interpolate(T64(x), size=out, mode="bilinear", align_corners=False).numpy()
    got, A = R.bilinear(x, *out)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    assert np.isfinite(A).all() and (A > 0).all()
    assert A.max() <= 1e-5 * np.abs(got).max()
    for e in ("bf16", "f16"):
        ref, A = R.bilinear(R.rnd(x, e), *out)
        assert A.max() <= 0.1 * float(R.ulp(np.abs(ref).max(), e)) / 2


@pytest.mark.parametrize("hw,out", [((9, 8), (3, 2)), ((10, 9), (2, 1)), ((5, 5), (5, 5)), ((7, 10), (3, 4)), ((7, 7), (8, 8)), ((10, 6), (1, 1))])
def test_adaptive_avgpool_is_torch(hw, out):
    x = _x((2, 3) + hw, 2) + 2.0      # (a mean of values that cancel is ill-conditioned: the ceiling is for data that does not)
    want = F.adaptive_avg_pool2d(T64(x), out).numpy()
    got, A = R.adaptive_avgpool(x, *out)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14
    assert np.isfinite(A).all() and (A > 0).all()
    assert A.max() <= 1e-5 * np.abs(got).max()
    for e in ("bf16", "f16"):
        ref, A = R.adaptive_avgpool(R.rnd(x, e), *out)
        assert A.max() <= 0.1 * float(R.ulp(np.abs(ref).max(), e)) / 2


def test_adaptive_windows_by_definition():
    assert R.adaptive_windows(10, 4) == [(0, 3), (2, 5), (5, 8), (7, 10)]
    assert R.adaptive_windows(7, 8)[3] == (2, 4) and R.adaptive_windows(9, 1) == [(0, 9)]


@pytest.mark.parametrize("d", [1, 63, 64, 65, 255, 256, 512, 768, 1024, 1152, 1280, 4608])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_layernorm_is_torch(d, eps):
    rng = np.random.default_rng(d)
    x = rng.standard_normal((5, d))
    x[1] += 1000.0
    x[2] = 0.375
    x[3, d // 2] = 1e4
    g, b = 1 + 0.1 * rng.standard_normal(d), 0.1 * rng.standard_normal(d)
    want = F.layer_norm(T64(x), (d,), T64(g), T64(b), eps).numpy()
    got, A = R.layernorm(x, g, b, eps)
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    assert np.isfinite(A).all() and (A > 0).all()
    if d >= 63:      # the well-conditioned rows: unit normal, g near 1
        for rows in ([0], [4]):
            assert A[rows].max() <= 1e-5 * np.abs(got[rows]).max(), (A[rows].max(), np.abs(got[rows]).max())
            for e in ("bf16", "f16"):
                assert A[rows].max() <= 0.1 * float(R.ulp(np.abs(got[rows]).max(), e)) / 2


@pytest.mark.parametrize("d", [1, 5, 17, 64, 65, 481, 1000, 2047, 2049])
def test_softmax_is_torch(d):
    rng = np.random.default_rng(d)
    x = rng.standard_normal((5, d))
    x[1] = 0.25
    x[2, d // 2] += 80.0
    x[3] = -1e4
    x[4] *= 3.0
    want = F.softmax(T64(x), dim=1).numpy()
    got, A = R.softmax(x)
    assert np.abs(got - want).max() <= 1e-15
    assert np.isfinite(A).all() and (A > 0).all()
    assert (A <= 1e-5 * got).all()      # relative, elementwise: within what LayerNorm is granted of the row's maximum
    assert np.abs(got[3] - 1.0 / d).max() <= 1e-15


@pytest.mark.parametrize("cin,cout,k,stride,pad,dil", [(8, 3, 1, 1, 0, 1), (24, 2, 3, 2, 1, 1), (40, 3, 3, 1, 2, 2), (16, 1, 3, 1, 1, 1), (64, 2, 3, 1, 2, 2),
                                                       (1024, 4, 1, 1, 0, 1)])
def test_conv_is_torch(cin, cout, k, stride, pad, dil):
    rng = np.random.default_rng(cin + cout)
    x, w = rng.standard_normal((2, cin, 7, 9)), rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)
    want = F.conv2d(T64(x), T64(w), None, stride, pad, dil).numpy()
    z, mag, taps = R.conv2d(x, w, stride, pad, dil)
    assert z.shape == want.shape and np.abs(z - want).max() <= 1e-12
    assert taps.shape[0] == k * k and (mag >= np.abs(z) - 1e-12).all()
    narrow_chain = k * k * -(-cin // 64) + 8
    for name in R.LIPSCHITZ:
        ref, A = R.epilogue(z, mag, narrow_chain, None, None, name)
        assert np.isfinite(A).all() and (A > 0).all() and A.max() <= 2e-4 * max(1.0, np.abs(ref).max())


def test_activations_are_torch():
    v = np.linspace(-30, 30, 601)
    t = T64(v)
    for name, f in [("relu", F.relu), ("gelu", F.gelu), ("sigmoid", torch.sigmoid), ("softplus", F.softplus), ("quickgelu", lambda a: a * torch.sigmoid(1.702 * a))]:
        assert np.abs(R.act(v, name) - f(t).numpy()).max() <= 1e-12, name
        # the Lipschitz constants hold on a fine grid
        fine = np.linspace(-12, 12, 240001)
        assert np.abs(np.diff(R.act(fine, name)) / np.diff(fine)).max() <= R.LIPSCHITZ[name], name


@pytest.mark.parametrize("K", [4, 252, 256, 260, 1028])
def test_gemm_bound(K):
    rng = np.random.default_rng(K)
    x, w = rng.standard_normal((9, K + 4)), rng.standard_normal((67, K + 8)) / np.sqrt(K)
    z, mag, chain = R.gemm(x, w, K)
    assert np.abs(z - x[:, :K] @ w[:, :K].T).max() == 0 and chain == -(-K // 256) + 4
    sc, sh = rng.uniform(0.5, 1.5, 67), rng.standard_normal(67)
    for name in R.LIPSCHITZ:
        ref, A = R.epilogue(z, mag, chain, sc, sh, name)
        assert np.isfinite(A).all() and (A > 0).all() and A.max() <= 2e-4 * max(1.0, np.abs(ref).max())
        for e in ("bf16", "f16"):
            assert A.max() <= 0.1 * float(R.ulp(np.abs(ref).max(), e)) / 2


def test_rounding_helpers():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.1, 70000.0, 65519.0, 2.0 ** -25 * 3], np.float32)
    assert np.array_equal(R.rnd(a, "bf16"), T64(a).float().bfloat16().double().numpy())      # ties to even included
    assert np.array_equal(R.rnd(a, "f16")[[0, 3, 6]], a[[0, 3, 6]].astype(np.float16).astype(np.float64))
    assert R.rnd(a, "f16")[4] == 65504.0 and R.rnd(a, "f16")[5] == 65504.0      # saturating
    assert R.ulp(1.0, "bf16") == 2.0 ** -7 and R.ulp(1.999, "f16") == 2.0 ** -10 and R.ulp(2.0, "f16") == 2.0 ** -9 and R.ulp(1e-6, "f16") == 2.0 ** -24
    hi, lo = R.split_pair(np.array([0.1, 1000.3, -3e-5]))
    assert np.abs(hi + lo - np.array([0.1, 1000.3, -3e-5], np.float32).astype(np.float64)).max() <= 2.0 ** -11 * R.ulp(hi, "f16").max()
