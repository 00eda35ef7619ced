"""GPU: the few-row GEMM (gemm_skinny_kernel, kernels_misc.hip) with residual rows, launched alone through fe_op_gemm_skinny_res, against the
float64 reference and the bound of tests/plain_ops_ref.py (the bound tests/test_plain_ops_gpu.py applies to this kernel: A + the store
rounding, A = L_act ((ceil(K / 256) + 10) u sum|x w| |scale| + u |z scale| + u |v| + u |v + res|) + the activation's evaluation error).

The residual is added after scale / shift and before the activation, where the conv epilogue adds its own. The shapes are those the pruned
last block of the CLIP image tower runs (model_clip.hip): (M, K, N) = (1, 128, 64) a small tower's projection, (5, 1024, 1024) the ViT-L/14
attention projections on the MR = 8 form, (32, 4096, 1024) its c_proj on a full chunk of the MR = 32 form. Without a residual the hook is
fe_op_gemm_skinny itself."""
import numpy as np
import pytest

import plain_ops_ref as R

pytestmark = pytest.mark.gpu

FILL = -7.0
POISON = 3e4
SHAPES = [(1, 128, 64), (5, 1024, 1024), (32, 4096, 1024)]
TRIPLES = [("f32", "f32", "f32"), ("bf16", "bf16", "bf16"), ("bf16", "bf16", "f32"), ("f16", "f16", "f16"), ("f16", "f16", "f32"), ("f32", "bf16", "f32"),
           ("f32", "f16", "f32")]


@pytest.fixture(scope="module")
def eng():
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 30)
    yield e
    e.close()


def _case(rng, M, K, N, types):
    """Operands as rounded to their types, with poisoned padding columns: x [M, K + 4], w [N, K + 8], res [M, N + 5], scale, shift [N]."""
    ti, tw, to = types
    x, wt = R.rnd(rng.standard_normal((M, K + 4)), ti), R.rnd(rng.standard_normal((N, K + 8)) / np.sqrt(K), tw)
    res = R.rnd(rng.standard_normal((M, N + 5)), to)
    x[:, K:], wt[:, K:], res[:, N:] = POISON, POISON, POISON
    return x, wt, res, rng.uniform(0.5, 1.5, N).astype(np.float32), rng.standard_normal(N).astype(np.float32)


def _check(w, key, what, got, N, ref, bound):
    assert got.shape[0] == ref.shape[0] and got.shape[1] >= N, (got.shape, ref.shape)
    w.exact(key, what + " columns past N", got[:, N:], np.full_like(got[:, N:], FILL))
    w.close(key, what, got[:, :N], ref, bound)


def test_gemm_skinny_residual_f32(eng):
    """fp32 at the three shapes, ACT_NONE and ACT_GELU, with and without the residual, scale / shift present (the layers' biases)."""
    w = R.Worst("gemm_skinny +res f32")
    types = ("f32", "f32", "f32")
    for M, K, N in SHAPES:
        x, wt, res, sc, sh = _case(R.case_rng("skinny res", M, K, N), M, K, N, types)
        z, mag, chain = R.gemm(x, wt, K)
        for act in (None, "gelu"):
            for r in (None, res):
                ref, A = R.epilogue(z, mag, chain, sc, sh, act, res=None if r is None else r[:, :N])
                got = eng.gemm_skinny(x, wt, K, types=types, scale=sc, shift=sh, act=act, ldy=N + 3, fill=FILL, res=r)
                _check(w, f"MR{8 if M <= 8 else 32} {'res' if r is not None else 'plain'}", f"M {M} K {K} N {N} act {act}", got, N, ref, A)
    w.report()


@pytest.mark.parametrize("types", TRIPLES[1:], ids="-".join)
def test_gemm_skinny_residual_two_byte(eng, types):
    """Every other instantiation takes the residual in its OUTPUT type: one case per form (M = 5 / 9), ragged N, K above one trip of a wave."""
    w = R.Worst("gemm_skinny +res " + "-".join(types))
    for M, act in ((5, "gelu"), (9, None)):
        K, N = 516, 67
        x, wt, res, sc, sh = _case(R.case_rng("skinny res", M, types), M, K, N, types)
        z, mag, chain = R.gemm(x, wt, K)
        ref, A = R.epilogue(z, mag, chain, sc, sh, act, res=res[:, :N])
        got = eng.gemm_skinny(x, wt, K, types=types, scale=sc, shift=sh, act=act, ldy=N + 3, fill=FILL, res=res)
        _check(w, f"MR{8 if M <= 8 else 32}", f"M {M} act {act}", got, N, ref, A + R.store(ref, types[2]))
    w.report()


def test_gemm_skinny_residual_many_rows(eng):
    """M above 32: one launch, blockIdx.y walks the chunks of 32 rows (40 = 32 + 8, 127 = 3 x 32 + 31), with and without the residual, against
    float64 under the same bound; the padding columns of every row keep the fill value."""
    w = R.Worst("gemm_skinny +res many rows")
    types = ("f32", "f32", "f32")
    for M, K, N, act in ((40, 128, 64, "gelu"), (127, 1024, 1024, None)):
        x, wt, res, sc, sh = _case(R.case_rng("skinny res many", M), M, K, N, types)
        z, mag, chain = R.gemm(x, wt, K)
        for r in (None, res):
            ref, A = R.epilogue(z, mag, chain, sc, sh, act, res=None if r is None else r[:, :N])
            got = eng.gemm_skinny(x, wt, K, types=types, scale=sc, shift=sh, act=act, ldy=N + 3, fill=FILL, res=r, many_rows=True)
            _check(w, "res" if r is not None else "plain", f"M {M} K {K} N {N} act {act}", got, N, ref, A)
    w.report()


def test_gemm_skinny_residual_is_exact_on_integers(eng):
    """Integer-valued data (|sum| <= 252 + 8, exact in fp32): the residual form equals the plain result plus the residual, bit for bit, and
    both equal the exact product - with the residual in padded rows (ldr > N)."""
    rng = R.case_rng("skinny res ints")
    for M in (3, 32):
        x, wt = rng.integers(-1, 2, (M, 252)).astype(np.float64), rng.integers(-1, 2, (67, 252)).astype(np.float64)
        res = rng.integers(-8, 9, (M, 70)).astype(np.float64)
        plain = eng.gemm_skinny(x, wt, 252, ldy=67, fill=FILL)
        got = eng.gemm_skinny(x, wt, 252, ldy=67, fill=FILL, res=res)
        assert np.array_equal(plain.astype(np.float64), x @ wt.T)
        assert np.array_equal(got, plain + res[:, :67].astype(np.float32))


def test_gemm_skinny_row_does_not_depend_on_its_call(eng):
    """One input row (and its residual row) in calls of 1, 3 and 32 rows, first, last and in the middle, and in calls of 33 and 127 rows (one
    launch over chunks of 32; first and last chunk, a chunk of one row): the same bits. The pruned CLIP block sends one row per image through
    this kernel, so this is what keeps that block from tying an image's features to its batch."""
    for K, N, act in ((1024, 1024, None), (1024, 4096, "gelu"), (4096, 1024, None)):
        rng = R.case_rng("skinny res rows", K, N)
        x, wt, res, sc, sh = _case(rng, 32, K, N, ("f32", "f32", "f32"))
        row = eng.gemm_skinny(x[5:6], wt, K, scale=sc, shift=sh, act=act, res=res[5:6])[0, :N]
        others = [i for i in range(32) if i != 5]
        for M, at in ((3, 0), (3, 2), (8, 7), (9, 8), (32, 0), (32, 17), (32, 31), (33, 32), (127, 0), (127, 64), (127, 126)):
            order = (others * 5)[:M]
            order[at] = 5
            got = eng.gemm_skinny(x[order], wt, K, scale=sc, shift=sh, act=act, res=res[order], many_rows=True)
            assert np.array_equal(got[at, :N], row), (K, N, act, M, at)
