"""GPU: perceptual hashes of images of mixed sizes in one engine call (fe_phash_mixed, Engine.phash_mixed, facet_amd.phash.phash_mixed).

The 20 images are those of tests/mixed_index_cases.py. Reference of the bits: fe_phash of every image alone (hash and the 64 doubles,
bit for bit) and Pillow itself for the 32 x 32 gray image; reference of the hash: the PIL + scipy.fftpack restatement of imagehash.phash
(tests/golden/make_phash_golden.py), for every image whose block stays farther than TIE_BAND (1e-6, tests/test_phash_host.py) from its
median. The three images with a one-pixel side are constant on an axis, so whole rows or columns of the block are exact zeros and tie with
the median; they are the only ones inside the band (the closest of the other 17 is the second 80 x 80 at 4.9e-4)."""
import ctypes

import numpy as np
import pytest
from PIL import Image

from facet_amd._lib import FE_ERR_CAPACITY, FE_ERR_INVALID, EngineCapacityError, EngineError
from facet_amd.phash import phash_mixed
from facet_amd.thumbnail import thumbnail_plan, thumbnails_mixed
from mixed_index_cases import ALL_SHAPES, CHUNK_ARENA, all_images, chunk_images
from test_phash_host import TIE_BAND

pytestmark = pytest.mark.gpu

ONE_PIXEL_SIDE = [i for i, (h, w) in enumerate(ALL_SHAPES) if h == 1 or w == 1]


@pytest.fixture(scope="module")
def imgs():
    return all_images()


@pytest.fixture(scope="module")
def singles(engine, imgs):
    """fe_phash of every image alone: (hashes [n], small [n,32,32], lo [n,8,8]). Computed once, never changed."""
    got = [engine.phash(a[None], want_small=True, want_dct=True) for a in imgs]
    out = tuple(np.concatenate([g[k] for g in got]) for k in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def _restated(a):
    """(hash, lo, small) of imagehash.phash(Image.fromarray(a)) restated with PIL and scipy."""
    from scipy import fftpack
    small = np.asarray(Image.fromarray(a).convert('L').resize((32, 32), Image.Resampling.LANCZOS))
    lo = fftpack.dct(fftpack.dct(small, axis=0), axis=1)[:8, :8]
    bits = (lo > np.median(lo)).flatten()
    return int("".join(str(int(b)) for b in bits), 2), lo, small


def test_one_call_equals_the_per_image_call(engine, imgs, singles):
    assert len(imgs) == 20 and len(ONE_PIXEL_SIDE) == 3
    hashes, small, lo = engine.phash_mixed(imgs, want_small=True, want_dct=True)
    assert np.array_equal(hashes, singles[0])
    assert small.tobytes() == singles[1].tobytes()
    assert lo.tobytes() == singles[2].tobytes()          # the doubles themselves, not their values
    assert np.array_equal(engine.phash_mixed(imgs), hashes) and np.array_equal(phash_mixed(engine, imgs), hashes)      # the plain calls


def test_one_call_equals_pillow_and_scipy(engine, imgs):
    """`small` is Pillow's for every image, and the hash is the restatement's for every image outside the tie band. 2000 x 10 is the
    image Pillow's Image.resize treats differently: more than 100 times taller than wide, so its vertical pass runs first. With the
    horizontal pass first (what fe_phash did for every shape before fe_phash_mixed came) 184 of its 1024 bytes of `small` were off by 1
    and 2 bits of the hash differed; both calls now take Pillow's order there (phash_tall_kernel)."""
    hashes, small, lo = engine.phash_mixed(imgs, want_small=True, want_dct=True)
    inside, wrong = [], []
    for i, a in enumerate(imgs):
        want_hash, want_lo, want_small = _restated(a)
        margin = float(np.abs(want_lo - np.median(want_lo)).min())
        diff = int((small[i] != want_small).sum())
        print(f"[phash_mixed] image {i} {ALL_SHAPES[i]}: small differs in {diff} bytes (max |d| {int(np.abs(small[i].astype(int) - want_small.astype(int)).max())}), "
              f"margin {margin:.3e}, max |lo - scipy| {np.abs(lo[i] - want_lo).max():.3e}, hash differs in {bin(int(hashes[i]) ^ want_hash).count('1')} bits")
        if diff or not np.abs(lo[i] - want_lo).max() < TIE_BAND:
            wrong.append((i, ALL_SHAPES[i]))
        if margin <= TIE_BAND:
            inside.append(i)
        elif int(hashes[i]) != want_hash:
            wrong.append((i, ALL_SHAPES[i], "hash"))
    assert inside == ONE_PIXEL_SIDE, inside
    assert not wrong, wrong


def test_bgr_order(engine, imgs, singles):
    assert np.array_equal(engine.phash_mixed([np.ascontiguousarray(a[..., ::-1]) for a in imgs], order='bgr'), singles[0])


def test_resident_images_at_every_byte_offset(engine, imgs, singles):
    """The images back to back in one allocation behind one byte: neighbours share dwords, and the last image ends with the buffer."""
    offs = np.concatenate([[0], np.cumsum([a.nbytes for a in imgs])])
    assert {int(o) % 4 for o in offs[:-1]} == {0, 1, 2, 3}
    buf = engine.dev_alloc(int(offs[-1]))
    try:
        for a, o in zip(imgs, offs):
            engine.h2d(ctypes.c_void_p(buf.value + int(o)), a)
        got = engine.phash_mixed(([buf.value + int(o) for o in offs[:-1]], [a.shape[:2] for a in imgs]), want_small=True, want_dct=True)
    finally:
        engine.dev_free(buf)
    assert np.array_equal(got[0], singles[0]) and got[1].tobytes() == singles[1].tobytes() and got[2].tobytes() == singles[2].tobytes()


def test_permutation_and_one_image(engine, imgs, singles):
    perm = np.random.default_rng(3).permutation(len(imgs))
    assert np.array_equal(engine.phash_mixed([imgs[i] for i in perm]), singles[0][perm])
    for i in (0, 7, 15):
        assert np.array_equal(engine.phash_mixed([imgs[i]]), singles[0][i:i + 1])


def test_257_small_images(engine):
    rng = np.random.default_rng(11)
    arrs = [rng.integers(0, 256, (int(rng.integers(1, 40)), int(rng.integers(1, 40)), 3), dtype=np.uint8) for _ in range(257)]
    got = engine.phash_mixed(arrs, want_dct=True)
    for i in (0, 1, 100, 255, 256):
        one = engine.phash(arrs[i][None], want_dct=True)
        assert got[0][i] == one[0][0] and got[2][i].tobytes() == one[2][0].tobytes(), i
    by_shape = {}
    for i, a in enumerate(arrs):
        by_shape.setdefault(a.shape, []).append(i)
    shape, idx = max(by_shape.items(), key=lambda kv: len(kv[1]))          # the largest group against one uniform call
    assert np.array_equal(got[0][idx], engine.phash(np.stack([arrs[i] for i in idx])))


def test_several_chunks_give_the_same(engine):
    """A 1 MiB arena cuts the eleven images of tests/mixed_index_cases.py into chunks of 5, 5 and 1 (the figures are there): every output
    equals the default engine's, from the host and resident. An image that cannot fit raises and leaves the engine usable."""
    from facet_amd import Engine
    arrs = chunk_images()
    want = engine.phash_mixed(arrs, want_small=True, want_dct=True)
    e = Engine(0, arena_bytes=CHUNK_ARENA)
    try:
        def check(got):
            assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        check(e.phash_mixed(arrs, want_small=True, want_dct=True))
        assert np.array_equal(e.phash_mixed(arrs), want[0])
        offs = np.concatenate([[0], np.cumsum([a.nbytes for a in arrs])])
        buf = e.dev_alloc(int(offs[-1]))
        try:
            for a, o in zip(arrs, offs):
                e.h2d(ctypes.c_void_p(buf.value + int(o)), a)
            check(e.phash_mixed(([buf.value + int(o) for o in offs[:-1]], [a.shape[:2] for a in arrs]), want_small=True, want_dct=True))
        finally:
            e.dev_free(buf)
        big = np.zeros((700, 700, 3), np.uint8)      # 1.47 MB staged
        with pytest.raises(EngineCapacityError, match=r"image 1 \(700 x 700\) needs \d+ bytes of scratch, the arena holds 1048576") as ei:
            e.phash_mixed([arrs[4], big])
        assert ei.value.status == FE_ERR_CAPACITY
        check(e.phash_mixed(arrs, want_small=True, want_dct=True))          # the next good call is still right
    finally:
        e.close()


def test_bad_arguments_name_the_image_and_leave_the_context_usable(engine, imgs, singles):
    for bad, what in ((None, "null"), (np.zeros((0, 64, 3), np.uint8), "h = 0"), (np.zeros((1, 32769, 3), np.uint8), "w = 32769")):
        with pytest.raises(EngineError, match=r"image 2\b") as ei:
            engine.phash_mixed(list(imgs[:2]) + [bad] + list(imgs[2:4]))
        assert ei.value.status == FE_ERR_INVALID, what
    with pytest.raises(EngineError, match=r"order 2\b") as ei:
        engine.phash_mixed(imgs[:3], order=2)
    assert ei.value.status == FE_ERR_INVALID
    assert np.array_equal(engine.phash_mixed(imgs), singles[0])


def test_no_table_is_cached_per_size(engine):
    """Three calls over new sizes each: the mixed calls leave the context's per-size tables as they were, fe_phash adds to them."""
    rng = np.random.default_rng(5)

    def fresh(k):      # sizes no other test uses
        return [rng.integers(0, 256, (201 + 7 * k + j, 333 + 5 * k + 2 * j, 3), dtype=np.uint8) for j in range(3)]
    before = engine.resize_cache_entries()
    for k in range(3):
        arrs = fresh(k)
        engine.phash_mixed(arrs)
        thumbnails_mixed(engine, arrs, size=64)
        assert all(not thumbnail_plan(a.shape[1], a.shape[0], 64).unchanged for a in arrs)
    assert engine.resize_cache_entries() == before
    a = fresh(3)[0]
    engine.phash(a[None])
    assert engine.resize_cache_entries() == before + 2          # one table per new side
