"""GPU: technical statistics of images of mixed sizes in one engine call (fe_image_stats_mixed, Engine.image_stats_mixed,
ImageCache.from_mixed, TechnicalAnalyzer.analyze_mixed, BatchScorer(mixed_sizes=True)).

The shapes are those of tests/mixed_cases.py plus 3 x 5, 1 x 7 and 257 x 131. The reference of the record tests is fe_image_stats on every
image alone: all 264 doubles must be equal, the entropy term [260] included, at the default segment size (every image one segment: the
pass-1 block finishes the entropy itself) and at 4096 pixels (96 x 64 spans 2 segments, 300 x 260 spans 20 with a ragged last one,
33 x 47 ends off a 4-pixel boundary: the global histogram and the entropy kernel). 1 x 7 is tested on the raw records only: the host
formula for noise_sigma divides by (w - 2)(h - 2)."""
import contextlib
import ctypes
import math

import numpy as np
import pytest

from facet_amd._lib import FE_ERR_CAPACITY, FE_ERR_INVALID, FE_MODEL_TOPIQ, EngineCapacityError, EngineError
from facet_amd.batch import BatchScorer
from facet_amd.image_stats import TechnicalAnalyzer
from facet_amd.weights import synthetic_state_dict
from mixed_cases import CHUNK_ARENA, SHAPES, STATS_CHUNK_SHAPES, images
from oracle import technical_ref as R

pytestmark = pytest.mark.gpu

ALL_SHAPES = list(SHAPES) + [(3, 5), (1, 7), (257, 131)]
SEGMENTS = [0, 4096]


def _kind(kind, h, w, seed):
    """The image kinds of tests/test_stats_gpu.py."""
    rng = np.random.default_rng(seed)
    if kind == "noise":      # dense bins: every block merges thousands of them
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a = np.zeros((h, w, 3), np.uint8)      # flat: whole waves share a bin
    a[: h // 2] = 17
    a[h // 2:, : w // 3] = 250
    a[h // 2:, w // 3:] = rng.integers(100, 104, (h - h // 2, w - w // 3, 1), dtype=np.uint8)
    return a


@pytest.fixture(scope="module")
def imgs():
    return images(shapes=ALL_SHAPES)


@pytest.fixture(scope="module")
def singles(engine, imgs):
    """fe_image_stats of every image alone. Computed once, never changed."""
    st = np.stack([engine.image_stats(a[None])[0][0] for a in imgs])
    st.setflags(write=False)
    return st


@contextlib.contextmanager
def _segment(engine, pixels):
    engine.set_stats_segment(pixels)
    try:
        yield
    finally:
        engine.set_stats_segment(0)      # the engine fixture is session-wide


def _assert_records(got, want, what):
    assert got.shape == want.shape, what
    for i in range(len(want)):
        bad = np.flatnonzero(got[i] != want[i])
        assert np.array_equal(got[i], want[i]), f"{what}: image {i} {ALL_SHAPES[i] if len(want) == len(ALL_SHAPES) else ''} differs at {bad[:8]}"


@pytest.mark.parametrize("segment", SEGMENTS)
def test_equals_the_per_image_call_in_either_order_and_twice(engine, imgs, singles, segment):
    if segment:      # what the module docstring says about 4096
        assert -(-96 * 64 // segment) == 2 and -(-300 * 260 // segment) == 20 and (300 * 260) % segment and (33 * 47) % 4
    with _segment(engine, segment):
        got = engine.image_stats_mixed(imgs)
        again = engine.image_stats_mixed(imgs)
        rev = engine.image_stats_mixed(imgs[::-1])
    _assert_records(got, singles, "forward")
    _assert_records(rev[::-1], singles, "reversed")
    assert got.tobytes() == again.tobytes()


@pytest.mark.parametrize("segment", SEGMENTS)
def test_against_the_oracle(engine, segment):
    """Integer fields against oracle.technical_ref as in test_stats_gpu.py::test_planes_and_integer_sums_bit_exact; [260] within 1e-12
    relative of the float64 sum over the oracle's hue-saturation histogram."""
    arrs = [_kind("flat", 120, 200, 5), _kind("noise", 96, 128, 5), _kind("flat", 257, 131, 6), _kind("noise", 300, 260, 6)]
    with _segment(engine, segment):
        st = engine.image_stats_mixed(arrs)
    for i, a in enumerate(arrs):
        c = R.ImageCache(a)
        assert np.array_equal(st[i, :256], np.bincount(c.gray.ravel(), minlength=256).astype(np.float64)), i
        lap = R.laplacian64(c.gray)
        assert st[i, 256] == lap.sum() and st[i, 257] == (lap * lap).sum(), i
        assert st[i, 258] == np.abs(R.filter2d_immerkaer(c.gray.astype(np.float64))).sum(), i
        assert st[i, 259] == c.hsv[..., 1].astype(np.int64).sum(), i
        cnt = np.bincount(c.hsv[..., 0].ravel().astype(np.int64) * 256 + c.hsv[..., 1].ravel(), minlength=180 * 256).astype(np.float64)
        want = float((cnt[cnt > 0] * np.log2(cnt[cnt > 0])).sum())
        print(f"[stats_mixed] segment {segment} image {i}: [260] {st[i, 260]!r} oracle {want!r}")
        assert abs(st[i, 260] - want) <= 1e-12 * max(1.0, want), i
        assert not st[i, 261:].any()


@pytest.mark.parametrize("segment", SEGMENTS)
def test_device_pointers_at_every_alignment(engine, imgs, singles, segment):
    """The images back to back in one allocation, no padding."""
    offs = np.concatenate([[0], np.cumsum([a.nbytes for a in imgs])])
    assert {int(o) % 4 for o in offs[:-1]} == {0, 1, 2, 3}
    assert offs[ALL_SHAPES.index((300, 260))] % 4 != 0      # a multi-segment image on the shifted path
    buf = engine.dev_alloc(int(offs[-1]))
    try:
        for a, o in zip(imgs, offs):
            engine.h2d(ctypes.c_void_p(buf.value + int(o)), a)
        with _segment(engine, segment):
            got = engine.image_stats_mixed(([buf.value + int(o) for o in offs[:-1]], [a.shape[:2] for a in imgs]))
    finally:
        engine.dev_free(buf)
    _assert_records(got, singles, "device input")


@pytest.mark.parametrize("segment", SEGMENTS)
def test_channel_order(engine, imgs, singles, segment):
    with _segment(engine, segment):
        got = engine.image_stats_mixed([np.ascontiguousarray(a[..., ::-1]) for a in imgs], order='rgb')
    _assert_records(got, singles, "rgb input")


def test_several_chunks_give_the_same(engine):
    """A 1 MiB arena cuts the eleven images of tests/mixed_cases.py into chunks of 5, 5 and 1 (the figures are there): every double of
    the records equals the default engine's, from the host and resident. An image that cannot fit raises and leaves the engine usable."""
    from facet_amd import Engine
    arrs = images(seed=23, shapes=STATS_CHUNK_SHAPES)
    want = engine.image_stats_mixed(arrs)
    e = Engine(0, arena_bytes=CHUNK_ARENA)
    try:
        assert e.image_stats_mixed(arrs).tobytes() == want.tobytes()
        offs = np.concatenate([[0], np.cumsum([a.nbytes for a in arrs])])
        buf = e.dev_alloc(int(offs[-1]))
        try:
            for a, o in zip(arrs, offs):
                e.h2d(ctypes.c_void_p(buf.value + int(o)), a)
            got = e.image_stats_mixed(([buf.value + int(o) for o in offs[:-1]], [a.shape[:2] for a in arrs]))
        finally:
            e.dev_free(buf)
        assert got.tobytes() == want.tobytes()
        big = np.zeros((600, 500, 3), np.uint8)      # 0.3 MB of gray and 0.9 MB staged
        with pytest.raises(EngineCapacityError, match=r"image 2 \(600 x 500\) needs \d+ bytes of scratch, the arena holds 1048576") as ei:
            e.image_stats_mixed([arrs[0], arrs[4], big])
        assert ei.value.status == FE_ERR_CAPACITY
        assert e.image_stats_mixed(arrs[:7]).tobytes() == want[:7].tobytes()          # the next good call is still right
    finally:
        e.close()


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def test_analyze_mixed_equals_analyze_batch(engine, imgs):
    keep = [i for i, (h, w) in enumerate(ALL_SHAPES) if h >= 3 and w >= 3]
    got = TechnicalAnalyzer.analyze_mixed(engine, [imgs[i] for i in keep], 0.15, 0.10, 0.1)
    assert len(got) == len(keep)
    for g, i in zip(got, keep):
        want = TechnicalAnalyzer.analyze_batch(engine, imgs[i][None], 0.15, 0.10, 0.1)[0]
        assert g.keys() == want.keys()
        assert (g['cache'].height, g['cache'].width) == ALL_SHAPES[i]
        for key in want:
            if key != 'cache':
                assert g[key].keys() == want[key].keys() and all(_same(g[key][k], want[key][k]) for k in want[key]), (i, key)


class _Calls:
    """Counts the calls of some Engine methods of one context."""
    def __init__(self, eng, names):
        self.eng, self.names, self.count = eng, names, {n: 0 for n in names}

    def __enter__(self):
        for n in self.names:
            real = getattr(self.eng, n)

            def spy(*a, _real=real, _n=n, **kw):
                self.count[_n] += 1
                return _real(*a, **kw)
            setattr(self.eng, n, spy)
        return self.count

    def __exit__(self, *exc):
        for n in self.names:
            delattr(self.eng, n)      # the instance attribute goes, the method of the class is back


@pytest.mark.parametrize("aux", [False, True], ids=["one_context", "aux_engine"])
def test_batch_scorer_uses_one_statistics_call_and_gives_the_same_dicts(aux):
    from facet_amd import Engine
    e = Engine(0, arena_bytes=2 << 30)
    e2 = Engine(0, arena_bytes=1 << 30) if aux else None
    try:
        e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
        arrs = images()
        want = BatchScorer(e).process_images(arrs)
        names = ("image_stats", "image_stats_mixed", "swap_rb")
        with contextlib.ExitStack() as stack:
            main = stack.enter_context(_Calls(e, names))
            side = stack.enter_context(_Calls(e2, names)) if aux else main
            got = BatchScorer(e, mixed_sizes=True, aux_engine=e2).process_images(arrs)
        # one statistics call for the ten images of eight shapes, on the aux context when there is one; no BGR copy: no stage reads one
        assert side["image_stats_mixed"] == 1 and main["image_stats"] == 0 and side["image_stats"] == 0 and main["swap_rb"] == 0
        assert len(got) == len(want) == len(arrs)
        for i, (g, r) in enumerate(zip(got, want)):
            assert g.keys() == r.keys(), i
            for key in r:
                if key in ('aesthetic', 'quality_score'):      # TOPIQ on a mixed call against a uniform batch: tests/test_mixed_gpu.py
                    assert g[key] == pytest.approx(r[key], abs=0.011), (i, key)
                else:
                    assert _same(g[key], r[key]), (i, key)
        # with a stage that reads BGR pixels the copy is still made, per shape group, and the dicts still agree
        want_p = BatchScorer(e, phash=True).process_images(arrs)
        with _Calls(e, names) as main:
            got_p = BatchScorer(e, mixed_sizes=True, phash=True, aux_engine=e2).process_images(arrs)
        assert main["swap_rb"] == len(set(SHAPES))
        assert [g['phash'] for g in got_p] == [r['phash'] for r in want_p]
        assert [g['noise_sigma'] for g in got_p] == [r['noise_sigma'] for r in want_p]
    finally:
        e.close()
        if e2 is not None:
            e2.close()


def test_bad_arguments_are_invalid_and_launch_nothing(engine, imgs, singles):
    """A zero height and a null pointer name image 2; a bad order and a bad segment size name the value (they belong to no image)."""
    zero = list(imgs[:2]) + [np.zeros((0, 64, 3), np.uint8)] + list(imgs[2:4])
    with pytest.raises(EngineError, match=r"image 2\b") as ei:
        engine.image_stats_mixed(zero)
    assert ei.value.status == FE_ERR_INVALID
    null = list(imgs[:2]) + [None] + list(imgs[2:4])
    with pytest.raises(EngineError, match=r"image 2\b") as ei:
        engine.image_stats_mixed(null)
    assert ei.value.status == FE_ERR_INVALID
    with pytest.raises(EngineError, match=r"order 2\b") as ei:
        engine.image_stats_mixed(imgs[:3], order=2)
    assert ei.value.status == FE_ERR_INVALID
    try:
        with pytest.raises(EngineError, match=r"\b5000\b") as ei:
            engine.set_stats_segment(5000)
        assert ei.value.status == FE_ERR_INVALID
        _assert_records(engine.image_stats_mixed(imgs), singles, "after the refused calls")      # the context stays usable, the segment unchanged
    finally:
        engine.set_stats_segment(0)
