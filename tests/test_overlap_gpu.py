"""GPU: the ensemble call on two lanes (CLIP and SAMP on a side stream beside TOPIQ, facet_amd/csrc/ensemble_plan.h) against the same
call on one lane (FE_NO_OVERLAP, read per call). Neither path changes a launch or its arguments, so the records are compared bit for
bit; a serial-against-serial control runs first, and a column that control finds unstable is held to the control's spread instead."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 96, 80


@pytest.fixture(scope="module")
def eng():
    from facet_amd import Engine
    from facet_amd._lib import FE_MODEL_TOPIQ, FE_MODEL_CLIP, FE_MODEL_AESTHETIC, FE_MODEL_SAMP, FE_MODEL_U2NETP
    from facet_amd.weights import synthetic_state_dict
    e = Engine(0, arena_bytes=12 << 30)
    for model, name in ((FE_MODEL_TOPIQ, "topiq"), (FE_MODEL_CLIP, "clip"), (FE_MODEL_AESTHETIC, "aesthetic"), (FE_MODEL_U2NETP, "u2netp"),
                        (FE_MODEL_SAMP, "samp_net")):
        e.load_weights(model, synthetic_state_dict(name, 21))
    yield e
    e.close()


@pytest.fixture(scope="module")
def images():
    from facet_amd.weights import synthetic_images
    return synthetic_images(17, 70, H, W)


@pytest.fixture(scope="module")
def resident(eng, images):
    p = eng.dev_alloc(images.nbytes)
    eng.h2d(p, images)
    yield p
    eng.dev_free(p)


def score(eng, monkeypatch, imgs, overlap, lanes=None):
    """lanes: None = the engine's choice for the models' precision (an fp32 CLIP tower stays on the main lane), "both" = CLIP and SAMP
    on the side lane, as 2-byte towers run by default (FE_OVERLAP_LANES, read per call)."""
    if overlap:
        monkeypatch.delenv("FE_NO_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("FE_NO_OVERLAP", "1")
    if lanes:
        monkeypatch.setenv("FE_OVERLAP_LANES", lanes)
    else:
        monkeypatch.delenv("FE_OVERLAP_LANES", raising=False)
    rec, mask = eng.ensemble_score(imgs)
    return rec, mask


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("mb", [8, 16, 64])
@pytest.mark.parametrize("n", [1, 7, 45, 70])      # 45 and 70: both towers run a full chunk plus a shifted remainder
def test_overlapped_records_equal_serial_bit_for_bit(eng, images, resident, monkeypatch, n, mb, kind):
    imgs = images[:n] if kind == "host" else (resident, n, H, W)
    eng.set_microbatch(mb)
    try:
        for mask in range(1, 8):
            eng.ensemble_select(mask)
            want, ran = score(eng, monkeypatch, imgs, overlap=False)
            again, _ = score(eng, monkeypatch, imgs, overlap=False)       # the control
            for lanes in (None, "both"):
                got, ran2 = score(eng, monkeypatch, imgs, overlap=True, lanes=lanes)
                assert ran == ran2 == mask
                if same_bits(want, again):
                    assert same_bits(got, want), (mask, lanes, np.argwhere(got != want)[:8].tolist(), float(np.abs(got - want).max()))
                else:      # a column the serial path itself does not reproduce: the overlap may differ by as much, no more
                    spread = np.abs(want - again).max(axis=0)
                    print(f"mask {mask}: serial control differs in columns {np.nonzero(spread)[0][:16].tolist()}, max {float(spread.max()):.3e}")
                    assert (np.abs(got - want).max(axis=0) <= spread).all(), (mask, lanes, float(np.abs(got - want).max()), float(spread.max()))
    finally:
        eng.ensemble_select(7)


def test_repeated_and_resized_calls(eng, images, monkeypatch):
    eng.set_microbatch(16)
    eng.ensemble_select(7)
    first, _ = score(eng, monkeypatch, images[:20], overlap=True, lanes="both")
    for _ in range(2):
        rec, _ = score(eng, monkeypatch, images[:20], overlap=True, lanes="both")
        assert same_bits(rec, first)
    from facet_amd import Engine
    from facet_amd._lib import FE_MODEL_TOPIQ, FE_MODEL_CLIP, FE_MODEL_AESTHETIC, FE_MODEL_SAMP, FE_MODEL_U2NETP
    from facet_amd.weights import synthetic_state_dict
    e = Engine(0, arena_bytes=12 << 30)      # a fresh context: its staging buffers start empty and regrow between the two calls
    try:
        for model, name in ((FE_MODEL_TOPIQ, "topiq"), (FE_MODEL_CLIP, "clip"), (FE_MODEL_AESTHETIC, "aesthetic"), (FE_MODEL_U2NETP, "u2netp"),
                            (FE_MODEL_SAMP, "samp_net")):
            e.load_weights(model, synthetic_state_dict(name, 21))
        e.set_microbatch(4)
        small, _ = score(e, monkeypatch, images[:5], overlap=True, lanes="both")
        e.set_microbatch(16)
        large, _ = score(e, monkeypatch, images[:45], overlap=True, lanes="both")
    finally:
        e.close()
    eng.set_microbatch(4)
    want_small, _ = score(eng, monkeypatch, images[:5], overlap=False)
    eng.set_microbatch(16)
    want_large, _ = score(eng, monkeypatch, images[:45], overlap=False)
    assert same_bits(small, want_small) and same_bits(large, want_large)


def test_flop_counters_do_not_depend_on_the_lanes(eng, images, monkeypatch):
    eng.set_microbatch(16)
    eng.ensemble_select(7)
    counts = []
    for overlap in (False, True):
        eng.flops_reset()
        score(eng, monkeypatch, images[:45], overlap=overlap, lanes="both")
        counts.append((eng.flops(), eng.flops_executed(), eng.flops_half()))
    assert counts[0][0] > 0 and counts[0][1] > 0
    for serial, lanes in zip(*counts):
        assert abs(lanes - serial) <= 1e-12 * abs(serial), (counts)


def test_error_with_side_work_in_flight_then_a_full_call(eng, images, monkeypatch):
    """TOPIQ's first micro-batch of sixteen 1024^2 images wants about twice the 12 GiB arena; the CLIP and SAMP crops of that micro-batch
    are already queued on the side lane when the allocation fails. The next call, all models, must equal its one-lane result."""
    from facet_amd import EngineError
    from facet_amd.weights import synthetic_images
    eng.set_microbatch(16)
    eng.ensemble_select(7)
    monkeypatch.delenv("FE_NO_OVERLAP", raising=False)
    monkeypatch.setenv("FE_OVERLAP_LANES", "both")
    with pytest.raises(EngineError, match="arena exhausted"):
        eng.ensemble_score(synthetic_images(18, 16, 1024, 1024))
    got, ran = score(eng, monkeypatch, images[:20], overlap=True, lanes="both")
    want, _ = score(eng, monkeypatch, images[:20], overlap=False)
    assert ran == 7 and same_bits(got, want)


def test_error_with_side_work_in_flight_leaves_the_engine_usable(monkeypatch):
    """A 64 MiB arena, TOPIQ + SAMP. U2-Net-P on ONE 224^2 crop needs 70.3 MB of scratch (measured: "need 12845056 at 57493760 of
    67108864"; the side arena is never larger than the main one), so in this engine no call that selects SAMP can succeed, whatever the image size; the call
    that follows the error therefore selects TOPIQ alone. test_error_with_side_work_in_flight_then_a_full_call is the same sequence
    with every model in the call that follows."""
    from facet_amd import Engine, EngineError
    from facet_amd._lib import FE_MODEL_TOPIQ, FE_MODEL_SAMP, FE_MODEL_U2NETP
    from facet_amd.weights import synthetic_state_dict, synthetic_images
    e = Engine(0, arena_bytes=64 << 20)
    try:
        e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 21))
        e.load_weights(FE_MODEL_U2NETP, synthetic_state_dict("u2netp", 21))
        e.load_weights(FE_MODEL_SAMP, synthetic_state_dict("samp_net", 21))
        e.set_microbatch(8)
        monkeypatch.delenv("FE_NO_OVERLAP", raising=False)
        # the crops of the first micro-batch are queued on the side lane before TOPIQ's 512^2 micro-batch asks the arena for more than it has
        with pytest.raises(EngineError, match="arena exhausted"):
            e.ensemble_score(synthetic_images(18, 16, 512, 512))
        small = synthetic_images(19, 2, H, W)
        e.set_microbatch(1)
        e.ensemble_select(1)
        got, ran = score(e, monkeypatch, small, overlap=True)
        want, _ = score(e, monkeypatch, small, overlap=False)
        assert ran == 1 and same_bits(got, want) and np.isfinite(got).all() and (got[:, 0] != 0).all()
    finally:
        e.close()
