"""GPU: error behaviour and edge cases of the C-ABI entry points (the reference's failure conventions)."""
import ctypes as C

import numpy as np
import pytest
import torch

from facet_amd import Engine, EngineError
from facet_amd._lib import FE_MODEL_TOPIQ, FE_MODEL_CLIP, FE_MODEL_SAMP
from facet_amd.weights import synthetic_state_dict, synthetic_images

pytestmark = pytest.mark.gpu


def test_not_loaded_and_bad_arguments_return_errors_not_crashes(engine):
    engine.unload(FE_MODEL_TOPIQ)
    with pytest.raises(EngineError, match="not loaded"):
        engine.topiq_score(synthetic_images(1, 1, 64, 64))
    engine.unload(FE_MODEL_CLIP)
    with pytest.raises(EngineError, match="not loaded"):
        engine.clip_encode_image(np.zeros((1, 3, 224, 224), np.float32))
    with pytest.raises(EngineError):
        engine.load_weights(FE_MODEL_TOPIQ, {"semantic_model.conv1.weight": np.zeros((64, 3, 7, 7), np.float32)})  # missing tensors
    assert "missing weight tensor" in engine.lib.fe_last_error(engine.h).decode()
    engine.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 3))
    with pytest.raises(EngineError, match="bad arguments"):
        engine.topiq_score(np.zeros((1, 16, 16, 3), np.uint8))       # smaller than the 32-px pyramid stride
    with pytest.raises((EngineError, ValueError)):
        engine.conv2d(np.zeros((1, 8, 4, 4), np.float32), np.zeros((8, 8, 7, 7), np.float32))  # empty output


def test_a_failed_check_outside_the_vlm_path_is_a_runtime_error_by_number(engine):
    """An FE_CHECK that fails in an entry point without a capacity rule returns FE_ERR_RUNTIME (-2) with its text and launches nothing."""
    src, dst = np.zeros((1, 4, 4, 3), np.uint8), np.full((1, 2, 2, 3), 0xA5, np.uint8)
    box = np.array([0, 0, 5, 4], np.int32)                                              # one column past the image
    rc = engine.lib.fe_reduce_u8(engine.h, src.ctypes.data_as(C.c_void_p), 1, 4, 4, 2, 2, box.ctypes.data_as(C.c_void_p), 0,
                                 dst.ctypes.data_as(C.c_void_p))
    assert rc == -2 and b"reduce: box outside the image or empty" in engine.lib.fe_last_error(engine.h)
    assert (dst == 0xA5).all()


def test_arena_exhaustion_is_a_clean_error_and_recoverable():
    small = Engine(0, arena_bytes=64 << 20)
    small.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 3))
    with pytest.raises(EngineError, match="arena exhausted"):
        small.topiq_score(synthetic_images(1, 2, 512, 512))
    got = small.topiq_score(synthetic_images(1, 1, 64, 96))           # still usable afterwards
    assert np.isfinite(got).all()
    small.close()


@pytest.mark.parametrize("hw", [(97, 131), (250, 333), (64, 64), (33, 500)])
def test_topiq_arbitrary_sizes_match_oracle(engine, hw):
    """Sizes that are not multiples of 32: ceil-mode pyramid, adaptive pooling with ragged windows, odd token grids."""
    from oracle.topiq import CFANet
    sd = synthetic_state_dict("topiq", 3)
    engine.load_weights(FE_MODEL_TOPIQ, sd)
    net = CFANet().eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    imgs = synthetic_images(21, 2, *hw)
    with torch.no_grad():
        ref = net(torch.from_numpy(imgs.astype(np.float32) / 255).permute(0, 3, 1, 2)).flatten().numpy()
    engine.set_microbatch(8)
    got = engine.topiq_score(imgs)
    assert (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)).max() < 1e-3


def test_single_image_and_microbatch_larger_than_batch(engine):
    engine.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 3))
    imgs = synthetic_images(22, 3, 96, 96)
    engine.set_microbatch(64)
    a = engine.topiq_score(imgs)
    engine.set_microbatch(1)
    b = engine.topiq_score(imgs)
    one = engine.topiq_score(imgs[1:2])
    assert np.allclose(a, b, rtol=1e-5, atol=1e-6) and np.allclose(one, a[1:2], rtol=1e-5, atol=1e-6)
    with pytest.raises(EngineError):
        engine.set_microbatch(0)


def test_reload_cycles_do_not_leak_device_memory(engine):
    sd = synthetic_state_dict("samp_net", 5)
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(4):
        engine.load_weights(FE_MODEL_SAMP, sd)
        engine.unload(FE_MODEL_SAMP)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < (64 << 20), f"leaked {(free0 - free1) >> 20} MiB over 4 load/unload cycles"


def test_topiq_long_edge_cap_matches_reference_preprocessing(engine):
    """Images with a long edge > 1024 are LANCZOS-reduced on the GPU exactly like PyIQAScorer._preprocess_image does with
    PIL on the host (reference pyiqa_scorer.py:131-153): engine(raw big image) == engine(PIL-resized image)."""
    from PIL import Image
    engine.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 3))
    big = synthetic_images(31, 2, 700, 1400)
    scale = 1024 / 1400
    small = np.stack([np.asarray(Image.fromarray(a).resize((int(1400 * scale), int(700 * scale)), Image.LANCZOS)) for a in big])
    engine.set_microbatch(2)
    a = engine.topiq_score(big)
    b = engine.topiq_score(small)
    assert np.array_equal(a, b)


# ---- face / statistics entry points: empty results, degenerate shapes, misuse ------------------------------------------------
def test_face_analyze_without_detections_and_without_models(engine):
    from standins import synthetic_onnx as S
    from facet_amd._lib import EngineError, FE_GRAPH_FACE_DET, FE_GRAPH_FACE_LMK, FE_GRAPH_FACE_REC
    imgs = np.random.default_rng(0).integers(0, 256, (2, 96, 160, 3), dtype=np.uint8)
    for slot in (FE_GRAPH_FACE_DET, FE_GRAPH_FACE_LMK, FE_GRAPH_FACE_REC):
        if engine.graph_loaded(slot):
            engine.graph_unload(slot)
    with pytest.raises(EngineError, match="no graph loaded"):
        engine.face_analyze(imgs, (160, 160))
    engine.graph_load(FE_GRAPH_FACE_DET, S.scrfd_like(seed=12, size=160)[0])
    faces, counts, mask = engine.face_analyze(imgs, (160, 160), det_thresh=0.999)      # nothing passes: empty, not an error
    assert mask == 1 and counts.tolist() == [0, 0] and not faces.any()
    faces, counts, mask = engine.face_analyze(imgs, (160, 160), det_thresh=0.5, max_faces=4)   # detector only: boxes + keypoints, no more
    assert mask == 1 and counts.min() > 0
    k = min(int(counts[0]), 4)
    assert np.isfinite(faces).all() and faces[0, :k, 4].min() >= 0.5 and not faces[0, :k, 15:].any()
    assert (np.diff(faces[0, :k, 4]) <= 0).all()                                        # best score first
    with pytest.raises(EngineError):
        engine.face_analyze(imgs, (100, 100))                                           # det size must be a multiple of 32
    engine.graph_unload(FE_GRAPH_FACE_DET)


def test_crops_and_rois_edge_cases(engine):
    from facet_amd._lib import EngineError, FE_GRAPH_FACE_REC
    imgs = np.random.default_rng(1).integers(0, 256, (1, 40, 50, 3), dtype=np.uint8)
    out, crops = engine.face_crops_run(FE_GRAPH_FACE_REC, imgs, np.zeros(0, np.int32), np.zeros((0, 2, 3)), 112, 0.0, 1.0, out_dim=0, want_crops=True)
    assert crops.shape == (0, 112, 112, 3)
    # a crop entirely outside the image is black (borderValue = 0); a singular matrix must not fault
    M = np.array([[[1.0, 0, 500.0], [0, 1.0, 500.0]], [[0.0, 0, 0], [0, 0.0, 0]]])
    _, crops = engine.face_crops_run(FE_GRAPH_FACE_REC, imgs, [0, 0], M, 112, 0.0, 1.0, out_dim=0, want_crops=True)
    assert not crops[0].any() and crops.shape == (2, 112, 112, 3)
    with pytest.raises(EngineError):
        engine.face_crops_run(FE_GRAPH_FACE_REC, imgs, [3], M[:1], 112, 0.0, 1.0, out_dim=0, want_crops=True)      # image index out of range
    assert engine.roi_laplacian(imgs, np.zeros(0, np.int32), np.zeros((0, 4), np.int32)).shape == (0, 4)
    with pytest.raises(EngineError):
        engine.roi_laplacian(imgs, [0], [[0, 0, 51, 40]])                                                            # leaves the image


@pytest.mark.parametrize("shape", [(1, 37), (29, 1), (1, 1), (2, 2), (5, 1024)])
def test_image_stats_degenerate_shapes(engine, shape):
    from oracle import technical_ref as R
    imgs = np.random.default_rng(shape[0] * 7 + shape[1]).integers(0, 256, (2, shape[0], shape[1], 3), dtype=np.uint8)
    st, gray, hsv = engine.image_stats(imgs, want_gray=True, want_hsv=True)
    for i in range(2):
        c = R.ImageCache(imgs[i])
        assert np.array_equal(gray[i], c.gray) and np.array_equal(hsv[i], c.hsv)
        lap = R.laplacian64(c.gray)
        assert st[i, 256] == lap.sum() and st[i, 257] == (lap * lap).sum()
        assert st[i, 258] == np.abs(R.filter2d_immerkaer(c.gray.astype(np.float64))).sum()
        assert st[i, :256].sum() == shape[0] * shape[1]


def test_swap_rb_on_device_and_from_host():
    """fe_swap_rb_u8: the device-side BGR copy of an RGB batch (any pixel count, host or resident source)."""
    from facet_amd import Engine
    e = Engine(0, arena_bytes=1 << 30)
    rng = np.random.default_rng(0)
    for npx in (1, 3, 4, 5, 1023, 64 * 77):
        a = rng.integers(0, 256, (npx, 3), dtype=np.uint8)
        d_src, d_dst = e.dev_alloc(a.nbytes), e.dev_alloc(a.nbytes)
        e.h2d(d_src, a)
        out = np.empty_like(a)
        e.swap_rb(d_src, npx, d_dst)
        e.d2h(out, d_dst)
        assert np.array_equal(out, a[:, ::-1])
        e.swap_rb(a, npx, d_dst)
        e.d2h(out, d_dst)
        assert np.array_equal(out, a[:, ::-1])
        e.dev_free(d_src)
        e.dev_free(d_dst)
    e.close()
