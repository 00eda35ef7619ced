"""ctypes binding of libfacet_engine.so (C ABI: include/facet_engine.h).

The product path has no CPU fallback: if the shared library or a gfx950 device is missing every
entry point raises EngineError. Only plain pointers and sizes cross the boundary; numpy is used as
the host buffer container.
"""
import ctypes as C
import importlib.util
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FACET_AMD_LIB") or os.path.join(_HERE, "libfacet_engine.so")   # env: developer A/B builds only

FE_MODEL_TOPIQ, FE_MODEL_CLIP, FE_MODEL_SAMP, FE_MODEL_U2NETP, FE_MODEL_AESTHETIC, FE_MODEL_VLM = range(6)
FE_RECORD_FLOATS = 789
FE_GRAPH_FACE_DET, FE_GRAPH_FACE_LMK, FE_GRAPH_FACE_REC = 0, 1, 2
FE_FACE_FLOATS = 739
FE_STATS_DOUBLES = 264
FILTERS = {"lanczos": 1, "bilinear": 2, "bicubic": 3}
FE_PRECISION_RES32 = 16      # or-ed onto a 2-byte precision: fp32 residual streams (include/facet_engine.h fe_precision)
FE_PRECISION_SPLIT3 = 32     # or-ed onto f16: split-operand GEMMs of the CLIP tower ("f16x3")
PRECISION = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "f16": 2, "fp16": 2, "float16": 2, "half": 2,
             "bf16+r32": 1 | FE_PRECISION_RES32, "f16+r32": 2 | FE_PRECISION_RES32, "f16x3": 2 | FE_PRECISION_RES32 | FE_PRECISION_SPLIT3}
PRECISION_NAME = {0: "f32", 1: "bf16", 2: "f16", 1 | FE_PRECISION_RES32: "bf16+r32", 2 | FE_PRECISION_RES32: "f16+r32",
                  2 | FE_PRECISION_RES32 | FE_PRECISION_SPLIT3: "f16x3"}
ACT = {"none": 0, None: 0, "relu": 1, "gelu": 2, "sigmoid": 3, "softplus": 5, "quickgelu": 6}
ELEM = {"f32": 0, "bf16": 1, "f16": 2}      # FE_ELEM_*


VLM_WEIGHT_FORMATS = {"bf16": 0, "fp8": 1}      # FE_VLM_WEIGHTS_BF16 / FE_VLM_WEIGHTS_E4M3
VLM_KV_FORMATS = {"bf16": 0, "fp8": 1, "bf16_e4m3": 2}      # FE_VLM_KV_BF16 / FE_VLM_KV_E4M3 / FE_VLM_KV_BF16_E4M3


class EngineError(RuntimeError):
    pass


class EngineCapacityError(EngineError):
    """The batch did not fit (device memory, arena, KV cache): FE_ERR_CAPACITY, raised by the padded-batch image path only
    (vlm_preprocess_rgb, vlm_encode_preprocessed, vlm_prefill with pad). Fewer images at a time may fit. jpeg_encode / face_thumbnails raise it when the
    caller's `cap` is too small for an image."""


FE_ERR_INVALID = -1
FE_ERR_CAPACITY = -4
FE_MIXED_CLIP, FE_MIXED_SAMP = 0, 1      # fe_preprocess224_mixed modes
FE_ORDER_BGR, FE_ORDER_RGB = 0, 1        # fe_image_stats_mixed / fe_phash_mixed / fe_thumbnail_jpeg_mixed: byte order of a pixel
# fe_thumb_plan (include/facet_engine.h), 52 bytes
THUMB_PLAN_DTYPE = np.dtype([('oh', '<i4'), ('ow', '<i4'), ('fx', '<i4'), ('fy', '<i4'), ('reduce_box', '<i4', (4,)), ('resize_box', '<f4', (4,)),
                             ('tall', '<i4')])


_lib = None
_lib_lock = threading.Lock()

_f32p = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)
_i64p = C.POINTER(C.c_int64)

# name -> (restype, argtypes); every symbol declared in include/facet_engine.h is listed here and
# tests/test_abi.py checks the two stay in sync.
SIGNATURES = {
    "fe_create": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]),
    "fe_destroy": (None, [C.c_void_p]),
    "fe_last_error": (C.c_char_p, [C.c_void_p]),
    "fe_version": (C.c_char_p, []),
    "fe_sync": (C.c_int, [C.c_void_p]),
    "fe_set_microbatch": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_model_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_dev_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "fe_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fe_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fe_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fe_timer_start": (C.c_int, [C.c_void_p]),
    "fe_timer_stop": (C.c_int, [C.c_void_p, _f32p]),
    "fe_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_profile_count": (C.c_int, [C.c_void_p]),
    "fe_profile_get": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), _f32p]),
    "fe_flops_reset": (C.c_int, [C.c_void_p]),
    "fe_flops_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fe_flops_get_executed": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fe_flops_get_half": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fe_weights_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_weights_set": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, _f32p, _i64p, C.c_int]),
    "fe_weights_commit": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_model_unload": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_model_loaded": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_op_conv2d": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, C.c_int,
                               C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "fe_op_gate_rowpool": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p, C.c_int, _f32p, C.c_int,
                                     C.c_int, C.c_int, C.c_int, _f32p, C.POINTER(C.c_int)]),
    "fe_op_wino64": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, _f32p]),
    "fe_op_topiq_gate64": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float,
                                     _f32p, _f32p, C.c_int, C.c_int, _f32p]),
    "fe_op_conv3x3_c64": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _f32p, C.c_int, _f32p, _f32p, _f32p,
                                    _f32p, _f32p]),
    "fe_op_maxpool2d": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, _f32p]),
    "fe_op_bilinear": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "fe_op_adaptive_avgpool": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         _f32p]),
    "fe_op_layernorm": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, _f32p, _f32p, C.c_float, _f32p]),
    "fe_op_plane": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _f32p] + [C.c_int] * 14 + [C.c_float, C.c_float, _f32p]),
    "fe_op_rowpass": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _f32p] + [C.c_int] * 6 + [_f32p, _f32p, C.c_int, C.c_int, C.c_float, C.c_float, _f32p]),
    "fe_op_gemm_skinny": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, _f32p, _f32p, C.c_int,
                                    C.c_int, C.c_float, _f32p]),
    "fe_op_gemm_skinny_res": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, _f32p, _f32p, _f32p,
                                        C.c_int, C.c_int, C.c_int, C.c_float, _f32p]),
    "fe_op_attention": (C.c_int, [C.c_void_p, _f32p, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "fe_op_mha": (C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p,
                            C.c_int, _f32p]),
    "fe_op_vlm_select": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.POINTER(C.c_int32), _f32p]),
    "fe_op_vlm_decode_attention": (C.c_int, [C.c_void_p, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                             _f32p, _f32p, _f32p]),
    "fe_op_vlm_linear": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, _f32p, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _f32p, C.c_float,
                                   C.POINTER(C.c_int32), _f32p, C.c_int, C.c_int, C.c_int, _f32p, _f32p, C.POINTER(C.c_int32)]),
    "fe_op_vlm_rope_cache": (C.c_int, [C.c_void_p, _f32p, C.POINTER(C.c_int32), _f32p, C.c_int, _f32p, _f32p, C.c_float] + [C.c_int] * 12 +
                             [_f32p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _f32p, _f32p]),
    "fe_op_vlm_rows": (C.c_int, [C.c_void_p, C.c_int, _f32p, _f32p, _f32p, C.POINTER(C.c_int32), _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_float, C.c_int, C.c_int, _f32p, _f32p]),
    "fe_op_vlm_vis_rope": (C.c_int, [C.c_void_p, _f32p, C.POINTER(C.c_int32), _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p]),
    "fe_op_vlm_vis_attention": (C.c_int, [C.c_void_p, _f32p, _f32p, _f32p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "fe_op_vlm_prefill_attention": (C.c_int, [C.c_void_p, _f32p, _f32p, _f32p] + [C.c_int] * 6 + [C.POINTER(C.c_int32), _f32p]),
    "fe_set_conv_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_bench_conv": (C.c_int, [C.c_void_p] + [C.c_int] * 12 + [_f32p]),
    "fe_topiq_configure": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "fe_topiq_f32_below": (C.c_int, [C.c_void_p, C.c_longlong]),
    "fe_topiq_feature_shape": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "fe_ensemble_select": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_ensemble_score_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_int)]),
    "fe_topiq_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "fe_topiq_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "fe_clip_encode_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _f32p, _f32p, _f32p]),
    "fe_resize_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_void_p]),
    "fe_clip_encode_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _f32p]),
    "fe_samp_score_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p,
                                       _f32p, _f32p]),
    "fe_clip_encode_text": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, _f32p]),
    "fe_tag_similarities": (C.c_int, [C.c_void_p, _f32p, C.c_int, _f32p, C.c_int, C.c_int, _f32p]),
    "fe_vlm_configure": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int)]),
    "fe_vlm_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "fe_vlm_set_weight_format": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_vlm_weight_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "fe_vlm_set_kv_format": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_vlm_kv_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "fe_vlm_kv_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p]),
    "fe_vlm_prefill": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), _f32p]),
    "fe_vlm_decode_step": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), _f32p]),
    "fe_vlm_vision_configure": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "fe_vlm_encode_images": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                       C.POINTER(C.c_int32), C.c_int, _f32p]),
    "fe_vlm_prefill_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                        C.POINTER(C.c_int32), _f32p]),
    "fe_vlm_generate": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "fe_vlm_generate_scored": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), _f32p]),
    "fe_vlm_last_logprobs": (C.c_int, [C.c_void_p, _f32p]),
    "fe_vlm_preprocess_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), _f32p, _f32p, _f32p]),
    "fe_vlm_encode_preprocessed": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                             C.POINTER(C.c_int32), C.c_int, _f32p]),
    "fe_vlm_vision_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "fe_vlm3_configure": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int]),
    "fe_vlm3_encode_images": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _f32p, C.POINTER(C.c_int32), C.c_int, _f32p, _f32p]),
    "fe_vlm2_configure": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int), C.c_int]),
    "fe_vlm2_encode_images": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, _f32p]),
    "fe_vlm_generate_until": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                        C.POINTER(C.c_int32), _f32p, C.POINTER(C.c_int)]),
    "fe_vlm_prefill_images_padded": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                               C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), _f32p]),
    "fe_ensemble_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p,
                                    C.POINTER(C.c_int)]),
    "fe_ensemble_score_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, _f32p, C.POINTER(C.c_int)]),
    "fe_preprocess224_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, _u8p]),
    "fe_u2netp_saliency": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    "fe_samp_forward": (C.c_int, [C.c_void_p, _f32p, C.c_int, _f32p, _f32p, _f32p, _f32p]),
    "fe_onnx_probe": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _i64p,
                                C.c_char_p, C.c_int]),
    "fe_graph_load": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "fe_graph_unload": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_graph_loaded": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_graph_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _i64p, C.POINTER(C.c_int)]),
    "fe_graph_run": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fe_graph_output_info": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, _i64p, C.POINTER(C.c_int)]),
    "fe_graph_output_copy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _f32p, C.c_size_t]),
    "fe_face_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                 _f32p, C.POINTER(C.c_int), _f32p]),
    "fe_face_crops_run": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                    C.POINTER(C.c_double), C.c_int, C.c_float, C.c_float, C.c_int, _f32p, C.c_int, C.c_void_p]),
    "fe_face_analyze": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                  C.c_int, _f32p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fe_image_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "fe_image_stats_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "fe_set_stats_segment": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_tag_vocab_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "fe_set_tag_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "fe_tag_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fe_tag_select_sims": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fe_roi_laplacian": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_double)]),
    # the mixed-size face calls: ctx, [slot,] images, hw, n, on_device, order, ...
    "fe_face_analyze_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                        C.c_float, C.c_int, _f32p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fe_face_crops_run_mixed": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_float, C.c_float, C.c_int, _f32p, C.c_int, C.c_void_p]),
    "fe_face_det_input_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "fe_roi_laplacian_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "fe_face_thumbnails_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fe_face_cache_entries": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "fe_cv_resize_linear_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fe_aesthetic_score": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float)]),
    "fe_swap_rb_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "fe_leading_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "fe_external_contours": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    "fe_subject_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "fe_leading_lines_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fe_subject_region_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "fe_lines_host_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "fe_phash": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fe_phash_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fe_thumbnail_jpeg_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_size_t, C.c_void_p]),
    "fe_resize_cache_entries": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "fe_resize_u8_box": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "fe_reduce_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "fe_jpeg_bound": (C.c_size_t, [C.c_int, C.c_int]),
    "fe_jpeg_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fe_thumbnail_jpeg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fe_face_thumbnails": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "fe_jpeg_probe": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "fe_jpeg_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fe_jpeg_probe_ex": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "fe_jpeg_decode_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    "fe_jpeg_entropy_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fe_jpeg_scaled_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fe_jpeg_decode_scaled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "fe_jpeg_thumbnail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "fe_hamming_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, _i64p]),
    "fe_burst_links": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                 C.c_int64, C.c_void_p]),
    "fe_knn_core_distances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fe_mreach_mst": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "fe_cosine_best_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fe_similar_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_void_p]),
    "fe_similar_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int, C.c_int64, C.c_void_p, C.c_void_p, _i64p]),
}

FE_CONTOUR_FIELDS = 8      # long longs per contour record
FE_SIM_FUSED, FE_SIM_COSINE = 0, 1
FE_SIM_K_MAX = 32
FE_JPEG_PROGRESSIVE = 1    # flag of fe_jpeg_probe_ex / fe_jpeg_decode_ex (and the status of a progressive file without it)
FE_JPEG_FLAG_PARALLEL = 0x100      # flag of the decode entry points: baseline segments decoded by one lane per 128-byte subsequence
FE_SIM_NO_DATE = -(1 << 63)
FE_BURST_HAS_HASH, FE_BURST_HAS_DATE = 1, 2      # flags of fe_burst_links


class _SimRowsC(C.Structure):
    """fe_sim_rows of include/facet_engine.h"""
    _fields_ = [("emb", C.c_void_p), ("n", C.c_int32), ("on_device", C.c_int32), ("normalise", C.c_int32), ("n_person_ids", C.c_int32),
                ("has_emb", C.c_void_p), ("date", C.c_void_p), ("aggregate", C.c_void_p), ("person_off", C.c_void_p), ("person_ids", C.c_void_p)]


class SimRows:
    """One side (queries or candidates) of Engine.similar_topk / similar_pairs: embeddings plus the optional per-row metadata of the
    fused score. Host form: emb float32 [n,d]; has_emb uint8 [n]; date int64 [n] seconds (FE_SIM_NO_DATE = absent); aggregate float32
    [n] (0 / NaN = absent); person_off int32 [n+1] and person_ids int32 (CSR, ascending and unique per row). Engine.upload_sim_rows
    gives the resident form, in which emb is a (device_ptr, n, d) tuple and the other fields are device pointers."""
    FIELDS = (("has_emb", np.uint8), ("date", np.int64), ("aggregate", np.float32), ("person_off", np.int32), ("person_ids", np.int32))

    def __init__(self, emb, has_emb=None, date=None, aggregate=None, person_off=None, person_ids=None, normalise=True):
        self.on_device = isinstance(emb, tuple)
        self.normalise = bool(normalise)
        self.keep = None                                  # whatever owns the device memory
        self.n_person_ids = 0
        if self.on_device:
            self.emb = (int(emb[0]), int(emb[1]), int(emb[2]))
            self.n, self.d = self.emb[1], self.emb[2]
            self.has_emb, self.date, self.aggregate, self.person_off = has_emb, date, aggregate, person_off
            if person_ids is not None:
                self.person_ids, self.n_person_ids = int(person_ids[0]), int(person_ids[1])   # (device_ptr, count)
            else:
                self.person_ids = None
        else:
            self.emb = np.ascontiguousarray(emb, dtype=np.float32)
            if self.emb.ndim != 2:
                raise ValueError("emb must be [n, d]")
            self.n, self.d = self.emb.shape
            given = dict(has_emb=has_emb, date=date, aggregate=aggregate, person_off=person_off, person_ids=person_ids)
            for name, dt in self.FIELDS:
                v = given[name]
                v = None if v is None else np.ascontiguousarray(v, dtype=dt).reshape(-1)
                want = {"person_off": self.n + 1, "person_ids": None}.get(name, self.n)
                if v is not None and want is not None and v.shape[0] != want:
                    raise ValueError(f"{name}: {v.shape[0]} entries for {self.n} rows")
                setattr(self, name, v)
            if (self.person_off is None) != (self.person_ids is None):
                raise ValueError("person_off and person_ids go together")
            if self.person_ids is not None:
                self.n_person_ids = int(self.person_ids.shape[0])

    def c_struct(self):
        def ptr(v):
            if v is None:
                return None
            return int(v) if self.on_device else v.ctypes.data
        emb = self.emb[0] if self.on_device else self.emb.ctypes.data
        return _SimRowsC(emb, self.n, 1 if self.on_device else 0, 1 if self.normalise else 0, self.n_person_ids, ptr(self.has_emb),
                         ptr(self.date), ptr(self.aggregate), ptr(self.person_off), ptr(self.person_ids))


def _share_hip_runtime_with_torch():
    """One HIP runtime per process. PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64; the engine links the system
    ROCm's. Loaded in the order engine -> torch, the process ends up with two runtimes and torch reports "No HIP GPUs are
    available" (measured: tools/hip_coexist_probe.py); in the order torch -> engine both share torch's copy and work. Facet runs
    torch models (and RCCL through torch.distributed) next to this engine, so when a torch wheel with a bundled runtime is
    installed its copy is mapped first - without importing torch - which makes the import order irrelevant. FACET_AMD_SYSTEM_HIP=1
    keeps the system runtime."""
    if os.environ.get("FACET_AMD_SYSTEM_HIP") == "1" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except (OSError, ImportError, ValueError):
        pass            # no bundled runtime to share: the system one is used


def load_library():
    """dlopen the in-tree engine; raises EngineError (never falls back) when it is missing."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise EngineError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _share_hip_runtime_with_torch()
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:
            raise EngineError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise EngineError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def left_padding(attention_mask):
    """attention_mask int [n, len] -> pad [n] int32, the number of leading zeros of every row. Only left padding is accepted (the one side
    on which batched greedy generation of a decoder-only model is defined): a row whose ones are not one trailing run raises ValueError."""
    am = np.asarray(attention_mask)
    if am.ndim != 2 or not np.isin(am, (0, 1)).all():
        raise ValueError("attention_mask must be a 0/1 matrix [n_seq, len]")
    pad = np.where(am.any(axis=1), np.argmax(am == 1, axis=1), am.shape[1])
    L = am.shape[1]
    for b, p in enumerate(pad):
        if p >= L or not am[b, p:].all():
            raise ValueError(f"attention_mask row {b} is not left padding (zeros, then ones, at least one real token)")
    return pad.astype(np.int32)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_f32p)


def onnx_probe(onnx_bytes):
    """Host-only parse of an .onnx buffer -> dict(nodes, initializers, outputs, input_dims). Raises EngineError on a bad file."""
    lib = load_library()
    buf = C.create_string_buffer(bytes(onnx_bytes), len(onnx_bytes))
    nn, ni, no = C.c_int(), C.c_int(), C.c_int()
    dims = (C.c_int64 * 4)()
    err = C.create_string_buffer(512)
    if lib.fe_onnx_probe(buf, len(onnx_bytes), C.byref(nn), C.byref(ni), C.byref(no), dims, err, 512) != 0:
        raise EngineError(err.value.decode())
    return {"nodes": nn.value, "initializers": ni.value, "outputs": no.value, "input_dims": list(dims)}


class Engine:
    """One engine context = one GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device=0, arena_bytes=0, precision="f32"):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.fe_create(int(device), int(arena_bytes), C.byref(h))
        if rc != 0:
            raise EngineError("fe_create failed: " + (self.lib.fe_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        if PRECISION[precision]:
            self.set_precision(precision)

    def close(self):
        if getattr(self, "h", None):
            self.lib.fe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            err = (EngineCapacityError if rc == FE_ERR_CAPACITY else EngineError)((self.lib.fe_last_error(self.h) or b"?").decode())
            err.status = rc      # the fe_status code (include/facet_engine.h)
            raise err

    # -- misc -------------------------------------------------------------------------------
    def sync(self):
        self._ck(self.lib.fe_sync(self.h))

    def set_precision(self, precision):
        """Precision of the models loaded AFTER this call: 'f32' (default, the reference's CPU numerics), 'f16' (what the reference
        runs CLIP in on a GPU), 'bf16' (BASELINE configs[3]); '+r32' keeps the residual streams in fp32 ('f16+r32', 'bf16+r32')."""
        self._ck(self.lib.fe_set_precision(self.h, PRECISION[precision]))

    def model_precision(self, model):
        """'f32' / 'f16' / 'bf16' (+ '+r32') of a loaded model, None when it is not loaded."""
        v = self.lib.fe_model_precision(self.h, int(model))
        return PRECISION_NAME.get(v)

    def set_microbatch(self, n):
        self._ck(self.lib.fe_set_microbatch(self.h, int(n)))

    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._ck(self.lib.fe_dev_alloc(self.h, int(nbytes), C.byref(p)))
        return p

    def dev_free(self, p):
        self._ck(self.lib.fe_dev_free(self.h, p))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._ck(self.lib.fe_memcpy_h2d(self.h, dptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        self._ck(self.lib.fe_memcpy_d2h(self.h, arr.ctypes.data_as(C.c_void_p), dptr, arr.nbytes))

    def timer_start(self):
        self._ck(self.lib.fe_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._ck(self.lib.fe_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def profile_enable(self, on=True):
        self._ck(self.lib.fe_profile_enable(self.h, 1 if on else 0))

    def profile_records(self):
        out = []
        n = self.lib.fe_profile_count(self.h)
        buf = C.create_string_buffer(160)
        for i in range(n):
            fl, by, ms = C.c_double(), C.c_double(), C.c_float()
            self._ck(self.lib.fe_profile_get(self.h, i, buf, 160, C.byref(fl), C.byref(by), C.byref(ms)))
            out.append({"name": buf.value.decode(), "flops": fl.value, "bytes": by.value, "ms": ms.value})
        return out

    def flops_executed(self):
        f = C.c_double()
        self._ck(self.lib.fe_flops_get_executed(self.h, C.byref(f)))
        return f.value

    def flops_half(self):
        """The part of flops() issued on the 2-byte (bf16 / fp16) matrix instructions."""
        f = C.c_double()
        self._ck(self.lib.fe_flops_get_half(self.h, C.byref(f)))
        return f.value

    def flops_reset(self):
        self._ck(self.lib.fe_flops_reset(self.h))

    def flops(self):
        v = C.c_double()
        self._ck(self.lib.fe_flops_get(self.h, C.byref(v)))
        return v.value

    # -- weights ----------------------------------------------------------------------------
    def load_weights(self, model, state_dict):
        """state_dict: name -> array-like (numpy or torch CPU tensor), PyTorch checkpoint layout."""
        self._ck(self.lib.fe_weights_begin(self.h, model))
        for name, t in state_dict.items():
            a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
            if a.dtype.kind not in "fiu" or a.ndim > 6:
                continue
            a, ap = _f32(a)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._ck(self.lib.fe_weights_set(self.h, model, name.encode(), ap, shape, a.ndim))
        self._ck(self.lib.fe_weights_commit(self.h, model))

    def unload(self, model):
        self._ck(self.lib.fe_model_unload(self.h, model))

    def loaded(self, model):
        return bool(self.lib.fe_model_loaded(self.h, model))

    # -- ops --------------------------------------------------------------------------------
    def conv2d(self, x, w, scale=None, shift=None, res=None, res_after_act=False, stride=1, pad=0, dil=1, act=None):
        x, xp = _f32(x)
        w, wp = _f32(w)
        n, c, h, ww = x.shape
        cout, cin, kh, kw = w.shape
        assert cin == c
        ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
        wo = (ww + 2 * pad - dil * (kw - 1) - 1) // stride + 1
        y = np.empty((n, cout, ho, wo), np.float32)
        sp = hp = rp = None
        if scale is not None:
            scale, sp = _f32(scale)
        if shift is not None:
            shift, hp = _f32(shift)
        if res is not None:
            res, rp = _f32(res)
        self._ck(self.lib.fe_op_conv2d(self.h, xp, n, c, h, ww, wp, cout, kh, kw, sp, hp, rp, int(res_after_act),
                                       stride, pad, dil, ACT[act], y.ctypes.data_as(_f32p)))
        return y

    def gate_rowpool(self, x, weight, bias, gate, th, tw, act="gelu", fused=True, ldx=None):
        """Test hook of the pooled gate of the fp32 TOPIQ head: x [n, cin, h, w], weight [cout, cin], bias [cout] or None, gate [n, h, w] ->
        (mean over the adaptive th x tw windows of act(weight x + bias) * gate as [n, cout, th, tw], whether the row-pooling route ran).
        fused=False forces the plain conv + adaptive pool; ldx > cin places the input rows in a wider NHWC buffer."""
        x = np.asarray(x, np.float32)
        n, cin, h, w = x.shape
        ldx = cin if ldx is None else int(ldx)
        xr = np.full((n, h, w, ldx), 3e4, np.float32)
        xr[..., :cin] = x.transpose(0, 2, 3, 1)
        xr, xp = _f32(xr)
        weight, wp = _f32(weight)
        cout = weight.shape[0]
        assert weight.shape == (cout, cin)
        bp = None
        if bias is not None:
            bias, bp = _f32(bias)
        gate, gp = _f32(gate)
        assert gate.shape == (n, h, w)
        y = np.empty((n, th, tw, cout), np.float32)
        routed = C.c_int(0)
        self._ck(self.lib.fe_op_gate_rowpool(self.h, xp, n, h, w, cin, ldx, wp, bp, cout, gp, ACT[act], th, tw, int(bool(fused)),
                                             y.ctypes.data_as(_f32p), C.byref(routed)))
        return np.ascontiguousarray(y.transpose(0, 3, 1, 2)), bool(routed.value)

    def wino64_conv(self, x, w, scale=None, shift=None, res=None, res_after_act=False, act=None):
        """Test hook of the in-register Winograd kernel (fp32 3x3, stride 1, padding 1, up to 64 -> 64 channels, both multiples of 4), launched
        alone whatever conv2d's routing would choose: act = None, "relu" or "gelu"."""
        x, xp = _f32(x)
        w, wp = _f32(w)
        n, c, h, ww = x.shape
        cout = w.shape[0]
        assert w.shape == (cout, c, 3, 3)
        y = np.empty((n, cout, h, ww), np.float32)
        sp = hp = rp = None
        if scale is not None:
            scale, sp = _f32(scale)
        if shift is not None:
            shift, hp = _f32(shift)
        if res is not None:
            res, rp = _f32(res)
            assert res.shape == y.shape
        self._ck(self.lib.fe_op_wino64(self.h, xp, n, c, h, ww, wp, cout, sp, hp, rp, int(res_after_act), ACT[act], y.ctypes.data_as(_f32p)))
        return y

    def topiq_gate64(self, x, w0, b0, w2, b2, w4, b4, wx, bx, wblk_act="gelu", gate_act="gelu"):
        """Test hook of the fused gate + 16x16 pool of TOPIQ's 64-channel level (2-byte precisions): x [n, 64, h, w]."""
        x, xp = _f32(x)
        n, c, h, w = x.shape
        assert c == 64
        arrs = [_f32(a) for a in (w0, b0, w2, b2, w4, wx, bx)]
        y = np.empty((n, 64, h // 16, w // 16), np.float32)
        self._ck(self.lib.fe_op_topiq_gate64(self.h, xp, n, h, w, arrs[0][1], arrs[1][1], arrs[2][1], arrs[3][1], arrs[4][1], C.c_float(float(b4)),
                                             arrs[5][1], arrs[6][1], ACT[wblk_act], ACT[gate_act], y.ctypes.data_as(_f32p)))
        return y

    def conv3x3_c64(self, x, w2, scale2=None, shift2=None, act2="relu", w3=None, scale3=None, shift3=None, res=None):
        """Test hook of the halo-tiled 3x3 (64 -> 64) kernel and its chained 1x1 expand + identity + ReLU (2-byte precisions)."""
        x, xp = _f32(x)
        n, c, h, w = x.shape
        assert c == 64
        keep = [_f32(a) if a is not None else (None, None) for a in (w2, scale2, shift2, w3, scale3, shift3, res)]
        y = np.empty((n, 256 if w3 is not None else 64, h, w), np.float32)
        self._ck(self.lib.fe_op_conv3x3_c64(self.h, xp, n, h, w, keep[0][1], keep[1][1], keep[2][1], ACT[act2], keep[3][1], keep[4][1], keep[5][1],
                                            keep[6][1], y.ctypes.data_as(_f32p)))
        return y

    def maxpool2d(self, x, k, stride, pad=0, ceil_mode=False):
        x, xp = _f32(x)
        n, c, h, w = x.shape

        def od(i):
            if ceil_mode:
                o = -(-(i + 2 * pad - k) // stride) + 1
                if (o - 1) * stride >= i + pad:
                    o -= 1
                return o
            return (i + 2 * pad - k) // stride + 1
        y = np.empty((n, c, od(h), od(w)), np.float32)
        self._ck(self.lib.fe_op_maxpool2d(self.h, xp, n, c, h, w, k, stride, pad, int(ceil_mode),
                                          y.ctypes.data_as(_f32p)))
        return y

    def bilinear(self, x, ho, wo):
        x, xp = _f32(x)
        n, c, h, w = x.shape
        y = np.empty((n, c, ho, wo), np.float32)
        self._ck(self.lib.fe_op_bilinear(self.h, xp, n, c, h, w, ho, wo, y.ctypes.data_as(_f32p)))
        return y

    def adaptive_avgpool(self, x, ho, wo):
        x, xp = _f32(x)
        n, c, h, w = x.shape
        y = np.empty((n, c, ho, wo), np.float32)
        self._ck(self.lib.fe_op_adaptive_avgpool(self.h, xp, n, c, h, w, ho, wo, y.ctypes.data_as(_f32p)))
        return y

    def layernorm(self, x, g, b, eps=1e-5):
        x, xp = _f32(x)
        g, gp = _f32(g)
        b, bp = _f32(b)
        rows, d = x.shape
        y = np.empty_like(x)
        self._ck(self.lib.fe_op_layernorm(self.h, xp, rows, d, gp, bp, eps, y.ctypes.data_as(_f32p)))
        return y

    PLANE_ROUTES = {"maxpool": 0, "bilinear": 1, "adaptive_avgpool": 2}

    def plane(self, route, x, elem="f32", ho=None, wo=None, k=0, stride=0, pad=0, ceil_mode=False, ctot_in=None, c0_in=0, ctot_out=None, c0_out=0,
              poison=3e4, fill=-7.0):
        """A pooling / resampling kernel launched alone on element type `elem` (fe_op_plane): x [n, c, h, w] sits at channels c0_in .. of a
        device tensor of ctot_in channels (the others hold `poison`), the result is written to channels c0_out .. of a tensor of ctot_out
        channels prefilled with `fill` -> that WHOLE tensor [n, ctot_out, ho, wo]. "maxpool" takes k, stride, pad, ceil_mode (ho / wo
        default to torch's output size), the other two ho and wo."""
        x, xp = _f32(x)
        n, c, h, w = x.shape
        if route == "maxpool":
            def od(i):
                o = (-(-(i + 2 * pad - k) // stride) if ceil_mode else (i + 2 * pad - k) // stride) + 1
                return o - 1 if ceil_mode and (o - 1) * stride >= i + pad else o
            ho, wo = od(h) if ho is None else ho, od(w) if wo is None else wo
        ctot_in = c0_in + c if ctot_in is None else int(ctot_in)
        ctot_out = c0_out + c if ctot_out is None else int(ctot_out)
        y = np.empty((n, ctot_out, int(ho), int(wo)), np.float32)
        self._ck(self.lib.fe_op_plane(self.h, self.PLANE_ROUTES[route], ELEM[elem], xp, n, c, h, w, ctot_in, int(c0_in), ctot_out, int(c0_out), int(k), int(stride),
                                      int(pad), int(bool(ceil_mode)), int(ho), int(wo), float(poison), float(fill), y.ctypes.data_as(_f32p)))
        return y

    ROWPASS_ROUTES = {"layernorm": 0, "layernorm_split": 1, "softmax_rows": 2, "softmax_rows_pad": 3, "add_rows_bcast": 4, "split_hi_lo": 5, "convert": 6}

    def rowpass(self, route, x, d=None, elem_in="f32", elem_out=None, g=None, b=None, ldy=None, eps=1e-5, off_x=0, off_y=None, off_gb=0, fill=-7.0):
        """A row kernel launched alone on explicit element types (fe_op_rowpass): x [rows, ldx] whole (d <= ldx values a row are used),
        -> the WHOLE output [rows, ldy]. "layernorm" / "layernorm_split": g, b [d]; "add_rows_bcast": g = pos [L, d]; the in-place routes
        ("softmax_rows", "softmax_rows_pad", "add_rows_bcast") run on a copy of x, the others write a buffer prefilled with `fill`.
        off_x / off_y / off_gb: elements added to the device base of x / the output / g and b (0 .. 3)."""
        r = self.ROWPASS_ROUTES[route]
        x, xp = _f32(x)
        rows, ldx = x.shape
        d = ldx if d is None else int(d)
        in_place = route in ("softmax_rows", "softmax_rows_pad", "add_rows_bcast")
        elem_out = elem_in if elem_out is None else elem_out
        ldy = (ldx if in_place else 2 * d if route in ("layernorm_split", "split_hi_lo") else d) if ldy is None else int(ldy)
        off_y = off_x if off_y is None else int(off_y)
        null = C.cast(None, _f32p)
        (g, gp), (b, bp) = ((None, null) if g is None else _f32(g)), ((None, null) if b is None else _f32(b))
        L = g.shape[0] if route == "add_rows_bcast" else 0
        assert g is None or g.shape == ((L, d) if L else (d,)), g.shape
        assert b is None or b.shape == (d,), b.shape
        y = np.empty((rows, ldy), np.float32)
        self._ck(self.lib.fe_op_rowpass(self.h, r, ELEM[elem_in], ELEM[elem_out], xp, rows, d, ldx, ldy, int(off_x), off_y, gp, bp, int(off_gb), L, float(eps),
                                        float(fill), y.ctypes.data_as(_f32p)))
        return y

    def gemm_skinny(self, x, w, K, types=("f32", "f32", "f32"), scale=None, shift=None, act=None, ldy=None, fill=-7.0, res=None, many_rows=False):
        """The skinny GEMM launched alone (fe_op_gemm_skinny): x [M, ldx], w [N, ldw], the first K columns of both are contracted; types =
        (activations, weights, output) -> the WHOLE output [M, ldy] (columns >= N keep `fill`). res [M, ldr >= N]: residual rows added before
        the activation; res or many_rows (M up to 4096, chunks of 32 in one launch) go through fe_op_gemm_skinny_res."""
        (x, xp), (w, wp) = _f32(x), _f32(w)
        (M, ldx), (N, ldw) = x.shape, w.shape
        ldy = N if ldy is None else int(ldy)
        null = C.cast(None, _f32p)
        (scale, sp), (shift, hp) = ((None, null) if scale is None else _f32(scale)), ((None, null) if shift is None else _f32(shift))
        assert (scale is None or scale.shape == (N,)) and (shift is None or shift.shape == (N,))
        y = np.empty((M, ldy), np.float32)
        if res is not None or many_rows:
            (res, rp), ldr = (_f32(res), res.shape[1]) if res is not None else ((None, null), 0)
            assert res is None or (res.ndim == 2 and res.shape[0] == M and ldr >= N), res.shape
            self._ck(self.lib.fe_op_gemm_skinny_res(self.h, ELEM[types[0]], ELEM[types[1]], ELEM[types[2]], xp, M, int(K), ldx, wp, N, ldw, sp, hp, rp,
                                                    ldr, ACT[act], ldy, float(fill), y.ctypes.data_as(_f32p)))
            return y
        self._ck(self.lib.fe_op_gemm_skinny(self.h, ELEM[types[0]], ELEM[types[1]], ELEM[types[2]], xp, M, int(K), ldx, wp, N, ldw, sp, hp, ACT[act], ldy,
                                            float(fill), y.ctypes.data_as(_f32p)))
        return y

    def attention(self, q, k, v, bv=None, causal=False, form=0):
        """Test hook of the fused head_dim-64 attention kernels: q [B, Lq, H*64], k / v [B, Lk, H*64], bv [H*64] ->
        softmax(q k^T) v + bv per head (q as the kernel receives it, already scaled). form 1: the split-f16 kernel (f16 precision)."""
        q, qp = _f32(q)
        k, kp = _f32(k)
        v, vp = _f32(v)
        B, Lq, d = q.shape
        Lk = k.shape[1]
        assert d % 64 == 0 and k.shape == (B, Lk, d) and v.shape == (B, Lk, d)
        bv, bp = _f32(np.zeros(d, np.float32) if bv is None else bv)
        assert bv.shape == (d,)
        o = np.empty((B, Lq, d), np.float32)
        self._ck(self.lib.fe_op_attention(self.h, qp, kp, vp, bp, B, d // 64, Lq, Lk, int(causal), int(form), o.ctypes.data_as(_f32p)))
        return o

    def mha(self, x_q, x_kv, heads, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, res=None, causal=False):
        """Test hook of the nn.MultiheadAttention wiring (batch_first): x_q [B, Lq, d], x_kv [B, Lk, d] -> res + out_proj(attention)."""
        x_q, qp = _f32(x_q)
        x_kv, kp = _f32(x_kv)
        B, Lq, d = x_q.shape
        Lk = x_kv.shape[1]
        assert x_kv.shape == (B, Lk, d)
        w = [_f32(a) for a in (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias)]
        assert w[0][0].shape == (3 * d, d) and w[1][0].shape == (3 * d,) and w[2][0].shape == (d, d) and w[3][0].shape == (d,)
        rp = None
        if res is not None:
            res, rp = _f32(res)
            assert res.shape == x_q.shape
        y = np.empty((B, Lq, d), np.float32)
        self._ck(self.lib.fe_op_mha(self.h, qp, kp, B, Lq, Lk, d, int(heads), w[0][1], w[1][1], w[2][1], w[3][1], rp, int(causal),
                                    y.ctypes.data_as(_f32p)))
        return y

    def set_conv_variant(self, v):
        self._ck(self.lib.fe_set_conv_variant(self.h, int(v)))

    def bench_conv(self, n, h, w, cin, cout, k, stride=1, pad=0, res=False, act="relu", variant=0, iters=10):
        ms = C.c_float()
        self._ck(self.lib.fe_bench_conv(self.h, n, h, w, cin, cout, k, stride, pad, int(res), ACT[act], variant, iters,
                                        C.byref(ms)))
        return ms.value

    # -- TOPIQ ------------------------------------------------------------------------------
    @staticmethod
    def _img_ptr(images):
        """images: numpy uint8 [n,h,w,3] (host) or (device_ptr, n, h, w) tuple."""
        if isinstance(images, tuple):
            p, n, h, w = images
            return p, n, h, w, 1, None
        a = np.ascontiguousarray(images, dtype=np.uint8)
        assert a.ndim == 4 and a.shape[3] == 3
        return a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1], a.shape[2], 0, a

    def topiq_configure(self, gate_act="gelu", weight_blk_act="gelu"):
        """Activations of pyiqa's GatedConv used by the NEXT load_weights(FE_MODEL_TOPIQ): 'relu' | 'gelu' | 'softplus'."""
        self._ck(self.lib.fe_topiq_configure(self.h, ACT[gate_act], ACT[weight_blk_act]))

    def topiq_f32_below(self, pixels):
        """2-byte TOPIQ: images with fewer than `pixels` pixels are scored on the model's fp32 weights (0 = never, the default)."""
        self._ck(self.lib.fe_topiq_f32_below(self.h, int(pixels)))

    def topiq_feature_shape(self, h, w, level):
        """(channels, height, width) of pyramid level `level` for h x w images, as the engine computes it (conv / pool output
        sizes, after the > 1024 LANCZOS cap)."""
        dims = (C.c_int * 3)()
        if self.lib.fe_topiq_feature_shape(int(h), int(w), int(level), dims) != 0:
            raise EngineError(f"topiq_feature_shape: bad arguments h={h} w={w} level={level}")
        return tuple(dims)

    def topiq_features(self, images, level):
        p, n, h, w, dev, keep = self._img_ptr(images)
        y = np.empty((n,) + self.topiq_feature_shape(h, w, level), np.float32)
        self._ck(self.lib.fe_topiq_features(self.h, p, n, h, w, dev, level, y.ctypes.data_as(_f32p)))
        return y

    def topiq_score(self, images):
        p, n, h, w, dev, keep = self._img_ptr(images)
        y = np.empty((n,), np.float32)
        self._ck(self.lib.fe_topiq_score(self.h, p, n, h, w, dev, y.ctypes.data_as(_f32p)))
        return y

    # -- U2-Net-P + SAMP-Net ------------------------------------------------------------------
    def u2netp_saliency(self, x):
        """x: float32 [n,3,h,w] normalised -> saliency [n,1,h,w]."""
        x, xp = _f32(x)
        n, c, h, w = x.shape
        assert c == 3
        y = np.empty((n, 1, h, w), np.float32)
        self._ck(self.lib.fe_u2netp_saliency(self.h, xp, n, h, w, y.ctypes.data_as(_f32p)))
        return y

    def samp_forward(self, x, want_saliency=False):
        """x: float32 [n,3,224,224] normalised -> (pattern_weights [n,8], attributes [n,6], score_dist [n,5][, sal])."""
        x, xp = _f32(x)
        n = x.shape[0]
        assert x.shape[1:] == (3, 224, 224)
        pw = np.empty((n, 8), np.float32)
        at = np.empty((n, 6), np.float32)
        sd = np.empty((n, 5), np.float32)
        sal = np.empty((n, 1, 224, 224), np.float32) if want_saliency else None
        self._ck(self.lib.fe_samp_forward(self.h, xp, n, pw.ctypes.data_as(_f32p), at.ctypes.data_as(_f32p),
                                          sd.ctypes.data_as(_f32p),
                                          sal.ctypes.data_as(_f32p) if want_saliency else None))
        return (pw, at, sd, sal) if want_saliency else (pw, at, sd)

    # -- CLIP -------------------------------------------------------------------------------
    def clip_encode_image(self, x, normalized=False, aesthetic=False, out_dim=768):
        """x: float32 [n,3,224,224] (host array) or (device_ptr, n) tuple. Returns features [n,768]
        (+ normalised embedding, + raw aesthetic score) like Facet.get_aesthetic_and_quality_batch needs."""
        if isinstance(x, tuple):
            p, n = x
            dev, keep = 1, None
        else:
            keep = np.ascontiguousarray(x, dtype=np.float32)
            n, dev = keep.shape[0], 0
            p = keep.ctypes.data_as(C.c_void_p)
        feat = np.empty((n, out_dim), np.float32)
        emb = np.empty((n, out_dim), np.float32) if normalized else None
        aes = np.empty((n,), np.float32) if aesthetic else None
        self._ck(self.lib.fe_clip_encode_image(self.h, p, n, dev, feat.ctypes.data_as(_f32p),
                                               emb.ctypes.data_as(_f32p) if normalized else None,
                                               aes.ctypes.data_as(_f32p) if aesthetic else None))
        out = [feat]
        if normalized:
            out.append(emb)
        if aesthetic:
            out.append(aes)
        return out[0] if len(out) == 1 else tuple(out)

    # -- preprocessing + image-level entry points ------------------------------------------
    def resize_u8(self, imgs, oh, ow, filter="bilinear"):
        """PIL-exact resize of a uint8 [n,h,w,3] batch -> [n,oh,ow,3]."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        n, h, w, _ = a.shape
        out = np.empty((n, oh, ow, 3), np.uint8)
        self._ck(self.lib.fe_resize_u8(self.h, a.ctypes.data_as(C.c_void_p), n, h, w, oh, ow, FILTERS[filter], 0,
                                       out.ctypes.data_as(C.c_void_p)))
        return out

    def aesthetic_score(self, feats):
        """feats float32 [n,768] -> raw aesthetic_head outputs [n] (before the (x+1)*5 clamp)."""
        a = np.ascontiguousarray(feats, dtype=np.float32).reshape(-1, 768)
        out = np.empty((a.shape[0],), np.float32)
        self._ck(self.lib.fe_aesthetic_score(self.h, a.ctypes.data_as(_f32p), a.shape[0], out.ctypes.data_as(_f32p)))
        return out

    def clip_encode_images(self, images, normalized=True, aesthetic=True):
        p, n, h, w, dev, keep = self._img_ptr(images)
        feat = np.empty((n, 768), np.float32)
        emb = np.empty((n, 768), np.float32) if normalized else None
        aes = np.empty((n,), np.float32) if aesthetic else None
        self._ck(self.lib.fe_clip_encode_images(self.h, p, n, h, w, dev, feat.ctypes.data_as(_f32p),
                                                emb.ctypes.data_as(_f32p) if normalized else None,
                                                aes.ctypes.data_as(_f32p) if aesthetic else None))
        return feat, emb, aes

    def samp_score_images(self, images, bgr=False):
        p, n, h, w, dev, keep = self._img_ptr(images)
        pw = np.empty((n, 8), np.float32)
        at = np.empty((n, 6), np.float32)
        sd = np.empty((n, 5), np.float32)
        self._ck(self.lib.fe_samp_score_images(self.h, p, n, h, w, int(bgr), dev, pw.ctypes.data_as(_f32p),
                                               at.ctypes.data_as(_f32p), sd.ctypes.data_as(_f32p)))
        return pw, at, sd

    def ensemble_score(self, images):
        """-> (records float32 [n, 789], models_run bitmask). Layout: include/facet_engine.h fe_ensemble_score."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        rec = np.empty((n, FE_RECORD_FLOATS), np.float32)
        mask = C.c_int(0)
        self._ck(self.lib.fe_ensemble_score(self.h, p, n, h, w, dev, rec.ctypes.data_as(_f32p), C.byref(mask)))
        return rec, mask.value

    @staticmethod
    def _img_list(images):
        """A list of uint8 [h, w, 3] arrays (host), or (device_pointers, sizes) with sizes [(h, w), ...] -> the pointer array, the int32
        [n][2] sizes, n, on_device and what must stay alive for the call."""
        if isinstance(images, tuple):
            ptrs, sizes = images
            vals = [p.value if isinstance(p, C.c_void_p) else (None if p is None else int(p)) for p in ptrs]
            hw = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(len(vals), 2))
            return (C.c_void_p * len(vals))(*vals), hw, len(vals), 1, None
        arrs = []
        for i, a in enumerate(images):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint8)
                if a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError(f"image {i}: expected [h,w,3], got {a.shape}")
            arrs.append(a)
        hw = np.ascontiguousarray(np.array([(0, 0) if a is None else a.shape[:2] for a in arrs], dtype=np.int32).reshape(len(arrs), 2))
        return (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs]), hw, len(arrs), 0, arrs

    @staticmethod
    def _hwp(hw):      # the sizes of _img_list as the mixed-size entry points take them
        return hw.ctypes.data_as(C.POINTER(C.c_int32))

    def ensemble_score_mixed(self, images):
        """ensemble_score for images that each have their own size: a list of uint8 [h, w, 3] arrays, or (device_pointers, sizes) for
        resident images. -> (records float32 [n, 789] in input order, models_run bitmask). include/facet_engine.h fe_ensemble_score_mixed."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        rec = np.empty((n, FE_RECORD_FLOATS), np.float32)
        mask = C.c_int(0)
        self._ck(self.lib.fe_ensemble_score_mixed(self.h, ptrs, self._hwp(hw), n, dev, rec.ctypes.data_as(_f32p), C.byref(mask)))
        return rec, mask.value

    def preprocess224_mixed(self, images, mode):
        """The 224 x 224 uint8 crops the mixed-size call feeds CLIP (mode 'clip' / 0) or SAMP-Net (mode 'samp' / 1): [n, 224, 224, 3], Pillow's bytes."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        crops = np.empty((n, 224, 224, 3), np.uint8)
        m = {"clip": FE_MIXED_CLIP, "samp": FE_MIXED_SAMP}.get(mode, mode)
        self._ck(self.lib.fe_preprocess224_mixed(self.h, ptrs, self._hwp(hw), n, dev, int(m), crops.ctypes.data_as(_u8p)))
        return crops

    def ensemble_select(self, models=7):
        """Which loaded models ensemble_score runs: 1 topiq | 2 clip (+ aesthetic) | 4 samp."""
        self._ck(self.lib.fe_ensemble_select(self.h, int(models)))
        self.ensemble_mask = int(models)

    def ensemble_score_dev(self, images, d_records, ld_records=FE_RECORD_FLOATS):
        """ensemble_score with the [n, ld_records] float32 records left in device memory at `d_records` (an int address or
        c_void_p, e.g. torch_tensor.data_ptr()); returns the models_run bitmask after the engine stream has drained."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        mask = C.c_int(0)
        self._ck(self.lib.fe_ensemble_score_dev(self.h, p, n, h, w, dev, C.c_void_p(int(d_records) if not isinstance(d_records, C.c_void_p)
                                                                                     else d_records.value),
                                                int(ld_records), C.byref(mask)))
        return mask.value

    # -- VLM tagger text decoder (models/vlm_tagger.py) ---------------------------------------------------
    def vlm_configure(self, n_heads=28, n_kv_heads=4, head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24)):
        """Geometry read by the NEXT load_weights(FE_MODEL_VLM, ...) (transformers Qwen2_5_VLTextConfig; defaults = Qwen2.5-VL-7B)."""
        ms = (C.c_int * 3)(*[int(v) for v in mrope_section])
        self._ck(self.lib.fe_vlm_configure(self.h, int(n_heads), int(n_kv_heads), int(head_dim), float(rope_theta), float(rms_eps), ms))

    def vlm_weight_format(self, fmt="bf16"):
        """Storage of the decoder's Linear weights (q|k|v, o, gate, up, down of every layer, lm_head) built by the NEXT
        load_weights(FE_MODEL_VLM, ...): "bf16" (default, the reference's dtype) or "fp8" - OCP e4m3 codes with one power-of-two scale
        per output row (facet_amd.weights.quantize_e4m3_rows), half the bytes a decode step streams. Activations, attention, the KV
        cache, the embedding table and the vision tower stay bf16."""
        if fmt not in VLM_WEIGHT_FORMATS:
            raise ValueError(f"vlm_weight_format {fmt!r}: one of {sorted(VLM_WEIGHT_FORMATS)}")
        self._ck(self.lib.fe_vlm_set_weight_format(self.h, VLM_WEIGHT_FORMATS[fmt]))

    def vlm_weight_info(self):
        """The loaded decoder's weight storage (fe_vlm_weight_info): format "bf16" / "fp8", the stored bytes of the matrices a decode step
        streams (layer projections + lm_head), the bytes of their row scales, the number of quantised rows."""
        d = (C.c_int64 * 4)()
        self._ck(self.lib.fe_vlm_weight_info(self.h, d))
        return dict(format={v: k for k, v in VLM_WEIGHT_FORMATS.items()}[int(d[0])], weight_bytes=int(d[1]), scale_bytes=int(d[2]), quantized_rows=int(d[3]))

    def vlm_kv_format(self, fmt="bf16"):
        """Storage of the decoder's KV cache, read by the NEXT prefill (fe_vlm_set_kv_format); independent of vlm_weight_format. "bf16"
        (default), "fp8" - every cache row (the 128 values of one sequence, KV head and position, K and V separately) as OCP e4m3 codes
        with one power-of-two scale, the row rule of facet_amd.weights.quantize_e4m3_rows: 264 bytes per token, KV head and layer instead
        of 512, read directly by the decode attention - or "bf16_e4m3": a bf16 cache holding dequantize(quantize(row)), the arithmetic of
        "fp8" at the storage of "bf16" (for tests and accuracy studies). A change of format drops the live cache."""
        if fmt not in VLM_KV_FORMATS:
            raise ValueError(f"vlm_kv_format {fmt!r}: one of {sorted(VLM_KV_FORMATS)}")
        self._ck(self.lib.fe_vlm_set_kv_format(self.h, VLM_KV_FORMATS[fmt]))

    def vlm_kv_info(self):
        """fe_vlm_kv_info: the format of the next prefill's cache, the bytes one token of one sequence takes in it over all layers, the
        bytes allocated for the live cache (0 before a prefill) and its max_seq."""
        d = (C.c_int64 * 4)()
        self._ck(self.lib.fe_vlm_kv_info(self.h, d))
        return dict(format={v: k for k, v in VLM_KV_FORMATS.items()}[int(d[0])], bytes_per_token=int(d[1]), allocated_bytes=int(d[2]), max_seq=int(d[3]))

    def vlm_kv_rows(self, layer, seq, kv_head, pos0=0, n=None):
        """Rows pos0 .. pos0 + n - 1 (n None: up to the cache length) of the live cache of (layer, sequence, KV head), dequantised:
        (k, v) float32 [n, 128] (fe_vlm_kv_rows)."""
        if n is None:
            n = self.vlm_dims()["cur_len"] - int(pos0)
        k, v = np.empty((int(n), 128), np.float32), np.empty((int(n), 128), np.float32)
        self._ck(self.lib.fe_vlm_kv_rows(self.h, int(layer), int(seq), int(kv_head), int(pos0), int(n), k.ctypes.data_as(_f32p), v.ctypes.data_as(_f32p)))
        return k, v

    def vlm_decode_attention(self, q, k, v, pad=None, kv_format="bf16", len_from_device=False):
        """The decode attention of the VLM decoders launched alone (fe_op_vlm_decode_attention): q [B, nh, 128], k / v [B, nkv, Lk, 128]
        (rounded to bf16), pad int [B] (left padding; None: zeros), the cache built in kv_format by the engine's own fill pass ->
        (out [B, nh, 128], k_image, v_image [B, nkv, Lk, 128]: the dequantised cache rows)."""
        if kv_format not in VLM_KV_FORMATS:
            raise ValueError(f"kv_format {kv_format!r}: one of {sorted(VLM_KV_FORMATS)}")
        (q, qp), (k, kp), (v, vp) = _f32(q), _f32(k), _f32(v)
        B, nh, _ = q.shape
        _, nkv, Lk, _ = k.shape
        assert q.shape == (B, nh, 128) and k.shape == (B, nkv, Lk, 128) and v.shape == k.shape, (q.shape, k.shape, v.shape)
        pd, pdp = self._i32(np.zeros(B, np.int32) if pad is None else pad)
        assert pd.shape == (B,), pd.shape
        out, ki, vi = np.empty_like(q), np.empty_like(k), np.empty_like(v)
        self._ck(self.lib.fe_op_vlm_decode_attention(self.h, qp, kp, vp, B, nh, nkv, Lk, pdp, VLM_KV_FORMATS[kv_format], int(bool(len_from_device)),
                                                     out.ctypes.data_as(_f32p), ki.ctypes.data_as(_f32p), vi.ctypes.data_as(_f32p)))
        return out, ki, vi

    VLM_LINEAR_ROUTES = {"linear": 0, "logits": 1, "add_rmsnorm": 2, "silu_mul": 3}
    VLM_LINEAR_KERNELS = {"auto": 0, "gemv": 1, "gemm32": 2}
    VLM_LINEAR_FAMILIES = {1: "gemv", 2: "gemm32", 3: "wrapper"}

    def vlm_linear(self, x, w, bias=None, weight_format="bf16", route="linear", kernel="auto", w2=None, xres=None, g=None, eps=1e-6,
                   slot=None, ds=None):
        """A decode projection of the VLM decoders launched alone (fe_op_vlm_linear), on weights packed as a model's are and freed on return.
        x [M, ldx] (ldx >= K, ldx % 8 == 0), w [N, K], bias [N] or None; weight_format "bf16" / "fp8". route:
          "linear"       y = bf16(x w^T + bias)                         -> (y, info)
          "logits"       y = x w^T + bias in fp32 (the lm_head's form)  -> (y, info)
          "add_rmsnorm"  r = bf16(xres + bf16(x w^T)) (+ ds[slot[m]] where slot[m] >= 0), n = RMSNorm(r, eps) * g  -> (r, n, info)
          "silu_mul"     h = bf16(silu(bf16(x w^T))) * bf16(x w2^T), one launch for both products  -> (h, info)
        kernel: "auto" (the decoder's choice), "gemv" or "gemm32" (forced; a shape it does not take raises EngineError). info: dict(family
        "gemv" / "gemm32" / "wrapper", mr, splits, direct). All results float32 [M, N]."""
        (x, xp), (w, wp) = _f32(x), _f32(w)
        M, ldx = x.shape
        N, Kw = w.shape
        assert ldx >= Kw and ldx % 8 == 0, (ldx, Kw)
        null, nulli = C.cast(None, _f32p), C.cast(None, C.POINTER(C.c_int32))

        def opt(a, shape):
            if a is None:
                return None, null
            a, p = _f32(a)
            assert a.shape == shape, (a.shape, shape)
            return a, p
        b, bp = opt(bias, (N,))
        w2a, w2p = opt(w2, (N, Kw))
        xr, xrp = opt(xres, (M, N))
        ga, gp = opt(g, (N,))
        dsa, dsp = opt(ds, (0 if ds is None else len(ds), N))
        sl, slp = (None, nulli) if slot is None else self._i32(slot)
        assert sl is None or sl.shape == (M,), sl.shape
        y, y2 = np.empty((M, N), np.float32), np.empty((M, N), np.float32)
        info = (C.c_int32 * 4)()
        self._ck(self.lib.fe_op_vlm_linear(self.h, xp, M, ldx, wp, bp, N, Kw, VLM_WEIGHT_FORMATS[weight_format], w2p, xrp, gp, float(eps), slp, dsp,
                                           0 if dsa is None else dsa.shape[0], self.VLM_LINEAR_ROUTES[route], self.VLM_LINEAR_KERNELS[kernel],
                                           y.ctypes.data_as(_f32p), y2.ctypes.data_as(_f32p), info))
        d = dict(family=self.VLM_LINEAR_FAMILIES.get(int(info[0]), int(info[0])), mr=int(info[1]), splits=int(info[2]), direct=bool(info[3]))
        return (y, y2, d) if route == "add_rmsnorm" else (y, d)

    VLM_ROPE_FAMILIES = {"qwen2_5": 0, "qwen3": 1}

    def vlm_rope_cache(self, qkv, pos, inv_freq, nh, nkv, B, L, sections, family="qwen2_5", qn=None, kn=None, eps=1e-6, start=0,
                       start_from_device=False, max_seq=None, kv_format="bf16", max_blocks=0, fill=0xA5):
        """The rotary embedding + KV-cache append of the VLM decoders launched alone (fe_op_vlm_rope_cache). qkv [B * L, (nh + 2 nkv) * 128]
        (rounded to bf16), pos int [3, B * L], inv_freq [64]; sections: the two section sizes the family reads ("qwen2_5": temporal and
        height of the chunked form; "qwen3": height and width of the interleaved one, with qn / kn [128] and eps). Both caches (and the
        scale arrays of "fp8") are filled with the byte `fill` before the launch.
        -> (q [B * L, nh * 128] float32, k_raw, v_raw [B, nkv, max_seq, 128] as stored: uint16 bf16 bit patterns, or uint8 e4m3 codes,
        k_scale, v_scale [B, nkv, max_seq] float32 for "fp8", else None)."""
        (qkv, qp), (fr, fp) = _f32(qkv), _f32(inv_freq)
        pos, pp = self._i32(pos)
        rows, heads = B * L, nh + 2 * nkv
        max_seq = start + L if max_seq is None else int(max_seq)
        assert qkv.shape == (rows, heads * 128) and pos.shape == (3, rows) and fr.shape == (64,), (qkv.shape, pos.shape, fr.shape)
        null = C.cast(None, _f32p)
        (qn, qnp), (kn, knp) = ((None, null), (None, null)) if qn is None else (_f32(qn), _f32(kn))
        assert qn is None or (qn.shape == (128,) and kn.shape == (128,))
        f8 = kv_format == "fp8"
        q = np.empty((rows, nh * 128), np.float32)
        k = np.empty((B, nkv, max_seq, 128), np.uint8 if f8 else np.uint16)
        v = np.empty_like(k)
        ks, vs = (np.empty((B, nkv, max_seq), np.float32), np.empty((B, nkv, max_seq), np.float32)) if f8 else (None, None)
        u8 = C.POINTER(C.c_uint8)
        self._ck(self.lib.fe_op_vlm_rope_cache(self.h, qp, pp, fp, self.VLM_ROPE_FAMILIES[family], qnp, knp, float(eps), int(sections[0]), int(sections[1]),
                                               int(B), int(L), int(nh), int(nkv), int(start), int(bool(start_from_device)), max_seq,
                                               VLM_KV_FORMATS[kv_format], int(max_blocks), int(fill), q.ctypes.data_as(_f32p), k.ctypes.data_as(u8),
                                               v.ctypes.data_as(u8), ks.ctypes.data_as(_f32p) if f8 else null, vs.ctypes.data_as(_f32p) if f8 else null))
        return q, k, v, ks, vs

    VLM_ROWS_ROUTES = {"rmsnorm": 0, "add": 1, "add_rmsnorm": 2, "add_rmsnorm_no_w": 3, "add_rmsnorm_ds": 4, "few_rows_rmsnorm": 5, "silu_mul": 6}

    def vlm_rows(self, route, x, y=None, w=None, slot=None, ds=None, eps=1e-6, d=None, ldy=None, alias=False, max_blocks=0):
        """A row pass of the VLM decoders launched alone (fe_op_vlm_rows); inputs are rounded to bf16, results are float32 bf16 values.
          "rmsnorm"           x [rows, ldx], d <= ldx values per row normed, w [d] -> n [rows, ldy] (columns past d keep 768)
          "add"               -> bf16(x + y)
          "add_rmsnorm"       -> (r, n): r = bf16(x + y), n = RMSNorm(r) w
          "add_rmsnorm_no_w"  -> r
          "add_rmsnorm_ds"    -> (r, n) with r = bf16(r + ds[slot[row]]) on rows whose slot >= 0, before the norm
          "few_rows_rmsnorm"  -> (x, n), rows <= 64
          "silu_mul"          -> bf16(bf16(silu(x)) y); alias: written over x's buffer"""
        r = self.VLM_ROWS_ROUTES[route]
        x, xp = _f32(x)
        rows, ldx = x.shape
        d = ldx if d is None else int(d)
        ldy = d if ldy is None else int(ldy)
        null, nulli = C.cast(None, _f32p), C.cast(None, C.POINTER(C.c_int32))

        def opt(a, shape):
            if a is None:
                return None, null
            a, p = _f32(a)
            assert a.shape == shape, (a.shape, shape)
            return a, p
        ya, yp = opt(y, (rows, d))
        wa, wp = opt(w, (d,))
        dsa, dsp = opt(ds, (0 if ds is None else len(ds), d))
        sl, slp = (None, nulli) if slot is None else self._i32(slot)
        assert sl is None or sl.shape == (rows,), sl.shape
        gives_x, gives_n = route != "rmsnorm", wa is not None
        ox = np.empty((rows, d), np.float32) if gives_x else None
        on = np.empty((rows, ldy), np.float32) if gives_n else None
        self._ck(self.lib.fe_op_vlm_rows(self.h, r, xp, yp, wp, slp, dsp, 0 if dsa is None else dsa.shape[0], rows, d, ldx, ldy, float(eps), int(bool(alias)),
                                         int(max_blocks), ox.ctypes.data_as(_f32p) if gives_x else null, on.ctypes.data_as(_f32p) if gives_n else null))
        if gives_x and gives_n:
            return ox, on
        return ox if gives_x else on

    def vlm_vis_rope(self, qkv, pos, inv_freq, hd, heads, max_blocks=0):
        """The 2-D rotary embedding of the vision towers launched alone (fe_op_vlm_vis_rope): qkv [rows, 3 * heads * hd] (rounded to bf16), pos
        int [rows, 2], inv_freq [hd / 4] -> (q, k) float32 [rows, heads * hd]."""
        (qkv, qp), (fr, fp) = _f32(qkv), _f32(inv_freq)
        pos, pp = self._i32(pos)
        rows = qkv.shape[0]
        assert qkv.shape == (rows, 3 * heads * hd) and pos.shape == (rows, 2) and fr.shape == (hd // 4,), (qkv.shape, pos.shape, fr.shape)
        q, k = np.empty((rows, heads * hd), np.float32), np.empty((rows, heads * hd), np.float32)
        self._ck(self.lib.fe_op_vlm_vis_rope(self.h, qp, pp, fp, int(hd), rows, int(heads), int(max_blocks), q.ctypes.data_as(_f32p), k.ctypes.data_as(_f32p)))
        return q, k

    def vlm_vis_attention(self, q, k, v, cu, hd, heads, max_seg=None):
        """The segment attention of the vision towers launched alone (fe_op_vlm_vis_attention): q, k, v [N, heads * hd] (rounded to bf16),
        cu int [n_seg + 1] (segment s = rows cu[s] .. cu[s + 1] - 1), hd 64 or 80; max_seg None: the longest segment -> o float32
        [N, heads * hd]. The kernel reads v out of fused rows whose q and k thirds the hook fills with 1.0e4."""
        (q, qp), (k, kp), (v, vp) = _f32(q), _f32(k), _f32(v)
        cu, cp = self._i32(cu)
        n_seg = cu.shape[0] - 1
        N = q.shape[0]
        assert cu.ndim == 1 and n_seg >= 1 and q.shape == (N, heads * hd) and k.shape == q.shape and v.shape == q.shape, (cu.shape, q.shape, k.shape, v.shape)
        assert N == int(cu[-1]), (N, cu)
        if max_seg is None:
            max_seg = int(np.diff(cu).max())
        o = np.empty_like(q)
        self._ck(self.lib.fe_op_vlm_vis_attention(self.h, qp, kp, vp, cp, n_seg, int(max_seg), int(hd), int(heads), o.ctypes.data_as(_f32p)))
        return o

    def vlm_prefill_attention(self, q, k, v, nh, nkv, qpos0=0, max_seq=None, pad=None):
        """The prefill attention of the VLM decoders launched alone (fe_op_vlm_prefill_attention): q [B, Lq, nh * 128], k / v
        [B, nkv, qpos0 + Lq, 128] (rounded to bf16), pad int [B] (left padding; None: zeros); the bf16 caches of max_seq rows (None: Lk) are
        built by the engine's own fill pass over NaN rows -> o float32 [B, Lq, nh * 128]."""
        (q, qp), (k, kp), (v, vp) = _f32(q), _f32(k), _f32(v)
        B, Lq, _ = q.shape
        Lk = int(qpos0) + Lq
        assert q.shape == (B, Lq, nh * 128) and k.shape == (B, nkv, Lk, 128) and v.shape == k.shape, (q.shape, k.shape, v.shape)
        pd, pdp = self._i32(np.zeros(B, np.int32) if pad is None else pad)
        assert pd.shape == (B,), pd.shape
        o = np.empty_like(q)
        self._ck(self.lib.fe_op_vlm_prefill_attention(self.h, qp, kp, vp, B, int(nh), int(nkv), Lq, int(qpos0), Lk if max_seq is None else int(max_seq), pdp,
                                                      o.ctypes.data_as(_f32p)))
        return o

    def vlm_vision_configure(self, n_heads=16, fullatt_block_indexes=(7, 15, 23, 31)):
        """Vision-tower geometry read by the NEXT load_weights(FE_MODEL_VLM, ...) (Qwen2_5_VLVisionConfig; defaults = Qwen2.5-VL-7B)."""
        fa = (C.c_int * max(1, len(fullatt_block_indexes)))(*[int(v) for v in fullatt_block_indexes])
        self._ck(self.lib.fe_vlm_vision_configure(self.h, int(n_heads), fa, len(fullatt_block_indexes)))

    def vlm_encode_images(self, pixel_values, patch_pos_hw, window_index, cu_window_seqlens, cu_seqlens, want_embeds=True):
        """model.visual(pixel_values, grid_thw).pooler_output: float32 [n_patches / 4, hidden] (bf16 values), raster order; the embeddings
        also stay on the device for the next vlm_prefill(..., image_rows=...). Index arrays: facet_amd.vlm_tagger.vision_indices."""
        pv = np.ascontiguousarray(pixel_values, dtype=np.float32)
        n = pv.shape[0]
        pos, pp = self._i32(patch_pos_hw)
        wi, wp = self._i32(window_index)
        cw, cwp = self._i32(cu_window_seqlens)
        cf, cfp = self._i32(cu_seqlens)
        assert pos.shape == (n, 2) and wi.shape == (n // 4,), (pos.shape, wi.shape)
        out = np.empty((n // 4, self.vlm_dims()["hidden"]), np.float32) if want_embeds else None
        self._ck(self.lib.fe_vlm_encode_images(self.h, pv.ctypes.data_as(_f32p), n, pp, wp, cwp, len(cw) - 1, cfp, len(cf) - 1,
                                               out.ctypes.data_as(_f32p) if want_embeds else None))
        return out

    def vlm_preprocess_rgb(self, images, sizes, mean, std, want_pixel_values=False):
        """Qwen2-VL's image processor on the GPU: images = list of uint8 RGB arrays [h, w, 3], sizes = the target (oh, ow) of each
        (facet_amd.vlm_tagger.smart_resize). The patch rows stay on the device for vlm_encode_preprocessed; with want_pixel_values they
        are also returned as the processor's float32 pixel_values [n_patches, 1176] (a Qwen3-VL model: 16-pixel patches, [n_patches, 1536];
        the engine patchifies by the tower it holds, and so are the rows sized here)."""
        imgs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        assert imgs and all(a.ndim == 3 and a.shape[2] == 3 for a in imgs), [a.shape for a in imgs]
        sz, szp = self._i32([[a.shape[0], a.shape[1], int(oh), int(ow)] for a, (oh, ow) in zip(imgs, sizes)])
        assert sz.shape == (len(imgs), 4), sz.shape
        packed = np.concatenate([a.reshape(-1) for a in imgs])
        m, mp = _f32(mean)
        s, sp = _f32(std)
        out = None
        if want_pixel_values:      # rows of the committed tower's patch side (the engine checks the sizes against it before writing)
            patch = self.vlm_vision_dims()["patch"]
            n = int(((sz[:, 2] // patch) * (sz[:, 3] // patch)).sum())
            out = np.empty((n, 6 * patch * patch), np.float32)
        self._ck(self.lib.fe_vlm_preprocess_rgb(self.h, packed.ctypes.data_as(C.c_void_p), len(imgs), szp, mp, sp,
                                                out.ctypes.data_as(_f32p) if want_pixel_values else None))
        return out

    def vlm_encode_preprocessed(self, patch_pos_hw, window_index, cu_window_seqlens, cu_seqlens, want_embeds=True):
        """vlm_encode_images on the patch rows the last vlm_preprocess_rgb left on the device (same index arrays, no pixel upload)."""
        pos, pp = self._i32(patch_pos_hw)
        wi, wp = self._i32(window_index)
        cw, cwp = self._i32(cu_window_seqlens)
        cf, cfp = self._i32(cu_seqlens)
        n = pos.shape[0]
        assert wi.shape == (n // 4,), (pos.shape, wi.shape)
        out = np.empty((n // 4, self.vlm_dims()["hidden"]), np.float32) if want_embeds else None
        self._ck(self.lib.fe_vlm_encode_preprocessed(self.h, pp, wp, cwp, len(cw) - 1, cfp, len(cf) - 1, out.ctypes.data_as(_f32p) if want_embeds else None))
        return out

    def vlm3_configure(self, n_heads=16, n_kv_heads=8, head_dim=128, rope_theta=5e6, rms_eps=1e-6, mrope_section=(24, 20, 20), vis_heads=16,
                       deepstack_indexes=(5, 11, 17)):
        """The NEXT load_weights(FE_MODEL_VLM, ...) builds Qwen3-VL (Qwen3VLForConditionalGeneration; defaults = Qwen3-VL-2B's geometry)."""
        ms = (C.c_int * 3)(*[int(v) for v in mrope_section])
        ds = (C.c_int * max(1, len(deepstack_indexes)))(*[int(v) for v in deepstack_indexes])
        self._ck(self.lib.fe_vlm3_configure(self.h, int(n_heads), int(n_kv_heads), int(head_dim), float(rope_theta), float(rms_eps), ms, int(vis_heads),
                                            ds, len(deepstack_indexes)))

    def vlm2_configure(self, n_heads=12, n_kv_heads=2, head_dim=128, rope_theta=1e6, rms_eps=1e-6, mrope_section=(16, 24, 24), vis_heads=16):
        """The NEXT load_weights(FE_MODEL_VLM, ...) builds Qwen2-VL (Qwen2VLForConditionalGeneration; defaults = Qwen2-VL-2B's geometry)."""
        ms = (C.c_int * 3)(*[int(v) for v in mrope_section])
        self._ck(self.lib.fe_vlm2_configure(self.h, int(n_heads), int(n_kv_heads), int(head_dim), float(rope_theta), float(rms_eps), ms, int(vis_heads)))

    def vlm2_encode_images(self, pixel_values, patch_pos_hw, cu_seqlens, want_embeds=True):
        """Qwen2-VL `model.visual(pixel_values, grid_thw).pooler_output`: pixel_values float [n_patches, 1176], or None = the rows of the
        last vlm_preprocess_rgb; patch_pos_hw [n_patches, 2] and cu_seqlens [n_images + 1] as facet_amd.vlm_tagger.vision_inputs_qwen2
        gives them. The merged embeddings stay on the device for the next vlm_prefill(..., image_rows=...). -> [n/4, hidden] float32
        (bf16 values widened) or None."""
        pos, pp = self._i32(patch_pos_hw)
        n = pos.shape[0]
        assert pos.shape == (n, 2) and n % 4 == 0, pos.shape
        cf, cfp = self._i32(cu_seqlens)
        pvp = None
        if pixel_values is not None:
            pv = np.ascontiguousarray(pixel_values, dtype=np.float32)
            pd = self.vlm_vision_dims()["patch_dim"]
            if pv.shape != (n, pd):
                raise ValueError(f"pixel_values {pv.shape}: expected ({n}, {pd})")
            pvp = pv.ctypes.data_as(_f32p)
        out = np.empty((n // 4, self.vlm_dims()["hidden"]), np.float32) if want_embeds else None
        self._ck(self.lib.fe_vlm2_encode_images(self.h, pvp, n, pp, cfp, len(cf) - 1, out.ctypes.data_as(_f32p) if want_embeds else None))
        return out

    def vlm_vision_dims(self):
        """The committed vision tower: patch side, patch row width, DeepStack levels, position-table side (fe_vlm_vision_dims)."""
        d = (C.c_int * 4)()
        self._ck(self.lib.fe_vlm_vision_dims(self.h, d))
        return dict(zip(("patch", "patch_dim", "n_deepstack", "pos_side"), list(d)))

    def vlm3_encode_images(self, pixel_values, patch_pos_hw, interp_idx, interp_w, cu_seqlens, want_embeds=True, want_deepstack=False):
        """Qwen3-VL `model.visual(pixel_values, grid_thw)`: pixel_values float [n_patches, 1536], or None = the rows of the last
        vlm_preprocess_rgb. Index arrays: facet_amd.vlm_tagger.vision_inputs_qwen3. The merged embeddings and the DeepStack features stay
        on the device for the next vlm_prefill(..., image_rows=...). -> (embeds [n/4, hidden] or None, deepstack [levels, n/4, hidden]
        or None), bf16 values widened to float32; the output shapes come from the committed model (vlm_dims / vlm_vision_dims)."""
        pos, pp = self._i32(patch_pos_hw)
        n = pos.shape[0]
        assert pos.shape == (n, 2) and n % 4 == 0, pos.shape
        ii, iip = self._i32(np.asarray(interp_idx).reshape(n, 4))
        iw, iwp = _f32(np.asarray(interp_w, np.float32).reshape(n, 4))
        cf, cfp = self._i32(cu_seqlens)
        vd = self.vlm_vision_dims()
        pvp = None
        if pixel_values is not None:
            pv = np.ascontiguousarray(pixel_values, dtype=np.float32)
            if pv.shape != (n, vd["patch_dim"]):
                raise ValueError(f"pixel_values {pv.shape}: expected ({n}, {vd['patch_dim']})")
            pvp = pv.ctypes.data_as(_f32p)
        hidden = self.vlm_dims()["hidden"]
        out = np.empty((n // 4, hidden), np.float32) if want_embeds else None
        ds = np.empty((vd["n_deepstack"], n // 4, hidden), np.float32) if want_deepstack and vd["n_deepstack"] > 0 else None
        self._ck(self.lib.fe_vlm3_encode_images(self.h, pvp, n, pp, iip, iwp, cfp, len(cf) - 1, out.ctypes.data_as(_f32p) if want_embeds else None,
                                                ds.ctypes.data_as(_f32p) if ds is not None else None))
        return out, ds

    def vlm_dims(self):
        d = (C.c_int * 8)()
        self._ck(self.lib.fe_vlm_dims(self.h, d))
        return dict(zip(("vocab", "hidden", "layers", "heads", "kv_heads", "intermediate", "max_seq", "cur_len"), list(d)))

    @staticmethod
    def _i32(a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        return a, a.ctypes.data_as(C.POINTER(C.c_int32))

    def vlm_prefill(self, tokens, position_ids=None, max_seq=None, want_logits=False, image_rows=None, pad=None):
        """tokens int [n_seq, len]; position_ids int [3, n_seq, len] (None: text-only positions 0..len-1 on all three axes).
        image_rows: flat row indices (sequence * len + position) of the <|image_pad|> tokens, in order - they take the embeddings of
        the last vlm_encode_images. pad int [n_seq]: left padding of every sequence (fe_vlm_prefill_images_padded; kept for the decode
        steps that follow).
        -> next token ids [n_seq] (greedy) and, with want_logits, the bf16 logits widened to float32 [n_seq, vocab]."""
        tok, tp = self._i32(tokens)
        n, L = tok.shape
        if position_ids is None:
            position_ids = np.broadcast_to(np.arange(L, dtype=np.int32), (3, n, L))
        pos, pp = self._i32(position_ids)
        assert pos.shape == (3, n, L), pos.shape
        nxt = np.empty(n, np.int32)
        lg = np.empty((n, self.vlm_dims()["vocab"]), np.float32) if want_logits else None
        if pad is not None:
            pd, pdp = self._i32(pad)
            assert pd.shape == (n,), pd.shape
            ir, irp = self._i32(image_rows if image_rows is not None else np.zeros(0, np.int32))
            self._ck(self.lib.fe_vlm_prefill_images_padded(self.h, tp, pp, n, L, int(max_seq or min(8192, L + 256)), pdp, irp, int(ir.size),
                                                           nxt.ctypes.data_as(C.POINTER(C.c_int32)), lg.ctypes.data_as(_f32p) if want_logits else None))
        elif image_rows is not None:
            ir, irp = self._i32(image_rows)
            self._ck(self.lib.fe_vlm_prefill_images(self.h, tp, pp, n, L, int(max_seq or min(8192, L + 256)), irp, int(ir.size),
                                                    nxt.ctypes.data_as(C.POINTER(C.c_int32)), lg.ctypes.data_as(_f32p) if want_logits else None))
        else:
            self._ck(self.lib.fe_vlm_prefill(self.h, tp, pp, n, L, int(max_seq or min(8192, L + 256)), nxt.ctypes.data_as(C.POINTER(C.c_int32)),
                                             lg.ctypes.data_as(_f32p) if want_logits else None))
        return (nxt, lg) if want_logits else nxt

    def vlm_decode_step(self, tokens, position_ids, want_logits=False):
        """tokens int [n_seq] (the tokens chosen at the previous step), position_ids int [3, n_seq]."""
        tok, tp = self._i32(tokens)
        pos, pp = self._i32(position_ids)
        n = tok.shape[0]
        assert pos.shape == (3, n), pos.shape
        nxt = np.empty(n, np.int32)
        lg = np.empty((n, self.vlm_dims()["vocab"]), np.float32) if want_logits else None
        self._ck(self.lib.fe_vlm_decode_step(self.h, tp, pp, n, nxt.ctypes.data_as(C.POINTER(C.c_int32)), lg.ctypes.data_as(_f32p) if want_logits else None))
        return (nxt, lg) if want_logits else nxt

    def _vlm_last_logprobs(self, n_seq):
        """Log-probabilities [n_seq] of the tokens chosen by the most recent prefill, decode step or generate step (fe_vlm_last_logprobs;
        n_seq: the sequence count of that prefill)."""
        out = np.empty(int(n_seq), np.float32)
        self._ck(self.lib.fe_vlm_last_logprobs(self.h, out.ctypes.data_as(_f32p)))
        return out

    def select(self, logits):
        """The decoder's greedy selection on caller logits (fe_op_vlm_select): float [rows, vocab], rounded to bf16 first ->
        (ids int32 [rows], log-probabilities float32 [rows] of those ids)."""
        lg, lgp = _f32(logits)
        rows, vocab = lg.shape
        ids = np.empty(rows, np.int32)
        lp = np.empty(rows, np.float32)
        self._ck(self.lib.fe_op_vlm_select(self.h, lgp, rows, vocab, ids.ctypes.data_as(C.POINTER(C.c_int32)), lp.ctypes.data_as(_f32p)))
        return ids, lp

    def vlm_generate_until(self, first_tokens, position_ids, max_steps, eos_token_ids, poll=8, return_logprobs=False):
        """fe_vlm_generate_until after a prefill: first_tokens int [n_seq] (the prefill's choice), position_ids int [3, n_seq] ->
        (tokens int32 [max_steps, n_seq], log-probs float32 [max_steps, n_seq] or None, steps_run)."""
        ft, fp = self._i32(first_tokens)
        n = ft.shape[0]
        ps, pp = self._i32(position_ids)
        assert ps.shape == (3, n), ps.shape
        eos, ep = self._i32(np.asarray([int(e) for e in eos_token_ids], np.int32))
        out = np.empty((int(max_steps), n), np.int32)
        lp = np.empty((int(max_steps), n), np.float32) if return_logprobs else None
        ran = C.c_int(0)
        self._ck(self.lib.fe_vlm_generate_until(self.h, fp, pp, n, int(max_steps), ep, int(eos.size), int(poll), out.ctypes.data_as(C.POINTER(C.c_int32)),
                                                lp.ctypes.data_as(_f32p) if return_logprobs else None, C.byref(ran)))
        return out, lp, int(ran.value)

    def vlm_generate(self, tokens, max_new_tokens, position_ids=None, eos_token_ids=(), want_logits=False, forced_tokens=None, image_rows=None,
                     attention_mask=None, return_logprobs=False, stop_at_eos=False, poll=8):
        """Greedy generation (`generate(..., do_sample=False)`, models/vlm_tagger.py:255-259): prefill + max_new_tokens - 1 decode
        steps for all sequences in lockstep; a sequence that emitted an EOS id keeps receiving that id (what generate's padding does).
        New positions continue from max(position_ids) + 1 per sequence. forced_tokens [n_seq, max_new_tokens]: teacher forcing - the
        token FED at each step is taken from there instead of the engine's own choice (parity tests).
        attention_mask int [n_seq, len]: a LEFT-padded batch (zeros, then ones, per row; position_ids must then be given, e.g.
        vlm_tagger.rope_index(..., attention_mask=...)). None: every position is real (the unpadded path, unchanged).
        return_logprobs: also the log-probability of every chosen token, float32 [n_seq, max_new_tokens] (log_softmax of the step's bf16
        logits at that id, as `generate(..., output_scores=True)` gives it); steps after a row's first EOS are NaN (not generated). Returns
        (ids, logprobs), or (ids, logits, logprobs) with want_logits. The ids are the same with or without it.
        stop_at_eos (the device loop only: no want_logits / forced_tokens): the decode loop ends once every row has emitted one of
        eos_token_ids (at most 8), checked on the host every `poll` steps (fe_vlm_generate_until); same ids and log-probs, fewer steps."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        n, L = tok.shape
        pad = None
        if attention_mask is not None:
            pad = left_padding(attention_mask)
            assert pad.shape == (n,), pad.shape
            if position_ids is None:
                raise ValueError("a padded batch needs its position_ids (vlm_tagger.rope_index with the attention mask)")
        if position_ids is None:
            position_ids = np.broadcast_to(np.arange(L, dtype=np.int32), (3, n, L))
        position_ids = np.ascontiguousarray(position_ids, dtype=np.int32)
        nxt_pos = position_ids.max(axis=(0, 2)) + 1            # [n_seq]
        if not want_logits and forced_tokens is None:
            # the product path: prefill, then every decode step on the device (fe_vlm_generate: captured graph, no host round trips)
            first = self.vlm_prefill(tok, position_ids, max_seq=min(8192, L + max_new_tokens), image_rows=image_rows, pad=pad)
            out = np.empty((n, max_new_tokens), np.int32)
            out[:, 0] = first
            lps = np.empty((n, max_new_tokens), np.float32) if return_logprobs else None
            if return_logprobs:
                lps[:, 0] = self._vlm_last_logprobs(n)
            if max_new_tokens > 1:
                ft, fp = self._i32(first)
                ps, pp = self._i32(np.broadcast_to(nxt_pos.astype(np.int32), (3, n)))
                steps = np.empty((max_new_tokens - 1, n), np.int32)
                if stop_at_eos:
                    steps, slp, _ = self.vlm_generate_until(ft, ps, max_new_tokens - 1, eos_token_ids, poll=poll, return_logprobs=return_logprobs)
                    if return_logprobs:
                        lps[:, 1:] = slp.T
                elif return_logprobs:      # the same device loop, each step's log-probs beside its ids (fe_vlm_generate_scored)
                    slp = np.empty((max_new_tokens - 1, n), np.float32)
                    self._ck(self.lib.fe_vlm_generate_scored(self.h, fp, pp, n, max_new_tokens - 1, steps.ctypes.data_as(C.POINTER(C.c_int32)),
                                                             slp.ctypes.data_as(_f32p)))
                    lps[:, 1:] = slp.T
                else:
                    self._ck(self.lib.fe_vlm_generate(self.h, fp, pp, n, max_new_tokens - 1, steps.ctypes.data_as(C.POINTER(C.c_int32))))
                out[:, 1:] = steps.T
            eos = [int(e) for e in eos_token_ids]
            for b in range(n if eos else 0):      # generate() pads a finished sequence with its EOS id
                hit = np.flatnonzero(np.isin(out[b], eos))
                if hit.size:
                    out[b, hit[0]:] = out[b, hit[0]]
                    if return_logprobs:
                        lps[b, hit[0] + 1:] = np.nan
            return (out, lps) if return_logprobs else out
        out = np.zeros((n, max_new_tokens), np.int32)
        lps = np.full((n, max_new_tokens), np.nan, np.float32) if return_logprobs else None
        logits = []
        r = self.vlm_prefill(tok, position_ids, max_seq=min(8192, L + max_new_tokens), want_logits=want_logits, image_rows=image_rows, pad=pad)
        cur = r[0] if want_logits else r
        cur_lp = self._vlm_last_logprobs(n) if return_logprobs else None
        done = np.zeros(n, bool)
        eos = set(int(e) for e in eos_token_ids)
        for step in range(max_new_tokens):
            if want_logits:
                logits.append(r[1])
            out[:, step] = cur
            if return_logprobs:
                lps[:, step] = cur_lp
            done |= np.isin(cur, list(eos)) if eos else False
            if step + 1 == max_new_tokens or done.all():
                out[:, step + 1:] = cur[:, None] if done.all() else 0
                break
            feed = cur if forced_tokens is None else np.asarray(forced_tokens)[:, step].astype(np.int32)
            r = self.vlm_decode_step(feed, np.broadcast_to(nxt_pos.astype(np.int32), (3, n)), want_logits=want_logits)
            nxt_pos = nxt_pos + 1
            new = r[0] if want_logits else r
            cur = np.where(done, cur, new)
            if return_logprobs:
                cur_lp = np.where(done, np.float32(np.nan), self._vlm_last_logprobs(n))
        if return_logprobs:
            return (out, np.stack(logits, 1), lps) if want_logits else (out, lps)
        return (out, np.stack(logits, 1)) if want_logits else out

    # -- ONNX graphs (InsightFace sessions) -------------------------------------------------------------
    def graph_load(self, slot, onnx_bytes):
        buf = C.create_string_buffer(bytes(onnx_bytes), len(onnx_bytes))
        self._ck(self.lib.fe_graph_load(self.h, int(slot), buf, len(onnx_bytes)))

    def graph_unload(self, slot):
        self._ck(self.lib.fe_graph_unload(self.h, int(slot)))

    def graph_loaded(self, slot):
        return bool(self.lib.fe_graph_loaded(self.h, int(slot)))

    def graph_info(self, slot):
        nn, no, fl = C.c_int(), C.c_int(), C.c_int()
        dims = (C.c_int64 * 4)()
        self._ck(self.lib.fe_graph_info(self.h, int(slot), C.byref(nn), C.byref(no), dims, C.byref(fl)))
        return {"nodes": nn.value, "outputs": no.value, "input_dims": list(dims), "has_sub": bool(fl.value & 1),
                "has_mul": bool(fl.value & 2)}

    def graph_run(self, slot, x):
        """x: float32 [n,c,h,w] -> list of numpy outputs in the model's declared order (ONNX layouts)."""
        x, xp = _f32(x)
        n, c, h, w = x.shape
        self._ck(self.lib.fe_graph_run(self.h, int(slot), xp, n, c, h, w, 0))
        outs = []
        for i in range(self.graph_info(slot)["outputs"]):
            dims = (C.c_int64 * 6)()
            rank = C.c_int()
            name = C.create_string_buffer(256)
            self._ck(self.lib.fe_graph_output_info(self.h, int(slot), i, name, 256, dims, C.byref(rank)))
            shape = tuple(dims[k] for k in range(rank.value))
            y = np.empty(shape, np.float32)
            self._ck(self.lib.fe_graph_output_copy(self.h, int(slot), i, y.ctypes.data_as(_f32p), y.size))
            outs.append(y)
        return outs

    # -- face path ------------------------------------------------------------------------------------------
    def face_detect(self, images, det_size=(640, 640), thresh=0.5, max_cand=512):
        """images: BGR uint8 [n,h,w,3] or (device_ptr,n,h,w). -> (cand [n,max_cand,16], counts [n], det_scale)."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        cand = np.zeros((n, max_cand, 16), np.float32)
        counts = np.zeros((n,), np.int32)
        ds = C.c_float()
        self._ck(self.lib.fe_face_detect(self.h, p, n, h, w, dev, int(det_size[0]), int(det_size[1]), float(thresh), int(max_cand),
                                         cand.ctypes.data_as(_f32p), counts.ctypes.data_as(C.POINTER(C.c_int)), C.byref(ds)))
        return cand, counts, ds.value

    def face_crops_run(self, slot, images, img_index, M, size, mean, scale, swap_rb=True, out_dim=0, want_crops=False):
        """M: float64 [m,2,3] forward affine matrices. -> (out [m,out_dim] or None, crops uint8 [m,size,size,3] or None)."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        idx = np.ascontiguousarray(img_index, dtype=np.int32)
        Mm = np.ascontiguousarray(M, dtype=np.float64).reshape(-1, 6)
        m = idx.shape[0]
        assert Mm.shape[0] == m
        out = np.empty((m, out_dim), np.float32) if out_dim else None
        crops = np.empty((m, size, size, 3), np.uint8) if want_crops else None
        self._ck(self.lib.fe_face_crops_run(self.h, int(slot), p, n, h, w, dev, m, idx.ctypes.data_as(C.POINTER(C.c_int)),
                                            Mm.ctypes.data_as(C.POINTER(C.c_double)), int(size), float(mean), float(scale), int(swap_rb),
                                            out.ctypes.data_as(_f32p) if out_dim else None, int(out_dim),
                                            crops.ctypes.data_as(C.c_void_p) if want_crops else None))
        return out, crops

    def face_analyze(self, images, det_size=(640, 640), det_thresh=0.5, nms_thresh=0.4, max_faces=8):
        """-> (faces float32 [n,max_faces,739], counts int32 [n], models_run bitmask); layout: include/facet_engine.h."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        faces = np.empty((n, max_faces, FE_FACE_FLOATS), np.float32)
        counts = np.zeros((n,), np.int32)
        mask = C.c_int(0)
        self._ck(self.lib.fe_face_analyze(self.h, p, n, h, w, dev, int(det_size[0]), int(det_size[1]), float(det_thresh),
                                          float(nms_thresh), int(max_faces), faces.ctypes.data_as(_f32p),
                                          counts.ctypes.data_as(C.POINTER(C.c_int)), C.byref(mask)))
        return faces, counts, mask.value

    # -- face path over images that each have their own size: `images` is a list of uint8 [h, w, 3] arrays, or (device_pointers, sizes)
    #    for resident images; order 'bgr' / 'rgb' (or FE_ORDER_*) is the byte order of a pixel. include/facet_engine.h
    @staticmethod
    def _order(order):
        return int({"bgr": FE_ORDER_BGR, "rgb": FE_ORDER_RGB}.get(order, order))

    def face_analyze_mixed(self, images, det_size=(640, 640), det_thresh=0.5, nms_thresh=0.4, max_faces=8, order='bgr'):
        """face_analyze for a list of images of any sizes in one call: every graph runs over full micro-batches whatever the shapes.
        -> (faces float32 [n,max_faces,739], counts int32 [n], models_run bitmask), in input order."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        faces = np.empty((max(n, 0), max_faces, FE_FACE_FLOATS), np.float32)
        counts = np.zeros((max(n, 0),), np.int32)
        mask = C.c_int(0)
        self._ck(self.lib.fe_face_analyze_mixed(self.h, ptrs, self._hwp(hw), n, dev, self._order(order), int(det_size[0]),
                                                int(det_size[1]), float(det_thresh), float(nms_thresh), int(max_faces), faces.ctypes.data_as(_f32p),
                                                counts.ctypes.data_as(C.POINTER(C.c_int)), C.byref(mask)))
        return faces, counts, mask.value

    def face_crops_run_mixed(self, slot, images, img_index, M, size, mean, scale, swap_rb=True, out_dim=0, want_crops=False, order='bgr'):
        """face_crops_run with img_index into a list of images of any sizes. The crops come back in the images' own byte order."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        idx = np.ascontiguousarray(img_index, dtype=np.int32)
        Mm = np.ascontiguousarray(M, dtype=np.float64).reshape(-1, 6)
        m = idx.shape[0]
        assert Mm.shape[0] == m
        out = np.empty((m, out_dim), np.float32) if out_dim else None
        crops = np.empty((m, size, size, 3), np.uint8) if want_crops else None
        self._ck(self.lib.fe_face_crops_run_mixed(self.h, int(slot), ptrs, self._hwp(hw), n, dev, self._order(order), m,
                                                  idx.ctypes.data_as(C.POINTER(C.c_int)), Mm.ctypes.data_as(C.POINTER(C.c_double)), int(size), float(mean),
                                                  float(scale), int(swap_rb), out.ctypes.data_as(_f32p) if out_dim else None, int(out_dim),
                                                  crops.ctypes.data_as(C.c_void_p) if want_crops else None))
        return out, crops

    def face_det_input_mixed(self, images, det_size=(640, 640), order='bgr'):
        """The detector input face_analyze_mixed makes of every image: float32 [n, det_h, det_w, 4] (R, G, B, 0). For the parity tests."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        out = np.empty((max(n, 0), int(det_size[0]), int(det_size[1]), 4), np.float32)
        self._ck(self.lib.fe_face_det_input_mixed(self.h, ptrs, self._hwp(hw), n, dev, self._order(order), int(det_size[0]),
                                                  int(det_size[1]), out.ctypes.data_as(_f32p)))
        return out

    def roi_laplacian_mixed(self, images, img_index, rois, order='bgr'):
        """roi_laplacian with img_index into a list of images of any sizes -> float64 [m,4], every double equal to roi_laplacian's."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        idx = np.ascontiguousarray(img_index, dtype=np.int32)
        r = np.ascontiguousarray(rois, dtype=np.int32).reshape(-1, 4)
        out = np.zeros((idx.shape[0], 4), np.float64)
        self._ck(self.lib.fe_roi_laplacian_mixed(self.h, ptrs, self._hwp(hw), n, dev, self._order(order), idx.shape[0],
                                                 idx.ctypes.data_as(C.POINTER(C.c_int)), r.ctypes.data_as(C.POINTER(C.c_int)),
                                                 out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def face_cache_entries(self):
        """How many cv2.resize weight tables the context keeps per size (fe_face_cache_entries): face_detect / face_analyze /
        cv_resize_linear add to it with every new size, the mixed-size face calls never do."""
        v = C.c_int32(0)
        self._ck(self.lib.fe_face_cache_entries(self.h, C.byref(v)))
        return v.value

    def image_stats(self, images, want_gray=False, want_hsv=False):
        """BGR uint8 [n,h,w,3] (or device tuple) -> (stats float64 [n,264], gray uint8 [n,h,w] | None, hsv uint8 [n,h,w,3] | None)."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        stats = np.empty((n, FE_STATS_DOUBLES), np.float64)
        gray = np.empty((n, h, w), np.uint8) if want_gray else None
        hsv = np.empty((n, h, w, 3), np.uint8) if want_hsv else None
        self._ck(self.lib.fe_image_stats(self.h, p, n, h, w, dev, stats.ctypes.data_as(C.POINTER(C.c_double)),
                                         gray.ctypes.data_as(C.c_void_p) if want_gray else None,
                                         hsv.ctypes.data_as(C.c_void_p) if want_hsv else None))
        return stats, gray, hsv

    def image_stats_mixed(self, images, order='bgr'):
        """image_stats for images that each have their own size: a list of uint8 [h, w, 3] arrays, or (device_pointers, sizes) for resident
        images, any h, w >= 1. order 'bgr' / 'rgb' (or FE_ORDER_*): the byte order of a pixel. -> stats float64 [n, 264] in input order,
        every double equal to image_stats's for that image. include/facet_engine.h fe_image_stats_mixed."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        stats = np.empty((n, FE_STATS_DOUBLES), np.float64)
        self._ck(self.lib.fe_image_stats_mixed(self.h, ptrs, self._hwp(hw), n, dev, self._order(order),
                                               stats.ctypes.data_as(C.POINTER(C.c_double))))
        return stats

    def set_stats_segment(self, pixels=0):
        """Pixels per segment of image_stats_mixed's first pass: 0 = the default, else a multiple of 4096 (>= 4096). The records do not
        depend on it."""
        self._ck(self.lib.fe_set_stats_segment(self.h, int(pixels)))

    def roi_laplacian(self, images, img_index, rois):
        """rois int [m,4] (x1,y1,x2,y2 exclusive, clipped) -> float64 [m,4]: sum lap, sum lap^2, sum gray, pixel count."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        idx = np.ascontiguousarray(img_index, dtype=np.int32)
        r = np.ascontiguousarray(rois, dtype=np.int32).reshape(-1, 4)
        out = np.zeros((idx.shape[0], 4), np.float64)
        self._ck(self.lib.fe_roi_laplacian(self.h, p, n, h, w, dev, idx.shape[0], idx.ctypes.data_as(C.POINTER(C.c_int)),
                                           r.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def swap_rb(self, src, pixels, dst_device):
        """dst_device (device pointer) <- src (host uint8 array or device pointer) with R and B exchanged, `pixels` 3-byte pixels."""
        if isinstance(src, np.ndarray):
            a = np.ascontiguousarray(src, dtype=np.uint8)
            assert a.size == pixels * 3
            self._ck(self.lib.fe_swap_rb_u8(self.h, a.ctypes.data_as(C.c_void_p), 0, pixels, dst_device))
        else:
            self._ck(self.lib.fe_swap_rb_u8(self.h, src, 1, pixels, dst_device))

    def leading_lines(self, images, canny_low=50, canny_high=150, threshold=80, min_line_length=None, max_line_gap=20, max_lines=2048,
                      want_edges=False):
        """BGR uint8 batch -> list of int32 [k,4] segment arrays (x1,y1,x2,y2; what cv2.HoughLinesP(cv2.Canny(cv2.GaussianBlur(gray,
        (5,5), 0), low, high), 1, pi/180, threshold, minLineLength, maxLineGap) returns per image, in the order found), and the
        Canny edge images uint8 [n,h,w] when want_edges. min_line_length defaults to int(min(h, w) * 0.15) (composition.py:219)."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        if min_line_length is None:
            min_line_length = int(min(h, w) * 0.15)
        edges = np.empty((n, h, w), np.uint8) if want_edges else None
        while True:
            lines = np.zeros((n, max_lines, 4), np.int32)
            counts = np.zeros(n, np.int32)
            self._ck(self.lib.fe_leading_lines(self.h, p, n, h, w, dev, canny_low, canny_high, threshold, min_line_length, max_line_gap, max_lines,
                                               lines.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                               edges.ctypes.data_as(C.c_void_p) if want_edges else None))
            if int(counts.max()) <= max_lines:
                break
            max_lines = int(counts.max())          # rare: more segments than room - run again with enough
        out = [lines[i, :counts[i]].copy() for i in range(n)]
        return (out, edges) if want_edges else out

    def external_contours(self, binary, min_twice_area=0, max_contours=256):
        """binary: uint8 [n,h,w] (host array, nonzero = foreground) or (device_ptr, n, h, w) -> list of int64 [k,8] record arrays, one per
        image: start_index, a00, a10, a01, x_min, y_min, x_max, y_max of every external contour (cv2.findContours RETR_EXTERNAL) with
        |a00| >= min_twice_area, in descending start_index order (include/facet_engine.h). Runs again with more room when an image has
        more than max_contours."""
        if isinstance(binary, tuple):
            p, n, h, w = binary
            dev, keep = 1, None
        else:
            keep = np.ascontiguousarray(binary, dtype=np.uint8)
            assert keep.ndim == 3, "expected [n,h,w]"
            (n, h, w), p, dev = keep.shape, keep.ctypes.data_as(C.c_void_p), 0
        return self._contour_call(lambda room, rec, cnt: self.lib.fe_external_contours(self.h, p, n, h, w, dev, int(min_twice_area), room, rec, cnt),
                                  n, max_contours)

    def _contour_call(self, call, n, max_contours):
        room = max(1, int(max_contours))
        for _ in range(2):
            rec = np.zeros((n, room, FE_CONTOUR_FIELDS), np.int64)
            counts = np.zeros(n, np.int32)
            self._ck(call(room, rec.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
            if int(counts.max()) <= room:
                return [rec[i, :counts[i]].copy() for i in range(n)]
            room = int(counts.max())
        raise EngineError(f"contours: {int(counts.max())} contours found after making room for {room}")

    def subject_contours(self, images, max_contours=256, want_edges=False, want_thresholds=False):
        """BGR uint8 [n,h,w,3] (or device tuple) -> list of int64 [k,8] record arrays (as external_contours) of the external contours of
        cv2.Canny(gray, 0.5 median, 1.5 median) whose area can pass the reference's `> h*w*0.0001` filter (fe_subject_region;
        facet_amd.composition.subject_box picks the subject). With want_edges / want_thresholds the return is
        (records, edges uint8 [n,h,w] | None, thresholds int32 [n,2] | None)."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        edges = np.empty((n, h, w), np.uint8) if want_edges else None
        thr = np.zeros((n, 2), np.int32) if want_thresholds else None
        out = self._contour_call(lambda room, rec, cnt: self.lib.fe_subject_region(
            self.h, p, n, h, w, dev, room, rec, cnt, thr.ctypes.data_as(C.c_void_p) if want_thresholds else None,
            edges.ctypes.data_as(C.c_void_p) if want_edges else None), n, max_contours)
        return (out, edges, thr) if (want_edges or want_thresholds) else out

    @staticmethod
    def _split_edges(flat, hw):
        """The flat edge buffer of a mixed-size call -> one [h, w] view per image."""
        ends = np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])
        return [flat[e - h * w:e].reshape(h, w) for e, (h, w) in zip(ends.tolist(), hw.tolist())]

    def leading_lines_mixed(self, images, order='bgr', canny_low=50, canny_high=150, threshold=80, min_line_length=None, max_line_gap=20,
                            max_lines=2048, want_edges=False):
        """leading_lines for images that each have their own size: a list of uint8 [h, w, 3] arrays, or (device_pointers, sizes) for
        resident images at any byte alignment. order 'bgr' / 'rgb' (or FE_ORDER_*): the byte order of a pixel. min_line_length: one
        value, one per image, or None = int(min(h, w) * 0.15) of each image. -> list of int32 [k,4] segment arrays in input order and, with
        want_edges, the list of uint8 [h,w] edge images; each equal to leading_lines's for that image alone. fe_leading_lines_mixed."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        if min_line_length is None:
            min_len = np.array([int(min(h, w) * 0.15) for h, w in hw.tolist()], np.int32)
        else:
            min_len = np.ascontiguousarray(np.broadcast_to(np.asarray(min_line_length, np.int32), (max(n, 0),)))
        flat = np.empty(int((hw[:, 0].astype(np.int64) * hw[:, 1]).clip(0).sum()) if n > 0 else 0, np.uint8) if want_edges else None
        while True:
            lines = np.zeros((max(n, 0), max_lines, 4), np.int32)
            counts = np.zeros(max(n, 0), np.int32)
            self._ck(self.lib.fe_leading_lines_mixed(self.h, ptrs, self._hwp(hw), n, dev, self._order(order), canny_low,
                                                     canny_high, threshold, min_len.ctypes.data_as(C.c_void_p), max_line_gap, max_lines,
                                                     lines.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                     flat.ctypes.data_as(C.c_void_p) if want_edges else None))
            if int(counts.max()) <= max_lines:
                break
            max_lines = int(counts.max())          # rare: more segments than room - run again with enough
        out = [lines[i, :counts[i]].copy() for i in range(n)]
        return (out, self._split_edges(flat, hw)) if want_edges else out

    def lines_host_ms(self):
        """Milliseconds the host stage (hysteresis + Hough) of this context's last leading_lines / leading_lines_mixed call took."""
        v = C.c_double(0.0)
        self._ck(self.lib.fe_lines_host_ms(self.h, C.byref(v)))
        return v.value

    def subject_contours_mixed(self, images, order='bgr', max_contours=256, want_edges=False, want_thresholds=False):
        """subject_contours for images that each have their own size: a list of uint8 [h, w, 3] arrays, or (device_pointers, sizes) for
        resident images at any byte alignment; order as above. -> list of int64 [k,8] record arrays in input order; with want_edges /
        want_thresholds (records, list of uint8 [h,w] edge images | None, thresholds int32 [n,2] | None). Every record, byte and threshold
        equals subject_contours's for that image alone; runs again with more room when an image has more than max_contours.
        fe_subject_region_mixed."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        flat = np.empty(int((hw[:, 0].astype(np.int64) * hw[:, 1]).clip(0).sum()) if n > 0 else 0, np.uint8) if want_edges else None
        thr = np.zeros((max(n, 0), 2), np.int32) if want_thresholds else None
        out = self._contour_call(lambda room, rec, cnt: self.lib.fe_subject_region_mixed(
            self.h, ptrs, self._hwp(hw), n, dev, self._order(order), room, rec, cnt,
            thr.ctypes.data_as(C.c_void_p) if want_thresholds else None, flat.ctypes.data_as(C.c_void_p) if want_edges else None), max(n, 0), max_contours)
        return (out, self._split_edges(flat, hw) if want_edges else None, thr) if (want_edges or want_thresholds) else out

    def phash(self, images, bgr=False, want_small=False, want_dct=False):
        """uint8 [n,h,w,3] (or device tuple), RGB or (bgr=True) BGR bytes -> uint64 [n]: imagehash.phash(pil_img) of every image as
        an integer (facet_amd.phash.to_hex gives the reference's strings). With want_small / want_dct the return is
        (hashes, small uint8 [n,32,32] | None, lo float64 [n,8,8] | None): the resized gray image and the low-frequency DCT block."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        hashes = np.empty((n,), np.uint64)
        small = np.empty((n, 32, 32), np.uint8) if want_small else None
        lo = np.empty((n, 8, 8), np.float64) if want_dct else None
        self._ck(self.lib.fe_phash(self.h, p, n, h, w, 1 if bgr else 0, dev, hashes.ctypes.data_as(C.c_void_p),
                                   small.ctypes.data_as(C.c_void_p) if want_small else None,
                                   lo.ctypes.data_as(C.c_void_p) if want_dct else None))
        return (hashes, small, lo) if (want_small or want_dct) else hashes

    def phash_mixed(self, images, order='rgb', want_small=False, want_dct=False):
        """phash for images that each have their own size: a list of uint8 [h, w, 3] arrays, or (device_pointers, sizes) for resident
        images. order 'rgb' / 'bgr' (or FE_ORDER_*): the byte order of a pixel. -> uint64 [n] in input order, every hash (and, with
        want_small / want_dct, every byte and double of `small` and `lo`) equal to phash's for that image alone. Nothing is cached per
        size. include/facet_engine.h fe_phash_mixed."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        hashes = np.empty((n,), np.uint64)
        small = np.empty((n, 32, 32), np.uint8) if want_small else None
        lo = np.empty((n, 8, 8), np.float64) if want_dct else None
        self._ck(self.lib.fe_phash_mixed(self.h, ptrs, self._hwp(hw), n, dev, self._order(order), hashes.ctypes.data_as(C.c_void_p),
                                         small.ctypes.data_as(C.c_void_p) if want_small else None,
                                         lo.ctypes.data_as(C.c_void_p) if want_dct else None))
        return (hashes, small, lo) if (want_small or want_dct) else hashes

    def resize_cache_entries(self):
        """How many per-size resampling tables the context holds (fe_resize_cache_entries): phash / thumbnail_jpeg / resize calls add to
        it with every new size, the mixed-size calls never do."""
        v = C.c_int32(0)
        self._ck(self.lib.fe_resize_cache_entries(self.h, C.byref(v)))
        return v.value

    def resize_u8_box(self, imgs, oh, ow, box, filter="lanczos"):
        """PIL `resize((ow, oh), filter, box)` of a uint8 [n,h,w,3] batch; box = (x0, y0, x1, y1) in source pixels, fractional."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        n, h, w, _ = a.shape
        b = np.asarray(box, dtype=np.float32).reshape(4)
        out = np.empty((n, oh, ow, 3), np.uint8)
        self._ck(self.lib.fe_resize_u8_box(self.h, a.ctypes.data_as(C.c_void_p), n, h, w, oh, ow, FILTERS[filter], b.ctypes.data_as(C.c_void_p), 0,
                                           out.ctypes.data_as(C.c_void_p)))
        return out

    def reduce_u8(self, imgs, factor, box=None):
        """PIL `reduce(factor, box)` of a uint8 [n,h,w,3] batch: factor an int or (fx, fy), box (x0, y0, x1, y1) in pixels."""
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        n, h, w, _ = a.shape
        fx, fy = (factor, factor) if isinstance(factor, int) else factor
        b = np.asarray(box if box is not None else (0, 0, w, h), dtype=np.int32).reshape(4)
        out = np.empty((n, -(-int(b[3] - b[1]) // fy), -(-int(b[2] - b[0]) // fx), 3), np.uint8)
        self._ck(self.lib.fe_reduce_u8(self.h, a.ctypes.data_as(C.c_void_p), n, h, w, fx, fy, b.ctypes.data_as(C.c_void_p), 0, out.ctypes.data_as(C.c_void_p)))
        return out

    def jpeg_bound(self, h, w):
        """Bytes that no JPEG of an h x w image exceeds (fe_jpeg_bound)."""
        return int(self.lib.fe_jpeg_bound(int(h), int(w)))

    @staticmethod
    def _jpeg_rows(out, lengths):
        return [out[i, :int(lengths[i])].tobytes() for i in range(out.shape[0])]

    def jpeg_encode(self, images, quality=80, bgr=False, cap=None):
        """uint8 [n,h,w,3] (or device tuple), RGB or (bgr=True) BGR bytes -> list of bytes: what PIL `save(buf, "JPEG", quality=quality)`
        writes for each image. cap: bytes of room per image (default: fe_jpeg_bound, which always fits; less raises EngineCapacityError
        when an image needs more)."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        cap = self.jpeg_bound(h, w) if cap is None else int(cap)
        out = np.empty((n, cap), np.uint8)
        lengths = np.zeros(n, np.int32)
        self._ck(self.lib.fe_jpeg_encode(self.h, p, n, h, w, 1 if bgr else 0, dev, int(quality), out.ctypes.data_as(C.c_void_p), cap,
                                         lengths.ctypes.data_as(C.c_void_p)))
        return self._jpeg_rows(out, lengths)

    def thumbnail_jpeg(self, images, plan, quality=80, bgr=False):
        """uint8 [n,h,w,3] (or device tuple) -> list of bytes: the reference's generate_photo_thumbnail of each image; plan =
        facet_amd.thumbnail.thumbnail_plan(w, h, size). Reduce, resize and encode run back to back on the device."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        if (plan.src_w, plan.src_h) != (w, h):
            raise ValueError(f"thumbnail_jpeg: the plan is for {plan.src_w} x {plan.src_h} images, these are {w} x {h}")
        ow, oh = plan.size
        fx, fy = plan.factors
        rbox = np.asarray(plan.reduce_box, dtype=np.int32).reshape(4) if plan.reduce_box is not None else None
        box = np.asarray(plan.resize_box, dtype=np.float32).reshape(4)
        cap = self.jpeg_bound(oh, ow)
        out = np.empty((n, cap), np.uint8)
        lengths = np.zeros(n, np.int32)
        self._ck(self.lib.fe_thumbnail_jpeg(self.h, p, n, h, w, 1 if bgr else 0, dev, oh, ow, fx, fy,
                                            rbox.ctypes.data_as(C.c_void_p) if rbox is not None else None, box.ctypes.data_as(C.c_void_p),
                                            1 if plan.tall else 0, int(quality), out.ctypes.data_as(C.c_void_p), cap, lengths.ctypes.data_as(C.c_void_p)))
        return self._jpeg_rows(out, lengths)

    @staticmethod
    def thumb_plans(plans, sizes):
        """ThumbnailPlan tuples (facet_amd.thumbnail.thumbnail_plan) of images of the given (h, w) sizes -> the fe_thumb_plan array
        (numpy, THUMB_PLAN_DTYPE) fe_thumbnail_jpeg_mixed takes."""
        arr = np.zeros(len(plans), THUMB_PLAN_DTYPE)
        for i, (p, (h, w)) in enumerate(zip(plans, sizes)):
            if (p.src_w, p.src_h) != (int(w), int(h)):
                raise ValueError(f"thumbnail_jpeg_mixed: plan {i} is for a {p.src_w} x {p.src_h} image, image {i} is {w} x {h}")
            arr[i] = (p.size[1], p.size[0], p.factors[0], p.factors[1], p.reduce_box if p.reduce_box is not None else (0, 0, 0, 0), p.resize_box,
                      1 if p.tall else 0)
        return arr

    def thumbnail_jpeg_mixed(self, images, plans, quality=80, order='rgb', cap=None):
        """thumbnail_jpeg for images that each have their own size: a list of uint8 [h, w, 3] arrays, or (device_pointers, sizes) for
        resident images, and one plan per image (facet_amd.thumbnail.thumbnail_plan(w, h, size)). order 'rgb' / 'bgr' (or FE_ORDER_*).
        -> list of bytes in input order, each what thumbnail_jpeg writes for that image alone. Nothing is cached per size. cap: bytes of
        room per image (default: fe_jpeg_bound of the largest thumbnail, which always fits); when an image needs more the
        EngineCapacityError carries `lengths` (int32 [n]: bytes written, or minus the bytes needed) and `rows` (bytes, or None for an image
        that did not fit). include/facet_engine.h fe_thumbnail_jpeg_mixed."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        if len(plans) != n:
            raise ValueError(f"thumbnail_jpeg_mixed: {len(plans)} plans for {n} images")
        arr = self.thumb_plans(plans, hw)
        if cap is None:
            cap = self.jpeg_bound(max(int(arr['oh'].max()), 1), max(int(arr['ow'].max()), 1)) if n else 1
        cap = int(cap)
        out = np.empty((n, cap), np.uint8)
        lengths = np.zeros(n, np.int32)
        try:
            self._ck(self.lib.fe_thumbnail_jpeg_mixed(self.h, ptrs, self._hwp(hw), n, dev, self._order(order), arr.ctypes.data_as(C.c_void_p),
                                                      int(quality), out.ctypes.data_as(C.c_void_p), cap, lengths.ctypes.data_as(C.c_void_p)))
        except EngineCapacityError as err:
            err.lengths = lengths
            err.rows = [out[i, :int(l)].tobytes() if 0 < l <= cap else None for i, l in enumerate(lengths)]
            raise
        return self._jpeg_rows(out, lengths)

    def jpeg_thumbnail(self, blobs, scale, plan, quality=80, progressive=False, cap=None, parallel_entropy=False):
        """JPEG files (a list of bytes) of one size -> (list of bytes, status int32 [n]): what `Image.open(f)`,
        `thumbnail((size, size), LANCZOS)`, `save(buf, "JPEG", quality=quality)` writes for each, with (scale, plan) =
        facet_amd.thumbnail.thumbnail_plan_jpeg(W, H, size) (fe_jpeg_thumbnail). Scaled decode, reduce, resize and encode run back to back
        on the device. A file with a non-zero status (jpeg_decode's codes) gives b"". cap as in jpeg_encode, against the plan's size.
        parallel_entropy: as in jpeg_decode; the bytes do not depend on it."""
        if scale not in (1, 2, 4, 8):
            raise ValueError(f"jpeg_thumbnail: scale {scale!r} (1, 2, 4 or 8)")
        blobs = [bytes(b) for b in blobs]
        n = len(blobs)
        if n == 0:
            return [], np.zeros(0, np.int32)
        ptrs = (C.c_char_p * n)(*blobs)
        lens = (C.c_size_t * n)(*[len(b) for b in blobs])
        ow, oh = plan.size
        fx, fy = plan.factors
        rbox = np.asarray(plan.reduce_box, dtype=np.int32).reshape(4) if plan.reduce_box is not None else None
        box = np.asarray(plan.resize_box, dtype=np.float32).reshape(4)
        cap = self.jpeg_bound(oh, ow) if cap is None else int(cap)
        out = np.empty((n, cap), np.uint8)
        lengths = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        self._ck(self.lib.fe_jpeg_thumbnail(self.h, ptrs, lens, n, int(plan.src_h), int(plan.src_w), int(scale),
                                            (FE_JPEG_PROGRESSIVE if progressive else 0) | (FE_JPEG_FLAG_PARALLEL if parallel_entropy else 0), oh, ow, fx, fy, rbox.ctypes.data_as(C.c_void_p) if rbox is not None else None,
                                            box.ctypes.data_as(C.c_void_p), 1 if plan.tall else 0, int(quality), out.ctypes.data_as(C.c_void_p), cap,
                                            lengths.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        return self._jpeg_rows(out, lengths), status

    def face_thumbnails(self, images, img_index, crops, out_sizes, quality=85, cap=None):
        """BGR uint8 [n,h,w,3] (or device tuple) -> list of bytes, one per face: crops int [m,4] (x0,y0,x1,y1 exclusive, inside the image,
        not empty) of images img_index [m], each resized to out_sizes [m,2] = (ow, oh) with PIL's BOX filter and saved as the JPEG
        `Image.fromarray(crop[:, :, ::-1]).resize((ow, oh), Image.BOX).save(buf, "JPEG", quality=quality)` writes (fe_face_thumbnails;
        facet_amd.face.face_thumbnail_plan gives the rectangle and size of a face box). cap as in jpeg_encode, against
        fe_jpeg_bound(max oh, max ow)."""
        p, n, h, w, dev, keep = self._img_ptr(images)
        idx = np.ascontiguousarray(img_index, dtype=np.int32).reshape(-1)
        m = idx.shape[0]
        if m == 0:
            return []
        r = np.ascontiguousarray(crops, dtype=np.int32).reshape(m, 4)
        sz = np.ascontiguousarray(out_sizes, dtype=np.int32).reshape(m, 2)
        if cap is None:
            cap = self.jpeg_bound(max(1, int(sz[:, 1].max())), max(1, int(sz[:, 0].max())))
        cap = int(cap)
        out = np.empty((m, cap), np.uint8)
        lengths = np.zeros(m, np.int32)
        self._ck(self.lib.fe_face_thumbnails(self.h, p, n, h, w, dev, m, idx.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                                             sz.ctypes.data_as(C.c_void_p), int(quality), out.ctypes.data_as(C.c_void_p), cap,
                                             lengths.ctypes.data_as(C.c_void_p)))
        return self._jpeg_rows(out, lengths)

    def face_thumbnails_mixed(self, images, img_index, crops, out_sizes, quality=85, cap=None, order='bgr'):
        """face_thumbnails with img_index into a list of images of any sizes (a list of uint8 [h, w, 3] arrays, or (device_pointers,
        sizes)); order 'bgr' / 'rgb': the byte order of a pixel. The bytes are face_thumbnails' for each image alone."""
        ptrs, hw, n, dev, keep = self._img_list(images)
        idx = np.ascontiguousarray(img_index, dtype=np.int32).reshape(-1)
        m = idx.shape[0]
        if m == 0:
            return []
        r = np.ascontiguousarray(crops, dtype=np.int32).reshape(m, 4)
        sz = np.ascontiguousarray(out_sizes, dtype=np.int32).reshape(m, 2)
        if cap is None:
            cap = self.jpeg_bound(max(1, int(sz[:, 1].max())), max(1, int(sz[:, 0].max())))
        cap = int(cap)
        out = np.empty((m, cap), np.uint8)
        lengths = np.zeros(m, np.int32)
        self._ck(self.lib.fe_face_thumbnails_mixed(self.h, ptrs, self._hwp(hw), n, dev, self._order(order), m,
                                                   idx.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), sz.ctypes.data_as(C.c_void_p), int(quality),
                                                   out.ctypes.data_as(C.c_void_p), cap, lengths.ctypes.data_as(C.c_void_p)))
        return self._jpeg_rows(out, lengths)

    @staticmethod
    def jpeg_probe(blob, progressive=False):
        """The markers of one JPEG file (bytes) -> dict(width, height, components, hsamp, vsamp, restart_interval, orientation, status);
        status 0: jpeg_decode takes the file, > 0: a kind it leaves to Pillow, < 0: corrupt (JPEG_STATUS names them). Host only.
        progressive=True (fe_jpeg_probe_ex): the answer for jpeg_decode(..., progressive=True), where a complete progressive file is 0
        too; the dict gains `progressive` (the frame is SOF2) and `scans`."""
        blob = bytes(blob)
        if progressive:
            info = (C.c_int32 * 10)()
            rc = load_library().fe_jpeg_probe_ex(blob, len(blob), FE_JPEG_PROGRESSIVE, info)
            if rc != 0:
                raise EngineError("fe_jpeg_probe_ex failed")
            return dict(zip(("width", "height", "components", "hsamp", "vsamp", "restart_interval", "orientation", "status", "progressive", "scans"),
                            (int(v) for v in info)))
        info = (C.c_int32 * 8)()
        rc = load_library().fe_jpeg_probe(blob, len(blob), info)
        if rc != 0:
            raise EngineError("fe_jpeg_probe failed")
        return dict(zip(("width", "height", "components", "hsamp", "vsamp", "restart_interval", "orientation", "status"), (int(v) for v in info)))

    @staticmethod
    def jpeg_scaled_size(h, w, scale):
        """(h, w) of an H x W file decoded at 1/scale: ceil(H / scale), ceil(W / scale) (fe_jpeg_scaled_size). Host only."""
        sh, sw = C.c_int32(), C.c_int32()
        if load_library().fe_jpeg_scaled_size(int(h), int(w), int(scale), C.byref(sh), C.byref(sw)) != 0:
            raise ValueError(f"jpeg_scaled_size: {h} x {w} at scale {scale} (a positive size; scale 1, 2, 4 or 8)")
        return sh.value, sw.value

    def jpeg_entropy_stats(self):
        """What the entropy stage of this engine's last jpeg_decode / jpeg_thumbnail call did (fe_jpeg_entropy_stats): dict(
        parallel_segments, subsequences, max_rounds, redone) = segments decoded by one lane per subsequence, those subsequences, the most
        rounds any segment needed to settle its entry states, images decoded again by the serial kernel after an error. All zero for
        a call without parallel_entropy."""
        out = (C.c_int32 * 4)()
        self._ck(self.lib.fe_jpeg_entropy_stats(self.h, out))
        return dict(zip(("parallel_segments", "subsequences", "max_rounds", "redone"), (int(v) for v in out)))

    def jpeg_decode(self, blobs, h, w, bgr=False, apply_orientation=True, device=False, progressive=False, scale=1, parallel_entropy=False):
        """JPEG files (a list of bytes) whose decoded size is h x w -> (pixels, status). pixels: uint8 [n,h,w,3], what Pillow's
        `ImageOps.exif_transpose(Image.open(f)).convert('RGB')` gives (apply_orientation=False: without the transpose; bgr: B,G,R bytes),
        a host array, or with device=True a (device_ptr, n, h, w) tuple whose buffer the caller releases with dev_free (device=<pointer>
        decodes into the caller's own buffer). status: int32 [n], 0 where the image was decoded; the slot of any other image is left as it
        was (zeros in a host array allocated here, undefined in a device buffer allocated here). progressive=True (fe_jpeg_decode_ex):
        progressive files that jpeg_probe(blob, progressive=True) gives status 0 are decoded too, in the same call as baseline ones.
        scale = 2, 4 or 8 (fe_jpeg_decode_scaled): the decode at 1/scale that `im.draft()` switches on, the pixels of the drafted image;
        h, w are then the scaled size, jpeg_scaled_size(H, W, scale), exchanged for orientations 5 .. 8 like the full size.
        parallel_entropy=True (FE_JPEG_FLAG_PARALLEL): a baseline file's entropy-coded segments of at least 256 bytes are decoded by one
        lane per 128 bytes instead of one lane per segment, which is what a file without restart markers needs; pixels and statuses do
        not depend on it, and jpeg_entropy_stats() tells what it did."""
        if scale not in (1, 2, 4, 8):
            raise ValueError(f"jpeg_decode: scale {scale!r} (1, 2, 4 or 8)")
        blobs = [bytes(b) for b in blobs]
        n = len(blobs)
        if n == 0:
            raise ValueError("jpeg_decode: no files")
        ptrs = (C.c_char_p * n)(*blobs)
        lens = (C.c_size_t * n)(*[len(b) for b in blobs])
        status = np.zeros(n, np.int32)
        flags = (FE_JPEG_PROGRESSIVE if progressive else 0) | (FE_JPEG_FLAG_PARALLEL if parallel_entropy else 0)
        def call(on_device, dst):
            head = (self.h, ptrs, lens, n, int(h), int(w), 1 if bgr else 0, 1 if apply_orientation else 0, on_device)
            if scale != 1:
                self._ck(self.lib.fe_jpeg_decode_scaled(self.h, ptrs, lens, n, int(h), int(w), int(scale), *head[6:], flags, dst,
                                                        status.ctypes.data_as(C.c_void_p)))
            elif flags:
                self._ck(self.lib.fe_jpeg_decode_ex(*head, flags, dst, status.ctypes.data_as(C.c_void_p)))
            else:
                self._ck(self.lib.fe_jpeg_decode(*head, dst, status.ctypes.data_as(C.c_void_p)))
        if device is False or device is None:
            out = np.zeros((n, h, w, 3), np.uint8)
            call(0, out.ctypes.data_as(C.c_void_p))
            return out, status
        own = device is True
        d = self.dev_alloc(n * h * w * 3) if own else device
        try:
            call(1, d)
        except Exception:
            if own:
                self.dev_free(d)
            raise
        return (d, n, h, w), status

    def hamming_pairs(self, hashes, max_distance, max_pairs=None):
        """hashes: uint64 [n] (host array) or (device_ptr, n). -> int32 [k,2]: every i < j whose hashes differ in at most
        max_distance bits, in ascending (i, j) order. max_pairs: room for the first attempt (default max(1024, 4 n)); when there
        are more, the call is repeated once with exactly enough."""
        if isinstance(hashes, tuple):
            p, n = hashes
            dev, keep = 1, None
        else:
            keep = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1)
            p, n, dev = keep.ctypes.data_as(C.c_void_p), keep.shape[0], 0
        room = int(max_pairs) if max_pairs is not None else max(1024, 4 * n)
        count = C.c_int64(0)
        for _ in range(2):
            pairs = np.empty((room, 2), np.int32)
            self._ck(self.lib.fe_hamming_pairs(self.h, p, n, dev, int(max_distance), room, pairs.ctypes.data_as(C.c_void_p) if room else None,
                                               C.byref(count)))
            if count.value <= room:
                return pairs[:count.value].copy()
            room = count.value
        raise EngineError(f"hamming_pairs: {count.value} pairs found after making room for {room}")

    def burst_links(self, hashes, times, flags, thr, window_s, rapid_s, person_off=None, person_ids=None):
        """Rows in the reference's burst order. hashes: uint64 [n] (host array) or (device_ptr, n); times: int64 [n] seconds; flags:
        uint8 [n] of FE_BURST_HAS_HASH | FE_BURST_HAS_DATE; person_off int32 [n+1] / person_ids int32: CSR lists, ascending and distinct
        per row, or both None; thr / window_s / rapid_s: the settings floored to integers (facet_amd.bursts.burst_settings).
        -> int32 [n]: per row the largest earlier row it is similar to, or -1 (fe_burst_links)."""
        if isinstance(hashes, tuple):
            p, n = hashes
            dev, keep = 1, None
        else:
            keep = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1)
            p, n, dev = keep.ctypes.data_as(C.c_void_p), keep.shape[0], 0
        n = int(n)
        t = np.ascontiguousarray(times, dtype=np.int64).reshape(-1)
        f = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        if t.shape[0] != n or f.shape[0] != n:
            raise ValueError(f"burst_links: {n} hashes, {t.shape[0]} times, {f.shape[0]} flags")
        if (person_off is None) != (person_ids is None):
            raise ValueError("burst_links: person_off and person_ids go together")
        off = ids = None
        if person_off is not None:
            off = np.ascontiguousarray(person_off, dtype=np.int32).reshape(-1)
            ids = np.ascontiguousarray(person_ids, dtype=np.int32).reshape(-1)
            if off.shape[0] != n + 1:
                raise ValueError(f"burst_links: person_off has {off.shape[0]} entries for {n} rows")
        n_ids = 0 if ids is None else ids.shape[0]
        if ids is not None and n_ids == 0:
            ids = np.zeros(1, np.int32)                            # a pointer that is not null; none of it is read
        lim = (1 << 63) - 1
        clamp = lambda v, m: max(-m - 1, min(int(v), m))          # whatever the settings gave, as a C integer
        link = np.empty(n, np.int32)
        self._ck(self.lib.fe_burst_links(self.h, p, dev, t.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), n,
                                         off.ctypes.data_as(C.c_void_p) if off is not None else None,
                                         ids.ctypes.data_as(C.c_void_p) if ids is not None else None, n_ids,
                                         clamp(thr, (1 << 31) - 1), clamp(window_s, lim), clamp(rapid_s, lim), link.ctypes.data_as(C.c_void_p)))
        return link

    @staticmethod
    def _rows_ptr(x):
        """x: float32 [n,d] (host array) or (device_ptr, n, d)."""
        if isinstance(x, tuple):
            p, n, d = x
            return p, int(n), int(d), 1, None
        a = np.ascontiguousarray(x, dtype=np.float32)
        assert a.ndim == 2
        return a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1], 0, a

    def core_distances(self, x, k, normalise=True):
        """x: float32 [n,d] (or device tuple) -> (core float64 [n], core_idx int32 [n]): distance to, and index of, the k-th nearest
        row, the row itself counting as the first (HDBSCAN's min_samples). Rows are L2-normalised first unless normalise=False."""
        p, n, d, dev, keep = self._rows_ptr(x)
        core = np.empty((n,), np.float64)
        idx = np.empty((n,), np.int32)
        self._ck(self.lib.fe_knn_core_distances(self.h, p, n, d, dev, 1 if normalise else 0, int(k), core.ctypes.data_as(C.c_void_p),
                                                idx.ctypes.data_as(C.c_void_p)))
        return core, idx

    def mreach_mst(self, x, k, normalise=True):
        """x: float32 [n,d] (or device tuple) -> (edge_u int32 [n-1], edge_v int32 [n-1], edge_w float64 [n-1], core float64 [n],
        rounds): the minimum spanning tree of the mutual-reachability graph max(core_u, core_v, |x_u - x_v|) with k = min_samples."""
        p, n, d, dev, keep = self._rows_ptr(x)
        m = max(n - 1, 0)
        eu, ev = np.empty((m,), np.int32), np.empty((m,), np.int32)
        ew = np.empty((m,), np.float64)
        core = np.empty((n,), np.float64)
        rounds = C.c_int32(0)
        self._ck(self.lib.fe_mreach_mst(self.h, p, n, d, dev, 1 if normalise else 0, int(k), eu.ctypes.data_as(C.c_void_p),
                                        ev.ctypes.data_as(C.c_void_p), ew.ctypes.data_as(C.c_void_p), core.ctypes.data_as(C.c_void_p),
                                        C.cast(C.byref(rounds), C.c_void_p)))
        return eu, ev, ew, core, int(rounds.value)

    def cosine_best_match(self, queries, candidates):
        """float32 [nq,d], [nc,d] (host) -> (best_sim float32 [nq], best_idx int32 [nq]): for every query the candidate of largest
        cosine similarity, the first among equals. Both sides are L2-normalised inside."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        c = np.ascontiguousarray(candidates, dtype=np.float32)
        assert q.ndim == 2 and c.ndim == 2 and q.shape[1] == c.shape[1]
        sim = np.empty((q.shape[0],), np.float32)
        idx = np.empty((q.shape[0],), np.int32)
        self._ck(self.lib.fe_cosine_best_match(self.h, q.ctypes.data_as(C.c_void_p), q.shape[0], c.ctypes.data_as(C.c_void_p), c.shape[0],
                                               q.shape[1], sim.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)))
        return sim, idx

    # -- similar photos / merge suggestions --------------------------------------------------
    @staticmethod
    def _sim_rows(x):
        return x if isinstance(x, SimRows) else SimRows(x)

    def upload_sim_rows(self, rows):
        """SimRows on the host -> the same rows resident on this engine's GPU (torch owns the memory; the result keeps it alive).
        Upload a library once and pass the result to any number of similar_topk / similar_pairs calls."""
        import torch
        rows = self._sim_rows(rows)
        if rows.on_device:
            return rows
        dev = torch.device("cuda", int(self.device))
        keep = {"emb": torch.from_numpy(rows.emb).to(dev)}
        for name, _ in SimRows.FIELDS:
            v = getattr(rows, name)
            if v is not None and v.shape[0]:
                keep[name] = torch.from_numpy(v).to(dev)
        torch.cuda.synchronize(dev)
        p = {k: t.data_ptr() for k, t in keep.items()}
        has_ids = "person_ids" in p
        out = SimRows((p["emb"], rows.n, rows.d), p.get("has_emb"), p.get("date"), p.get("aggregate"), p.get("person_off") if has_ids else None,
                      (p["person_ids"], rows.n_person_ids) if has_ids else None, normalise=rows.normalise)
        out.keep = keep
        return out

    def _sim_args(self, queries, candidates, weights, cosine, q_self, visible):
        q, c = self._sim_rows(queries), self._sim_rows(candidates)
        if q.d != c.d:
            raise ValueError(f"queries have d = {q.d}, candidates d = {c.d}")
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if w.shape[0] != 4:
            raise ValueError("weights = (clip, person, date, score)")
        qs = None if q_self is None else np.ascontiguousarray(q_self, dtype=np.int32).reshape(-1)
        vis = None if visible is None else np.ascontiguousarray(visible, dtype=np.uint8).reshape(-1)
        if qs is not None and qs.shape[0] != q.n:
            raise ValueError("q_self: one entry per query")
        if vis is not None and vis.shape[0] != c.n:
            raise ValueError("visible: one entry per candidate")
        qc, cc = q.c_struct(), (None if candidates is queries else c.c_struct())
        cc = qc if cc is None else cc
        head = (self.h, C.cast(C.byref(qc), C.c_void_p), C.cast(C.byref(cc), C.c_void_p), q.d, FE_SIM_COSINE if cosine else FE_SIM_FUSED,
                w.ctypes.data_as(C.c_void_p), None if qs is None else qs.ctypes.data_as(C.c_void_p),
                None if vis is None else vis.ctypes.data_as(C.c_void_p))
        return q, c, head, (q, c, qc, cc, w, qs, vis)

    def similar_topk(self, queries, candidates, k, weights=(0.4, 0.3, 0.2, 0.1), cosine=False, q_self=None, visible=None):
        """queries / candidates: SimRows (host or resident), or plain float32 [n,d] rows / (device_ptr, n, d). -> (idx int32 [nq,k],
        score float32 [nq,k]): per query the k best candidates by the fused "similar photos" score (or the plain cosine), score
        descending, candidate index ascending among equals, -1 / 0 padded. q_self int [nq]: the candidate index of the query itself
        (-1: none), visible uint8 [n]: candidates with 0 are skipped. 1 <= k <= FE_SIM_K_MAX."""
        q, c, head, keep = self._sim_args(queries, candidates, weights, cosine, q_self, visible)
        idx = np.empty((q.n, int(k)), np.int32)
        score = np.empty((q.n, int(k)), np.float32)
        self._ck(self.lib.fe_similar_topk(*head, int(k), idx.ctypes.data_as(C.c_void_p), score.ctypes.data_as(C.c_void_p)))
        return idx, score

    def similar_pairs(self, queries, candidates, thr, weights=(0.4, 0.3, 0.2, 0.1), cosine=False, q_self=None, visible=None, upper=False,
                      max_pairs=None):
        """-> (pairs int32 [m,2] = (query, candidate), score float32 [m]) in ascending (query, candidate) order: every pair whose
        score is >= thr (one value, or one per query); upper=True (queries is candidates): candidate > query only. max_pairs: room
        for the first attempt (default max(1024, 4 (nq + n))); when there are more the call is repeated once with exactly enough."""
        q, c, head, keep = self._sim_args(queries, candidates, weights, cosine, q_self, visible)
        t = np.ascontiguousarray(thr, dtype=np.float32).reshape(-1)
        room = int(max_pairs) if max_pairs is not None else max(1024, 4 * (q.n + c.n))
        count = C.c_int64(0)
        for _ in range(2):
            pairs = np.empty((room, 2), np.int32)
            score = np.empty((room,), np.float32)
            self._ck(self.lib.fe_similar_pairs(*head, t.ctypes.data_as(C.c_void_p), t.shape[0], 1 if upper else 0, room,
                                               pairs.ctypes.data_as(C.c_void_p) if room else None,
                                               score.ctypes.data_as(C.c_void_p) if room else None, C.byref(count)))
            if count.value <= room:
                return pairs[:count.value].copy(), score[:count.value].copy()
            room = count.value
        raise EngineError(f"similar_pairs: {count.value} pairs found after making room for {room}")

    def similar_pairs_count(self, queries, candidates, thr, **kw):
        """The exact number of pairs similar_pairs would return, without fetching them."""
        q, c, head, keep = self._sim_args(queries, candidates, kw.get("weights", (0.4, 0.3, 0.2, 0.1)), kw.get("cosine", False), kw.get("q_self"),
                                          kw.get("visible"))
        t = np.ascontiguousarray(thr, dtype=np.float32).reshape(-1)
        count = C.c_int64(0)
        self._ck(self.lib.fe_similar_pairs(*head, t.ctypes.data_as(C.c_void_p), t.shape[0], 1 if kw.get("upper") else 0, 0, None, None,
                                           C.byref(count)))
        return int(count.value)

    def cv_resize_linear(self, imgs, oh, ow):
        a = np.ascontiguousarray(imgs, dtype=np.uint8)
        n, h, w, _ = a.shape
        out = np.empty((n, oh, ow, 3), np.uint8)
        self._ck(self.lib.fe_cv_resize_linear_u8(self.h, a.ctypes.data_as(C.c_void_p), n, h, w, oh, ow, out.ctypes.data_as(C.c_void_p)))
        return out

    def tag_similarities(self, emb, text):
        """emb [n,d], text [T,d] (L2-normalised rows) -> cosine similarities [n,T] computed on the GPU."""
        emb, ep = _f32(emb)
        text, tp = _f32(text)
        n, d = emb.shape
        T = text.shape[0]
        out = np.empty((n, T), np.float32)
        self._ck(self.lib.fe_tag_similarities(self.h, ep, n, tp, T, d, out.ctypes.data_as(_f32p)))
        return out

    def tag_vocab(self, text, tag_of_prompt):
        """The context's tag vocabulary (fe_tag_vocab_set): text float32 [T,d] (L2-normalised rows), tag_of_prompt int [T] with the tag
        id of every prompt - ids 0 .. G-1, all used, first appearing in ascending order. Packed once; a second call replaces it;
        text=None clears it. -> G."""
        if text is None:
            self._ck(self.lib.fe_tag_vocab_set(self.h, None, 0, 0, None, 0))
            self._tag_dims = None
            return 0
        t = np.ascontiguousarray(text, dtype=np.float32)
        ids = np.ascontiguousarray(tag_of_prompt, dtype=np.int32).reshape(-1)
        if t.ndim != 2 or ids.shape[0] != t.shape[0]:
            raise ValueError(f"tag_vocab: text of shape {t.shape} with {ids.shape[0]} tag ids")
        G = int(ids.max()) + 1 if ids.size else 0
        self._ck(self.lib.fe_tag_vocab_set(self.h, t.ctypes.data_as(C.c_void_p), t.shape[0], t.shape[1], ids.ctypes.data_as(C.c_void_p), G))
        self._tag_dims = (t.shape[0], t.shape[1], G)
        return G

    def set_tag_chunk(self, rows=0):
        """Rows per chunk of tag_select / tag_select_sims: 0 = sized from the arena, else a positive count (the arena's size still caps it)."""
        self._ck(self.lib.fe_set_tag_chunk(self.h, int(rows)))

    def _tag_select(self, fn, who, x, width, threshold, max_tags):
        if isinstance(x, tuple):
            p, n, ld = x
            dev, keep = 1, None
        else:
            keep = np.ascontiguousarray(x, dtype=np.float32)
            if keep.ndim != 2 or (width is not None and keep.shape[1] != width):
                raise ValueError(f"{who}: rows of shape {keep.shape}, the vocabulary wants [n, {width}]")
            p, n, ld, dev = keep.ctypes.data_as(C.c_void_p), keep.shape[0], keep.shape[1], 0
        n, k = int(n), int(max_tags)
        ids = np.full((n, max(k, 0)), -1, np.int32)
        scores = np.zeros((n, max(k, 0)), np.float32)
        counts = np.zeros(n, np.int32)
        self._ck(fn(self.h, p, n, int(ld), dev, float(threshold), k, ids.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p),
                    counts.ctypes.data_as(C.c_void_p)))
        return ids, scores, counts

    def tag_select(self, emb, threshold, max_tags):
        """emb: float32 [n,d] (host array) or (device_ptr, n, ld) - n rows of d floats, ld floats apart, read in place (the ensemble
        record at column 21: (records_ptr + 84, n, 789)). -> ids int32 [n,max_tags] padded with -1, scores float32 [n,max_tags] padded
        with 0, counts int32 [n]: per row the reference's tag choice (per-tag max over the synonyms, float(score) >= threshold,
        descending score, ties by tag id, the first max_tags) on the vocabulary of tag_vocab (fe_tag_select)."""
        dims = getattr(self, "_tag_dims", None)
        return self._tag_select(self.lib.fe_tag_select, "tag_select", emb, dims[1] if dims else None, threshold, max_tags)

    def tag_select_sims(self, sims, threshold, max_tags):
        """The selection of tag_select alone on given similarities: float32 [n,T] (host array) or (device_ptr, n, ld) (fe_tag_select_sims)."""
        dims = getattr(self, "_tag_dims", None)
        return self._tag_select(self.lib.fe_tag_select_sims, "tag_select_sims", sims, dims[0] if dims else None, threshold, max_tags)

    def clip_encode_text(self, tokens, out_dim=768):
        """tokens: int [n, 77] -> un-normalised text features [n, 768]."""
        tk = np.ascontiguousarray(tokens, dtype=np.int32)
        n, L = tk.shape
        out = np.empty((n, out_dim), np.float32)
        self._ck(self.lib.fe_clip_encode_text(self.h, tk.ctypes.data_as(C.POINTER(C.c_int32)), n, L, out.ctypes.data_as(_f32p)))
        return out
