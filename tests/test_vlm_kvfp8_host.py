"""CPU: the e4m3 KV cache of the VLM decoders (Engine.vlm_kv_format) - the new entry points are exported, declared and bound; the
kv_format switch of VLMTagger / Qwen2VLModel against a stub engine; the golden file's own consistency
(tests/golden/make_vlm_kvfp8_golden.py: transformers' class over a cache that keeps dequantize(quantize(row)))."""
import ctypes
import os
import re

import numpy as np
import pytest

from facet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fe_vlm_set_kv_format", "fe_vlm_kv_info", "fe_vlm_kv_rows", "fe_op_vlm_decode_attention")


def test_new_symbols_are_exported_declared_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "facet_amd", "libfacet_engine.so"))
    header = open(os.path.join(ROOT, "include", "facet_engine.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in doc, name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"FE_VLM_KV_BF16\s*=\s*0\s*,\s*FE_VLM_KV_E4M3\s*=\s*1\s*,\s*FE_VLM_KV_BF16_E4M3\s*=\s*2", header)
    assert _lib.VLM_KV_FORMATS == {"bf16": 0, "fp8": 1, "bf16_e4m3": 2}
    for m in ("vlm_kv_format", "vlm_kv_info", "vlm_kv_rows", "vlm_decode_attention"):
        assert callable(getattr(_lib.Engine, m)), m


class _StubEngine:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, a))
        return f


@pytest.mark.parametrize("path,fmt", [("Qwen/Qwen2.5-VL-7B-Instruct", "fp8"), ("Qwen/Qwen3-VL-2B-Instruct", "bf16_e4m3"), ("Qwen/Qwen2.5-VL-7B-Instruct", None)])
def test_tagger_sets_the_kv_format_when_it_loads(path, fmt):
    from facet_amd.vlm_tagger import VLMTagger
    e = _StubEngine()
    cfg = dict(model_path=path, weight_format="fp8")          # independent of, and combinable with, the weight format
    if fmt:
        cfg["kv_format"] = fmt
    VLMTagger(cfg, engine=e).load(state_dict={})
    names = [c[0] for c in e.calls]
    assert e.calls[names.index("vlm_kv_format")][1] == (fmt or "bf16",)
    assert e.calls[names.index("vlm_weight_format")][1] == ("fp8",)


def test_unknown_kv_format_is_rejected():
    from facet_amd.model_manager import ModelManager  # noqa: F401  (the composition model's entry: imports with the package)
    from facet_amd.vlm_composition import Qwen2VLModel
    from facet_amd.vlm_tagger import VLMTagger
    with pytest.raises(ValueError, match="kv_format.*int4"):
        VLMTagger(dict(model_path="Qwen/Qwen2.5-VL-7B-Instruct", kv_format="int4"), engine=_StubEngine())
    with pytest.raises(ValueError, match="kv_format.*int4"):
        Qwen2VLModel(_StubEngine(), {}, kv_format="int4")
    e = _StubEngine()
    Qwen2VLModel(e, {}, weight_format="fp8", kv_format="fp8").to("cuda")
    names = [c[0] for c in e.calls]
    assert e.calls[names.index("vlm_kv_format")][1] == ("fp8",) and e.calls[names.index("vlm_weight_format")][1] == ("fp8",)
    assert Qwen2VLModel(_StubEngine(), {}).kv_format == "bf16"


def test_golden_is_consistent():
    g = np.load(os.path.join(ROOT, "tests", "golden", "vlm_kvfp8_golden.npz"))
    B, L, new = 2, 24, 40
    assert g["prompts"].shape == (B, L) and g["prompts"].dtype == np.int32 and g["tokens"].shape == (B, new)
    vocab = int(g["vocab"])
    assert g["logits_step0"].shape == (B, vocab) and g["logits_last"].shape == (B, vocab) and g["margin"].shape == (B, new)
    assert (g["prompts"] >= 0).all() and (g["prompts"] < vocab).all() and (g["tokens"] >= 0).all() and (g["tokens"] < vocab).all()
    # the stored tokens are the argmax of the stored logits, with the stored margins; the margins are decisive
    for lg, step in ((g["logits_step0"], 0), (g["logits_last"], new - 1)):
        assert np.array_equal(lg.argmax(-1), g["tokens"][:, step])
        t2 = np.sort(lg, -1)[:, -2:]
        assert np.array_equal((t2[:, 1] - t2[:, 0]).astype(np.float32), g["margin"][:, step])
        assert np.array_equal(lg.max(-1), g["top_logit"][:, step])
        bits = lg.view(np.uint32)
        assert not (bits & 0xFFFF).any()          # bf16 logits
    assert g["margin"].min() > 1.0
    assert float(g["plain_diff_max"]) > 0.0          # the format moved the logits of the plain-cache run
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vlm_kvfp8_golden.npz")) < 500 * 1024
