"""CPU: the e4m3 weight format of the VLM decoders (facet_amd/csrc/fp8_core.h), run by a stand-alone harness compiled under
AddressSanitizer + UBSan, against torch's float8_e4m3fn and against the format's own rule; facet_amd.weights.quantize_e4m3_rows against
the harness; VLMTagger's weight_format switch against a stub engine. Every comparison is exact."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from facet_amd.weights import dequantize_e4m3_rows, quantize_e4m3_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("fp8core") / "fp8_core_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "fp8_core_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode, tmp, payload=None):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    args = [exe, mode]
    if payload is not None:
        with open(fin, "wb") as f:
            f.write(payload)
        args.append(fin)
    r = subprocess.run(args + [fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]          # a sanitizer report ends the run with a status of its own
    return open(fout, "rb").read()


def _rows(exe, tmp, w):
    """harness quantiser on w [N, K] float32 -> (ok [N], exponents [N], codes [N, K], w' [N, K])"""
    w = np.ascontiguousarray(w, np.float32)
    N, K = w.shape
    raw = _run(exe, "rows", tmp, struct.pack("2i", N, K) + w.tobytes())
    rec = np.dtype([("ok", "<i4"), ("e", "<i4"), ("c", "u1", (K,)), ("w", "<f4", (K,))])
    a = np.frombuffer(raw, rec)
    assert a.shape == (N,)
    return a["ok"], a["e"], a["c"], a["w"]


def _bf16(x):
    return torch.from_numpy(np.array(x, np.float32)).to(torch.bfloat16).float().numpy()


def _torch_values():
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).float().numpy()


def test_decode_of_every_code_equals_torch(harness, tmp_path):
    got = np.frombuffer(_run(harness, "decode", str(tmp_path)), np.float32)
    want = _torch_values()
    assert got.shape == (256,)
    assert np.isnan(got[0x7F]) and np.isnan(got[0xFF]) and np.isnan(got).sum() == 2
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))          # bit for bit: -0 is -0
    assert np.array_equal(dequantize_e4m3_rows(np.arange(256, dtype=np.uint8)[None], [0])[0][ok].view(np.uint32), want[ok].view(np.uint32))


def _encode_cases():
    rng = np.random.default_rng(5)
    vals = _torch_values()
    fin = np.sort(vals[~np.isnan(vals)])
    mids = ((fin[1:].astype(np.float64) + fin[:-1]) / 2).astype(np.float32)          # every midpoint between neighbours (exact in fp32)
    parts = [fin, mids, np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)),
             np.array([0.0, -0.0, 448.0, -448.0, 2.0 ** -9, 2.0 ** -10, -2.0 ** -10, 2.0 ** -11, 1e-30, -1e-30, 1e-45], np.float32),
             rng.uniform(-2.0 ** -6, 2.0 ** -6, 8000).astype(np.float32)]          # the subnormal range
    n_rest = 100000 - sum(p.size for p in parts)
    for scale in (1e-3, 0.02, 0.5, 4.0, 60.0, 150.0):
        parts.append((rng.standard_normal(n_rest // 6 + 1) * scale).astype(np.float32))
    x = np.concatenate(parts)[:100000]
    return np.clip(x, -448.0, 448.0)


def test_encode_of_1e5_values_equals_torch(harness, tmp_path):
    x = _encode_cases()
    assert x.size == 100000 and np.abs(x).max() == 448.0
    got = np.frombuffer(_run(harness, "encode", str(tmp_path), x.tobytes()), np.uint8)
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:10]]


def _rule_rows():
    """(name, row, expected exponent) - rows of bf16 values, K = 64"""
    rng = np.random.default_rng(6)
    out = []
    for j in (-100, -20, -9, -1, 0, 3, 40, 100):
        top = np.float32(448.0 * 2.0 ** j)
        ulp = np.float32(2.0 ** (8 + j - 7))          # bf16 spacing at 448 * 2^j = 1.75 * 2^(8 + j)
        for name, a, e in (("at", top, j), ("above", top + ulp, j + 1), ("below", top - ulp, j)):
            row = _bf16(rng.uniform(-1, 1, 64) * float(a))
            row[rng.integers(64)] = a * (1 if j % 2 else -1)
            assert _bf16(row).tobytes() == row.tobytes() and np.abs(row).max() == a
            out.append((f"448*2^{j} {name}", row, e))
    out.append(("zero row", np.zeros(64, np.float32), 0))
    base = _bf16(rng.standard_normal(64) * 0.02)
    base[17] = _bf16(np.array([150.0 * np.abs(base).max()]))[0]
    out.append(("outlier 150x", base, int(np.ceil(np.log2(float(np.abs(base[17])) / 448.0)))))
    out.append(("1e-38", _bf16(np.full(64, 1e-38, np.float32) * rng.choice([-1.0, 1.0], 64)), -117))
    return out


def test_row_rule(harness, tmp_path):
    cases = _rule_rows()
    W = np.stack([r for _, r, _ in cases])
    ok, e, codes, wd = _rows(harness, str(tmp_path), W)
    assert ok.all()
    for (name, row, want_e), ei, ci, wi in zip(cases, e, codes, wd):
        assert ei == want_e, (name, int(ei), want_e)
        a = float(np.abs(row).max())
        if a > 0 and ei > -117:          # the smallest exponent that keeps the row inside 448
            assert a * 2.0 ** -float(ei) <= 448.0 < a * 2.0 ** -(float(ei) - 1), name
        assert not ((ci & 0x7F) == 0x7F).any(), name          # no NaN code
        assert np.isfinite(wi).all() and _bf16(wi).tobytes() == wi.tobytes(), name          # float32 -> bfloat16 -> float32 unchanged
        # and w' is the nearest value of the scaled e4m3 grid: torch's cast of the exactly scaled row
        scaled = torch.from_numpy((row.astype(np.float64) * 2.0 ** -float(ei)).astype(np.float32))
        assert np.array_equal(ci, scaled.to(torch.float8_e4m3fn).view(torch.uint8).numpy()), name
        assert np.array_equal(wi, (scaled.to(torch.float8_e4m3fn).float().numpy().astype(np.float64) * 2.0 ** float(ei)).astype(np.float32)), name
        if name == "1e-38":
            assert (np.abs(wi) >= 2.0 ** -126).all()          # a normal bf16
    # NaN / Inf rows are refused, not quantised
    bad = np.zeros((2, 64), np.float32)
    bad[0, 3], bad[1, 60] = np.nan, -np.inf
    assert not _rows(harness, str(tmp_path), bad)[0].any()
    with pytest.raises(ValueError, match="NaN or Inf"):
        quantize_e4m3_rows(bad)


def test_numpy_restatement_equals_the_harness(harness, tmp_path):
    rng = np.random.default_rng(8)
    rows = [r for _, r, _ in _rule_rows()]
    rows += list(_bf16(rng.standard_normal((40, 64)) * rng.choice([1e-30, 1e-3, 0.03, 1.0, 500.0, 1e30], (40, 1))))
    enc = _bf16(_encode_cases()[:64 * 600]).reshape(600, 64)          # midpoints and subnormals as row members
    W = np.concatenate([np.stack(rows), enc]).astype(np.float32)
    ok, e, codes, wd = _rows(harness, str(tmp_path), W)
    c2, e2 = quantize_e4m3_rows(W)
    assert ok.all() and c2.dtype == np.uint8 and e2.dtype == np.int8
    assert np.array_equal(e2, e) and np.array_equal(c2, codes)
    assert np.array_equal(dequantize_e4m3_rows(c2, e2).view(np.uint32), wd.view(np.uint32))
    # a weight that is not a bf16 value is rounded to one first, as the engine's commit does
    raw = (rng.standard_normal((8, 64)) * 0.05).astype(np.float32)
    assert all(np.array_equal(a, b) for a, b in zip(quantize_e4m3_rows(raw), quantize_e4m3_rows(_bf16(raw))))


class _StubEngine:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, a))
        return f


@pytest.mark.parametrize("path,fmt", [("Qwen/Qwen2.5-VL-7B-Instruct", "fp8"), ("Qwen/Qwen3-VL-2B-Instruct", "fp8"), ("Qwen/Qwen2.5-VL-7B-Instruct", None)])
def test_tagger_sets_the_weight_format_before_it_loads(path, fmt):
    from facet_amd.vlm_tagger import VLMTagger
    e = _StubEngine()
    cfg = dict(model_path=path)
    if fmt:
        cfg["weight_format"] = fmt
    VLMTagger(cfg, engine=e).load(state_dict={})
    names = [c[0] for c in e.calls]
    assert e.calls[names.index("vlm_weight_format")][1] == (fmt or "bf16",)
    assert names.index("vlm_weight_format") < names.index("load_weights")


def test_unknown_weight_format_is_rejected():
    from facet_amd.vlm_composition import Qwen2VLModel
    from facet_amd.vlm_tagger import VLMTagger
    with pytest.raises(ValueError, match="weight_format"):
        VLMTagger(dict(model_path="Qwen/Qwen2.5-VL-7B-Instruct", weight_format="int4"), engine=_StubEngine())
    with pytest.raises(ValueError, match="weight_format"):
        Qwen2VLModel(_StubEngine(), {}, weight_format="int4")
    e = _StubEngine()
    Qwen2VLModel(e, {}, weight_format="fp8").to("cuda")
    names = [c[0] for c in e.calls]
    assert e.calls[names.index("vlm_weight_format")][1] == ("fp8",) and names.index("vlm_weight_format") < names.index("load_weights")
