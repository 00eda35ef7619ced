"""CPU: the tag selection's host side. tag_select_core.h (the arithmetic the kernel shares) in a stand-alone harness compiled under
AddressSanitizer + UBSan, exactly equal to a plain-Python restatement of the reference's loop (tests/tags_ref.py) on duplicates, NaN,
+-inf, the float32 / double threshold compare, G of 1 / 61 / 64 / 65 and non-contiguous groups; the grouping and its errors; and
the Python layer (CLIPTagger.select_batch / scores_batch / is_artwork_batch, tag_existing.tag_rows / get_tag_params) against what the
reference's own functions returned (tests/golden/tags_golden.json), with a numpy engine standing in for the device."""
import json
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest

import tags_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tags_golden.json")


# ---- tag_select_core.h, sanitized ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("tagsel") / "tag_select_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "facet_amd", "csrc"), os.path.join(ROOT, "tests", "native", "tag_select_harness.cpp"), "-o", exe], check=True)
    return exe


def run_harness(exe, cases, tmp, pad=0):
    """cases: [(sims [n, T], tag_of_prompt [T], G, threshold, max_tags)] -> per case (status, where, perm, goff, ids, scores, counts)"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for sims, top, G, thr, mt in cases:
            sims = np.asarray(sims, np.float32)
            n, T = sims.shape
            rows = np.full((n, T + pad), np.float32("nan"), np.float32)      # the columns past T hold NaN: reading one would show
            rows[:, :T] = sims
            f.write(struct.pack("=5id", n, T, G, mt, T + pad, thr))
            f.write(np.asarray(top, np.int32).tobytes())
            f.write(rows.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    raw, o, out = open(fout, "rb").read(), 0, []

    def take(dtype, count):
        nonlocal o
        a = np.frombuffer(raw, dtype, count, o)
        o += a.nbytes
        return a
    for sims, top, G, thr, mt in cases:
        n, T = np.asarray(sims).shape
        status, where = (int(v) for v in take(np.int32, 2))
        if status != 0:
            out.append((status, where) + (None,) * 5)
            continue
        perm, goff = take(np.int32, T), take(np.int32, G + 1)
        out.append((0, where, perm, goff, take(np.int32, n * mt).reshape(n, mt), take(np.float32, n * mt).reshape(n, mt), take(np.int32, n)))
    assert o == len(raw)
    return out


@pytest.mark.parametrize("pad", [0, 3])
def test_core_equals_the_python_restatement(harness, tmp_path, pad):
    cases = R.cases()
    assert {int(top.max()) + 1 for _, _, top, _, _ in cases} >= {1, 61, 64, 65}
    res = run_harness(harness, [(s, top, int(top.max()) + 1, thr, mt) for _, s, top, thr, mt in cases], str(tmp_path), pad)
    for (name, s, top, thr, mt), (status, _, perm, goff, ids, scores, counts) in zip(cases, res):
        assert status == 0, name
        assert np.array_equal(perm, np.argsort(top, kind="stable")), name                 # sorted by (tag, prompt index)
        assert np.array_equal(goff, np.concatenate([[0], np.cumsum(np.bincount(top))])), name
        assert R.same((ids, scores, counts), R.select(s, top, thr, mt)), name


def test_the_cases_decide_what_they_claim():
    """The restatement itself on the hand-made rows: which tags the NaN, inf and threshold rules keep."""
    by = {name: (s, top) for name, s, top, _, _ in R.cases()}
    s, top = by["nan/inf thr=0.0 max_tags=4"]
    # row 0: tag 0 starts with NaN and stays NaN (dropped); tag 1 = 0.7 (the NaN after 0.5 is skipped); tag 2 = 0.3 (NaN later skipped); tag 3 NaN
    assert [g for g, _ in R.select_row(s[0], top, 0.0, 4)] == [1, 2]
    # row 2: tag 0 = +inf, tag 3 = -inf; at threshold -inf all four tags pass, +inf first and the two ties in id order
    assert [g for g, _ in R.select_row(s[2], top, float("-inf"), 4)] == [0, 2, 1, 3]
    assert R.select_row(s[2], top, float("inf"), 4) == [(0, float("inf")), (2, float("inf"))]
    assert R.select_row(s[3], top, float("nan"), 4) == []
    s, top = by["threshold 0.22"]
    assert float(R.F22) < 0.22
    assert [g for g, _ in R.select_row(s[0], top, 0.22, 3)] == [2]                        # only nextafter(float32(0.22)) passes 0.22
    assert [g for g, _ in R.select_row(s[0], top, float(R.F22), 3)] == [2, 0, 1]          # float32(0.22) twice: the tie in id order
    assert [g for g, _ in R.select_row(s[1], top, 0.22, 3)] == [1]
    assert [g for g, _ in R.select_row(s[1], top, float(R.F22), 3)] == [1, 0, 2]
    top2 = by["scattered G=7 T=23"][1]
    assert any(np.any(np.diff(np.flatnonzero(top2 == g)) > 1) for g in range(7)), "a tag's prompts are not contiguous"


def test_grouping_errors(harness, tmp_path):
    z = np.zeros((1, 3), np.float32)
    res = run_harness(harness, [(z, [0, 0, 2], 3, 0.0, 1),      # id 2 before id 1: a skipped value
                                (z, [0, 1, 1], 3, 0.0, 1),      # id 2 never used
                                (z, [1, 0, 1], 2, 0.0, 1),      # first appearances out of order
                                (z, [0, 3, 1], 3, 0.0, 1),      # outside 0 .. G-1
                                (z, [0, -1, 1], 2, 0.0, 1),
                                (z, [0, 1, 0], 2, 0.0, 2)], str(tmp_path))
    assert [(r[0], r[1]) for r in res[:5]] == [(2, 2), (3, 2), (2, 0), (1, 1), (1, 1)]
    assert res[5][0] == 0 and list(res[5][2]) == [0, 2, 1] and list(res[5][3]) == [0, 2, 3]


# ---- the Python layer against the reference's answers -------------------------------------------------------------------------------
class NumpyEngine:
    """Engine.tag_vocab / tag_select with numpy for the GEMM (exact on the golden's dyadic inputs) and the restatement for the rest."""
    def __init__(self):
        self.calls = 0

    def tag_vocab(self, text, tag_of_prompt):
        self.text, self.top = np.asarray(text, np.float32), np.asarray(tag_of_prompt, np.int32)
        firsts = [int(np.flatnonzero(self.top == g)[0]) for g in range(int(self.top.max()) + 1)]
        assert firsts == sorted(firsts)
        return int(self.top.max()) + 1

    def tag_select(self, emb, threshold, max_tags):
        self.calls += 1
        assert 1 <= max_tags <= int(self.top.max()) + 1
        return R.select(np.asarray(emb, np.float32) @ self.text.T, self.top, threshold, max_tags)


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(GOLDEN))
    from facet_amd.tagger import CLIPTagger
    names = [t for t, s in zip(g["tags"], g["sizes"]) for _ in range(s)]
    cfg = types.SimpleNamespace(get_tag_vocabulary=lambda: {t: [""] * s for t, s in zip(g["tags"], g["sizes"])}, get_art_tags=lambda: set(g["art_tags"]))
    tg = CLIPTagger(None, "cpu", cfg)
    tg.tag_names, tg.text_embeddings = names, R.golden_text(g["seed"], len(names))        # by hand: set_text_embeddings would normalise
    emb = R.golden_embeddings(g["seed"], [tuple(p) for p in g["picks"]])
    eng = NumpyEngine()
    tg.use_engine(eng)
    return g, tg, emb, eng


def test_golden_inputs_are_exact(golden):
    g, tg, emb, _ = golden
    assert (len(g["tags"]), sum(g["sizes"]), emb.shape) == (61, 239, (5, 768))
    for a in (emb, tg.text_embeddings):
        k = a.astype(np.float64) * 64
        assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 8
    s64 = emb.astype(np.float64) @ tg.text_embeddings.astype(np.float64).T
    assert np.array_equal(emb @ tg.text_embeddings.T, s64)                                # fp32 accumulation is exact here


def test_batch_forms_equal_the_reference(golden):
    g, tg, emb, eng = golden
    blobs = [e.tobytes() for e in emb]
    for case in g["lists"]:
        assert tg.select_batch(emb, case["threshold"], case["max_tags"]) == case["rows"], case["threshold"]
        assert tg.select_batch(blobs, case["threshold"], case["max_tags"]) == case["rows"]
        assert [tg.get_tags_from_embedding(b, case["threshold"], case["max_tags"]) for b in blobs] == case["rows"]      # the per-row path agrees
    for case in g["dicts"]:
        got = tg.scores_batch(emb, case["threshold"])
        assert [[[k, v] for k, v in d.items()] for d in got] == case["rows"]              # keys in vocabulary order, round(score, 3)
        assert got == [tg.get_tags_with_scores(b, case["threshold"]) for b in blobs]
    for case in g["artwork"]:
        assert tg.is_artwork_batch(emb, case["threshold"]) == case["rows"]
    assert tg.select_batch([], 0.25, 5) == [] and tg.scores_batch([], 0.2) == []
    assert tg.select_batch(emb, 0.25, 0) == [[] for _ in emb]                             # the reference's slice [:0]
    with pytest.raises(ValueError, match="embedding 1 has 767 floats"):
        tg.select_batch([blobs[0], blobs[1][:-4]], 0.25, 5)


def test_tag_rows_mirrors_both_library_loops(golden):
    from facet_amd.tag_existing import tag_rows
    g, tg, emb, eng = golden
    want = next(c for c in g["lists"] if (c["threshold"], c["max_tags"]) == (0.22, 5))["rows"]
    rows = [("a.jpg", emb[0].tobytes()), ("none.jpg", None), ("b.jpg", emb[1].tobytes()), ("empty.jpg", b""), ("c.jpg", emb[2].tobytes()),
            ("d.jpg", emb[3].tobytes()), ("e.jpg", emb[4].tobytes())]
    keys = ["a.jpg", "b.jpg", "c.jpg", "d.jpg", "e.jpg"]
    calls = eng.calls
    # --recompute-tags (photos.py:613-623): every row with a blob, None where no tag passes
    got = tag_rows(eng, tg, rows, threshold=0.22, max_tags=5)
    assert eng.calls == calls + 1                                                         # one engine call for the library
    assert got == [(",".join(t) if t else None, k) for t, k in zip(want, keys)]
    assert any(s is None for s, _ in got)
    # tag_untagged_photos (tag_existing.py:51-58): only the rows with a tag
    assert tag_rows(eng, tg, rows, 0.22, 5, only_tagged=True) == [(s, k) for s, k in got if s is not None]
    assert tag_rows(eng, tg, [("x", None), ("y", b"")], 0.22, 5) == []
    with pytest.raises(ValueError, match=r"row 2 \('b.jpg'\).*3068 bytes"):
        tag_rows(eng, tg, rows[:2] + [("b.jpg", emb[1].tobytes()[:-4])], 0.22, 5)


def test_get_tag_params(golden):
    from facet_amd.tag_existing import get_tag_params
    g = golden[0]
    assert len(g["tag_params"]) == 4
    for p in g["tag_params"]:
        cfg = types.SimpleNamespace(get_clip_settings=lambda p=p: p["clip"], get_tagging_settings=lambda p=p: p["tagging"])
        assert get_tag_params(cfg) == (p["threshold"], p["max_tags"])
    assert (g["tag_params"][0]["threshold"], g["tag_params"][0]["max_tags"]) == (0.22, 5)      # the shipped settings
