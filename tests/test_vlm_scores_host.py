"""CPU: per-tag confidence scores of the VLM tagger (facet_amd/vlm_tagger.py: tag_confidences, VLMTagger.tag_image_with_scores /
get_tags_with_scores / tag_batch_with_scores) against what the reference's own VLMTagger returned for scripted generations
(tests/golden/make_vlm_scores_host_golden.py -> vlm_scores_host_golden.json): EOS inside the run and none, leading and adjacent commas,
single-character and duplicate tags (tags and segments misaligned), more tags than segments, multi-character tokens, confidences of 1,
empty output, vocabulary matches, thresholds 0 / 0.3 / 1. The ids and log-probs are the golden's; the engine's generation is replaced by
them, padded the way Engine.vlm_generate(return_logprobs=True) pads a row after its EOS (EOS ids, NaN log-probs)."""
import json
import math
import os

import numpy as np
import pytest

from facet_amd._lib import EngineCapacityError
from facet_amd.vlm_tagger import VLMTagger, tag_confidences

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "vlm_scores_host_golden.json")))
EOS = G["eos_token_ids"]
CASES = {c["name"]: c for c in G["cases"]}
WIDTH = max(c["max_new_tokens"] for c in G["cases"])


class _Cfg:
    config = {"standalone_tags": {}}

    def get_categories(self):
        return [{"name": "subject", "tags": {"cat": [], "dog": [], "bird": [], "sky": []}}]

    def get_tag_vocabulary(self):
        return {"cat": [], "dog": [], "bird": [], "sky": []}


def _decoder(case):
    table = {int(k): v for k, v in case["token_text"].items()}
    return lambda ids: "".join(table[int(t)] for t in ids)


def _row(case, width=None):
    """The engine's form of a generated row: EOS-padded ids and NaN log-probs after the first EOS, max_new_tokens wide."""
    width = width or case["max_new_tokens"]
    ids = np.full(width, EOS[0], np.int32)
    lps = np.full(width, np.nan, np.float32)
    ids[:len(case["ids"])] = case["ids"]
    lps[:len(case["ids"])] = case["logprobs"]
    assert np.array_equal(lps[:len(case["ids"])].astype(np.float64), np.asarray(case["logprobs"]))      # fp32 values, exact
    return ids, lps


def _tagger(case, decode=None):
    t = VLMTagger({"model_path": "Qwen/Qwen2.5-VL-7B-Instruct", "max_new_tokens": case["max_new_tokens"]}, _Cfg() if case["vocabulary"] else None,
                  decode=decode or _decoder(case), special_tokens={"eos_token_ids": tuple(EOS)})
    t.model = object()
    return t


def _same(got, want):
    assert list(got) == [k for k, _ in want], (list(got), want)
    for k, v in want:
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tag_confidences_match_the_reference(name):
    c = CASES[name]
    t = _tagger(c)
    dec = _decoder(c)
    assert dec(c["ids"]) == c["text"]
    for mt in (5, 2):
        tags = t._parse_tags(c["text"], mt)
        want = c["result"][f"max_tags_{mt}"]
        if not want:
            assert not tags
            continue
        _same(tag_confidences(c["ids"], c["logprobs"], tags, lambda i: dec([i])), want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dict_methods_match_the_reference(name, monkeypatch):
    c = CASES[name]
    t = _tagger(c)
    ids, lps = _row(c)

    def fake(images, max_new_tokens=None, prompt=None, return_logprobs=False):
        assert return_logprobs and len(images) == 1
        return ids[None], lps[None]
    monkeypatch.setattr(t, "generate_from_images", fake)
    for mt in (5, 2):
        _same(t.tag_image_with_scores("photo", max_tags=mt), c["result"][f"max_tags_{mt}"])
    for th, want in c["threshold"].items():
        _same(t.get_tags_with_scores("photo", threshold=float(th)), want)


def test_golden_covers_the_quirks():
    """The cases exercise what makes the reference's scoring surprising (guards against a regenerated golden losing them)."""
    r = {n: dict((k, v) for k, v in c["result"]["max_tags_5"]) for n, c in CASES.items()}
    assert r["empty_output"] == {} and r["only_commas"] == {}
    assert r["more_tags_than_segments"]["owl"] == 1.0 and r["clamped_at_one"]["cat"] == 1.0
    assert EOS[0] not in CASES["no_eos"]["ids"] and CASES["eos_inside"]["ids"][-1] == EOS[0]
    assert any(0 < len(c["threshold"]["0.3"]) < len(c["result"]["max_tags_5"]) for c in CASES.values())
    assert all(len(c["threshold"]["1.0"]) == sum(v == 1.0 for _, v in c["result"]["max_tags_5"]) for c in CASES.values())
    assert all(len(c["threshold"]["0.0"]) == len(c["result"]["max_tags_5"]) for c in CASES.values())


def test_tag_batch_with_scores_rows_and_capacity_fallback(monkeypatch):
    names = ["eos_inside", "leading_comma", "single_char_and_duplicates", "empty_output", "more_tags_than_segments"]      # (rows end at an EOS)
    cases = [CASES[n] for n in names]
    table = {}
    for c in cases:
        table.update({int(k): v for k, v in c["token_text"].items()})
    decode = lambda ids: "".join(table[int(t)] for t in ids)      # noqa: E731
    t = _tagger(cases[0], decode)
    t.batch_size = 3
    calls = []

    def fake(images, max_new_tokens=None, prompt=None, return_logprobs=False):
        assert return_logprobs
        calls.append(len(images))
        rows = [_row(CASES[n], WIDTH) for n in images]
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    monkeypatch.setattr(t, "generate_from_images", fake)
    want = [dict(c["result"]["max_tags_5"]) for c in cases]
    got = t.tag_batch_with_scores(names)
    assert calls == [3, 2] and len(got) == len(want)
    for g, w in zip(got, want):
        _same(g, list(w.items()))
    # a sub-batch that does not fit: one photo at a time; a photo that still does not fit gets {}
    calls.clear()

    def tight(images, max_new_tokens=None, prompt=None, return_logprobs=False):
        if len(images) > 1 or images[0] == "leading_comma":
            raise EngineCapacityError("does not fit")
        return fake(images, return_logprobs=return_logprobs)
    monkeypatch.setattr(t, "generate_from_images", tight)
    got = t.tag_batch_with_scores(names)
    assert got[1] == {} and calls == [1, 1, 1, 1]
    for i in (0, 2, 3, 4):
        _same(got[i], list(want[i].items()))


def test_nan_after_eos_is_never_read():
    c = CASES["eos_inside"]
    ids, lps = _row(c)
    assert math.isnan(float(lps[-1]))
    t = _tagger(c)
    got = t._scored_tags(ids, lps, 5)
    assert all(math.isfinite(v) for v in got.values())
    _same(got, c["result"]["max_tags_5"])
