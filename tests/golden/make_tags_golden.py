"""Generates tests/golden/tags_golden.json by RUNNING THE REFERENCE'S OWN `CLIPTagger` (models/tagger.py:77-158) and `get_tag_params`
(utils/tags.py:38-52). Nothing of the reference is stored except the tag names, group sizes and art tags of its shipped vocabulary
(scoring_config.json: 61 tags / 239 prompts) and what its functions returned on OUR inputs.

    python tests/golden/make_tags_golden.py /path/to/reference

The tagger is built with clip_model=None and gets `tag_names` and `text_embeddings` (a torch CPU tensor) by hand. The inputs are seeded
and dyadic (tests/tags_ref.py: every entry k/64, |k| <= 8, d = 768), so every similarity is exact in fp32 in any summation order and the
engine's GEMM must reproduce the reference's matmul bit for bit. Candidate embedding rows are searched for the edge cases below with
exact integer arithmetic; the five rows picked are then judged by the reference, and the generator asserts on ITS output that each
case is there (at threshold 0.25 = 1024 units of 2^-12, max_tags 5, the defaults of get_tags_from_embedding):
  none       no tag kept
  exact      exactly max_tags kept
  more+tie   more than max_tags kept, and the tags at positions max_tags-1 and max_tags have the same score (the tie straddles the cut)
  equal      a kept tag whose score equals the threshold
  second     a kept tag whose best synonym is not its first
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tags_ref as R      # noqa: E402

SEED = 61239
THRESHOLD, MAX_TAGS = 0.25, 5
LISTS = [(0.25, 5), (0.22, 5), (0.25, 1), (0.25, 61), (0.24, 10), (0.0, 3)]       # (threshold, max_tags) of get_tags_from_embedding
DICTS = [0.20, 0.25]                                                               # thresholds of get_tags_with_scores
ART = [0.24, 0.0]                                                                  # thresholds of is_artwork
UNIT = 4096


def main(ref):
    sys.path.insert(0, ref)
    import torch
    with contextlib.redirect_stdout(io.StringIO()):
        from config import ScoringConfig
        from models.tagger import CLIPTagger
        from utils import get_tag_params
        cfg = ScoringConfig(os.path.join(ref, "scoring_config.json"))
    vocab = cfg.get_tag_vocabulary()
    tags = list(vocab)
    sizes = [len(vocab[t]) for t in tags]
    assert (len(tags), sum(sizes)) == (61, 239)
    names = [t for t, s in zip(tags, sizes) for _ in range(s)]
    T = len(names)
    text = R.golden_text(SEED, T)
    tk = np.rint(text * 64).astype(np.int64)

    # ---- the search, in exact integers (units of 2^-12) ----
    def fold(units):                                   # per-tag max and whether the best synonym is the first
        off = np.concatenate([[0], np.cumsum(sizes)])
        best = np.array([units[off[g]:off[g + 1]].max() for g in range(len(sizes))])
        first = np.array([units[off[g]] for g in range(len(sizes))])
        return best, first
    want = {}
    thr_u = int(THRESHOLD * UNIT)
    for amp in (1, 2, 3, 4, 5, 6, 8):
        rows = np.arange(4000)
        units = R.dyadic_rows(SEED, amp, rows, amp) @ tk.T
        for r in rows:
            best, first = fold(units[r])
            kept = np.sort(best[best >= thr_u])[::-1]
            second = bool(((best >= thr_u) & (best > first)).any())
            if len(kept) == 0:
                want.setdefault("none", (int(r), amp))
            if len(kept) == MAX_TAGS and second:
                want.setdefault("exact", (int(r), amp))
            if len(kept) > MAX_TAGS and kept[MAX_TAGS - 1] == kept[MAX_TAGS] and kept[MAX_TAGS] > thr_u:
                want.setdefault("more+tie", (int(r), amp))
            if len(kept) and kept[-1] == thr_u and len(kept) != MAX_TAGS:
                want.setdefault("equal", (int(r), amp))
            if len(kept) > MAX_TAGS + 2 and second and kept[MAX_TAGS - 1] != kept[MAX_TAGS]:
                want.setdefault("second", (int(r), amp))
    order = ["more+tie", "none", "exact", "equal", "second"]
    assert all(k in want for k in order), sorted(want)
    picks = [want[k] for k in order]
    emb = R.golden_embeddings(SEED, picks)

    # ---- the reference ----
    tagger = CLIPTagger(clip_model=None, device="cpu", config=cfg)
    assert tagger.text_embeddings is None
    tagger.tag_names = list(names)
    tagger.text_embeddings = torch.from_numpy(text.copy())
    blobs = [e.tobytes() for e in emb]
    lists = [[tagger.get_tags_from_embedding(b, threshold=t, max_tags=m) for b in blobs] for t, m in LISTS]
    dicts = [[tagger.get_tags_with_scores(b, threshold=t) for b in blobs] for t in DICTS]
    art = [[bool(tagger.is_artwork(b, threshold=t)) for b in blobs] for t in ART]
    assert tagger.get_tags_from_embedding(None) == [] and tagger.get_tags_with_scores(None) == {}

    # ---- each case, asserted on what the reference answered ----
    full = [tagger.get_tags_with_scores(b, threshold=THRESHOLD) for b in blobs]          # rounded, only to count
    default = lists[0]
    sims = (emb.astype(np.float64) @ text.astype(np.float64).T)
    assert np.array_equal(sims * UNIT, np.rint(sims * UNIT)) and np.abs(sims * UNIT).max() < 2 ** 24
    exact_scores = []
    for i in range(len(blobs)):
        sc = {}
        for n_, s in zip(names, sims[i]):
            if n_ not in sc or s > sc[n_]:
                sc[n_] = s
        exact_scores.append(sc)
    k = {name: i for i, name in enumerate(order)}
    assert default[k["none"]] == [] and full[k["none"]] == {}
    assert len(full[k["exact"]]) == MAX_TAGS and len(default[k["exact"]]) == MAX_TAGS
    i = k["more+tie"]
    all_i = lists[3][i]                                                                   # max_tags = 61: every kept tag in order
    assert len(all_i) > MAX_TAGS and default[i] == all_i[:MAX_TAGS]
    a, b = all_i[MAX_TAGS - 1], all_i[MAX_TAGS]
    assert exact_scores[i][a] == exact_scores[i][b] and tags.index(a) < tags.index(b), "the tie straddles the cut, lower tag id first"
    i = k["equal"]
    assert any(exact_scores[i][t] == THRESHOLD for t in lists[3][i]), "a kept score equals the threshold"
    first_of = {t: int(np.concatenate([[0], np.cumsum(sizes)])[g]) for g, t in enumerate(tags)}
    for i in (k["second"], k["exact"]):
        assert any(exact_scores[i][t] > sims[i][first_of[t]] for t in default[i]), "a kept tag's best synonym is not its first"
    assert len(lists[3][k["second"]]) > MAX_TAGS

    # ---- get_tag_params on the shipped settings and on settings of ours ----
    params = []
    shipped = [cfg.get_clip_settings(), cfg.get_tagging_settings()]
    for clip, tagging in (shipped, [{}, {}], [{"similarity_threshold_percent": 25}, {"max_tags": 8}], [{"similarity_threshold_percent": 7, "model_name": "x"}, {"enabled": False}]):
        fake = types.SimpleNamespace(get_clip_settings=lambda c=clip: c, get_tagging_settings=lambda t=tagging: t)
        thr, mt = get_tag_params(fake)
        params.append({"clip": clip, "tagging": tagging, "threshold": thr, "max_tags": mt})

    out = {"seed": SEED, "d": R.GOLDEN_D, "tags": tags, "sizes": sizes, "art_tags": sorted(cfg.get_art_tags()), "picks": picks, "covers": order,
           "lists": [{"threshold": t, "max_tags": m, "rows": rows} for (t, m), rows in zip(LISTS, lists)],
           "dicts": [{"threshold": t, "rows": [list(map(list, d.items())) for d in rows]} for t, rows in zip(DICTS, dicts)],
           "artwork": [{"threshold": t, "rows": rows} for t, rows in zip(ART, art)],
           "tag_params": params}
    with open(os.path.join(HERE, "tags_golden.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("picked", dict(zip(order, picks)), "| kept at 0.25:", [len(d) for d in full], "| default lists:", default)


if __name__ == "__main__":
    main(sys.argv[1])
