"""Reads tests/golden/similar_golden.json (written by tests/golden/make_similar_golden.py) and regenerates the inputs it describes:
embeddings and centroids are not stored, only the seeds they are drawn from."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "similar_golden.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def vector(spec, d):
    """None -> None; {"seed"} -> seeded normal float32 [d]; {"seed", "base", "eps"} -> the base seed's vector plus eps times this
    seed's (eps = 0: an exact copy, whose totals tie exactly)."""
    if spec is None:
        return None
    own = np.random.default_rng(spec["seed"]).standard_normal(d).astype(np.float32)
    if "base" not in spec:
        return own
    base = np.random.default_rng(spec["base"]).standard_normal(d).astype(np.float32)
    return (base + np.float32(spec["eps"]) * own).astype(np.float32)


def build_index_inputs(lib):
    """-> keyword arguments of SimilarPhotoIndex.add"""
    ph = lib["photos"]
    blobs = [None if p["emb"] is None else vector(p["emb"], lib["d"]).tobytes() for p in ph]
    return dict(paths=[p["path"] for p in ph], clip_embedding_bytes=blobs, date_taken=[p["date_taken"] for p in ph],
                aggregate=[p["aggregate"] for p in ph], person_ids=[p["persons"] for p in ph], filenames=[p["filename"] for p in ph],
                aesthetic=[p["aesthetic"] for p in ph])


def build_persons(merge):
    """-> the person dicts merge_groups / merge_candidates take (in table order, not yet sorted by face count)"""
    out = []
    for p in merge["persons"]:
        v = vector(p["centroid"], merge["d"])
        out.append({"id": p["id"], "name": p["name"], "face_count": p["face_count"], "centroid": None if v is None else v.tobytes()})
    return out
