"""Generates tests/golden/similar_golden.json by running the reference's own `api_similar_photos` (api/routers/gallery.py) and
`get_merge_groups` (faces/merge_analyzer.py) on a small library made up HERE.

    python tests/golden/make_similar_golden.py /path/to/the/reference/checkout

The route is imported with the working directory at the reference root, a stub module for the absent `jwt`, a scratch SQLite file
holding `photos`, `faces` and `persons`, and `get_db_connection`, `load_viewer_config` and `get_visibility_clause` patched on the
module; it is a coroutine whose defaults are `Query(...)` objects, so every weight is passed explicitly. Only our seeded inputs
(embeddings as seeds, tests/similar_golden_lib.py regenerates them) and the recorded results are written.

The library covers: planted near-copies; 22 exact copies whose totals tie to all digits and straddle the `limit` cut (and, seen from one of them, the whole shortlist); photos
without dates, aggregates, persons or embeddings; aggregate 0; dates 0, 7, 8, 30, 31 and 400 days from the source, each also just
under the next whole day; a source without persons; a source without an embedding; a limit larger than the library; a visibility
mask; weights other than the defaults.

The tie band: this script refuses (asserts) any input for which a total lies within 1e-6 of a 4-digit rounding boundary, or a
breakdown value within 1e-6 of a 3-digit one - such a value could round either way under a legitimate change of summation order.
"""
import asyncio
import json
import os
import sqlite3
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from similar_golden_lib import GOLDEN, build_index_inputs, build_persons, vector  # noqa: E402

D = 128
W = [0.4, 0.3, 0.2, 0.1]


def make_library(salt):
    """salt moves every seed: main() tries salts until no recorded value lies in the tie band."""
    photos = []
    S = 10000 * salt

    def add(name, emb, date, agg, persons, aesthetic=None):
        photos.append({"path": f"/photos/{name}.jpg", "filename": f"{name}.jpg", "emb": emb, "date_taken": date, "aggregate": agg,
                       "aesthetic": aesthetic, "persons": persons})

    add("src", {"seed": S + 100}, "2024:06:15 12:00:00", 7.25, [3, 5], 6.5)
    for i, eps in enumerate((0.02, 0.05, 0.1, 0.3)):                       # planted near-copies of the source
        add(f"copy{i}", {"seed": S + 110 + i, "base": S + 100, "eps": eps}, "2024:06:15 09:30:00", 7.0 - i, [3, 5] if i % 2 else [5], 5.0 + i)
    for i in range(22):                                                    # exact ties: the same vector and metadata 22 times
        add(f"tie{i}", {"seed": S + 1, "base": S + 120, "eps": 0.0}, "2024:06:01 08:00:00", 6.0, [5, 8])
    dates = ["2024:06:16 11:59:59", "2024:06:22 12:00:00", "2024:06:23 11:59:59", "2024:06:23 12:00:00", "2024:07:15 12:00:00",
             "2024:07:16 11:59:59", "2024:07:16 12:00:00", "2025:07:20 12:00:00", "2025:07:21 11:59:59", "2023:05:12 12:00:00",
             "2024:06:14 12:00:01", "2024:06:15 12:00:00+02:00"]
    for i, dt in enumerate(dates):                                         # 0, 7, 7, 8, 30, 30, 31, 400, 400, 400 days, 0, 0
        add(f"date{i}", {"seed": S + 230 + i}, dt, round(5.41 + 0.23 * i, 2), [])
    add("nodate", {"seed": S + 300}, None, 8.0, [3])
    add("baddate", {"seed": S + 301}, "not a date", 8.0, [3])
    add("emptydate", {"seed": S + 302}, "", 4.0, [9])
    add("noagg", {"seed": S + 303}, "2024:06:10 10:00:00", None, [5, 3, 9, 11])
    add("zeroagg", {"seed": S + 304}, "2024:06:10 10:00:00", 0.0, [5])
    add("farscore", {"seed": S + 305}, "2024:06:15 13:00:00", 1.0, [])
    add("noemb", None, "2024:06:15 12:30:00", 7.5, [3, 5], 7.0)            # a source, never a candidate
    add("noemb2", None, None, None, [])
    add("nopersons", {"seed": S + 306, "base": S + 100, "eps": 0.5}, "2024:06:15 18:00:00", 7.25, [])
    add("bare", {"seed": S + 307}, None, None, [])
    for i in range(24):                                                    # a crowd around a second centre
        add(f"crowd{i}", {"seed": S + 400 + i, "base": S + 120, "eps": 0.6 + 0.05 * (i % 5)}, f"2024:0{5 + i % 3}:{10 + i % 17} 1{i % 10}:15:00",
            round(3.0 + 0.3 * i, 2), [[5], [8], [3, 8], [], [11, 5, 8]][i % 5])
    return {"d": D, "photos": photos}


ALL_BUT = ["src", "copy1", "tie0", "tie1", "date0", "date7", "noemb", "zeroagg", "crowd2", "crowd4"]      # "limit above library": what stays visible
CASES = [  # name, source, limit, weights, hidden (a list of names, or ("all but", names))
    ("default", "src", 20, W, None),
    ("tie cut", "src", 7, W, None),
    ("tie cut in crowd", "crowd3", 5, W, None),
    ("tie source", "tie2", 4, W, None),
    ("top 1", "src", 1, W, None),
    ("limit above library", "src", 500, W, ("all but", ALL_BUT)),
    ("no persons", "nopersons", 6, W, None),
    ("no embedding", "noemb", 8, W, None),
    ("nothing but an embedding", "bare", 3, W, None),
    ("nothing at all", "noemb2", 20, W, None),
    ("no date", "nodate", 4, W, None),
    ("masked", "src", 8, W, ["copy0", "tie1", "tie2", "date3", "crowd5"]),
    ("masked source", "src", 20, W, ["src"]),
    ("weights", "src", 9, [0.1, 0.5, 0.3, 0.1], None),
    ("clip only", "copy1", 5, [1.0, 0.0, 0.0, 0.0], None),
    ("no clip", "src", 10, [0.0, 0.45, 0.33, 0.22], None),
    ("date heavy", "date3", 14, [0.2, 0.0, 0.7, 0.1], None),
    ("unknown", "missing", 20, W, None),
]


def make_merge():
    persons = []
    for i in range(60):
        near = {7: (3, 0.4), 12: (3, 0.7), 20: (19, 0.3), 33: (20, 0.5), 41: (40, 0.9), 50: (49, 0.6), 51: (49, 0.6), 52: (51, 0.5)}.get(i)
        spec = {"seed": 700 + i} if near is None else {"seed": 700 + i, "base": 700 + near[0], "eps": near[1]}
        persons.append({"id": 1000 + i, "name": None if i % 3 else f"Person {i}", "face_count": [40, 7, 7, 120, 3][i % 5] + (i // 5) % 3,
                        "centroid": None if i in (5, 44) else spec})
    return {"d": 512, "threshold": 0.6, "persons": persons}


def reference_modules(ref):
    os.chdir(ref)
    sys.path.insert(0, ref)
    sys.modules.setdefault("jwt", types.ModuleType("jwt"))
    import api.routers.gallery as gallery
    from faces.merge_analyzer import get_merge_groups
    return gallery, get_merge_groups


def near_boundary(value, digits):
    scaled = value * 10 ** digits
    return abs(abs(scaled - np.floor(scaled)) - 0.5) < 1e-6 * 10 ** digits


class Refused(Exception):
    pass


def record_cases(gallery, lib):
    """The reference's responses for CASES on this library; Refused when a recorded value lies in the tie band."""
    inputs = build_index_inputs(lib)
    db = os.path.join(tempfile.mkdtemp(), "scratch.db")
    conn = sqlite3.connect(db)
    conn.executescript("""CREATE TABLE photos (path TEXT PRIMARY KEY, filename TEXT, clip_embedding BLOB, date_taken TEXT, aggregate REAL,
                                               aesthetic REAL, comp_score REAL);
                          CREATE TABLE faces (id INTEGER PRIMARY KEY, photo_path TEXT, person_id INTEGER);""")
    for i, p in enumerate(lib["photos"]):
        conn.execute("INSERT INTO photos VALUES (?,?,?,?,?,?,?)", (p["path"], p["filename"], inputs["clip_embedding_bytes"][i], p["date_taken"],
                                                                   p["aggregate"], p["aesthetic"], None))
        for pid in p["persons"]:
            conn.execute("INSERT INTO faces (photo_path, person_id) VALUES (?,?)", (p["path"], pid))
        conn.execute("INSERT INTO faces (photo_path, person_id) VALUES (?,NULL)", (p["path"],))      # an unassigned face
    conn.commit()
    conn.close()

    def connect():
        c = sqlite3.connect(db)
        c.row_factory = sqlite3.Row
        return c

    hidden = []
    gallery.get_db_connection = connect
    gallery.load_viewer_config = lambda: {}
    gallery.get_visibility_clause = lambda user_id: (("path NOT IN (%s)" % ",".join("?" * len(hidden)), list(hidden)) if hidden else ("1=1", []))

    # the unrounded totals and factors behind the recorded roundings, from this repository's restatement (it must agree anyway)
    from facet_amd.similar import SimilarPhotoIndex
    probe = SimilarPhotoIndex(None)
    probe.add(**inputs)
    cases = []
    for name, source, limit, weights, hide in CASES:
        if isinstance(hide, tuple):
            hide = [os.path.basename(p)[:-4] for p in probe.paths if os.path.basename(p)[:-4] not in hide[1]]
        hidden[:] = [f"/photos/{h}.jpg" for h in (hide or [])]
        path = f"/photos/{source}.jpg"
        result = asyncio.run(gallery.api_similar_photos(path, limit, *weights, user=None))
        assert "error" not in result or result["error"] == "Photo not found", result
        if "similar" in result and result["similar"]:
            # every value that is recorded, and every total that the cut could have let in
            cut = result["similar"][-1]["similarity"] - 1e-4
            listed = {e["path"] for e in result["similar"]}
            for cand in range(len(probe)):
                if cand == probe._row_of[path] or probe.raw[cand] is None or probe.paths[cand] in hidden:
                    continue
                total, factors = probe._rescore(probe._row_of[path], cand, weights)
                if probe.paths[cand] not in listed and total < cut:
                    continue
                if near_boundary(total, 4):
                    raise Refused(f"{name}: total {total!r} of {probe.paths[cand]} is within 1e-6 of a rounding boundary")
                for key, v in factors.items():
                    if probe.paths[cand] in listed and near_boundary(v, 3):
                        raise Refused(f"{name}: {key} {v!r} of {probe.paths[cand]} is within 1e-6 of a rounding boundary")
        cases.append({"name": name, "source": path, "limit": limit, "weights": list(weights), "hidden": list(hidden) if hide else None,
                      "result": json.loads(json.dumps(result))})
    return cases


def main(ref):
    gallery, get_merge_groups = reference_modules(os.path.abspath(ref))
    for salt in range(2000):
        lib = make_library(salt)
        try:
            cases = record_cases(gallery, lib)
            break
        except Refused as e:
            print(f"salt {salt} refused - {e}")
    else:
        raise SystemExit("no salt gave a library outside the tie band")
    lib["salt"] = salt
    for c in cases:
        print(f"{c['name']}: {len(c['result'].get('similar', []))} results" if "similar" in c["result"] else f"{c['name']}: {c['result']}")
    merge = make_merge()
    db = os.path.join(tempfile.mkdtemp(), "persons.db")
    conn = sqlite3.connect(db)
    conn.execute("CREATE TABLE persons (id INTEGER PRIMARY KEY, name TEXT, face_count INTEGER, centroid BLOB)")
    for p in build_persons(merge):
        conn.execute("INSERT INTO persons VALUES (?,?,?,?)", (p["id"], p["name"], p["face_count"], p["centroid"]))
    conn.commit()
    conn.close()
    groups = get_merge_groups(db, merge["threshold"])
    rows = sorted((p for p in build_persons(merge) if p["centroid"]), key=lambda p: -p["face_count"])
    cents = [np.frombuffer(p["centroid"], np.float32) for p in rows]
    cents = [c / (np.linalg.norm(c) + 1e-10) for c in cents]
    cand = []
    for i in range(len(rows)):
        for j in range(i + 1, len(rows)):
            sim = float(np.dot(cents[i], cents[j]))
            assert abs(sim - merge["threshold"]) > 1e-4, "a centroid pair within 1e-4 of the threshold: the input is refused"
            if sim >= merge["threshold"]:
                cand.append((sim, rows[i]["id"], rows[j]["id"]))
    cand.sort(key=lambda c: c[0], reverse=True)
    merge["groups"] = json.loads(json.dumps(groups))
    merge["candidate_ids"] = [[a, b] for _, a, b in cand]        # suggest_person_merges only prints: its loop restated on the same centroids
    print(f"merge: {len(groups)} groups, {len(cand)} candidate pairs")
    with open(GOLDEN, "w") as f:
        json.dump({"library": lib, "cases": cases, "merge": merge}, f, indent=0, separators=(",", ":"))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
