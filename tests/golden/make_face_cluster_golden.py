"""Generates tests/golden/face_cluster_golden.npz: the CPU oracle of the face-clustering feature.

Inputs are made up HERE from seeds (the tests regenerate them and check a SHA-1); only seeds and results are stored.
Per case (rows x, scaled by random norms 5..30 like raw ArcFace outputs; xn = x / (|x| + 1e-10) in float32, then float64):
  * core distances for min_samples 1, 2, 5: brute force on the float64 distance matrix (direct differences), the point itself
    counted, as sklearn and `hdbscan` do;
  * a minimum spanning tree of the float64 mutual-reachability matrix (Prim, in this file - scipy's csgraph drops zero weights,
    which exact duplicates produce), its weights sorted; where no weight is zero the sorted weights must equal those of
    scipy.sparse.csgraph.minimum_spanning_tree;
  * the labels of sklearn.cluster.HDBSCAN(metric='precomputed') 1.7.2 on the float64 distance matrix for min_cluster_size 2,
    min_samples 1 / 2 / 5 and cluster_selection_epsilon 0 and sqrt(0.3).
A case is REFUSED (the script stops) unless sklearn's labels are the same partition when the distance matrix is formed the way
the GPU sweeps form it (n2_i + n2_j - 2 X X^T in float32) - the fixture then has margin against selection error - and when the
points are presented in another order (sklearn's own answer must not hang on how it breaks ties).

Person assignment: the reference's own `_update_database` / `match_face_to_person` (faces/clusterer.py:327-520) are RUN on a
scratch SQLite file; what they wrote is stored. Needs the reference checkout:

    FACET_REFERENCE_ROOT=<checkout> python tests/golden/make_face_cluster_golden.py

The `hdbscan` package the reference imports is not installed here: parity with it (and with cuML) stays unpinned.
"""
import contextlib
import hashlib
import io
import os
import sqlite3
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True

MIN_SAMPLES = (1, 2, 5)
EPSILONS = (0.0, float(np.sqrt(0.3)))
SPREAD = 0.035
D = 512


def planted(seed, identities, lo, hi, randoms, duplicates=0):
    """identities x (lo..hi faces: centre / |centre| + SPREAD * N(0,1)) + random rows, shuffled, scaled by norms 5..30; then
    `duplicates` exact copies of earlier rows appended. -> float32 [n, 512], int64 identity per row (-1: random row)."""
    rng = np.random.default_rng(seed)
    rows, ident = [], []
    for k in range(identities):
        c = rng.standard_normal(D)
        c /= np.linalg.norm(c)
        for _ in range(int(rng.integers(lo, hi + 1))):
            rows.append(c + SPREAD * rng.standard_normal(D))
            ident.append(k)
    for _ in range(randoms):
        rows.append(rng.standard_normal(D))
        ident.append(-1)
    x = np.asarray(rows)
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * rng.uniform(5.0, 30.0, (len(rows), 1))
    order = rng.permutation(len(rows))
    x, ident = x[order].astype(np.float32), np.asarray(ident, np.int64)[order]
    if duplicates:
        src = rng.choice(len(x), size=duplicates, replace=False)
        x, ident = np.concatenate([x, x[src]]), np.concatenate([ident, ident[src]])
    return np.ascontiguousarray(x), ident


# name -> (seed, identities, lo, hi, randoms, duplicates)
CASES = {
    "a": (101, 40, 2, 29, 60, 0),
    "b": (204, 120, 6, 22, 300, 0),      # 6..22: an identity stays larger than min_samples 5; seeds 202 / 203 were refused (order)
    "c": (303, 10, 3, 12, 8, 6),
    "n2": (404, 1, 2, 2, 0, 0),
    "n3": (505, 1, 3, 3, 0, 0),
}


def normalise32(x):
    return (x / (np.linalg.norm(x, axis=1, keepdims=True) + np.float32(1e-10))).astype(np.float32)


def dist64(xn):
    x = xn.astype(np.float64)
    out = np.empty((len(x), len(x)))
    for i in range(len(x)):
        out[i] = np.sqrt(((x - x[i]) ** 2).sum(axis=1))
    return out


def dist_gemm32(xn):
    n2 = (xn * xn).sum(axis=1, dtype=np.float32)
    d2 = (n2[:, None] + n2[None, :]) - np.float32(2) * (xn @ xn.T)
    d2 = np.maximum(d2, np.float32(0))
    np.fill_diagonal(d2, 0)
    return np.sqrt(d2.astype(np.float64))


def prim(w):
    """Minimum spanning tree of a dense symmetric matrix: edges (u < v) and weights in the order Prim adds them."""
    n = len(w)
    inside = np.zeros(n, bool)
    inside[0] = True
    best, src = w[0].copy(), np.zeros(n, np.int64)
    best[0] = np.inf
    eu, ev, ew = [], [], []
    for _ in range(n - 1):
        j = int(np.argmin(best))
        eu.append(min(j, int(src[j]))); ev.append(max(j, int(src[j]))); ew.append(float(best[j]))
        inside[j] = True
        best[j] = np.inf
        closer = (w[j] < best) & ~inside
        best[closer] = w[j][closer]
        src[closer] = j
    return np.asarray(eu), np.asarray(ev), np.asarray(ew)


def same_partition(a, b):
    """Equal up to renaming of the clusters; the noise sets identical."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    fwd, back = {}, {}
    for p, q in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(p, q) != q or back.setdefault(q, p) != p:
            return False
    return True


def sk_labels(dist, ms, eps):
    from sklearn.cluster import HDBSCAN
    return HDBSCAN(metric="precomputed", min_cluster_size=2, min_samples=ms, cluster_selection_epsilon=eps,
                   allow_single_cluster=False, copy=True).fit(dist).labels_


def cluster_case(name, out):
    from scipy.sparse.csgraph import minimum_spanning_tree
    x, ident = planted(*CASES[name])
    n = len(x)
    xn = normalise32(x)
    d64, d32 = dist64(xn), dist_gemm32(xn)
    off = ~np.eye(n, dtype=bool)
    err = float(np.abs(d64 ** 2 - d32 ** 2)[off].max())
    out[f"{name}_sha1"] = hashlib.sha1(x.tobytes()).hexdigest()
    out[f"{name}_n"] = n
    perm = np.random.default_rng(9).permutation(n)
    for ms in MIN_SAMPLES:
        if ms > n:
            continue
        core = np.sort(d64, axis=1)[:, ms - 1]
        mr = np.maximum(np.maximum(core[:, None], core[None, :]), d64)
        eu, ev, ew = prim(mr)
        if ew.min() > 0:
            ref = np.sort(minimum_spanning_tree(np.triu(mr, 1)).data)
            assert len(ref) == n - 1 and np.array_equal(ref, np.sort(ew)), f"{name} ms={ms}: Prim and scipy disagree"
        out[f"{name}_core_{ms}"] = core
        out[f"{name}_mst_u_{ms}"] = eu.astype(np.uint16)
        out[f"{name}_mst_v_{ms}"] = ev.astype(np.uint16)
        out[f"{name}_mst_w_{ms}"] = ew
        for ei, eps in enumerate(EPSILONS):
            lab = sk_labels(d64, ms, eps)
            assert same_partition(lab, sk_labels(d32, ms, eps)), f"{name} ms={ms} eps={eps:.3f}: no margin against the fp32 GEMM form - REFUSED"
            again = np.empty_like(lab)
            again[perm] = sk_labels(d64[np.ix_(perm, perm)], ms, eps)
            assert same_partition(lab, again), f"{name} ms={ms} eps={eps:.3f}: sklearn's answer depends on the point order - REFUSED"
            out[f"{name}_labels_{ms}_{ei}"] = lab.astype(np.int16)
            planted_ok = same_partition(lab[ident >= 0], ident[ident >= 0]) if (ident >= 0).any() else None
            print(f"case {name}: n={n} min_samples={ms} eps={eps:.3f}: {lab.max() + 1} clusters, {(lab < 0).sum()} noise, "
                  f"ties in MST {n - 1 - len(np.unique(ew))}, planted recovered {planted_ok}, max |d2_64 - d2_gemm32| {err:.2e}")


# ---- person assignment: the reference's own code on a scratch database -------------------------------------------------------
def person_inputs(seed=606):
    """14 clusters of unit embeddings + noise faces; 5 existing persons: two near cluster 0 (the closer one second), one near
    cluster 3, one between clusters (below the threshold), one unrelated. -> emb [n,512] f32 (normalised), labels, face ids,
    existing {id: centroid f32}, queries [(bytes)]"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((14, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows, labels = [], []
    for k in range(14):
        for _ in range(int(rng.integers(2, 9))):
            rows.append(centres[k] + SPREAD * rng.standard_normal(D))
            labels.append(k)
    for _ in range(9):
        rows.append(rng.standard_normal(D))
        labels.append(-1)
    order = rng.permutation(len(rows))
    emb = np.asarray(rows)[order]
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    labels = np.asarray(labels, np.int64)[order]
    face_ids = (1000 + 3 * rng.permutation(len(rows))).tolist()

    def near(k, noise):
        v = centres[k] + noise * rng.standard_normal(D)
        return (v * rng.uniform(0.5, 4.0)).astype(np.float32)          # stored centroids need not be unit length

    existing = {7: near(0, 0.030), 3: near(0, 0.012), 12: near(3, 0.02), 5: ((centres[5] + centres[6]) * 0.7).astype(np.float32),
                9: rng.standard_normal(D).astype(np.float32)}
    queries = [near(0, 0.02).tobytes(), near(3, 0.03).tobytes(), near(8, 0.02).tobytes(), rng.standard_normal(D).astype(np.float32).tobytes(),
               near(5, 0.05).tobytes(), np.ones(256, np.float32).tobytes()]
    return emb, labels, face_ids, existing, queries


def run_reference_persons(out):
    root = os.environ.get("FACET_REFERENCE_ROOT")
    assert root and os.path.isdir(root), "set FACET_REFERENCE_ROOT to the reference checkout"
    sys.path.insert(0, root)
    from faces.clusterer import FaceClusterer as RefClusterer            # noqa: E402

    emb, labels, face_ids, existing, queries = person_inputs()
    out["persons_sha1"] = hashlib.sha1(emb.tobytes() + b"".join(existing[k].tobytes() for k in existing)).hexdigest()
    for tag, use_existing in (("fresh", False), ("merge", True)):
        with tempfile.TemporaryDirectory() as d:
            db = os.path.join(d, "faces.db")
            with sqlite3.connect(db) as conn:
                conn.execute("CREATE TABLE faces (id INTEGER PRIMARY KEY, photo_path TEXT, embedding BLOB, person_id INTEGER, "
                             "face_thumbnail BLOB, bbox_x1 REAL, bbox_y1 REAL, bbox_x2 REAL, bbox_y2 REAL)")
                conn.execute("CREATE TABLE persons (id INTEGER PRIMARY KEY AUTOINCREMENT, name TEXT, representative_face_id INTEGER, "
                             "face_count INTEGER, centroid BLOB, auto_clustered INTEGER, face_thumbnail BLOB)")
                conn.executemany("INSERT INTO faces (id, photo_path, embedding) VALUES (?, ?, ?)",
                                 [(fid, f"/p/{fid}.jpg", e.tobytes()) for fid, e in zip(face_ids, emb)])
                if use_existing:
                    conn.executemany("INSERT INTO persons (id, name, centroid, auto_clustered) VALUES (?, ?, ?, 0)",
                                     [(pid, f"person {pid}", c.tobytes()) for pid, c in existing.items()])
                conn.commit()
            ref = RefClusterer(db, merge_threshold=0.6)
            with contextlib.redirect_stdout(io.StringIO()):
                ref._update_database(dict(zip(face_ids, labels.tolist())), emb, face_ids)
            with sqlite3.connect(db) as conn:
                person_of = dict(conn.execute("SELECT id, person_id FROM faces").fetchall())
                # what _update_database inserted, in insertion order; centroids of new persons are not touched afterwards
                new = conn.execute("SELECT id, representative_face_id, face_count, centroid FROM persons WHERE auto_clustered = 1 "
                                   "ORDER BY id").fetchall()
                # the order in which the reference reads existing persons (its dict order decides ties)
                read_order = [r[0] for r in conn.execute("SELECT id FROM persons WHERE centroid IS NOT NULL AND auto_clustered = 0")]
            out[f"persons_{tag}_face_person"] = np.asarray([person_of[f] if person_of[f] is not None else -1 for f in face_ids], np.int64)
            out[f"persons_{tag}_new_id"] = np.asarray([r[0] for r in new], np.int64)
            out[f"persons_{tag}_new_rep"] = np.asarray([r[1] for r in new], np.int64)
            out[f"persons_{tag}_new_count"] = np.asarray([r[2] for r in new], np.int64)
            out[f"persons_{tag}_new_centroid"] = np.stack([np.frombuffer(r[3], np.float32) for r in new])
            out[f"persons_{tag}_read_order"] = np.asarray(read_order, np.int64)
            old = set(existing) if use_existing else set()
            print(f"persons {tag}: {len(new)} new persons, {sum(1 for f in face_ids if person_of[f] in old)} faces merged into "
                  f"existing persons {sorted(set(person_of[f] for f in face_ids if person_of[f] in old))}")
            if use_existing:
                # match_face_to_person on the database as _update_database left it would see recomputed centroids; use a copy that
                # holds the ORIGINAL existing persons only, which is what the test hands to our method
                db2 = os.path.join(d, "match.db")
                with sqlite3.connect(db2) as conn:
                    conn.execute("CREATE TABLE persons (id INTEGER PRIMARY KEY AUTOINCREMENT, name TEXT, centroid BLOB)")
                    conn.executemany("INSERT INTO persons (id, name, centroid) VALUES (?, ?, ?)",
                                     [(pid, f"person {pid}", c.tobytes()) for pid, c in existing.items()])
                    conn.commit()
                ref2 = RefClusterer(db2, merge_threshold=0.6)
                got = [ref2.match_face_to_person(q) for q in queries]
                got_strict = [ref2.match_face_to_person(q, threshold=0.95) for q in queries]
                out["persons_match"] = np.asarray([-1 if g is None else g for g in got], np.int64)
                out["persons_match_095"] = np.asarray([-1 if g is None else g for g in got_strict], np.int64)
                print("match_face_to_person:", got, "| threshold 0.95:", got_strict)
    # margins: no decision of the fixture may sit within 1e-3 of a threshold or of a tie, so fp32 summation order cannot flip it
    ex = np.stack([existing[k] / (np.linalg.norm(existing[k]) + 1e-10) for k in existing])
    cents = []
    for k in sorted(set(labels[labels >= 0].tolist())):
        c = emb[labels == k].mean(axis=0)
        cents.append(c / np.linalg.norm(c))
    qs = [np.frombuffer(q, np.float32) for q in queries if len(q) == 4 * D]
    sims = np.concatenate([np.stack(cents) @ ex.T, np.stack([q / np.linalg.norm(q) for q in qs]) @ ex.T])
    top = np.sort(sims, axis=1)
    assert np.abs(sims - 0.6).min() > 1e-3 and np.abs(sims - 0.95).min() > 1e-3 and (top[:, -1] - top[:, -2]).min() > 1e-3, "persons: a decision has no margin"


def write_npz(path, arrays):
    """numpy.savez_compressed with a fixed member timestamp, so that a re-run reproduces the file byte for byte."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    out = {}
    for name in CASES:
        cluster_case(name, out)
    run_reference_persons(out)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "face_cluster_golden.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
