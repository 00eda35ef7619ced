"""Face clustering: the reference's `FaceClusterer` (faces/clusterer.py) without its database.

`cluster_faces` (:126-216) L2-normalises the stored ArcFace embeddings and runs HDBSCAN on them (euclidean,
min_cluster_size = min_faces, min_samples = min(min_faces, 2), cluster_selection_epsilon = sqrt(2 * auto_merge_distance)), then
`_update_database` (:327-478) turns clusters into persons. Here the two O(n^2 d) stages of HDBSCAN* - core distances and the
minimum spanning tree of the mutual-reachability graph - are exact sweeps on the GPU (`Engine.mreach_mst`, fe_mreach_mst); what
follows the tree is `hdbscan_labels` below, plain host code that restates the published algorithm (Campello, Moulavi, Sander 2013;
McInnes, Healy, Astels 2017): single-linkage tree, condensed tree, stabilities, excess-of-mass selection and the epsilon merge of
Malzer & Baum 2020. It is pinned against sklearn.cluster.HDBSCAN 1.7.2 on float64 distances
(tests/golden/make_face_cluster_golden.py); parity with the `hdbscan` package the reference imports, and with cuML, is unpinned:
neither is available offline.

There is no host fallback for the sweeps: without an engine the clusterer cannot run."""
import numpy as np

__all__ = ["hdbscan_labels", "FaceClusterer", "normalise_rows"]


def normalise_rows(embeddings):
    """clusterer.py:157-158 in the dtype given (the stored embeddings are float32)."""
    e = np.asarray(embeddings)
    return e / (np.linalg.norm(e, axis=1, keepdims=True) + 1e-10)


def _single_linkage(n, u, v, w):
    """Edges sorted by weight -> merge t joins nodes left[t], right[t] (points < n, earlier merges n + t') at dist[t]."""
    parent = np.arange(2 * n - 1, dtype=np.int64).tolist()
    size = [1] * n + [0] * (n - 1)
    left, right = [0] * (n - 1), [0] * (n - 1)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for t in range(n - 1):
        a, b = find(int(u[t])), find(int(v[t]))
        if a == b:
            raise ValueError("hdbscan_labels: the edges do not form a tree")
        node = n + t
        left[t], right[t] = a, b
        size[node] = size[a] + size[b]
        parent[a] = parent[b] = node
    return left, right, size


def hdbscan_labels(n, edge_u, edge_v, edge_w, min_cluster_size, cluster_selection_epsilon=0.0):
    """Labels of HDBSCAN* (excess of mass, allow_single_cluster=False) from a minimum spanning tree of the mutual-reachability graph.

    edge_u, edge_v, edge_w: the n - 1 tree edges in any order. -> int64 [n], clusters numbered from 0 in the order of their birth
    in the condensed tree, noise = -1. cluster_selection_epsilon > 0: a selected cluster born below that distance is replaced by
    its first ancestor born at or above it (the ancestor next to the root when there is none)."""
    n = int(n)
    m = int(min_cluster_size)
    if m < 2:
        raise ValueError("min_cluster_size must be at least 2")
    labels = np.full((n,), -1, np.int64)
    if n < 2:
        return labels
    u, v, w = np.asarray(edge_u), np.asarray(edge_v), np.asarray(edge_w, np.float64)
    if not (u.shape == v.shape == w.shape == (n - 1,)):
        raise ValueError("hdbscan_labels: a tree over n points has n - 1 edges")
    # equal weights are taken in the order of their end points, so the answer does not hang on the order the edges arrive in
    u, v = np.minimum(u, v), np.maximum(u, v)
    order = np.lexsort((v, u, w))
    u, v, w = u[order], v[order], w[order]
    left, right, size = _single_linkage(n, u, v, w)

    def leaves(node):
        out, stack = [], [node]
        while stack:
            x = stack.pop()
            if x < n:
                out.append(x)
            else:
                stack.append(left[x - n])
                stack.append(right[x - n])
        return out

    # condensed tree: cluster 0 is the root. A split whose two sides both hold min_cluster_size points gives birth to two clusters;
    # otherwise the small side's points fall out of the cluster at that level and the cluster lives on in the large side.
    birth = [0.0]            # lambda = 1 / distance at which the cluster appeared
    up = [-1]                # parent cluster
    stability = [0.0]
    kids = [[]]
    point_cluster = np.zeros((n,), np.int64)
    stack = [(2 * n - 2, 0)]
    while stack:
        node, c = stack.pop()
        if node < n:         # a single point that outlived its cluster's last split
            continue
        t = node - n
        lam = 1.0 / w[t] if w[t] > 0.0 else np.inf
        a, b = left[t], right[t]
        sa, sb = size[a], size[b]
        if sa >= m and sb >= m:
            for child, sz in ((a, sa), (b, sb)):
                birth.append(lam)
                up.append(c)
                stability.append(0.0)
                kids.append([])
                kids[c].append(len(birth) - 1)
                stability[c] += (lam - birth[c]) * sz
                stack.append((child, len(birth) - 1))
        else:
            for child, sz in ((a, sa), (b, sb)):
                if sz >= m:
                    stack.append((child, c))
                else:
                    pts = leaves(child)
                    point_cluster[pts] = c
                    stability[c] += (lam - birth[c]) * sz
    k = len(birth)

    # excess of mass, children before parents (a child is always born after its parent); the root is never a cluster
    selected = [True] * k
    selected[0] = False
    best = list(stability)
    for c in range(k - 1, 0, -1):
        below = sum(best[x] for x in kids[c])
        if kids[c] and stability[c] < below:
            selected[c] = False
            best[c] = below
        else:
            stack = list(kids[c])
            while stack:
                x = stack.pop()
                selected[x] = False
                stack.extend(kids[x])

    eps = float(cluster_selection_epsilon or 0.0)
    if eps > 0.0 and k > 1:
        def born_at(c):      # distance at which the cluster appeared
            return 1.0 / birth[c] if birth[c] > 0.0 else np.inf

        final, covered = [False] * k, [False] * k
        for c in range(1, k):
            if not selected[c] or covered[c]:
                continue
            top = c
            if born_at(c) < eps:
                while up[top] != 0 and born_at(top) < eps:
                    top = up[top]
            final[top] = True
            stack = list(kids[top])
            while stack:
                x = stack.pop()
                covered[x] = True
                stack.extend(kids[x])
        selected = [final[c] and not covered[c] for c in range(k)]

    number, nxt = [-1] * k, 0
    for c in range(1, k):
        if selected[c]:
            number[c] = nxt
            nxt += 1
    resolved = [-1] * k      # cluster -> label of its nearest selected ancestor-or-self
    for c in range(1, k):
        resolved[c] = number[c] if selected[c] else resolved[up[c]]
    labels[:] = np.asarray(resolved, np.int64)[point_cluster]
    return labels


def _centroid(rows):
    """clusterer.py:393-394: the normalised float32 mean."""
    c = np.mean(rows, axis=0).astype(np.float32)
    return c / (np.linalg.norm(c) + 1e-10)


def _as_centroid(value):
    if isinstance(value, dict):
        value = value["centroid"]
    if isinstance(value, (bytes, bytearray, memoryview)):
        value = np.frombuffer(value, dtype=np.float32)
    return np.asarray(value, np.float32)


class FaceClusterer:
    """The clustering and person-matching rules of the reference's FaceClusterer, on an engine instead of a database.

    engine: a facet_amd.Engine (anything with mreach_mst / cosine_best_match)."""

    def __init__(self, engine, min_faces=2, min_samples=None, auto_merge_distance=0.15, merge_threshold=0.6):
        self.engine = engine
        self.min_faces = min_faces
        self.min_samples = min_samples if min_samples is not None else min(min_faces, 2)       # clusterer.py:70
        self.cluster_selection_epsilon = auto_merge_distance if auto_merge_distance > 0 else None   # :72
        self.merge_threshold = merge_threshold

    @property
    def euclidean_epsilon(self):
        """clusterer.py:163-165: cosine distance -> euclidean distance between unit vectors."""
        return float(np.sqrt(2 * self.cluster_selection_epsilon)) if self.cluster_selection_epsilon else 0.0

    def cluster_embeddings(self, embeddings):
        """float32 [n,d] raw embeddings -> int64 [n] labels, noise = -1 (steps 2-3 of cluster_faces)."""
        e = np.ascontiguousarray(embeddings, dtype=np.float32)
        n = e.shape[0] if e.ndim == 2 else 0
        if n < self.min_faces or n < 2:                       # :151-153
            return np.full((n,), -1, np.int64)
        if self.engine is None:
            raise RuntimeError("FaceClusterer needs an engine: the clustering sweeps run on the GPU only")
        eu, ev, ew, _, _ = self.engine.mreach_mst(e, self.min_samples, normalise=True)
        return hdbscan_labels(n, eu, ev, ew, self.min_faces, self.euclidean_epsilon)

    def assign_persons(self, labels, embeddings_normalised, face_ids, existing_persons=None):
        """clusterer.py:364-446 without the SQL. labels [n], embeddings_normalised [n,d], face_ids [n];
        existing_persons: {person_id: centroid (array, bytes or {'centroid': ...})} in the order the reference would read them.
        -> ({face_id: person key}, new_persons): the key is an existing person's id or ('new', i) for new_persons[i] =
        {'centroid': bytes, 'representative_face_id': id, 'face_count': int, 'face_ids': [...]}. Noise faces get no entry."""
        emb = np.asarray(embeddings_normalised)
        face_ids = list(face_ids)
        clusters = {}
        for fid, label in zip(face_ids, labels):
            if label >= 0:
                clusters.setdefault(int(label), []).append(fid)
        position = {fid: i for i, fid in enumerate(face_ids)}
        items = [(ids, emb[[position[f] for f in ids]]) for ids in clusters.values()]
        centroids = [_centroid(rows) for _, rows in items]
        sims = idx = None
        pids = list(existing_persons.keys()) if existing_persons else []
        if pids and centroids:
            existing = np.stack([_as_centroid(existing_persons[p]) for p in pids])
            sims, idx = self.engine.cosine_best_match(np.stack(centroids), existing)
        assignment, new_persons = {}, []
        for i, ((ids, rows), centroid) in enumerate(zip(items, centroids)):
            # "similarity > best so far, starting at the threshold": the first person of largest similarity, if above it
            if sims is not None and float(sims[i]) > self.merge_threshold:
                key = pids[int(idx[i])]
            else:
                rep = ids[int(np.argmin(np.linalg.norm(rows - centroid, axis=1)))]
                new_persons.append({"centroid": centroid.tobytes(), "representative_face_id": rep, "face_count": len(ids),
                                    "face_ids": list(ids)})
                key = ("new", len(new_persons) - 1)
            for fid in ids:
                assignment[fid] = key
        return assignment, new_persons

    def match_face_to_person(self, embedding_bytes, persons, threshold=None):
        """clusterer.py:480-520: the person whose centroid is most similar to the embedding, above the threshold; else None.
        persons: {person_id: centroid} as for assign_persons."""
        if threshold is None:
            threshold = self.merge_threshold
        e = np.frombuffer(embedding_bytes, dtype=np.float32)
        if len(e) != 512 or not persons:
            return None
        pids = list(persons.keys())
        sims, idx = self.engine.cosine_best_match(e[None, :], np.stack([_as_centroid(persons[p]) for p in pids]))
        return pids[int(idx[0])] if float(sims[0]) > threshold else None
