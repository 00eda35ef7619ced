"""Person merge suggestions: the mirror of reference faces/merge_analyzer.py (`get_merge_groups`, `suggest_person_merges`).

The reference compares every pair of person centroids in a double Python loop (one numpy dot each), joins the pairs at or above
the threshold with a union-find and reports min / max / avg similarity per group. Here the pair search is one engine call
(`fe_similar_pairs`: plain cosine, i < j only, on the fp32 matrix cores); the grouping below is the reference's own sequential
logic on that short list. The pair search has no host version in this package.

Exactness: the device cosine is fp32 in another summation order than numpy's, so the device is asked for every pair at or above
`threshold - margin`, margin = 2 (d + 40) 2^-24 (the device's and the reference's own fp32 error against the exact cosine, derived
in facet_amd/similar.py), and the host re-evaluates the returned pairs with the reference's expression and applies `>= threshold`
itself. A pair the device leaves out is below threshold - margin there, hence below the threshold for the reference.
"""
import numpy as np

from .similar import cosine_error_bound, thr_below


def _prepare(persons):
    """persons: dicts with id, name, face_count and centroid (float32 bytes or array; None / empty: skipped), in any order ->
    the reference's list: `ORDER BY face_count DESC` (ties keep the given order), centroids scaled as merge_analyzer.py:48-49."""
    rows = []
    for p in sorted((p for p in persons if p.get('centroid') is not None), key=lambda p: p['face_count'], reverse=True):
        c = p['centroid']
        c = np.frombuffer(c, dtype=np.float32) if isinstance(c, (bytes, bytearray, memoryview)) else np.asarray(c, dtype=np.float32)
        if c.size == 0:
            continue
        rows.append({'id': p['id'], 'name': p['name'], 'face_count': p['face_count'], 'centroid': c / (np.linalg.norm(c) + 1e-10)})
    return rows


def similar_person_pairs(engine, rows, threshold):
    """rows from _prepare -> [(i, j, similarity)] with i < j in ascending order, similarity = the reference's float(np.dot(...)),
    every pair with similarity >= threshold."""
    if len(rows) < 2:
        return []
    x = np.stack([r['centroid'] for r in rows]).astype(np.float32)
    margin = 2 * cosine_error_bound(x.shape[1])
    pairs, _ = engine.similar_pairs(x, x, thr_below(threshold - margin), cosine=True, upper=True)
    out = []
    for i, j in pairs.tolist():
        sim = float(np.dot(rows[i]['centroid'], rows[j]['centroid']))
        if sim >= threshold:
            out.append((i, j, sim))
    return out


def merge_groups(engine, persons, threshold=0.6):
    """-> the list `get_merge_groups` returns: groups of two or more persons joined through pairs at or above the threshold, each
    {'persons': [{id, name, face_count}] by face count descending, 'min_similarity', 'max_similarity', 'avg_similarity'}, groups by
    average similarity descending."""
    rows = _prepare(persons)
    n = len(rows)
    if n < 2:
        return []
    pairs = similar_person_pairs(engine, rows, threshold)
    # the reference's forest: full path compression on lookup, union by rank, the first row's tree wins equal ranks
    above = list(range(n))
    height = [0] * n

    def top(v):
        root = v
        while above[root] != root:
            root = above[root]
        while above[v] != root:
            above[v], v = root, above[v]
        return root

    pair_sim = {}
    for i, j, sim in pairs:
        a, b = top(i), top(j)
        if a != b:
            if height[a] < height[b]:
                a, b = b, a
            above[b] = a
            if height[a] == height[b]:
                height[a] += 1
        pair_sim[(i, j)] = sim
    members = {}
    for v in range(n):
        members.setdefault(top(v), []).append(v)       # groups in order of first appearance of their root, rows ascending
    groups = []
    for rows_of in members.values():
        if len(rows_of) < 2:
            continue
        sims = [pair_sim[(a, b)] for k, a in enumerate(rows_of) for b in rows_of[k + 1:] if (a, b) in pair_sim]
        people = [{'id': rows[v]['id'], 'name': rows[v]['name'], 'face_count': rows[v]['face_count']} for v in rows_of]
        people.sort(key=lambda p: p['face_count'], reverse=True)
        groups.append({'persons': people,
                       'min_similarity': min(sims) if sims else 0,
                       'max_similarity': max(sims) if sims else 0,
                       'avg_similarity': sum(sims) / len(sims) if sims else 0})
    groups.sort(key=lambda g: g['avg_similarity'], reverse=True)
    return groups


def merge_candidates(engine, persons, threshold=0.6):
    """-> the candidate list of `suggest_person_merges` (which prints it): [{'person1', 'person2', 'similarity'}] for every pair at
    or above the threshold, highest similarity first, equal similarities in pair order. person1 / person2 are {id, name, face_count}."""
    rows = _prepare(persons)
    strip = lambda r: {'id': r['id'], 'name': r['name'], 'face_count': r['face_count']}
    out = [{'person1': strip(rows[i]), 'person2': strip(rows[j]), 'similarity': sim} for i, j, sim in similar_person_pairs(engine, rows, threshold)]
    out.sort(key=lambda c: c['similarity'], reverse=True)
    return out
