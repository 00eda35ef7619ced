"""Duplicate detection over stored perceptual hashes: the mirror of reference utils/duplicate.py.

The reference compares all photos pairwise (a Python loop of n iterations, eight numpy passes each, :89-119), joins matches
transitively with a union-find, numbers the groups and marks the highest-scoring member of each as the lead. Here the pair
search is one engine call (`fe_hamming_pairs`: xor + popcount + compare per pair on the GPU, pairs back in ascending order);
the grouping below is the reference's own sequential logic on that short list. The pair search has no host version in this
package: without a GPU context it is an error, as everywhere else.
"""
import numpy as np

from .phash import from_hex


def max_hamming_distance(similarity_pct):
    """utils/duplicate.py:63 - float arithmetic on purpose (90 -> 6, 95 -> 3)."""
    return int(64 * (1 - similarity_pct / 100))


def group_duplicates(n, pairs, aggregates):
    """n rows, pairs: int [k,2] matching (i, j) in ascending order (the order the reference's loop meets them), aggregates: per-row
    score or None. -> (group_id: list[int | None], is_lead: list[int]) as the reference writes `duplicate_group_id` /
    `is_duplicate_lead` (utils/duplicate.py:121-162): groups of two or more are numbered from 1 in ascending order of their
    representative row, the lead is the first member with the highest `aggregate or 0.0`; rows outside any group get (None, 0).

    The representative of a group is whatever the reference's disjoint-set forest ends up with, and the numbering follows it, so
    the forest is rebuilt under the same rules: trees are merged by rank - the shallower one goes under the deeper one, and on
    equal ranks the tree of the pair's second row goes under the tree of its first row, whose rank grows by one. Lookups shorten
    the path they walk (each visited row is re-pointed to its grandparent), which changes no representative."""
    leader = list(range(n))          # leader[v] == v: v represents its tree
    depth = [0] * n                  # rank of a representative

    def representative(v):
        while True:
            up = leader[v]
            if up == v:
                return v
            leader[v] = leader[up]
            v = leader[v]

    for i, j in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        keep, drop = representative(i), representative(j)
        if keep == drop:
            continue
        if depth[keep] < depth[drop]:
            keep, drop = drop, keep
        elif depth[keep] == depth[drop]:
            depth[keep] += 1
        leader[drop] = keep

    members_of = {}
    for row in range(n):
        members_of.setdefault(representative(row), []).append(row)
    group_id, is_lead = [None] * n, [0] * n
    number = 0
    for rep in sorted(members_of):
        members = members_of[rep]
        if len(members) < 2:
            continue
        number += 1
        lead, lead_score = members[0], aggregates[members[0]] or 0.0
        for row in members[1:]:
            score = aggregates[row] or 0.0
            if score > lead_score:       # strictly: among equals the earliest row stays the lead
                lead, lead_score = row, score
        for row in members:
            group_id[row] = number
        is_lead[lead] = 1
    return group_id, is_lead


def find_duplicates(engine, hex_hashes, aggregates, similarity_pct=90):
    """hex_hashes: the `phash` strings of the rows to compare, in the caller's order (the reference orders by path and leaves rows
    without a hash out: so does the caller); aggregates: their scores (None allowed). -> (group_id, is_lead) per row."""
    n = len(hex_hashes)
    if len(aggregates) != n:
        raise ValueError(f"{n} hashes but {len(aggregates)} aggregates")
    pairs = engine.hamming_pairs(from_hex(hex_hashes), max_hamming_distance(similarity_pct)) if n else np.zeros((0, 2), np.int32)
    return group_duplicates(n, pairs, aggregates)
