"""What the tag-selection tests share: a plain-Python restatement of the reference's selection (models/tagger.py:103-114) on one row
of float32 similarities, and the cases both the host harness and the GPU kernel are held to, exactly."""
import numpy as np


def select_row(sims, tag_of_prompt, threshold, max_tags):
    """-> [(tag id, score as a Python float)] for one row: the reference's loop with tag ids for names. The ids first appear in
    ascending order, so the dict's insertion order is the id order."""
    tag_scores = {}
    for tag, sim in zip(tag_of_prompt, sims):                  # sim: np.float32, as `similarities.cpu().numpy()` yields
        if tag not in tag_scores or sim > tag_scores[tag]:
            tag_scores[tag] = float(sim)
    filtered = [(tag, score) for tag, score in tag_scores.items() if score >= threshold]
    filtered.sort(key=lambda x: x[1], reverse=True)
    return filtered[:max_tags]


def select(sims, tag_of_prompt, threshold, max_tags):
    """-> ids int32 [n, max_tags] padded with -1, scores float32 [n, max_tags] padded with 0, counts int32 [n]"""
    sims = np.asarray(sims, np.float32)
    top = [int(t) for t in tag_of_prompt]
    n = sims.shape[0]
    ids = np.full((n, max_tags), -1, np.int32)
    scores = np.zeros((n, max_tags), np.float32)
    counts = np.zeros(n, np.int32)
    for i in range(n):
        kept = select_row(sims[i], top, threshold, max_tags)
        counts[i] = len(kept)
        for k, (g, s) in enumerate(kept):
            ids[i, k], scores[i, k] = g, np.float32(s)
    return ids, scores, counts


def same(got, want):
    """exact equality of (ids, scores, counts); the scores bit for bit (+-inf included, no kept score is NaN)"""
    return all(np.array_equal(np.asarray(g), w) for g, w in zip(got, want)) and \
        np.array_equal(np.asarray(got[1]).view(np.uint32), want[1].view(np.uint32))


def groups(sizes):
    """tag_of_prompt of contiguous groups of the given sizes"""
    return np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)


def scattered(G, T, rng):
    """tag_of_prompt [T] over G tags whose prompts are not contiguous: a shuffled sequence that uses every tag, relabelled so that
    the ids first appear in ascending order"""
    seq = np.concatenate([rng.permutation(G), rng.integers(0, G, T - G)])
    rng.shuffle(seq)
    _, first = np.unique(seq, return_index=True)
    relabel = np.empty(G, np.int32)
    relabel[np.argsort(first)] = np.arange(G, dtype=np.int32)
    return relabel[seq]


F22 = np.float32(0.22)


def cases():
    """[(name, sims [n, T] float32, tag_of_prompt [T], threshold, max_tags)]: the issue's list, small enough for the Python loop."""
    rng = np.random.default_rng(20261021)
    out = []

    def dup_rows(n, T):      # many duplicates: 9 distinct values, so ties within tags, across tags and across the cut
        return (rng.integers(-4, 5, (n, T)) / 16).astype(np.float32)

    for G in (1, 61, 64, 65):
        sizes = rng.integers(1, 6, G)
        top = groups(sizes)
        T = len(top)
        for mt in sorted({1, min(5, G), G}):
            out.append((f"dup G={G} max_tags={mt}", dup_rows(5, T), top, 0.0, mt))
        out.append((f"dup G={G} n=1", dup_rows(1, T), top, 0.125, min(5, G)))
    # NaN first in a group stays (the tag is never kept), NaN later is skipped
    top = groups([3, 3, 2, 1])
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = np.array([[nan, 0.9, 0.8, 0.5, nan, 0.7, 0.3, nan, nan],
                     [0.1, nan, 0.4, nan, nan, nan, nan, 0.2, 0.6],
                     [inf, 0.0, 0.0, -inf, -inf, -inf, 0.5, inf, -inf],
                     [-inf, inf, nan, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25]], np.float32)
    for thr in (0.0, 0.25, float("-inf"), float("inf"), float("nan")):
        for mt in (1, 2, 4):
            out.append((f"nan/inf thr={thr} max_tags={mt}", rows, top, thr, mt))
    # np.float32(0.22) < 0.22 as doubles: rejected at 0.22, kept at float(np.float32(0.22))
    top = groups([2, 1, 2])
    rows = np.array([[F22, 0.1, F22, 0.0, np.nextafter(F22, np.float32(1))], [0.0, F22, 0.3, F22, F22]], np.float32)
    out.append(("threshold 0.22", rows, top, 0.22, 3))
    out.append(("threshold float32(0.22)", rows, top, float(F22), 3))
    # non-contiguous groups
    for G, T in ((7, 23), (61, 239), (65, 130)):
        top = scattered(G, T, rng)
        out.append((f"scattered G={G} T={T}", dup_rows(5, T), top, 0.0625, min(5, G)))
        out.append((f"scattered G={G} T={T} all", dup_rows(3, T), top, -1.0, G))
    out.append(("T=1", np.array([[0.5], [-0.5], [nan], [0.0], [inf]], np.float32), np.zeros(1, np.int32), 0.0, 1))
    return out


# ---- the inputs of tests/golden/tags_golden.json (made by tests/golden/make_tags_golden.py) -----------------------------------------
# Dyadic on purpose: every entry is k/64 with integer |k| <= 8 and d = 768, so every dot product is an integer multiple of 2^-12 of at
# most 768 * 64 < 2^24 units - exact in fp32 in any summation order. The reference's matmul, numpy and the MFMA GEMM give the same bits.
GOLDEN_D = 768


def _splitmix64(x):
    """numpy uint64 array -> the splitmix64 finaliser of every element (wrapping arithmetic; no numpy stream to depend on)"""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dyadic_rows(seed, stream, rows, amplitude):
    """int [len(rows), 768]: the integers k of the rows numbered `rows` of a stream, uniform in -amplitude .. amplitude"""
    rows = np.asarray(rows, np.uint64).reshape(-1, 1)
    col = np.arange(GOLDEN_D, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):
        x = (np.uint64(seed) << np.uint64(40)) + (np.uint64(stream) << np.uint64(36)) + rows * np.uint64(GOLDEN_D) + col
    h = _splitmix64(x) >> np.uint64(33)
    return (h % np.uint64(2 * amplitude + 1)).astype(np.int64) - amplitude


def golden_text(seed, T):
    return (dyadic_rows(seed, 0, np.arange(T), 8) / 64).astype(np.float32)


def golden_embeddings(seed, picks):
    """picks: [(candidate row, amplitude)] -> float32 [n, 768]"""
    return np.stack([(dyadic_rows(seed, amp, [row], amp)[0] / 64).astype(np.float32) for row, amp in picks])


# ---- realistic floats: unit rows, float64 as the judge --------------------------------------------------------------------------------
MARGIN = 1e-5      # the bound tests/test_mirrors_gpu.py holds fe_tag_similarities to: a decision closer than this may fall either way


def realistic(seed, n, sizes, d=768):
    """text [T, d]: unit rows. emb [n, d]: each the normalised sum of 1 to 4 text rows plus noise 2.5 to 4.5 times as long as one row, so
    the similarities to the chosen prompts spread over 0.2 .. 0.37, across the shipped thresholds. -> text, emb (float32), tag_of_prompt"""
    rng = np.random.default_rng(seed)
    top = groups(sizes)
    T = len(top)
    text = rng.standard_normal((T, d))
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    emb = np.empty((n, d))
    for i in range(n):
        pick = rng.choice(T, size=int(rng.integers(1, 5)), replace=False)
        noise = rng.standard_normal(d)
        emb[i] = text[pick].sum(0) + noise / np.linalg.norm(noise) * rng.uniform(2.5, 4.5)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    return text.astype(np.float32), emb.astype(np.float32), top


def judge64(sims64, sizes, threshold, max_tags):
    """The fold on float64 similarities [n, T] of contiguous groups (no NaN: the fold is the maximum). -> order: per row the kept tag
    ids, best first, ties by id, ALL of them; scores [n, G]; near [n] bool: a decision of the row is closer than MARGIN - a score
    against the threshold, or two neighbours among the first max_tags + 1 kept."""
    off = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    scores = np.maximum.reduceat(sims64, off, axis=1)
    order, near = [], np.zeros(len(scores), bool)
    for i, s in enumerate(scores):
        kept = np.flatnonzero(s >= threshold)
        kept = kept[np.argsort(-s[kept], kind="stable")]
        order.append(kept)
        head = s[kept[:max_tags + 1]]
        near[i] = bool((np.abs(s - threshold) < MARGIN).any() or (len(head) > 1 and (-np.diff(head) < MARGIN).any()))
    return order, scores, near
