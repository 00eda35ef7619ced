"""Test helpers for the similarity sweeps: a float64 brute force of the two engine calls' contracts, a numpy stand-in engine built
on it (for the host tests: no GPU, scores perturbed inside the fp32 bound), and seeded inputs."""
import numpy as np

from facet_amd._lib import FE_SIM_K_MAX, FE_SIM_NO_DATE, SimRows


def normalise64(x):
    x = np.asarray(x, np.float64)
    return x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-10)


def _persons_matrix(rows, width):
    m = np.zeros((rows.n, width), np.float64)
    if rows.person_off is not None:
        for r in range(rows.n):
            m[r, rows.person_ids[rows.person_off[r]:rows.person_off[r + 1]]] = 1.0
    return m


def brute_scores(q, c, weights=(0.4, 0.3, 0.2, 0.1), cosine=False, q_self=None, visible=None, upper=False):
    """SimRows (host) x SimRows -> (score float64 [nq,n], eligible bool [nq,n]): the header's formula in float64; eligible is False
    for the query itself, invisible candidates and (upper) candidates at or below the query. The s <= 0 rule is left to the caller."""
    qe = normalise64(q.emb) if q.normalise else q.emb.astype(np.float64)
    ce = normalise64(c.emb) if c.normalise else c.emb.astype(np.float64)
    cos = qe @ ce.T
    elig = np.ones(cos.shape, bool)
    if q_self is not None:
        qs = np.asarray(q_self)
        elig[np.nonzero(qs >= 0)[0], qs[qs >= 0]] = False
    if visible is not None:
        elig &= np.asarray(visible).astype(bool)[None, :]
    if upper:
        elig &= np.arange(c.n)[None, :] > np.arange(q.n)[:, None]
    if cosine:
        return cos, elig
    wc, wp, wd, ws = (float(v) for v in weights)
    has = np.ones(q.n) if q.has_emb is None else q.has_emb.astype(np.float64)
    s = wc * (cos + 1.0) / 2.0 * has[:, None]
    if q.person_off is not None and c.person_off is not None:
        width = int(max(q.person_ids.max(initial=0), c.person_ids.max(initial=0))) + 1
        mq, mc = _persons_matrix(q, width), _persons_matrix(c, width)
        nq_, nc_ = mq.sum(1), mc.sum(1)
        both = (nq_[:, None] > 0) & (nc_[None, :] > 0)
        s += wp * np.where(both, (mq @ mc.T) / np.maximum(np.maximum(nq_[:, None], nc_[None, :]), 1.0), 0.0)
    if q.date is not None and c.date is not None:
        both = (q.date != FE_SIM_NO_DATE)[:, None] & (c.date != FE_SIM_NO_DATE)[None, :]
        diff = np.where(both, q.date[:, None].astype(np.float64) - c.date[None, :].astype(np.float64), 0.0)   # exact below 2^53
        days = np.abs(np.floor(diff / 86400.0))            # abs(timedelta.days): the signed difference is floored first
        dsim = np.where(days == 0, 1.0, np.where(days <= 7, 0.5, np.where(days <= 30, 0.2, np.maximum(0.0, 1.0 - days / 365.0))))
        s += wd * np.where(both, dsim, 0.0)
    if q.aggregate is not None and c.aggregate is not None:
        qa, ca = q.aggregate.astype(np.float64), c.aggregate.astype(np.float64)
        both = ((qa == qa) & (qa != 0))[:, None] & ((ca == ca) & (ca != 0))[None, :]
        s += ws * np.where(both, np.maximum(0.0, 1.0 - np.abs(qa[:, None] - ca[None, :]) / 10.0), 0.0)
    return s, elig


class StandInEngine:
    """Honours Engine.similar_topk / similar_pairs / upload_sim_rows with numpy. Every score is moved by a seeded amount of up to
    `wobble` (the callers pass the derived fp32 bound), so that code relying on more than the contract fails here."""

    def __init__(self, wobble=0.0, seed=0):
        self.wobble = float(wobble)
        self.seed = seed
        self.calls = {"topk": 0, "pairs": 0}

    def upload_sim_rows(self, rows):
        return rows if isinstance(rows, SimRows) else SimRows(rows)

    def _scores(self, queries, candidates, weights, cosine, q_self, visible, upper=False):
        q, c = self.upload_sim_rows(queries), self.upload_sim_rows(candidates)
        s, elig = brute_scores(q, c, weights, cosine, q_self, visible, upper)
        rng = np.random.default_rng([self.seed, q.n, c.n])
        s = (s + rng.uniform(-self.wobble, self.wobble, s.shape)).astype(np.float32)
        keep = elig & ((s == s) if cosine else (s > 0))
        return s, keep

    def similar_topk(self, queries, candidates, k, weights=(0.4, 0.3, 0.2, 0.1), cosine=False, q_self=None, visible=None):
        assert 1 <= k <= FE_SIM_K_MAX
        self.calls["topk"] += 1
        s, keep = self._scores(queries, candidates, weights, cosine, q_self, visible)
        idx = np.full((s.shape[0], k), -1, np.int32)
        out = np.zeros((s.shape[0], k), np.float32)
        for r in range(s.shape[0]):
            cols = np.nonzero(keep[r])[0]
            order = cols[np.lexsort((cols, -s[r, cols].astype(np.float64)))][:k]
            idx[r, :len(order)] = order
            out[r, :len(order)] = s[r, order]
        return idx, out

    def similar_pairs(self, queries, candidates, thr, weights=(0.4, 0.3, 0.2, 0.1), cosine=False, q_self=None, visible=None, upper=False,
                      max_pairs=None):
        self.calls["pairs"] += 1
        s, keep = self._scores(queries, candidates, weights, cosine, q_self, visible, upper)
        t = np.asarray(thr, np.float32).reshape(-1)
        t = np.broadcast_to(t, (s.shape[0],)) if t.shape[0] == 1 else t
        hit = keep & (s >= t[:, None])
        qi, ci = np.nonzero(hit)
        return np.stack([qi, ci], 1).astype(np.int32), s[qi, ci]

    def similar_pairs_count(self, queries, candidates, thr, **kw):
        return len(self.similar_pairs(queries, candidates, thr, **kw)[1])


def random_rows(seed, n, d, persons=12, normalise=True, clusters=0):
    """Seeded SimRows with every kind of gap: rows without dates, aggregates (absent and 0), persons or embeddings."""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((n, d)).astype(np.float32)
    if clusters:
        centres = rng.standard_normal((clusters, d)).astype(np.float32)
        emb = (centres[rng.integers(0, clusters, n)] + 0.7 * emb).astype(np.float32)
    has = (rng.random(n) > 0.05).astype(np.uint8)
    date = (1_600_000_000 + rng.integers(0, 500 * 86400, n)).astype(np.int64)
    date[rng.random(n) < 0.1] = FE_SIM_NO_DATE
    agg = rng.uniform(1.0, 10.0, n).astype(np.float32)
    agg[rng.random(n) < 0.1] = 0.0
    agg[rng.random(n) < 0.03] = np.nan
    counts = rng.choice([0, 0, 1, 2, 3, 6], n)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ids = np.concatenate([np.sort(rng.choice(persons, cnt, replace=False)) for cnt in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return SimRows(emb, has, date, agg, off, ids, normalise=normalise)
