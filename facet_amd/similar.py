"""Similar photos: the mirror of the reference's `/api/similar_photos` route (api/routers/gallery.py:410-539).

The reference scores one source photo against every other photo of the library in a Python loop - one numpy dot and one SQL
query per candidate - keeps the candidates whose total is positive, rounds the totals to four digits, sorts (stably, so equal
rounded totals stay in candidate order) and cuts to `limit`. Here the library is uploaded once and stays on the GPU; a query
is one sweep (`fe_similar_topk`, include/facet_engine.h) whose epilogue fuses the four factors in fp32 and keeps a short list.
The search has no host version in this package: without a GPU context it is an error, as everywhere else.

Exactness. The device score is fp32 and the reference sorts on a 4-digit rounding of its own arithmetic, so the device only
shortlists: the shortlist is re-scored below in the reference's arithmetic, rounded and sorted as the reference does, and a guard
proves that nothing outside the shortlist could have entered the first `limit` places - or the full tie set is fetched with
`fe_similar_pairs` and the same steps run on that.

The margin of the guard (`guard_margin`). Write u = 2^-24 (half an ulp of 1 in fp32), d for the embedding length.
  * cosine, device against exact (`cosine_error_bound`): rows are normalised in fp32 - the norm is a sum of d squares (relative
    error below 16 u for d <= 1024 with pairwise or matrix-core summation, one sqrt, one add of 1e-10, one division per component) -
    so a unit row is off by at most 20 u in length and u per component; the dot product of two unit rows accumulates d products
    in fp32 in some order, error at most d u sum|a_i b_i| <= d u. Together |cos_dev - cos| <= (d + 40) u.
  * the reference's own cosine is float32 too (np.dot and np.linalg.norm of float32 arrays): the same (d + 40) u against exact.
  * the fused score (`score_error_bound`, device against exact, per unit of weight): clip: (cos + 1) * 0.5 * wc is the cosine
    error halved plus three roundings of values <= 1 and the weight's conversion: ((d + 40) / 2 + 4) u. persons: one division, one
    product, the weight: 3 u. date: the day count is integer arithmetic on both sides, the tiers are exact constants, beyond 30
    days one division and one subtraction: 4 u. aggregate: the two values are rounded to fp32 (|a| <= 100 assumed: 200 u on the
    difference, 20 u after / 10), three operations, the weight: 24 u. The three additions of the running total (<= sum|w|): 3 u
    sum|w|.
  * the guard compares a device score with a reference total, so the cosine term enters twice:
        margin = 1e-4 + score_error_bound + |wc| (d + 40) u / 2
    where 1e-4 is the rounding step (a total moves by at most 0.5e-4 when it is rounded; a full step keeps a rounded tie inside).
For d = 768 and the default weights the error part is 2.6e-5; nothing here is fitted to observed scores.
"""
import os
from datetime import datetime

import numpy as np

from ._lib import FE_SIM_K_MAX, FE_SIM_NO_DATE, SimRows

U = 2.0 ** -24
SLACK = 12                       # shortlist entries asked for beyond `limit`: with the default limit of 20 this is K_MAX


def cosine_error_bound(d):
    return (d + 40) * U


def score_error_bound(d, weights):
    wc, wp, wd, ws = (abs(float(w)) for w in weights)
    return U * (wc * ((d + 40) / 2 + 4) + 3 * wp + 4 * wd + 24 * ws + 3 * (wc + wp + wd + ws))


def guard_margin(d, weights):
    return 1e-4 + score_error_bound(d, weights) + abs(float(weights[0])) * (d + 40) * U / 2


def thr_below(x):
    """The largest float32 that is <= x: a threshold handed to the device must not round upwards."""
    t = np.float32(x)
    return t if float(t) <= x else np.nextafter(t, np.float32(-np.inf))


def _seconds(date_taken):
    """'YYYY:MM:DD HH:MM:SS...' -> whole seconds on a fixed calendar origin, None when the reference's strptime would fail or the
    value is empty (gallery.py:486-503: such a photo takes no part in the date factor)."""
    if not date_taken:
        return None
    try:
        t = datetime.strptime(date_taken[:19], '%Y:%m:%d %H:%M:%S')
    except (ValueError, TypeError):
        return None
    delta = t - datetime(1970, 1, 1)
    return delta.days * 86400 + delta.seconds


class SimilarPhotoIndex:
    """The photos of a library with what the similarity score reads, resident on the engine's GPU.

    add(...) collects rows (in the order the reference's query meets them: the candidate order that decides ties); the first query
    after an add uploads everything once. Embeddings are stored L2-normalised in fp32 (x / (|x| + 1e-10)), so a sweep reads them
    in place. A photo without an embedding is never a candidate (the reference's `clip_embedding IS NOT NULL`; an empty blob is
    treated the same) but can be a source."""

    def __init__(self, engine):
        self.engine = engine
        self.paths, self.filenames, self.date_taken, self.aggregate, self.aesthetic = [], [], [], [], []
        self.raw, self.persons = [], []
        self._row_of = {}
        self._host = self._dev = None
        self.stats = {"topk_calls": 0, "guard_passed": 0, "guard_failed": 0, "pairs_calls": 0, "exhaustive": 0}

    def __len__(self):
        return len(self.paths)

    def add(self, paths, clip_embedding_bytes, date_taken, aggregate, person_ids, filenames=None, aesthetic=None):
        """Parallel sequences, one entry per photo: path, `clip_embedding` blob (float32 bytes) or None, `date_taken` string or None,
        `aggregate` or None, the person ids of the photo's faces (any iterable; ids of any hashable, sortable type)."""
        n = len(paths)
        filenames = filenames if filenames is not None else [os.path.basename(p) for p in paths]
        aesthetic = aesthetic if aesthetic is not None else [None] * n
        for seq in (clip_embedding_bytes, date_taken, aggregate, person_ids, filenames, aesthetic):
            if len(seq) != n:
                raise ValueError("add(): sequences of different lengths")
        for i in range(n):
            if paths[i] in self._row_of:
                raise ValueError(f"{paths[i]} is already in the index")
            self._row_of[paths[i]] = len(self.paths)
            self.paths.append(paths[i])
            self.filenames.append(filenames[i])
            self.date_taken.append(date_taken[i])
            self.aggregate.append(aggregate[i])
            self.aesthetic.append(aesthetic[i])
            blob = clip_embedding_bytes[i]
            self.raw.append(np.frombuffer(blob, dtype=np.float32) if blob else None)
            self.persons.append(frozenset(p for p in person_ids[i] if p is not None))
        self._host = self._dev = None

    # -- device side ------------------------------------------------------------------------------------------------------------
    def _resident(self):
        if self._dev is not None:
            return self._dev
        n = len(self.paths)
        dims = {r.shape[0] for r in self.raw if r is not None}
        if len(dims) != 1:
            raise ValueError(f"embeddings of lengths {sorted(dims)}: the index needs exactly one length")
        d = dims.pop()
        emb = np.zeros((n, d), np.float32)
        has = np.zeros(n, np.uint8)
        for i, r in enumerate(self.raw):
            if r is not None:
                emb[i] = r / (np.linalg.norm(r) + np.float32(1e-10))
                has[i] = 1
        secs = [_seconds(t) for t in self.date_taken]
        date = np.array([FE_SIM_NO_DATE if s is None else s for s in secs], np.int64)
        agg = np.array([0.0 if a is None else a for a in self.aggregate], np.float32)
        dense = {p: k for k, p in enumerate(sorted({p for ps in self.persons for p in ps}))}
        lists = [sorted(dense[p] for p in ps) for ps in self.persons]
        off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
        ids = np.array([k for l in lists for k in l], np.int32)
        self._host = SimRows(emb, has, date, agg, off, ids, normalise=False)
        self._dev = self.engine.upload_sim_rows(self._host)
        self.d = d
        return self._dev

    def _query_rows(self, rows):
        h = self._host
        if list(rows) == list(range(h.n)):
            return self._dev                              # every photo against every photo: both sides are the resident rows
        r = np.asarray(rows, np.int64)
        cnt = (h.person_off[r + 1] - h.person_off[r]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        ids = np.concatenate([h.person_ids[h.person_off[i]:h.person_off[i + 1]] for i in r] + [np.zeros(0, np.int32)]).astype(np.int32)
        return SimRows(h.emb[r], h.has_emb[r], h.date[r], h.aggregate[r], off, ids, normalise=False)

    # -- the reference's arithmetic ---------------------------------------------------------------------------------------------
    def _rescore(self, src, cand, weights):
        """Total and breakdown of candidate row `cand` for source row `src`, operation by operation as gallery.py:459-509 (numpy
        float32 dot and norms, Python floats for the rest). -> (total, factors): both unrounded; _entry rounds them."""
        wc, wp, wd, ws = weights
        breakdown = {}
        total = 0
        a, b = self.raw[src], self.raw[cand]
        if a is not None and b is not None:
            cosine = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-10))
            clip = (cosine + 1) / 2
            breakdown['clip'] = clip
            total += clip * wc
        ps, pc = self.persons[src], self.persons[cand]
        if ps and pc:
            psim = len(ps & pc) / max(len(ps), len(pc))
            breakdown['persons'] = psim
            total += psim * wp
        ts, tc = self.date_taken[src], self.date_taken[cand]
        if ts and tc:
            try:
                days = abs((datetime.strptime(ts[:19], '%Y:%m:%d %H:%M:%S') - datetime.strptime(tc[:19], '%Y:%m:%d %H:%M:%S')).days)
            except Exception:
                days = None
            if days is not None:
                dsim = 1.0 if days == 0 else 0.5 if days <= 7 else 0.2 if days <= 30 else max(0, 1 - days / 365)
                breakdown['date'] = dsim
                total += dsim * wd
        gs, gc = self.aggregate[src], self.aggregate[cand]
        if gs and gc:
            ssim = max(0, 1 - abs(gs - gc) / 10)
            breakdown['score'] = ssim
            total += ssim * ws
        return total, breakdown

    def _entry(self, cand, total, breakdown):
        return {'path': self.paths[cand], 'filename': self.filenames[cand], 'similarity': round(total, 4),
                'breakdown': {k: round(v, 3) for k, v in breakdown.items()},
                'aggregate': self.aggregate[cand], 'aesthetic': self.aesthetic[cand], 'date_taken': self.date_taken[cand]}

    def _ranked(self, src, cands, weights):
        """Candidate rows -> the reference's result entries for them: positive totals only, candidate order, then the stable sort
        on the rounded total."""
        out = []
        for cand in sorted(int(c) for c in cands):
            total, breakdown = self._rescore(src, cand, weights)
            if total > 0:
                out.append(self._entry(cand, total, breakdown))
        out.sort(key=lambda e: e['similarity'], reverse=True)
        return out

    # -- queries ----------------------------------------------------------------------------------------------------------------
    def similar(self, path_or_row, limit=20, clip_weight=0.4, person_weight=0.3, date_weight=0.2, score_weight=0.1, visible=None):
        """The reference's response for one source photo: {'source', 'weights', 'similar': [{path, filename, similarity, breakdown,
        aggregate, aesthetic, date_taken}]}, or {'error': 'Photo not found'}. visible: per-row flags of the viewer (None: all)."""
        return self.similar_batch([path_or_row], limit, clip_weight, person_weight, date_weight, score_weight, visible)[0]

    def similar_batch(self, rows, limit=20, clip_weight=0.4, person_weight=0.3, date_weight=0.2, score_weight=0.1, visible=None):
        """similar() for many sources (paths or row numbers) in one sweep; one response per source, in order."""
        weights = (clip_weight, person_weight, date_weight, score_weight)
        dev = self._resident()
        n = len(self.paths)
        vis = np.ones(n, bool) if visible is None else np.asarray(visible).astype(bool)
        eligible = (vis & self._host.has_emb.astype(bool)).astype(np.uint8)
        out = [None] * len(rows)
        src = []
        for i, r in enumerate(rows):
            row = self._row_of.get(r) if not isinstance(r, (int, np.integer)) else (int(r) if 0 <= int(r) < n else None)
            if row is None or not vis[row]:
                out[i] = {'error': 'Photo not found'}
            else:
                src.append((i, row))
        if src:
            lists = self._search([row for _, row in src], limit, weights, eligible, dev)
            for (i, row), entries in zip(src, lists):
                out[i] = {'source': self.paths[row],
                          'weights': {'clip': clip_weight, 'person': person_weight, 'date': date_weight, 'score': score_weight},
                          'similar': entries}
        return out

    def _search(self, src_rows, limit, weights, eligible, dev):
        margin = guard_margin(self.d, weights)
        q = self._query_rows(src_rows)
        q_self = np.asarray(src_rows, np.int32)
        n_elig = int(eligible.sum())
        results = [None] * len(src_rows)
        thr = np.full(len(src_rows), -np.inf, np.float32)           # per source: the threshold of the pair fetch, should one be needed
        if 1 <= limit < FE_SIM_K_MAX:
            k = min(FE_SIM_K_MAX, limit + SLACK)
            idx, score = self.engine.similar_topk(q, dev, k, weights, q_self=q_self, visible=eligible)
            self.stats["topk_calls"] += 1
            for j, row in enumerate(src_rows):
                got = idx[j][idx[j] >= 0]
                ranked = self._ranked(row, got, weights)
                others = n_elig - int(eligible[row])
                if len(got) == others:                                # the shortlist is every candidate there is
                    results[j] = ranked[:limit]
                elif len(got) < k:                                    # every candidate the device scores above 0 is here; the
                    self.stats["exhaustive"] += 1                     # rest total at most the error bound, yet may be positive
                    rest = np.setdiff1d(np.nonzero(eligible)[0], np.append(got, row))
                    results[j] = self._ranked(row, np.concatenate([got, rest]), weights)[:limit]
                elif len(ranked) >= limit and float(score[j][k - 1]) + margin < ranked[limit - 1]['similarity']:
                    self.stats["guard_passed"] += 1                   # nothing outside can reach the limit-th rounded total
                    results[j] = ranked[:limit]
                else:
                    self.stats["guard_failed"] += 1
                    if len(ranked) >= limit:
                        thr[j] = thr_below(ranked[limit - 1]['similarity'] - margin)
        todo = [j for j in range(len(src_rows)) if results[j] is None]
        while todo:
            # every candidate whose device score reaches thr; whatever is left out scores below thr on the device
            sub = self._query_rows([src_rows[j] for j in todo])
            if sub is dev:
                sub = q
            pairs, _ = self.engine.similar_pairs(sub, dev, thr[todo], weights, q_self=q_self[todo], visible=eligible)
            self.stats["pairs_calls"] += 1
            again = []
            for pos, j in enumerate(todo):
                row = src_rows[j]
                got = pairs[pairs[:, 0] == pos, 1]
                if thr[j] == -np.inf:                                 # the device dropped only scores <= 0: see `exhaustive` above
                    rest = np.setdiff1d(np.nonzero(eligible)[0], np.append(got, row))
                    got = np.concatenate([got, rest])
                ranked = self._ranked(row, got, weights)
                if thr[j] == -np.inf or limit < 1 or (len(ranked) >= limit and float(thr[j]) + margin <= ranked[limit - 1]['similarity']):
                    results[j] = ranked[:limit]
                else:                                                 # fewer than limit so far, or the cut is not yet proven
                    thr[j] = thr_below(ranked[limit - 1]['similarity'] - margin) if len(ranked) >= limit else -np.inf
                    again.append(j)
            todo = again
        return results
