"""Cases, float64 reference and error bounds for the two kernels of the Qwen-VL attention tile (facet_amd/csrc/vlm_attn_tile.h), launched
alone by fe_op_vlm_vis_attention (vlm_vis_attn_kernel<HD, NW>, HD 64 / 80) and fe_op_vlm_prefill_attention (vlm_attn_prefill_kernel, HD
128). Pure numpy; tests/test_vlm_attn_host.py (CPU) and tests/test_vlm_attn_gpu.py import it.

The reference is softmax attention in float64 on inputs ALREADY rounded to bf16, with the mask written out as a boolean matrix:
  vision    key j is visible to query i  iff  seg(j) == seg(i)                      (rows of the packed sequence, segments cu[s] .. cu[s+1])
  prefill   key j is visible to query i of sequence b  iff  pad[b] <= j <= qpos0 + i; a pad row (qpos0 + i < pad[b]) is all zeros
            KV head of query head h: h // (nh // nkv)
It returns the output, R = the largest spread (max - min) of the visible scaled scores of a row and S = the largest |scaled score|.

Three input families (after tests/test_attention_gpu.py):
  random   q, k, v ~ N(0, 1): the scaled scores have standard deviation 1, a spread of about 8 over a few hundred keys.
  spike    random, plus ONE key per segment list / per sequence that every query scores 12 (the rest score about 0 +- 1) and whose v row is
           50 (_spike_inputs of test_attention_gpu.py, with the planted components sqrt(12 / scale) because this tile applies the scale
           itself, and with the planted key made of the planted direction alone: over 300 keys and 900 query rows a random part of that
           key leaves some row under the 40 asserted below). Where the key is visible the output is about 50, elsewhere about 0: the reference is asserted > 40 / < 10, so a key
           masked in or out moves the result by O(1), not O(1 / Lk). Planted at keys 0, 31, 32 and the last key of a segment / sequence;
           vision: every placement at a segment's first or last key is also the next segment's first key / the previous one's last for the
           neighbour, which must not see it; prefill: at pad - 1 (masked) and pad (visible), and causally hidden from the rows before it.
  exact    q = 0: every visible probability is exp(0) = 1 exactly. v is one-hot by column, v[j][c] = 1 iff c == j mod HD (j the packed row
           of the vision kernel, the position of the prefill), so output entry c is count_c(visible keys) / n_visible: one key too many or
           too few on ANY row turns a 0 into 1 / n or c / n into (c +- 1) / (n +- 1).

Bounds (derived, not fitted; Vmax = max |v|):
  random, spike   |o - ref| <= 4 * 2^-9 * Vmax + 4 (4 + R + S) * 2^-23 * Vmax,  R asserted <= 24 (then S <= 24 too, asserted)
    This is the bf16 bound of test_attention_gpu.py's docstring plus the term S. Its terms here:
      * P is rounded to bf16 for the P V product (the exponentiated accumulator IS the MFMA operand; the row sum l is taken from the
        unrounded fp32 values). A bf16 rounding moves a value by between 2^-9 (just under a power of two) and 2^-8 (just above one)
        of itself at most: each product moves by <= 2^-8 p |v|, the normalised sum by <= 2^-8 Vmax. The output is rounded to bf16
        once: <= 2^-8 |o| <= 2^-8 Vmax. Together 2 * 2^-8 Vmax = 4 * 2^-9 Vmax - that file's term, which is the sum of the two worst
        cases (its "margin 2 each" is against the typical 2^-9, not the worst 2^-8).
      * __expf's argument x = s - m, |x| <= R, is scaled by log2(e) in fp32: a relative error 2^-24 of x, so p moves by R 2^-24
        relatively and the normalised output by at most twice that times Vmax; with the fp32 accumulation ("4") and the leading margin 4
        this is that file's fp32 term 4 (4 + R) 2^-23 Vmax.
      * The scale. kernels_attn.hip receives q already scaled; this tile computes st * scale in fp32 inside the kernel (softmax() of
        vlm_attn_tile.h), and 1 / sqrt(80), 1 / sqrt(128) are no powers of two. The products q k are exact in fp32 and the MFMA sum is
        correct to fp32 accumulation (inside the "4"), but the product with scale rounds s and, independently, the running maximum m:
        x = s - m moves by up to 2^-24 (|s| + |m|) <= 2^-23 S - in terms of |s|, not of the spread, so R does not cover it (a row of
        two keys scoring 3.0 and 3.5 has R = 0.5, S = 3.5). It needs a term of its own: p moves by 2^-23 S relatively, the normalised
        output by <= 2 * 2^-23 S Vmax, with the same margin 2 as the R term: 4 S 2^-23 Vmax. At S <= 24 it is 1.1e-5 Vmax beside
        7.8e-3 Vmax of the bf16 term: it widens the bound by less than 0.15 %. (At HD 64 scale = 2^-3 and the term is not needed; it is
        kept for one formula.)
  exact    |o - ref| <= 2^-8 |ref|, and an entry whose reference is 0 must be exactly 0. l and the counts are integers (exact in fp32;
           the counts are also exact as bf16 P V operands' sums, asserted on the CPU: every count is bf16-representable); the only
           roundings are 1 / l (2^-24), the product (2^-24) and the output's to bf16, at most 2^-8 / (1 + 2^-8) of the value:
           2^-8 - 2^-16 + 2^-23 < 2^-8.
  always   no NaN, no 768 (both hooks fill the output with 768 before the launch), prefill pad rows exactly 0.0.

Cases (the smallest shapes at which each branch of the kernels is taken; nothing here is the workload's own size).
Vision, hd in {64, 80} x heads in {1, 3}, segment lists:
  short  [1, 31, 32, 33, 63, 64, 4]   max_seg 64: NW = 2, one query block; 1, 1, 1, 2, 2, 2, 1 key tiles (64 keys are two tiles, not three):
                                      both buffer parities; last tiles of 1, 31 and 32 keys
  mixed  [65, 4, 128, 97, 1, 129]     NW = 4, two query blocks; blocks that return at once (q0 >= len); in the 97-key segment the last
                                      wave has ONE valid query
  long   [257] and [300, 64]          the full-attention blocks' shape: 9 and 10 key tiles, three query blocks
  The K / V chunk copy (32 keys x hd / 8 chunks of 16 bytes per tile, spread over the workgroup's threads): at hd 80 it is 320 chunks over
  128 or 256 threads, ragged in both launches (the `c < CHUNKS` branch of load / store runs with some threads idle); at hd 64 it is 256
  chunks, even in both. Hence every list runs at both head sizes.
Prefill, B = 2, one launch per case, (nh, nkv) in {(4, 2), (3, 1), (7, 1)}: every Lq of {2, 31, 32, 33, 64, 65, 127, 128, 129, 257, 300} at
  (4, 2) with two of the three qpos0 {0, 11 (the first workgroup's kend falls inside a tile), 133 (past a whole 128-key block)} each,
  max_seq alternating between Lk and Lk + 37 (rows of NaN behind the keys), the pad pairs (0, 0), (0, 1), (5, 37), (32, 33), (64, 0) in
  turn (the next one that fits pad < Lk), plus (130, 0) at Lq 257: a first workgroup whose queries are all padding and kt0 == nt, and a
  buffer parity shifted by kt0. Lq {2, 33, 129, 300} at (3, 1) and (7, 1). PREFILL_SHAPES below is the pruned list; random and exact run
  all of it, the spikes a list of their own (PREFILL_SPIKES)."""
import functools
import zlib

import numpy as np

R_CAP = 24.0
FILL = 768.0
SENTINEL = 1.0e4          # the q and k thirds of the fused rows the vision hook builds

VIS_LISTS = {"short": (1, 31, 32, 33, 63, 64, 4), "mixed": (65, 4, 128, 97, 1, 129), "long257": (257,), "long300": (300, 64)}
VIS_HEADS = ((64, 1), (64, 3), (80, 1), (80, 3))          # (hd, heads)
# (list, segment, key inside the segment): keys 0, 31, 32 and the last; every first / last key is the neighbour's "must not see" key
VIS_SPIKES = (("short", 3, 0), ("short", 3, 31), ("short", 3, 32), ("short", 5, 0), ("short", 5, 31), ("short", 5, 32), ("short", 5, 63), ("short", 0, 0),
              ("mixed", 2, 0), ("mixed", 2, 31), ("mixed", 2, 32), ("mixed", 2, 127), ("mixed", 3, 96), ("mixed", 4, 0), ("mixed", 5, 128),
              ("long257", 0, 256), ("long300", 0, 0), ("long300", 0, 31), ("long300", 0, 32), ("long300", 0, 299), ("long300", 1, 0), ("long300", 1, 63))
# the spikes run at 3 heads and both head sizes; these also at 1 head
VIS_SPIKES_1HEAD = (("short", 3, 32), ("mixed", 3, 96), ("long300", 0, 299), ("long300", 1, 0))

PREFILL_LQ = (2, 31, 32, 33, 64, 65, 127, 128, 129, 257, 300)
PREFILL_QPOS0 = (0, 11, 133)
PREFILL_HEADS = ((4, 2), (3, 1), (7, 1))
PREFILL_PADS = ((0, 0), (0, 1), (5, 37), (32, 33), (64, 0))
PAD_ALL_PADDING = (130, 0)          # at Lq 257


def bf16(x):
    """-> the nearest-even bf16 value of every element, as float32 (finite inputs)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32).reshape(x.shape)


def _prefill_shapes():
    """The pruned product: (nh, nkv, Lq, qpos0, extra rows of max_seq, pad pair)."""
    out, n = [], 0

    def add(nh, nkv, Lq, qpos0, pad=None):
        nonlocal n
        Lk = qpos0 + Lq
        if pad is None:
            pad = next(p for i in range(len(PREFILL_PADS)) for p in [PREFILL_PADS[(n + i) % len(PREFILL_PADS)]] if max(p) < Lk)
        out.append((nh, nkv, Lq, qpos0, 37 * (n % 2), pad))
        n += 1
    for i, Lq in enumerate(PREFILL_LQ):
        for t in range(2):
            add(4, 2, Lq, PREFILL_QPOS0[(i + t) % 3])
    add(4, 2, 257, 0, PAD_ALL_PADDING)
    add(4, 2, 257, 11, PAD_ALL_PADDING)
    for nh, nkv in PREFILL_HEADS[1:]:
        for i, Lq in enumerate((2, 33, 129, 300)):
            add(nh, nkv, Lq, PREFILL_QPOS0[(i + nh) % 3])
    return tuple(out)


PREFILL_SHAPES = _prefill_shapes()
# (nh, nkv, Lq, qpos0, extra, pad pair, spike key of each sequence)
PREFILL_SPIKES = (
    (4, 2, 65, 0, 0, (0, 0), (0, 0)), (4, 2, 65, 0, 37, (0, 0), (31, 32)), (4, 2, 65, 0, 0, (0, 0), (32, 31)), (4, 2, 65, 0, 37, (0, 0), (64, 64)),
    (4, 2, 2, 0, 0, (0, 1), (0, 0)),                                                # sequence 1: key pad - 1 = 0
    (4, 2, 129, 11, 37, (5, 37), (4, 36)), (4, 2, 129, 11, 0, (5, 37), (5, 37)), (4, 2, 129, 11, 37, (5, 37), (139, 0)), (4, 2, 129, 11, 0, (5, 37), (31, 32)),
    (4, 2, 33, 133, 0, (32, 33), (31, 32)), (4, 2, 33, 133, 37, (32, 33), (32, 33)), (4, 2, 33, 133, 0, (32, 33), (165, 133)), (4, 2, 33, 133, 37, (32, 33), (134, 164)),
    (4, 2, 257, 0, 0, (130, 0), (129, 0)), (4, 2, 257, 0, 37, (130, 0), (130, 31)), (4, 2, 257, 0, 0, (130, 0), (256, 256)),
    (4, 2, 128, 0, 37, (64, 0), (63, 32)), (4, 2, 128, 0, 0, (64, 0), (64, 127)),
    (3, 1, 33, 11, 37, (5, 37), (36, 37)), (3, 1, 129, 0, 0, (0, 0), (128, 32)), (7, 1, 33, 11, 0, (32, 33), (32, 32)), (7, 1, 300, 133, 37, (64, 0), (432, 63)),
)


def _vis_id(family, name, hd, heads, spike=None):
    return "vis-%s-%s-hd%d-h%d%s" % (family, name, hd, heads, "" if spike is None else "-s%dk%d" % spike)


def _prefill_id(family, s, spike=None):
    nh, nkv, Lq, qpos0, extra, pad = s
    return "prefill-%s-%dq%dkv-L%d-p%d-x%d-pad%d_%d%s" % (family, nh, nkv, Lq, qpos0, extra, pad[0], pad[1], "" if spike is None else "-j%d_%d" % spike)


@functools.lru_cache(maxsize=None)
def cases():
    """id -> case (a dict without arrays; inputs(id) and expect(id) make those)."""
    out = {}
    for family in ("random", "exact"):
        for name, lens in VIS_LISTS.items():
            for hd, heads in VIS_HEADS:
                cid = _vis_id(family, name, hd, heads)
                out[cid] = dict(id=cid, kernel="vis", family=family, list=name, lens=lens, hd=hd, heads=heads, spike=None)
    for spikes, head_sets in ((VIS_SPIKES, [(64, 3), (80, 3)]), (VIS_SPIKES_1HEAD, [(64, 1), (80, 1)])):
        for name, seg, key in spikes:
            for hd, heads in head_sets:
                cid = _vis_id("spike", name, hd, heads, (seg, key))
                out[cid] = dict(id=cid, kernel="vis", family="spike", list=name, lens=VIS_LISTS[name], hd=hd, heads=heads, spike=(seg, key))
    for family in ("random", "exact"):
        for s in PREFILL_SHAPES:
            cid = _prefill_id(family, s)
            out[cid] = dict(id=cid, kernel="prefill", family=family, nh=s[0], nkv=s[1], Lq=s[2], qpos0=s[3], max_seq=s[2] + s[3] + s[4], pad=s[5], spike=None)
    for s in PREFILL_SPIKES:
        cid = _prefill_id("spike", s[:6], s[6])
        out[cid] = dict(id=cid, kernel="prefill", family="spike", nh=s[0], nkv=s[1], Lq=s[2], qpos0=s[3], max_seq=s[2] + s[3] + s[4], pad=s[5], spike=s[6])
    return out


def case_ids(kernel, family):
    return [cid for cid, c in cases().items() if c["kernel"] == kernel and c["family"] == family]


def scale_of(hd):
    return float(np.float32(1.0) / np.sqrt(np.float32(hd)))          # the launch functions' 1.0f / sqrtf((float)hd)


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(cid):
    """The case's host arrays (float32 holding bf16 values, read-only).
    vision: dict(q, k, v [N, heads * hd], cu);  prefill: dict(q [B, Lq, nh * 128], k, v [B, nkv, Lk, 128], pad).
    The spike is _spike_inputs of test_attention_gpu.py: q and k are made orthogonal to a unit vector u per head, then every query gains
    a u and the planted key IS a u with a^2 scale = 12, and v of that key is 50."""
    c = cases()[cid]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    if c["kernel"] == "vis":
        hd, heads, cu = c["hd"], c["heads"], cu_of(c["lens"])
        N = int(cu[-1])
        q, k, v = (rng.normal(0, 1, (N, heads, hd)) for _ in range(3))
        if c["family"] == "spike":
            u = rng.normal(0, 1, (heads, hd))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            for x in (q, k):
                x -= (x * u).sum(-1, keepdims=True) * u
            a = np.sqrt(12.0 / scale_of(hd))
            q += a * u
            j = int(cu[c["spike"][0]]) + c["spike"][1]
            k[j] = a * u
            v[j] = 50.0
        elif c["family"] == "exact":
            q[:] = 0.0
            v[:] = 0.0
            v[np.arange(N), :, np.arange(N) % hd] = 1.0
        out = dict(q=bf16(q.reshape(N, -1)), k=bf16(k.reshape(N, -1)), v=bf16(v.reshape(N, -1)), cu=cu)
    else:
        nh, nkv, Lq, Lk, B = c["nh"], c["nkv"], c["Lq"], c["qpos0"] + c["Lq"], 2
        q = rng.normal(0, 1, (B, Lq, nh, 128))
        k, v = (rng.normal(0, 1, (B, nkv, Lk, 128)) for _ in range(2))
        if c["family"] == "spike":
            G = nh // nkv
            u = rng.normal(0, 1, (nkv, 128))          # one direction per KV head, shared by its group of query heads
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            uq = np.repeat(u, G, 0)
            q -= (q * uq).sum(-1, keepdims=True) * uq
            k -= (k * u[:, None]).sum(-1, keepdims=True) * u[:, None]
            a = np.sqrt(12.0 / scale_of(128))
            q += a * uq
            for b in range(B):
                k[b, :, c["spike"][b]] = a * u
                v[b, :, c["spike"][b]] = 50.0
        elif c["family"] == "exact":
            q[:] = 0.0
            v[:] = 0.0
            v[:, :, np.arange(Lk), np.arange(Lk) % 128] = 1.0
        out = dict(q=bf16(q.reshape(B, Lq, -1)), k=bf16(k), v=bf16(v), pad=np.asarray(c["pad"], np.int32))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the reference, and the modelled faults ------------------------------------------------------------------------------------------------
VIS_FAULTS = ("seg_last_key_dropped", "prev_seg_last_key_visible", "last_partial_tile_dropped", "v_from_k_third", "hd80_tail_unwritten")
PREFILL_FAULTS = ("causal_one_late", "causal_one_early", "qpos0_ignored", "pad_minus_1_visible", "pad_rows_not_zeroed", "kv_head_modulo")


def _attend(s, visible, v):
    """softmax over the visible keys of scaled scores s [.., Lq, Lk] times v [.., Lk, hd]; a row without a visible key gives zeros.
    -> (o, R, S)."""
    live = visible.any(-1)
    sv = np.where(visible, s, -np.inf)
    hi = np.where(live, sv.max(-1), 0.0)
    lo = np.where(visible, s, np.inf).min(-1)
    R = float(np.where(live, hi - lo, 0.0).max())
    S = float(np.abs(np.where(visible, s, 0.0)).max())
    p = np.exp(sv - hi[..., None])
    l = p.sum(-1, keepdims=True)
    o = (p / np.where(l > 0, l, 1.0)) @ v
    return o, R, S


def vis_reference(q, k, v, cu, hd, heads, fault=None):
    """float64 reference of the segment attention -> (o [N, heads * hd], R, S)."""
    assert fault is None or fault in VIS_FAULTS
    N = q.shape[0]
    cu = np.asarray(cu, np.int64)
    seg = np.searchsorted(cu, np.arange(N), side="right") - 1          # segment of every row
    within = np.arange(N) - cu[seg]                                    # its index inside the segment
    length = (cu[1:] - cu[:-1])[seg]
    visible = seg[:, None] == seg[None, :]                             # [query i][key j]
    if fault == "seg_last_key_dropped":
        visible &= (within != length - 1)[None, :]
    elif fault == "prev_seg_last_key_visible":
        visible |= (np.arange(N)[None, :] == (cu[seg] - 1)[:, None])
    elif fault == "last_partial_tile_dropped":
        visible &= (within < (length // 32) * 32)[None, :] | (length % 32 == 0)[None, :]
    h = lambda a: np.asarray(a, np.float64).reshape(N, heads, hd).transpose(1, 0, 2)
    vv = np.full((N, heads * hd), float(bf16([SENTINEL])[0])) if fault == "v_from_k_third" else v
    s = (h(q) @ h(k).transpose(0, 2, 1)) * scale_of(hd)
    o, R, S = _attend(s, visible[None], h(vv))
    o = o.transpose(1, 0, 2).copy()
    if fault == "hd80_tail_unwritten" and hd == 80:
        o[:, :, 64:] = FILL
    return o.reshape(N, heads * hd), R, S


def prefill_reference(q, k, v, nh, nkv, qpos0, pad, fault=None):
    """float64 reference of the prefill attention -> (o [B, Lq, nh * 128], R, S)."""
    assert fault is None or fault in PREFILL_FAULTS
    B, Lq, _ = q.shape
    Lk = k.shape[2]
    assert Lk == qpos0 + Lq
    i, j = np.arange(Lq)[:, None], np.arange(Lk)[None, :]
    kvh = np.arange(nh) % nkv if fault == "kv_head_modulo" else np.arange(nh) // (nh // nkv)
    o = np.zeros((B, nh, Lq, 128))
    R = S = 0.0
    for b in range(B):
        p = int(pad[b])
        qpos = (0 if fault == "qpos0_ignored" else qpos0) + i
        edge = qpos + 1 if fault == "causal_one_late" else qpos - 1 if fault == "causal_one_early" else qpos
        first = p - 1 if fault == "pad_minus_1_visible" else p
        visible = (j >= first) & (j <= edge) & (j < Lk)
        if fault == "pad_rows_not_zeroed":
            visible = np.where(qpos0 + i < p, j <= qpos0 + i, visible)
        else:
            visible &= (qpos0 + i >= p)                                # a pad row is all zeros (under every other fault too)
        qh = np.asarray(q[b], np.float64).reshape(Lq, nh, 128).transpose(1, 0, 2)
        kh, vh = np.asarray(k[b], np.float64)[kvh], np.asarray(v[b], np.float64)[kvh]
        s = (qh @ kh.transpose(0, 2, 1)) * scale_of(128)
        o[b], r, sm = _attend(s, visible[None], vh)
        R, S = max(R, r), max(S, sm)
    return o.transpose(0, 2, 1, 3).reshape(B, Lq, nh * 128), R, S


def reference(cid, fault=None):
    c, x = cases()[cid], inputs(cid)
    if c["kernel"] == "vis":
        return vis_reference(x["q"], x["k"], x["v"], x["cu"], c["hd"], c["heads"], fault)
    return prefill_reference(x["q"], x["k"], x["v"], c["nh"], c["nkv"], c["qpos0"], x["pad"], fault)


@functools.lru_cache(maxsize=None)
def expect(cid):
    """(ref, R, S, Vmax) of the case, computed once and read-only."""
    ref, R, S = reference(cid)
    ref.setflags(write=False)
    return ref, R, S, float(np.abs(inputs(cid)["v"]).max())


def model_output(cid, fault=None):
    """What a kernel with the named fault (None: a correct one) would return: the float64 result rounded to bf16."""
    return bf16(reference(cid, fault)[0])


def pad_rows(cid):
    """Boolean [B, Lq]: the prefill rows that are left padding."""
    c = cases()[cid]
    return c["qpos0"] + np.arange(c["Lq"])[None, :] < np.asarray(c["pad"])[:, None]


def spike_seen(cid):
    """Boolean over the output rows of a spike case ([N] vision, [B, Lq] prefill): True where the planted key is visible."""
    c = cases()[cid]
    if c["kernel"] == "vis":
        cu = cu_of(c["lens"])
        seg = np.searchsorted(cu, np.arange(cu[-1]), side="right") - 1
        return seg == c["spike"][0]
    pos = c["qpos0"] + np.arange(c["Lq"])[None, :]
    j, pad = np.asarray(c["spike"])[:, None], np.asarray(c["pad"])[:, None]
    return (j >= pad) & (j <= pos)


def bound(cid):
    """The absolute bound of a random / spike case (a scalar), or the relative one of an exact case (an array: 2^-8 |ref|)."""
    ref, R, S, vmax = expect(cid)
    if cases()[cid]["family"] == "exact":
        return 2.0 ** -8 * np.abs(ref)
    return 4.0 * 2.0 ** -9 * vmax + 4.0 * (4.0 + R + S) * 2.0 ** -23 * vmax


def premises(cid):
    """What the bounds assume of a case, from the reference alone -> list of violations (empty: the case is sound)."""
    c = cases()[cid]
    ref, R, S, vmax = expect(cid)
    bad = []
    if not np.isfinite(ref).all():
        bad.append("reference not finite")
    if R > R_CAP or S > R_CAP:
        bad.append("R %.2f, S %.2f above the cap %.0f" % (R, S, R_CAP))
    if c["family"] == "spike":
        seen = spike_seen(cid)
        rows = ref.reshape(seen.shape + (-1,))
        if seen.any() and rows[seen].min() <= 40.0:
            bad.append("spike visible but the reference is %.2f" % rows[seen].min())
        if (~seen).any() and np.abs(rows[~seen]).max() >= 10.0:
            bad.append("spike hidden but the reference reaches %.2f" % np.abs(rows[~seen]).max())
        if not (seen.any() and (~seen).any()) and c["kernel"] == "vis" and len(c["lens"]) > 1:
            bad.append("the spike is seen by all rows or by none")
    if c["family"] == "exact":
        if R != 0.0 or S != 0.0:
            bad.append("scores not zero")
        hd = c["hd"] if c["kernel"] == "vis" else 128
        # the numerators count_c(visible keys), counted here and not taken from the reference: whole numbers that bf16 holds
        counts = (_exact_counts_vis(c) if c["kernel"] == "vis" else _exact_counts_prefill(c)).reshape(-1, hd)
        if not np.array_equal(bf16(counts.astype(np.float32)).astype(np.float64), counts) or counts.max() > 256:
            bad.append("a numerator is not representable in bf16")
        nvis = counts.sum(-1, keepdims=True)
        want = np.where(nvis > 0, counts / np.where(nvis > 0, nvis, 1), 0.0)
        if not np.allclose(ref.reshape(-1, hd), want, rtol=0, atol=1e-12):
            bad.append("the exact reference is not count / n_visible")
    return bad


def _exact_counts_vis(c):
    """count_c(visible keys) per (row, head, column), by counting - not through the reference."""
    cu, hd = cu_of(c["lens"]), c["hd"]
    N = int(cu[-1])
    out = np.zeros((N, c["heads"], hd))
    for s in range(len(c["lens"])):
        cnt = np.bincount(np.arange(cu[s], cu[s + 1]) % hd, minlength=hd)
        out[cu[s]:cu[s + 1]] = cnt
    return out


def _exact_counts_prefill(c):
    Lq, qpos0 = c["Lq"], c["qpos0"]
    out = np.zeros((2, Lq, c["nh"], 128))
    for b in range(2):
        for i in range(Lq):
            if qpos0 + i >= c["pad"][b]:
                out[b, i] = np.bincount(np.arange(c["pad"][b], qpos0 + i + 1) % 128, minlength=128)
    return out


def compare(cid, got):
    """got: the hook's output (any shape with the reference's size) -> (failures, worst err / bound)."""
    c = cases()[cid]
    ref = expect(cid)[0]
    got = np.asarray(got, np.float64).reshape(ref.shape)
    bad = []
    if np.isnan(got).any():
        bad.append("%d NaN" % int(np.isnan(got).sum()))
    if (got == FILL).any():
        bad.append("%d entries still hold the fill 768" % int((got == FILL).sum()))
    if c["kernel"] == "prefill":
        pr = got[pad_rows(cid)]
        if pr.size and (pr != 0.0).any():
            bad.append("%d non-zero entries in pad rows" % int((pr != 0.0).sum()))
    err, tol = np.abs(got - ref), bound(cid)
    if c["family"] == "exact":
        zero = ref == 0.0
        if (got[zero] != 0.0).any():
            bad.append("%d entries must be exactly 0, worst %.3e" % (int((got[zero] != 0.0).sum()), np.abs(got[zero]).max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.nan_to_num(np.where(zero, 0.0, err / np.where(zero, 1.0, tol)), nan=np.inf).max())
    else:
        ratio = float(np.nan_to_num(err, nan=np.inf).max() / tol)
    if ratio > 1.0:
        at = np.unravel_index(np.nan_to_num(err / np.where(tol > 0, tol, 1.0) if c["family"] == "exact" else err, nan=np.inf).argmax(), ref.shape)
        bad.append("worst err / bound %.3f at %s (got %.6g, ref %.6g)" % (ratio, at, got[at], ref[at]))
    return bad, ratio
