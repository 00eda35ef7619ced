"""numpy emulations (no torch) of the VLM decoders' row kernels, in the kernels' own float32 arithmetic and order, and the cases that
tests/test_vlm_rows_gpu.py runs and tests/test_vlm_rows_host.py checks on the CPU.

What is emulated (facet_amd/csrc/model_vlm.hip, model_vlm_vision.hip; the library is built with -ffp-contract=off, so every fp32
operation below is one IEEE operation, and numpy float32 reproduces it bit for bit):

  vlm_rmsnorm_kernel, vlm_add_rmsnorm_kernel   one wave per row. Lane l starts from ss = 0 and adds, for i = 4 l, 4 l + 256, ... < d,
      (x0^2 + x1^2) + (x2^2 + x3^2) of the four values at i (`lane_sums`); the 64 lane sums are merged by the xor butterfly
      ss += shfl_xor(ss, o), o = 32, 16, 8, 4, 2, 1 (`butterfly`; a + b == b + a, so every lane ends with the same bits);
      rs = rsqrtf(ss / float(d) + eps); n = bf16(w * bf16(x * rs)).
      add_rmsnorm first stores r = bf16(x + y) (DS: r = bf16(r + ds[slot]) on rows with slot >= 0) and norms the ROUNDED r.
  vlm_finish_add_rmsnorm_kernel with part == nullptr and 0 splits (the "few rows" form)   its own order: one 1024-thread workgroup per
      row; thread t adds the quads at i = 4 t, 4 t + 4096, ...; each of the 16 waves runs the same butterfly over its 64 threads; lane 0
      of wave k stores red[k]; every thread then sums tot = ((0 + red[0]) + red[1]) + ... + red[15] in index order. x is rewritten as
      bf16(x + bf16(0)): its own bits, except that -0 becomes +0.
  vlm_add_kernel           bf16(x + y)
  vlm_silu_mul_kernel      bf16(bf16(x / (1 + expf(-x))) * u)
  vlm_rope_cache_kernel    frequency d < 64 reads the position component of its chunk (d < s0: temporal, d < s0 + s1: height, else width);
      ang = float(pos) * inv_freq[d]; c = bf16(cosf(ang)), s = bf16(sinf(ang));
      o[d] = bf16(bf16(x[d] c) + bf16(-x[d + 64] s)), o[d + 64] = bf16(bf16(x[d + 64] c) + bf16(x[d] s)); V is copied.
  vlm3_qk_rope_cache_kernel    q / k heads first take y = bf16(w * bf16(x * rs)), rs = rsqrtf(ss / 128 + eps), ss the butterfly over the
      lanes' x[l]^2 + x[l + 64]^2; frequency j reads height if j % 3 == 1 and j < 3 s1, width if j % 3 == 2 and j < 3 s2, else temporal.
  vlm_kv_store_row         FE_VLM_KV_E4M3: codes and scale of facet_amd.weights.quantize_e4m3_rows on the bf16 row (a row with a NaN or
      Inf: codes 0x7F, scale 1); FE_VLM_KV_BF16_E4M3: the dequantised image of that.
  vlm_vis_rope_kernel<64|80>   fp32 throughout, one rounding: bf16(x1 c - x2 s), bf16(x2 c + x1 s) with c = cosf(ang), s = sinf(ang).

bf16 rounds to nearest even exactly where `bf16(...)` stands above.

The four device functions cosf, sinf, rsqrtf and expf are the only steps that cannot be restated bit for bit. Each is evaluated in
float64 and rounded to fp32, and carried as three variants: that value and the values K[fn] fp32 ulps below and above it (`dev`;
cosf(0), sinf(0) and expf(0) are exact, and an infinite result stays infinite). An emulation runs once per combination of the variants
that reach an output (`Var`): an element whose bits agree over all combinations is FIRM and the GPU must give exactly those bits; any
other is FRAGILE and the GPU must land between the smallest and the largest variant result. Every function involved is monotone in each
device-function value between the variants (a product with a fixed factor, a sum, a rounding), so the extremes bound what any result
inside the +-K ulp interval can give. No other tolerance exists. K: the HIP math API's accuracy table is not shipped with the ROCm
installation, so the issue's starting value of 2 ulp is used for all four; DESIGN.md records the smallest k that passes on the GPU.

The float64 guards (`guard_*`) protect against a mistake in the emulations themselves: the plain formula in float64 with a bound summed
from the listed roundings (a bf16 rounding: at most 2^-8 of the value, half an ulp at 8 significant bits)."""
import functools
import itertools

import numpy as np

from facet_amd.weights import dequantize_e4m3_rows, quantize_e4m3_rows

f32 = np.float32
K = dict(cosf=2, sinf=2, rsqrtf=2, expf=2)          # fp32 ulps either side of the correctly rounded value
FRAGILE_CAP = 0.02
FILL = 0xA5                                          # the byte the hook fills the caches and scale arrays with
KV_FORMATS = ("bf16", "fp8", "bf16_e4m3")


# ---- number formats ---------------------------------------------------------------------------------------------------------------
def bf16(x):
    """float32 -> the nearest-even bf16 value, as float32 (NaN stays NaN, Inf stays Inf)."""
    x = np.ascontiguousarray(x, f32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(f32)
    return np.where(np.isnan(x), f32(np.nan), r).astype(f32)


def bits16(x):
    """bf16 values held in float32 -> their bit patterns (uint16)."""
    return (np.ascontiguousarray(x, f32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits16(u):
    return (np.ascontiguousarray(u, np.uint16).astype(np.uint32) << 16).view(f32)


def ulps(v, n):
    """v moved n fp32 ulps (n < 0: down); non-finite values stay."""
    v = np.asarray(v, f32)
    out = v.copy()
    for _ in range(abs(int(n))):
        out = np.nextafter(out, f32(np.inf) if n > 0 else f32(-np.inf))
    return np.where(np.isfinite(v), out, v).astype(f32)


def dev(fn, arg, off):
    """A device function at fp32 arguments: float64 value rounded to fp32, moved off * K[fn] ulps (off in -1, 0, 1)."""
    arg = np.asarray(arg, f32)
    a = arg.astype(np.float64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        v = dict(cosf=np.cos, sinf=np.sin, expf=np.exp, rsqrtf=lambda t: 1.0 / np.sqrt(t))[fn](a).astype(f32)
    if not off:
        return v
    # exact whatever the implementation: cosf(0), sinf(0), expf(0), and the 0 or Inf an infinite argument or an overflow gives
    exact = ~np.isfinite(arg) | ~np.isfinite(v) | ((arg == 0) & (fn != "rsqrtf"))
    return np.where(exact, v, ulps(v, off * K[fn]))


class Var:
    """The results of one output over all variant combinations: all [n_comb, ...] float32, combination 0 = no offsets."""

    def __init__(self, stack):
        self.all = np.stack(stack).astype(f32)
        self.center = self.all[0]
        b = self.all.view(np.uint32)
        self.firm = (b == b[0]).all(0)
        with np.errstate(invalid="ignore"):
            self.lo, self.hi = self.all.min(0), self.all.max(0)

    @property
    def n_fragile(self):
        return int((~self.firm).sum())


def variants(fns, emulate):
    """emulate(off: {fn: -1|0|1}) -> tuple of arrays; -> tuple of Var over the product of offsets of `fns` (all-zero first)."""
    combos = sorted(itertools.product((0, -1, 1), repeat=len(fns)), key=lambda c: any(c))
    assert not any(combos[0])
    outs = [emulate(dict(zip(fns, c))) for c in combos]
    return tuple(Var([o[i] for o in outs]) for i in range(len(outs[0])))


def compare(got, var, what=""):
    """The two rules. got: float32 array of bf16 values. -> list of failure strings (empty: accepted)."""
    got = np.ascontiguousarray(got, f32)
    assert got.shape == var.center.shape, (what, got.shape, var.center.shape)
    bad = []
    firm = var.firm
    # (a NaN is a NaN: IEEE 754 fixes neither its sign nor its payload)
    gb, wb = (np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)) for a in (got, var.center))
    if not np.array_equal(gb[firm], wb[firm]):
        d = (gb != wb) & firm
        i = tuple(np.argwhere(d)[0])
        bad.append("%s: %d of %d firm elements differ in bits, first at %s: got %r, want %r" % (what, int(d.sum()), int(firm.sum()), i, got[i], var.center[i]))
    with np.errstate(invalid="ignore"):
        out = ~firm & ~((got >= var.lo) & (got <= var.hi))
    if out.any():
        i = tuple(np.argwhere(out)[0])
        bad.append("%s: %d fragile elements outside their variants, first at %s: got %r, range %r .. %r" % (what, int(out.sum()), i, got[i], var.lo[i], var.hi[i]))
    return bad


def half_ulp_bf16(v):
    """Half an ulp of the bf16 grid at |v| (0 at 0): 2^(floor(log2 |v|) - 8)."""
    v = np.abs(np.asarray(v, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    return np.where(v > 0, 2.0 ** (e - 8), 0.0)


def worst(got, ref, bound):
    """max |got - ref| / bound over the finite references."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    ok = np.isfinite(ref) & np.isfinite(bound)
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        r = np.abs(got - ref)[ok] / bound[ok]
    return float(np.nan_to_num(r, nan=np.inf).max())


# ---- reductions -------------------------------------------------------------------------------------------------------------------
def butterfly(ss):
    """ss [..., 64] float32 lane values -> what every lane holds after ss += shfl_xor(ss, o), o = 32 .. 1."""
    ss = np.asarray(ss, f32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[..., lane ^ o]
    assert ss.dtype == f32
    return ss[..., 0]


def lane_sums(v, lanes):
    """v [rows, d] float32 -> [rows, lanes]: thread t's sum over i = 4 t, 4 t + 4 lanes, ... of (x0^2 + x1^2) + (x2^2 + x3^2).
    (The zero padding stands for the trips a thread does not make: adding 0 to a non-negative sum changes no bit.)"""
    v = np.asarray(v, f32)
    rows, d = v.shape
    assert d % 4 == 0
    trips = -(-d // (4 * lanes))
    p = np.zeros((rows, trips * lanes * 4), f32)
    p[:, :d] = v
    p = p.reshape(rows, trips, lanes, 4)
    q = (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + (p[..., 2] * p[..., 2] + p[..., 3] * p[..., 3])
    ss = np.zeros((rows, lanes), f32)
    for j in range(trips):
        ss = ss + q[:, j]
    assert ss.dtype == f32
    return ss


def sumsq_wave(v):
    return butterfly(lane_sums(v, 64))


def sumsq_few_rows(v):
    red = butterfly(lane_sums(v, 1024).reshape(len(v), 16, 64))          # [rows, 16]
    tot = np.zeros(len(v), f32)
    for k in range(16):
        tot = tot + red[:, k]
    return tot


# ---- the row kernels --------------------------------------------------------------------------------------------------------------
def emu_norm(r, w, eps, off, sumsq=sumsq_wave, read=None):
    """n = bf16(w * bf16(r * rs)); `read` (a fault model): the values the norm reads instead of r."""
    v = np.asarray(r if read is None else read, f32)
    rs = dev("rsqrtf", sumsq(v) / f32(v.shape[1]) + f32(eps), off["rsqrtf"])[:, None]
    return bf16(np.asarray(w, f32) * bf16(v * rs))


def emu_add(x, y):
    return bf16(np.asarray(x, f32) + np.asarray(y, f32))


def emu_add_rmsnorm(x, y, w, eps, off, slot=None, ds=None, fault=None):
    """-> (r, n); n is None without w."""
    s = np.asarray(x, f32) + np.asarray(y, f32)
    r = bf16(s)
    read = None
    if slot is not None:
        sl = np.asarray(slot).copy()
        if fault == "ds_minus1_as_0":
            sl[sl < 0] = 0
        on = sl >= 0
        r[on] = bf16(r[on] + np.asarray(ds, f32)[sl[on]])
    elif fault == "sum_unrounded":
        read = s
    return r, (None if w is None else emu_norm(r, w, eps, off, read=read))


def emu_few_rows(x, w, eps, off):
    r = bf16(np.asarray(x, f32) + bf16(f32(0)))
    return r, emu_norm(r, w, eps, off, sumsq=sumsq_few_rows)


def emu_silu_mul(g, u, off, fault=None):
    g, u = np.asarray(g, f32), np.asarray(u, f32)
    with np.errstate(over="ignore"):
        s = g / (f32(1) + dev("expf", -g, off["expf"]))
    assert s.dtype == f32
    return bf16((s if fault == "silu_unrounded" else bf16(s)) * u)


# ---- the rotary kernels -------------------------------------------------------------------------------------------------------------
def components(family, sections):
    """The position component (0 temporal, 1 height, 2 width) of each of the 64 frequencies. sections: the two sizes the kernel reads."""
    j = np.arange(64)
    a, b = sections
    if family == "qwen2_5":
        return np.where(j < a, 0, np.where(j < a + b, 1, 2))
    return np.where((j % 3 == 1) & (j < 3 * a), 1, np.where((j % 3 == 2) & (j < 3 * b), 2, 0))


def emu_rope(c, off, fault=None):
    """One launch of a rope kernel on case c -> (q [rows, nh, 128], k [rows, nkv, 128], v [rows, nkv, 128]), bf16 values."""
    with np.errstate(invalid="ignore", over="ignore"):          # (the Inf rows of the e4m3 edge cases)
        return _emu_rope(c, off, fault)


def _emu_rope(c, off, fault):
    nh, nkv, rows = c["nh"], c["nkv"], c["B"] * c["L"]
    x = np.asarray(c["qkv"], f32).reshape(rows, nh + 2 * nkv, 128)
    family, sections = c["family"], tuple(c["sections"])
    if fault == "section":
        sections = (sections[0] + 1, sections[1])
    if fault == "routing":
        # the other family's rule on this family's sections (qwen2_5 reads (temporal, height), qwen3 (height, width) sizes)
        comp = components("qwen3", (sections[1], 64 - sections[0] - sections[1])) if family == "qwen2_5" else components("qwen2_5", (64 - sum(sections), sections[0]))
    else:
        comp = components(family, sections)
    if fault == "swap_hw":
        comp = np.where(comp == 1, 2, np.where(comp == 2, 1, comp))
    p = np.asarray(c["pos"]).reshape(3, rows)[comp, np.arange(rows)[:, None]].astype(f32)          # [rows, 64]
    ang = p * np.asarray(c["inv_freq"], f32)
    assert ang.dtype == f32
    cs, sn = dev("cosf", ang, off["cosf"]), dev("sinf", ang, off["sinf"])
    cs = (cs if fault == "cos_unrounded" else bf16(cs))[:, None, :]
    sn = bf16(sn)[:, None, :]
    qk = x[:, :nh + nkv]
    x1, x2 = qk[..., :64], qk[..., 64:]
    if family == "qwen3":
        rs = dev("rsqrtf", butterfly(x1 * x1 + x2 * x2) / f32(128) + f32(c["eps"]), off["rsqrtf"])[..., None]
        qn, kn = (c["kn"], c["qn"]) if fault == "qn_kn" else (c["qn"], c["kn"])
        w = np.concatenate([np.broadcast_to(np.asarray(qn, f32), (nh, 128)), np.broadcast_to(np.asarray(kn, f32), (nkv, 128))])
        x1, x2 = bf16(w[:, :64] * bf16(x1 * rs)), bf16(w[:, 64:] * bf16(x2 * rs))
    c2, s2 = (np.roll(cs, 1, -1), np.roll(sn, 1, -1)) if fault == "freq_partner" else (cs, sn)
    rnd = (lambda t: t) if fault == "product_unrounded" else bf16
    o1 = bf16(rnd(x1 * cs) + bf16(-x2 * sn))
    o2 = bf16(bf16(x2 * c2) + bf16(x1 * s2))
    o = np.concatenate([o1, o2], -1)
    return o[:, :nh], o[:, nh:], x[:, nh + nkv:].copy()


def cache_rows(c, fault=None):
    """Index arrays (b, position) of the cache row each input row lands in."""
    L, rows = c["L"], c["B"] * c["L"]
    r = np.arange(rows)
    Lw = L + 1 if fault == "row_L" else L
    b, t = r // Lw, r - (r // Lw) * Lw
    start = c["start"] + (1 if fault == "start" else 0)
    return b, np.minimum(start + t, c["max_seq"] - 1)


def e4m3_candidates(var_rows):
    """var_rows [n_comb, 128]: one cache row under every variant combination -> (codes [n, 128] uint8, scales [n] float32) of every row the
    kernel may have quantised: each fragile element takes each of its variant values independently of the others (their device-function
    calls are independent). A row that holds a NaN or Inf in any combination: one candidate, codes 0x7F with scale 1."""
    if not np.isfinite(var_rows).all():
        return np.full((1, 128), 0x7F, np.uint8), np.ones(1, f32)
    b = var_rows.view(np.uint32)
    frag = np.flatnonzero((b != b[0]).any(0))
    choices = [np.unique(var_rows[:, i]) for i in frag]
    if np.prod([len(ch) for ch in choices], dtype=np.float64) > 4096:
        cands = np.unique(var_rows, axis=0)
    else:
        cands = np.repeat(var_rows[:1], max(1, int(np.prod([len(ch) for ch in choices]))), 0)
        for n, pick in enumerate(itertools.product(*choices)):
            cands[n, frag] = pick
    codes, exps = quantize_e4m3_rows(cands)
    return codes, np.ldexp(f32(1), np.asarray(exps).astype(np.int32)).astype(f32)


def raw_fill(fmt, shape):
    return np.full(shape, FILL if fmt == "fp8" else FILL * 0x0101, np.uint8 if fmt == "fp8" else np.uint16)


FILL_SCALE = np.full(1, FILL * 0x01010101, np.uint32).view(f32)[0]


class RopeExpect:
    """What one rope case must produce. q: Var [rows, nh, 128]; krows / vrows: Var [rows, nkv, 128] (the bf16 rows before the format)."""

    def __init__(self, c):
        self.c = c
        fns = ("cosf", "sinf", "rsqrtf") if c["family"] == "qwen3" else ("cosf", "sinf")
        self.q, self.krows, self.vrows = variants(fns, lambda off: emu_rope(c, dict(dict(rsqrtf=0), **off)))
        self.b, self.p = cache_rows(c)
        self._cand = {}

    def cand(self, which, row, head):
        key = (which, row, head)
        if key not in self._cand:
            self._cand[key] = e4m3_candidates((self.vrows if which == "v" else self.krows).all[:, row, head])
        return self._cand[key]

    def fragile_share(self, fmt):
        """Fragile elements over compared elements: q and both caches' written rows (and, fp8, their scales)."""
        c = self.c
        n = self.q.center.size + self.krows.center.size + self.vrows.center.size
        frag = self.q.n_fragile
        if fmt == "bf16":
            return (frag + self.krows.n_fragile + self.vrows.n_fragile) / n
        for which in "kv":
            for r in range(c["B"] * c["L"]):
                for h in range(c["nkv"]):
                    codes, sc = self.cand(which, r, h)
                    if len(codes) == 1:
                        continue
                    img = dequantize_e4m3_rows(codes, np.log2(sc).astype(np.int32)) if fmt == "bf16_e4m3" else codes
                    frag += int((img != img[0]).any(0).sum()) + (int((sc != sc[0]).any()) if fmt == "fp8" else 0)
        return frag / (n + (2 * c["B"] * c["L"] * c["nkv"] if fmt == "fp8" else 0))

    def check(self, fmt, q, k_raw, v_raw, k_scale=None, v_scale=None):
        """The GPU's (or a fault model's) outputs against the expectation -> list of failures; q, K and V each get their own entries."""
        c = self.c
        rows, nkv = c["B"] * c["L"], c["nkv"]
        bad = compare(np.asarray(q, f32).reshape(rows, c["nh"], 128), self.q, "q")
        for which, raw, sc, var in (("k", k_raw, k_scale, self.krows), ("v", v_raw, v_scale, self.vrows)):
            raw = np.asarray(raw)
            assert raw.shape == (c["B"], nkv, c["max_seq"], 128) and raw.dtype == (np.uint8 if fmt == "fp8" else np.uint16), (raw.shape, raw.dtype)
            written = np.zeros(raw.shape[:3], bool)
            written[self.b, :, self.p] = True
            if not np.array_equal(raw[~written], raw_fill(fmt, raw[~written].shape)):
                bad.append("%s cache: %d rows outside [start, start + L) lost their fill" % (which, int((raw[~written] != raw_fill(fmt, (1,))[0]).any(-1).sum())))
            if not np.array_equal(written.sum(2), np.full(written.shape[:2], c["L"])):
                bad.append("%s cache: the case writes a row twice" % which)
            if fmt == "fp8" and not np.array_equal(np.asarray(sc, f32)[~written].view(np.uint32), np.full(int((~written).sum()), FILL * 0x01010101, np.uint32)):
                bad.append("%s scales: entries outside [start, start + L) lost their fill" % which)
            got = raw[self.b, :, self.p]          # [rows, nkv, 128]
            if fmt == "bf16":
                bad += compare(from_bits16(got), var, which + " cache")
                continue
            for r in range(rows):
                for h in range(nkv):
                    codes, scales = self.cand(which, r, h)
                    if fmt == "fp8":
                        gs = np.asarray(sc, f32)[self.b[r], h, self.p[r]]
                        ok = ((codes == got[r, h]).all(1) & (scales.view(np.uint32) == gs.view(np.uint32))).any()
                    elif codes[0, 0] == 0x7F and (codes == 0x7F).all():
                        ok = np.isnan(from_bits16(got[r, h])).all()
                    else:
                        img = bits16(dequantize_e4m3_rows(codes, np.log2(scales).astype(np.int32)))
                        ok = (img == got[r, h]).all(1).any()
                    if not ok:
                        bad.append("%s cache row (row %d, kv head %d): none of the %d candidate quantisations" % (which, r, h, len(codes)))
        return bad

    def model_outputs(self, fmt, fault=None):
        """The outputs a kernel with `fault` (None: a correct one, centre variants) would return, in the hook's formats."""
        c = self.c
        off = dict(cosf=0, sinf=0, rsqrtf=0)
        q, k, v = emu_rope(c, off, fault)
        b, p = cache_rows(c, fault)
        shape = (c["B"], c["nkv"], c["max_seq"], 128)
        out = [q.reshape(len(q), -1)]
        scs = []
        kexp = None
        for which, rows in (("k", k), ("v", v)):
            raw = raw_fill(fmt, shape)
            sc = np.full(shape[:3], FILL_SCALE, f32)
            if fmt == "bf16":
                raw[b, :, p] = bits16(rows)
            else:
                flat = rows.reshape(-1, 128)
                fin = np.isfinite(flat).all(1)
                codes, exps = np.full(flat.shape, 0x7F, np.uint8), np.zeros(len(flat), np.int32)
                codes[fin], e = quantize_e4m3_rows(flat[fin])
                exps[fin] = e
                if fault == "v_with_k_scale" and which == "v":
                    exps = kexp
                    codes = _encode_with(flat, exps)
                if fault == "neighbour_scale":
                    exps = np.roll(exps, 1)
                kexp = exps if which == "k" else kexp
                scale = np.ldexp(f32(1), exps).astype(f32)
                if fmt == "fp8":
                    raw[b, :, p] = codes.reshape(rows.shape)
                    sc[b, :, p] = scale.reshape(rows.shape[:2])
                else:
                    img = dequantize_e4m3_rows(codes, exps)
                    raw[b, :, p] = bits16(np.where(fin[:, None], img, f32(np.nan))).reshape(rows.shape)
            out.append(raw)
            scs.append(sc if fmt == "fp8" else None)
        return out + scs


def _encode_with(rows, exps):
    """e4m3 codes of rows scaled by GIVEN exponents (a fault model: another row's scale). Values that leave the range take the NaN code."""
    scaled = np.ldexp(np.asarray(rows, f32), -np.asarray(exps, np.int32)[:, None]).astype(f32)
    table = dequantize_e4m3_rows(np.arange(256, dtype=np.uint8)[None], np.zeros(1, np.int32))[0]
    codes = np.full(scaled.shape, 0x7F, np.uint8)
    ok = np.isfinite(table)
    cand = np.flatnonzero(ok)
    with np.errstate(invalid="ignore"):
        near = np.abs(scaled[..., None].astype(np.float64) - table[cand].astype(np.float64)).argmin(-1)
    inr = np.abs(scaled) <= 448
    codes[inr] = cand[near][inr]
    return codes


# ---- the vision rotary kernel -------------------------------------------------------------------------------------------------------
def emu_vis_rope(c, off):
    hd, heads, rows = c["hd"], c["heads"], c["rows"]
    half, quarter = hd // 2, hd // 4
    x = np.asarray(c["qkv"], f32).reshape(rows, 3, heads, hd)[:, :2]
    d = np.arange(half)
    p = np.asarray(c["pos"]).reshape(rows, 2)[:, np.where(d < quarter, 0, 1)].astype(f32)          # [rows, half]
    ang = p * np.asarray(c["inv_freq"], f32)[np.where(d < quarter, d, d - quarter)]
    assert ang.dtype == f32
    cs, sn = dev("cosf", ang, off["cosf"])[:, None, None, :], dev("sinf", ang, off["sinf"])[:, None, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    o = np.concatenate([bf16(x1 * cs - x2 * sn), bf16(x2 * cs + x1 * sn)], -1)
    return o[:, 0].reshape(rows, -1), o[:, 1].reshape(rows, -1)


# ---- float64 guards: (reference, bound) of the plain formulas ----------------------------------------------------------------------------
R8 = 2.0 ** -8 * (1 + 2.0 ** -6)          # one bf16 rounding, relative, with room for the fp32 operations under it
TINY = 2.0 ** -126


def guard_norm(r, w, eps, r_err=None):
    """RMSNorm(r) w in float64. Roundings: bf16(r * rs) and the product; r_err: the absolute error of r itself against the float64 r."""
    r, w = np.asarray(r, np.float64), np.asarray(w, np.float64)
    rms = np.sqrt((r * r).mean(-1, keepdims=True) + eps)
    ref = w * r / rms
    bound = 2 * R8 * np.abs(ref) + TINY
    if r_err is not None:
        rel = np.sqrt((r_err ** 2).sum(-1, keepdims=True)) / np.maximum(np.sqrt((r * r).sum(-1, keepdims=True)), TINY)
        bound = bound * (1 + 2 * rel) + np.abs(w) * r_err / rms * (1 + R8) ** 2 + np.abs(ref) * 2 * rel
    return ref, bound


def guard_add(x, y, slot=None, ds=None):
    s = np.asarray(x, np.float64) + np.asarray(y, np.float64)
    err = half_ulp_bf16(s)
    if slot is not None:
        on = np.asarray(slot) >= 0
        s2 = s.copy()
        s2[on] += np.asarray(ds, np.float64)[np.asarray(slot)[on]]
        err = np.where(on[:, None], err + half_ulp_bf16(s2) + 2.0 ** -8 * err, err)
        s = s2
    return s, err


def guard_silu_mul(g, u):
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    with np.errstate(over="ignore"):
        ref = g / (1 + np.exp(-g)) * u
    # (below -88.7 expf(-g) is infinite in fp32 and the kernel gives 0 where float64 still holds |g| e^g < |g| 2^-127)
    return ref, 2 * R8 * np.abs(ref) + np.abs(u) * np.abs(g) * 2.0 ** -127 + 2.0 ** -140


def guard_rope(c):
    """-> (q, k, v) references and (eq, ek) bounds in float64: c and s rounded to bf16, both products and the sum (Qwen3: and the two
    roundings of the norm under them)."""
    nh, nkv, rows = c["nh"], c["nkv"], c["B"] * c["L"]
    x = np.asarray(c["qkv"], np.float64).reshape(rows, nh + 2 * nkv, 128)
    comp = components(c["family"], c["sections"])
    p = np.asarray(c["pos"]).reshape(3, rows)[comp, np.arange(rows)[:, None]].astype(np.float64)
    ang = (p * np.asarray(c["inv_freq"], np.float64))[:, None, :]
    qk = x[:, :nh + nkv]
    ey = np.zeros_like(qk)
    if c["family"] == "qwen3":
        w = np.concatenate([np.broadcast_to(np.asarray(c["qn"], np.float64), (nh, 128)), np.broadcast_to(np.asarray(c["kn"], np.float64), (nkv, 128))])
        with np.errstate(invalid="ignore", over="ignore"):
            qk = w * qk / np.sqrt((qk * qk).mean(-1, keepdims=True) + c["eps"])
        ey = 2 * R8 * np.abs(qk)
    x1, x2, e1, e2 = qk[..., :64], qk[..., 64:], ey[..., :64], ey[..., 64:]
    cs, sn = np.cos(ang), np.sin(ang)
    # fp32 angle: float(pos) * inv_freq carries up to 2^-24 |ang| of rounding, which moves cos and sin by as much
    ea = np.abs(ang) * 2.0 ** -23 + 2.0 ** -8 * (1 + 2.0 ** -6)
    o1, o2 = x1 * cs - x2 * sn, x2 * cs + x1 * sn
    with np.errstate(invalid="ignore"):
        b1 = (np.abs(x1) + np.abs(x2)) * (ea + R8) + (e1 + e2) * (1 + R8) + R8 * np.abs(o1) + TINY
        b2 = (np.abs(x1) + np.abs(x2)) * (ea + R8) + (e1 + e2) * (1 + R8) + R8 * np.abs(o2) + TINY
    o, b = np.concatenate([o1, o2], -1), np.concatenate([b1, b2], -1)
    return (o[:, :nh], o[:, nh:], x[:, nh + nkv:]), (b[:, :nh], b[:, nh:])


def e4m3_step(v):
    """The quantisation error of a row's e4m3 image, per element: half a step at 4 significant bits, or half the subnormal step 2^-10
    of the row's scale."""
    v = np.asarray(v, np.float64)
    a = np.abs(v).max(-1, keepdims=True)
    return np.maximum(2.0 ** -4 * np.abs(v), a * 2.0 ** -17) * (1 + 2.0 ** -6)


def guard_vis_rope(c):
    hd, heads, rows = c["hd"], c["heads"], c["rows"]
    half, quarter = hd // 2, hd // 4
    x = np.asarray(c["qkv"], np.float64).reshape(rows, 3, heads, hd)[:, :2]
    d = np.arange(half)
    p = np.asarray(c["pos"]).reshape(rows, 2)[:, np.where(d < quarter, 0, 1)].astype(np.float64)
    ang = (p * np.asarray(c["inv_freq"], np.float64)[np.where(d < quarter, d, d - quarter)])[:, None, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    o = np.concatenate([x1 * np.cos(ang) - x2 * np.sin(ang), x2 * np.cos(ang) + x1 * np.sin(ang)], -1)
    mag = np.concatenate([np.abs(x1) + np.abs(x2)] * 2, -1)
    bound = R8 * np.abs(o) + mag * (np.concatenate([np.abs(ang)] * 2, -1) * 2.0 ** -23 + 2.0 ** -20) + TINY
    return (o[:, 0].reshape(rows, -1), o[:, 1].reshape(rows, -1)), (bound[:, 0].reshape(rows, -1), bound[:, 1].reshape(rows, -1))


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def small_grid(n_threads):
    """A max_blocks under which the grid-stride loop over n_threads makes at least three trips, the last one partial."""
    blocks = -(-n_threads // 256)
    for mb in range(max(1, (blocks - 1) // 3), 0, -1):
        trips = -(-n_threads // (mb * 256))
        if trips >= 3 and n_threads % (mb * 256) != 0:
            return mb
    raise AssertionError("no such grid for %d threads" % n_threads)


def inv_freq_text(theta=1e6):
    """1 / theta^(2 i / 128) in fp32, as the decoders build it."""
    return (f32(1) / np.power(f32(theta), np.arange(0, 128, 2, dtype=f32) / f32(128))).astype(f32)


def inv_freq_vision(hd):
    return (f32(1) / np.power(f32(10000), np.arange(0, hd // 2, 2, dtype=f32) / f32(hd // 2))).astype(f32)


GEOMETRIES = ((4, 2), (7, 1), (3, 1))
# form -> (B, L, start, max_seq, start_from_device, formats): the launch forms of vlm_forward. The e4m3 formats reach a rope kernel in
# decode steps only (their prefills are staged through the bf16 instantiation); a prefill that continues a cache exists for bf16 only.
FORMS = dict(staged=(3, 5, 0, 5, False, ("bf16",)), prefill=(3, 5, 0, 23, False, ("bf16",)), cont=(3, 4, 11, 23, False, ("bf16",)),
             decode=(5, 1, 37, 41, False, KV_FORMATS), decode_dev=(5, 1, 37, 41, True, KV_FORMATS))
SECTIONS = dict(qwen2_5=((16, 24), (8, 8)), qwen3=((20, 20), (12, 17)))          # production's, and a second split (see components)


def rope_case(family, geom, form, sections=None, kind="random", seed=0):
    """kind: "random" positions (three independent components below 4096); "zero" positions (the exact case); "special": random positions
    and the e4m3 edge rows - all-zero rows, one huge value among tiny ones, an Inf - in the K and V heads."""
    nh, nkv = geom
    B, L, start, max_seq, from_dev, formats = FORMS[form]
    rows, heads = B * L, nh + 2 * nkv
    rng = np.random.default_rng([seed, nh, nkv, B, L, start, int(family == "qwen3")])
    qkv = bf16(rng.normal(0, 1, (rows, heads, 128)) * rng.choice([0.25, 1.0, 8.0], (rows, heads, 1)))
    pos = np.zeros((3, rows), np.int32) if kind == "zero" else rng.integers(0, 4096, (3, rows)).astype(np.int32)
    if kind == "special":
        kv = qkv[:, nh:]
        kv[0, 0::2] = 0                                         # all-zero rows (K of head 0, and every second K / V head)
        kv[1 % rows] = bf16(rng.normal(0, 1, kv[0].shape) * 2.0 ** -20)
        kv[1 % rows, :, 5] = 30720.0                              # one huge value among tiny ones
        kv[2 % rows, :, 77] = np.inf
        kv[3 % rows, nkv:, 3] = -np.inf                         # (V only)
    c = dict(family=family, nh=nh, nkv=nkv, B=B, L=L, start=start, max_seq=max_seq, start_from_device=from_dev, formats=formats, form=form, kind=kind,
             sections=tuple(sections or SECTIONS[family][0]), qkv=qkv.reshape(rows, heads * 128), pos=pos, inv_freq=inv_freq_text(), eps=1e-6,
             qn=bf16(rng.normal(1, 0.3, 128)), kn=bf16(rng.normal(1, 0.3, 128)))
    c["id"] = "%s-%dq%dkv-%s-%s-s%dx%d" % (family, nh, nkv, form, kind, c["sections"][0], c["sections"][1])
    c["small_grid"] = small_grid(rows * heads * 64)
    return c


@functools.lru_cache(maxsize=None)
def rope_cases():
    out = []
    for family in ("qwen2_5", "qwen3"):
        for geom in GEOMETRIES:
            for form in FORMS:
                out.append(rope_case(family, geom, form))
            out.append(rope_case(family, geom, "prefill", kind="zero"))
            out.append(rope_case(family, geom, "decode", kind="zero"))
        for form in ("prefill", "decode"):
            out.append(rope_case(family, (4, 2), form, sections=SECTIONS[family][1], seed=1))
        out.append(rope_case(family, (4, 2), "decode", kind="special", seed=2))
        out.append(rope_case(family, (3, 1), "decode_dev", kind="special", seed=3))
    return {c["id"]: c for c in out}


@functools.lru_cache(maxsize=None)
def rope_expect(case_id):
    return RopeExpect(rope_cases()[case_id])


ROW_D = (8, 252, 256, 260, 1536, 3584)
ROW_ROWS = (1, 3, 65)
ROW_ROUTES = ("rmsnorm", "add", "add_rmsnorm", "add_rmsnorm_no_w", "add_rmsnorm_ds", "few_rows_rmsnorm", "silu_mul")


def _rows_data(rng, kind, rows, d):
    if kind == "ints":          # squares below 2^6, sums below 2^24: every order of additions is exact
        return rng.integers(-7, 8, (rows, d)).astype(f32)
    return bf16(rng.normal(0, 1, (rows, d)) * rng.choice([0.03, 1.0, 30.0], (rows, 1)))


def rows_case(route, rows, d, kind="random", eps=1e-6, seed=0, alias=False, pad=False):
    rng = np.random.default_rng([seed, ROW_ROUTES.index(route), rows, d, int(kind == "ints")])
    c = dict(route=route, rows=rows, d=d, kind=kind, eps=eps, alias=alias, ldx=d + 8 if pad else d, ldy=d + 4 if pad else d)
    c["x"] = _rows_data(rng, kind, rows, d)
    if route not in ("rmsnorm", "few_rows_rmsnorm"):
        c["y"] = _rows_data(rng, kind, rows, d)
    if route in ("rmsnorm", "add_rmsnorm", "add_rmsnorm_ds", "few_rows_rmsnorm"):
        c["w"] = bf16(rng.normal(1, 0.3, d))
    if route == "add_rmsnorm_ds":          # slots -1 and >= 0 mixed, slot 1 repeated where there are rows for it
        c["ds"] = _rows_data(rng, kind, 3, d)
        c["slot"] = np.resize(np.array([1, -1, 1, 0, -1, 2], np.int32), rows)
    if route == "few_rows_rmsnorm":
        c["x"][0, :4] = [-0.0, 0.0, -0.0, 1.0]          # x is rewritten as x + 0: a negative zero comes back positive
    if route == "silu_mul":
        g = c["x"].reshape(-1)
        sp = np.array([-89.0, -100.0, -1.0e4, -80.0, 40.0, 41.5, 100.0, 3.0e4, 0.0, -0.0, -20.0, 20.0], f32)
        at = rng.permutation(g.size)[:min(g.size, 3 * sp.size)]
        g[at] = bf16(np.resize(sp, at.size))
    n_threads = rows * d // 4 if route in ("add", "silu_mul") else rows * 64
    c["small_grid"] = None if route == "few_rows_rmsnorm" or -(-n_threads // 256) < 4 else small_grid(n_threads)
    c["id"] = "%s-%dx%d-%s-eps%g%s%s" % (route, rows, d, kind, eps, "-alias" if alias else "", "-padded" if pad else "")
    return c


@functools.lru_cache(maxsize=None)
def rows_cases():
    out = []
    for route in ("rmsnorm", "add_rmsnorm", "add_rmsnorm_no_w", "add_rmsnorm_ds"):
        for i, d in enumerate(ROW_D):
            for j, rows in enumerate(ROW_ROWS):
                out.append(rows_case(route, rows, d, eps=(1e-6, 1e-5)[(i + j) % 2]))
        out.append(rows_case(route, 3, 260, kind="ints"))
        out.append(rows_case(route, 65, 1536, kind="ints", eps=1e-5))
    out += [rows_case("rmsnorm", rows, d, pad=True, seed=1) for rows, d in ((3, 8), (65, 260), (3, 3584))]
    out += [rows_case("add", rows, d) for rows, d in ((1, 4), (3, 260), (65, 1536), (65, 3584))]
    for rows in (1, 64):
        for d in (512, 4352):
            out += [rows_case("few_rows_rmsnorm", rows, d, eps=eps) for eps in (1e-6, 1e-5)]
    out.append(rows_case("few_rows_rmsnorm", 64, 512, kind="ints"))
    for alias in (False, True):          # n4 = 1, odd counts of quads, a size with several trips
        out += [rows_case("silu_mul", rows, d, alias=alias) for rows, d in ((1, 4), (3, 260), (1, 12), (65, 1536))]
    return {c["id"]: c for c in out}


def rows_emulate(c, off, fault=None):
    """-> (out_x or None, out_n or None) as the hook returns them."""
    route, eps = c["route"], c["eps"]
    if route == "rmsnorm":
        return None, emu_norm(c["x"], c["w"], eps, off)
    if route == "add":
        return emu_add(c["x"], c["y"]), None
    if route == "few_rows_rmsnorm":
        return emu_few_rows(c["x"], c["w"], eps, off)
    if route == "silu_mul":
        return emu_silu_mul(c["x"], c["y"], off, fault), None
    return emu_add_rmsnorm(c["x"], c["y"], c.get("w"), eps, off, c.get("slot"), c.get("ds"), fault)


@functools.lru_cache(maxsize=None)
def rows_expect(case_id):
    """-> (Var of out_x or None, Var of out_n or None)."""
    c = rows_cases()[case_id]
    fns = ("expf",) if c["route"] == "silu_mul" else (() if c["route"] in ("add", "add_rmsnorm_no_w") else ("rsqrtf",))
    present = [o is not None for o in rows_emulate(c, dict(rsqrtf=0, expf=0))]
    vs = iter(variants(fns, lambda off: tuple(o for o in rows_emulate(c, dict(dict(rsqrtf=0, expf=0), **off)) if o is not None)))
    return tuple(next(vs) if p else None for p in present)


def rows_check(case_id, out_x, out_n):
    """-> (failures, fragile share)."""
    c = rows_cases()[case_id]
    ex, en = rows_expect(case_id)
    bad, frag, n = [], 0, 0
    for got, var, what in ((out_x, ex, "x"), (out_n, en, "n")):
        if var is None:
            continue
        got = np.asarray(got, f32)
        if what == "n" and c["ldy"] != c["d"]:
            if not (got[:, c["d"]:] == 768).all():
                bad.append("n: the columns past d were written")
            got = got[:, :c["d"]]
        bad += compare(got, var, what)
        frag, n = frag + var.n_fragile, n + var.center.size
    return bad, frag / n


def rows_guard(case_id, out_x, out_n):
    """worst err / bound of the outputs against the float64 formulas."""
    c = rows_cases()[case_id]
    route, d = c["route"], c["d"]
    x = c["x"][:, :d]
    if route == "rmsnorm":
        return worst(np.asarray(out_n)[:, :d], *guard_norm(x, c["w"], c["eps"]))
    if route == "few_rows_rmsnorm":
        return max(worst(out_x, x, np.full(x.shape, TINY)), worst(out_n, *guard_norm(x, c["w"], c["eps"])))
    if route == "silu_mul":
        return worst(out_x, *guard_silu_mul(x, c["y"]))
    r, err = guard_add(x, c["y"], c.get("slot"), c.get("ds"))
    w = worst(out_x, r, err + TINY)
    return w if out_n is None else max(w, worst(out_n, *guard_norm(r, c["w"], c["eps"], r_err=err)))


@functools.lru_cache(maxsize=None)
def vis_cases():
    out = {}
    for hd in (64, 80):
        for heads in (1, 3):
            for rows in (1, 70):
                for kind in ("random", "zero"):
                    rng = np.random.default_rng([hd, heads, rows])
                    c = dict(hd=hd, heads=heads, rows=rows, kind=kind, qkv=bf16(rng.normal(0, 1, (rows, 3 * heads * hd))), inv_freq=inv_freq_vision(hd),
                             pos=np.zeros((rows, 2), np.int32) if kind == "zero" else rng.integers(0, 4096, (rows, 2)).astype(np.int32))
                    n_threads = rows * 2 * heads * (hd // 2)
                    c["small_grid"] = small_grid(n_threads) if -(-n_threads // 256) >= 4 else None
                    c["id"] = "hd%d-%dh-%drows-%s" % (hd, heads, rows, kind)
                    out[c["id"]] = c
    return out


@functools.lru_cache(maxsize=None)
def vis_expect(case_id):
    c = vis_cases()[case_id]
    return variants(("cosf", "sinf"), lambda off: emu_vis_rope(c, off))
