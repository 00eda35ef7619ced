// Face clustering sweeps: exact all-pairs passes over n unit rows (ArcFace embeddings, d = 512) on the fp32 matrix cores.
//
// The reference clusters faces with HDBSCAN (faces/clusterer.py:126-216): L2-normalise, then `hdbscan` on the CPU (approximate
// boruvka_balltree, :187) or cuML on an NVIDIA GPU (:167-181). Here the two O(n^2 d) stages of HDBSCAN* - core distances and the
// minimum spanning tree of the mutual-reachability graph - are exact sweeps; the tree condensing stays on the host
// (facet_amd/face_cluster.py). The n x n matrix is never written: a block forms one 128 x 128 tile of dot products at a time and
// reduces it on the spot.
//
//   tile core (cl_sweep_kernel, shared by all three modes): 256 threads = 2 x 2 waves, wave tile 64 x 64 = 2 x 2 accumulators of
//     v_mfma_f32_32x32x2_f32. Rows of A (the block's 128 rows) and of B (the column tile's 128 rows) are staged k-contiguous in
//     32-float slabs, double buffered, global -> VGPR before the MFMA phase and VGPR -> LDS after it, as kernels_conv.hip does.
//     LDS rows are 36 floats: a lane's ds_read_b128 of (row r, k = 8s + 4h ..) lands on slot (9r + 2s + h) mod 16 of the 16-slot
//     bank row, 16 distinct slots per 16-lane group. Grid = (row tiles, column strips): block (ti, s) walks column tiles s, s +
//     strips, ...
//   epilogue: the accumulators go to LDS as a [128][130] image over the dead staging buffers (a store instruction's 32 lanes of one
//     half hold 32 consecutive columns of one row: conflict free), then thread t owns row t >> 1 and scans the columns 2c + (t & 1)
//     (bank (2 row + (t & 1) + 2c) mod 32: the 32 lanes of a half hit 32 banks). Squared distance = (|a|^2 + |b|^2) - 2 a.b, clamped
//     at 0; the diagonal is 0 by definition.
//   bit-identical (i, j) and (j, i): the dot product of rows i and j is the same chain whichever of them is the A row: every tile
//     runs the same k order (slab, step s, component, lane half h <-> k slot h of the instruction), x_i[k] * x_j[k] commutes, and
//     a zero-initialised accumulator is all the tile position contributes. |a|^2 + |b|^2 commutes too, 2 * dot is exact, and max is
//     symmetric, so the swept mutual-reachability value of an edge is one number seen from both ends - which the Boruvka key needs.
//
//   CL_KNN:     every scanning thread keeps its k smallest (d^2 bits << 32 | column) keys sorted in LDS; the 2 x strips partial lists
//               of a row are merged by cl_knn_merge_kernel, and cl_refine_core_kernel recomputes the chosen k-th neighbour's distance
//               from direct differences in fp64: the GEMM form picks the neighbour, it never supplies the value.
//   CL_BORUVKA: every row finds its lightest edge to another component under the order (fp32 bits of mr^2, min(i,j), max(i,j)). For
//               a fixed row i that order is the order of (mr^2 bits, j) - whichever side of i the two columns lie, the smaller column
//               gives the smaller (min, max) pair - so the row's minimum is one 64-bit vector atomicMin on mr^2 bits << 32 | j. The
//               full triple needs 32 + 18 + 18 bits, so the minimum per component and the union-find run on the host over the n row
//               keys (8 n bytes per round); rounds are bounded by ceil(log2 n) + 1.
//   CL_MATCH:   rows of Q against rows of C, both normalised: largest dot product, first column on ties.
//
// Similar-photo search and person-merge suggestions (reference api/routers/gallery.py:410-539, faces/merge_analyzer.py:29-187) are two
// more epilogues of the same tile core, rows = queries, columns = candidates, both normalised so that the dot product is the cosine:
//   SIM_TOPK:   score = sim_score() (the reference's four weighted factors in fp32, or the plain cosine); the scanning thread keeps its
//               k best (cl_sim_key(score) << 32 | column) keys in the same sorted LDS lists as CL_KNN - ascending keys are (score
//               descending, column ascending) - and sim_merge_kernel merges the 2 x strips lists of a query into idx / score [k].
//   SIM_PAIRS:  every (query, column) with score >= thr[query] is appended to a capacity-checked triple buffer under one counter
//               (the fe_hamming_pairs protocol: the count is exact, a store happens only below the capacity); with `upper` only
//               column > row, and the column tiles left of the diagonal are not formed at all.
//   sim_gemv_kernel: for at most SIM_GEMV_Q queries the sweep is a read of C, not a GEMM - a 128-row tile would spend 128 / nq times
//               the matrix work on zero rows. One wave per candidate row: the row is read once (float4 per lane), dotted with every
//               query row held in LDS, lane q evaluates sim_score() for query q and feeds the same list / triple outputs.
#include "engine.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace fe {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CL_T = 128;                              // tile rows = tile columns
constexpr int CL_BK = 32, CL_S = CL_BK + 4;            // k slab, LDS row stride of the staging buffers
constexpr int CL_ES = CL_T + 2;                        // row stride of the epilogue image
constexpr int CL_STAGE = 2 * 2 * CL_T * CL_S;          // floats: [2 buffers][A | B][128][36]
constexpr int CL_META = 3 * CL_T;                      // per column of the tile: |b|^2, core^2, component
static_assert(CL_T * CL_ES <= CL_STAGE, "the epilogue image must fit in the staging buffers");
enum : int { CL_KNN = 0, CL_BORUVKA = 1, CL_MATCH = 2, SIM_TOPK = 3, SIM_PAIRS = 4 };
constexpr unsigned long long CL_NONE = ~0ull;
constexpr int SIM_META = 6 * CL_T;                     // floats, per column of the tile: date (8 B), aggregate, person start, person count, eligible
constexpr int SIM_K_MAX = 32;                          // 72 KB staging + 4.5 KB metadata + k x 2 KB lists <= 160 KB of LDS: 41 would fit, 32 matches CL_KNN
constexpr int SIM_GEMV_Q = 8;                          // queries up to which the sweep is the one-wave-per-candidate read
constexpr long long SIM_NO_DATE = (long long)0x8000000000000000ull;   // FE_SIM_NO_DATE
static_assert(SIM_K_MAX == FE_SIM_K_MAX, "the header's K_MAX is the kernel's");

// per-row metadata of one side of a similarity sweep: device pointers, any of them null (= absent for every row)
struct SimSide {
  const unsigned char* has_emb;           // [n]
  const long long* date;                  // [n] seconds, SIM_NO_DATE = absent
  const float* agg;                       // [n], 0 / NaN = absent
  const int* poff; const int* pid;        // CSR person lists: ids of row r are pid [poff[r] .. poff[r + 1]), ascending, unique
  int npid;
};
struct SimParams {
  SimSide q, c;
  const int* q_self;                      // [nq] candidate index of the query itself, -1: none (nullable)
  const unsigned char* visible;           // [nc] (nullable)
  float wc, wp, wd, ws;
  int cosine, upper;
  const float* thr; int thr_stride;       // PAIRS: thr [row * thr_stride]
  unsigned long long cap;                 // PAIRS: room in pairs / pscore
  int* pairs; float* pscore; unsigned long long* count;
};

struct SweepParams {
  const float* a; int na;                 // rows    [na][d]
  const float* b; int nb;                 // columns [nb][d]
  int d, tiles_b;
  const float* n2a; const float* n2b;     // squared norms (KNN, BORUVKA)
  const float* core2; const int* comp;    // BORUVKA: fp32 core distance squared, component id, per point
  int k; unsigned long long* part;        // KNN: part [na][2 * strips][k]
  unsigned long long* rowkey;             // BORUVKA, MATCH: [na], preset to CL_NONE
  SimParams sim;                          // SIM_TOPK (with k, part), SIM_PAIRS
};

// sim -> 32 bits that DEcrease as sim grows, so that atomicMin finds the largest similarity and, among equals, the first column
__device__ __forceinline__ uint32_t cl_sim_key(float s) {
  const uint32_t b = __float_as_uint(s);
  return ~(b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u));
}
static inline float cl_sim_from_key(uint32_t k) {
  const uint32_t o = ~k;
  const uint32_t b = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

// what a scanning thread (tile path) or lane (gemv path) knows about its query
struct SimRow { int emb; long long date; float agg; int p0, pn, self; float thr; };

__device__ __forceinline__ void sim_person_range(const SimSide& s, int row, int& p0, int& pn) {
  p0 = 0; pn = 0;
  if (!s.poff || !s.pid) return;
  const int a = min(max(s.poff[row], 0), s.npid), b = min(max(s.poff[row + 1], a), s.npid);   // the clamp only guards the loads
  p0 = a; pn = b - a;
}
__device__ __forceinline__ SimRow sim_load_row(const SimParams& sp, int row, bool valid) {
  SimRow q{1, SIM_NO_DATE, 0.f, 0, 0, -1, 0.f};
  if (!valid) return q;
  if (sp.q.has_emb) q.emb = sp.q.has_emb[row] ? 1 : 0;
  if (sp.q.date) q.date = sp.q.date[row];
  if (sp.q.agg) q.agg = sp.q.agg[row];
  sim_person_range(sp.q, row, q.p0, q.pn);
  if (sp.q_self) q.self = sp.q_self[row];
  if (sp.thr) q.thr = sp.thr[(size_t)row * sp.thr_stride];
  return q;
}
__device__ __forceinline__ bool sim_agg_present(float a) { return a == a && a != 0.f; }

// the score of (query, candidate) from their cosine: the one epilogue function of the tile path and the gemv path.
//   wc (cos + 1) / 2 [query has an embedding] + wp |Pq n Pc| / max(|Pq|, |Pc|) [both non-empty]
//   + wd D(|floor((tq - tc) / 86400)|) [both dated] + ws max(0, 1 - |aq - ac| / 10) [both aggregates present and non-zero]
// every operation is one fp32 rounding (-ffp-contract=off): facet_amd/similar.py derives the error bound from this sequence.
__device__ __forceinline__ float sim_score(const SimParams& sp, const SimRow& q, long long cdate, float cagg, int cp0, int cpn, float cosv) {
  if (sp.cosine) return cosv;
  float s = 0.f;
  if (q.emb) s = sp.wc * ((cosv + 1.f) * 0.5f);
  if (q.pn > 0 && cpn > 0) {
    int i = 0, j = 0, shared = 0;
    while (i < q.pn && j < cpn) {
      const int a = sp.q.pid[q.p0 + i], b = sp.c.pid[cp0 + j];
      shared += a == b ? 1 : 0;
      i += a <= b ? 1 : 0;
      j += b <= a ? 1 : 0;
    }
    s += sp.wp * ((float)shared / (float)max(q.pn, cpn));
  }
  if (q.date != SIM_NO_DATE && cdate != SIM_NO_DATE) {
    // the reference takes abs((t_q - t_c).days): the SIGNED difference is floored to whole days first, so a candidate 30 days and one
    // second after the query is 31 days away, one 30 days and one second before it 30 (gallery.py:491)
    const long long diff = q.date - cdate;
    long long whole = diff / 86400;
    if (diff % 86400 != 0 && diff < 0) --whole;
    const long long days = whole < 0 ? -whole : whole;
    const float dsim = days == 0 ? 1.f : days <= 7 ? 0.5f : days <= 30 ? 0.2f : fmaxf(0.f, 1.f - (float)days / 365.f);
    s += sp.wd * dsim;
  }
  if (sim_agg_present(q.agg) && sim_agg_present(cagg)) s += sp.ws * fmaxf(0.f, 1.f - fabsf(q.agg - cagg) / 10.f);
  return s;
}
// fused scores keep only s > 0 (the reference's `if total_similarity > 0`), a NaN is never kept
__device__ __forceinline__ bool sim_keep(const SimParams& sp, float s) { return sp.cosine ? s == s : s > 0.f; }

__device__ __forceinline__ void sim_emit(const SimParams& sp, int row, int col, float s) {
  const unsigned long long at = atomicAdd(sp.count, 1ull);
  if (at < sp.cap) { sp.pairs[2 * at] = row; sp.pairs[2 * at + 1] = col; sp.pscore[at] = s; }
}

template <int MODE>
__global__ __launch_bounds__(256) void cl_sweep_kernel(SweepParams p) {
  extern __shared__ __attribute__((aligned(16))) float cl_lds[];
  float* As = cl_lds;                                   // [2][128][36]
  float* Bs = cl_lds + 2 * CL_T * CL_S;
  float* E = cl_lds;                                    // [128][130], after the k loop
  float* cn2 = cl_lds + CL_STAGE;
  float* ccore = cn2 + CL_T;
  int* ccomp = reinterpret_cast<int*>(ccore + CL_T);
  constexpr bool SIM = MODE == SIM_TOPK || MODE == SIM_PAIRS;
  constexpr bool LISTS = MODE == CL_KNN || MODE == SIM_TOPK;
  long long* sdate = reinterpret_cast<long long*>(cl_lds + CL_STAGE + CL_META);                    // SIM: the tile's column metadata
  float* sagg = cl_lds + CL_STAGE + CL_META + 2 * CL_T;
  int* sp0 = reinterpret_cast<int*>(sagg + CL_T);
  int* spn = sp0 + CL_T;
  int* sok = spn + CL_T;
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(cl_lds + CL_STAGE + CL_META + (SIM ? SIM_META : 0));   // KNN, SIM_TOPK: [k][256]

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int chunk = t & 7, srow = t >> 3;               // staging: 8 x 16 B per row, 32 rows per pass, 4 passes
  const int row0 = blockIdx.x * CL_T;
  const int nk = p.d / CL_BK;

  // the scanning role: row, column parity
  const int erow = t >> 1, half = t & 1;
  const int grow = row0 + erow;
  const bool rvalid = grow < p.na;
  float rn2 = 0.f, rcore = 0.f;
  int rcomp = 0;
  if (MODE != CL_MATCH && !SIM && rvalid) rn2 = p.n2a[grow];
  SimRow qrow{};
  if (SIM) qrow = sim_load_row(p.sim, grow, rvalid);
  if (MODE == CL_BORUVKA && rvalid) { rcore = p.core2[grow]; rcomp = p.comp[grow]; }
  unsigned long long best = CL_NONE;                    // BORUVKA / MATCH; KNN: the list's last (k-th) key
  if (LISTS)
    for (int s = 0; s < p.k; ++s) lists[s * 256 + t] = CL_NONE;

  const float* arow[4];
  bool aval[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = row0 + srow + 32 * i;
    aval[i] = m < p.na;
    arow[i] = p.a + (size_t)(aval[i] ? m : 0) * p.d + chunk * 4;
  }

  for (int tj = blockIdx.y; tj < p.tiles_b; tj += gridDim.y) {
    const int col0 = tj * CL_T;
    if (MODE == SIM_PAIRS && p.sim.upper && tj < (int)blockIdx.x) continue;   // block-uniform: the tile lies left of the diagonal
    const float* brow[4];
    bool bval[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = col0 + srow + 32 * i;
      bval[i] = m < p.nb;
      brow[i] = p.b + (size_t)(bval[i] ? m : 0) * p.d + chunk * 4;
    }
    float4 ra[4], rb[4];
    auto load_tile = [&](int kt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = aval[i] ? *reinterpret_cast<const float4*>(arow[i] + kt * CL_BK) : make_float4(0.f, 0.f, 0.f, 0.f);
        rb[i] = bval[i] ? *reinterpret_cast<const float4*>(brow[i] + kt * CL_BK) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(&As[(buf * CL_T + srow + 32 * i) * CL_S + chunk * 4]) = ra[i];
        *reinterpret_cast<float4*>(&Bs[(buf * CL_T + srow + 32 * i) * CL_S + chunk * 4]) = rb[i];
      }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nk) load_tile(kt + 1);
      const float* Ab = As + (buf * CL_T + wm * 64 + r) * CL_S + h * 4;
      const float* Bb = Bs + (buf * CL_T + wn * 64 + r) * CL_S + h * 4;
#pragma unroll
      for (int s = 0; s < CL_BK / 8; ++s) {
        float4 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const float4*>(Ab + i * 32 * CL_S + s * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const float4*>(Bb + j * 32 * CL_S + s * 8);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
          }
      }
      if (kt + 1 < nk) store_tile(buf ^ 1);
      __syncthreads();
    }

    // the staging buffers are dead (barrier above): C/D map col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          E[(wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * CL_ES + wn * 64 + j * 32 + r] = acc[i][j][e];
    if (SIM && t < CL_T) {
      const int c = col0 + t;
      const bool ok = c < p.nb && (!p.sim.visible || p.sim.visible[c]);
      sok[t] = ok ? 1 : 0;
      sdate[t] = ok && p.sim.c.date ? p.sim.c.date[c] : SIM_NO_DATE;
      sagg[t] = ok && p.sim.c.agg ? p.sim.c.agg[c] : 0.f;
      int c0 = 0, cn = 0;
      if (ok) sim_person_range(p.sim.c, c, c0, cn);
      sp0[t] = c0; spn[t] = cn;
    }
    if (MODE != CL_MATCH && !SIM && t < CL_T) {
      const int c = col0 + t;
      const bool ok = c < p.nb;
      cn2[t] = ok ? p.n2b[c] : 0.f;
      if (MODE == CL_BORUVKA) { ccore[t] = ok ? p.core2[c] : 0.f; ccomp[t] = ok ? p.comp[c] : 0; }
    }
    __syncthreads();

    if (rvalid) {
      const int ncol = min(CL_T, p.nb - col0);
      const float* Er = E + erow * CL_ES;
      for (int c = half; c < ncol; c += 2) {
        const int gc = col0 + c;
        const float dot = Er[c];
        if (SIM) {
          if (!sok[c] || gc == qrow.self || (p.sim.upper && gc <= grow)) continue;
          const float sc = sim_score(p.sim, qrow, sdate[c], sagg[c], sp0[c], spn[c], dot);
          if (!sim_keep(p.sim, sc)) continue;
          if (MODE == SIM_PAIRS) {
            if (sc >= qrow.thr) sim_emit(p.sim, grow, gc, sc);
          } else {
            const unsigned long long key = ((unsigned long long)cl_sim_key(sc) << 32) | (uint32_t)gc;
            if (key < best) {                           // the insertion of CL_KNN: ascending keys = (score descending, column ascending)
              int q = p.k - 1;
              while (q > 0) {
                const unsigned long long prev = lists[(q - 1) * 256 + t];
                if (prev <= key) break;
                lists[q * 256 + t] = prev;
                --q;
              }
              lists[q * 256 + t] = key;
              best = lists[(p.k - 1) * 256 + t];
            }
          }
        } else if (MODE == CL_MATCH) {
          const unsigned long long key = ((unsigned long long)cl_sim_key(dot) << 32) | (uint32_t)gc;
          best = key < best ? key : best;
        } else {
          float d2 = (rn2 + cn2[c]) - 2.f * dot;
          d2 = d2 > 0.f ? d2 : 0.f;
          if (MODE == CL_KNN) {
            if (gc == grow) d2 = 0.f;
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)gc;
            if (key < best) {                           // insertion into the sorted list; rare once the list has warmed up
              int q = p.k - 1;
              while (q > 0) {
                const unsigned long long prev = lists[(q - 1) * 256 + t];
                if (prev <= key) break;
                lists[q * 256 + t] = prev;
                --q;
              }
              lists[q * 256 + t] = key;
              best = lists[(p.k - 1) * 256 + t];
            }
          } else if (ccomp[c] != rcomp) {
            const float mr2 = fmaxf(fmaxf(rcore, ccore[c]), d2);
            const unsigned long long key = ((unsigned long long)__float_as_uint(mr2) << 32) | (uint32_t)gc;
            best = key < best ? key : best;
          }
        }
      }
    }
    __syncthreads();                                    // the next tile's staging overwrites the image
  }

  if (LISTS) {
    if (rvalid) {
      unsigned long long* out = p.part + ((size_t)grow * (2 * gridDim.y) + 2 * blockIdx.y + half) * p.k;
      for (int s = 0; s < p.k; ++s) out[s] = lists[s * 256 + t];
    }
  } else if (MODE != SIM_PAIRS) {
    const unsigned long long other = __shfl_xor(best, 1);
    best = other < best ? other : best;
    if (half == 0 && rvalid && best != CL_NONE) atomicMin(p.rowkey + grow, best);
  }
}

// x [n][d] -> xn [n][d] (x / (|x| + 1e-10) in fp32 as clusterer.py:157-158, or a copy), n2 [n] = |xn|^2. One wave per row.
__global__ __launch_bounds__(256) void cl_prepare_kernel(const float* __restrict__ x, int n, int d, int normalise, float* __restrict__ xn,
                                                         float* __restrict__ n2) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* src = x + (size_t)row * d;
  float* dst = xn + (size_t)row * d;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += src[c] * src[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float den = normalise ? sqrtf(s) + 1e-10f : 1.f;
  float s2 = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = normalise ? src[c] / den : src[c];
    dst[c] = v;
    s2 += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
  if (lane == 0) n2[row] = s2;
}

// part [n][lists][k] sorted partial lists (keys unique per row: a column sits in one list) -> sel [n]: the k-th smallest key
__global__ __launch_bounds__(256) void cl_knn_merge_kernel(const unsigned long long* __restrict__ part, int n, int lists, int k,
                                                           unsigned long long* __restrict__ sel) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const unsigned long long* p = part + (size_t)row * lists * k;
  const int total = lists * k;
  unsigned long long last = 0;
  for (int rnk = 0; rnk < k; ++rnk) {
    unsigned long long cur = CL_NONE;
    for (int q = 0; q < total; ++q) {
      const unsigned long long v = p[q];
      if ((rnk == 0 || v > last) && v < cur) cur = v;
    }
    last = cur;
  }
  sel[row] = last;
}

// sum (a_i - b_i)^2 over two fp32 rows in fp64, by the whole wave (every lane returns the sum)
__device__ __forceinline__ double cl_wave_sqdist(const float* __restrict__ a, const float* __restrict__ b, int d, int lane) {
  double s = 0.0;
  for (int c = lane; c < d; c += 64) {
    const double df = (double)a[c] - (double)b[c];
    s += df * df;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

__global__ __launch_bounds__(256) void cl_refine_core_kernel(const float* __restrict__ xn, int n, int d, const unsigned long long* __restrict__ sel,
                                                             double* __restrict__ core, float* __restrict__ core2, int* __restrict__ idx) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  int j = (int)(uint32_t)(sel[row] & 0xFFFFFFFFull);
  j = min(max(j, 0), n - 1);                            // a key is a column of this sweep; the clamp only guards the loads
  const double s = cl_wave_sqdist(xn + (size_t)row * d, xn + (size_t)j * d, d, lane);
  if (lane == 0) { core[row] = sqrt(s); core2[row] = (float)s; idx[row] = j; }
}

__global__ __launch_bounds__(256) void cl_refine_edges_kernel(const float* __restrict__ xn, int n, int d, int m, const int* __restrict__ eu,
                                                              const int* __restrict__ ev, const double* __restrict__ core, double* __restrict__ ew) {
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (e >= m) return;
  const int u = min(max(eu[e], 0), n - 1), v = min(max(ev[e], 0), n - 1);
  const double s = cl_wave_sqdist(xn + (size_t)u * d, xn + (size_t)v * d, d, lane);
  if (lane == 0) ew[e] = fmax(fmax(core[u], core[v]), sqrt(s));
}

// ---- similarity sweeps: the small-nq path and the list merge ---------------------------------------------------------------------

// na <= SIM_GEMV_Q queries against nb candidates, one wave per candidate row: the row is read once as float4 per lane and dotted
// with every query row held in LDS (a butterfly leaves the sum in every lane), then lane q scores the candidate for query q.
// TOPK: lane q keeps the wave's sorted k-list of query q in LDS; part [na][waves][k]. PAIRS: lane q appends its hits.
// LDS: [na][d] floats, then (TOPK) [4 waves][na][k] keys.
template <int MODE>
__global__ __launch_bounds__(256) void sim_gemv_kernel(SweepParams p) {
  extern __shared__ __attribute__((aligned(16))) float sg_lds[];
  float* qs = sg_lds;
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(sg_lds + (size_t)p.na * p.d);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int i = t; i < p.na * p.d; i += 256) qs[i] = p.a[i];
  const bool qlane = lane < p.na;
  const SimRow qrow = sim_load_row(p.sim, lane, qlane);
  unsigned long long* mine = lists + ((size_t)wave * p.na + (qlane ? lane : 0)) * p.k;
  unsigned long long best = CL_NONE;
  if (MODE == SIM_TOPK && qlane)
    for (int s = 0; s < p.k; ++s) mine[s] = CL_NONE;
  __syncthreads();

  const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
  for (int c = gw; c < p.nb; c += nw) {                  // wave-uniform
    if (p.sim.visible && !p.sim.visible[c]) continue;
    const float* row = p.b + (size_t)c * p.d;
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k0 = (i * 64 + lane) * 4;
      v[i] = k0 < p.d ? *reinterpret_cast<const float4*>(row + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float cosv = 0.f;
    for (int q = 0; q < p.na; ++q) {
      const float* qr = qs + (size_t)q * p.d;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k0 = (i * 64 + lane) * 4;
        if (k0 < p.d) {
          const float4 w = *reinterpret_cast<const float4*>(qr + k0);
          acc += v[i].x * w.x; acc += v[i].y * w.y; acc += v[i].z * w.z; acc += v[i].w * w.w;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
      if (lane == q) cosv = acc;
    }
    if (!qlane || c == qrow.self || (p.sim.upper && c <= lane)) continue;
    long long cdate = SIM_NO_DATE;
    float cagg = 0.f;
    int cp0 = 0, cpn = 0;
    if (!p.sim.cosine) {
      if (p.sim.c.date) cdate = p.sim.c.date[c];
      if (p.sim.c.agg) cagg = p.sim.c.agg[c];
      sim_person_range(p.sim.c, c, cp0, cpn);
    }
    const float sc = sim_score(p.sim, qrow, cdate, cagg, cp0, cpn, cosv);
    if (!sim_keep(p.sim, sc)) continue;
    if (MODE == SIM_PAIRS) {
      if (sc >= qrow.thr) sim_emit(p.sim, lane, c, sc);
    } else {
      const unsigned long long key = ((unsigned long long)cl_sim_key(sc) << 32) | (uint32_t)c;
      if (key < best) {
        int q = p.k - 1;
        while (q > 0) {
          const unsigned long long prev = mine[q - 1];
          if (prev <= key) break;
          mine[q] = prev;
          --q;
        }
        mine[q] = key;
        best = mine[p.k - 1];
      }
    }
  }
  if (MODE == SIM_TOPK && qlane) {
    unsigned long long* out = p.part + ((size_t)lane * nw + gw) * p.k;
    for (int s = 0; s < p.k; ++s) out[s] = mine[s];
  }
}

// part [nq][lists][k]: ascending partial lists, CL_NONE padded, keys unique per query (a column sits in one list) -> idx / score
// [nq][k], -1 / 0 padded. One wave per query: lane l owns the lists l, l + 64, ... and their heads (LDS, one byte per list); a rank
// is the smallest head of all lists, and the one lane that holds it advances that list.
__global__ __launch_bounds__(64) void sim_merge_kernel(const unsigned long long* __restrict__ part, int lists, int k, int* __restrict__ idx,
                                                       float* __restrict__ score) {
  extern __shared__ unsigned char sm_heads[];
  const int row = blockIdx.x, lane = threadIdx.x;
  const unsigned long long* p = part + (size_t)row * lists * k;
  for (int l = lane; l < lists; l += 64) sm_heads[l] = 0;
  for (int rnk = 0; rnk < k; ++rnk) {
    unsigned long long cur = CL_NONE;
    int from = -1;
    for (int l = lane; l < lists; l += 64) {
      const int hd = sm_heads[l];
      if (hd < k) {
        const unsigned long long v = p[(size_t)l * k + hd];
        if (v < cur) { cur = v; from = l; }
      }
    }
    unsigned long long m = cur;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(m, o);
      m = other < m ? other : m;
    }
    if (m != CL_NONE && cur == m) sm_heads[from] += 1;
    if (lane == 0) {
      const uint32_t kb = ~(uint32_t)(m >> 32);          // cl_sim_key backwards
      const uint32_t fb = (kb & 0x80000000u) ? (kb ^ 0x80000000u) : ~kb;
      idx[(size_t)row * k + rnk] = m == CL_NONE ? -1 : (int)(uint32_t)(m & 0xFFFFFFFFull);
      score[(size_t)row * k + rnk] = m == CL_NONE ? 0.f : __uint_as_float(fb);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
namespace {

// device memory of one call: sized by n, so it does not come out of the model arena
struct DevMem {
  std::vector<void*> ptrs;
  ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
  template <typename T> T* get(size_t count) {
    void* p = nullptr;
    FE_HIP(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)));
    ptrs.push_back(p);
    return (T*)p;
  }
};

constexpr unsigned long long CL_CANARY = 0xA5A5A5A5A5A5A5A5ull;

template <int MODE>
void cl_launch_sweep(SweepParams p, hipStream_t s, int* strips_out = nullptr, int strips_fixed = 0) {
  const int tiles_a = (p.na + CL_T - 1) / CL_T;
  p.tiles_b = (p.nb + CL_T - 1) / CL_T;
  // enough blocks for four rounds of the chip's 256 CUs when the row tiles alone are too few
  const int strips = strips_fixed ? strips_fixed : std::max(1, std::min(p.tiles_b, (1024 + tiles_a - 1) / tiles_a));
  if (strips_out) *strips_out = strips;
  constexpr bool lists = MODE == CL_KNN || MODE == SIM_TOPK;
  constexpr size_t fixed = (size_t)(CL_STAGE + CL_META + (MODE == SIM_TOPK || MODE == SIM_PAIRS ? SIM_META : 0)) * sizeof(float);
  const size_t lds = fixed + (lists ? (size_t)p.k * 256 * sizeof(unsigned long long) : 0);
  static std::atomic<uint64_t> lds_set{0};
  ensure_dynamic_lds((const void*)cl_sweep_kernel<MODE>, fixed + (lists ? 32 * 256 * 8 : 0), lds_set);
  hipLaunchKernelGGL(cl_sweep_kernel<MODE>, dim3(tiles_a, strips), dim3(256), lds, s, p);
  FE_HIP(hipGetLastError());
}

int cl_strips(int na, int nb) {
  const int tiles_a = (na + CL_T - 1) / CL_T, tiles_b = (nb + CL_T - 1) / CL_T;
  return std::max(1, std::min(tiles_b, (1024 + tiles_a - 1) / tiles_a));
}

// host or device rows -> normalised (or copied) device rows + squared norms
void cl_prepare(Ctx& c, DevMem& mem, const float* x, int n, int d, int on_device, int normalise, float*& xn, float*& n2) {
  const float* d_x = x;
  if (!on_device) {
    float* in = mem.get<float>((size_t)n * d);
    FE_HIP(hipMemcpyAsync(in, x, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, c.stream));
    d_x = in;
  }
  xn = mem.get<float>((size_t)n * d);
  n2 = mem.get<float>(n);
  hipLaunchKernelGGL(cl_prepare_kernel, dim3((n + 3) / 4), dim3(256), 0, c.stream, d_x, n, d, normalise ? 1 : 0, xn, n2);
  FE_HIP(hipGetLastError());
}

struct CoreDev { double* core; float* core2; int* idx; };

CoreDev cl_core(Ctx& c, DevMem& mem, const float* xn, const float* n2, int n, int d, int k) {
  const int strips = cl_strips(n, n), lists = 2 * strips;
  // part [n][lists][k], then a canary word: a store past the lists would land on it
  const size_t words = (size_t)n * lists * k;
  unsigned long long* part = mem.get<unsigned long long>(words + 1);
  FE_HIP(hipMemsetAsync(part + words, 0xA5, sizeof(unsigned long long), c.stream));
  unsigned long long* sel = mem.get<unsigned long long>(n);
  CoreDev o{mem.get<double>(n), mem.get<float>(n), mem.get<int>(n)};
  SweepParams p{};
  p.a = xn; p.na = n; p.b = xn; p.nb = n; p.d = d; p.n2a = n2; p.n2b = n2; p.k = k; p.part = part;
  cl_launch_sweep<CL_KNN>(p, c.stream, nullptr, strips);
  hipLaunchKernelGGL(cl_knn_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, c.stream, part, n, lists, k, sel);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(cl_refine_core_kernel, dim3((n + 3) / 4), dim3(256), 0, c.stream, xn, n, d, sel, o.core, o.core2, o.idx);
  FE_HIP(hipGetLastError());
  unsigned long long tail = 0;
  FE_HIP(hipMemcpyAsync(&tail, part + words, sizeof(tail), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipStreamSynchronize(c.stream));
  FE_CHECK(tail == CL_CANARY, "core distances: the word after the neighbour lists was overwritten");
  return o;
}

}  // namespace

int cluster_max_rounds(int n) {
  int lg = 0;
  while ((1ll << lg) < n) ++lg;                         // ceil(log2 n)
  return lg + 1;
}

void cluster_core_distances(Ctx& c, const float* x, int n, int d, int on_device, int normalise, int k, double* core, int32_t* core_idx) {
  DevMem mem;
  float *xn, *n2;
  cl_prepare(c, mem, x, n, d, on_device, normalise, xn, n2);
  const CoreDev cd = cl_core(c, mem, xn, n2, n, d, k);
  FE_HIP(hipMemcpyAsync(core, cd.core, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  if (core_idx) FE_HIP(hipMemcpyAsync(core_idx, cd.idx, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipStreamSynchronize(c.stream));
}

void cluster_mreach_mst(Ctx& c, const float* x, int n, int d, int on_device, int normalise, int k, int32_t* edge_u, int32_t* edge_v,
                        double* edge_w, double* core, int32_t* rounds_out) {
  DevMem mem;
  float *xn, *n2;
  cl_prepare(c, mem, x, n, d, on_device, normalise, xn, n2);
  const CoreDev cd = cl_core(c, mem, xn, n2, n, d, k);

  int* d_comp = mem.get<int>(n);
  unsigned long long* d_key = mem.get<unsigned long long>((size_t)n + 1);      // row keys, then a canary word
  FE_HIP(hipMemsetAsync(d_key + n, 0xA5, sizeof(unsigned long long), c.stream));
  std::vector<int> comp(n), parent(n);
  std::iota(comp.begin(), comp.end(), 0);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int v) {
    while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
    return v;
  };
  struct Cand { uint32_t w; int lo, hi; };
  std::vector<unsigned long long> keys((size_t)n + 1);
  std::vector<Cand> cand(n);
  std::vector<int32_t> eu, ev;
  eu.reserve(n - 1); ev.reserve(n - 1);
  const int max_rounds = cluster_max_rounds(n);
  int rounds = 0, ncomp = n;
  SweepParams p{};
  p.a = xn; p.na = n; p.b = xn; p.nb = n; p.d = d; p.n2a = n2; p.n2b = n2; p.core2 = cd.core2; p.comp = d_comp; p.rowkey = d_key;
  while (ncomp > 1) {
    FE_CHECK(rounds < max_rounds, "mreach_mst: %d components left after %d rounds (bound ceil(log2 n) + 1)", ncomp, rounds);
    FE_HIP(hipMemcpyAsync(d_comp, comp.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c.stream));
    FE_HIP(hipMemsetAsync(d_key, 0xFF, (size_t)n * sizeof(unsigned long long), c.stream));
    cl_launch_sweep<CL_BORUVKA>(p, c.stream);
    FE_HIP(hipMemcpyAsync(keys.data(), d_key, ((size_t)n + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
    FE_HIP(hipStreamSynchronize(c.stream));
    FE_CHECK(keys[n] == CL_CANARY, "mreach_mst: the word after the row keys was overwritten");
    // lightest edge per component under (mr^2 bits, min, max): the same order from both ends, so no round closes a cycle
    for (int i = 0; i < n; ++i) cand[i] = Cand{0xFFFFFFFFu, -1, -1};
    for (int i = 0; i < n; ++i) {
      const unsigned long long key = keys[i];
      FE_CHECK(key != CL_NONE, "mreach_mst: row %d found no edge to another component", i);
      const int j = (int)(uint32_t)(key & 0xFFFFFFFFull);
      FE_CHECK(j >= 0 && j < n && j != i, "mreach_mst: row %d reported column %d", i, j);
      const Cand e{(uint32_t)(key >> 32), std::min(i, j), std::max(i, j)};
      Cand& b = cand[comp[i]];
      if (b.lo < 0 || e.w < b.w || (e.w == b.w && (e.lo < b.lo || (e.lo == b.lo && e.hi < b.hi)))) b = e;
    }
    for (int ci = 0; ci < n; ++ci) {
      const Cand& e = cand[ci];
      if (e.lo < 0) continue;
      const int ru = find(e.lo), rv = find(e.hi);
      if (ru == rv) continue;                           // the edge both of its components chose
      parent[std::max(ru, rv)] = std::min(ru, rv);
      eu.push_back(e.lo); ev.push_back(e.hi);
      --ncomp;
    }
    for (int i = 0; i < n; ++i) comp[i] = find(i);
    ++rounds;
  }
  FE_CHECK((int)eu.size() == n - 1, "mreach_mst: %zu edges for %d points", eu.size(), n);
  int* d_eu = mem.get<int>(n);
  int* d_ev = mem.get<int>(n);
  double* d_ew = mem.get<double>(n);
  FE_HIP(hipMemcpyAsync(d_eu, eu.data(), (size_t)(n - 1) * sizeof(int), hipMemcpyHostToDevice, c.stream));
  FE_HIP(hipMemcpyAsync(d_ev, ev.data(), (size_t)(n - 1) * sizeof(int), hipMemcpyHostToDevice, c.stream));
  hipLaunchKernelGGL(cl_refine_edges_kernel, dim3((n - 1 + 3) / 4), dim3(256), 0, c.stream, xn, n, d, n - 1, d_eu, d_ev, cd.core, d_ew);
  FE_HIP(hipGetLastError());
  FE_HIP(hipMemcpyAsync(edge_w, d_ew, (size_t)(n - 1) * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  if (core) FE_HIP(hipMemcpyAsync(core, cd.core, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipStreamSynchronize(c.stream));
  std::copy(eu.begin(), eu.end(), edge_u);
  std::copy(ev.begin(), ev.end(), edge_v);
  if (rounds_out) *rounds_out = rounds;
}

void cluster_best_match(Ctx& c, const float* q, int nq, const float* cc, int nc, int d, float* best_sim, int32_t* best_idx) {
  DevMem mem;
  float *qn, *q2, *cn, *c2;
  cl_prepare(c, mem, q, nq, d, 0, 1, qn, q2);
  cl_prepare(c, mem, cc, nc, d, 0, 1, cn, c2);
  unsigned long long* d_key = mem.get<unsigned long long>((size_t)nq + 1);
  FE_HIP(hipMemsetAsync(d_key, 0xFF, (size_t)nq * sizeof(unsigned long long), c.stream));
  FE_HIP(hipMemsetAsync(d_key + nq, 0xA5, sizeof(unsigned long long), c.stream));
  SweepParams p{};
  p.a = qn; p.na = nq; p.b = cn; p.nb = nc; p.d = d; p.rowkey = d_key;
  cl_launch_sweep<CL_MATCH>(p, c.stream);
  std::vector<unsigned long long> keys((size_t)nq + 1);
  FE_HIP(hipMemcpyAsync(keys.data(), d_key, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipStreamSynchronize(c.stream));
  FE_CHECK(keys[nq] == CL_CANARY, "cosine_best_match: the word after the row keys was overwritten");
  for (int i = 0; i < nq; ++i) {
    FE_CHECK(keys[i] != CL_NONE, "cosine_best_match: row %d found no column", i);
    best_sim[i] = cl_sim_from_key((uint32_t)(keys[i] >> 32));
    best_idx[i] = (int32_t)(uint32_t)(keys[i] & 0xFFFFFFFFull);
  }
}

// ---- similar photos / merge suggestions -----------------------------------------------------------------------------------------
namespace {

template <typename T> const T* sim_to_device(Ctx& c, DevMem& mem, const T* src, size_t count, int on_device) {
  if (!src || on_device) return src;
  T* d = mem.get<T>(count);
  FE_HIP(hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, c.stream));
  return d;
}

// the rows of one side on the device: normalised (or copied up), or the caller's own when they are resident and taken as they are
const float* sim_rows(Ctx& c, DevMem& mem, const fe_sim_rows& r, int d) {
  if (!r.normalise && r.on_device) return r.emb;
  float *xn, *n2;
  cl_prepare(c, mem, r.emb, r.n, d, r.on_device, r.normalise, xn, n2);
  return xn;
}

SimSide sim_meta(Ctx& c, DevMem& mem, const fe_sim_rows& r) {
  if (!r.on_device && r.person_off) {                   // host lists can be checked here; device lists are clamped where they are read
    FE_CHECK(r.person_off[0] == 0 && r.person_off[r.n] == r.n_person_ids, "similar: person_off must run from 0 to n_person_ids");
    for (int i = 0; i < r.n; ++i) FE_CHECK(r.person_off[i] <= r.person_off[i + 1], "similar: person_off decreases at row %d", i);
  }
  SimSide out{};
  out.has_emb = sim_to_device(c, mem, r.has_emb, (size_t)r.n, r.on_device);
  out.date = reinterpret_cast<const long long*>(sim_to_device(c, mem, r.date, (size_t)r.n, r.on_device));
  out.agg = sim_to_device(c, mem, r.aggregate, (size_t)r.n, r.on_device);
  const bool persons = r.person_off && r.person_ids && r.n_person_ids > 0;
  out.poff = persons ? sim_to_device(c, mem, r.person_off, (size_t)r.n + 1, r.on_device) : nullptr;
  out.pid = persons ? sim_to_device(c, mem, r.person_ids, (size_t)r.n_person_ids, r.on_device) : nullptr;
  out.npid = persons ? r.n_person_ids : 0;
  return out;
}

SweepParams sim_params(Ctx& c, DevMem& mem, const fe_sim_rows& q, const fe_sim_rows& cand, int d, int cosine, const float* w, const int32_t* q_self,
                       const uint8_t* visible) {
  SweepParams p{};
  p.d = d; p.na = q.n; p.nb = cand.n;
  p.a = sim_rows(c, mem, q, d);
  // Q == C (every photo against every photo, the merge suggestions): the rows are prepared once
  const bool same = q.emb == cand.emb && q.n == cand.n && q.on_device == cand.on_device && q.normalise == cand.normalise;
  p.b = same ? p.a : sim_rows(c, mem, cand, d);
  if (!cosine) { p.sim.q = sim_meta(c, mem, q); p.sim.c = sim_meta(c, mem, cand); }
  p.sim.q_self = sim_to_device(c, mem, q_self, (size_t)q.n, 0);
  p.sim.visible = sim_to_device(c, mem, visible, (size_t)cand.n, 0);
  p.sim.cosine = cosine ? 1 : 0;
  if (w) { p.sim.wc = w[0]; p.sim.wp = w[1]; p.sim.wd = w[2]; p.sim.ws = w[3]; }
  return p;
}

int sim_gemv_blocks(int nb) { return std::max(1, std::min(1024, (nb + 3) / 4)); }

template <int MODE> void sim_launch_gemv(SweepParams p, int blocks, hipStream_t s) {
  const size_t lds = (size_t)p.na * p.d * sizeof(float) + (MODE == SIM_TOPK ? (size_t)4 * p.na * p.k * sizeof(unsigned long long) : 0);
  hipLaunchKernelGGL(sim_gemv_kernel<MODE>, dim3(blocks), dim3(256), lds, s, p);   // at most 32 KB + 8 KB: below the static limit
  FE_HIP(hipGetLastError());
}

}  // namespace

void similar_topk(Ctx& c, const fe_sim_rows& q, const fe_sim_rows& cand, int d, int cosine, const float* w, const int32_t* q_self,
                  const uint8_t* visible, int k, int32_t* idx, float* score) {
  DevMem mem;
  SweepParams p = sim_params(c, mem, q, cand, d, cosine, w, q_self, visible);
  p.k = k;
  const bool gemv = q.n <= SIM_GEMV_Q;
  const int blocks = sim_gemv_blocks(cand.n);
  const int lists = gemv ? 4 * blocks : 2 * cl_strips(q.n, cand.n);
  const size_t words = (size_t)q.n * lists * k;
  unsigned long long* part = mem.get<unsigned long long>(words + 1);        // then a canary word, as cl_core does
  FE_HIP(hipMemsetAsync(part + words, 0xA5, sizeof(unsigned long long), c.stream));
  p.part = part;
  if (gemv) sim_launch_gemv<SIM_TOPK>(p, blocks, c.stream);
  else cl_launch_sweep<SIM_TOPK>(p, c.stream, nullptr, lists / 2);
  int* d_idx = mem.get<int>((size_t)q.n * k + 1);
  float* d_score = mem.get<float>((size_t)q.n * k);
  FE_HIP(hipMemsetAsync(d_idx + (size_t)q.n * k, 0xA5, sizeof(int), c.stream));
  hipLaunchKernelGGL(sim_merge_kernel, dim3(q.n), dim3(64), (size_t)lists, c.stream, part, lists, k, d_idx, d_score);
  FE_HIP(hipGetLastError());
  unsigned long long tail = 0;
  int tail2 = 0;
  FE_HIP(hipMemcpyAsync(&tail, part + words, sizeof(tail), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipMemcpyAsync(&tail2, d_idx + (size_t)q.n * k, sizeof(int), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipMemcpyAsync(idx, d_idx, (size_t)q.n * k * sizeof(int), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipMemcpyAsync(score, d_score, (size_t)q.n * k * sizeof(float), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipStreamSynchronize(c.stream));
  FE_CHECK(tail == CL_CANARY && (uint32_t)tail2 == 0xA5A5A5A5u, "similar_topk: a word after an output buffer was overwritten");
}

void similar_pairs(Ctx& c, const fe_sim_rows& q, const fe_sim_rows& cand, int d, int cosine, const float* w, const int32_t* q_self,
                   const uint8_t* visible, const float* thr, int n_thr, int upper, int64_t max_pairs, int32_t* pairs, float* scores, int64_t* count) {
  DevMem mem;
  SweepParams p = sim_params(c, mem, q, cand, d, cosine, w, q_self, visible);
  p.sim.upper = upper ? 1 : 0;
  p.sim.thr = sim_to_device(c, mem, thr, (size_t)n_thr, 0);
  p.sim.thr_stride = n_thr == 1 ? 0 : 1;
  // pairs [max_pairs][2], scores [max_pairs], then the counter and a canary word: a store past the capacity would show on them
  int* d_pairs = mem.get<int>((size_t)max_pairs * 2);
  float* d_scores = mem.get<float>((size_t)max_pairs + 4);
  unsigned long long* d_count = mem.get<unsigned long long>(2);
  FE_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), c.stream));
  FE_HIP(hipMemsetAsync(d_count + 1, 0xA5, sizeof(unsigned long long), c.stream));
  FE_HIP(hipMemsetAsync(d_scores + max_pairs, 0xA5, 4 * sizeof(float), c.stream));
  p.sim.cap = (unsigned long long)max_pairs; p.sim.pairs = d_pairs; p.sim.pscore = d_scores; p.sim.count = d_count;
  if (q.n <= SIM_GEMV_Q) sim_launch_gemv<SIM_PAIRS>(p, sim_gemv_blocks(cand.n), c.stream);
  else cl_launch_sweep<SIM_PAIRS>(p, c.stream);
  unsigned long long tail[2] = {0, 0};
  uint32_t guard[4] = {0, 0, 0, 0};
  FE_HIP(hipMemcpyAsync(tail, d_count, sizeof(tail), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipMemcpyAsync(guard, d_scores + max_pairs, sizeof(guard), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipStreamSynchronize(c.stream));
  FE_CHECK(tail[1] == CL_CANARY && guard[0] == 0xA5A5A5A5u, "similar_pairs: a word after an output buffer was overwritten");
  *count = (int64_t)tail[0];
  const size_t found = (size_t)tail[0];
  if (found && found <= (size_t)max_pairs) {
    std::vector<int32_t> hp(found * 2);
    std::vector<float> hs(found);
    FE_HIP(hipMemcpyAsync(hp.data(), d_pairs, found * 2 * sizeof(int), hipMemcpyDeviceToHost, c.stream));
    FE_HIP(hipMemcpyAsync(hs.data(), d_scores, found * sizeof(float), hipMemcpyDeviceToHost, c.stream));
    FE_HIP(hipStreamSynchronize(c.stream));
    // the order of arrival is the order the waves ran in; the caller gets ascending (q, c)
    std::vector<size_t> order(found);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      return hp[2 * a] != hp[2 * b] ? hp[2 * a] < hp[2 * b] : hp[2 * a + 1] < hp[2 * b + 1];
    });
    for (size_t i = 0; i < found; ++i) {
      pairs[2 * i] = hp[2 * order[i]]; pairs[2 * i + 1] = hp[2 * order[i] + 1];
      scores[i] = hs[order[i]];
    }
  }
}

}  // namespace fe
