// Fused multi-head attention for head_dim 64: O = softmax(Q K^T) V, never materialising the score matrix. One kernel body for three
// operand formats. Stands behind torch.nn.MultiheadAttention inside open_clip's resblocks (reference call: model.encode_image,
// processing/scorer.py:662, in half precision on a GPU at :513-516) and pyiqa's CFANet layers (models/pyiqa_scorer.py:212).
//
// The shared tile (attn_fwd_body). One wave owns 32 queries; a workgroup (NW waves) shares 32-key K / V^T tiles through
// double-buffered LDS: the next tile is prefetched into registers while this one is computed, then stored to the other buffer.
//   S^T = K Q^T     A = K tile (rows = keys), B = the wave's Q fragment kept in registers (columns = queries)
//   online softmax  each lane owns ONE query (accumulator column) and 16 of the tile's 32 keys - register e holds key
//                   (e&3) + 8(e>>2) + 4*half; the other 16 sit in lane^32, so a row max / sum is 15 VALU ops + one cross-half shuffle
//   O^T += V^T P^T  the exponentiated S^T accumulator is the B operand, A = V^T tile (rows = d)
// Keys past Lk are clamped on load and masked after the QK^T product; queries past Lq are clamped and not stored.
// Q is pre-scaled by 1/sqrt(64) in the projection epilogue; V^T comes straight from the role-swapped projection GEMM.
//
// What each operand policy changes:
//   AttnF32      v_mfma_f32_32x32x2_f32: 32 MFMAs per tile for S^T, the accumulator used AS IS as the B operand of O^T (its key
//                order is exactly the k-slot pairing of the instruction); LDS rows of 68 / 36 floats; V bias added; __expf
//   AttnHalf<E>  E = bf16 | f16 (fe_common.h: fe_mfma16 / fe_pack2 overloads) on v_mfma_f32_32x32x16: 4 MFMAs per tile for S^T
//                (lane (r, h) reads 8 consecutive d: one ds_read_b128); P rounded pairwise to E only as the operand of P.V: registers
//                8s .. 8s+7 form the fragment of k-step s, whose element j is key 16s + 8(j>>2) + 4h + (j&3) - so the A operand takes
//                the same keys with two 8-byte LDS reads per step (the k order inside a step is free as long as both operands
//                agree); fp32 scores, softmax and O; LDS rows of 144 / 72 bytes; V bias added; __expf
//   AttnSplit    fp16 pairs hi + lo (~22 significant bits) for Q, K, V and P, every product as its three leading terms (lh + hl + hh,
//                small terms first): 12 matrix instructions per tile for S^T instead of 4, 12 for O^T instead of 4; hi | lo planes in
//                LDS; the output leaves as a pair again, no bias, no causal mask; expf. The attention of the split-operand CLIP tower
//                (ClipModel::split3, model_clip.hip), whose error budget against the fp32 path is 1e-3 on the FINAL scores: with
//                plain fp16 q / k / v / o the tower holds 4e-4 on the features, which an ill-conditioned aesthetic head turns into
//                1.7e-3. Attention is 4 % of the tower's multiply-adds.
#include <type_traits>

#include "fe_common.h"

namespace fe {

template <class T>
struct AttnParamsH {
  const T* q; int ldq;         // [B*Lq][ldq], head h at column h*64
  const T* k; int ldk;         // [B*Lk][ldk]
  const T* vt; int lp;         // [B][d_model][lp]  (V transposed, zero padded to lp >= roundup32(Lk))
  const float* bv;             // [d_model] V bias, added to the output (softmax rows sum to 1)
  T* o; int ldo;               // [B*Lq][ldo]
  int B, H, Lq, Lk, dmodel;
  int causal;                  // 1: key j is visible to query i only if j <= i (CLIP text tower)
};
struct AttnParams : AttnParamsH<float> {};   // a name of its own: kernel traces and profiles are keyed by the fp32 kernel's signature
struct AttnSplitParams {
  const f16* q; const f16* k; int ld; int lo_off;      // rows [B*L][ld]: hi at column c, lo at column lo_off + c (q pre-scaled)
  const f16* vt_hi; const f16* vt_lo; int lp;          // [B][d_model][lp], zero padded
  f16* o; int ldo; int o_lo_off;                       // [B*Lq][ldo]: hi | lo
  int B, H, Lq, Lk, dmodel;
};

// ---- staging, common to the three policies: one 32-key tile of K (rows = keys, 64 elements) and of V^T (64 rows = d, 32 keys) ------
template <class T>
struct AttnLds {
  static constexpr int KS = 64 * sizeof(T) + 16;                 // K tile row stride in bytes (68 floats | 144 B): conflict-free ds_read_b128
  static constexpr int VS = sizeof(T) == 4 ? 144 : 72;           // V^T tile row stride in bytes (36 floats | 64 + 8 B)
  static constexpr int K_BYTES = 32 * KS, V_BYTES = 64 * VS;     // one buffer of each
};
// A thread's share of the tile in flight: K in 16-byte chunks, V^T in 4-element pieces (8 per row). The prefetch registers are arrays
// of NATIVE vectors on purpose: arrays of HIP's uint4 / float4 (structs) hipcc keeps in memory even with fully unrolled static indices -
// in scratch (88 MB/image of WRITE_SIZE in the fp32 kernel's profile, 80 B/lane in the split kernel) or in 16 B/thread of extra LDS.
template <class T, int NT>
struct AttnStage {
  typedef unsigned U4 __attribute__((ext_vector_type(4)));
  typedef unsigned U2 __attribute__((ext_vector_type(2)));
  using V4 = std::conditional_t<sizeof(T) == 4, U4, U2>;
  static constexpr int KE = 16 / sizeof(T), KC = 64 / KE;        // elements per K chunk, chunks per K row
  static constexpr int KN = 32 * KC / NT, VN = 64 * 8 / NT;      // chunks / pieces per thread
  const T* Kp; int ldk;
  const T* Vp; int lp;
  U4 kr[KN];
  V4 vr[VN];
  __device__ __forceinline__ void load(int kt, int Lk, int t) {
#pragma unroll
    for (int i = 0; i < KN; ++i) {
      const int c = t + i * NT;
      int row = kt * 32 + c / KC;
      if (row > Lk - 1) row = Lk - 1;   // masked after the QK^T product
      kr[i] = *reinterpret_cast<const U4*>(Kp + (size_t)row * ldk + (c % KC) * KE);
    }
#pragma unroll
    for (int i = 0; i < VN; ++i) {
      const int c = t + i * NT;
      vr[i] = *reinterpret_cast<const V4*>(Vp + (size_t)(c >> 3) * lp + kt * 32 + (c & 7) * 4);   // pad = 0
    }
  }
  __device__ __forceinline__ void store(char* Ks, char* Vs, int t) const {
#pragma unroll
    for (int i = 0; i < KN; ++i) { const int c = t + i * NT; *reinterpret_cast<U4*>(&Ks[(c / KC) * AttnLds<T>::KS + (c % KC) * 16]) = kr[i]; }
#pragma unroll
    for (int i = 0; i < VN; ++i) { const int c = t + i * NT; *reinterpret_cast<V4*>(&Vs[(c >> 3) * AttnLds<T>::VS + (c & 7) * sizeof(V4)]) = vr[i]; }
  }
};

// ---- what the fp32 and the 2-byte policies share: one plane, causal flag, V bias in the epilogue ------------------------------------
template <class T, class ParamsT>
struct AttnDense {
  using Params = ParamsT;
  static constexpr int K_BYTES = AttnLds<T>::K_BYTES, V_BYTES = AttnLds<T>::V_BYTES;
  static __device__ __forceinline__ bool causal(const Params& p) { return p.causal; }
  static __device__ __forceinline__ float ex(float x) { return __expf(x); }
  static __device__ __forceinline__ const T* q_row(const Params& p, int b, int head, int qc) {
    return p.q + (size_t)b * p.Lq * p.ldq + head * 64 + (size_t)qc * p.ldq;
  }
  template <int NT>
  static __device__ __forceinline__ AttnStage<T, NT> stage(const Params& p, int b, int head) {
    return {p.k + (size_t)b * p.Lk * p.ldk + head * 64, p.ldk, p.vt + ((size_t)b * p.dmodel + head * 64) * p.lp, p.lp};
  }
  // O[q][head*64 + d] = O^T[d][q] / l + bv[d]; register e of tile dt is d = 32*dt + (e&3) + 8(e>>2) + 4h
  static __device__ __forceinline__ void write(const Params& p, int b, int head, int q, int h, const fe_f32x16& o0, const fe_f32x16& o1, float inv) {
    T* op = p.o + ((size_t)b * p.Lq + q) * p.ldo + head * 64;
    const float* bp = p.bv + head * 64;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = 8 * g + 4 * h;
      const float4 b0 = *reinterpret_cast<const float4*>(bp + d0);
      const float4 b1 = *reinterpret_cast<const float4*>(bp + 32 + d0);
      st4(op + d0, make_float4(o0[4 * g] * inv + b0.x, o0[4 * g + 1] * inv + b0.y, o0[4 * g + 2] * inv + b0.z, o0[4 * g + 3] * inv + b0.w));
      st4(op + 32 + d0, make_float4(o1[4 * g] * inv + b1.x, o1[4 * g + 1] * inv + b1.y, o1[4 * g + 2] * inv + b1.z, o1[4 * g + 3] * inv + b1.w));
    }
  }
};

struct AttnF32 : AttnDense<float, AttnParams> {
  struct Q {
    float4 f[8];
    __device__ __forceinline__ void load(const Params& p, int b, int head, int qc, int h) {
#pragma unroll
      for (int s = 0; s < 8; ++s) f[s] = *reinterpret_cast<const float4*>(q_row(p, b, head, qc) + 8 * s + 4 * h);
    }
  };
  static __device__ __forceinline__ fe_f32x16 scores(const char* Ks, const Q& q, int r, int h) {
    fe_f32x16 st;
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
    const char* kb = &Ks[r * AttnLds<float>::KS + 16 * h];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float4 kf = *reinterpret_cast<const float4*>(kb + 32 * s);
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, q.f[s].x, st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, q.f[s].y, st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, q.f[s].z, st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, q.f[s].w, st, 0, 0, 0);
    }
    return st;
  }
  static __device__ __forceinline__ void pv(fe_f32x16& o0, fe_f32x16& o1, const fe_f32x16& st, const char* Vs, int r, int h) {
    const char* vb = &Vs[r * AttnLds<float>::VS + 16 * h];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 v0 = *reinterpret_cast<const float4*>(vb + 32 * g);
      const float4 v1 = *reinterpret_cast<const float4*>(vb + 32 * AttnLds<float>::VS + 32 * g);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0.x, st[4 * g + 0], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1.x, st[4 * g + 0], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0.y, st[4 * g + 1], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1.y, st[4 * g + 1], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0.z, st[4 * g + 2], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1.z, st[4 * g + 2], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0.w, st[4 * g + 3], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1.w, st[4 * g + 3], o1, 0, 0, 0);
    }
  }
};

// ---- fragments of the 32x32x16 instructions, for AttnHalf and for each plane of AttnSplit -------------------------------------------
union AttnF8 { uint4 u; fe_v4f f; };
struct AttnQ8 {   // B operand of S^T = K Q^T: Q[query][16s + 8h .. +8]
  AttnF8 f[4];
  template <class E>
  __device__ __forceinline__ void load(const E* row, int h) {
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s].u = *reinterpret_cast<const uint4*>(row + 16 * s + 8 * h);
  }
};
// kb / vb: this lane's place in a K plane (key r, d from 8h) / a V^T plane (d = r, keys from 4h), formed by the caller as ONE value -
// folded into each fragment's index instead, its parts are added up again in every tile (1 to 3 more instructions per tile).
// K[key][16s + 8h .. +8]
static __device__ __forceinline__ fe_v4f attn_k8(const char* kb, int s) {
  AttnF8 k;
  k.u = *reinterpret_cast<const uint4*>(kb + 32 * s);
  return k.f;
}
// V^T[d][keys 16s + 4h .. +4 | 16s + 8 + 4h .. +4]
static __device__ __forceinline__ fe_v4f attn_v8(const char* vb, int s) {
  const uint2 a0 = *reinterpret_cast<const uint2*>(vb + 32 * s), a1 = *reinterpret_cast<const uint2*>(vb + 32 * s + 16);
  AttnF8 v;
  v.u = make_uint4(a0.x, a0.y, a1.x, a1.y);
  return v.f;
}
// registers 8s .. 8s+7 of x rounded pairwise to E: the B operand of k-step s
template <class E>
static __device__ __forceinline__ fe_v4f attn_p8(const E* tag, const fe_f32x16& x, int s) {
  AttnF8 pf;
  pf.u = make_uint4(fe_pack2(tag, x[8 * s], x[8 * s + 1]), fe_pack2(tag, x[8 * s + 2], x[8 * s + 3]),
                    fe_pack2(tag, x[8 * s + 4], x[8 * s + 5]), fe_pack2(tag, x[8 * s + 6], x[8 * s + 7]));
  return pf.f;
}

template <class E>
struct AttnHalf : AttnDense<E, AttnParamsH<E>> {
  using Params = AttnParamsH<E>;
  struct Q : AttnQ8 {
    __device__ __forceinline__ void load(const Params& p, int b, int head, int qc, int h) { AttnQ8::load(AttnHalf::q_row(p, b, head, qc), h); }
  };
  static __device__ __forceinline__ fe_f32x16 scores(const char* Ks, const Q& q, int r, int h) {
    const E* const tag = nullptr;
    fe_f32x16 st;
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
    const char* kb = &Ks[r * AttnLds<f16>::KS + 16 * h];
#pragma unroll
    for (int s = 0; s < 4; ++s) st = fe_mfma16(tag, attn_k8(kb, s), q.f[s].f, st);
    return st;
  }
  // k-step s uses accumulator registers 8s .. 8s+7 = keys 16s + 8(j>>2) + 4h + (j&3)
  static __device__ __forceinline__ void pv(fe_f32x16& o0, fe_f32x16& o1, const fe_f32x16& st, const char* Vs, int r, int h) {
    const E* const tag = nullptr;
    const char* vb = &Vs[r * AttnLds<f16>::VS + 8 * h];      // d = r; d = 32 + r lies 32 rows on
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const fe_v4f pf = attn_p8(tag, st, s);
      o0 = fe_mfma16(tag, attn_v8(vb, s), pf, o0);
      o1 = fe_mfma16(tag, attn_v8(vb + 32 * AttnLds<f16>::VS, s), pf, o1);
    }
  }
};

struct AttnSplit {
  using Params = AttnSplitParams;
  using L = AttnLds<f16>;
  static constexpr int K_BYTES = 2 * L::K_BYTES, V_BYTES = 2 * L::V_BYTES;   // hi | lo planes
  static __device__ __forceinline__ bool causal(const Params&) { return false; }
  static __device__ __forceinline__ float ex(float x) { return expf(x); }
  struct Q {
    AttnQ8 hi, lo;
    __device__ __forceinline__ void load(const Params& p, int b, int head, int qc, int h) {
      const f16* row = p.q + (size_t)b * p.Lq * p.ld + head * 64 + (size_t)qc * p.ld;
      hi.load(row, h);
      lo.load(row + p.lo_off, h);
    }
  };
  template <int NT>
  struct Stage {
    AttnStage<f16, NT> hi, lo;
    __device__ __forceinline__ void load(int kt, int Lk, int t) { hi.load(kt, Lk, t); lo.load(kt, Lk, t); }
    __device__ __forceinline__ void store(char* Ks, char* Vs, int t) const {
      hi.store(Ks, Vs, t);
      lo.store(Ks + L::K_BYTES, Vs + L::V_BYTES, t);
    }
  };
  template <int NT>
  static __device__ __forceinline__ Stage<NT> stage(const Params& p, int b, int head) {
    const f16* Kp = p.k + (size_t)b * p.Lk * p.ld + head * 64;
    const size_t v0 = ((size_t)b * p.dmodel + head * 64) * p.lp;
    return {{Kp, p.ld, p.vt_hi + v0, p.lp}, {Kp + p.lo_off, p.ld, p.vt_lo + v0, p.lp}};
  }
  static __device__ __forceinline__ fe_f32x16 scores(const char* Ks, const Q& q, int r, int h) {
    const f16* const tag = nullptr;
    fe_f32x16 st;
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
    const char* kb = &Ks[r * AttnLds<f16>::KS + 16 * h];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const fe_v4f kh = attn_k8(kb, s), kl = attn_k8(kb + L::K_BYTES, s);
      st = fe_mfma16(tag, kl, q.hi.f[s].f, st);      // small terms first
      st = fe_mfma16(tag, kh, q.lo.f[s].f, st);
      st = fe_mfma16(tag, kh, q.hi.f[s].f, st);
    }
    return st;
  }
  static __device__ __forceinline__ void pv(fe_f32x16& o0, fe_f32x16& o1, const fe_f32x16& st, const char* Vs, int r, int h) {
    const f16* const tag = nullptr;
    const char* vb = &Vs[r * L::VS + 8 * h];
    fe_f32x16 lo;   // what the rounding of P to fp16 leaves behind
#pragma unroll
    for (int e = 0; e < 16; ++e) lo[e] = st[e] - (float)fe_to_f16(st[e]);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const fe_v4f ph = attn_p8(tag, st, s), pl = attn_p8(tag, lo, s);
      const fe_v4f v0h = attn_v8(vb, s), v1h = attn_v8(vb + 32 * L::VS, s);
      const fe_v4f v0l = attn_v8(vb + L::V_BYTES, s), v1l = attn_v8(vb + L::V_BYTES + 32 * L::VS, s);
      o0 = fe_mfma16(tag, v0l, ph, o0); o0 = fe_mfma16(tag, v0h, pl, o0); o0 = fe_mfma16(tag, v0h, ph, o0);
      o1 = fe_mfma16(tag, v1l, ph, o1); o1 = fe_mfma16(tag, v1h, pl, o1); o1 = fe_mfma16(tag, v1h, ph, o1);
    }
  }
  // each normalised output as hi = fp16(x) at column d, lo = x - hi at column o_lo_off + d
  static __device__ __forceinline__ void write(const Params& p, int b, int head, int q, int h, const fe_f32x16& o0, const fe_f32x16& o1, float inv) {
    f16* op = p.o + ((size_t)b * p.Lq + q) * p.ldo + head * 64;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = 8 * g + 4 * h;
      const float4 a = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
      const float4 c = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
      const float4 ah = make_float4((float)fe_to_f16(a.x), (float)fe_to_f16(a.y), (float)fe_to_f16(a.z), (float)fe_to_f16(a.w));
      const float4 ch = make_float4((float)fe_to_f16(c.x), (float)fe_to_f16(c.y), (float)fe_to_f16(c.z), (float)fe_to_f16(c.w));
      st4(op + d0, ah); st4(op + 32 + d0, ch);
      st4(op + p.o_lo_off + d0, make_float4(a.x - ah.x, a.y - ah.y, a.z - ah.z, a.w - ah.w));
      st4(op + p.o_lo_off + 32 + d0, make_float4(c.x - ch.x, c.y - ch.y, c.z - ch.z, c.w - ch.w));
    }
  }
};

// ---- the tile ------------------------------------------------------------------------------------------------------------------------
template <class P, int NW>
__device__ __forceinline__ void attn_fwd_body(const typename P::Params& p) {
  __shared__ __attribute__((aligned(16))) char Ks[2][P::K_BYTES];
  __shared__ __attribute__((aligned(16))) char Vs[2][P::V_BYTES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, b = bh / p.H, head = bh - b * p.H;
  const int q = (blockIdx.x * NW + wave) * 32 + r;
  const bool qok = q < p.Lq;
  typename P::Q qf;
  qf.load(p, b, head, qok ? q : p.Lq - 1, h);
  auto stage = P::template stage<NW * 64>(p, b, head);

  fe_f32x16 o0, o1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
  float m = -INFINITY, l = 0.f;

  const int nt = (p.Lk + 31) / 32;
  stage.load(0, p.Lk, t);
  stage.store(Ks[0], Vs[0], t);
  __syncthreads();
  for (int kt = 0; kt < nt; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nt) stage.load(kt + 1, p.Lk, t);
    fe_f32x16 st = P::scores(Ks[buf], qf, r, h);
    // online softmax over this lane's query
    const int kbase = kt * 32 + 4 * h;
    float tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = kbase + (e & 3) + 8 * (e >> 2);
      if (key >= p.Lk || (P::causal(p) && key > q)) st[e] = -INFINITY;
      tmax = fmaxf(tmax, st[e]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mn = fmaxf(m, tmax);
    const float alpha = P::ex(m - mn);          // exp(-inf) = 0 on the first tile
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) { st[e] = P::ex(st[e] - mn); psum += st[e]; }
    psum += __shfl_xor(psum, 32);
    l = l * alpha + psum;
    m = mn;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
    P::pv(o0, o1, st, Vs[buf], r, h);
    if (kt + 1 < nt) stage.store(Ks[buf ^ 1], Vs[buf ^ 1], t);
    __syncthreads();
  }
  if (qok) P::write(p, b, head, q, h, o0, o1, 1.f / l);
}

template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_kernel(const AttnParams p) { attn_fwd_body<AttnF32, NW>(p); }
template <class E, int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_bf16_kernel(const AttnParamsH<E> p) { attn_fwd_body<AttnHalf<E>, NW>(p); }
template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_split_kernel(const AttnSplitParams p) { attn_fwd_body<AttnSplit, NW>(p); }

// 4 waves (128 queries) per workgroup when that wastes little; 2 waves for short / ragged sequences (CLIP: 257). A policy without a
// 2-wave kernel (k2 = nullptr) always takes 4.
template <class Params>
static void attn_launch(void (*k4)(Params), void (*k2)(Params), const Params& p, hipStream_t s) {
  const int w4 = (p.Lq + 127) / 128 * 128, w2 = (p.Lq + 63) / 64 * 64;
  if (k2 == nullptr || w4 * 100 <= w2 * 108) {
    hipLaunchKernelGGL(k4, dim3((p.Lq + 127) / 128, p.B * p.H), dim3(256), 0, s, p);
  } else {
    hipLaunchKernelGGL(k2, dim3((p.Lq + 63) / 64, p.B * p.H), dim3(128), 0, s, p);
  }
  FE_HIP(hipGetLastError());
}

void launch_attention(const float* q, int ldq, const float* k, int ldk, const float* vt, int lp, const float* bv, float* o,
                      int ldo, int B, int H, int Lq, int Lk, int dmodel, int causal, hipStream_t s) {
  FE_CHECK(dmodel == H * 64, "attention kernel is built for head_dim 64 (d_model %d, %d heads)", dmodel, H);
  FE_CHECK(ldq % 4 == 0 && ldk % 4 == 0 && lp % 4 == 0 && ldo % 4 == 0 && lp >= (Lk + 31) / 32 * 32, "attention: strides");
  FE_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)bv | (uintptr_t)o) & 15) == 0, "attention: alignment");
  const AttnParams p{{q, ldq, k, ldk, vt, lp, bv, o, ldo, B, H, Lq, Lk, dmodel, causal}};
  attn_launch<AttnParams>(attn_fwd_kernel<4>, attn_fwd_kernel<2>, p, s);
}

template <class E>
static void launch_attention_half(const E* q, int ldq, const E* k, int ldk, const E* vt, int lp, const float* bv, E* o,
                                  int ldo, int B, int H, int Lq, int Lk, int dmodel, int causal, hipStream_t s) {
  FE_CHECK(dmodel == H * 64, "attention kernel is built for head_dim 64 (d_model %d, %d heads)", dmodel, H);
  FE_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && lp % 4 == 0 && ldo % 4 == 0 && lp >= (Lk + 31) / 32 * 32, "attention(2-byte): strides");
  FE_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)bv) & 15) == 0 && (((uintptr_t)vt | (uintptr_t)o) & 7) == 0, "attention(2-byte): alignment");
  const AttnParamsH<E> p{q, ldq, k, ldk, vt, lp, bv, o, ldo, B, H, Lq, Lk, dmodel, causal};
  attn_launch<AttnParamsH<E>>(attn_fwd_bf16_kernel<E, 4>, attn_fwd_bf16_kernel<E, 2>, p, s);
}
void launch_attention(const bf16* q, int ldq, const bf16* k, int ldk, const bf16* vt, int lp, const float* bv, bf16* o,
                      int ldo, int B, int H, int Lq, int Lk, int dmodel, int causal, hipStream_t s) {
  launch_attention_half(q, ldq, k, ldk, vt, lp, bv, o, ldo, B, H, Lq, Lk, dmodel, causal, s);
}
void launch_attention(const f16* q, int ldq, const f16* k, int ldk, const f16* vt, int lp, const float* bv, f16* o,
                      int ldo, int B, int H, int Lq, int Lk, int dmodel, int causal, hipStream_t s) {
  launch_attention_half(q, ldq, k, ldk, vt, lp, bv, o, ldo, B, H, Lq, Lk, dmodel, causal, s);
}

void launch_attention_split(const f16* q, const f16* k, int ld, int lo_off, const f16* vt_hi, const f16* vt_lo, int lp, f16* o, int ldo, int o_lo_off,
                            int B, int H, int Lq, int Lk, int dmodel, hipStream_t s) {
  FE_CHECK(dmodel == H * 64 && ld % 8 == 0 && lo_off % 8 == 0 && lp % 4 == 0 && ldo % 4 == 0 && o_lo_off % 4 == 0 && lp >= (Lk + 31) / 32 * 32, "attention(split): geometry");
  FE_CHECK((((uintptr_t)q | (uintptr_t)k) & 15) == 0 && (((uintptr_t)vt_hi | (uintptr_t)vt_lo | (uintptr_t)o) & 7) == 0, "attention(split): alignment");
  const AttnSplitParams p{q, k, ld, lo_off, vt_hi, vt_lo, lp, o, ldo, o_lo_off, B, H, Lq, Lk, dmodel};
  attn_launch<AttnSplitParams>(attn_fwd_split_kernel<4>, nullptr, p, s);
}

}  // namespace fe
