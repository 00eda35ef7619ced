// The flash-attention tile of the Qwen-VL encoders and of the decoder's prefill: one wave = 32 queries, 32-key K / V tiles through
// double-buffered LDS, on v_mfma_f32_32x32x16_bf16. S^T = K Q^T with one query per accumulator column (the Q fragment stays in registers),
// online softmax per lane, the exponentiated accumulator rounded to bf16 IS the B operand of O^T += V^T P^T (registers 8s..8s+7 = k-step
// s; the V^T fragment takes the same permuted keys with two 8-byte LDS reads). K rows are copied into LDS as they are, V is transposed
// on its way in by a two-byte scatter. HD = 64 (Qwen3-VL tower), 80 (Qwen2-VL / Qwen2.5-VL towers: rows 80..95 of V^T are zeros) or 128
// (decoder prefill). The kernels own addressing, the key range and the mask; every step of the tile is a function here.
#pragma once
#include "fe_common.h"

namespace fe {

template <int HD>
struct VlmAttnTile {
  static_assert(HD == 64 || HD == 80 || HD == 128, "attention tile: head_dim 64, 80 or 128");
  static constexpr int KSTEPS = HD / 16;            // MFMAs per S tile
  static constexpr int DT = (HD + 31) / 32;         // 32-row d-tiles of O
  static constexpr int CPR = HD / 8;                // 16-byte chunks per key row
  static constexpr int CHUNKS = 32 * CPR;           // per 32-key tile
  static constexpr int KS = 2 * HD + 16;            // K tile row stride in bytes (conflict-free 16-byte reads over rows distinct mod 16)
  static constexpr int VS = 72;                     // V^T tile row stride in bytes (64 + 8)
  static constexpr int K_BYTES = 32 * KS, V_BYTES = 32 * DT * VS;      // one buffer of each
  static constexpr int pieces(int nt) { return (CHUNKS + nt - 1) / nt; }
  union F8 { uint4 u; fe_v4f f; };

  // this lane's Q fragment: query row `qrow` (h = lane >> 5 picks the 8-element half of every 16-wide k-step)
  static __device__ __forceinline__ void load_q(F8 (&qf)[KSTEPS], const bf16* qrow, int h) {
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) qf[s].u = *reinterpret_cast<const uint4*>(qrow + 16 * s + 8 * h);
  }
  // global -> registers: tile kt of K (leading dimension ldk) and V (ldv), the key clamped to last_key (such keys are masked after QK^T)
  template <int NT, int P>
  static __device__ __forceinline__ void load(uint4 (&kr)[P], uint4 (&vr)[P], const bf16* Kp, size_t ldk, const bf16* Vp, size_t ldv, int kt, int last_key, int t) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int c = t + i * NT;
      if (CHUNKS % NT == 0 || c < CHUNKS) {
        int key = kt * 32 + c / CPR;
        if (key > last_key) key = last_key;
        kr[i] = *reinterpret_cast<const uint4*>(Kp + (size_t)key * ldk + (c % CPR) * 8);
        vr[i] = *reinterpret_cast<const uint4*>(Vp + (size_t)key * ldv + (c % CPR) * 8);
      }
    }
  }
  // registers -> LDS: K rows copied, V transposed; keys from n_keys on give zero rows of V (their probabilities are zero anyway)
  template <int NT, int P>
  static __device__ __forceinline__ void store(char* Ks, char* Vs, const uint4 (&kr)[P], const uint4 (&vr)[P], int kt, int n_keys, int t) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int c = t + i * NT;
      if (CHUNKS % NT == 0 || c < CHUNKS) {
        const int key = c / CPR, d0 = (c % CPR) * 8;
        *reinterpret_cast<uint4*>(&Ks[key * KS + d0 * 2]) = kr[i];
        const bool live = kt * 32 + key < n_keys;
        const unsigned w[4] = {vr[i].x, vr[i].y, vr[i].z, vr[i].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned short v = live ? (unsigned short)((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xFFFFu)) : (unsigned short)0;
          *reinterpret_cast<unsigned short*>(&Vs[(d0 + e) * VS + key * 2]) = v;
        }
      }
    }
  }
  // rows HD .. 32 DT - 1 of both V^T buffers: zeros, never written again (nothing to do when HD fills its d-tiles)
  template <int NT>
  static __device__ __forceinline__ void zero_vt_tail(char (&Vs)[2][V_BYTES], int t) {
    if constexpr (HD % 32 != 0) {
      constexpr int W = (32 * DT - HD) * VS / 4;
      for (int i = t; i < 2 * W; i += NT) reinterpret_cast<unsigned*>(&Vs[i / W][HD * VS])[i % W] = 0u;
    }
  }
  // S^T tile: lane (r, h) gets the scores of query r against keys 4 h + (e & 3) + 8 (e >> 2) of the tile
  static __device__ __forceinline__ fe_f32x16 scores(const char* Ks, const F8 (&qf)[KSTEPS], int r, int h) {
    fe_f32x16 st;
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
    const char* kb = &Ks[r * KS + 16 * h];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      F8 kf;
      kf.u = *reinterpret_cast<const uint4*>(kb + 32 * s);
      st = fe_mfma16((const bf16*)nullptr, kf.f, qf[s].f, st);
    }
    return st;
  }
  // online softmax over tile kt: st becomes exp(scale * s - max), (m, l) the running max / sum, o is rescaled. dead(key) masks a key; a
  // query whose keys so far are all masked keeps m = -inf, l = 0 and a zero o (no -inf - -inf)
  template <class Dead>
  static __device__ __forceinline__ void softmax(fe_f32x16& st, float& m, float& l, fe_f32x16 (&o)[DT], float scale, int kt, int h, Dead dead) {
    const int kbase = kt * 32 + 4 * h;
    float tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = kbase + (e & 3) + 8 * (e >> 2);
      st[e] = dead(key) ? -INFINITY : st[e] * scale;
      tmax = fmaxf(tmax, st[e]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mn = fmaxf(m, tmax);
    const float msafe = mn == -INFINITY ? 0.f : mn;
    const float alpha = __expf(m - msafe);
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) { st[e] = __expf(st[e] - msafe); psum += st[e]; }
    psum += __shfl_xor(psum, 32);
    l = l * alpha + psum;
    m = mn;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
  }
  // O^T += V^T P^T over the DT d-tiles
  static __device__ __forceinline__ void pv(fe_f32x16 (&o)[DT], const fe_f32x16& st, const char* Vs, int r, int h) {
    const bf16* const tag = nullptr;
    const char* vb = &Vs[r * VS + 8 * h];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      F8 pf;
      pf.u = make_uint4(fe_pack2(tag, st[8 * s], st[8 * s + 1]), fe_pack2(tag, st[8 * s + 2], st[8 * s + 3]),
                        fe_pack2(tag, st[8 * s + 4], st[8 * s + 5]), fe_pack2(tag, st[8 * s + 6], st[8 * s + 7]));
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const uint2 a0 = *reinterpret_cast<const uint2*>(vb + dt * 32 * VS + 32 * s), a1 = *reinterpret_cast<const uint2*>(vb + dt * 32 * VS + 32 * s + 16);
        F8 v;
        v.u = make_uint4(a0.x, a0.y, a1.x, a1.y);
        o[dt] = fe_mfma16(tag, v.f, pf.f, o[dt]);
      }
    }
  }
  // this lane's HD / 2 outputs of its query row, normalised (a row without a live key: zeros, not 0 / 0)
  static __device__ __forceinline__ void write(bf16* op, const fe_f32x16 (&o)[DT], float l, int h) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = dt * 32 + 8 * g + 4 * h;
        if (HD % 32 == 0 || d0 < HD) st4(op + d0, make_float4(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv));
      }
  }
};

}  // namespace fe
