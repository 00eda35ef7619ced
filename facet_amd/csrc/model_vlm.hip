// VLM tagger, slice 1: the text decoder of Qwen2.5-VL (SURVEY 8(f)-4 / BASELINE configs[4]) - prefill + single-token decode with a
// contiguous KV cache, greedy next-token selection.
//
// Stands behind reference models/vlm_tagger.py: `Qwen2_5_VLForConditionalGeneration.from_pretrained(..., dtype=torch.bfloat16)`
// (:163-184) and `self.model.generate(**inputs, max_new_tokens=..., do_sample=False)` (:250-259, :355-360). The arithmetic is
// transformers' (modeling_qwen2_5_vl.py: Qwen2_5_VLDecoderLayer = RMSNorm -> q/k/v projections with bias -> multimodal rotary
// embedding (sections 16/24/24 over the 64 frequency pairs of head_dim 128) -> grouped-query causal attention -> o_proj -> residual ->
// RMSNorm -> SwiGLU MLP -> residual; final RMSNorm; untied lm_head), restated here in the precision the reference loads: bf16 storage
// of every activation with the SAME rounding points as the bf16 torch modules (each Linear output, RMSNorm's normalised value before the
// weight multiply, both products of the rotary embedding, SiLU before the gate multiply, each residual sum, the logits), fp32
// accumulation inside every contraction. Parity: tests/test_vlm_gpu.py against vectors of the reference's own model class
// (tests/golden/make_vlm_golden.py) - pinned.
// Not in this slice: the vision tower (window attention, patch merger) and fp8 matrix-core attention; image tokens enter as rows of `embeds`.
// KV-cache storage: bf16, or (FE_VLM_KV_E4M3) e4m3 rows with one power-of-two scale each, read by a decode attention kernel of their own -
// see "KV-cache formats" below.
// Weight storage: bf16, or (FE_VLM_WEIGHTS_E4M3) e4m3 rows with one power-of-two scale each (fp8_core.h) for the Linear layers - the
// same arithmetic on other weight values, see "e4m3 weights" below.
#include "engine.h"
#include "fp8_core.h"
#include "vlm_attn_tile.h"
#include <type_traits>
#include <cmath>
#include <cstring>

namespace fe {

__device__ __forceinline__ void h_unpack8_bf16(const uint4 u, float v[8]) {
  const bf16* tag = nullptr;
  fe_unpack2(tag, u.x, v[0], v[1]); fe_unpack2(tag, u.y, v[2], v[3]); fe_unpack2(tag, u.z, v[4], v[5]); fe_unpack2(tag, u.w, v[6], v[7]);
}

// ---- small row kernels ------------------------------------------------------------------------------------------------------------
// x[row][:] = E[tok[row]][:]   (bf16 table)
__global__ void vlm_embed_kernel(const int* __restrict__ tok, const bf16* __restrict__ E, bf16* __restrict__ x, int rows, int d, int vocab) {
  const size_t total = (size_t)rows * (d / 8);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / (d / 8)), c = (int)(i % (d / 8)) * 8;
    int t = tok[row];
    t = t < 0 ? 0 : (t >= vocab ? vocab - 1 : t);
    *reinterpret_cast<uint4*>(x + (size_t)row * d + c) = *reinterpret_cast<const uint4*>(E + (size_t)t * d + c);
  }
}

// transformers' RMSNorm in bf16: x32 = float(x); y = w * bf16(x32 * rsqrt(mean(x32^2) + eps)), the product rounded to bf16.
// One wave per row; d, ldx and ldy multiples of 4: a lane moves 4 values (8 bytes) at a time, the last trip over a row may be partial
// (vlm_rmsnorm checks it).
__global__ void vlm_rmsnorm_kernel(const bf16* __restrict__ x, int ldx, const bf16* __restrict__ w, bf16* __restrict__ y, int ldy, int rows, int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int row = wave; row < rows; row += nwaves) {
    const bf16* xr = x + (size_t)row * ldx;
    float ss = 0.f;
    for (int i = lane * 4; i < d; i += 256) { const float4 v = ld4(xr + i); ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float rs = rsqrtf(ss / (float)d + eps);
    bf16* yr = y + (size_t)row * ldy;
    for (int i = lane * 4; i < d; i += 256) {
      const float4 v = ld4(xr + i), g = ld4(w + i);
      st4(yr + i, make_float4(g.x * (float)(bf16)(v.x * rs), g.y * (float)(bf16)(v.y * rs), g.z * (float)(bf16)(v.z * rs), g.w * (float)(bf16)(v.w * rs)));
    }
  }
}

// ---- KV-cache formats (FE_VLM_KV_*, fe_vlm_set_kv_format) --------------------------------------------------------------------------------
// One cache row = the 128 values of one (sequence, KV head, position), K and V separately. FE_VLM_KV_E4M3 stores it as 128 OCP e4m3 codes
// and the fp32 scale 2^e of fp8_core.h's row rule (codes [B][nkv][max_seq][128] uint8, scales [B][nkv][max_seq]): 132 bytes instead of 256.
// Every dequantised value is exactly a bf16 value, so the engine under it is the bf16 engine whose cache rows were replaced by
// dequantize(quantize(row)); FE_VLM_KV_BF16_E4M3 stores exactly those rows in a bf16 cache (the arithmetic of the format at the storage of
// bf16: it separates what the format costs from what the e4m3 kernels do, for tests and accuracy studies).
// The store of one row held by a wave, lane l owning dims l and l + 64 (the layout of both rope kernels): the row maximum is a wave
// reduction over the magnitudes' bit patterns (monotone for non-negative floats; a NaN or Inf sorts above every finite value), then
// row_exponent / e4m3_encode of fp8_core.h, so the bits are the host's. A row with a NaN or Inf becomes NaN codes with scale 1.
// `cache` is the bf16 cache, or (E4M3) the code array; `ri` the row index (b * nkv + head) * max_seq + position.
template <int KV>
__device__ __forceinline__ void vlm_kv_store_row(bf16* __restrict__ cache, float* __restrict__ scales, const size_t ri, const int lane, const bf16 r1, const bf16 r2) {
  if constexpr (KV == FE_VLM_KV_BF16) {
    bf16* dst = cache + ri * 128;
    dst[lane] = r1; dst[lane + 64] = r2;
  } else {
    const float x1 = (float)r1, x2 = (float)r2;
    uint32_t a = max(fp8::f32_bits(x1) & 0x7FFFFFFFu, fp8::f32_bits(x2) & 0x7FFFFFFFu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = max(a, (uint32_t)__shfl_xor((int)a, o));
    const bool finite = a < 0x7F800000u;
    const int e = finite ? fp8::row_exponent(fp8::bits_f32(a)) : 0;
    const float inv = fp8::row_scale(-e), sc = fp8::row_scale(e);
    const uint8_t c1 = finite ? fp8::e4m3_encode(x1 * inv) : (uint8_t)0x7F, c2 = finite ? fp8::e4m3_encode(x2 * inv) : (uint8_t)0x7F;
    if constexpr (KV == FE_VLM_KV_E4M3) {
      uint8_t* dst = reinterpret_cast<uint8_t*>(cache) + ri * 128;
      dst[lane] = c1; dst[lane + 64] = c2;
      if (lane == 0) scales[ri] = sc;
    } else {      // the image of the row, exactly bf16 values
      bf16* dst = cache + ri * 128;
      dst[lane] = (bf16)(fp8::e4m3_decode(c1) * sc); dst[lane + 64] = (bf16)(fp8::e4m3_decode(c2) * sc);
    }
  }
}
// rows [n][L][128] bf16 (a prefill's K or V of one layer, n = sequences x KV heads) -> positions 0 .. L - 1 of a cache in format KV. One
// wave per row. The prefill under the e4m3 formats attends to the unquantised rows and fills the cache with this pass.
template <int KV>
__global__ void vlm_kv_fill_kernel(const bf16* __restrict__ ksrc, const bf16* __restrict__ vsrc, bf16* __restrict__ kc, bf16* __restrict__ vc, float* __restrict__ ksc,
                                   float* __restrict__ vsc, int n, int L, int max_seq) {
  const int lane = threadIdx.x & 63;
  const size_t total = (size_t)2 * n * L, nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t wv = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv < total; wv += nwaves) {
    const bool isv = wv >= (size_t)n * L;
    const size_t r = isv ? wv - (size_t)n * L : wv;
    const bf16* src = (isv ? vsrc : ksrc) + r * 128;
    const size_t ri = (r / L) * max_seq + r % L;
    vlm_kv_store_row<KV>(isv ? vc : kc, isv ? vsc : ksc, ri, lane, src[lane], src[lane + 64]);
  }
}

// The tail both rope kernels share: rotate the pair (y1, y2) = dims (d, d + 64) of head hd by `ang`, then append it to the K cache or write
// it to q_out. cos / sin are rounded to bf16 and y*cos, rotate_half(y)*sin and their sum are each rounded to bf16, as
// apply_multimodal_rotary_pos_emb does on bf16 tensors. A wave holds one (row, head) and lane d its pair d, so under the e4m3 formats
// the append quantises the row in place (vlm_kv_store_row). cpos: the row's position in the cache.
template <int KV>
__device__ __forceinline__ void vlm_rope_rotate_append(const float y1, const float y2, const float ang, const int hd, const int nh, const int nkv, const int d,
                                                       const int row, const int b, const int cpos, const int max_seq, bf16* __restrict__ q_out,
                                                       bf16* __restrict__ kc, float* __restrict__ ksc) {
  const float c = (float)(bf16)cosf(ang), s = (float)(bf16)sinf(ang);
  const bf16 o1 = (bf16)((float)(bf16)(y1 * c) + (float)(bf16)(-y2 * s));
  const bf16 o2 = (bf16)((float)(bf16)(y2 * c) + (float)(bf16)(y1 * s));
  if (hd >= nh) {      // (wave-uniform)
    vlm_kv_store_row<KV>(kc, ksc, ((size_t)b * nkv + (hd - nh)) * max_seq + cpos, d, o1, o2);
    return;
  }
  bf16* dst = q_out + ((size_t)row * nh + hd) * 128;
  dst[d] = o1; dst[d + 64] = o2;
}

// Multimodal rotary embedding on the q and k heads of a fused QKV row block + the KV-cache append (Qwen2 / 2.5).
//   qkv: [rows][(nh + 2 nkv) * 128]; pos: [3][rows] (temporal, height, width position of every token; equal for text tokens)
//   q_out: [rows][nh * 128]; kc / vc: cache [B][nkv][max_seq][128], row `row` = (b, t) lands at position start + t.
// Dimension i of a head takes frequency i % 64 and the position component of its section (sections doubled over the two halves:
// [16, 24, 24, 16, 24, 24]). One thread per (row, head, pair d < 64); a wave covers exactly one (row, head) per loop trip (64 lanes = the
// 64 pairs). KV: the cache format; K and V rows reach the cache through vlm_kv_store_row alone (ksc / vsc: the scale arrays of
// FE_VLM_KV_E4M3, kc / vc then the code arrays).
template <int KV>
__global__ void vlm_rope_cache_kernel(const bf16* __restrict__ qkv, const int* __restrict__ pos, const float* __restrict__ inv_freq, bf16* __restrict__ q_out,
                                      bf16* __restrict__ kc, bf16* __restrict__ vc, int rows, int L, int nh, int nkv, int s0, int s1, int start, int max_seq,
                                      const int* __restrict__ start_dev, float* __restrict__ ksc, float* __restrict__ vsc) {
  if (start_dev) start = *start_dev;      // decode steps replayed from a captured graph: the cache length lives in device memory
  const int heads = nh + 2 * nkv;
  const size_t total = (size_t)rows * heads * 64;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i & 63), hd = (int)((i >> 6) % heads), row = (int)(i / ((size_t)heads * 64));
    const bf16* src = qkv + ((size_t)row * heads + hd) * 128;
    const int b = row / L, t = row - b * L;
    if (hd >= nh + nkv) {      // V: plain copy into the cache
      vlm_kv_store_row<KV>(vc, vsc, ((size_t)b * nkv + (hd - nh - nkv)) * max_seq + start + t, d, src[d], src[d + 64]);
      continue;
    }
    const int comp = d < s0 ? 0 : (d < s0 + s1 ? 1 : 2);
    const float ang = (float)pos[(size_t)comp * rows + row] * inv_freq[d];
    vlm_rope_rotate_append<KV>((float)src[d], (float)src[d + 64], ang, hd, nh, nkv, d, row, b, start + t, max_seq, q_out, kc, ksc);
  }
}

// Qwen3-VL form of vlm_rope_cache_kernel: q_norm / k_norm (RMSNorm over each head's 128 dims), then the INTERLEAVED multimodal rotary
// embedding, then the KV-cache append - one pass over the fused q|k|v rows. One wave per (row, head); lane l owns dims l and l + 64 (the
// rotate_half pair of frequency l).
//   norm: the fp32 sum of squares over the wave, n = bf16(x * rsqrt(mean + eps)), y = bf16(w * n)   (Qwen3VLTextRMSNorm on a bf16 tensor)
//   rope: frequency j takes the height position when j % 3 == 1 and j < 3 s1, the width position when j % 3 == 2 and j < 3 s2, the temporal
//         one otherwise (apply_interleaved_mrope); the rotation and the append are vlm_rope_rotate_append
// KV, ksc, vsc: the cache format, as in vlm_rope_cache_kernel
template <int KV>
__global__ void vlm3_qk_rope_cache_kernel(const bf16* __restrict__ qkv, const int* __restrict__ pos, const float* __restrict__ inv_freq, const bf16* __restrict__ qn,
                                          const bf16* __restrict__ kn, bf16* __restrict__ q_out, bf16* __restrict__ kc, bf16* __restrict__ vc, int rows, int L, int nh,
                                          int nkv, int s1, int s2, int start, int max_seq, const int* __restrict__ start_dev, float eps, float* __restrict__ ksc,
                                          float* __restrict__ vsc) {
  if (start_dev) start = *start_dev;      // decode steps replayed from a captured graph: the cache length lives in device memory
  const int lane = threadIdx.x & 63;
  const int heads = nh + 2 * nkv;
  const size_t total = (size_t)rows * heads;
  const size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
  const int j = lane;
  const int comp = (j % 3 == 1 && j < 3 * s1) ? 1 : ((j % 3 == 2 && j < 3 * s2) ? 2 : 0);
  const float fr = inv_freq[j];
  for (size_t wv = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv < total; wv += nwaves) {
    const int hd = (int)(wv % heads), row = (int)(wv / heads);
    const bf16* src = qkv + wv * 128;
    const int b = row / L, t = row - b * L;
    const bf16 r1 = src[lane], r2 = src[lane + 64];
    if (hd >= nh + nkv) {      // V: plain copy into the cache (wave-uniform branch)
      vlm_kv_store_row<KV>(vc, vsc, ((size_t)b * nkv + (hd - nh - nkv)) * max_seq + start + t, lane, r1, r2);
      continue;
    }
    const float x1 = (float)r1, x2 = (float)r2;
    float ss = x1 * x1 + x2 * x2;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float rs = rsqrtf(ss / 128.f + eps);
    const bf16* w = hd < nh ? qn : kn;
    const float y1 = (float)(bf16)((float)w[lane] * (float)(bf16)(x1 * rs)), y2 = (float)(bf16)((float)w[lane + 64] * (float)(bf16)(x2 * rs));
    vlm_rope_rotate_append<KV>(y1, y2, (float)pos[(size_t)comp * rows + row] * fr, hd, nh, nkv, lane, row, b, start + t, max_seq, q_out, kc, ksc);
  }
}

// h = bf16(bf16(silu(g)) * u)   (Qwen2MLP: act_fn(gate_proj(x)) * up_proj(x) on bf16 tensors)
__global__ void vlm_silu_mul_kernel(const bf16* g, const bf16* __restrict__ u, bf16* h, size_t n4) {      // h may be g
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = ld4(g + 4 * i), b = ld4(u + 4 * i);
    auto f = [](float x, float y) { return (float)(bf16)(x / (1.f + expf(-x))) * y; };
    st4(h + 4 * i, make_float4(f(a.x, b.x), f(a.y, b.y), f(a.z, b.z), f(a.w, b.w)));
  }
}
// x = bf16(x + y)
__global__ void vlm_add_kernel(bf16* __restrict__ x, const bf16* __restrict__ y, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = ld4(x + 4 * i), b = ld4(y + 4 * i);
    st4(x + 4 * i, make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w));
  }
}
// last[b][:] = x[b * L + L - 1][:]
__global__ void vlm_last_rows_kernel(const bf16* __restrict__ x, bf16* __restrict__ last, int B, int L, int d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * d) return;
  const int b = i / d, c = i - b * d;
  last[i] = x[((size_t)b * L + L - 1) * d + c];
}

// ---- prefill attention: causal, grouped-query, head_dim 128, on the bf16 matrix cores --------------------------------------------------
// One wave owns 32 queries; a workgroup (4 waves = 128 queries) shares 32-key K / V tiles through LDS: the tile of vlm_attn_tile.h (the
// vision towers' too) with 8 k-steps per S tile and four 32-row d-tiles of O. K / V come straight from the cache rows ([pos][128]).
struct VlmAttnParams {
  const bf16* q; int ldq;       // [B*Lq][nh*128]
  const bf16* kc; const bf16* vc;   // caches [B][nkv][max_seq][128]
  bf16* o; int ldo;             // [B*Lq][nh*128]
  int B, nh, nkv, Lq, Lk, max_seq, qpos0;      // query i sits at sequence position qpos0 + i and sees keys 0 .. qpos0 + i
  float scale;
  const int* pad;               // device [B]: sequence b's first pad[b] positions are left padding (masked keys, zero output rows)
};

__global__ __launch_bounds__(256, 2) void vlm_attn_prefill_kernel(const VlmAttnParams p) {
  using T = VlmAttnTile<128>;
  __shared__ __attribute__((aligned(16))) char Ks[2][T::K_BYTES];
  __shared__ __attribute__((aligned(16))) char Vs[2][T::V_BYTES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, b = bh / p.nh, head = bh - b * p.nh, kvh = head / (p.nh / p.nkv);
  const bf16* Qp = p.q + (size_t)b * p.Lq * p.ldq + head * 128;
  const bf16* Kp = p.kc + ((size_t)b * p.nkv + kvh) * p.max_seq * 128;
  const bf16* Vp = p.vc + ((size_t)b * p.nkv + kvh) * p.max_seq * 128;
  const int q = (blockIdx.x * 4 + wave) * 32 + r;
  const bool qok = q < p.Lq;
  const int qc = qok ? q : p.Lq - 1;
  const int qpos = p.qpos0 + q;
  const int padb = p.pad[b];
  T::F8 qf[T::KSTEPS];
  T::load_q(qf, Qp + (size_t)qc * p.ldq, h);
  // this workgroup's queries end at position qpos0 + (blockIdx.x + 1) * 128 - 1: later keys are masked for all of them
  const int kend = min(p.Lk, p.qpos0 + (int)(blockIdx.x + 1) * 128);
  const int nt = (kend + 31) / 32;
  // left padding: the key loop starts at the first 32-key tile that holds a live key (whole pad tiles cost nothing)
  const int kt0 = min(padb / 32, nt);
  uint4 kr[T::pieces(256)], vr[T::pieces(256)];
  fe_f32x16 o[T::DT];
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;
  T::load<256>(kr, vr, Kp, 128, Vp, 128, kt0, p.Lk - 1, t);
  T::store<256>(Ks[0], Vs[0], kr, vr, kt0, p.Lk, t);
  __syncthreads();
  for (int kt = kt0; kt < nt; ++kt) {
    const int buf = (kt - kt0) & 1;
    if (kt + 1 < nt) T::load<256>(kr, vr, Kp, 128, Vp, 128, kt + 1, p.Lk - 1, t);
    fe_f32x16 st = T::scores(Ks[buf], qf, r, h);
    // a query row whose keys so far are all masked (rows past Lq, pad rows) keeps a zero sum: it writes zeros
    T::softmax(st, m, l, o, p.scale, kt, h, [&](int key) { return (key >= p.Lk) | (key > qpos) | (key < padb); });
    T::pv(o, st, Vs[buf], r, h);
    if (kt + 1 < nt) T::store<256>(Ks[buf ^ 1], Vs[buf ^ 1], kr, vr, kt + 1, p.Lk, t);
    __syncthreads();
  }
  if (qok) T::write(p.o + ((size_t)b * p.Lq + q) * p.ldo + head * 128, o, l, h);
}

// x[index[i]][:] = rows[i][:]   (image embeddings into the rows of their <|image_pad|> tokens)
__global__ void vlm_put_rows_kernel(bf16* __restrict__ x, const bf16* __restrict__ rows, const int* __restrict__ index, int n, int d) {
  const size_t total = (size_t)n * (d / 8);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / (d / 8)), c = (int)(i % (d / 8)) * 8;
    *reinterpret_cast<uint4*>(x + (size_t)index[r] * d + c) = *reinterpret_cast<const uint4*>(rows + (size_t)r * d + c);
  }
}

// ---- e4m3 weights (FE_VLM_WEIGHTS_E4M3): a Linear layer is [Cout][KpH] codes (ConvW.w8) and [Cout] scales 2^e (ConvW.w8_scale), the format
// of fp8_core.h. Layout along K: PLAIN order, one byte per element, rows padded with zero codes to KpH (a multiple of 64) - code k of a
// row multiplies activation k. v_cvt_scalef32_pk_bf16_fp8 (scale 1) widens two neighbouring codes of a 32-bit word to a packed bf16 pair
// exactly (4 significant bits into 8), element 0 from the lower byte: 16 codes of a 16-byte load become the 8 pairs that face the 8
// dwords of 16 activations, with no permutation. The products and the fp32 sums are then those of the bf16 kernels; the row scale
// multiplies the fp32 sum (exact: a power of two) before the bias.
typedef __bf16 vlm_bf2 __attribute__((ext_vector_type(2)));
template <bool HI>
__device__ __forceinline__ unsigned vlm_e4m3_pair(const unsigned word) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, HI));
}
// 16 codes (K order) -> 16 bf16 (K order): lo = elements 0 .. 7, hi = 8 .. 15
__device__ __forceinline__ void vlm_e4m3_widen16(const uint4 c, uint4& lo, uint4& hi) {
  lo.x = vlm_e4m3_pair<false>(c.x); lo.y = vlm_e4m3_pair<true>(c.x); lo.z = vlm_e4m3_pair<false>(c.y); lo.w = vlm_e4m3_pair<true>(c.y);
  hi.x = vlm_e4m3_pair<false>(c.z); hi.y = vlm_e4m3_pair<true>(c.z); hi.z = vlm_e4m3_pair<false>(c.w); hi.w = vlm_e4m3_pair<true>(c.w);
}
// acc + the dot product of 8 bf16 pairs on v_dot2c_f32_bf16 (two bf16 pairs per instruction, fp32 accumulate): no unpacking of either
// operand - with it the 2- and 4-sequence GEMV steps were bound by the vector ALU, not by the weight stream
__device__ __forceinline__ float vlm_dot8(const uint4 p, const uint4 q, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(vlm_bf2, p.x), __builtin_bit_cast(vlm_bf2, q.x), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(vlm_bf2, p.y), __builtin_bit_cast(vlm_bf2, q.y), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(vlm_bf2, p.z), __builtin_bit_cast(vlm_bf2, q.z), acc, false);
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(vlm_bf2, p.w), __builtin_bit_cast(vlm_bf2, q.w), acc, false);
}

// ---- decode GEMV: y[m][n] = sum_k x[m][k] w[n][k] (+ bias) for M <= 4 sequences - the shape of every projection of a decode step at the
// reference's batch sizes (vlm_batch_size 2, models/vlm_tagger.py:76). Pure weight streaming: one wave per TWO output columns, 16-byte
// loads, the M activation rows come from L1 / L2; fp32 accumulation, one rounding to bf16 (or fp32 out for the logits). HBM-bound.
// WT = bf16: E = 8 weights per lane and load, N * K * 2 bytes per launch; K % 8 == 0.
// WT = uint8_t: e4m3 rows (above), E = 16 codes per lane and load, N * K bytes per launch; K % 16 == 0. The conversion is 8 instructions
// per 16 weights of a column, shared by the M rows: against the 16 M dot instructions of those weights it leaves the 2- and 4-row steps
// where the bf16 weights have them. The row scale (wscale; unused for bf16) multiplies the merged fp32 sum before the bias.
template <int MR, class TO, class WT>
__global__ __launch_bounds__(256) void vlm_gemv_kernel(const bf16* __restrict__ x, int ldx, const WT* __restrict__ w, int ldw, const float* __restrict__ wscale,
                                                       const float* __restrict__ bias, TO* __restrict__ y, int ldy, int M, int N, int K) {
  constexpr bool F8 = sizeof(WT) == 1;
  constexpr int E = F8 ? 16 : 8, STEP = 256 * E;
  // one workgroup = two output columns; its four waves take interleaved 64 E-column steps of K (so even the 3584-column projections put
  // 7 waves on every SIMD) and meet in LDS
  __shared__ float red[4][MR][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 2;
  const bool two = n0 + 1 < N;
  const WT* w0 = w + (size_t)n0 * ldw;
  const WT* w1 = w + (size_t)(two ? n0 + 1 : n0) * ldw;
  float a0[MR], a1[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) { a0[m] = 0.f; a1[m] = 0.f; }
  // one load's weights of both columns against activations k .. k + E - 1 of every row (e4m3: the low 8, then the high 8)
  auto fma_step = [&](const uint4 wa, const uint4 wb, const int k) __attribute__((always_inline)) {
    [[maybe_unused]] uint4 al, ah, bl, bh;
    if constexpr (F8) { vlm_e4m3_widen16(wa, al, ah); vlm_e4m3_widen16(wb, bl, bh); }
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      if (m < M) {
        const bf16* xr = x + (size_t)m * ldx + k;
        const uint4 xl = *reinterpret_cast<const uint4*>(xr);
        if constexpr (F8) {
          const uint4 xh = *reinterpret_cast<const uint4*>(xr + 8);
          a0[m] = vlm_dot8(xh, ah, vlm_dot8(xl, al, a0[m]));
          a1[m] = vlm_dot8(xh, bh, vlm_dot8(xl, bl, a1[m]));
        } else {
          a0[m] = vlm_dot8(xl, wa, a0[m]);
          a1[m] = vlm_dot8(xl, wb, a1[m]);
        }
      }
    }
  };
  typedef unsigned v4u __attribute__((ext_vector_type(4)));      // weights are read once per step: streamed past the caches
  auto ldw16 = [](const WT* ptr) __attribute__((always_inline)) {
    const v4u a = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(ptr));
    return make_uint4(a[0], a[1], a[2], a[3]);
  };
  int k = (wave * 64 + lane) * E;
  for (; k + 3 * STEP < K; k += 4 * STEP) {      // four steps per trip, their eight weight loads issued before the first is used
    uint4 wa[4], wb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { wa[j] = ldw16(w0 + k + STEP * j); wb[j] = ldw16(w1 + k + STEP * j); }
#pragma unroll
    for (int j = 0; j < 4; ++j) fma_step(wa[j], wb[j], k + STEP * j);
  }
  for (; k + STEP < K; k += 2 * STEP) {
    const uint4 p0 = ldw16(w0 + k), q0 = ldw16(w1 + k), p1 = ldw16(w0 + k + STEP), q1 = ldw16(w1 + k + STEP);
    fma_step(p0, q0, k); fma_step(p1, q1, k + STEP);
  }
  for (; k < K; k += STEP) fma_step(ldw16(w0 + k), ldw16(w1 + k), k);
#pragma unroll
  for (int m = 0; m < MR; ++m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a0[m] += __shfl_xor(a0[m], o); a1[m] += __shfl_xor(a1[m], o); }
  }
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < MR; ++m) { red[wave][m][0] = a0[m]; red[wave][m][1] = a1[m]; }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 2 * MR) {
    const int m = t >> 1, c = t & 1;
    if (m < M && (c == 0 || two)) {
      float v = (red[0][m][c] + red[1][m][c]) + (red[2][m][c] + red[3][m][c]);
      if constexpr (F8) v *= wscale[n0 + c];
      stf(y + (size_t)m * ldy + n0 + c, v + (bias ? bias[n0 + c] : 0.f));
    }
  }
}
// the e4m3 GEMV takes a layer whose K is a multiple of 16 (a lane's 16-byte load); vlm_linear sends other shapes through the bf16 scratch
static bool vlm_e4m3_gemv_ok(const ConvW& w) { return w.CinPadH % 16 == 0; }
template <class TO>
static void vlm_gemv(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, TO* y, int ldy, VlmLinearInfo* info = nullptr) {
  if (info) *info = VlmLinearInfo{VLM_LIN_GEMV, M == 1 ? 1 : M == 2 ? 2 : 4, 0, 0};
  if (w.w8) FE_CHECK(w.w8_scale && vlm_e4m3_gemv_ok(w) && w.KpH % 16 == 0 && ldx % 8 == 0 && M >= 1 && M <= 4 && !w.scale, "vlm_gemv(e4m3): unsupported layer");
  else FE_CHECK(w.wh && w.hprec == PREC_BF16 && w.KpH % 8 == 0 && ldx % 8 == 0 && M >= 1 && M <= 4 && !w.scale, "vlm_gemv: unsupported layer");
  const int K = w.CinPadH, blocks = (w.Cout + 1) / 2;
#define VLM_GEMV(MR, WT, wp, ws) hipLaunchKernelGGL((vlm_gemv_kernel<MR, TO, WT>), dim3(blocks), dim3(256), 0, c.stream, x, ldx, (const WT*)(wp), w.KpH, (const float*)(ws), (const float*)w.shift, y, ldy, M, w.Cout, K)
  if (w.w8) { if (M == 1) VLM_GEMV(1, uint8_t, w.w8, w.w8_scale); else if (M == 2) VLM_GEMV(2, uint8_t, w.w8, w.w8_scale); else VLM_GEMV(4, uint8_t, w.w8, w.w8_scale); }
  else { if (M == 1) VLM_GEMV(1, bf16, w.wh, nullptr); else if (M == 2) VLM_GEMV(2, bf16, w.wh, nullptr); else VLM_GEMV(4, bf16, w.wh, nullptr); }
#undef VLM_GEMV
  FE_HIP(hipGetLastError());
  c.flops_accum += 2.0 * M * (double)w.Cin * w.Cout;
}
// ---- decode GEMM for 5 .. 32 sequences: the weight rows are the A operand of v_mfma_f32_32x32x16_bf16 (32 output columns per wave),
// the activation rows the B operand (batch rows padded to 32 with zeros); every weight byte is read once per step. A workgroup takes
// FOUR column tiles (one per wave) over one K range (grid.y = the K split), in stages of 128 K-elements.
//   * Weights reach the matrix fragments through a wave-private LDS image: the fragment layout wants 16 bytes of each of 32 rows per
//     load instruction - 64 sectors touched for 1 KiB, every 64-byte sector fetched four times from L2 by the four instructions that share
//     it (measured: 1.6 TB/s with nontemporal loads, 2.1 with cached ones). The loads instead take 4 rows x 256 contiguous bytes per
//     instruction (whole sectors, once), the registers go to LDS (16-byte slots XORed with the row number: conflict-free for the writes'
//     8-lane groups and the fragment reads' 16-lane groups) and come back as fragments. Loads run one stage ahead in registers.
//   * The activation slice of a stage (32 rows x 256 B) is staged once per workgroup, double-buffered, for all four waves - fetched per
//     wave from L2 it was half of the load traffic of a "weight-streaming" kernel.
// Inside a 64-element block of K lane (r, h) owns elements 32 h .. 32 h + 31 of its row (four fragments; the contraction order is free as
// long as both operands use it). Partial sums [split][M][N] in fp32, added in a fixed order by the finishing kernel (no atomics: the
// same token ids on every run).
constexpr int VLM_G32_XP = 272;      // bytes per staged activation row: 128 elements + 16 (conflict-free 16-byte reads at stride 1 row)
// (w2 / part2: a second weight matrix of the same shape on the same activations - the gate and up projections of the MLP as ONE launch:
// workgroup columns [cols1, 2 cols1) take it)
// WT = uint8_t: e4m3 rows (see "e4m3 weights" above; wscale / wscale2 their row scales). A stage of a tile is then 32 rows x 128 bytes:
// FOUR loads per lane, each 8 rows x 128 contiguous bytes per instruction (whole sectors, once), half the bytes of the bf16 stage. The
// codes are widened on the way into the SAME wave-private LDS image (16 codes = the two neighbouring 16-byte slots 2 p and 2 p + 1 of
// the row; under the XOR the second is the first's address ^ 16, and the 8-lane groups of two neighbouring rows cover the 16 slots of a
// 256-byte bank line between them), so the fragment reads and the bf16 MFMA below do not know the difference. Each accumulator row is
// multiplied by its scale before the partial sums are stored (exact, a power of two: the sum over the splits is the scaled sum), which
// leaves the finishing passes as they are. K % 128 == 0 as for bf16.
template <class WT>
__global__ __launch_bounds__(256) void vlm_gemm32_kernel(const bf16* __restrict__ x, int ldx, const WT* __restrict__ w, int ldw, float* __restrict__ part, int M, int N,
                                                         int K, int stages_per_wg, const WT* __restrict__ w2, float* __restrict__ part2, int cols1,
                                                         const float* __restrict__ wscale, const float* __restrict__ wscale2) {
  constexpr bool F8 = sizeof(WT) == 1;
  constexpr int NP = F8 ? 4 : 8;      // 16-byte weight pieces per lane and stage
  __shared__ __attribute__((aligned(16))) char ws[4][32 * 256];
  __shared__ __attribute__((aligned(16))) char xs[2][32 * VLM_G32_XP];
  const bf16* const tag = nullptr;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int ntiles = (N + 31) / 32;
  int bx = blockIdx.x;
  if (bx >= cols1) { bx -= cols1; w = w2; part = part2; wscale = wscale2; }
  const int nt = min(bx * 4 + wave, ntiles - 1);      // a workgroup's waves past the last tile repeat it (and do not store)
  const int n0 = nt * 32;
  const int nst = K / 128;
  const int s0 = blockIdx.y * stages_per_wg, s1 = min(s0 + stages_per_wg, nst);
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  // weight piece i of a stage: row 4 i + lane / 16 of the tile, 16 bytes at 16 (lane % 16) of the row's 256
  // (e4m3: row 8 i + lane / 8, 16 codes at 16 (lane % 8) of the row's 128, bound for the image's slots 2 (lane % 8) and 2 (lane % 8) + 1)
  const int wrow = F8 ? lane >> 3 : lane >> 4, wpc = F8 ? lane & 7 : lane & 15;
  const WT* wsrc[NP];
  int wdst[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int row = (F8 ? 8 : 4) * i + wrow, nr = min(n0 + row, N - 1);      // rows past N: a valid row, dropped at the store
    wsrc[i] = w + (size_t)nr * ldw + wpc * (F8 ? 16 : 8);
    wdst[i] = row * 256 + (((F8 ? 2 * wpc : wpc) ^ (row & 15)) << 4);
  }
  auto fetch_w = [&](const int st, v4u (&dst)[NP]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NP; ++i) dst[i] = *reinterpret_cast<const v4u*>(wsrc[i] + (size_t)st * 128);
  };
  // activation piece i (of 2) of a stage: row (t + 256 i) / 16, 16 bytes at 16 ((t + 256 i) % 16)
  auto stage_x = [&](const int st, char* dst) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = t + 256 * i, row = p >> 4, col = (p & 15) * 8;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row < M) v = *reinterpret_cast<const uint4*>(x + (size_t)row * ldx + (size_t)st * 128 + col);
      *reinterpret_cast<uint4*>(dst + row * VLM_G32_XP + col * 2) = v;
    }
  };
  fe_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  v4u wr[2][NP];
  char* const wl = ws[wave];
  if (s0 < s1) { fetch_w(s0, wr[0]); stage_x(s0, xs[0]); }
  __syncthreads();
  // (unrolled by two so the register sets and the activation buffers are compile-time choices)
  for (int st = s0; st < s1; st += 2) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int cur = st + u;
      if (cur < s1) {
        if (cur + 1 < s1) fetch_w(cur + 1, wr[u ^ 1]);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          if constexpr (F8) {
            uint4 lo, hi;
            vlm_e4m3_widen16(make_uint4(wr[u][i][0], wr[u][i][1], wr[u][i][2], wr[u][i][3]), lo, hi);
            *reinterpret_cast<uint4*>(wl + wdst[i]) = lo;
            *reinterpret_cast<uint4*>(wl + (wdst[i] ^ 16)) = hi;
          } else {
            *reinterpret_cast<v4u*>(wl + wdst[i]) = wr[u][i];
          }
        }
        if (cur + 1 < s1) stage_x(cur + 1, xs[u ^ 1]);      // the other buffer: its readers passed the barrier one stage ago
        const char* const xb = xs[u] + r * VLM_G32_XP + 64 * h;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int pc = kb * 8 + h * 4 + q;      // the 16-byte piece of the row this fragment is
            const fe_v4f a = *reinterpret_cast<const fe_v4f*>(wl + r * 256 + ((pc ^ (r & 15)) << 4));
            acc = fe_mfma16(tag, a, *reinterpret_cast<const fe_v4f*>(xb + kb * 128 + 16 * q), acc);
          }
      }
      __syncthreads();
    }
  }
  // acc: lane (r, h) holds column m = r (batch row) of the 32 x 32 tile, rows n = (e & 3) + 8 (e >> 2) + 4 h
  if (bx * 4 + wave < ntiles && r < M) {
    float* out = part + ((size_t)blockIdx.y * M + r) * N + n0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int nn = (e & 3) + 8 * (e >> 2) + 4 * h;
      if (n0 + nn < N) out[nn] = F8 ? acc[e] * wscale[n0 + nn] : acc[e];
    }
  }
}
template <class TO>
__global__ void vlm_gemm32_finish_kernel(const float* __restrict__ part, int splits, int M, int N, const float* __restrict__ bias, TO* __restrict__ y, int ldy) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
  float v = bias ? bias[n] : 0.f;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += part[((size_t)k * M + m) * N + n];
  stf(y + (size_t)m * ldy + n, s + v);
}
// launches the partial products of y = x W^T into `part` ([splits][M][N] fp32, taken from the arena: the CALLER rewinds); returns the split count
// `direct` (optional): where the result may be written straight when the layer needs no K split - a single split's partial sums ARE the
// product (the 152064-row lm_head: 1188 workgroup columns already fill the chip), so its finishing pass is skipped by the caller
static int vlm_gemm32_partials(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, float** part, const ConvW* w2 = nullptr, float** part2 = nullptr,
                               float* direct = nullptr) {
  const int K = w.CinPadH, N = w.Cout;
  const bool f8 = w.w8 != nullptr;
  FE_CHECK((f8 ? w.w8_scale && w.KpH % 16 == 0 : w.wh && w.hprec == PREC_BF16 && w.KpH % 8 == 0) && !w.scale && K % 128 == 0 && ldx % 8 == 0 && M >= 1 && M <= 32,
           "vlm_gemm32: unsupported layer");
  FE_CHECK(!w2 || ((f8 ? w2->w8 && w2->w8_scale : w2->wh && w2->hprec == PREC_BF16) && !w2->scale && w2->CinPadH == K && w2->Cout == N && w2->KpH == w.KpH && part2),
           "vlm_gemm32: the paired matrix differs in shape or format");
  const int ntiles = (N + 31) / 32, cols = (ntiles + 3) / 4, nst = K / 128, allcols = w2 ? 2 * cols : cols;
  // ~3 workgroups per CU stream from all of HBM; the partial sums of a split cost 4 M N bytes each way: no more splits than that needs,
  // and at least 4 stages per workgroup
  int splits = std::max(1, std::min(nst / 4, (768 + allcols - 1) / allcols));
  const int per = (nst + splits - 1) / splits;
  splits = (nst + per - 1) / per;
  *part = splits == 1 && direct ? direct : c.arena.array<float>((size_t)splits * M * N);
  if (w2) *part2 = c.arena.array<float>((size_t)splits * M * N);
  if (f8)
    hipLaunchKernelGGL(vlm_gemm32_kernel<uint8_t>, dim3(allcols, splits), dim3(256), 0, c.stream, x, ldx, (const uint8_t*)w.w8, w.KpH, *part, M, N, K, per,
                       w2 ? (const uint8_t*)w2->w8 : (const uint8_t*)nullptr, w2 ? *part2 : (float*)nullptr, cols, (const float*)w.w8_scale,
                       w2 ? (const float*)w2->w8_scale : (const float*)nullptr);
  else
    hipLaunchKernelGGL(vlm_gemm32_kernel<bf16>, dim3(allcols, splits), dim3(256), 0, c.stream, x, ldx, (const bf16*)w.wh, w.KpH, *part, M, N, K, per,
                       w2 ? (const bf16*)w2->wh : (const bf16*)nullptr, w2 ? *part2 : (float*)nullptr, cols, (const float*)nullptr, (const float*)nullptr);
  FE_HIP(hipGetLastError());
  const double fl = 2.0 * M * (double)w.Cin * N * (w2 ? 2 : 1);
  c.flops_accum += fl; c.flops_half += fl;
  return splits;
}
template <class TO>
static void vlm_gemm32(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, TO* y, int ldy, VlmLinearInfo* info = nullptr) {
  const size_t mark = c.arena.mark();
  float* part = nullptr;
  float* direct = nullptr;
  if constexpr (std::is_same<TO, float>::value) { if (!w.shift && ldy == w.Cout) direct = y; }
  const int splits = vlm_gemm32_partials(c, w, x, ldx, M, &part, nullptr, nullptr, direct), N = w.Cout;
  if (info) *info = VlmLinearInfo{VLM_LIN_GEMM32, 0, splits, direct && part == direct};
  if (!(direct && part == direct)) {
    hipLaunchKernelGGL((vlm_gemm32_finish_kernel<TO>), dim3((unsigned)(((size_t)M * N + 255) / 256)), dim3(256), 0, c.stream, (const float*)part, splits, M, N,
                       (const float*)w.shift, y, ldy);
    FE_HIP(hipGetLastError());
  }
  c.arena.rewind(mark);
}
static bool vlm_uses_gemm32(const ConvW& w, int M) {
  static const bool no32 = getenv("FE_VLM_NO_GEMM32") != nullptr;      // A/B hook
  return M > 3 && M <= 32 && w.CinPadH % 128 == 0 && !no32;      // measured: 4 sequences 0.94 ms / step here, 1.02 through the GEMV
}
// Finishing passes of the decode GEMM fused with what follows them (a 32-sequence step was ~30 launches per layer of which the 5-us ones -
// split sums, residual sums, norms, the gate product - were a quarter of the time). One workgroup per sequence row.
//   x = bf16(x + bf16(sum_k part + bias)); n = RMSNorm(x) * w   (w == nullptr: the sum only)
// DS (Qwen3-VL prefill, layers below n_deepstack): rows with slot[row] >= 0 (image tokens) also take x = bf16(x + ds[slot][:]) before the norm
template <bool DS>
__global__ __launch_bounds__(1024) void vlm_finish_add_rmsnorm_kernel(const float* __restrict__ part, int splits, int M, int d, const float* __restrict__ bias, bf16* __restrict__ x,
                                                                     const bf16* __restrict__ w, bf16* __restrict__ n, float eps, const int* __restrict__ slot,
                                                                     const bf16* __restrict__ ds) {
  __shared__ float red[16];
  const int row = blockIdx.x, t = threadIdx.x;      // 1024 threads: with 256 a row of 25 splits was 100 dependent-latency loads per thread
  bf16* const xr = x + (size_t)row * d;
  float ss = 0.f;
  for (int i = t * 4; i < d; i += 4096) {
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    // eight loads in flight, added in split order (the order of the stand-alone finishing pass: same bits)
    for (int k0 = 0; k0 < splits; k0 += 8) {
      float4 p4[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        p4[j] = k0 + j < splits ? *reinterpret_cast<const float4*>(part + ((size_t)(k0 + j) * M + row) * d + i) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k0 + j < splits) { sum.x += p4[j].x; sum.y += p4[j].y; sum.z += p4[j].z; sum.w += p4[j].w; }
    }
    if (bias) { const float4 b4 = *reinterpret_cast<const float4*>(bias + i); sum.x += b4.x; sum.y += b4.y; sum.z += b4.z; sum.w += b4.w; }
    const float4 a = ld4(xr + i);
    // the projection's output is a bf16 tensor, and so is the residual stream
    float4 v = make_float4((float)(bf16)(a.x + (float)(bf16)sum.x), (float)(bf16)(a.y + (float)(bf16)sum.y), (float)(bf16)(a.z + (float)(bf16)sum.z),
                           (float)(bf16)(a.w + (float)(bf16)sum.w));
    if constexpr (DS) {
      const int sl = slot[row];
      if (sl >= 0) {
        const float4 e = ld4(ds + (size_t)sl * d + i);
        v = make_float4((float)(bf16)(v.x + e.x), (float)(bf16)(v.y + e.y), (float)(bf16)(v.z + e.z), (float)(bf16)(v.w + e.w));
      }
    }
    st4(xr + i, v);
    ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  if (!w) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  if ((t & 63) == 0) red[t >> 6] = ss;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) tot += red[k];
  const float rs = rsqrtf(tot / (float)d + eps);
  bf16* const nr = n + (size_t)row * d;
  for (int i = t * 4; i < d; i += 4096) {
    const float4 v = ld4(xr + i), g = ld4(w + i);      // (this thread's own stores of the first loop)
    st4(nr + i, make_float4(g.x * (float)(bf16)(v.x * rs), g.y * (float)(bf16)(v.y * rs), g.z * (float)(bf16)(v.z * rs), g.w * (float)(bf16)(v.w * rs)));
  }
}
//   h = bf16(silu(bf16(sum_k pg))) * bf16(sum_k pu)   (the two projections of the SwiGLU MLP, same split count)
__global__ void vlm_finish_silu_mul_kernel(const float* __restrict__ pg, const float* __restrict__ pu, int splits, size_t mn4, bf16* __restrict__ hout) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < mn4; i += (size_t)gridDim.x * blockDim.x) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), u = g;
    for (int k = 0; k < splits; ++k) {
      const float4 a = *reinterpret_cast<const float4*>(pg + (k * mn4 + i) * 4), b = *reinterpret_cast<const float4*>(pu + (k * mn4 + i) * 4);
      g.x += a.x; g.y += a.y; g.z += a.z; g.w += a.w;
      u.x += b.x; u.y += b.y; u.z += b.z; u.w += b.w;
    }
    auto f = [](float x, float y) { x = (float)(bf16)x; y = (float)(bf16)y; return (float)(bf16)(x / (1.f + expf(-x))) * y; };
    st4(hout + 4 * i, make_float4(f(g.x, u.x), f(g.y, u.y), f(g.z, u.z), f(g.w, u.w)));
  }
}
// e4m3 rows -> a bf16 matrix [Cout][KpH] in the layout of ConvW.wh: decode(code) * 2^e, exactly a bf16 value (fp8_core.h), so the shared
// layer wrappers then compute what they compute for a bf16 model loaded with the dequantised weights. One thread per 16 codes.
__global__ void vlm_e4m3_dequant_kernel(const uint8_t* __restrict__ w8, const float* __restrict__ wscale, bf16* __restrict__ out, size_t n16, int kp16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
    const float sc = wscale[i / kp16];
    uint4 lo, hi;
    vlm_e4m3_widen16(*reinterpret_cast<const uint4*>(w8 + i * 16), lo, hi);
    // the scaled value has at most 4 significant bits and a normal exponent: the upper 16 bits of the fp32 product ARE its bf16 form
    auto sc2 = [sc](const unsigned u) { return (__float_as_uint(__uint_as_float(u << 16) * sc) >> 16) | (__float_as_uint(__uint_as_float(u & 0xFFFF0000u) * sc) & 0xFFFF0000u); };
    uint4* o = reinterpret_cast<uint4*>(out + i * 16);
    o[0] = make_uint4(sc2(lo.x), sc2(lo.y), sc2(lo.z), sc2(lo.w));
    o[1] = make_uint4(sc2(hi.x), sc2(hi.y), sc2(hi.z), sc2(hi.w));
  }
}
// the bf16 view of an e4m3 layer, in arena scratch (the CALLER rewinds): for more than 32 rows (prefill; decode beyond 32 sequences, which
// this extra pass makes slower than a bf16 model's) and for the shapes the e4m3 kernels do not take
static ConvW vlm_e4m3_widen(Ctx& c, const ConvW& w) {
  FE_CHECK(w.w8 && w.w8_scale && w.KpH % 16 == 0, "vlm: layer has no e4m3 rows");
  ConvW t = w;
  const size_t n = (size_t)w.Cout * w.KpH;
  bf16* wide = c.arena.array<bf16>(n);
  hipLaunchKernelGGL(vlm_e4m3_dequant_kernel, dim3(grid_n(n / 16)), dim3(256), 0, c.stream, (const uint8_t*)w.w8, (const float*)w.w8_scale, wide, n / 16, w.KpH / 16);
  FE_HIP(hipGetLastError());
  t.wh = wide; t.hprec = PREC_BF16; t.w8 = nullptr; t.w8_scale = nullptr;
  return t;
}
// y = x W^T (+ b) in bf16 for any row count: the streaming GEMV for up to 4 rows, the weight-streaming matrix-core GEMM up to 32, the
// shared layer wrapper above that (an e4m3 layer: the same choice among its own kernels, the wrapper on its bf16 scratch)
// (force, the test hook's: that kernel under its own checks; info: what ran)
void vlm_linear(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, bf16* y, int ldy, int force, VlmLinearInfo* info) {
  if (force == VLM_LIN_FORCE_GEMV) { vlm_gemv(c, w, x, ldx, M, y, ldy, info); return; }
  if (force == VLM_LIN_FORCE_GEMM32) { vlm_gemm32(c, w, x, ldx, M, y, ldy, info); return; }
  if (w.w8) {
    if (M <= 4 && !vlm_uses_gemm32(w, M) && vlm_e4m3_gemv_ok(w)) vlm_gemv(c, w, x, ldx, M, y, ldy, info);
    else if (vlm_uses_gemm32(w, M)) vlm_gemm32(c, w, x, ldx, M, y, ldy, info);
    else {
      const size_t mark = c.arena.mark();
      linear_forward(c, vlm_e4m3_widen(c, w), x, ldx, M, y, ldy, ACT_NONE);
      c.arena.rewind(mark);
      if (info) *info = VlmLinearInfo{VLM_LIN_WRAPPER, 0, 0, 0};
    }
    return;
  }
  if (M <= 4 && !vlm_uses_gemm32(w, M)) vlm_gemv(c, w, x, ldx, M, y, ldy, info);
  else if (vlm_uses_gemm32(w, M)) vlm_gemm32(c, w, x, ldx, M, y, ldy, info);
  else {
    linear_forward(c, w, x, ldx, M, y, ldy, ACT_NONE);
    if (info) *info = VlmLinearInfo{VLM_LIN_WRAPPER, 0, 0, 0};
  }
}
// the fp32 logits of the lm_head (hidden = w.Cin): the same three families, the wrapper's e4m3 scratch left in the arena (the CALLER rewinds)
void vlm_logits(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, float* lg, int ldy, int force, VlmLinearInfo* info) {
  if (force == VLM_LIN_FORCE_GEMV) { vlm_gemv(c, w, x, ldx, M, lg, ldy, info); return; }
  if (force == VLM_LIN_FORCE_GEMM32) { vlm_gemm32(c, w, x, ldx, M, lg, ldy, info); return; }
  if (M <= 4 && !vlm_uses_gemm32(w, M) && (!w.w8 || vlm_e4m3_gemv_ok(w))) { vlm_gemv(c, w, x, ldx, M, lg, ldy, info); return; }
  if (M <= 32 && w.Cin % 128 == 0) { vlm_gemm32(c, w, x, ldx, M, lg, ldy, info); return; }
  if (w.w8) linear_forward_f32(c, vlm_e4m3_widen(c, w), x, ldx, M, lg, ldy, ACT_NONE);
  else linear_forward_f32(c, w, x, ldx, M, lg, ldy, ACT_NONE);
  if (info) *info = VlmLinearInfo{VLM_LIN_WRAPPER, 0, 0, 0};
}
// The fused steps of a 4 .. 32-row layer (engine.h): the split sums of the weight-streaming GEMM are taken by the pass that follows the
// projection instead of a finishing launch of their own.
int vlm_proj_add_rmsnorm(Ctx& c, const ConvW& w, const bf16* a, int lda, int rows, bf16* x, const bf16* ln, bf16* n, float eps, const int* slot,
                         const bf16* ds) {
  FE_CHECK(w.Cout % 4 == 0 && !w.shift && (!ds || slot), "vlm_proj_add_rmsnorm: unsupported layer");
  float* part = nullptr;
  const int sp = vlm_gemm32_partials(c, w, a, lda, rows, &part);
  const int d = w.Cout;
  if (ds) hipLaunchKernelGGL(vlm_finish_add_rmsnorm_kernel<true>, dim3(rows), dim3(1024), 0, c.stream, (const float*)part, sp, rows, d, (const float*)nullptr, x, ln, n, eps, slot, ds);
  else hipLaunchKernelGGL(vlm_finish_add_rmsnorm_kernel<false>, dim3(rows), dim3(1024), 0, c.stream, (const float*)part, sp, rows, d, (const float*)nullptr, x, ln, n, eps,
                          (const int*)nullptr, (const bf16*)nullptr);
  FE_HIP(hipGetLastError());
  return sp;
}
int vlm_gate_up_silu_mul(Ctx& c, const ConvW& gate, const ConvW& up, const bf16* n, int ldn, int rows, bf16* h) {
  FE_CHECK(gate.Cout % 4 == 0 && !gate.shift && !up.shift, "vlm_gate_up_silu_mul: unsupported layer");
  float *pg = nullptr, *pu = nullptr;
  const int sg = vlm_gemm32_partials(c, gate, n, ldn, rows, &pg, &up, &pu);      // gate and up: one launch
  const size_t mn4 = (size_t)rows * gate.Cout / 4;
  hipLaunchKernelGGL(vlm_finish_silu_mul_kernel, dim3(grid_n(mn4)), dim3(256), 0, c.stream, (const float*)pg, (const float*)pu, sg, mn4, h);
  FE_HIP(hipGetLastError());
  return sg;
}

// device-resident decode state (graph replay): after a step, the chosen tokens become the next step's input, every position and the
// cache length advance by one, and the tokens are appended to the output table [step][B] (LP: their log-probs lp [B] to out_lp [step][B])
// UNTIL (fe_vlm_generate_until): fin [B] holds -1 while a sequence runs, else the EOS id it emitted. A finished sequence takes that id
// again instead of the step's choice (what generate's padding feeds it) and NaN as its log-prob; a running one that picks one of the
// eos ids is marked; *live = the sequences still running after this step (the host reads it between launches).
struct VlmEosIds { int n; int id[8]; };
template <bool LP, bool UNTIL>
__global__ void vlm_advance_kernel(const int* __restrict__ next, int* __restrict__ tok, int* __restrict__ pos, int* __restrict__ len, int* __restrict__ step,
                                   int* __restrict__ out, int B, const float* __restrict__ lp, float* __restrict__ out_lp, const VlmEosIds eos,
                                   int* __restrict__ fin, int* __restrict__ live) {
  const int b = threadIdx.x;
  const int st = *step;
  bool running = false;
  if (b < B) {
    int t = next[b];
    float l = LP ? lp[b] : 0.f;
    if (UNTIL) {
      const int f = fin[b];
      if (f >= 0) { t = f; l = __builtin_nanf(""); }
      else {
        bool hit = false;
        for (int e = 0; e < eos.n; ++e) hit = hit || t == eos.id[e];
        if (hit) fin[b] = t;
        running = !hit;
      }
    }
    tok[b] = t;
    out[(size_t)st * B + b] = t;
    if (LP) out_lp[(size_t)st * B + b] = l;
    pos[b] += 1; pos[B + b] += 1; pos[2 * B + b] += 1;
  }
  const int n_live = UNTIL ? __syncthreads_count(running) : 0;
  if (!UNTIL) __syncthreads();
  if (b == 0) { *len += 1; *step = st + 1; if (UNTIL) *live = n_live; }
}

// x = bf16(x + y) and, in the same pass, n = RMSNorm(x) * w (w == nullptr: the sum only). One wave per row: a decode step is a chain of
// ~12 launches per layer whose small ones cost their launch latency, so the residual sum rides with the norm that follows it.
// (DS: the DeepStack sum of vlm_finish_add_rmsnorm_kernel)
template <bool DS>
__global__ void vlm_add_rmsnorm_kernel(bf16* __restrict__ x, const bf16* __restrict__ y, const bf16* __restrict__ w, bf16* __restrict__ n, int rows, int d, float eps,
                                       const int* __restrict__ slot, const bf16* __restrict__ ds) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int row = wave; row < rows; row += nwaves) {
    bf16* xr = x + (size_t)row * d;
    const bf16* yr = y + (size_t)row * d;
    float ss = 0.f;
    const int sl = DS ? slot[row] : -1;
    for (int i = lane * 4; i < d; i += 256) {
      const float4 a = ld4(xr + i), b = ld4(yr + i);
      // the sum is rounded to bf16 first (the residual stream is a bf16 tensor), and the norm reads the rounded value
      float4 v = make_float4((float)(bf16)(a.x + b.x), (float)(bf16)(a.y + b.y), (float)(bf16)(a.z + b.z), (float)(bf16)(a.w + b.w));
      if (DS && sl >= 0) {
        const float4 e = ld4(ds + (size_t)sl * d + i);
        v = make_float4((float)(bf16)(v.x + e.x), (float)(bf16)(v.y + e.y), (float)(bf16)(v.z + e.z), (float)(bf16)(v.w + e.w));
      }
      st4(xr + i, v);
      ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    if (!w) continue;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float rs = rsqrtf(ss / (float)d + eps);
    bf16* nr = n + (size_t)row * d;
    for (int i = lane * 4; i < d; i += 256) {
      const float4 v = ld4(xr + i), g = ld4(w + i);      // (this lane's own stores of the first loop)
      st4(nr + i, make_float4(g.x * (float)(bf16)(v.x * rs), g.y * (float)(bf16)(v.y * rs), g.z * (float)(bf16)(v.z * rs), g.w * (float)(bf16)(v.w * rs)));
    }
  }
}

// argmax over a vocabulary row in two launches (one 256-thread block walked 152064 logits in 180 us): 64 chunks per row, then one wave
// per row over the 64 partial results. Logits are rounded to bf16 in place first; ties go to the lowest index (torch.argmax).
// LP: the same pass also takes the log-probability of the chosen token, -log sum_i exp(l_i - max_j l_j) over the bf16-rounded logits (the
// chosen logit is the maximum). Every thread keeps sum exp(l - best) beside its running best (rescaled when the best moves); the block and
// then the final wave merge (max, sum) pairs with s = s1 e^(m1 - m) + s2 e^(m2 - m). exp2 with a log2(e) scale (v_exp_f32); a part whose
// maximum is -inf contributes 0.
constexpr int VLM_AM_CHUNKS = 64;
constexpr float VLM_LOG2E = 1.4426950408889634f;
// s e^(mi - m) for mi <= m, 0 for an empty part (mi = -inf: no NaN from -inf - -inf)
__device__ __forceinline__ float vlm_lse_rescale(float s, float mi, float m) { return mi == -INFINITY ? 0.f : s * exp2f((mi - m) * VLM_LOG2E); }
template <bool LP>
__global__ void vlm_argmax_part_kernel(float* __restrict__ lg, int vocab, float* __restrict__ pv, int* __restrict__ pi, float* __restrict__ ps) {
  float* row = lg + (size_t)blockIdx.y * vocab;
  const int per = (vocab + VLM_AM_CHUNKS - 1) / VLM_AM_CHUNKS, i0 = blockIdx.x * per, i1 = min(i0 + per, vocab);
  float best = -INFINITY; int bi = 0x7fffffff;
  float s = 0.f;      // (LP) sum exp(l - best) over this thread's logits
  for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    const float v = (float)(bf16)row[i];
    row[i] = v;
    if (LP) {
      if (v > best) s = vlm_lse_rescale(s, best, v) + 1.f;
      else if (v != -INFINITY) s += exp2f((v - best) * VLM_LOG2E);
    }
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
  __shared__ float sv[256]; __shared__ int si[256];
  sv[threadIdx.x] = best; si[threadIdx.x] = bi;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const float v = sv[threadIdx.x + o]; const int j = si[threadIdx.x + o];
      if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && j < si[threadIdx.x])) { sv[threadIdx.x] = v; si[threadIdx.x] = j; }
    }
    __syncthreads();
  }
  if (LP) {      // sv[0] is the chunk's maximum: every thread's sum rescaled to it, summed over the block (waves, then 4 partials)
    __shared__ float sw[4];
    float t = vlm_lse_rescale(s, best, sv[0]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) ps[blockIdx.y * VLM_AM_CHUNKS + blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
  }
  if (threadIdx.x == 0) { pv[blockIdx.y * VLM_AM_CHUNKS + blockIdx.x] = sv[0]; pi[blockIdx.y * VLM_AM_CHUNKS + blockIdx.x] = si[0]; }
}
template <bool LP>
__global__ void vlm_argmax_final_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int* __restrict__ next, const float* __restrict__ ps,
                                        float* __restrict__ lp) {
  const int b = blockIdx.x, t = threadIdx.x;      // 64 threads = one wave
  const float v0 = pv[b * VLM_AM_CHUNKS + t];
  float v = v0; int j = pi[b * VLM_AM_CHUNKS + t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o); const int j2 = __shfl_xor(j, o);
    if (v2 > v || (v2 == v && j2 < j)) { v = v2; j = j2; }
  }
  if (LP) {      // v: the row maximum, in every lane after the butterfly
    float s = vlm_lse_rescale(ps[b * VLM_AM_CHUNKS + t], v0, v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (t == 0) lp[b] = -logf(s);
  }
  if (t == 0) next[b] = j;
}

// Decode attention, grouped-query aware: workgroup (sequence b, KV head kvh, chunk sp) takes keys [128 sp, 128 sp + 128) for ALL nh / nkv
// query heads that share the KV head - the first split form ran one workgroup per QUERY head, so every key / value row crossed L2 -> L1
// seven times at the 7B geometry, and it read K one row per lane (64 rows x 16 bytes per instruction: each 64-byte sector fetched four
// times): 54 us per layer at 32 sequences x 528 keys, a fifth of the step. Here 16 lanes share a key (1 KiB contiguous per instruction),
// the G dot products of a key come from one load, and a value row is multiplied into G outputs from one load. Writes the unnormalised
// outputs, running maxima and sums per (head, chunk); vlm_attn_combine_kernel merges the chunks. Lk by value or, for graph replay, from
// device memory (then the grid covers the whole cache and chunks past Lk write the neutral element).
// sum over the 16 lanes of a DPP row, result in every lane: four VALU adds with lane-permute modifiers (quad xor 1, quad xor 2, mirror of 8,
// mirror of 16) - __shfl_xor goes through the LDS crossbar (ds_bpermute), ~20x the latency, and the score phase needs 28 sums per step
__device__ __forceinline__ float vlm_row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));       // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));       // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));      // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));      // row_mirror
  return v;
}
// One kernel body for both cache storages. CT = bf16: a key row is 256 bytes, 16 lanes per key with 8 values each (16-byte loads, 1 KiB
// contiguous per wave instruction). CT = uint8_t, an FE_VLM_KV_E4M3 cache: a key row is 128 contiguous codes, 16 lanes per key with 8
// codes each (8-byte loads, 512 contiguous bytes per wave instruction), widened by v_cvt_scalef32_pk_f32_fp8 (gfx950: the OCP reading,
// scale 1) - half the K / V bytes. The K scale multiplies the score, (sum * kscale) * scale, and the V scale the bf16-rounded probability,
// both exactly (powers of two): the bf16 arithmetic on the dequantised rows, with the products and sums in its order (ksc / vsc: the scale
// arrays, unused for bf16). q stays bf16, accumulation fp32, the running sum pl comes from the unrounded exponentials.
// Both forms are bound by the vector ALU, not by the K / V bytes (G = 7, 32 sequences x 1716 keys: bf16 40 us, 2.8 TB/s). The file is
// compiled without contraction, and the bf16 form keeps its separate multiply and add per term (its test bounds and the recorded token ids
// rest on that rounding); the e4m3 form, written after them, takes explicit fused multiply-adds in the dot products and the P V sums: 1892
// against 2777 vector instructions at G = 7, 34 us (profiles/vlm_fp8_kv_perf.txt).
constexpr int VLM_DEC_CHUNK = 128;
__device__ __forceinline__ void vlm_e4m3_unpack8(const uint2 c, float v[8]) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c.x, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c.x, 1.0f, true);
  const f2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c.y, 1.0f, false), e = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c.y, 1.0f, true);
  v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1]; v[4] = d[0]; v[5] = d[1]; v[6] = e[0]; v[7] = e[1];
}
// a lane's 8 values of a cache row: 8 bf16 or 8 e4m3 codes
__device__ __forceinline__ void vlm_kv_unpack8(const uint4 u, float v[8]) { h_unpack8_bf16(u, v); }
__device__ __forceinline__ void vlm_kv_unpack8(const uint2 c, float v[8]) { vlm_e4m3_unpack8(c, v); }
// a + x * y: fused for the e4m3 cache, a rounded product and a rounded sum for bf16
template <bool FUSED>
__device__ __forceinline__ float vlm_kv_madd(const float x, const float y, const float a) {
  if constexpr (FUSED) return __builtin_fmaf(x, y, a);
  else return a + x * y;
}
template <int G, class CT>
__global__ __launch_bounds__(256, 3) void vlm_attn_decode_gqa_kernel(const bf16* __restrict__ q, const CT* __restrict__ kc, const CT* __restrict__ vc,
                                                                  const float* __restrict__ ksc, const float* __restrict__ vsc, float* __restrict__ po,
                                                                  float* __restrict__ pm, float* __restrict__ pl, int nh, int nkv, int Lk, int max_seq, float scale,
                                                                  const int* __restrict__ len_dev, int nsplit, const int* __restrict__ pad) {
  constexpr bool F8 = sizeof(CT) == 1;
  using Slice = std::conditional_t<F8, uint2, uint4>;      // a lane's 8 values of a row
  __shared__ float sc[G][VLM_DEC_CHUNK];      // scores, then probabilities (e4m3: times the V scales)
  __shared__ float part[4][G][128];
  if (len_dev) Lk = *len_dev + 1;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int bk = blockIdx.x, sp = blockIdx.y;
  const int b = bk / nkv, kvh = bk - b * nkv, head0 = kvh * G;
  const int k0 = sp * VLM_DEC_CHUNK, k1 = min(k0 + VLM_DEC_CHUNK, Lk);
  const int padb = pad[b];      // keys below it are left padding
  if (k0 >= Lk || k1 <= padb) {      // a chunk past the cache length or wholly in the pad: neutral element of the merge
    if (t < G) { pm[((size_t)b * nh + head0 + t) * nsplit + sp] = -INFINITY; pl[((size_t)b * nh + head0 + t) * nsplit + sp] = 0.f; }
    return;
  }
  const size_t row0 = ((size_t)b * nkv + kvh) * max_seq;
  const CT* const K = kc + row0 * 128;
  const CT* const V = vc + row0 * 128;
  [[maybe_unused]] const float* const KS = F8 ? ksc + row0 : nullptr;      // the rows' scales (e4m3 only)
  [[maybe_unused]] const float* const VS = F8 ? vsc + row0 : nullptr;
  // ---- scores: 16 lanes per key (8 dims each), 4 keys per wave instruction, 32 keys per wave ---------------------------------------------
  {
    const int sub = lane & 15, kk = lane >> 4;
    float qf[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) h_unpack8_bf16(*reinterpret_cast<const uint4*>(q + ((size_t)b * nh + head0 + g) * 128 + 8 * sub), qf[g]);
    Slice kr[8];
    [[maybe_unused]] float ks[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int key = min(k0 + wave * 32 + it * 4 + kk, k1 - 1);
      kr[it] = *reinterpret_cast<const Slice*>(K + (size_t)key * 128 + 8 * sub);
      if constexpr (F8) ks[it] = KS[key];
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int kl = wave * 32 + it * 4 + kk;
      float kf[8];
      vlm_kv_unpack8(kr[it], kf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a = vlm_kv_madd<F8>(kf[e], qf[g][e], a);
        a = vlm_row16_sum(a);
        if (sub == 0) {
          if constexpr (F8) a *= ks[it];
          sc[g][kl] = (k0 + kl < k1 && k0 + kl >= padb) ? a * scale : -INFINITY;
        }
      }
    }
  }
  __syncthreads();
  // ---- softmax pieces per head: wave w takes heads w, w + 4; 2 keys per lane ---------------------------------------------------------------
  for (int g = wave; g < G; g += 4) {
    const float s0 = sc[g][lane], s1 = sc[g][64 + lane];
    float mx = fmaxf(s0, s1);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    // probabilities as bf16 (the P operand of the reference's P V product); e4m3: then times the key's V scale, p * (2^e * code) = (p * 2^e) * code
    float e0 = (float)(bf16)__expf(s0 - mx), e1 = (float)(bf16)__expf(s1 - mx);
    if constexpr (F8) { e0 *= VS[min(k0 + lane, k1 - 1)]; e1 *= VS[min(k0 + 64 + lane, k1 - 1)]; }
    float sum = __expf(s0 - mx) + __expf(s1 - mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    sc[g][lane] = e0; sc[g][64 + lane] = e1;
    if (lane == 0) { pm[((size_t)b * nh + head0 + g) * nsplit + sp] = mx; pl[((size_t)b * nh + head0 + g) * nsplit + sp] = sum; }
  }
  __syncthreads();
  // ---- O partials: the same 16-lanes-per-row pattern on V (eight loads per wave in flight): lane (sub, kk) accumulates dims
  // 8 sub .. 8 sub + 7 over keys 32 wave + 4 it + kk for every head; the four kk groups are then added with two shuffles -----------------------
  {
    const int sub = lane & 15, kk = lane >> 4;
    Slice vr[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int key = k0 + wave * 32 + it * 4 + kk;
      vr[it] = *reinterpret_cast<const Slice*>(V + (size_t)min(key, k1 - 1) * 128 + 8 * sub);
    }
    float a[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) a[g][e] = 0.f;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int kl = wave * 32 + it * 4 + kk;      // probabilities of keys past the chunk's end are zero
      float vf[8];
      vlm_kv_unpack8(vr[it], vf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pj = sc[g][kl];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[g][e] = vlm_kv_madd<F8>(pj, vf[e], a[g][e]);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = a[g][e];
        v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
        if (kk == 0) part[wave][g][8 * sub + e] = v;
      }
  }
  __syncthreads();
  for (int i = t; i < G * 128; i += 256) {
    const int g = i >> 7, dm = i & 127;
    po[(((size_t)b * nh + head0 + g) * nsplit + sp) * 128 + dm] = (part[0][g][dm] + part[1][g][dm]) + (part[2][g][dm] + part[3][g][dm]);
  }
}
__global__ void vlm_attn_combine_kernel(const float* __restrict__ po, const float* __restrict__ pm, const float* __restrict__ pl, bf16* __restrict__ o, int nsplit) {
  const int bh = blockIdx.x, t = threadIdx.x;      // 128 threads: one per output dimension
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, pm[(size_t)bh * nsplit + s]);
  float l = 0.f, acc = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float mm = pm[(size_t)bh * nsplit + s];
    if (mm == -INFINITY) continue;
    const float f = __expf(mm - M);
    l += f * pl[(size_t)bh * nsplit + s];
    acc += f * po[((size_t)bh * nsplit + s) * 128 + t];
  }
  o[(size_t)bh * 128 + t] = (bf16)(acc / l);
}

// ---- model ---------------------------------------------------------------------------------------------------------------------------
bf16* upload_bf16(DeviceWeights& dw, const std::vector<float>& v) {
  std::vector<uint16_t> h(v.size());
  for (size_t i = 0; i < v.size(); ++i) h[i] = f32_to_bf16_bits(v[i]);
  return (bf16*)dw.upload_raw(h.data(), h.size() * sizeof(uint16_t));
}

// FE_VLM_WEIGHTS_E4M3: a Linear weight [N][K] (+ bias) as the e4m3 form of ConvW - every row rounded to bf16 as the bf16 commit does, then
// quantised by fp8_core.h; no bf16 copy goes to the device. `name` is the tensor in the error of a NaN / Inf weight.
static ConvW pack_linear_e4m3(DeviceWeights& dw, const HostTensor& W, const std::vector<float>* bias, const std::string& name) {
  FE_CHECK(W.shape.size() == 2, "vlm: %s is not a matrix", name.c_str());
  ConvW c;
  c.Cout = (int)W.shape[0]; c.Cin = (int)W.shape[1];
  c.CinPad = (c.Cin + 3) & ~3; c.K = c.CinPad; c.Kp = (c.K + CONV_KALIGN - 1) / CONV_KALIGN * CONV_KALIGN;
  c.CinPadH = (c.Cin + 7) & ~7; c.cb = 32;
  c.KpH = (c.CinPadH + CONV_KALIGN_H - 1) / CONV_KALIGN_H * CONV_KALIGN_H;
  FE_CHECK(!bias || (int)bias->size() == c.Cout, "vlm: %s bias size", name.c_str());
  std::vector<uint8_t> codes((size_t)c.Cout * c.KpH, 0);
  std::vector<float> scales((size_t)c.Cout), row((size_t)c.Cin);
  for (int n = 0; n < c.Cout; ++n) {
    for (int k = 0; k < c.Cin; ++k) {
      const uint32_t u = (uint32_t)f32_to_bf16_bits(W.data[(size_t)n * c.Cin + k]) << 16;
      memcpy(&row[k], &u, 4);
    }
    int e = 0;
    FE_CHECK(fp8::quantize_row(row.data(), (size_t)c.Cin, codes.data() + (size_t)n * c.KpH, &e), "vlm: %s holds a NaN or Inf (row %d): not quantised to e4m3", name.c_str(), n);
    scales[n] = fp8::row_scale(e);
  }
  c.w8 = (uint8_t*)dw.upload_raw(codes.data(), codes.size());
  c.w8_scale = dw.upload(scales);
  if (bias) c.shift = dw.upload(*bias);
  return c;
}
// a Linear of the decoder in the model's weight format (e4m3: `name` for the error message; bf16: build_linear_rows on all rows)
ConvW vlm_pack_linear(DeviceWeights& dw, int weight_format, const HostTensor& W, const HostTensor* bias, const std::string& name) {
  if (weight_format == FE_VLM_WEIGHTS_E4M3) return pack_linear_e4m3(dw, W, bias ? &bias->data : nullptr, name);
  return build_linear_rows(dw, W, bias, 0, (int)W.shape[0]);
}

void build_vlm(VlmModel& m, const WeightStore& ws, const VlmConfig& cfg, int weight_format) {
  FE_CHECK(weight_format == FE_VLM_WEIGHTS_BF16 || weight_format == FE_VLM_WEIGHTS_E4M3, "vlm: weight format %d", weight_format);
  m.weight_format = weight_format;
  const bool f8 = weight_format == FE_VLM_WEIGHTS_E4M3;
  // (e4m3: the parts of a fused q|k|v are checked under their own names before they are concatenated)
  auto finite = [&](const HostTensor& t, const std::string& name) {
    if (!f8) return;
    for (const float v : t.data) FE_CHECK(std::isfinite(v), "vlm: %s.weight holds a NaN or Inf: not quantised to e4m3", name.c_str());
  };
  auto linear = [&](const std::string& prefix) { return f8 ? vlm_pack_linear(m.dw, m.weight_format, ws.get(prefix + ".weight"), nullptr, prefix + ".weight") : build_linear(m.dw, ws, prefix, false); };
  m.cfg = cfg;
  m.dw.prec = PREC_BF16;
  m.dw.half_only = true;      // 7.6 G parameters: no fp32 / Winograd copies beside the bf16 ones
  const std::string P = "model.language_model.";
  const HostTensor& E = ws.get(P + "embed_tokens.weight");
  m.vocab = (int)E.shape[0]; m.hidden = (int)E.shape[1];
  FE_CHECK(cfg.head_dim == 128, "vlm: head_dim %d (the attention kernels are built for 128)", cfg.head_dim);
  FE_CHECK(cfg.n_heads > 0 && cfg.n_kv_heads > 0 && cfg.n_heads % cfg.n_kv_heads == 0, "vlm: %d heads / %d kv heads", cfg.n_heads, cfg.n_kv_heads);
  FE_CHECK(cfg.mrope[0] + cfg.mrope[1] + cfg.mrope[2] == 64, "vlm: mrope sections must sum to head_dim / 2");
  FE_CHECK(m.hidden % 64 == 0, "vlm: hidden size %d must be a multiple of 64", m.hidden);
  // Qwen3-VL checkpoints may tie lm_head to embed_tokens (no lm_head.weight): the packed lm_head rows then serve as the embedding table too
  // Qwen2-VL-2B ties it too; safetensors drops the shared tensor, a torch state dict keeps it under both names (equal values: one copy)
  bool tied = (cfg.qwen3 || cfg.qwen2) && !ws.has("lm_head.weight");
  if (!tied && cfg.qwen2) {
    const HostTensor& H = ws.get("lm_head.weight");
    tied = H.data.size() == E.data.size() && memcmp(H.data.data(), E.data.data(), E.data.size() * sizeof(float)) == 0;
  }
  if (!tied) m.embed = upload_bf16(m.dw, E.data);
  m.layers.clear();
  const int qd = cfg.n_heads * 128, kd = cfg.n_kv_heads * 128;
  for (int i = 0;; ++i) {
    const std::string L = P + "layers." + std::to_string(i);
    if (!ws.has(L + ".self_attn.q_proj.weight")) break;
    VlmLayerW w;
    if (cfg.qwen3) {      // Qwen3-VL: q | k | v without bias, then q_norm / k_norm over each head's 128 dims
      HostTensor W;
      W.shape = {qd + 2 * kd, m.hidden};
      for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
        FE_CHECK(!ws.has(L + ".self_attn." + n + ".bias"), "vlm (qwen3): layer %d %s carries a bias", i, n);
        const HostTensor& a = ws.get(L + ".self_attn." + n + ".weight");
        FE_CHECK((int)a.shape[1] == m.hidden, "vlm: %s input width", n);
        finite(a, L + ".self_attn." + n);
        W.data.insert(W.data.end(), a.data.begin(), a.data.end());
      }
      FE_CHECK((int64_t)W.data.size() == W.shape[0] * W.shape[1], "vlm: layer %d q/k/v shapes do not match %d heads / %d kv heads of 128", i, cfg.n_heads, cfg.n_kv_heads);
      w.qkv = vlm_pack_linear(m.dw, m.weight_format, W, nullptr, L + ".self_attn.q|k|v_proj.weight");
      const HostTensor& qn = ws.get(L + ".self_attn.q_norm.weight");
      const HostTensor& kn = ws.get(L + ".self_attn.k_norm.weight");
      FE_CHECK(qn.numel() == 128 && kn.numel() == 128, "vlm (qwen3): layer %d q_norm / k_norm must have 128 weights", i);
      w.qn = upload_bf16(m.dw, qn.data);
      w.kn = upload_bf16(m.dw, kn.data);
      w.o = linear(L + ".self_attn.o_proj");
      w.gate = linear(L + ".mlp.gate_proj");
      w.up = linear(L + ".mlp.up_proj");
      w.down = linear(L + ".mlp.down_proj");
      w.ln1 = upload_bf16(m.dw, ws.get(L + ".input_layernorm.weight").data);
      w.ln2 = upload_bf16(m.dw, ws.get(L + ".post_attention_layernorm.weight").data);
      m.layers.push_back(w);
      continue;
    }
    // q | k | v as ONE projection: rows concatenated, biases concatenated
    HostTensor W, Bv;
    W.shape = {qd + 2 * kd, m.hidden}; Bv.shape = {qd + 2 * kd};
    for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
      const HostTensor& a = ws.get(L + ".self_attn." + n + ".weight");
      const HostTensor& bb = ws.get(L + ".self_attn." + n + ".bias");
      FE_CHECK((int)a.shape[1] == m.hidden, "vlm: %s input width", n);
      finite(a, L + ".self_attn." + n);
      W.data.insert(W.data.end(), a.data.begin(), a.data.end());
      Bv.data.insert(Bv.data.end(), bb.data.begin(), bb.data.end());
    }
    FE_CHECK((int64_t)W.data.size() == W.shape[0] * W.shape[1], "vlm: layer %d q/k/v shapes do not match %d heads / %d kv heads of 128", i, cfg.n_heads, cfg.n_kv_heads);
    w.qkv = vlm_pack_linear(m.dw, m.weight_format, W, &Bv, L + ".self_attn.q|k|v_proj.weight");
    w.o = linear(L + ".self_attn.o_proj");
    w.gate = linear(L + ".mlp.gate_proj");
    w.up = linear(L + ".mlp.up_proj");
    w.down = linear(L + ".mlp.down_proj");
    w.ln1 = upload_bf16(m.dw, ws.get(L + ".input_layernorm.weight").data);
    w.ln2 = upload_bf16(m.dw, ws.get(L + ".post_attention_layernorm.weight").data);
    m.layers.push_back(w);
  }
  FE_CHECK(!m.layers.empty(), "vlm: no decoder layers found");
  m.norm = upload_bf16(m.dw, ws.get(P + "norm.weight").data);
  if (tied && f8) {      // the lookup keeps the bf16 table (looked-up rows are the original ones); the head is an e4m3 copy of it
    m.embed = upload_bf16(m.dw, E.data);
    m.lm_head = vlm_pack_linear(m.dw, m.weight_format, E, nullptr, P + "embed_tokens.weight");
  } else if (tied) {
    m.lm_head = build_linear_rows(m.dw, E, nullptr, 0, m.vocab);
    FE_CHECK(m.lm_head.wh && m.lm_head.hprec == PREC_BF16, "vlm: tied lm_head needs the bf16 form");
    if (m.lm_head.KpH == m.hidden) m.embed = (bf16*)m.lm_head.wh;      // one device copy: rows [vocab][hidden], row-major
    else m.embed = upload_bf16(m.dw, E.data);
  } else {
    m.lm_head = linear("lm_head");
  }
  m.weight_bytes = m.scale_bytes = m.quant_rows = 0;
  auto count = [&](const ConvW& w) {
    m.weight_bytes += (int64_t)w.Cout * w.KpH * (w.w8 ? 1 : 2);
    if (w.w8) { m.scale_bytes += 4 * (int64_t)w.Cout; m.quant_rows += w.Cout; }
  };
  for (const VlmLayerW& w : m.layers) { count(w.qkv); count(w.o); count(w.gate); count(w.up); count(w.down); }
  count(m.lm_head);
  FE_CHECK(cfg.n_deepstack <= (int)m.layers.size(), "vlm: %d DeepStack levels for %zu decoder layers", cfg.n_deepstack, m.layers.size());
  m.inter = m.layers[0].gate.Cout;
  // inv_freq as Qwen2_5_VLRotaryEmbedding.compute_default_rope_parameters: 1 / base^(2i / dim), fp32
  std::vector<float> inv(64);
  for (int i = 0; i < 64; ++i) inv[i] = 1.0f / powf(cfg.rope_theta, (float)(2 * i) / 128.0f);
  m.inv_freq = m.dw.upload(inv);
  if (cfg.qwen3 || cfg.qwen2) build_vlm_ln_vision(m, ws);      // model.visual.* when the checkpoint carries it
  else build_vlm_vision(m, ws);
}

int64_t VlmModel::kv_token_bytes(int format) const {
  return (int64_t)layers.size() * cfg.n_kv_heads * 2 * (format == FE_VLM_KV_E4M3 ? 128 + 4 : 256);
}
void VlmModel::reserve_cache(int B, int max_seq_, int format) {
  FE_CHECK(format == FE_VLM_KV_BF16 || format == FE_VLM_KV_E4M3 || format == FE_VLM_KV_BF16_E4M3, "vlm: kv format %d", format);
  const size_t rows = (size_t)B * cfg.n_kv_heads * max_seq_;
  if (B == cache_B && max_seq_ == max_seq && format == kv_format && !kcache.empty()) return;
  release_cache();
  kv_format = format;
  const bool f8 = format == FE_VLM_KV_E4M3;
  for (size_t i = 0; i < layers.size(); ++i) {
    void *k = nullptr, *v = nullptr;
    FE_HIP(hipMalloc(&k, rows * 128 * (f8 ? 1 : sizeof(bf16))));
    kcache.push_back((bf16*)k);
    FE_HIP(hipMalloc(&v, rows * 128 * (f8 ? 1 : sizeof(bf16))));
    vcache.push_back((bf16*)v);
    if (f8) {
      void *ks = nullptr, *vs = nullptr;
      FE_HIP(hipMalloc(&ks, rows * sizeof(float)));
      kscale.push_back((float*)ks);
      FE_HIP(hipMalloc(&vs, rows * sizeof(float)));
      vscale.push_back((float*)vs);
    }
  }
  cache_bytes = (int64_t)layers.size() * 2 * rows * (f8 ? 128 + 4 : 256);
  FE_HIP(hipMalloc((void**)&pad, (size_t)B * sizeof(int)));
  FE_HIP(hipMemset(pad, 0, (size_t)B * sizeof(int)));
  FE_HIP(hipMalloc((void**)&last_lp, (size_t)B * sizeof(float)));
  FE_HIP(hipMemset(last_lp, 0xff, (size_t)B * sizeof(float)));      // NaN until a selection writes it
  cache_B = B; max_seq = max_seq_; cur_len = 0;
}
void VlmModel::release_cache() {
  for (bf16* p : kcache) (void)hipFree(p);
  for (bf16* p : vcache) (void)hipFree(p);
  for (float* p : kscale) (void)hipFree(p);
  for (float* p : vscale) (void)hipFree(p);
  if (pad) (void)hipFree(pad);
  if (last_lp) (void)hipFree(last_lp);
  pad = nullptr; last_lp = nullptr;
  kcache.clear(); vcache.clear(); kscale.clear(); vscale.clear();
  cache_B = 0; max_seq = 0; cur_len = 0; cache_bytes = 0;
}

void vlm_kv_fill(Ctx& c, const VlmKv& kv, const bf16* ksrc, const bf16* vsrc, int n, int L) {
  FE_CHECK(n > 0 && L > 0 && L <= kv.max_seq && kv.k && kv.v && (kv.format != FE_VLM_KV_E4M3 || (kv.ks && kv.vs)), "vlm_kv_fill: %d rows of %d do not fit the cache", L, kv.max_seq);
  const dim3 grid(grid_n((size_t)2 * n * L * 64)), block(256);
#define VLM_FILL(F) hipLaunchKernelGGL(vlm_kv_fill_kernel<F>, grid, block, 0, c.stream, ksrc, vsrc, kv.k, kv.v, kv.ks, kv.vs, n, L, kv.max_seq)
  if (kv.format == FE_VLM_KV_E4M3) VLM_FILL(FE_VLM_KV_E4M3);
  else if (kv.format == FE_VLM_KV_BF16_E4M3) VLM_FILL(FE_VLM_KV_BF16_E4M3);
  else VLM_FILL(FE_VLM_KV_BF16);
#undef VLM_FILL
  FE_HIP(hipGetLastError());
}

void vlm_decode_attention(Ctx& c, const VlmKv& kv, const bf16* q, int B, int nh, int nkv, int Lk, const int* len_dev, const int* pad, float* po, float* pm,
                          float* pl, int nsplit, bf16* out) {
  const int G = nh / nkv;
  const float scale = 1.0f / sqrtf(128.f);
  FE_CHECK(nkv > 0 && nh % nkv == 0 && Lk > 0 && Lk <= kv.max_seq && nsplit == ((len_dev ? kv.max_seq : Lk) + VLM_DEC_CHUNK - 1) / VLM_DEC_CHUNK, "vlm decode attention: bad shape");
  const bool f8 = kv.format == FE_VLM_KV_E4M3;
  FE_CHECK(!f8 || (kv.ks && kv.vs), "vlm decode attention: an e4m3 cache without scales");
  const dim3 grid(B * nkv, nsplit);
#define VLM_DEC_LAUNCH(GG)                                                                                                                                  \
  if (f8)                                                                                                                                                   \
    hipLaunchKernelGGL((vlm_attn_decode_gqa_kernel<GG, uint8_t>), grid, dim3(256), 0, c.stream, q, (const uint8_t*)kv.k, (const uint8_t*)kv.v,                  \
                       (const float*)kv.ks, (const float*)kv.vs, po, pm, pl, nh, nkv, Lk, kv.max_seq, scale, len_dev, nsplit, pad);                         \
  else                                                                                                                                                      \
    hipLaunchKernelGGL((vlm_attn_decode_gqa_kernel<GG, bf16>), grid, dim3(256), 0, c.stream, q, (const bf16*)kv.k, (const bf16*)kv.v, (const float*)kv.ks,      \
                       (const float*)kv.vs, po, pm, pl, nh, nkv, Lk, kv.max_seq, scale, len_dev, nsplit, pad)
  switch (G) {
    case 1: VLM_DEC_LAUNCH(1); break;
    case 2: VLM_DEC_LAUNCH(2); break;
    case 3: VLM_DEC_LAUNCH(3); break;
    case 4: VLM_DEC_LAUNCH(4); break;
    case 5: VLM_DEC_LAUNCH(5); break;
    case 6: VLM_DEC_LAUNCH(6); break;
    case 7: VLM_DEC_LAUNCH(7); break;
    case 8: VLM_DEC_LAUNCH(8); break;
    default: FE_CHECK(false, "vlm decode attention: %d query heads per KV head (1 .. 8 are built)", G);
  }
#undef VLM_DEC_LAUNCH
  hipLaunchKernelGGL(vlm_attn_combine_kernel, dim3(B * nh), dim3(128), 0, c.stream, (const float*)po, (const float*)pm, (const float*)pl, out, nsplit);
  FE_HIP(hipGetLastError());
}

void vlm_prefill_attention(Ctx& c, const bf16* q, const bf16* kc, const bf16* vc, int max_seq, int B, int nh, int nkv, int Lq, int Lk, int qpos0, const int* pad,
                           bf16* out) {
  FE_CHECK(q && kc && vc && pad && out && B > 0 && nkv > 0 && nh % nkv == 0 && Lq > 0 && qpos0 >= 0 && Lk == qpos0 + Lq && Lk <= max_seq && (size_t)B * nh <= 65535,
           "vlm prefill attention: %d x %d heads over %d KV heads, %d queries from position %d, %d keys of a cache of %d", B, nh, nkv, Lq, qpos0, Lk, max_seq);
  const float scale = 1.0f / sqrtf(128.f);
  const int qd = nh * 128;
  VlmAttnParams ap{q, qd, kc, vc, out, qd, B, nh, nkv, Lq, Lk, max_seq, qpos0, scale, pad};
  hipLaunchKernelGGL(vlm_attn_prefill_kernel, dim3((Lq + 127) / 128, B * nh), dim3(256), 0, c.stream, ap);
  FE_HIP(hipGetLastError());
}


// ---- the launches of the row passes (engine.h): vlm_forward, the vision towers and the fe_op_vlm_* test hooks all come through here ------
int vlm_grid(size_t n_threads, int max_blocks) {
  int g = grid_n(n_threads);
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  // (the wave-per-row kernels derive row and lane from the global thread index)
  FE_CHECK(max_blocks >= 0 && ((size_t)g * 256) % 64 == 0, "vlm: a launch of %d workgroups (max_blocks %d) does not keep a wave on one row", g, max_blocks);
  return g;
}
void vlm_rmsnorm(Ctx& c, const bf16* x, int ldx, const bf16* w, bf16* y, int ldy, int rows, int d, float eps, int max_blocks) {
  FE_CHECK(rows > 0 && d > 0 && d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= d && ldy >= d, "vlm_rmsnorm: %d rows of %d values at strides %d, %d (multiples of 4)",
           rows, d, ldx, ldy);
  hipLaunchKernelGGL(vlm_rmsnorm_kernel, dim3(vlm_grid((size_t)rows * 64, max_blocks)), dim3(256), 0, c.stream, x, ldx, w, y, ldy, rows, d, eps);
  FE_HIP(hipGetLastError());
}
void vlm_add(Ctx& c, bf16* x, const bf16* y, size_t n, int max_blocks) {
  FE_CHECK(n % 4 == 0, "vlm_add: %zu values (a multiple of 4)", n);
  hipLaunchKernelGGL(vlm_add_kernel, dim3(vlm_grid(n / 4, max_blocks)), dim3(256), 0, c.stream, x, y, n / 4);
  FE_HIP(hipGetLastError());
}
void vlm_silu_mul(Ctx& c, const bf16* g, const bf16* u, bf16* h, size_t n, int max_blocks) {
  FE_CHECK(n % 4 == 0, "vlm_silu_mul: %zu values (a multiple of 4)", n);
  hipLaunchKernelGGL(vlm_silu_mul_kernel, dim3(vlm_grid(n / 4, max_blocks)), dim3(256), 0, c.stream, g, u, h, n / 4);
  FE_HIP(hipGetLastError());
}
void vlm_add_rmsnorm(Ctx& c, bf16* x, const bf16* y, const bf16* w, bf16* n, int rows, int d, float eps, const int* slot, const bf16* ds, int max_blocks) {
  FE_CHECK(rows > 0 && d > 0 && d % 4 == 0 && (!ds || slot) && (!w || n), "vlm_add_rmsnorm: %d rows of %d values (a multiple of 4)", rows, d);
  const dim3 grid(vlm_grid((size_t)rows * 64, max_blocks));
  if (ds) hipLaunchKernelGGL(vlm_add_rmsnorm_kernel<true>, grid, dim3(256), 0, c.stream, x, y, w, n, rows, d, eps, slot, ds);
  else hipLaunchKernelGGL(vlm_add_rmsnorm_kernel<false>, grid, dim3(256), 0, c.stream, x, y, w, n, rows, d, eps, (const int*)nullptr, (const bf16*)nullptr);
  FE_HIP(hipGetLastError());
}
void vlm_few_rows_rmsnorm(Ctx& c, bf16* x, const bf16* w, bf16* n, int rows, int d, float eps) {
  FE_CHECK(rows > 0 && rows <= 64 && d > 0 && d % 4 == 0 && w && n, "vlm_few_rows_rmsnorm: %d rows (1 .. 64) of %d values (a multiple of 4)", rows, d);
  hipLaunchKernelGGL(vlm_finish_add_rmsnorm_kernel<false>, dim3(rows), dim3(1024), 0, c.stream, (const float*)nullptr, 0, rows, d, (const float*)nullptr, x, w, n, eps,
                     (const int*)nullptr, (const bf16*)nullptr);
  FE_HIP(hipGetLastError());
}
void vlm_rope_cache(Ctx& c, const VlmRope& r, const VlmKv& kv, const bf16* qkv, const int* pos, const float* inv_freq, bf16* q_out) {
  const int rows = r.B * r.L;
  FE_CHECK(r.B > 0 && r.L > 0 && r.nh > 0 && r.nkv > 0 && qkv && pos && inv_freq && q_out && kv.k && kv.v, "vlm_rope_cache: %d x %d rows, %d + 2 x %d heads", r.B, r.L,
           r.nh, r.nkv);
  FE_CHECK(r.start_dev || (r.start >= 0 && r.start + r.L <= kv.max_seq), "vlm_rope_cache: positions %d .. %d do not fit the cache (%d)", r.start, r.start + r.L - 1,
           kv.max_seq);
  FE_CHECK(kv.format != FE_VLM_KV_E4M3 || (kv.ks && kv.vs), "vlm_rope_cache: an e4m3 cache without scales");
  FE_CHECK(!r.qwen3 || (r.qn && r.kn), "vlm_rope_cache: the Qwen3 form takes q / k norm weights");
  const dim3 grid(vlm_grid((size_t)rows * (r.nh + 2 * r.nkv) * 64, r.max_blocks)), block(256);
#define VLM_ROPE(F)                                                                                                                                                \
  do {                                                                                                                                                             \
    if (r.qwen3)                                                                                                                                                   \
      hipLaunchKernelGGL(vlm3_qk_rope_cache_kernel<F>, grid, block, 0, c.stream, qkv, pos, inv_freq, r.qn, r.kn, q_out, kv.k, kv.v, rows, r.L, r.nh, r.nkv, r.s1,  \
                         r.s2, r.start, kv.max_seq, r.start_dev, r.eps, kv.ks, kv.vs);                                                                             \
    else                                                                                                                                                           \
      hipLaunchKernelGGL(vlm_rope_cache_kernel<F>, grid, block, 0, c.stream, qkv, pos, inv_freq, q_out, kv.k, kv.v, rows, r.L, r.nh, r.nkv, r.s0, r.s1, r.start,   \
                         kv.max_seq, r.start_dev, kv.ks, kv.vs);                                                                                                   \
  } while (0)
  if (kv.format == FE_VLM_KV_BF16) VLM_ROPE(FE_VLM_KV_BF16);
  else if (kv.format == FE_VLM_KV_E4M3) VLM_ROPE(FE_VLM_KV_E4M3);
  else VLM_ROPE(FE_VLM_KV_BF16_E4M3);
#undef VLM_ROPE
  FE_HIP(hipGetLastError());
}
void vlm_put_rows(Ctx& c, bf16* x, const bf16* rows, const int* index, int n, int d) {
  hipLaunchKernelGGL(vlm_put_rows_kernel, dim3(grid_n((size_t)n * d / 8)), dim3(256), 0, c.stream, x, rows, index, n, d);
  FE_HIP(hipGetLastError());
}

// x: [B*L][hidden] bf16 rows (token embeddings, image rows already in place), pos: device [3][B*L]. Appends L positions to the cache of
// every sequence, leaves the next token of every sequence in next_dev [B], (optionally) the bf16-rounded logits in logits_dev [B][vocab] and
// (optionally) the log-probabilities of the chosen tokens in lp_dev [B]. len_dev (decode steps only): the cache length in device memory,
// read by the kernels instead of the host's cur_len - the form a captured graph replays.
void vlm_forward(Ctx& c, VlmModel& m, bf16* x, const int* pos, int B, int L, int* next_dev, float* logits_dev, const int* len_dev, float* lp_dev) {
  const VlmConfig& g = m.cfg;
  const int rows = B * L, d = m.hidden, nh = g.n_heads, nkv = g.n_kv_heads, qd = nh * 128, qkvd = (nh + 2 * nkv) * 128;
  const int start = m.cur_len, Lk = start + L;
  FE_CHECK(B == m.cache_B && Lk <= m.max_seq && m.pad, "vlm: %d sequences x %d positions do not fit the cache (%d x %d)", B, Lk, m.cache_B, m.max_seq);
  const size_t mark = c.arena.mark();
  bf16* n = c.arena.array<bf16>((size_t)rows * d);
  bf16* qkv = c.arena.array<bf16>((size_t)rows * qkvd);
  bf16* qr = c.arena.array<bf16>((size_t)rows * qd);
  bf16* ao = c.arena.array<bf16>((size_t)rows * qd);
  bf16* br = c.arena.array<bf16>((size_t)rows * d);
  bf16* gg = c.arena.array<bf16>((size_t)rows * m.inter);
  bf16* uu = c.arena.array<bf16>((size_t)rows * m.inter);
  FE_CHECK(m.kcache.size() == m.layers.size() && (m.kv_format != FE_VLM_KV_E4M3 || m.kscale.size() == m.layers.size()), "vlm: no KV cache");
  const bool f8kv = m.kv_format == FE_VLM_KV_E4M3;
  // (e4m3 formats: a prefill's own K / V, see the layer loop; every prefill entry point starts at position 0)
  FE_CHECK(m.kv_format == FE_VLM_KV_BF16 || L == 1 || start == 0, "vlm: a prefill under an e4m3 KV format starts at position 0 (cache holds %d)", start);
  bf16* const pk = m.kv_format != FE_VLM_KV_BF16 && L > 1 ? c.arena.array<bf16>((size_t)B * nkv * L * 128) : nullptr;
  bf16* const pv = pk ? c.arena.array<bf16>((size_t)B * nkv * L * 128) : nullptr;
  // decode attention: keys split over workgroups, merged by a second launch (graph replay: the grid covers the whole cache)
  const int nsplit = L == 1 ? ((len_dev ? m.max_seq : Lk) + VLM_DEC_CHUNK - 1) / VLM_DEC_CHUNK : 0;
  float* po = nsplit ? c.arena.array<float>((size_t)B * nh * nsplit * 128) : nullptr;
  float* pm = nsplit ? c.arena.array<float>((size_t)B * nh * nsplit) : nullptr;
  float* pl = nsplit ? c.arena.array<float>((size_t)B * nh * nsplit) : nullptr;
  // (few rows: one 1024-thread workgroup per row - the wave-per-row kernel walks a 3584-wide row in 14 dependent steps, 11 us for 32 rows;
  // with no split sums to take, the finishing pass is x = bf16(x + 0), n = RMSNorm(x) w)
  const bool few_rows = rows <= 64 && d % 4 == 0;
  if (few_rows) vlm_few_rows_rmsnorm(c, x, (const bf16*)m.layers[0].ln1, n, rows, d, g.rms_eps);
  else vlm_rmsnorm(c, (const bf16*)x, d, (const bf16*)m.layers[0].ln1, n, d, rows, d, g.rms_eps);
  for (size_t li = 0; li < m.layers.size(); ++li) {
    const VlmLayerW& w = m.layers[li];
    vlm_linear(c, w.qkv, (const bf16*)n, d, rows, qkv, qkvd);
    // e4m3 formats, prefill: the rope kernel writes the prompt's K / V as bf16 rows into scratch ([B][nkv][L][128], the bf16 instantiation
    // with max_seq = L), the prefill attention runs over that scratch unchanged, and vlm_kv_fill leaves the quantised rows in the cache.
    // Decode steps (L == 1) quantise in the rope kernel itself: no launch is added to a step.
    VlmKv kv{m.kv_format, m.kcache[li], m.vcache[li], f8kv ? m.kscale[li] : (float*)nullptr, f8kv ? m.vscale[li] : (float*)nullptr, m.max_seq};
    const bool staged = pk != nullptr;
    const VlmKv rkv = staged ? VlmKv{FE_VLM_KV_BF16, pk, pv, nullptr, nullptr, L} : kv;
    bf16* const rk = rkv.k;
    bf16* const rv = rkv.v;
    const int rseq = rkv.max_seq;
    VlmRope rope;
    rope.qwen3 = g.qwen3; rope.qn = (const bf16*)w.qn; rope.kn = (const bf16*)w.kn; rope.eps = g.rms_eps;
    rope.s0 = g.mrope[0]; rope.s1 = g.mrope[1]; rope.s2 = g.mrope[2];
    rope.B = B; rope.L = L; rope.nh = nh; rope.nkv = nkv;
    rope.start = start; rope.start_dev = L == 1 ? len_dev : (const int*)nullptr;
    vlm_rope_cache(c, rope, rkv, (const bf16*)qkv, pos, (const float*)m.inv_freq, qr);
    if (L == 1) {
      vlm_decode_attention(c, kv, (const bf16*)qr, B, nh, nkv, Lk, len_dev, (const int*)m.pad, po, pm, pl, nsplit, ao);
    } else {
      vlm_prefill_attention(c, (const bf16*)qr, (const bf16*)rk, (const bf16*)rv, rseq, B, nh, nkv, L, Lk, start, (const int*)m.pad, ao);
      if (staged) vlm_kv_fill(c, kv, (const bf16*)pk, (const bf16*)pv, B * nkv, L);
    }
    FE_HIP(hipGetLastError());
    c.flops_accum += 4.0 * B * nh * (double)L * (start + (L + 1) * 0.5) * 128;
    c.flops_half += 4.0 * B * nh * (double)L * (start + (L + 1) * 0.5) * 128;
    const bf16* const next_ln = li + 1 < m.layers.size() ? (const bf16*)m.layers[li + 1].ln1 : (const bf16*)nullptr;
    // DeepStack (Qwen3-VL prefill): the image rows of this layer's output take feature block li (the slot map is set for a prefill only)
    const bf16* const ds = m.ds_slot && (int)li < m.ds_n ? (const bf16*)m.ds_feats + (size_t)li * m.ds_cap * d : (const bf16*)nullptr;
    // 5 .. 32 sequences: the split sums of the weight-streaming GEMM are taken by the pass that follows the projection (residual +
    // norm, SwiGLU product) instead of a finishing launch of their own
    const bool fused = d % 4 == 0 && m.inter % 4 == 0 && vlm_uses_gemm32(w.o, rows) && vlm_uses_gemm32(w.gate, rows) && vlm_uses_gemm32(w.up, rows) &&
                       vlm_uses_gemm32(w.down, rows) && !w.o.shift && !w.gate.shift && !w.up.shift && !w.down.shift && w.gate.KpH == w.up.KpH;
    if (fused) {
      const size_t pm = c.arena.mark();
      vlm_proj_add_rmsnorm(c, w.o, (const bf16*)ao, qd, rows, x, (const bf16*)w.ln2, n, g.rms_eps, nullptr, nullptr);
      vlm_gate_up_silu_mul(c, w.gate, w.up, (const bf16*)n, d, rows, gg);
      vlm_proj_add_rmsnorm(c, w.down, (const bf16*)gg, m.inter, rows, x, next_ln, n, g.rms_eps, ds ? m.ds_slot : (const int*)nullptr, ds);
      c.arena.rewind(pm);
      continue;
    }
    vlm_linear(c, w.o, (const bf16*)ao, qd, rows, br, d);
    vlm_add_rmsnorm(c, x, (const bf16*)br, (const bf16*)w.ln2, n, rows, d, g.rms_eps);
    vlm_linear(c, w.gate, (const bf16*)n, d, rows, gg, m.inter);
    vlm_linear(c, w.up, (const bf16*)n, d, rows, uu, m.inter);
    vlm_silu_mul(c, (const bf16*)gg, (const bf16*)uu, gg, (size_t)rows * m.inter);
    vlm_linear(c, w.down, (const bf16*)gg, m.inter, rows, br, d);
    // x += down(...) and, in the same launch, the next layer's input norm (none after the last layer)
    vlm_add_rmsnorm(c, x, (const bf16*)br, next_ln, n, rows, d, g.rms_eps, ds ? m.ds_slot : (const int*)nullptr, ds);
  }
  // final norm + lm_head on the last position of every sequence
  bf16* last = c.arena.array<bf16>((size_t)B * d);
  bf16* lastn = c.arena.array<bf16>((size_t)B * d);
  hipLaunchKernelGGL(vlm_last_rows_kernel, dim3((B * d + 255) / 256), dim3(256), 0, c.stream, (const bf16*)x, last, B, L, d);
  if (B <= 64 && d % 4 == 0) vlm_few_rows_rmsnorm(c, last, (const bf16*)m.norm, lastn, B, d, g.rms_eps);
  else vlm_rmsnorm(c, (const bf16*)last, d, (const bf16*)m.norm, lastn, d, B, d, g.rms_eps);
  float* lg = logits_dev ? logits_dev : c.arena.array<float>((size_t)B * m.vocab);
  vlm_logits(c, m.lm_head, (const bf16*)lastn, d, B, lg, m.vocab);      // (scratch: rewound below)
  vlm_select(c, lg, B, m.vocab, next_dev, lp_dev);
  m.cur_len = Lk;
  c.arena.rewind(mark);
}

// greedy selection over rows of fp32 logits lg [B][vocab] (rounded to bf16 in place): next_dev [B] the chosen ids, lp_dev [B] (nullable) their
// log-probabilities. lp_dev == nullptr launches the plain kernels: the ids do not depend on it.
void vlm_select(Ctx& c, float* lg, int B, int vocab, int* next_dev, float* lp_dev) {
  FE_CHECK(B > 0 && B <= 65535 && vocab > 0, "vlm select: %d rows of %d logits", B, vocab);
  const size_t mark = c.arena.mark();
  float* apv = c.arena.array<float>((size_t)B * VLM_AM_CHUNKS);
  int* api = c.arena.array<int>((size_t)B * VLM_AM_CHUNKS);
  if (lp_dev) {
    float* aps = c.arena.array<float>((size_t)B * VLM_AM_CHUNKS);
    hipLaunchKernelGGL(vlm_argmax_part_kernel<true>, dim3(VLM_AM_CHUNKS, B), dim3(256), 0, c.stream, lg, vocab, apv, api, aps);
    hipLaunchKernelGGL(vlm_argmax_final_kernel<true>, dim3(B), dim3(64), 0, c.stream, (const float*)apv, (const int*)api, next_dev, (const float*)aps, lp_dev);
  } else {
    hipLaunchKernelGGL(vlm_argmax_part_kernel<false>, dim3(VLM_AM_CHUNKS, B), dim3(256), 0, c.stream, lg, vocab, apv, api, (float*)nullptr);
    hipLaunchKernelGGL(vlm_argmax_final_kernel<false>, dim3(B), dim3(64), 0, c.stream, (const float*)apv, (const int*)api, next_dev, (const float*)nullptr,
                       (float*)nullptr);
  }
  FE_HIP(hipGetLastError());
  c.arena.rewind(mark);
}

// n_steps greedy decode steps with NO host round trip: token ids, positions and the cache length live in device memory, one step is
// captured into a HIP graph (~12 launches per layer: at the reference's batch sizes a step is launch-bound otherwise) and replayed.
// tok_dev [B] holds the tokens to feed first (the prefill's choice), pos_dev [3][B] their positions; out_dev [n_steps][B] receives the
// tokens chosen by the steps and (out_lp != nullptr) out_lp [n_steps][B] their log-probabilities, by way of the model's last_lp. Leaves
// cur_len advanced by n_steps.
void vlm_decode_steps(Ctx& c, VlmModel& m, int* tok_dev, int* pos_dev, int B, int n_steps, int* out_dev, float* out_lp, VlmUntil* until) {
  if (until) until->steps_run = 0;
  if (n_steps <= 0) return;
  FE_CHECK(B <= 1024, "vlm: %d sequences (one workgroup advances the decode state: at most 1024)", B);
  FE_CHECK(!until || (until->n_eos >= 0 && until->n_eos <= 8 && until->poll >= 1 && until->fin_dev && until->live_dev), "vlm: bad stop rule");
  FE_CHECK(B == m.cache_B && m.cur_len > 0 && m.cur_len + n_steps <= m.max_seq, "vlm: %d more positions do not fit the cache (%d of %d used)", n_steps, m.cur_len, m.max_seq);
  const size_t mark = c.arena.mark();
  int* st = c.arena.array<int>(4);                 // [0] cache length, [1] step counter
  int* next = c.arena.array<int>((size_t)B);
  bf16* x = c.arena.array<bf16>((size_t)B * m.hidden);
  const int init[2] = {m.cur_len, 0};
  FE_HIP(hipMemcpyAsync(st, init, sizeof init, hipMemcpyHostToDevice, c.stream));
  VlmEosIds eos{};
  if (until) { eos.n = until->n_eos; for (int e = 0; e < until->n_eos; ++e) eos.id[e] = until->eos[e]; }
  auto one_step = [&]() {
    vlm_embed(c, m, tok_dev, B, x);
    vlm_forward(c, m, x, pos_dev, B, 1, next, nullptr, st, out_lp ? m.last_lp : nullptr);
#define VLM_ADVANCE(LP, UNTIL)                                                                                                                  \
  hipLaunchKernelGGL((vlm_advance_kernel<LP, UNTIL>), dim3(1), dim3(64 * ((B + 63) / 64)), 0, c.stream, (const int*)next, tok_dev, pos_dev, st, st + 1,   \
                     out_dev, B, LP ? (const float*)m.last_lp : (const float*)nullptr, out_lp, eos, until ? until->fin_dev : (int*)nullptr,   \
                     until ? until->live_dev : (int*)nullptr)
    if (until) { if (out_lp) VLM_ADVANCE(true, true); else VLM_ADVANCE(false, true); }
    else { if (out_lp) VLM_ADVANCE(true, false); else VLM_ADVANCE(false, false); }
#undef VLM_ADVANCE
    FE_HIP(hipGetLastError());
  };
  // the stop rule: after every `poll` steps (and never after the last) the host reads the running count and stops launching at zero
  int done = 1;      // steps launched so far
  auto stop_here = [&]() {
    if (!until || done % until->poll != 0 || done >= n_steps) return false;
    int live = 0;
    FE_HIP(hipMemcpyAsync(&live, until->live_dev, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    FE_HIP(hipStreamSynchronize(c.stream));
    return live == 0;
  };
  const int len0 = m.cur_len;
  one_step();                                      // outside the graph: first-use attributes (dynamic LDS sizes) are set here
  static const bool no_graph = getenv("FE_VLM_NO_GRAPH") != nullptr;      // A/B hook
  // replayed from a graph the ~60 launches of a step carry a dependency edge each: worth it while the step is launch-bound (1-2 sequences:
  // 0.68 vs 0.70 ms per 4-layer step), slower than back-to-back stream launches above that (32 sequences: 1.21 vs 1.10 ms; profiles/r03_vlm_perf.txt)
  if (stop_here()) {
    // every sequence had finished after the first step
  } else if (n_steps > 1 && !no_graph && B <= 2) {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    FE_HIP(hipStreamBeginCapture(c.stream, hipStreamCaptureModeThreadLocal));
    m.cur_len = len0 + 1;                          // (host copy: only the cache-capacity check reads it during capture)
    try { one_step(); } catch (...) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(c.stream, &g); if (g) (void)hipGraphDestroy(g); throw; }
    FE_HIP(hipStreamEndCapture(c.stream, &graph));
    FE_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    bool stop = false;
    try {
      for (; done < n_steps && !stop; stop = stop_here()) { FE_HIP(hipGraphLaunch(exec, c.stream)); ++done; }
      FE_HIP(hipStreamSynchronize(c.stream));
    } catch (...) { (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph); throw; }
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
  } else {
    for (bool stop = false; done < n_steps && !stop; stop = stop_here()) { m.cur_len = len0 + done; one_step(); ++done; }
  }
  if (until) until->steps_run = done;
  m.cur_len = len0 + done;
  c.arena.rewind(mark);
}

void vlm_embed(Ctx& c, const VlmModel& m, const int* tok_dev, int rows, bf16* x) {
  hipLaunchKernelGGL(vlm_embed_kernel, dim3(grid_n((size_t)rows * m.hidden / 8)), dim3(256), 0, c.stream, tok_dev, (const bf16*)m.embed, x, rows, m.hidden, m.vocab);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
