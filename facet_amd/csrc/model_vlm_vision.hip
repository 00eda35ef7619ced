// VLM tagger, slice 2: the vision tower of Qwen2.5-VL (SURVEY 8(f)-4 / BASELINE configs[4]) - pixel patches in, merged image embeddings out.
//
// Stands behind `Qwen2_5_VLForConditionalGeneration.get_image_features` = `model.visual(pixel_values, grid_thw).pooler_output`, which
// `generate(**inputs)` runs on the processor's `pixel_values [n_patches, 3*2*14*14]` / `image_grid_thw` (reference models/vlm_tagger.py:
// 245-259, 346-360). transformers' Qwen2_5_VisionTransformerPretrainedModel [modeling_qwen2_5_vl.py]: Conv3d patch embedding (a
// [n, 1176] x [1176, hidden] product) -> rows regrouped window by window (`window_index`, units of the 2x2 merge block) -> `depth` blocks
// { x += proj(attn(rope2d(qkv(RMSNorm(x))))) ; x += down(silu(gate(n)) * up(n)), n = RMSNorm(x) } where attention runs inside 112-pixel
// windows (<= 64 patches) except in the `fullatt_block_indexes` blocks (whole image) -> patch merger (RMSNorm, 4 rows -> 1, Linear - GELU -
// Linear to the decoder width) -> rows back in raster order. bf16 with the rounding points of the bf16 torch modules (each Linear output,
// RMSNorm before the weight multiply, SiLU before the gate multiply, residual sums, GELU); the rotary embedding is applied in fp32 on the
// bf16 q / k and rounded once, as apply_rotary_pos_emb_vision does. head_dim is 80 (1280 / 16): the attention tile (vlm_attn_tile.h) runs 5
// k-steps per S tile and three 32-row d-tiles of O (rows 80..95 of V^T are zeros). The index arrays (positions, window order, segment bounds) are
// the host's (facet_amd/vlm_tagger.py: numpy restatements of transformers.vision_utils, pinned by the golden vectors).
// Parity: tests/test_vlm_gpu.py against tests/golden/vlm_vision_golden.npz (the reference's own class) - pinned.
#include "engine.h"
#include "vlm_attn_tile.h"
#include <algorithm>
#include <cmath>

namespace fe {

// dst rows (4 i + j) = src rows (4 index[i] + j): the window regrouping (scatter = false) and its inverse on merged rows (units of 1 row)
__global__ void vlm_vis_gather_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, const int* __restrict__ index, int groups, int unit, int d, int scatter) {
  const size_t total = (size_t)groups * unit * (d / 8);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % (d / 8)) * 8;
    const size_t row = i / (d / 8);
    const int g = (int)(row / unit), j = (int)(row % unit);
    const size_t other = (size_t)index[g] * unit + j;
    const size_t s = scatter ? row : other, t = scatter ? other : row;
    *reinterpret_cast<uint4*>(dst + t * d + c) = *reinterpret_cast<const uint4*>(src + s * d + c);
  }
}

// 2-D rotary embedding of a vision tower on the q and k thirds of a fused qkv row block. Frequencies: inv_freq[j], j < HD/4; dimension
// i of a head (pairs (i, i + HD/2)) takes, with jj = i % (HD/2): the row position and inv_freq[jj] for jj < HD/4, the column position and
// inv_freq[jj - HD/4] otherwise. fp32 arithmetic on the bf16 values, one rounding (apply_rotary_pos_emb_vision).
template <int HD>
__global__ void vlm_vis_rope_kernel(const bf16* __restrict__ qkv, const int* __restrict__ pos, const float* __restrict__ inv_freq, bf16* __restrict__ q_out,
                                    bf16* __restrict__ k_out, int rows, int heads) {
  constexpr int hd = HD, half = HD / 2, quarter = HD / 4;
  const int dim = heads * hd;
  const size_t total = (size_t)rows * 2 * heads * half;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % half), hh = (int)((i / half) % (2 * heads)), row = (int)(i / ((size_t)half * 2 * heads));
    const int which = hh / heads, head = hh % heads;                    // 0: q, 1: k
    const bf16* src = qkv + (size_t)row * 3 * dim + which * dim + head * hd;
    const float p = (float)pos[2 * row + (d < quarter ? 0 : 1)];
    const float ang = p * inv_freq[d < quarter ? d : d - quarter];
    const float c = cosf(ang), s = sinf(ang);
    const float x1 = (float)src[d], x2 = (float)src[d + half];
    bf16* dst = (which ? k_out : q_out) + (size_t)row * dim + head * hd;
    dst[d] = (bf16)(x1 * c - x2 * s);
    dst[d + half] = (bf16)(x2 * c + x1 * s);
  }
}

// y = bf16(gelu_erf(x)) elementwise (nn.GELU() of the patch mergers on a bf16 tensor)
__global__ void vlm_gelu_kernel(bf16* __restrict__ x, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = ld4(x + 4 * i);
    auto f = [](float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); };
    st4(x + 4 * i, make_float4(f(a.x), f(a.y), f(a.z), f(a.w)));
  }
}

// ---- attention over packed variable-length segments, head_dim 64 or 80, non-causal ---------------------------------------------------------
// Segment s = rows cu[s] .. cu[s+1]-1 of the packed sequence (a window, or a whole image). One workgroup = NW waves x 32 queries of one
// (segment, head) on the tile of vlm_attn_tile.h, which the decoder's prefill kernel (model_vlm.hip) runs too.
struct VisAttnParams {
  const bf16* q; const bf16* k; int ldqk;       // rotated q / k: [N][heads*HD]
  const bf16* v; int ldv;                       // V third of the fused projection: [N][3*heads*HD] + 2*heads*HD
  bf16* o; int ldo;
  const int* cu; int heads; float scale;
};

template <int HD, int NW>
__global__ __launch_bounds__(NW * 64, 2) void vlm_vis_attn_kernel(const VisAttnParams p) {
  using T = VlmAttnTile<HD>;
  __shared__ __attribute__((aligned(16))) char Ks[2][T::K_BYTES];
  __shared__ __attribute__((aligned(16))) char Vs[2][T::V_BYTES];
  constexpr int NT = NW * 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int seg = blockIdx.y, head = blockIdx.z;
  const int s0 = p.cu[seg], len = p.cu[seg + 1] - s0;
  const int q0 = blockIdx.x * NW * 32;
  if (q0 >= len) return;
  T::template zero_vt_tail<NT>(Vs, t);
  const bf16* Qp = p.q + (size_t)s0 * p.ldqk + head * HD;
  const bf16* Kp = p.k + (size_t)s0 * p.ldqk + head * HD;
  const bf16* Vp = p.v + (size_t)s0 * p.ldv + head * HD;
  const int q = q0 + wave * 32 + r;
  const bool qok = q < len;
  const int qc = qok ? q : len - 1;
  typename T::F8 qf[T::KSTEPS];
  T::load_q(qf, Qp + (size_t)qc * p.ldqk, h);
  uint4 kr[T::pieces(NT)], vr[T::pieces(NT)];
  fe_f32x16 o[T::DT];
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int nt = (len + 31) / 32;
  T::template load<NT>(kr, vr, Kp, p.ldqk, Vp, p.ldv, 0, len - 1, t);
  T::template store<NT>(Ks[0], Vs[0], kr, vr, 0, len, t);
  __syncthreads();
  for (int kt = 0; kt < nt; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nt) T::template load<NT>(kr, vr, Kp, p.ldqk, Vp, p.ldv, kt + 1, len - 1, t);
    fe_f32x16 st = T::scores(Ks[buf], qf, r, h);
    T::softmax(st, m, l, o, p.scale, kt, h, [&](int key) { return key >= len; });      // every tile holds a live key: m stays finite
    T::pv(o, st, Vs[buf], r, h);
    if (kt + 1 < nt) T::template store<NT>(Ks[buf ^ 1], Vs[buf ^ 1], kr, vr, kt + 1, len, t);
    __syncthreads();
  }
  if (qok) T::write(p.o + (size_t)(s0 + q) * p.ldo + head * HD, o, l, h);
}

// ---- model ---------------------------------------------------------------------------------------------------------------------------------
void build_vlm_vision(VlmModel& m, const WeightStore& ws) {
  VlmVisionW& v = m.vis;
  const std::string P = "model.visual.";
  v.present = false;
  if (!ws.has(P + "patch_embed.proj.weight")) return;
  const HostTensor& pe = ws.get(P + "patch_embed.proj.weight");      // [hidden][3][t][p][p]
  HostTensor flat;
  flat.shape = {pe.shape[0], (int64_t)(pe.numel() / (size_t)pe.shape[0])};
  flat.data = pe.data;
  v.hidden = (int)flat.shape[0]; v.patch_dim = (int)flat.shape[1];
  v.heads = m.cfg.vis_heads;
  FE_CHECK(v.patch_dim % 8 == 0 && v.hidden % v.heads == 0 && v.hidden / v.heads == 80 && v.hidden % 32 == 0,
           "vlm vision: hidden %d over %d heads (the attention kernel is built for head_dim 80), patch vector %d", v.hidden, v.heads, v.patch_dim);
  v.patch = build_linear_rows(m.dw, flat, nullptr, 0, v.hidden);
  v.blocks.clear();
  for (int i = 0;; ++i) {
    const std::string B = P + "blocks." + std::to_string(i);
    if (!ws.has(B + ".attn.qkv.weight")) break;
    VlmVisionBlockW w;
    w.qkv = build_linear(m.dw, ws, B + ".attn.qkv", true);
    w.proj = build_linear(m.dw, ws, B + ".attn.proj", true);
    w.gate = build_linear(m.dw, ws, B + ".mlp.gate_proj", true);
    w.up = build_linear(m.dw, ws, B + ".mlp.up_proj", true);
    w.down = build_linear(m.dw, ws, B + ".mlp.down_proj", true);
    w.n1 = upload_bf16(m.dw, ws.get(B + ".norm1.weight").data);
    w.n2 = upload_bf16(m.dw, ws.get(B + ".norm2.weight").data);
    v.blocks.push_back(w);
  }
  FE_CHECK(!v.blocks.empty(), "vlm vision: no blocks found");
  v.inter = v.blocks[0].gate.Cout;
  v.ln_q = upload_bf16(m.dw, ws.get(P + "merger.ln_q.weight").data);
  v.m0 = build_linear(m.dw, ws, P + "merger.mlp.0", true);
  v.m2 = build_linear(m.dw, ws, P + "merger.mlp.2", true);
  v.out_hidden = v.m2.Cout;
  FE_CHECK(v.m0.Cin == 4 * v.hidden && v.out_hidden == m.hidden, "vlm vision: merger %d -> %d does not fit the tower (%d) / decoder (%d)", v.m0.Cin, v.out_hidden, v.hidden, m.hidden);
  v.inv_freq = vlm_vis_inv_freq(m.dw, 80);
  v.fullatt.assign(m.cfg.fullatt, m.cfg.fullatt + m.cfg.n_fullatt);
  v.present = true;
}

// ---- rope, segment attention and erf GELU of all three towers (the LayerNorm towers: model_vlm_ln_vision.hip) -----------------------------
static void vis_check_hd(int hd) { FE_CHECK(hd == 64 || hd == 80, "vlm vision: head_dim %d (the rope and attention kernels are built for 64 and 80)", hd); }
// VisionRotaryEmbedding(head_dim // 2): inv_freq = 1 / 10000^(arange(0, dim, 2) / dim), dim = head_dim / 2
float* vlm_vis_inv_freq(DeviceWeights& dw, int hd) {
  vis_check_hd(hd);
  std::vector<float> inv(hd / 4);
  for (int i = 0; i < hd / 4; ++i) inv[i] = 1.0f / powf(10000.0f, (float)(2 * i) / (float)(hd / 2));
  return dw.upload(inv);
}
void vlm_vis_rope(Ctx& c, int hd, const bf16* qkv, const int* pos, const float* inv_freq, bf16* q_out, bf16* k_out, int rows, int heads, int max_blocks) {
  vis_check_hd(hd);
  const dim3 grid(vlm_grid((size_t)rows * 2 * heads * (hd / 2), max_blocks));
  if (hd == 80) hipLaunchKernelGGL(vlm_vis_rope_kernel<80>, grid, dim3(256), 0, c.stream, qkv, pos, inv_freq, q_out, k_out, rows, heads);
  else hipLaunchKernelGGL(vlm_vis_rope_kernel<64>, grid, dim3(256), 0, c.stream, qkv, pos, inv_freq, q_out, k_out, rows, heads);
  FE_HIP(hipGetLastError());
}
template <int HD>
static void vis_attention_launch(Ctx& c, const VisAttnParams& ap, int n_seg, int max_seg) {
  if (max_seg <= 64) hipLaunchKernelGGL((vlm_vis_attn_kernel<HD, 2>), dim3((max_seg + 63) / 64, n_seg, ap.heads), dim3(128), 0, c.stream, ap);
  else hipLaunchKernelGGL((vlm_vis_attn_kernel<HD, 4>), dim3((max_seg + 127) / 128, n_seg, ap.heads), dim3(256), 0, c.stream, ap);
  FE_HIP(hipGetLastError());
}
void vlm_vis_attention(Ctx& c, int hd, const bf16* q, const bf16* k, const bf16* qkv, bf16* o, const int* cu, int n_seg, int max_seg, int heads) {
  vis_check_hd(hd);
  const int d = heads * hd;
  const VisAttnParams ap{q, k, d, qkv + 2 * d, 3 * d, o, d, cu, heads, 1.0f / sqrtf((float)hd)};
  if (hd == 80) vis_attention_launch<80>(c, ap, n_seg, max_seg);
  else vis_attention_launch<64>(c, ap, n_seg, max_seg);
}
void vlm_gelu_erf(Ctx& c, bf16* x, size_t n) {
  hipLaunchKernelGGL(vlm_gelu_kernel, dim3(grid_n(n / 4)), dim3(256), 0, c.stream, x, n / 4);
  FE_HIP(hipGetLastError());
}

static void vis_linear(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, bf16* y, int ldy) { linear_forward(c, w, x, ldx, M, y, ldy, ACT_NONE); }

// pv: device fp32 [N][patch_dim]; pos: device int [N][2] (row, column of every patch, ALREADY in window order); widx: device int [N/4]
// (window order -> raster group); cu_win / cu_full: device segment bounds (window order) with their host counts and longest segment;
// out: device bf16 [N/4][out_hidden], raster order.
void vlm_vision_forward(Ctx& c, VlmModel& m, const float* pv, int N, const int* pos, const int* widx, const int* cu_win, int n_win, int max_win,
                        const int* cu_full, int n_full, int max_full, bf16* out, const bf16* pv_bf16) {
  VlmVisionW& v = m.vis;
  FE_CHECK(v.present, "vlm: the checkpoint had no vision tower (model.visual.*)");
  FE_CHECK(N > 0 && N % 4 == 0, "vlm vision: %d patches (whole 2x2 merge blocks expected)", N);
  const int d = v.hidden, H = v.heads;
  const size_t mark = c.arena.mark();
  bf16* pvh = pv ? c.arena.array<bf16>((size_t)N * v.patch_dim) : nullptr;
  bf16* h0 = c.arena.array<bf16>((size_t)N * d);
  bf16* x = c.arena.array<bf16>((size_t)N * d);
  bf16* n = c.arena.array<bf16>((size_t)N * d);
  bf16* qkv = c.arena.array<bf16>((size_t)N * 3 * d);
  bf16* qr = c.arena.array<bf16>((size_t)N * d);
  bf16* kr = c.arena.array<bf16>((size_t)N * d);
  bf16* ao = c.arena.array<bf16>((size_t)N * d);
  bf16* br = c.arena.array<bf16>((size_t)N * d);
  // the MLP width (3420 at the 7B geometry) is not a multiple of 8: rows are padded to the 8 columns the 2-byte GEMM reads per chunk,
  // the padding zeroed once (silu(0) * 0 = 0 keeps it zero; the packed down_proj weights are zero there too)
  const int ip = (v.inter + 7) & ~7;
  bf16* gg = c.arena.array<bf16>((size_t)N * ip);
  bf16* uu = c.arena.array<bf16>((size_t)N * ip);
  if (ip != v.inter) {
    FE_HIP(hipMemsetAsync(gg, 0, (size_t)N * ip * sizeof(bf16), c.stream));
    FE_HIP(hipMemsetAsync(uu, 0, (size_t)N * ip * sizeof(bf16), c.stream));
  }
  if (pv) launch_convert(pv, pvh, (size_t)N * v.patch_dim, c.stream);      // pixel_values.to(bfloat16), as the patch embedding does
  vis_linear(c, v.patch, pv ? (const bf16*)pvh : pv_bf16, v.patch_dim, N, h0, d);
  hipLaunchKernelGGL(vlm_vis_gather_kernel, dim3(grid_n((size_t)N * d / 8)), dim3(256), 0, c.stream, (const bf16*)h0, x, widx, N / 4, 4, d, 0);
  FE_HIP(hipGetLastError());
  for (size_t li = 0; li < v.blocks.size(); ++li) {
    const VlmVisionBlockW& w = v.blocks[li];
    const bool full = std::find(v.fullatt.begin(), v.fullatt.end(), (int)li) != v.fullatt.end();
    vlm_rmsnorm(c, x, d, w.n1, n, d, N, d, 1e-6f);
    vis_linear(c, w.qkv, n, d, N, qkv, 3 * d);
    vlm_vis_rope(c, 80, qkv, pos, v.inv_freq, qr, kr, N, H);
    vlm_vis_attention(c, 80, qr, kr, qkv, ao, full ? cu_full : cu_win, full ? n_full : n_win, full ? max_full : max_win, H);
    vis_linear(c, w.proj, ao, d, N, br, d);
    vlm_add(c, x, br, (size_t)N * d);
    vlm_rmsnorm(c, x, d, w.n2, n, d, N, d, 1e-6f);
    vis_linear(c, w.gate, n, d, N, gg, ip);
    vis_linear(c, w.up, n, d, N, uu, ip);
    vlm_silu_mul(c, gg, uu, gg, (size_t)N * ip);
    vis_linear(c, w.down, gg, ip, N, br, d);
    vlm_add(c, x, br, (size_t)N * d);
  }
  // merger: RMSNorm per patch row, four consecutive rows = one merged row, Linear - GELU - Linear, then raster order
  vlm_rmsnorm(c, x, d, v.ln_q, n, d, N, d, 1e-6f);
  bf16* t0 = c.arena.array<bf16>((size_t)(N / 4) * 4 * d);
  bf16* e = c.arena.array<bf16>((size_t)(N / 4) * v.out_hidden);
  vis_linear(c, v.m0, n, 4 * d, N / 4, t0, 4 * d);
  vlm_gelu_erf(c, t0, (size_t)N * d);
  vis_linear(c, v.m2, t0, 4 * d, N / 4, e, v.out_hidden);
  hipLaunchKernelGGL(vlm_vis_gather_kernel, dim3(grid_n((size_t)(N / 4) * v.out_hidden / 8)), dim3(256), 0, c.stream, (const bf16*)e, out, widx, N / 4, 1, v.out_hidden, 1);
  FE_HIP(hipGetLastError());
  c.arena.rewind(mark);
}

}  // namespace fe
