// VLM tagger, Qwen3-VL: the vision tower - pixel patches in, merged image embeddings and the DeepStack feature blocks out.
//
// Stands behind `Qwen3VLForConditionalGeneration.get_image_features` (transformers Qwen3VLVisionModel [modeling_qwen3_vl.py]): Conv3d patch
// embedding with bias (a [n, 1536] x [1536, hidden] product: 16 x 16 patches, 2 frames) + the learned position table bilinearly resampled
// to each image's grid (align_corners=True: four taps per patch with fp32 weights, summed in fp32, rounded to bf16, added in bf16) ->
// `depth` blocks { x += proj(attn(rope2d(qkv(LayerNorm(x))))) ; x += fc2(gelu_tanh(fc1(LayerNorm(x)))) } with attention over each whole
// image (no windows; rows stay in the 2x2-block-major order of the processor) -> after the blocks named in deepstack_visual_indexes a
// DeepStack merger (4 rows viewed as one row of 4 hidden, LayerNorm over it, fc1, erf GELU, fc2 to the decoder width) -> the final merger
// (LayerNorm per patch row, then the same view and MLP). bf16 with the rounding points of the bf16 torch modules (each Linear output, each
// LayerNorm output, the GELUs, the residual sums); the rotary embedding in fp32 on the bf16 q / k with one rounding
// (apply_rotary_pos_emb_vision). head_dim is 64 (1024 / 16 at 2B): the attention kernel below runs 4 k-steps per S tile and two 32-row
// d-tiles of O, no zero padding. The index arrays (positions, interpolation taps, segment bounds) are the host's
// (facet_amd/vlm_tagger.py vision_inputs_qwen3, pinned by tests/golden/vlm3_golden.npz).
// The MLP's tanh GELU is the bf16 GEMM's epilogue (fe_gelu_fast: the tanh form with 1-ulp exp / rcp, applied to the fp32 sum before the
// one rounding; torch rounds fc1's output first). Measured against a separate pass with torch's rounding points (fc1 rounded, tanhf): the
// same embedding error (0.0234, the reference's own sdpa-vs-eager spread) and the same decoder logit errors - the epilogue stays.
#include "engine.h"
#include <algorithm>
#include <cmath>

namespace fe {

// x[r][:] = bf16(x[r][:] + bf16(sum_k w[r][k] * T[idx[r][k]][:]))   (pos_embed(idx) * weights, .sum(1) in fp32, .to(bf16), added in bf16)
__global__ void vlm3_pos_embed_kernel(bf16* __restrict__ x, const float* __restrict__ table, const int* __restrict__ idx, const float* __restrict__ wt, int N, int d) {
  const size_t total = (size_t)N * (d / 4);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / (d / 4)), c = (int)(i % (d / 4)) * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float wk = wt[(size_t)r * 4 + k];
      const float4 t = *reinterpret_cast<const float4*>(table + (size_t)idx[(size_t)r * 4 + k] * d + c);
      acc.x += t.x * wk; acc.y += t.y * wk; acc.z += t.z * wk; acc.w += t.w * wk;
    }
    const float4 a = ld4(x + (size_t)r * d + c);
    st4(x + (size_t)r * d + c, make_float4(a.x + (float)(bf16)acc.x, a.y + (float)(bf16)acc.y, a.z + (float)(bf16)acc.z, a.w + (float)(bf16)acc.w));
  }
}

// 2-D rotary embedding on the q and k thirds of the fused qkv rows (the vision tower's, hd = 64): dimension i of a head (pairs (i, i + 32))
// takes, with jj = i % 32, the row position and inv_freq[jj] for jj < 16, the column position and inv_freq[jj - 16] otherwise
__global__ void vlm3_vis_rope_kernel(const bf16* __restrict__ qkv, const int* __restrict__ pos, const float* __restrict__ inv_freq, bf16* __restrict__ q_out,
                                     bf16* __restrict__ k_out, int rows, int heads) {
  constexpr int hd = 64, half = 32, quarter = 16;
  const int dim = heads * hd;
  const size_t total = (size_t)rows * 2 * heads * half;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % half), hh = (int)((i / half) % (2 * heads)), row = (int)(i / ((size_t)half * 2 * heads));
    const int which = hh / heads, head = hh % heads;
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

// y = bf16(gelu_erf(x)) elementwise (nn.GELU() of the mergers on a bf16 tensor)
__global__ void vlm3_gelu_erf_kernel(bf16* __restrict__ x, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = ld4(x + 4 * i);
    auto f = [](float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); };
    st4(x + 4 * i, make_float4(f(a.x), f(a.y), f(a.z), f(a.w)));
  }
}

// ---- attention over packed variable-length segments (one per image), head_dim 64, non-causal ----------------------------------------------
// One workgroup = NW waves x 32 queries of one (segment, head); K / V tiles of 32 keys through LDS (V transposed on the way in), online
// softmax per lane, the exponentiated scores rounded to bf16 as the B operand of O^T += V^T P^T (the scheme of the decoder's prefill
// kernel). 64 dims: 4 k-steps of v_mfma_f32_32x32x16_bf16 per S tile, two 32-row d-tiles of O.
constexpr int V3_KS = 144;      // K tile row stride in bytes (128 + 16)
constexpr int V3_VS = 72;       // V^T tile row stride in bytes (64 + 8)
struct Vis3AttnParams {
  const bf16* q; const bf16* k; int ldqk;       // rotated q / k: [N][heads*64]
  const bf16* v; int ldv;                       // V third of the fused projection
  bf16* o; int ldo;
  const int* cu; int heads; float scale;
};
union V38 { uint4 u; fe_v4f f; };

template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void vlm3_vis_attn_kernel(const Vis3AttnParams p) {
  __shared__ __attribute__((aligned(16))) char Ks[2][32 * V3_KS];
  __shared__ __attribute__((aligned(16))) char Vs[2][64 * V3_VS];
  const bf16* const tag = nullptr;
  constexpr int NT = NW * 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int seg = blockIdx.y, head = blockIdx.z;
  const int s0 = p.cu[seg], len = p.cu[seg + 1] - s0;
  const int q0 = blockIdx.x * NW * 32;
  if (q0 >= len) return;
  const bf16* Qp = p.q + (size_t)s0 * p.ldqk + head * 64;
  const bf16* Kp = p.k + (size_t)s0 * p.ldqk + head * 64;
  const bf16* Vp = p.v + (size_t)s0 * p.ldv + head * 64;
  const int q = q0 + wave * 32 + r;
  const bool qok = q < len;
  const int qc = qok ? q : len - 1;
  V38 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s].u = *reinterpret_cast<const uint4*>(Qp + (size_t)qc * p.ldqk + 16 * s + 8 * h);
  constexpr int PIECES = (256 + NT - 1) / NT;      // 32 keys x 8 chunks of 16 B
  uint4 kr[PIECES], vr[PIECES];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int c = t + i * NT;
      if (c < 256) {
        int key = kt * 32 + (c >> 3);
        if (key > len - 1) key = len - 1;
        kr[i] = *reinterpret_cast<const uint4*>(Kp + (size_t)key * p.ldqk + (c & 7) * 8);
        vr[i] = *reinterpret_cast<const uint4*>(Vp + (size_t)key * p.ldv + (c & 7) * 8);
      }
    }
  };
  auto store_tile = [&](int buf, int kt) {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int c = t + i * NT;
      if (c < 256) {
        const int key = c >> 3, d0 = (c & 7) * 8;
        *reinterpret_cast<uint4*>(&Ks[buf][key * V3_KS + d0 * 2]) = kr[i];
        const bool live = kt * 32 + key < len;
        const unsigned w[4] = {vr[i].x, vr[i].y, vr[i].z, vr[i].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned short v = live ? (unsigned short)((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xFFFFu)) : (unsigned short)0;
          *reinterpret_cast<unsigned short*>(&Vs[buf][(d0 + e) * V3_VS + key * 2]) = v;
        }
      }
    }
  };
  fe_f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int nt = (len + 31) / 32;
  load_tile(0);
  store_tile(0, 0);
  __syncthreads();
  for (int kt = 0; kt < nt; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nt) load_tile(kt + 1);
    fe_f32x16 st;
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
    const char* kb = &Ks[buf][r * V3_KS + 16 * h];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      V38 kf;
      kf.u = *reinterpret_cast<const uint4*>(kb + 32 * s);
      st = fe_mfma16(tag, kf.f, qf[s].f, st);
    }
    const int kbase = kt * 32 + 4 * h;
    float tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = kbase + (e & 3) + 8 * (e >> 2);
      st[e] = key >= len ? -INFINITY : st[e] * p.scale;
      tmax = fmaxf(tmax, st[e]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mn = fmaxf(m, tmax);
    const float alpha = __expf(m - mn);
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) { st[e] = __expf(st[e] - mn); psum += st[e]; }
    psum += __shfl_xor(psum, 32);
    l = l * alpha + psum;
    m = mn;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
    const char* vb = &Vs[buf][r * V3_VS + 8 * h];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      V38 pf;
      pf.u = make_uint4(fe_pack2(tag, st[8 * s], st[8 * s + 1]), fe_pack2(tag, st[8 * s + 2], st[8 * s + 3]),
                        fe_pack2(tag, st[8 * s + 4], st[8 * s + 5]), fe_pack2(tag, st[8 * s + 6], st[8 * s + 7]));
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const uint2 a0 = *reinterpret_cast<const uint2*>(vb + dt * 32 * V3_VS + 32 * s), a1 = *reinterpret_cast<const uint2*>(vb + dt * 32 * V3_VS + 32 * s + 16);
        V38 v;
        v.u = make_uint4(a0.x, a0.y, a1.x, a1.y);
        o[dt] = fe_mfma16(tag, v.f, pf.f, o[dt]);
      }
    }
    if (kt + 1 < nt) store_tile(buf ^ 1, kt + 1);
    __syncthreads();
  }
  if (qok) {
    const float inv = 1.f / l;
    bf16* op = p.o + (size_t)(s0 + q) * p.ldo + head * 64;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = dt * 32 + 8 * g + 4 * h;
        st4(op + d0, make_float4(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv));
      }
  }
}

// ---- model ---------------------------------------------------------------------------------------------------------------------------------
static Vlm3MergerW build_merger3(DeviceWeights& dw, const WeightStore& ws, const std::string& P) {
  Vlm3MergerW w;
  w.ln_g = dw.upload(ws.get(P + ".norm.weight").data);
  w.ln_b = dw.upload(ws.get(P + ".norm.bias").data);
  w.fc1 = build_linear(dw, ws, P + ".linear_fc1", true);
  w.fc2 = build_linear(dw, ws, P + ".linear_fc2", true);
  return w;
}

void build_vlm3_vision(VlmModel& m, const WeightStore& ws) {
  Vlm3VisionW& v = m.vis3;
  const std::string P = "model.visual.";
  v.present = false;
  if (!ws.has(P + "patch_embed.proj.weight")) return;
  const HostTensor& pe = ws.get(P + "patch_embed.proj.weight");      // [hidden][3][t][p][p]
  FE_CHECK(pe.shape.size() == 5 && pe.shape[3] == pe.shape[4], "vlm3 vision: patch embedding shape");
  HostTensor flat;
  flat.shape = {pe.shape[0], (int64_t)(pe.numel() / (size_t)pe.shape[0])};
  flat.data = pe.data;
  v.hidden = (int)flat.shape[0]; v.patch_dim = (int)flat.shape[1]; v.patch_side = (int)pe.shape[3];
  v.heads = m.cfg.vis_heads;
  FE_CHECK(v.patch_dim % 8 == 0 && v.hidden % v.heads == 0 && v.hidden / v.heads == 64 && v.hidden % 8 == 0,
           "vlm3 vision: hidden %d over %d heads (the attention kernel is built for head_dim 64), patch vector %d", v.hidden, v.heads,
           v.patch_dim);
  v.patch = build_linear_rows(m.dw, flat, &ws.get(P + "patch_embed.proj.bias"), 0, v.hidden);
  const HostTensor& tab = ws.get(P + "pos_embed.weight");
  FE_CHECK(tab.shape.size() == 2 && tab.shape[1] == v.hidden, "vlm3 vision: position table width");
  v.n_pos = (int)tab.shape[0];
  v.pos_table = m.dw.upload(tab.data);
  v.blocks.clear();
  for (int i = 0;; ++i) {
    const std::string B = P + "blocks." + std::to_string(i);
    if (!ws.has(B + ".attn.qkv.weight")) break;
    Vlm3VisionBlockW w;
    w.qkv = build_linear(m.dw, ws, B + ".attn.qkv", true);
    w.proj = build_linear(m.dw, ws, B + ".attn.proj", true);
    w.fc1 = build_linear(m.dw, ws, B + ".mlp.linear_fc1", true);
    w.fc2 = build_linear(m.dw, ws, B + ".mlp.linear_fc2", true);
    w.n1g = m.dw.upload(ws.get(B + ".norm1.weight").data);
    w.n1b = m.dw.upload(ws.get(B + ".norm1.bias").data);
    w.n2g = m.dw.upload(ws.get(B + ".norm2.weight").data);
    w.n2b = m.dw.upload(ws.get(B + ".norm2.bias").data);
    v.blocks.push_back(w);
  }
  FE_CHECK(!v.blocks.empty(), "vlm3 vision: no blocks found");
  v.inter = v.blocks[0].fc1.Cout;
  FE_CHECK(v.inter % 8 == 0, "vlm3 vision: MLP width %d (a multiple of 8 expected)", v.inter);
  v.merger = build_merger3(m.dw, ws, P + "merger");
  v.out_hidden = v.merger.fc2.Cout;
  FE_CHECK(v.merger.fc1.Cin == 4 * v.hidden && v.out_hidden == m.hidden, "vlm3 vision: merger %d -> %d does not fit the tower (%d) / decoder (%d)", v.merger.fc1.Cin,
           v.out_hidden, v.hidden, m.hidden);
  v.ds_mergers.clear();
  for (int k = 0; ws.has(P + "deepstack_merger_list." + std::to_string(k) + ".linear_fc1.weight"); ++k)
    v.ds_mergers.push_back(build_merger3(m.dw, ws, P + "deepstack_merger_list." + std::to_string(k)));
  v.ds_blocks.assign(m.cfg.deepstack, m.cfg.deepstack + m.cfg.n_deepstack);
  FE_CHECK(v.ds_mergers.size() == v.ds_blocks.size(), "vlm3 vision: %zu DeepStack mergers in the checkpoint, %zu configured", v.ds_mergers.size(), v.ds_blocks.size());
  for (size_t k = 0; k < v.ds_blocks.size(); ++k) {
    FE_CHECK(v.ds_blocks[k] >= 0 && v.ds_blocks[k] < (int)v.blocks.size(), "vlm3 vision: DeepStack block %d of %zu", v.ds_blocks[k], v.blocks.size());
    FE_CHECK(v.ds_mergers[k].fc1.Cin == 4 * v.hidden && v.ds_mergers[k].fc2.Cout == m.hidden, "vlm3 vision: DeepStack merger %zu shape", k);
  }
  // Qwen3VLVisionRotaryEmbedding(head_dim // 2): inv_freq = 1 / 10000^(arange(0, dim, 2) / dim), dim = 32
  std::vector<float> inv(16);
  for (int i = 0; i < 16; ++i) inv[i] = 1.0f / powf(10000.0f, (float)(2 * i) / 32.0f);
  v.inv_freq = m.dw.upload(inv);
  v.present = true;
}

static inline int v3grid(size_t n, int per = 256) { size_t g = (n + per - 1) / per; return (int)(g > 262140 ? 262140 : (g ? g : 1)); }

static void vis3_linear(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, bf16* y, int ldy, int act = ACT_NONE) { linear_forward(c, w, x, ldx, M, y, ldy, act); }

// (shared with the Qwen2-VL tower, whose ln_q merger is the per-row form) a merger on the [N][d] rows: post-shuffle norm (DeepStack: LayerNorm over the 4 d-wide view) or per-row norm (final), fc1, erf GELU, fc2
void vlm_ln_merger(Ctx& c, const Vlm3MergerW& w, const bf16* x, int N, int d, bool postshuffle, bf16* n, bf16* t0, bf16* out, int out_d) {
  if (postshuffle) launch_layernorm<bf16, bf16>(x, 4 * d, n, 4 * d, w.ln_g, w.ln_b, N / 4, 4 * d, 1e-6f, c.stream);
  else launch_layernorm<bf16, bf16>(x, d, n, d, w.ln_g, w.ln_b, N, d, 1e-6f, c.stream);
  vis3_linear(c, w.fc1, n, 4 * d, N / 4, t0, 4 * d);
  hipLaunchKernelGGL(vlm3_gelu_erf_kernel, dim3(v3grid((size_t)N * d / 4)), dim3(256), 0, c.stream, t0, (size_t)N * d / 4);
  FE_HIP(hipGetLastError());
  vis3_linear(c, w.fc2, t0, 4 * d, N / 4, out, out_d);
}

void vlm3_vision_forward(Ctx& c, VlmModel& m, const float* pv, const bf16* pv_bf16, int N, const int* pos, const int* interp_idx, const float* interp_w,
                         const int* cu, int n_seg, int max_seg, bf16* out, bf16* ds) {
  Vlm3VisionW& v = m.vis3;
  FE_CHECK(v.present, "vlm: the checkpoint had no vision tower (model.visual.*)");
  FE_CHECK(N > 0 && N % 4 == 0, "vlm3 vision: %d patches (whole 2x2 merge blocks expected)", N);
  const int d = v.hidden, H = v.heads;
  const size_t mark = c.arena.mark();
  bf16* pvh = pv ? c.arena.array<bf16>((size_t)N * v.patch_dim) : nullptr;
  bf16* x = c.arena.array<bf16>((size_t)N * d);
  bf16* n = c.arena.array<bf16>((size_t)N * d);
  bf16* qkv = c.arena.array<bf16>((size_t)N * 3 * d);
  bf16* qr = c.arena.array<bf16>((size_t)N * d);
  bf16* kr = c.arena.array<bf16>((size_t)N * d);
  bf16* ao = c.arena.array<bf16>((size_t)N * d);
  bf16* br = c.arena.array<bf16>((size_t)N * d);
  bf16* hh = c.arena.array<bf16>((size_t)N * std::max(v.inter, d));
  if (pv) launch_convert(pv, pvh, (size_t)N * v.patch_dim, c.stream);      // pixel_values.to(bfloat16), as the patch embedding does
  vis3_linear(c, v.patch, pv ? (const bf16*)pvh : pv_bf16, v.patch_dim, N, x, d);
  hipLaunchKernelGGL(vlm3_pos_embed_kernel, dim3(v3grid((size_t)N * d / 4)), dim3(256), 0, c.stream, x, (const float*)v.pos_table, interp_idx, interp_w, N, d);
  FE_HIP(hipGetLastError());
  const float scale = 1.0f / sqrtf(64.f);
  const size_t ds_stride = (size_t)m.ds_cap * v.out_hidden;
  for (size_t li = 0; li < v.blocks.size(); ++li) {
    const Vlm3VisionBlockW& w = v.blocks[li];
    launch_layernorm<bf16, bf16>(x, d, n, d, w.n1g, w.n1b, N, d, 1e-6f, c.stream);
    vis3_linear(c, w.qkv, n, d, N, qkv, 3 * d);
    hipLaunchKernelGGL(vlm3_vis_rope_kernel, dim3(v3grid((size_t)N * 2 * H * 32)), dim3(256), 0, c.stream, (const bf16*)qkv, pos, (const float*)v.inv_freq, qr, kr, N, H);
    Vis3AttnParams ap{qr, kr, d, qkv + 2 * d, 3 * d, ao, d, cu, H, scale};
    if (max_seg <= 64) hipLaunchKernelGGL(vlm3_vis_attn_kernel<2>, dim3((max_seg + 63) / 64, n_seg, H), dim3(128), 0, c.stream, ap);
    else hipLaunchKernelGGL(vlm3_vis_attn_kernel<4>, dim3((max_seg + 127) / 128, n_seg, H), dim3(256), 0, c.stream, ap);
    FE_HIP(hipGetLastError());
    vis3_linear(c, w.proj, ao, d, N, br, d);
    vlm_add(c, x, br, (size_t)N * d);
    launch_layernorm<bf16, bf16>(x, d, n, d, w.n2g, w.n2b, N, d, 1e-6f, c.stream);
    vis3_linear(c, w.fc1, n, d, N, hh, v.inter, ACT_GELU);      // gelu_pytorch_tanh as the GEMM's epilogue
    vis3_linear(c, w.fc2, hh, v.inter, N, br, d);
    vlm_add(c, x, br, (size_t)N * d);
    const auto it = std::find(v.ds_blocks.begin(), v.ds_blocks.end(), (int)li);
    if (it != v.ds_blocks.end() && ds) {
      const size_t k = (size_t)(it - v.ds_blocks.begin());
      const size_t mm = c.arena.mark();
      bf16* n4 = c.arena.array<bf16>((size_t)N * d);
      bf16* t4 = c.arena.array<bf16>((size_t)N * d);
      vlm_ln_merger(c, v.ds_mergers[k], x, N, d, true, n4, t4, ds + k * ds_stride, v.out_hidden);
      c.arena.rewind(mm);
    }
  }
  bf16* t0 = c.arena.array<bf16>((size_t)N * d);
  vlm_ln_merger(c, v.merger, x, N, d, false, n, t0, out, v.out_hidden);
  c.arena.rewind(mark);
}

}  // namespace fe
