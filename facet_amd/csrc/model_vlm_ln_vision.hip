// The LayerNorm vision towers of the VLM families: Qwen2-VL (the composition analyzer) and Qwen3-VL (the tagger) - pixel patches in,
// merged image embeddings (and, for Qwen3-VL, the DeepStack feature blocks) out. One struct, one builder, one forward; the families differ
// in the tensor names, head_dim, the MLP activation and the two optional pieces (position table, DeepStack).
//
// Stands behind `get_image_features` of transformers' Qwen2VisionTransformerPretrainedModel [modeling_qwen2_vl.py] and Qwen3VLVisionModel
// [modeling_qwen3_vl.py]: Conv3d patch embedding (a [n, patch_dim] x [patch_dim, hidden] product; Qwen2: 14 x 14 patches, 2 frames, no
// bias; Qwen3: 16 x 16 patches with bias) (+ Qwen3: the learned position table bilinearly resampled to each image's grid, align_corners=True:
// four taps per patch with fp32 weights, summed in fp32, rounded to bf16, added in bf16) -> `depth` blocks
// { x += proj(attn(rope2d(qkv(LayerNorm(x))))) ; x += fc2(act(fc1(LayerNorm(x)))) } with attention over each whole image in every block (no
// windows; rows stay in the 2x2-block-major order of the processor, so nothing is gathered) (-> Qwen3: after the blocks named in
// deepstack_visual_indexes a DeepStack merger: 4 rows viewed as one row of 4 hidden, LayerNorm over it, fc1, erf GELU, fc2 to the decoder
// width) -> the final merger (LayerNorm per patch row, then the same view and MLP). bf16 with the rounding points of the bf16 torch modules
// (each Linear output, each LayerNorm output, the residual sums, the mergers' GELU); the rotary embedding in fp32 on the bf16 q / k with
// one rounding (apply_rotary_pos_emb_vision). head_dim is 80 (Qwen2: 1280 / 16) or 64 (Qwen3: 1024 / 16 at 2B): rope, segment attention and
// the erf GELU are those of the Qwen2.5-VL tower (vlm_vis_rope / vlm_vis_attention / vlm_gelu_erf, model_vlm_vision.hip). The index arrays
// (positions, interpolation taps, segment bounds) are the host's (facet_amd/vlm_tagger.py vision_inputs_qwen2 / vision_inputs_qwen3,
// pinned by tests/golden/vlm2_golden.npz / vlm3_golden.npz).
// The MLP activation is the bf16 GEMM's epilogue, applied to the fp32 sum before the one rounding (torch rounds fc1's output first):
//  * Qwen3, gelu_pytorch_tanh (ACT_GELU -> fe_gelu_fast: the tanh form with 1-ulp exp / rcp). Measured against a separate pass with torch's
//    rounding points (fc1 rounded, tanhf): the same embedding error (0.0234, the reference's own sdpa-vs-eager spread) and the same decoder
//    logit errors - the epilogue stays.
//  * Qwen2, QuickGELU x * sigmoid(1.702 x): torch rounds after fc1, the scale, the sigmoid and the product. Two forms are built: the
//    epilogue (ACT_QUICKGELU: bare v_exp / v_rcp, one rounding) and a separate pass with torch's rounding points (vlm2_quick_gelu_kernel;
//    FE_VLM2_QGELU_PASS=1 selects it, an A/B hook). Embedding error against tests/golden/vlm2_golden.npz (grids 10 x 12 and 6 x 6, max
//    |difference|; the reference's own sdpa-vs-eager spread there is 0.0278, the test's bound 0.0834): unmeasured for both forms, so the
//    choice between them is open (DESIGN.md section 4 states the rule that closes it). The epilogue is the default;
//    tests/test_vlm2_gpu.py prints the error of the form in use.
#include "engine.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

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

// y = bf16(x * bf16(sigmoid(bf16(1.702 x)))) elementwise: QuickGELUActivation on a bf16 tensor, torch's rounding points
__global__ void vlm2_quick_gelu_kernel(bf16* __restrict__ x, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = ld4(x + 4 * i);
    auto f = [](float v) {
      const float s = (float)(bf16)(1.702f * v);
      return v * (float)(bf16)(1.f / (1.f + expf(-s)));
    };
    st4(x + 4 * i, make_float4(f(a.x), f(a.y), f(a.z), f(a.w)));
  }
}

// ---- model ---------------------------------------------------------------------------------------------------------------------------------
// what the two checkpoints call the same tensors, and the geometry each family is built for
struct LnTowerFamily {
  const char* tag;                                      // prefix of the build errors
  int head_dim, act, hidden_mult;
  bool patch14, patch_bias, pos_table;
  const char *fc1, *fc2;                                // under blocks.i
  const char *merger_norm, *merger_fc1, *merger_fc2;    // under merger (and deepstack_merger_list.k)
};
static const LnTowerFamily QWEN2_TOWER = {"vlm2", 80, ACT_QUICKGELU, 32, true, false, false, ".mlp.fc1", ".mlp.fc2", ".ln_q", ".mlp.0", ".mlp.2"};
static const LnTowerFamily QWEN3_TOWER = {"vlm3", 64, ACT_GELU, 8, false, true, true, ".mlp.linear_fc1", ".mlp.linear_fc2", ".norm", ".linear_fc1", ".linear_fc2"};

static VlmLnMergerW build_ln_merger(DeviceWeights& dw, const WeightStore& ws, const std::string& P, const LnTowerFamily& F) {
  VlmLnMergerW w;
  w.ln_g = dw.upload(ws.get(P + F.merger_norm + ".weight").data);
  w.ln_b = dw.upload(ws.get(P + F.merger_norm + ".bias").data);
  w.fc1 = build_linear(dw, ws, P + F.merger_fc1, true);
  w.fc2 = build_linear(dw, ws, P + F.merger_fc2, true);
  return w;
}

void build_vlm_ln_vision(VlmModel& m, const WeightStore& ws) {
  const LnTowerFamily& F = m.cfg.qwen3 ? QWEN3_TOWER : QWEN2_TOWER;
  VlmLnVisionW& v = m.vis_ln;
  const std::string P = "model.visual.";
  v = VlmLnVisionW();
  if (!ws.has(P + "patch_embed.proj.weight")) return;
  const HostTensor& pe = ws.get(P + "patch_embed.proj.weight");      // [hidden][3][t][p][p]
  if (F.patch14) FE_CHECK(pe.shape.size() == 5 && pe.shape[3] == 14 && pe.shape[4] == 14, "%s vision: patch embedding shape (14-pixel patches expected)", F.tag);
  else FE_CHECK(pe.shape.size() == 5 && pe.shape[3] == pe.shape[4], "%s vision: patch embedding shape", F.tag);
  HostTensor flat;
  flat.shape = {pe.shape[0], (int64_t)(pe.numel() / (size_t)pe.shape[0])};
  flat.data = pe.data;
  v.hidden = (int)flat.shape[0]; v.patch_dim = (int)flat.shape[1]; v.patch_side = (int)pe.shape[3];
  v.heads = m.cfg.vis_heads; v.head_dim = F.head_dim; v.act = F.act;
  FE_CHECK(v.patch_dim % 8 == 0 && v.hidden % v.heads == 0 && v.hidden / v.heads == F.head_dim && v.hidden % F.hidden_mult == 0,
           "%s vision: hidden %d over %d heads (the attention kernel is built for head_dim %d), patch vector %d", F.tag, v.hidden, v.heads, F.head_dim, v.patch_dim);
  if (!F.patch_bias) FE_CHECK(!ws.has(P + "patch_embed.proj.bias"), "%s vision: the patch embedding carries a bias", F.tag);
  v.patch = build_linear_rows(m.dw, flat, F.patch_bias ? &ws.get(P + "patch_embed.proj.bias") : nullptr, 0, v.hidden);
  if (F.pos_table) {
    const HostTensor& tab = ws.get(P + "pos_embed.weight");
    FE_CHECK(tab.shape.size() == 2 && tab.shape[1] == v.hidden, "%s vision: position table width", F.tag);
    v.n_pos = (int)tab.shape[0];
    v.pos_table = m.dw.upload(tab.data);
  }
  for (int i = 0;; ++i) {
    const std::string B = P + "blocks." + std::to_string(i);
    if (!ws.has(B + ".attn.qkv.weight")) break;
    VlmLnBlockW w;
    w.qkv = build_linear(m.dw, ws, B + ".attn.qkv", true);
    w.proj = build_linear(m.dw, ws, B + ".attn.proj", true);
    w.fc1 = build_linear(m.dw, ws, B + F.fc1, true);
    w.fc2 = build_linear(m.dw, ws, B + F.fc2, true);
    w.n1g = m.dw.upload(ws.get(B + ".norm1.weight").data);
    w.n1b = m.dw.upload(ws.get(B + ".norm1.bias").data);
    w.n2g = m.dw.upload(ws.get(B + ".norm2.weight").data);
    w.n2b = m.dw.upload(ws.get(B + ".norm2.bias").data);
    v.blocks.push_back(w);
  }
  FE_CHECK(!v.blocks.empty(), "%s vision: no blocks found", F.tag);
  v.inter = v.blocks[0].fc1.Cout;
  FE_CHECK(v.inter % 8 == 0, "%s vision: MLP width %d (a multiple of 8 expected)", F.tag, v.inter);
  v.merger = build_ln_merger(m.dw, ws, P + "merger", F);
  v.out_hidden = v.merger.fc2.Cout;
  FE_CHECK(v.merger.fc1.Cin == 4 * v.hidden && v.out_hidden == m.hidden, "%s vision: merger %d -> %d does not fit the tower (%d) / decoder (%d)", F.tag, v.merger.fc1.Cin,
           v.out_hidden, v.hidden, m.hidden);
  for (int k = 0; ws.has(P + "deepstack_merger_list." + std::to_string(k) + F.merger_fc1 + ".weight"); ++k)
    v.ds_mergers.push_back(build_ln_merger(m.dw, ws, P + "deepstack_merger_list." + std::to_string(k), F));
  v.ds_blocks.assign(m.cfg.deepstack, m.cfg.deepstack + m.cfg.n_deepstack);
  FE_CHECK(v.ds_mergers.size() == v.ds_blocks.size(), "%s vision: %zu DeepStack mergers in the checkpoint, %zu configured", F.tag, v.ds_mergers.size(), v.ds_blocks.size());
  for (size_t k = 0; k < v.ds_blocks.size(); ++k) {
    FE_CHECK(v.ds_blocks[k] >= 0 && v.ds_blocks[k] < (int)v.blocks.size(), "%s vision: DeepStack block %d of %zu", F.tag, v.ds_blocks[k], v.blocks.size());
    FE_CHECK(v.ds_mergers[k].fc1.Cin == 4 * v.hidden && v.ds_mergers[k].fc2.Cout == m.hidden, "%s vision: DeepStack merger %zu shape", F.tag, k);
  }
  v.inv_freq = vlm_vis_inv_freq(m.dw, v.head_dim);
  v.present = true;
}

// a merger on the [N][d] rows: post-shuffle norm (DeepStack: LayerNorm over the 4 d-wide view) or per-row norm (final), fc1, erf GELU, fc2;
// n / t0: [N][d] scratch
static void ln_merger(Ctx& c, const VlmLnMergerW& w, const bf16* x, int N, int d, bool postshuffle, bf16* n, bf16* t0, bf16* out, int out_d) {
  if (postshuffle) launch_layernorm<bf16, bf16>(x, 4 * d, n, 4 * d, w.ln_g, w.ln_b, N / 4, 4 * d, 1e-6f, c.stream);
  else launch_layernorm<bf16, bf16>(x, d, n, d, w.ln_g, w.ln_b, N, d, 1e-6f, c.stream);
  linear_forward(c, w.fc1, n, 4 * d, N / 4, t0, 4 * d, ACT_NONE);
  vlm_gelu_erf(c, t0, (size_t)N * d);
  linear_forward(c, w.fc2, t0, 4 * d, N / 4, out, out_d, ACT_NONE);
}

void vlm_ln_vision_forward(Ctx& c, VlmModel& m, const float* pv, const bf16* pv_bf16, int N, const int* pos, const int* interp_idx, const float* interp_w,
                           const int* cu, int n_seg, int max_seg, bf16* out, bf16* ds) {
  VlmLnVisionW& v = m.vis_ln;
  FE_CHECK(v.present, "vlm: the checkpoint had no vision tower (model.visual.*)");
  FE_CHECK(N > 0 && N % 4 == 0, "%s vision: %d patches (whole 2x2 merge blocks expected)", m.cfg.qwen3 ? "vlm3" : "vlm2", N);
  static const bool gelu_pass = getenv("FE_VLM2_QGELU_PASS") != nullptr;      // A/B hook (Qwen2-VL): torch's rounding points instead of the epilogue
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
  linear_forward(c, v.patch, pv ? (const bf16*)pvh : pv_bf16, v.patch_dim, N, x, d, ACT_NONE);
  if (interp_idx) {
    hipLaunchKernelGGL(vlm3_pos_embed_kernel, dim3(grid_n((size_t)N * d / 4)), dim3(256), 0, c.stream, x, (const float*)v.pos_table, interp_idx, interp_w, N, d);
    FE_HIP(hipGetLastError());
  }
  const size_t ds_stride = (size_t)m.ds_cap * v.out_hidden;
  for (size_t li = 0; li < v.blocks.size(); ++li) {
    const VlmLnBlockW& w = v.blocks[li];
    launch_layernorm<bf16, bf16>(x, d, n, d, w.n1g, w.n1b, N, d, 1e-6f, c.stream);
    linear_forward(c, w.qkv, n, d, N, qkv, 3 * d, ACT_NONE);
    vlm_vis_rope(c, v.head_dim, qkv, pos, v.inv_freq, qr, kr, N, H);
    vlm_vis_attention(c, v.head_dim, qr, kr, qkv, ao, cu, n_seg, max_seg, H);
    linear_forward(c, w.proj, ao, d, N, br, d, ACT_NONE);
    vlm_add(c, x, br, (size_t)N * d);
    launch_layernorm<bf16, bf16>(x, d, n, d, w.n2g, w.n2b, N, d, 1e-6f, c.stream);
    if (v.act == ACT_QUICKGELU && gelu_pass) {
      linear_forward(c, w.fc1, n, d, N, hh, v.inter, ACT_NONE);
      const size_t n4 = (size_t)N * v.inter / 4;
      hipLaunchKernelGGL(vlm2_quick_gelu_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 262140)), dim3(256), 0, c.stream, hh, n4);
      FE_HIP(hipGetLastError());
    } else {
      linear_forward(c, w.fc1, n, d, N, hh, v.inter, v.act);      // the activation as the GEMM's epilogue
    }
    linear_forward(c, w.fc2, hh, v.inter, N, br, d, ACT_NONE);
    vlm_add(c, x, br, (size_t)N * d);
    const auto it = std::find(v.ds_blocks.begin(), v.ds_blocks.end(), (int)li);
    if (it != v.ds_blocks.end() && ds) {
      const size_t k = (size_t)(it - v.ds_blocks.begin());
      const size_t mm = c.arena.mark();
      bf16* n4 = c.arena.array<bf16>((size_t)N * d);
      bf16* t4 = c.arena.array<bf16>((size_t)N * d);
      ln_merger(c, v.ds_mergers[k], x, N, d, true, n4, t4, ds + k * ds_stride, v.out_hidden);
      c.arena.rewind(mm);
    }
  }
  bf16* t0 = c.arena.array<bf16>((size_t)N * d);
  ln_merger(c, v.merger, x, N, d, false, n, t0, out, v.out_hidden);
  c.arena.rewind(mark);
}

}  // namespace fe
