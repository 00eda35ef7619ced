// VLM composition analyzer, Qwen2-VL: the vision tower - pixel patches in, merged image embeddings out.
//
// Stands behind `Qwen2VLForConditionalGeneration.get_image_features` = `model.visual(pixel_values, grid_thw).pooler_output` (transformers
// Qwen2VisionTransformerPretrainedModel [modeling_qwen2_vl.py]; reference models/vlm_composition.py runs it inside `generate`): Conv3d
// patch embedding without bias (a [n, 1176] x [1176, hidden] product: 14 x 14 patches, 2 frames), no position table -> `depth` blocks
// { x += proj(attn(rope2d(qkv(LayerNorm(x))))) ; x += fc2(quick_gelu(fc1(LayerNorm(x)))) } with attention over each whole image in EVERY
// block (no windows; rows stay in the 2x2-block-major order of the processor, so nothing is gathered) -> the patch merger (LayerNorm ln_q
// per patch row, 4 rows viewed as one, Linear - erf GELU - Linear to the decoder width). bf16 with the rounding points of the bf16 torch
// modules (each Linear output, each LayerNorm output, the residual sums, the merger's GELU); the rotary embedding in fp32 on the bf16
// q / k with one rounding (apply_rotary_pos_emb_vision). head_dim is 80 (1280 / 16 at 2B).
// Every piece but the activation is shared with the other two towers: the head_dim-80 rope and segment attention of the Qwen2.5-VL tower
// (vlm_vis_rope80 / vlm_vis_attention80, model_vlm_vision.hip), the LayerNorm and the LayerNorm merger of the Qwen3-VL one
// (launch_layernorm, vlm_ln_merger, model_vlm3_vision.hip), the residual sum of the decoder (vlm_add).
// QuickGELU, x * sigmoid(1.702 x): torch computes it on fc1's bf16 output with a rounding after the scale, the sigmoid and the product
// (three roundings after fc1's own). Two forms are built: the bf16 GEMM's epilogue on the fp32 sum (ACT_QUICKGELU: bare v_exp / v_rcp, one
// rounding) and a separate pass with torch's rounding points (vlm2_quick_gelu_kernel; FE_VLM2_QGELU_PASS=1 selects it, an A/B hook).
// Embedding error against tests/golden/vlm2_golden.npz (grids 10 x 12 and 6 x 6, max |difference|; the reference's own sdpa-vs-eager
// spread there is 0.0278, the test's bound 0.0834): unmeasured for both forms, so the choice between them is open (DESIGN.md section 4
// states the rule that closes it). The epilogue is the default; tests/test_vlm2_gpu.py prints the error of the form in use.
#include "engine.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace fe {

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

void build_vlm2_vision(VlmModel& m, const WeightStore& ws) {
  Vlm2VisionW& v = m.vis2;
  const std::string P = "model.visual.";
  v.present = false;
  if (!ws.has(P + "patch_embed.proj.weight")) return;
  const HostTensor& pe = ws.get(P + "patch_embed.proj.weight");      // [hidden][3][t][p][p]
  FE_CHECK(pe.shape.size() == 5 && pe.shape[3] == 14 && pe.shape[4] == 14, "vlm2 vision: patch embedding shape (14-pixel patches expected)");
  HostTensor flat;
  flat.shape = {pe.shape[0], (int64_t)(pe.numel() / (size_t)pe.shape[0])};
  flat.data = pe.data;
  v.hidden = (int)flat.shape[0]; v.patch_dim = (int)flat.shape[1];
  v.heads = m.cfg.vis_heads;
  FE_CHECK(v.patch_dim % 8 == 0 && v.hidden % v.heads == 0 && v.hidden / v.heads == 80 && v.hidden % 32 == 0,
           "vlm2 vision: hidden %d over %d heads (the attention kernel is built for head_dim 80), patch vector %d", v.hidden, v.heads, v.patch_dim);
  FE_CHECK(!ws.has(P + "patch_embed.proj.bias"), "vlm2 vision: the patch embedding carries a bias");
  v.patch = build_linear_rows(m.dw, flat, nullptr, 0, v.hidden);
  v.blocks.clear();
  for (int i = 0;; ++i) {
    const std::string B = P + "blocks." + std::to_string(i);
    if (!ws.has(B + ".attn.qkv.weight")) break;
    Vlm3VisionBlockW w;
    w.qkv = build_linear(m.dw, ws, B + ".attn.qkv", true);
    w.proj = build_linear(m.dw, ws, B + ".attn.proj", true);
    w.fc1 = build_linear(m.dw, ws, B + ".mlp.fc1", true);
    w.fc2 = build_linear(m.dw, ws, B + ".mlp.fc2", true);
    w.n1g = m.dw.upload(ws.get(B + ".norm1.weight").data);
    w.n1b = m.dw.upload(ws.get(B + ".norm1.bias").data);
    w.n2g = m.dw.upload(ws.get(B + ".norm2.weight").data);
    w.n2b = m.dw.upload(ws.get(B + ".norm2.bias").data);
    v.blocks.push_back(w);
  }
  FE_CHECK(!v.blocks.empty(), "vlm2 vision: no blocks found");
  v.inter = v.blocks[0].fc1.Cout;
  FE_CHECK(v.inter % 8 == 0, "vlm2 vision: MLP width %d (a multiple of 8 expected)", v.inter);
  v.merger.ln_g = m.dw.upload(ws.get(P + "merger.ln_q.weight").data);
  v.merger.ln_b = m.dw.upload(ws.get(P + "merger.ln_q.bias").data);
  v.merger.fc1 = build_linear(m.dw, ws, P + "merger.mlp.0", true);
  v.merger.fc2 = build_linear(m.dw, ws, P + "merger.mlp.2", true);
  v.out_hidden = v.merger.fc2.Cout;
  FE_CHECK(v.merger.fc1.Cin == 4 * v.hidden && v.out_hidden == m.hidden, "vlm2 vision: merger %d -> %d does not fit the tower (%d) / decoder (%d)", v.merger.fc1.Cin,
           v.out_hidden, v.hidden, m.hidden);
  v.inv_freq = vlm_vis_inv_freq80(m.dw);
  v.present = true;
}

void vlm2_vision_forward(Ctx& c, VlmModel& m, const float* pv, const bf16* pv_bf16, int N, const int* pos, const int* cu, int n_seg, int max_seg, bf16* out) {
  Vlm2VisionW& v = m.vis2;
  FE_CHECK(v.present, "vlm: the checkpoint had no vision tower (model.visual.*)");
  FE_CHECK(N > 0 && N % 4 == 0, "vlm2 vision: %d patches (whole 2x2 merge blocks expected)", N);
  static const bool gelu_pass = getenv("FE_VLM2_QGELU_PASS") != nullptr;      // A/B hook: torch's rounding points instead of the epilogue
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
  for (size_t li = 0; li < v.blocks.size(); ++li) {
    const Vlm3VisionBlockW& w = v.blocks[li];
    launch_layernorm<bf16, bf16>(x, d, n, d, w.n1g, w.n1b, N, d, 1e-6f, c.stream);
    linear_forward(c, w.qkv, n, d, N, qkv, 3 * d, ACT_NONE);
    vlm_vis_rope80(c, qkv, pos, v.inv_freq, qr, kr, N, H);
    vlm_vis_attention80(c, qr, kr, qkv, ao, cu, n_seg, max_seg, H);
    linear_forward(c, w.proj, ao, d, N, br, d, ACT_NONE);
    vlm_add(c, x, br, (size_t)N * d);
    launch_layernorm<bf16, bf16>(x, d, n, d, w.n2g, w.n2b, N, d, 1e-6f, c.stream);
    if (gelu_pass) {
      linear_forward(c, w.fc1, n, d, N, hh, v.inter, ACT_NONE);
      const size_t n4 = (size_t)N * v.inter / 4;
      hipLaunchKernelGGL(vlm2_quick_gelu_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 262140)), dim3(256), 0, c.stream, hh, n4);
      FE_HIP(hipGetLastError());
    } else {
      linear_forward(c, w.fc1, n, d, N, hh, v.inter, ACT_QUICKGELU);      // QuickGELU as the GEMM's epilogue
    }
    linear_forward(c, w.fc2, hh, v.inter, N, br, d, ACT_NONE);
    vlm_add(c, x, br, (size_t)N * d);
  }
  bf16* t0 = c.arena.array<bf16>((size_t)N * d);
  vlm_ln_merger(c, v.merger, x, N, d, false, n, t0, out, v.out_hidden);
  c.arena.rewind(mark);
}

}  // namespace fe
