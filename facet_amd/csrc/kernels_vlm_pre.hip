// VLM tagger image preprocessing after the resample: Qwen2-VL's image processor (transformers Qwen2VLImageProcessorPil: rescale by 1/255,
// normalise by the CLIP mean / std, patchify with the temporal frame duplicated) on the GPU. The resample itself is the PIL-exact
// separable one of kernels_resize.hip (bicubic); the index arithmetic (smart_resize, grids) stays on the host.
//
// Values: the processor computes float32(float64(u) * (1/255)), then float32 (x - mean) / std. A channel's value depends on its uint8 only,
// so the host evaluates that arithmetic once per (channel, u) into lut [3][256] and the kernel is a gather: bit-exact by construction.
#include "engine.h"

namespace fe {

// One thread per (patch row, channel, y, x) of the output: the pixel is read once and written to both temporal copies (P = patch side:
// 14 for Qwen2.5-VL, 16 for Qwen3-VL).
//   row = ((bh * (gw / 2) + bw) * 2 + i) * 2 + j  ->  patch (ph, pw) = (2 bh + i, 2 bw + j)
//   col = ((c * 2 + t) * P + y) * P + x           ->  pixel (P ph + y, P pw + x), channel c
template <int P>
__global__ void vlm_patchify_kernel(const uint8_t* __restrict__ img, int ow, int gw, const float* __restrict__ lut, int rows,
                                    bf16* __restrict__ out_h, float* __restrict__ out_f) {
  constexpr int PP = P * P;
  const size_t total = (size_t)rows * 3 * PP;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int yx = (int)(i % PP), c = (int)((i / PP) % 3), row = (int)(i / (3 * PP));
    const int y = yx / P, x = yx - y * P;
    const int j = row & 1, ii = (row >> 1) & 1, blk = row >> 2, bw = blk % (gw / 2), bh = blk / (gw / 2);
    const int py = (2 * bh + ii) * P + y, px = (2 * bw + j) * P + x;
    const float v = lut[c * 256 + img[((size_t)py * ow + px) * 3 + c]];
    const size_t o0 = (size_t)row * (6 * PP) + (size_t)(c * 2) * PP + yx, o1 = o0 + PP;
    const bf16 h = (bf16)v;      // pixel_values.to(bfloat16), as the patch embedding does
    out_h[o0] = h; out_h[o1] = h;
    if (out_f) { out_f[o0] = v; out_f[o1] = v; }
  }
}

void vlm_patchify(Ctx& c, const uint8_t* img, int oh, int ow, const float* lut, bf16* out_bf16, float* out_f32) {
  FE_CHECK(oh > 0 && ow > 0 && oh % 28 == 0 && ow % 28 == 0, "vlm preprocess: resized size %dx%d is not a multiple of 28", oh, ow);
  const int gw = ow / 14, rows = (oh / 14) * gw;
  const size_t total = (size_t)rows * 588;
  size_t g = (total + 255) / 256;
  if (g > 65535 * 4) g = 65535 * 4;
  hipLaunchKernelGGL(vlm_patchify_kernel<14>, dim3((unsigned)g), dim3(256), 0, c.stream, img, ow, gw, lut, rows, out_bf16, out_f32);
  FE_HIP(hipGetLastError());
}
void vlm_patchify16(Ctx& c, const uint8_t* img, int oh, int ow, const float* lut, bf16* out_bf16, float* out_f32) {
  FE_CHECK(oh > 0 && ow > 0 && oh % 32 == 0 && ow % 32 == 0, "vlm preprocess: resized size %dx%d is not a multiple of 32", oh, ow);
  const int gw = ow / 16, rows = (oh / 16) * gw;
  const size_t total = (size_t)rows * 768;
  size_t g = (total + 255) / 256;
  if (g > 65535 * 4) g = 65535 * 4;
  hipLaunchKernelGGL(vlm_patchify_kernel<16>, dim3((unsigned)g), dim3(256), 0, c.stream, img, ow, gw, lut, rows, out_bf16, out_f32);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
