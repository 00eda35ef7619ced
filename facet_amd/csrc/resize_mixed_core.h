// PIL-exact 224 x 224 crops from a LIST of images of any sizes: one descriptor per image, one launch per resampling pass
// (kernels_resize_mixed.hip). Shared by host and device: the per-sample arithmetic below is what the kernels run, and
// tests/native/resize_mixed_harness.cpp runs the same functions on the CPU from the same descriptors and table pool.
//
// Geometry = preprocess_square224 (capi_models.hip): CLIP = bicubic, shorter side to 224, py_round_half_even centre crop (open_clip's eval
// transform); SAMP = bilinear to 224 x 224 (torchvision Resize((224, 224))). Arithmetic = libImaging/Resample.c: 22-bit fixed-point
// coefficients, int32 accumulation from 1 << 21, a uint8 intermediate between the horizontal and the vertical pass.
//
// Only what the crop needs is computed, which gives the same bytes: the horizontal pass makes the 224 output columns of the crop for the
// source rows the vertical pass reads (PIL restricts its horizontal pass to those rows too), so an image's intermediate is [nr][224][3]
// whatever its width, and its two tables hold the 224 output samples of the crop window only.
//
// The table pool is one int32 array per call: for each distinct (input size, output size, filter, first output sample) one block of
// 224 x ksize coefficients and one of 224 x 2 bounds. Descriptors address it by int32 offsets, so the pool can live anywhere in
// call-scoped memory and nothing is cached per size.
#pragma once
#include "resize_coeffs.h"
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FE_MHD __host__ __device__ __forceinline__
#else
#define FE_MHD inline
#endif

namespace fe {

constexpr int kMixedSide = 224;
enum MixedMode : int { MIXED_CLIP = 0, MIXED_SAMP = 1 };

struct MixedDesc {          // 72 bytes
  const uint8_t* src;       // [h][w][3] RGB, any alignment
  int32_t h, w;
  int32_t oh, ow;           // size after the resize
  int32_t y0, x0;           // origin of the 224 x 224 crop in the resized image
  int32_t r0, nr;           // source rows [r0, r0 + nr) feed the vertical pass (the crop rows themselves when there is none)
  int32_t kh, bh, ksize_h;  // pool offsets of the horizontal coefficients [224][ksize_h] and bounds [224][2]; ksize_h = 0: no horizontal pass
  int32_t kv, bv, ksize_v;  // the same for the vertical pass
  uint32_t inter;           // byte offset of the [nr][224][3] intermediate in the launch's scratch (unused without a horizontal pass)
  int32_t slot;             // crop slot of the launch's output this image goes to
};

// Horizontal pass: intermediate row r (source row r0 + r), crop column xx.
FE_MHD void mixed_h_sample(const MixedDesc& d, const int32_t* pool, int r, int xx, uint8_t out[3]) {
  const int xmin = pool[d.bh + xx * 2], xmax = pool[d.bh + xx * 2 + 1];
  const int32_t* k = pool + d.kh + (size_t)xx * d.ksize_h;
  const uint8_t* p = d.src + ((size_t)(d.r0 + r) * d.w + xmin) * 3;
  int s0 = 1 << (kResizePrecisionBits - 1), s1 = s0, s2 = s0;
  for (int x = 0; x < xmax; ++x) {
    const int c = k[x];
    s0 += p[x * 3 + 0] * c; s1 += p[x * 3 + 1] * c; s2 += p[x * 3 + 2] * c;
  }
  out[0] = pil_clip8(s0); out[1] = pil_clip8(s1); out[2] = pil_clip8(s2);
}

// Vertical pass: crop pixel (yy, x). inter = this image's intermediate; read only when there was a horizontal pass, else the source
// itself is read at the crop's columns.
FE_MHD void mixed_v_sample(const MixedDesc& d, const int32_t* pool, const uint8_t* inter, int yy, int x, uint8_t out[3]) {
  const uint8_t* base;
  size_t stride;
  int row0;
  if (d.ksize_h) { base = inter + (size_t)x * 3; stride = (size_t)kMixedSide * 3; row0 = d.r0; }
  else { base = d.src + (size_t)(x + d.x0) * 3; stride = (size_t)d.w * 3; row0 = 0; }
  if (!d.ksize_v) {
    const uint8_t* q = base + (size_t)(d.y0 + yy - row0) * stride;
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
    return;
  }
  const int ymin = pool[d.bv + yy * 2], ymax = pool[d.bv + yy * 2 + 1];
  const int32_t* k = pool + d.kv + (size_t)yy * d.ksize_v;
  const uint8_t* p = base + (size_t)(ymin - row0) * stride;
  int s0 = 1 << (kResizePrecisionBits - 1), s1 = s0, s2 = s0;
  for (int y = 0; y < ymax; ++y) {
    const int c = k[y];
    const uint8_t* q = p + (size_t)y * stride;
    s0 += q[0] * c; s1 += q[1] * c; s2 += q[2] * c;
  }
  out[0] = pil_clip8(s0); out[1] = pil_clip8(s1); out[2] = pil_clip8(s2);
}

// launch_u8_to_nhwc4_norm's arithmetic on one sample
FE_MHD float mixed_norm(uint8_t v, float mean, float stdv) { return ((float)v / 255.0f - mean) / stdv; }

}  // namespace fe

// ---- host side: descriptors and the table pool ------------------------------------------------------------------------------------
#include "mixed_list.h"
#include <algorithm>
#include <vector>

namespace fe {

inline int mixed_round_half_even(double v) {
  const double f = std::floor(v);
  const double d = v - f;
  if (d > 0.5) return (int)f + 1;
  if (d < 0.5) return (int)f;
  return ((long long)f % 2 == 0) ? (int)f : (int)f + 1;
}

// Builds the descriptors and the table pool of one call on the host. Tables are shared between images: a second image of a shape adds
// nothing to the pool.
class MixedTables : public mixed_list::PilTablePool {
 public:
  // Geometry and tables of an h x w image under `mode`; src / inter / slot are the caller's. false: a size the path does not take.
  bool describe(int mode, int h, int w, MixedDesc& d) {
    if (h < 1 || w < 1 || (mode != MIXED_CLIP && mode != MIXED_SAMP)) return false;
    d = MixedDesc();
    d.h = h; d.w = w; d.oh = kMixedSide; d.ow = kMixedSide;
    const int filter = mode == MIXED_CLIP ? kFilterBicubic : kFilterBilinear;
    if (mode == MIXED_CLIP) {   // torchvision Resize(224) + CenterCrop(224)
      if (w <= h) d.oh = (int)(224.0 * h / w); else d.ow = (int)(224.0 * w / h);
      d.y0 = mixed_round_half_even((d.oh - kMixedSide) / 2.0);
      d.x0 = mixed_round_half_even((d.ow - kMixedSide) / 2.0);
    }
    if (d.ow != w && !add(w, 0.0f, (float)w, d.ow, filter, d.x0, kMixedSide, d.kh, d.bh, d.ksize_h)) return false;
    if (d.oh != h) {
      if (!add(h, 0.0f, (float)h, d.oh, filter, d.y0, kMixedSide, d.kv, d.bv, d.ksize_v)) return false;
      const int32_t* b = pool.data() + d.bv;
      int lo = b[0], hi = b[0] + b[1];
      for (int yy = 1; yy < kMixedSide; ++yy) { lo = std::min(lo, b[yy * 2]); hi = std::max(hi, b[yy * 2] + b[yy * 2 + 1]); }
      d.r0 = lo; d.nr = hi - lo;
    } else {
      d.r0 = d.y0; d.nr = kMixedSide;
    }
    return d.r0 >= 0 && d.nr >= 1 && d.r0 + d.nr <= h && d.x0 >= 0 && d.x0 + kMixedSide <= d.ow && d.y0 >= 0 && d.y0 + kMixedSide <= d.oh;
  }
  static size_t inter_bytes(const MixedDesc& d) { return d.ksize_h ? (size_t)d.nr * kMixedSide * 3 : 0; }
};

}  // namespace fe
