// The two passes of resize_mixed_core.h as kernels: one launch per pass for a list of images of any sizes.
//
// Mapping: blockIdx.y is the image (its descriptor), blockIdx.x strides over that image's samples, one thread per output pixel (three
// channels). Neighbouring lanes take neighbouring crop columns, so in the vertical pass a wave reads 192 contiguous bytes of each
// intermediate row and in the horizontal pass its windows overlap or abut in one source row; sources may sit at any byte alignment, so
// loads are bytes. Coefficients are read from the pool in global memory: a table is 224 x ksize ints (a few KB, at most ~100 KB for a
// panorama) and is shared by every row of the image, so it stays in L2. The per-image work differs (nr rows); blocks past an image's
// last sample leave at once.
#include "engine.h"
#include "resize_mixed_core.h"

namespace fe {

static_assert(sizeof(MixedDesc) == 72, "MixedDesc layout");

__global__ void __launch_bounds__(256) resize_mixed_h_kernel(const MixedDesc* __restrict__ desc, const int32_t* __restrict__ pool,
                                                             uint8_t* __restrict__ scratch) {
  const MixedDesc d = desc[blockIdx.y];
  if (d.ksize_h == 0) return;
  const int total = d.nr * kMixedSide;
  uint8_t* inter = scratch + d.inter;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int r = i / kMixedSide, xx = i - r * kMixedSide;
    uint8_t o[3];
    mixed_h_sample(d, pool, r, xx, o);
    uint8_t* q = inter + (size_t)i * 3;
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
  }
}

// NORM: the crop goes out as the model's normalised fp32 NHWC4 input (out_f, slot stride 224 * 224 float4), else as uint8 [224][224][3]
template <bool NORM>
__global__ void __launch_bounds__(256) resize_mixed_v_kernel(const MixedDesc* __restrict__ desc, const int32_t* __restrict__ pool,
                                                             const uint8_t* __restrict__ scratch, uint8_t* __restrict__ out_u8,
                                                             float4* __restrict__ out_f, float m0, float m1, float m2, float s0, float s1,
                                                             float s2) {
  const MixedDesc d = desc[blockIdx.y];
  constexpr int total = kMixedSide * kMixedSide;
  const uint8_t* inter = scratch + d.inter;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int yy = i / kMixedSide, x = i - yy * kMixedSide;
    uint8_t o[3];
    mixed_v_sample(d, pool, inter, yy, x, o);
    if (NORM) {
      out_f[(size_t)d.slot * total + i] = make_float4(mixed_norm(o[0], m0, s0), mixed_norm(o[1], m1, s1), mixed_norm(o[2], m2, s2), 0.f);
    } else {
      uint8_t* q = out_u8 + ((size_t)d.slot * total + i) * 3;
      q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
    }
  }
}

// d_desc [count] and d_pool on the device; scratch holds every intermediate the descriptors name (max_nr = the largest nr among those with
// a horizontal pass, 0 when none has one). Exactly one of out_u8 / out_f: [slots][224][224][3] uint8, or normalised [slots][224][224][4] fp32.
void resize_mixed224(Ctx& c, const MixedDesc* d_desc, int count, int max_nr, const int32_t* d_pool, uint8_t* d_scratch, uint8_t* out_u8,
                     float* out_f, const float mean[3], const float stdv[3]) {
  FE_CHECK(d_desc && d_pool && count > 0 && count <= 65535 && max_nr >= 0 && (out_u8 != nullptr) != (out_f != nullptr), "resize_mixed224: bad arguments");
  FE_CHECK(!out_f || ((uintptr_t)out_f & 15) == 0, "resize_mixed224: output alignment");
  if (max_nr > 0) {
    FE_CHECK(d_scratch, "resize_mixed224: no scratch for the intermediates");
    const int gx = std::min(256, (max_nr * kMixedSide + 255) / 256);
    hipLaunchKernelGGL(resize_mixed_h_kernel, dim3(gx, count), dim3(256), 0, c.stream, d_desc, d_pool, d_scratch);
    FE_HIP(hipGetLastError());
  }
  const int gv = (kMixedSide * kMixedSide + 255) / 256;
  if (out_f)
    hipLaunchKernelGGL(resize_mixed_v_kernel<true>, dim3(gv, count), dim3(256), 0, c.stream, d_desc, d_pool, d_scratch, (uint8_t*)nullptr,
                       (float4*)out_f, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
  else
    hipLaunchKernelGGL(resize_mixed_v_kernel<false>, dim3(gv, count), dim3(256), 0, c.stream, d_desc, d_pool, d_scratch, out_u8,
                       (float4*)nullptr, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
