// PIL's resampling coefficients (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc) on the host. No HIP headers: the
// engine (kernels_resize.hip, the mixed-size path) and the CPU harnesses under tests/native build their tables from this one function.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define FE_RHD __host__ __device__ __forceinline__
#else
#define FE_RHD inline
#endif

namespace fe {

constexpr int kResizePrecisionBits = 32 - 8 - 2;
// Resample.c's clip8: a fixed-point accumulator (started at 1 << 21) back to a byte; what every resampling kernel and harness ends with
FE_RHD uint8_t pil_clip8(int v) {
  v >>= kResizePrecisionBits;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
// the PIL filters by their FE_FILTER_* numbers (include/facet_engine.h)
constexpr int kFilterLanczos = 1, kFilterBilinear = 2, kFilterBicubic = 3;

namespace resize_detail {
inline double filt_bilinear(double x) { if (x < 0.0) x = -x; return x < 1.0 ? 1.0 - x : 0.0; }
inline double filt_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
inline double sinc_filter(double x) { if (x == 0.0) return 1.0; x = x * M_PI; return std::sin(x) / x; }
inline double filt_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }
}  // namespace resize_detail

// kk [out_size][ksize] fixed-point coefficients (22 fractional bits), bounds [out_size][2] = (first sample, sample count).
// in0 / in1 are C floats in Resample.c too, their difference is taken in float. Returns ksize, or 0 for an unknown filter.
inline int pil_resize_coeffs(int in_size, float in0, float in1, int out_size, int filter, std::vector<int>& kk, std::vector<int>& bounds) {
  double (*f)(double);
  double fsupport;
  switch (filter) {
    case kFilterBilinear: f = resize_detail::filt_bilinear; fsupport = 1.0; break;
    case kFilterBicubic: f = resize_detail::filt_bicubic; fsupport = 2.0; break;
    case kFilterLanczos: f = resize_detail::filt_lanczos; fsupport = 3.0; break;
    default: return 0;
  }
  double scale, filterscale;
  filterscale = scale = (double)(in1 - in0) / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = fsupport * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  kk.assign((size_t)out_size * ksize, 0);
  bounds.assign((size_t)out_size * 2, 0);
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = in0 + (xx + 0.5) * scale;
    double ww = 0.0;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double w = f((x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = 0; x < xmax; ++x) {
      const double v = k[x];
      kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << kResizePrecisionBits)) : (int)(0.5 + v * (1 << kResizePrecisionBits));
    }
    bounds[xx * 2] = xmin;
    bounds[xx * 2 + 1] = xmax;
  }
  return ksize;
}

}  // namespace fe
