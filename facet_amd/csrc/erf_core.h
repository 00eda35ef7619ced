// fp32 erf without a branch, for the erf GELU of the fp32 contraction epilogues. Shared by host and device: the kernels evaluate the
// function below, and tests/native/erf_harness.cpp compares the same function with erf() in double on the CPU.
//
// ocml's erff is a two-sided branch per value (exec-mask edits around both sides, a full expf with range reduction on one of them): an
// epilogue that evaluates 4 .. 64 values per lane ran them as that many dependent chains one after another. This form evaluates both
// ranges and selects, so the compiler interleaves the values of a lane: ~26 vector instructions, one bare 2^z.
//
// Two-range minimax form (N. Juffa's erff):
//   |x| <= 0.921875:  erf(x) = x + x p(x^2),                  p of degree 5 in x^2 - relative accuracy down to denormals (erf(x) ~ 1.128 x)
//   |x| >  0.921875:  erf(x) = 1 - 2^(-log2(e) q(|x|)),       q(t) = t + t r(t), r of degree 6
// Large |x| (x^2 may overflow), +-inf: q = +inf, 2^-inf = 0, result +-1 exactly. NaN: the comparison is false, the first form returns NaN.
// Measured against erf() in double (tests/test_erf_host.py): see DESIGN.md.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FE_EHD __host__ __device__ __forceinline__
#else
#define FE_EHD inline
#endif

namespace fe {

FE_EHD float fe_erf_exp2(float z) {      // 2^z, z <= 0: the bare v_exp_f32 on the device (1 ulp; a denormal result may flush: 1 - 2^z is 1 there)
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(z);
#else
  return exp2f(z);
#endif
}

FE_EHD float fe_erf(float x) {
  const float t = fabsf(x), s = x * x;
  // |x| > 0.921875
  float r = fmaf(0x1.222900p-16f, t, -0x1.91d2ccp-12f);
  const float u = fmaf(0x1.fd1336p-09f, t, -0x1.8d6300p-06f);
  r = fmaf(r, s, u);
  r = fmaf(r, t, 0x1.b55cb0p-4f);
  r = fmaf(r, t, 0x1.450aa0p-1f);
  r = fmaf(r, t, 0x1.079d0cp-3f);
  r = fmaf(r, t, t);
  const float big = 1.0f - fe_erf_exp2(r * -1.44269504088896341f);
  // |x| <= 0.921875
  float p = -0x1.3a1a82p-11f;
  p = fmaf(p, s, 0x1.473f48p-08f);
  p = fmaf(p, s, -0x1.b68bd2p-06f);
  p = fmaf(p, s, 0x1.ce1a46p-04f);
  p = fmaf(p, s, -0x1.8126e0p-02f);
  p = fmaf(p, s, 0x1.06eba6p-03f);
  const float small = fmaf(p, t, t);
  return copysignf(t > 0.921875f ? big : small, x);
}

// GELU(v) = v Phi(v), the exact (erf) form
FE_EHD float fe_gelu_erf(float v) { return 0.5f * v * (1.f + fe_erf(v * 0.70710678f)); }

}  // namespace fe
