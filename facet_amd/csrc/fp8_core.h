// OCP e4m3 ("e4m3fn": 4 exponent bits of bias 7, 3 mantissa bits, no infinities, S.1111.111 = NaN, largest value 448) with one
// power-of-two scale per weight row, shared by the commit-time packer and the dequantise kernel of model_vlm.hip and by host code.
//
// A row w[0 .. K) of bf16 values gets one exponent e and K codes:
//   a = max |w[k]|;  e = the smallest integer with a * 2^-e <= 448 (0 for a zero row), clamped to e >= -117;
//   code[k] = w[k] * 2^-e rounded to nearest-even e4m3 (the scaling is exact, and by the choice of e nothing saturates);
//   w'[k] = decode(code[k]) * 2^e.
// decode(code) has 4 significant bits and 2^e is a power of two, so every w' is exactly a bf16 value: an engine that multiplies bf16
// activations with w' in fp32 computes what the bf16 engine computes on the weights w'. The clamp keeps the smallest code (2^-9) times
// 2^e at or above 2^-126, a normal bf16.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define FE_F8HD __host__ __device__ __forceinline__
#else
#define FE_F8HD inline
#endif

namespace fe {
namespace fp8 {

constexpr float E4M3_MAX = 448.f;
constexpr int ROW_EXP_MIN = -117;

FE_F8HD uint32_t f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
FE_F8HD float bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// code -> value: subnormals m * 2^-9 (exponent field 0), normals (8 + m) * 2^(E - 10), the two codes S.1111.111 NaN
FE_F8HD float e4m3_decode(uint8_t c) {
  const uint32_t sign = (uint32_t)(c & 0x80) << 24, E = (c >> 3) & 15, m = c & 7;
  if (E == 15 && m == 7) return bits_f32(sign | 0x7FC00000u);
  if (E == 0) return bits_f32(sign | f32_bits((float)m * 0.001953125f));
  return bits_f32(sign | ((E + 120) << 23) | (m << 20));
}

// value -> code, round to nearest even. What rounds past 448 (|x| > 464) and NaN give the NaN code: there is no infinity to saturate
// to, and the row rule never produces such a value.
FE_F8HD uint8_t e4m3_encode(float x) {
  uint32_t u = f32_bits(x);
  const uint8_t sign = (uint8_t)((u >> 24) & 0x80);
  u &= 0x7FFFFFFFu;
  if (u > 0x7F800000u) return sign | 0x7F;
  if (u < 0x3C800000u) {      // below 2^-6, the smallest normal: the subnormal grid has step 2^-9; 2^14 + a has exactly that ulp in fp32
    const uint32_t q = f32_bits(bits_f32(u) + 16384.f) - 0x46800000u;      // 0 .. 8 (8 = the code of 2^-6)
    return sign | (uint8_t)q;
  }
  if (u >= 0x47800000u) return sign | 0x7F;      // (far out of range: keeps the subtraction below inside 8 bits' reach)
  u += 0x7FFFFu + ((u >> 20) & 1u);      // nearest even at 3 mantissa bits
  const uint32_t c = (u >> 20) - (120u << 3);
  return sign | (uint8_t)(c > 0x7Eu ? 0x7Fu : c);
}

// the row exponent of absmax a (finite, >= 0): frexp gives a = f * 2^x with f in [0.5, 1); 448 = 0.875 * 2^9
FE_F8HD int row_exponent(float a) {
  if (!(a > 0.f)) return 0;
  int x = 0;
  const float f = frexpf(a, &x);
  const int e = f <= 0.875f ? x - 9 : x - 8;
  return e < ROW_EXP_MIN ? ROW_EXP_MIN : e;
}
// 2^e for e in -126 .. 127 (row exponents lie in -117 .. 120, so 2^e and 2^-e are both normal fp32 values)
FE_F8HD float row_scale(int e) { return bits_f32((uint32_t)(e + 127) << 23); }

// One row: K values -> K codes, *e_out = the row exponent. False (nothing useful written) when a value is NaN or infinite.
FE_F8HD bool quantize_row(const float* w, size_t K, uint8_t* code, int* e_out) {
  float a = 0.f;
  for (size_t k = 0; k < K; ++k) {
    const float v = fabsf(w[k]);
    if (!(v <= 3.4028234663852886e38f)) return false;
    a = v > a ? v : a;
  }
  const int e = row_exponent(a);
  // w * 2^-e is exact unless it falls below fp32's range, far under the half-step 2^-10 below which a value rounds to code 0 anyway
  const float inv = row_scale(-e);
  for (size_t k = 0; k < K; ++k) code[k] = e4m3_encode(w[k] * inv);
  *e_out = e;
  return true;
}

}  // namespace fp8
}  // namespace fe
