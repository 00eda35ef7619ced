// CPU check of facet_amd/csrc/erf_core.h (built with -fsanitize=address,undefined by tests/test_erf_host.py): fe_erf, the function the
// fp32 GELU epilogues evaluate on the device, compiled for the host and compared with erf() in double.
//
// Inputs: every 64th fp32 bit pattern of both signs, every pattern within 2^16 of the range threshold 0.921875, +-0, +-inf, NaN, the
// largest finite value, denormals. Checked: error <= 2 ulp of the result, oddness bit for bit, |erf| <= 1, non-decreasing along the
// sweep, exactly +-1 at and above 4.0. Prints the maximum error and where it falls.
//   erf_harness      exit status 0: all checks hold; 1: a check failed (the first few are printed)
#include "erf_core.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// one unit in the last place of the fp32 value nearest to |ref|
static double ulp_of(double ref) {
  const double a = std::fabs(ref);
  if (a < 0x1p-126) return 0x1p-149;
  int e;
  std::frexp(a, &e);      // a = m 2^e, m in [0.5, 1)
  return std::ldexp(1.0, e - 24);
}

struct State {
  double worst = 0.0; float worst_x = 0.f;
  double worst_gelu = 0.0; float worst_gelu_x = 0.f;      // |gelu - ref| / |v|, reported only
  float prev = 0.f; bool have_prev = false;
  long long n = 0; int bad = 0;
};

static void fail(State& s, const char* what, float x, float got) {
  if (s.bad++ < 10) printf("FAIL %s at x = %.9g (0x%08x): fe_erf = %.9g (0x%08x)\n", what, (double)x, to_bits(x), (double)got, to_bits(got));
}

// x >= 0, visited in ascending order
static void check(State& s, float x) {
  const float y = fe::fe_erf(x), yn = fe::fe_erf(-x);
  ++s.n;
  if (to_bits(yn) != (to_bits(y) ^ 0x80000000u)) fail(s, "oddness", x, yn);
  if (!(y <= 1.0f)) fail(s, "|erf| <= 1", x, y);
  if (s.have_prev && !(y >= s.prev)) fail(s, "non-decreasing", x, y);
  s.prev = y; s.have_prev = true;
  if (x >= 4.0f && y != 1.0f) fail(s, "exactly 1 at and above 4", x, y);
  const double ref = std::erf((double)x);
  const double err = std::fabs((double)y - ref) / ulp_of(ref);
  if (err > s.worst) { s.worst = err; s.worst_x = x; }
  if (!(err <= 2.0)) fail(s, "error <= 2 ulp", x, y);
  if (x >= 0x1p-100f && std::isfinite(x)) {      // (below that 0.5 v rounds in the denormals: nothing of the erf is in the figure)
    for (int sg = 0; sg < 2; ++sg) {
      const float v = sg ? -x : x;
      const double g = (double)fe::fe_gelu_erf(v), gr = 0.5 * (double)v * (1.0 + std::erf((double)v * 0.70710678118654752440));
      const double ge = std::fabs(g - gr) / std::fabs((double)v);
      if (ge > s.worst_gelu) { s.worst_gelu = ge; s.worst_gelu_x = v; }
    }
  }
}

int main() {
  State s;
  const uint32_t thr = to_bits(0.921875f), inf = 0x7f800000u;
  // ascending over the non-negative patterns: the coarse sweep, the dense band around the threshold merged in
  for (uint32_t b = 0; b <= inf; b += 64) {
    if (b + 64 > thr - 65536 && b <= thr + 65536) {      // the band starts inside this stride or the stride lies in it
      const uint32_t lo = b > thr - 65536 ? b : thr - 65536, hi = b + 63 < thr + 65536 ? b + 63 : thr + 65536;
      if (b < lo) check(s, from_bits(b));
      for (uint32_t d = lo; d <= hi; ++d) check(s, from_bits(d));
    } else {
      check(s, from_bits(b));
    }
  }
  const long long swept = s.n;
  // named values (ascending again from zero: restart the monotonic chain)
  s.have_prev = false;
  const float named[] = {0.f, from_bits(1), from_bits(2), from_bits(0x007fffffu), from_bits(0x00800000u), 1e-30f, 1e-10f, 0.921875f,
                         std::nextafterf(0.921875f, 1.f), 4.0f, 1e20f, from_bits(0x7f7fffffu), from_bits(inf)};
  for (float x : named) check(s, x);
  const float e0 = fe::fe_erf(0.f), e0n = fe::fe_erf(-0.f);
  if (to_bits(e0) != 0u || to_bits(e0n) != 0x80000000u) fail(s, "signed zero", -0.f, e0n);
  if (fe::fe_erf(from_bits(inf)) != 1.0f || fe::fe_erf(-from_bits(inf)) != -1.0f) fail(s, "+-inf", from_bits(inf), fe::fe_erf(from_bits(inf)));
  if (fe::fe_erf(from_bits(0x7f7fffffu)) != 1.0f) fail(s, "largest finite value", from_bits(0x7f7fffffu), fe::fe_erf(from_bits(0x7f7fffffu)));
  const float qn = fe::fe_erf(std::nanf("")), qg = fe::fe_gelu_erf(std::nanf(""));
  if (qn == qn || qg == qg) fail(s, "NaN in, NaN out", std::nanf(""), qn);

  printf("fe_erf: %lld inputs per sign (%lld in the sweep), max error %.4f ulp at x = %.9g (0x%08x)\n", s.n, swept, s.worst, (double)s.worst_x,
         to_bits(s.worst_x));
  printf("fe_gelu_erf: max |error| / |v| = %.4g at v = %.9g\n", s.worst_gelu, (double)s.worst_gelu_x);
  if (s.bad) { printf("%d checks failed\n", s.bad); return 1; }
  printf("ok\n");
  return 0;
}
