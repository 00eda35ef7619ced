// Host harness of facet_amd/csrc/fp8_core.h for tests/test_vlm_fp8_host.py (compiled under AddressSanitizer + UBSan).
//   fp8_core_harness decode OUT          -> 256 float32: the value of every code
//   fp8_core_harness encode IN OUT       IN: float32 values            -> one code per value
//   fp8_core_harness rows IN OUT         IN: int32 N, int32 K, N*K float32 -> per row: int32 ok, int32 exponent, K codes, K float32 w'
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fp8_core.h"

using namespace fe::fp8;

static std::vector<char> slurp(const char* path) {
  std::vector<char> b;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  FILE* out = fopen(argv[argc - 1], "wb");
  if (!out) return 2;
  if (mode == "decode") {
    for (int c = 0; c < 256; ++c) { const float v = e4m3_decode((uint8_t)c); fwrite(&v, 4, 1, out); }
  } else if (mode == "encode" && argc == 4) {
    const std::vector<char> in = slurp(argv[2]);
    std::vector<float> x(in.size() / 4);
    memcpy(x.data(), in.data(), x.size() * 4);
    std::vector<uint8_t> c(x.size());
    for (size_t i = 0; i < x.size(); ++i) c[i] = e4m3_encode(x[i]);
    fwrite(c.data(), 1, c.size(), out);
  } else if (mode == "rows" && argc == 4) {
    const std::vector<char> in = slurp(argv[2]);
    int32_t hdr[2];
    memcpy(hdr, in.data(), 8);
    const size_t N = (size_t)hdr[0], K = (size_t)hdr[1];
    if (in.size() != 8 + N * K * 4) { fprintf(stderr, "bad input size\n"); return 2; }
    std::vector<float> w(K), wd(K);
    std::vector<uint8_t> c(K);
    for (size_t n = 0; n < N; ++n) {
      memcpy(w.data(), in.data() + 8 + n * K * 4, K * 4);
      int e = 0;
      const int32_t ok = quantize_row(w.data(), K, c.data(), &e) ? 1 : 0;
      if (!ok) { std::fill(c.begin(), c.end(), 0); e = 0; }
      for (size_t k = 0; k < K; ++k) wd[k] = e4m3_decode(c[k]) * row_scale(e);
      const int32_t e32 = e;
      fwrite(&ok, 4, 1, out); fwrite(&e32, 4, 1, out);
      fwrite(c.data(), 1, K, out); fwrite(wd.data(), 4, K, out);
    }
  } else {
    return 2;
  }
  fclose(out);
  return 0;
}
