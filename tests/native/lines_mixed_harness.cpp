// lines_host_stage_mixed (facet_amd/csrc/lines_host.cpp) against lines_host_stage image by image, without a GPU and under
// AddressSanitizer + UBSan (tests/test_lines_mixed_host.py).
//
//   lines_mixed_harness <in.bin>      prints "images=<n> segments=<sum of counts> edge_pixels=<k>"
//
// in.bin: int32 n, threshold, max_gap, max_lines, threads; int32 hw [n][2]; int32 min_len [n]; then the n maps (2 / 0 / 1 bytes) back to
// back. The mixed stage runs once over the concatenated maps; the per-shape stage runs once per image on a copy of that image's map, on
// one thread. Every edge byte, every count and every stored segment must be equal; rows of `lines` beyond a count must stay untouched.
#include "lines_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: lines_mixed_harness <in.bin>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t head[5];
  if (fread(head, sizeof(int32_t), 5, f) != 5) return 2;
  const int n = head[0], threshold = head[1], max_gap = head[2], max_lines = head[3], threads = head[4];
  if (n < 1 || max_lines < 1) return 2;
  std::vector<int32_t> hw(2 * (size_t)n), min_len(n);
  if (fread(hw.data(), sizeof(int32_t), hw.size(), f) != hw.size() || fread(min_len.data(), sizeof(int32_t), n, f) != (size_t)n) return 2;
  std::vector<size_t> offsets(n);
  size_t total = 0;
  for (int i = 0; i < n; ++i) { offsets[i] = total; total += (size_t)hw[2 * i] * hw[2 * i + 1]; }
  std::vector<uint8_t> maps(total);
  if (fread(maps.data(), 1, total, f) != total) return 2;
  fclose(f);

  std::vector<uint8_t> mixed = maps;
  std::vector<int> lines((size_t)n * max_lines * 4, -1), counts(n, -1);
  fe::lines_host_stage_mixed(mixed.data(), offsets.data(), hw.data(), n, threshold, min_len.data(), max_gap, max_lines, lines.data(), counts.data(), threads);

  long long segments = 0, edge_pixels = 0;
  for (int i = 0; i < n; ++i) {
    const int h = hw[2 * i], w = hw[2 * i + 1];
    const size_t npx = (size_t)h * w;
    std::vector<uint8_t> one(maps.begin() + offsets[i], maps.begin() + offsets[i] + npx);
    std::vector<int> l1((size_t)max_lines * 4, -1);
    int c1 = -1;
    fe::lines_host_stage(one.data(), 1, h, w, threshold, min_len[i], max_gap, max_lines, l1.data(), &c1, 1);
    if (memcmp(one.data(), mixed.data() + offsets[i], npx) != 0) { fprintf(stderr, "FAILED: image %d (%d x %d): edges differ\n", i, h, w); return 1; }
    if (c1 != counts[i]) { fprintf(stderr, "FAILED: image %d (%d x %d): %d segments, per-shape %d\n", i, h, w, counts[i], c1); return 1; }
    if (memcmp(l1.data(), lines.data() + (size_t)i * max_lines * 4, l1.size() * sizeof(int)) != 0) {
      fprintf(stderr, "FAILED: image %d (%d x %d): segments differ\n", i, h, w);
      return 1;
    }
    segments += c1;
    edge_pixels += std::count(one.begin(), one.end(), (uint8_t)255);
  }
  // an edges-only call (lines null) must leave the same edges
  std::vector<uint8_t> edges_only = maps;
  fe::lines_host_stage_mixed(edges_only.data(), offsets.data(), hw.data(), n, threshold, min_len.data(), max_gap, max_lines, nullptr, nullptr, threads);
  if (edges_only != mixed) { fprintf(stderr, "FAILED: the edges-only call differs\n"); return 1; }
  printf("images=%d segments=%lld edge_pixels=%lld\n", n, segments, edge_pixels);
  return 0;
}
