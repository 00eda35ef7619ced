// Runs the two passes of facet_amd/csrc/resize_mixed_core.h on the CPU (tests/test_resize_mixed_host.py): the descriptors and the table
// pool are built by MixedTables exactly as the engine builds them for the device, and every sample goes through mixed_h_sample /
// mixed_v_sample, the functions the kernels call.
//
//   resize_mixed_harness <mode> <in> <out>
//
// in:  int32 n, then per image int32 h, int32 w and h*w*3 bytes; out: n crops of 224*224*3 bytes. The normalised value of every sample
// (mixed_norm) is compared here with launch_u8_to_nhwc4_norm's formula on the uint8 sample. Every image sits in a heap block of its exact
// size, and so does every intermediate, so AddressSanitizer sees any sample read or written outside them.
#include "resize_mixed_core.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace fe;

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s <mode> <in> <out>\n", argv[0]); return 2; }
  const int mode = atoi(argv[1]);
  FILE* fi = fopen(argv[2], "rb");
  if (!fi) { perror("in"); return 2; }
  int32_t n = 0;
  if (fread(&n, 4, 1, fi) != 1 || n < 1) return 2;
  std::vector<std::unique_ptr<uint8_t[]>> img(n), inter(n);
  std::vector<MixedDesc> desc(n);
  MixedTables tables;
  size_t pool_before_repeat = 0;
  for (int i = 0; i < n; ++i) {
    int32_t hw[2];
    if (fread(hw, 4, 2, fi) != 2) return 2;
    const size_t bytes = (size_t)hw[0] * hw[1] * 3;
    img[i].reset(new uint8_t[bytes]);
    if (fread(img[i].get(), 1, bytes, fi) != bytes) return 2;
    if (!tables.describe(mode, hw[0], hw[1], desc[i])) { printf("image %d: %d x %d not described\n", i, hw[0], hw[1]); return 1; }
    desc[i].src = img[i].get();
    desc[i].slot = i;
    desc[i].inter = 0;      // every intermediate is a block of its own here
    inter[i].reset(new uint8_t[MixedTables::inter_bytes(desc[i])]);
    pool_before_repeat = tables.pool.size();
  }
  fclose(fi);
  {   // a shape seen before adds nothing to the pool
    MixedDesc again;
    if (!tables.describe(mode, desc[0].h, desc[0].w, again) || tables.pool.size() != pool_before_repeat) { printf("the pool grew for a known shape\n"); return 1; }
  }
  const std::vector<int32_t> pool = tables.pool;      // a block of its exact size, like the images
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  FILE* fo = fopen(argv[3], "wb");
  if (!fo) { perror("out"); return 2; }
  std::vector<uint8_t> crop((size_t)kMixedSide * kMixedSide * 3);
  for (int i = 0; i < n; ++i) {
    const MixedDesc& d = desc[i];
    if (d.ksize_h)
      for (int r = 0; r < d.nr; ++r)
        for (int xx = 0; xx < kMixedSide; ++xx) mixed_h_sample(d, pool.data(), r, xx, inter[i].get() + ((size_t)r * kMixedSide + xx) * 3);
    for (int yy = 0; yy < kMixedSide; ++yy)
      for (int x = 0; x < kMixedSide; ++x) {
        uint8_t* o = crop.data() + ((size_t)yy * kMixedSide + x) * 3;
        mixed_v_sample(d, pool.data(), inter[i].get(), yy, x, o);
        for (int c = 0; c < 3; ++c)
          if (mixed_norm(o[c], mean[c], stdv[c]) != ((float)o[c] / 255.0f - mean[c]) / stdv[c]) { printf("normalisation differs\n"); return 1; }
      }
    if (fwrite(crop.data(), 1, crop.size(), fo) != crop.size()) return 2;
  }
  fclose(fo);
  printf("%d crops pool %zu ints\n", n, pool.size());
  return 0;
}
