// Runs the stages of facet_amd/csrc/thumb_mixed_core.h on the CPU (tests/test_thumb_mixed_host.py): the descriptors and the table pool
// are built by ThumbTables exactly as fe_thumbnail_jpeg_mixed builds them for the device, and every sample goes through
// thumb_reduce_sample / thumb_pass_sample, the functions the kernels call. Also prints the pool of fe_phash_mixed (phash_mixed_plan.h).
//
//   thumb_mixed_harness thumb <in> <out>
//     in:  int32 n, then per image int32 h, w, oh, ow, fx, fy, reduce_box[4], float resize_box[4], int32 tall (fe_thumb_plan's fields
//          behind the size) and h*w*3 bytes; out: per image oh*ow*3 bytes, the pixels the encoder would read.
//     Prints "tables <count> pool <ints>".
//   thumb_mixed_harness phash <h> <w> [<h> <w> ...]
//     Prints per image "desc <kh> <bh> <ksize_h> <kv> <bv> <ksize_v>", per distinct side "side <in> taps <k[0][0]> bounds <first> <count>
//     ... of output 0 and 31", and "tables <count>".
//
// Every image, every intermediate and the pool sit in heap blocks of their exact sizes, so AddressSanitizer sees any sample read or
// written outside them.
#include "phash_mixed_plan.h"
#include "thumb_mixed_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace fe;

static std::unique_ptr<uint8_t[]> block(size_t bytes) { return std::unique_ptr<uint8_t[]>(bytes ? new uint8_t[bytes] : nullptr); }

static int run_thumb(const char* in, const char* out) {
  FILE* fi = fopen(in, "rb");
  if (!fi) { perror("in"); return 2; }
  int32_t n = 0;
  if (fread(&n, 4, 1, fi) != 1 || n < 1) return 2;
  std::vector<std::unique_ptr<uint8_t[]>> img(n), red(n), mid(n), pix(n);
  std::vector<ThumbDesc> desc(n);
  ThumbTables tables;
  struct Plan { int32_t v[10]; float box[4]; int32_t tall; };
  std::vector<Plan> plans(n);
  for (int i = 0; i < n; ++i) {
    int32_t* v = plans[i].v;
    float* box = plans[i].box;
    int32_t& tall = plans[i].tall;
    if (fread(v, 4, 10, fi) != 10 || fread(box, 4, 4, fi) != 4 || fread(&tall, 4, 1, fi) != 1) return 2;
    const size_t bytes = (size_t)v[0] * v[1] * 3;
    img[i] = block(bytes);
    if (fread(img[i].get(), 1, bytes, fi) != bytes) return 2;
    if (const char* why = tables.describe(v[0], v[1], v[2], v[3], v[4], v[5], v + 6, box, tall, desc[i])) {
      printf("image %d (%d x %d): %s\n", i, v[0], v[1], why);
      return 1;
    }
    red[i] = block(ThumbTables::red_bytes(desc[i]));
    mid[i] = block(ThumbTables::mid_bytes(desc[i]));
    pix[i] = block(ThumbTables::pix_bytes(desc[i]));
    desc[i].src = img[i].get(); desc[i].red = red[i].get(); desc[i].mid = mid[i].get(); desc[i].pix = pix[i].get();
  }
  fclose(fi);
  for (int i = 0; i < n; ++i) {   // a plan seen before adds nothing to the pool and gets the same tables
    const size_t before = tables.pool.size(), count = tables.tables();
    ThumbDesc again;
    const Plan& p = plans[i];
    if (tables.describe(p.v[0], p.v[1], p.v[2], p.v[3], p.v[4], p.v[5], p.v + 6, p.box, p.tall, again) || tables.pool.size() != before ||
        tables.tables() != count || memcmp(again.pass, desc[i].pass, sizeof(again.pass)) != 0) {
      printf("image %d: described again, the pool or the tables changed\n", i);
      return 1;
    }
  }
  const std::unique_ptr<int32_t[]> pool(new int32_t[tables.pool.size() ? tables.pool.size() : 1]);      // a block of its exact size
  if (!tables.pool.empty()) memcpy(pool.get(), tables.pool.data(), tables.pool.size() * sizeof(int32_t));
  FILE* fo = fopen(out, "wb");
  if (!fo) { perror("out"); return 2; }
  for (int i = 0; i < n; ++i) {
    const ThumbDesc& d = desc[i];
    if (thumb_reduces(d))
      for (int y = 0; y < d.rh; ++y)
        for (int x = 0; x < d.rw; ++x) thumb_reduce_sample(d, y, x, d.red + ((size_t)y * d.rw + x) * 3);
    for (int p = 0; p < 2; ++p) {
      const ThumbPass& ps = d.pass[p];
      if (!ps.ksize) continue;
      const uint8_t* src = thumb_pass_in(d, p);
      uint8_t* dst = thumb_pass_out(d, p);
      for (int y = 0; y < ps.oh; ++y)
        for (int x = 0; x < ps.ow; ++x) thumb_pass_sample(ps, pool.get(), src, y, x, dst + ((size_t)y * ps.ow + x) * 3);
    }
    const size_t bytes = (size_t)d.oh * d.ow * 3;
    if (fwrite(thumb_pixels(d), 1, bytes, fo) != bytes) return 2;
  }
  fclose(fo);
  printf("tables %zu pool %zu\n", tables.tables(), tables.pool.size());
  return 0;
}

static int run_phash(int argc, char** argv) {
  PhashTables tables;
  std::vector<int> sides;
  for (int a = 2; a + 1 < argc; a += 2) {
    const int h = atoi(argv[a]), w = atoi(argv[a + 1]);
    PhashDesc d;
    if (!tables.describe(h, w, d)) { printf("image %d x %d not described\n", h, w); return 1; }
    printf("desc %d %d %d %d %d %d\n", d.kh, d.bh, d.ksize_h, d.kv, d.bv, d.ksize_v);
    sides.push_back(h); sides.push_back(w);
  }
  const std::unique_ptr<int32_t[]> pool(new int32_t[tables.pool.size()]);
  memcpy(pool.get(), tables.pool.data(), tables.pool.size() * sizeof(int32_t));
  for (int s : sides) {
    int32_t k, b, ks;
    const size_t before = tables.pool.size();
    if (!tables.table(s, k, b, ks) || tables.pool.size() != before) { printf("the pool grew for a known side\n"); return 1; }
    long long sum0 = 0, sum31 = 0;      // every window's coefficients add up to about 1.0 in 22-bit fixed point
    for (int t = 0; t < pool[b + 1]; ++t) sum0 += pool[k + t];
    for (int t = 0; t < pool[b + 2 * 31 + 1]; ++t) sum31 += pool[k + (size_t)31 * ks + t];
    printf("side %d ksize %d first %d %d count %d %d sum %lld %lld tap %d\n", s, ks, pool[b], pool[b + 2 * 31], pool[b + 1], pool[b + 2 * 31 + 1], sum0, sum31,
           pool[k]);
  }
  printf("tables %zu\n", tables.tables());
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "thumb")) return run_thumb(argv[2], argv[3]);
  if (argc >= 4 && !strcmp(argv[1], "phash") && argc % 2 == 0) return run_phash(argc, argv);
  fprintf(stderr, "usage: %s thumb <in> <out> | phash <h> <w> [<h> <w> ...]\n", argv[0]);
  return 2;
}
