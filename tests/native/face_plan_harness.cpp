// Checks the plan of the mixed-size face calls (facet_amd/csrc/face_mixed_plan.h: what fe_face_analyze_mixed executes) without a GPU.
//   face_plan_harness <det_h> <det_w> <max_images> <staged> <stage_room> h w [h w ...]
// prints one line per image, "img <i> <new_h> <new_w> <mode> <det_scale bits, hex> <ok>", then "bad=<i>" (the first image whose staged
// bytes exceed stage_room, -1 for none) and, when there is none, one line per micro-batch "cut <i0> <i1> <bytes>" and "tables=<k>
// words=<n>". Checked here, with a non-zero exit on failure: every micro-batch holds 1 .. max_images images, its staged images start on
// 256-byte boundaries, do not overlap and end within stage_room (a micro-batch of one image may not exceed it either, which too_large
// guarantees); the cuts tile the list in order; the pool holds one table per distinct (source, target, clamp) of the images on the
// weighted route, and every table reads back what the builder made (offsets, then the two shorts of a pair in one word, signs kept).
// tests/test_face_mixed_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "face_mixed_plan.h"

using namespace fe::face_plan;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// a stand-in for cv_resize_tables with values that tell the tables apart and exercise negative shorts
static void fake_tables(int src, int dst, bool clamp, std::vector<int>& ofs, std::vector<short>& coef) {
  ofs.resize(dst);
  coef.resize((size_t)dst * 2);
  for (int d = 0; d < dst; ++d) {
    ofs[d] = (clamp ? 1 : -1) * (src + d);
    coef[2 * d] = (short)(2048 - (d % 4096));
    coef[2 * d + 1] = (short)(-(d % 3000) - (clamp ? 1 : 0));
  }
}

int main(int argc, char** argv) {
  if (argc < 8 || (argc - 6) % 2) {
    fprintf(stderr, "usage: face_plan_harness <det_h> <det_w> <max_images> <staged> <stage_room> h w [h w ...]\n");
    return 2;
  }
  const int det_h = atoi(argv[1]), det_w = atoi(argv[2]), max_images = atoi(argv[3]);
  const bool staged = atoi(argv[4]) != 0;
  const size_t room = (size_t)strtoull(argv[5], nullptr, 10);
  std::vector<int32_t> hw;
  for (int a = 6; a < argc; ++a) hw.push_back(atoi(argv[a]));
  const int n = (int)hw.size() / 2;

  TablePool pool;
  std::vector<ImageDesc> descs(n);
  std::set<std::tuple<int, int, int>> want_tables;
  for (int i = 0; i < n; ++i) {
    const bool ok = describe(hw.data(), i, det_h, det_w, pool, fake_tables, descs[i]);
    uint32_t bits;
    memcpy(&bits, &descs[i].det_scale, 4);
    printf("img %d %d %d %d %08x %d\n", i, descs[i].new_h, descs[i].new_w, descs[i].mode, bits, ok ? 1 : 0);
    if (ok && descs[i].mode == kResize) {
      want_tables.insert(std::make_tuple(descs[i].w, descs[i].new_w, 1));
      want_tables.insert(std::make_tuple(descs[i].h, descs[i].new_h, 0));
    }
  }
  CHECK(pool.tables() == want_tables.size(), "pool holds %zu tables, the list has %zu distinct ones", pool.tables(), want_tables.size());
  size_t words = 0;
  for (const auto& t : want_tables) words += 2 * (size_t)std::get<1>(t);
  CHECK(pool.words.size() == words, "pool holds %zu words, expected %zu", pool.words.size(), words);
  for (int i = 0; i < n; ++i) {
    if (descs[i].mode != kResize || descs[i].new_h <= 0 || descs[i].new_w <= 0) continue;
    for (int axis = 0; axis < 2; ++axis) {
      const int src = axis ? descs[i].h : descs[i].w, dst = axis ? descs[i].new_h : descs[i].new_w, at = axis ? descs[i].ytab : descs[i].xtab;
      std::vector<int> ofs;
      std::vector<short> coef;
      fake_tables(src, dst, axis == 0, ofs, coef);
      CHECK(at >= 0 && (size_t)at + 2 * (size_t)dst <= pool.words.size(), "image %d: table at %d leaves the pool", i, at);
      for (int d = 0; d < dst; ++d) {
        const int32_t w = pool.words[(size_t)at + dst + d];
        CHECK(pool.words[(size_t)at + d] == ofs[d], "image %d axis %d: offset %d", i, axis, d);
        CHECK((short)(w & 0xffff) == coef[2 * d] && (short)(w >> 16) == coef[2 * d + 1], "image %d axis %d: weights %d", i, axis, d);
      }
    }
  }

  const int bad = too_large(hw.data(), n, staged, room);
  printf("bad=%d\n", bad);
  if (bad >= 0) {
    CHECK(staged && staged_bytes(hw[2 * bad], hw[2 * bad + 1]) > room, "image %d fits", bad);
    for (int i = 0; i < bad; ++i) CHECK(staged_bytes(hw[2 * i], hw[2 * i + 1]) <= room, "image %d before the reported one does not fit", i);
    return 0;
  }
  std::vector<size_t> offs;
  for (int i0 = 0; i0 < n;) {
    size_t bytes = 0;
    const int i1 = cut(hw.data(), n, i0, max_images, staged, room, &offs, &bytes);
    CHECK(i1 > i0 && i1 <= n && i1 - i0 <= max_images && (int)offs.size() == i1 - i0, "cut [%d, %d)", i0, i1);
    size_t end = 0;
    for (int i = i0; i < i1; ++i) {
      const size_t b = staged ? (size_t)hw[2 * i] * hw[2 * i + 1] * 3 : 0;
      CHECK(offs[i - i0] % kAlign == 0 && offs[i - i0] >= end, "image %d starts at %zu, the one before ends at %zu", i, offs[i - i0], end);
      end = offs[i - i0] + b;
    }
    CHECK(end <= bytes && bytes <= room, "micro-batch [%d, %d) stages %zu bytes (images end at %zu), the room is %zu", i0, i1, bytes, end, room);
    // the cut is greedy: it ended at max_images, at the end of the list, or because the next image would not fit
    if (i1 < n && i1 - i0 < max_images) CHECK(staged && bytes + staged_bytes(hw[2 * i1], hw[2 * i1 + 1]) > room, "cut [%d, %d) ends early", i0, i1);
    printf("cut %d %d %zu\n", i0, i1, bytes);
    i0 = i1;
  }
  printf("tables=%zu words=%zu\n", pool.tables(), pool.words.size());
  return 0;
}
