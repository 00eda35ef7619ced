// Checks what the plans of the mixed-size calls share (facet_amd/csrc/mixed_list.h) without a GPU, and prints the arena chunks of the
// pHash, thumbnail and statistics calls for a list (tests/test_mixed_list_host.py; built with -fsanitize=address,undefined).
//   mixed_list_harness cutter <seed> <lists>      the greedy cutter over random lists of 1 .. 40 images with sides 1 .. 3000
//   mixed_list_harness offsets <seed> <lists>     the staged offsets of such lists, aligned and packed
//   mixed_list_harness pool                       PilTablePool
//   mixed_list_harness cuts phash <arena> <staged> <small> <dct> h w [h w ...]
//   mixed_list_harness cuts stats <arena> <staged> <segment> h w [h w ...]
//   mixed_list_harness cuts thumb <arena> <staged> <row bytes> <in>      in: the input file of thumb_mixed_harness
//     print "cuts <count> <count> ..." (images per chunk), or "bad <image> <bytes>"
// A failed check prints FAIL with its line and exits 1.
#include "phash_mixed_plan.h"
#include "stats_plan.h"
#include "thumb_mixed_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace fe;
using namespace fe::mixed_list;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static std::vector<int32_t> random_list(std::mt19937& rng) {
  const int n = 1 + (int)(rng() % 40);
  const int top = (rng() % 3 == 0) ? 3000 : 200;      // lists of small images fill chunks with many
  std::vector<int32_t> hw(2 * (size_t)n);
  for (auto& v : hw) v = 1 + (int32_t)(rng() % top);
  return hw;
}

// A step like the calls': staged bytes against a room, at most max_images to a chunk.
static int run_cutter(unsigned seed, int lists) {
  std::mt19937 rng(seed);
  int with_bad = 0, several = 0, by_count = 0, by_room = 0;
  for (int l = 0; l < lists; ++l) {
    const std::vector<int32_t> hw = random_list(rng);
    const int n = (int)hw.size() / 2, max_images = 1 + (int)(rng() % 12);
    size_t largest = 0, total = 0;
    std::vector<size_t> need(n);
    for (int i = 0; i < n; ++i) { need[i] = align_up(image_bytes(hw.data(), i)) + 64; largest = std::max(largest, need[i]); total += need[i]; }
    // rooms that force every case: below the largest image, exactly it, a few images, the whole list
    const size_t rooms[4] = {largest - 1 - rng() % largest, largest, largest + rng() % (total - largest + 1), total};
    for (const size_t room : rooms) {
      size_t used = 0;
      const Cuts cuts = cut_list(n, [&](int) { used = 0; }, [&](int i, int held, size_t& bytes) {
        bytes = need[i];
        if (held >= max_images || used + need[i] > room) return false;
        used += need[i];
        return true;
      });
      int first_bad = -1;
      for (int i = 0; i < n && first_bad < 0; ++i) if (need[i] > room) first_bad = i;
      CHECK(cuts.bad_image == first_bad, "list %d room %zu: bad image %d, the first that cannot stand alone is %d", l, room, cuts.bad_image, first_bad);
      if (first_bad >= 0) {
        CHECK(cuts.ends.empty() && cuts.bad_bytes == need[first_bad], "list %d room %zu: bad image %d with %zu bytes", l, room, first_bad, cuts.bad_bytes);
        ++with_bad;
        continue;
      }
      int i0 = 0;
      for (const int i1 : cuts.ends) {
        CHECK(i1 > i0 && i1 <= n && i1 - i0 <= max_images, "list %d room %zu: chunk [%d, %d)", l, room, i0, i1);      // in order, never empty
        size_t sum = 0;
        for (int i = i0; i < i1; ++i) sum += need[i];
        CHECK(sum <= room, "list %d: chunk [%d, %d) takes %zu of %zu", l, i0, i1, sum, room);
        if (i1 < n) {      // maximal: the next image would not have fitted
          CHECK(i1 - i0 == max_images || sum + need[i1] > room, "list %d room %zu: chunk [%d, %d) ends early", l, room, i0, i1);
          if (i1 - i0 == max_images) ++by_count; else ++by_room;
        }
        if (i1 - i0 > 1) ++several;
        i0 = i1;
      }
      CHECK(i0 == n, "list %d room %zu: the chunks end at %d of %d", l, room, i0, n);
    }
  }
  CHECK(with_bad && several && by_count && by_room, "a case never occurred: %d %d %d %d", with_bad, several, by_count, by_room);
  printf("cutter ok: %d lists, %d refused, %d chunks of several, %d ended by the count, %d by the room\n", lists, with_bad, several, by_count, by_room);
  return 0;
}

static int run_offsets(unsigned seed, int lists) {
  std::mt19937 rng(seed);
  for (int l = 0; l < lists; ++l) {
    const std::vector<int32_t> hw = random_list(rng);
    const int n = (int)hw.size() / 2, i0 = (int)(rng() % n);
    for (const bool aligned : {true, false}) {
      std::vector<size_t> off;
      const size_t sum = staged_offsets(hw.data(), i0, n, aligned, off);
      CHECK((int)off.size() == n - i0, "list %d: %zu offsets for %d images", l, off.size(), n - i0);
      size_t end = 0;
      for (int i = i0; i < n; ++i) {
        const size_t at = off[i - i0];
        CHECK(at >= end && (aligned ? at % kAlign == 0 && at < end + kAlign : at == end), "list %d image %d: at %zu, the one before ends at %zu", l, i, at, end);
        end = at + image_bytes(hw.data(), i);
      }
      CHECK(end <= sum && sum == (aligned ? align_up(end) : end), "list %d: images end at %zu, the region has %zu", l, end, sum);
    }
  }
  printf("offsets ok: %d lists\n", lists);
  return 0;
}

static int run_pool() {
  PilTablePool p;
  struct Key { int in; float in0, in1; int out, filter, first, count; };
  const Key base = {300, 0.0f, 300.0f, 64, kFilterLanczos, 0, 64};
  // the base key, then one field changed at a time
  const Key keys[] = {base, {301, 0.0f, 300.0f, 64, kFilterLanczos, 0, 64}, {300, 0.5f, 300.0f, 64, kFilterLanczos, 0, 64}, {300, 0.0f, 299.5f, 64, kFilterLanczos, 0, 64},
                      {300, 0.0f, 300.0f, 65, kFilterLanczos, 0, 64}, {300, 0.0f, 300.0f, 64, kFilterBicubic, 0, 64}, {300, 0.0f, 300.0f, 64, kFilterLanczos, 1, 63},
                      {300, 0.0f, 300.0f, 64, kFilterLanczos, 0, 63}, {224, 0.0f, 224.0f, 2240, kFilterBicubic, 1008, 224}};
  std::vector<int32_t> k_at, b_at;
  size_t tables = 0;
  for (const Key& q : keys) {
    const size_t before = p.pool.size();
    int32_t k, b, ks;
    CHECK(p.add(q.in, q.in0, q.in1, q.out, q.filter, q.first, q.count, k, b, ks), "key %zu refused", tables);
    std::vector<int> kk, bounds;
    const int want = pil_resize_coeffs(q.in, q.in0, q.in1, q.out, q.filter, kk, bounds);
    CHECK(ks == want && k == (int32_t)before && b == k + q.count * ks && p.pool.size() == before + (size_t)q.count * (ks + 2), "key %zu: layout", tables);
    CHECK(!memcmp(&p.pool[k], &kk[(size_t)q.first * ks], (size_t)q.count * ks * 4) && !memcmp(&p.pool[b], &bounds[(size_t)q.first * 2], (size_t)q.count * 8),
          "key %zu: not the slice of pil_resize_coeffs", tables);
    CHECK(p.tables() == ++tables, "key %zu shares a table", tables);
    k_at.push_back(k); b_at.push_back(b);
  }
  for (size_t t = 0; t < tables; ++t) {      // a repeated key adds no words and gives the same offsets
    const Key& q = keys[t];
    const size_t before = p.pool.size();
    int32_t k, b, ks;
    CHECK(p.add(q.in, q.in0, q.in1, q.out, q.filter, q.first, q.count, k, b, ks) && p.pool.size() == before && p.tables() == tables && k == k_at[t] && b == b_at[t],
          "key %zu again", t);
  }
  int32_t k, b, ks;
  const size_t before = p.pool.size();
  CHECK(p.add_identity(32, k, b, ks) && ks == 1 && p.pool.size() == before + 32 * 3 && p.tables() == tables + 1, "the identity table");
  for (int i = 0; i < 32; ++i) CHECK(p.pool[k + i] == 1 << 22 && p.pool[b + 2 * i] == i && p.pool[b + 2 * i + 1] == 1, "identity tap %d", i);
  CHECK(p.add_identity(32, k, b, ks) && p.pool.size() == before + 32 * 3, "the identity table again");
  CHECK(!p.add(300, 0.0f, 300.0f, 64, kFilterLanczos, 1, 64, k, b, ks) && !p.add(300, 0.0f, 300.0f, 64, 9, 0, 64, k, b, ks), "a range past the table or an unknown filter");
  // A box that ends 10 samples behind the axis: pil_resize_coeffs clamps every window to the axis, so the table is good and every window
  // of it lies inside. One that ends 100 behind: the last windows start behind the axis (first sample 378 of 300, a negative count),
  // which is what the pool refuses.
  CHECK(p.add(300, 0.0f, 310.0f, 64, kFilterLanczos, 0, 64, k, b, ks), "a box whose windows are clamped to the axis");
  for (int i = 0; i < 64; ++i) CHECK(p.pool[b + 2 * i] >= 0 && p.pool[b + 2 * i + 1] >= 0 && p.pool[b + 2 * i] + p.pool[b + 2 * i + 1] <= 300, "window %d leaves the axis", i);
  const size_t words = p.pool.size();
  CHECK(!p.add(300, 0.0f, 400.0f, 64, kFilterLanczos, 0, 64, k, b, ks) && p.pool.size() == words, "a window past the axis");
  printf("pool ok: %zu tables, %zu words\n", p.tables(), p.pool.size());
  return 0;
}

static void print_cuts(const std::vector<int>& ends) {
  printf("cuts");
  int i0 = 0;
  for (const int i1 : ends) { printf(" %d", i1 - i0); i0 = i1; }
  printf("\n");
}

static int run_cuts(int argc, char** argv) {
  const size_t arena = (size_t)strtoull(argv[3], nullptr, 10);
  const bool staged = atoi(argv[4]) != 0;
  if (!strcmp(argv[2], "thumb")) {
    const size_t dcap = (size_t)strtoull(argv[5], nullptr, 10);
    FILE* f = fopen(argv[6], "rb");
    int32_t n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n < 1) return 2;
    ThumbTables tables;
    std::vector<ThumbDesc> descs(n);
    for (int i = 0; i < n; ++i) {
      int32_t v[10], tall;
      float box[4];
      if (fread(v, 4, 10, f) != 10 || fread(box, 4, 4, f) != 4 || fread(&tall, 4, 1, f) != 1 || fseek(f, (long)v[0] * v[1] * 3, SEEK_CUR)) return 2;
      CHECK(!tables.describe(v[0], v[1], v[2], v[3], v[4], v[5], v + 6, box, tall, descs[i]), "image %d not described", i);
    }
    fclose(f);
    // as fe_thumbnail_jpeg_mixed: the pool is the arena's first allocation
    print_cuts(thumb_mixed_cuts(descs.data(), n, staged, dcap, arena, tables.pool.size() * sizeof(int32_t)));
    return 0;
  }
  const bool phash = !strcmp(argv[2], "phash");
  const int first = phash ? 7 : 6;
  std::vector<int32_t> hw;
  for (int a = first; a < argc; ++a) hw.push_back(atoi(argv[a]));
  const int n = (int)hw.size() / 2;
  if (phash) {
    PhashTables tables;
    for (int i = 0; i < n; ++i) { PhashDesc d; CHECK(tables.describe(hw[2 * i], hw[2 * i + 1], d), "image %d not described", i); }
    const Cuts c = phash_cuts(hw.data(), n, atoi(argv[5]) != 0, atoi(argv[6]) != 0, staged, tables.pool.size(), arena);
    if (c.bad_image >= 0) printf("bad %d %zu\n", c.bad_image, c.bad_bytes); else print_cuts(c.ends);
    return 0;
  }
  const stats_plan::Plan plan = stats_plan::build(hw.data(), n, staged, atoi(argv[5]), arena);
  if (plan.bad_image >= 0) { printf("bad %d %zu\n", plan.bad_image, plan.bad_bytes); return 0; }
  std::vector<int> ends;
  for (const auto& ck : plan.chunks) ends.push_back(ck.first + ck.count);
  print_cuts(ends);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "cutter")) return run_cutter((unsigned)atoi(argv[2]), atoi(argv[3]));
  if (argc == 4 && !strcmp(argv[1], "offsets")) return run_offsets((unsigned)atoi(argv[2]), atoi(argv[3]));
  if (argc == 2 && !strcmp(argv[1], "pool")) return run_pool();
  if (argc >= 6 && !strcmp(argv[1], "cuts") && (!strcmp(argv[2], "thumb") ? argc == 7 : argc >= 8)) return run_cuts(argc, argv);
  fprintf(stderr, "usage: %s cutter|offsets <seed> <lists> | pool | cuts phash|stats|thumb ...\n", argv[0]);
  return 2;
}
