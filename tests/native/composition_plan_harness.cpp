// Checks the plan of the mixed-size lines / subject calls (facet_amd/csrc/composition_mixed_plan.h: what fe_leading_lines_mixed and
// fe_subject_region_mixed execute) without a GPU (tests/test_composition_plan_host.py).
//
//   composition_plan_harness <staged> <subject> <arena> h w [h w ...]      prints "chunks=<k> bad=<i> need=<bytes>"
//
// arena: "big" (8 GiB), "fit:<i>" (exactly what image i needs when it is alone in a chunk), "short:<i>" (one byte less), a byte count, or
// "cap:<pixels>" (8 GiB, and no chunk of several images may hold more pixels than that; an image alone may).
// A plan that reports an image that cannot fit (bad >= 0) must be empty and say what the image needs. Checked for every other plan:
//   1. the chunks take the images in input order, each exactly once;
//   2. per chunk the layout is the one its own sizes give, every region of the allocation starts on 256 bytes, no two overlap, all lie
//      inside the arena; the zeroed block covers exactly cnt, strong, outer, the histograms and the counters;
//   3. the descriptors: sizes, pixel offsets (sums of h * w, unpadded), work-list offsets and capacities; planes and work lists of different
//      images do not overlap and end at the chunk's totals;
//   4. every prefix table equals tile counts computed here from the tile sizes written out as numbers (32x8, 64x4, 16x16, 64 entries,
//      8192 pixels), and walking every block of every grid the way the kernels do (bisection, then row and column) covers every pixel of
//      every image exactly once and never leaves the image's tile range.
#include "composition_mixed_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace fe::comp_plan;

namespace {
std::string why;
bool fail(const std::string& m) { why = m; return false; }

int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// the kernels' bisection: prefix [n + 1], the k with prefix[k] <= b < prefix[k + 1]
int image_of_block(const std::vector<int32_t>& prefix, int n, int b, int* tile) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b) lo = mid; else hi = mid;
  }
  *tile = b - prefix[lo];
  return lo;
}

bool check(const Plan& plan, const std::vector<int32_t>& hw, bool staged, bool subject, size_t arena, size_t max_pixels) {
  const int n = (int)hw.size() / 2;
  int next = 0;
  for (size_t c = 0; c < plan.chunks.size(); ++c) {
    const Chunk& ck = plan.chunks[c];
    const std::string at = "chunk " + std::to_string(c) + ": ";
    if (ck.first != next || ck.count < 1) return fail(at + "does not continue the list");
    next += ck.count;
    const int m = ck.count;
    if (ck.descs.size() != (size_t)m) return fail(at + "descriptor count");
    // 3. descriptors
    size_t P = 0, W = 0;
    for (int k = 0; k < m; ++k) {
      const ImageDesc& d = ck.descs[k];
      const int h = hw[2 * (ck.first + k)], w = hw[2 * (ck.first + k) + 1];
      if (d.h != h || d.w != w || d.src != nullptr) return fail(at + "descriptor size");
      if (d.px != P || d.work != W) return fail(at + "descriptor offsets are not the running sums");
      if (d.cap != ((h + 1) / 2) * ((w + 1) / 2) || d.cap < 1) return fail(at + "work capacity");
      P += (size_t)h * w;
      W += (size_t)d.cap;
    }
    if (P != ck.pixels || W != ck.work || P > kMaxChunkPixels || (m > 1 && P > max_pixels)) return fail(at + "totals");
    // 2. layout
    const Layout L = layout((size_t)m, P, W, staged, subject);
    if (memcmp(&L, &ck.lay, sizeof L) != 0) return fail(at + "layout differs from its own sizes");
    if (L.total > arena) return fail(at + "exceeds the arena");
    std::vector<std::pair<size_t, size_t>> iv = {{L.blob, L.blob_bytes}, {L.gray, P}, {L.grad, P * 4}, {L.mag, P * 2}, {L.map, P}};
    if (L.blob_prefix != (size_t)m * sizeof(ImageDesc) || L.blob_bytes != L.blob_prefix + (size_t)kTilings * (m + 1) * sizeof(int32_t))
      return fail(at + "descriptor blob");
    if (subject) {
      const std::vector<std::pair<size_t, size_t>> zeroed = {{L.cnt, P * 4}, {L.strong, P * 4}, {L.outer, P}, {L.hist, (size_t)m * 1024},
                                                             {L.counters, counter_ints(m) * 4}};
      for (const auto& v : zeroed) {
        if (v.first < L.zero || v.first + v.second > L.zero + L.zero_bytes) return fail(at + "a zeroed plane outside the zeroed block");
        iv.push_back(v);
      }
      if (counter_ints(m) != 2 * (size_t)m + 2) return fail(at + "counters");
      iv.insert(iv.end(), {{L.fill, P * 12}, {L.thr, (size_t)m * 8}, {L.lab_fg, P * 4}, {L.lab_bg, P * 4}, {L.edge, P}, {L.work, W * 4}, {L.recs, W * 64}});
    }
    if (staged) iv.push_back({L.stage, P * 3});
    std::sort(iv.begin(), iv.end());
    size_t end = 0;
    for (const auto& v : iv) {
      if (v.first % kAlign != 0) return fail(at + "region off 256 bytes");
      if (v.first < end) return fail(at + "regions overlap");
      end = v.first + v.second;
    }
    if (end > L.total) return fail(at + "a region ends behind the allocation");
    if (subject) {      // nothing that is not zeroed lies inside the zeroed block
      for (const auto& v : iv)
        if (v.first >= L.zero && v.first < L.zero + L.zero_bytes && v.first != L.cnt && v.first != L.strong && v.first != L.outer && v.first != L.hist &&
            v.first != L.counters)
          return fail(at + "a live region inside the zeroed block");
    }
    // 4. prefix tables and the walk of every grid
    const int tw[3] = {32, 64, 16}, th[3] = {8, 4, 16};
    for (int t = 0; t < kTilings; ++t) {
      const std::vector<int32_t>& pre = ck.prefix[t];
      if (pre.size() != (size_t)m + 1 || pre[0] != 0) return fail(at + "prefix table size");
      for (int k = 0; k < m; ++k) {
        const int h = ck.descs[k].h, w = ck.descs[k].w;
        int want;
        if (t == kWalk) want = ceil_div(((h + 1) / 2) * ((w + 1) / 2), 64);
        else if (t == kGray) want = ceil_div((long long)h * w, 8192);
        else want = ceil_div(w, tw[t]) * ceil_div(h, th[t]);
        if (pre[k + 1] - pre[k] != want || want < 1) return fail(at + "prefix table " + std::to_string(t) + " at image " + std::to_string(k));
      }
      std::vector<std::vector<uint8_t>> seen(m);
      for (int k = 0; k < m; ++k) seen[k].assign(t == kWalk ? (size_t)ck.descs[k].cap : (size_t)ck.descs[k].h * ck.descs[k].w, 0);
      for (int b = 0; b < pre[m]; ++b) {
        int tile;
        const int k = image_of_block(pre, m, b, &tile);
        if (k < 0 || k >= m || tile < 0 || tile >= pre[k + 1] - pre[k]) return fail(at + "a block finds no image");
        const int h = ck.descs[k].h, w = ck.descs[k].w;
        if (t == kWalk || t == kGray) {
          const size_t run = t == kWalk ? 64 : 8192, p0 = (size_t)tile * run;
          if (p0 >= seen[k].size()) return fail(at + "an empty run");
          for (size_t p = p0; p < std::min(seen[k].size(), p0 + run); ++p) ++seen[k][p];
        } else {
          const int across = ceil_div(w, tw[t]), by = tile / across, bx = tile - by * across;
          if (by * th[t] >= h || bx * tw[t] >= w) return fail(at + "a tile outside its image");
          for (int y = by * th[t]; y < std::min(h, (by + 1) * th[t]); ++y)
            for (int x = bx * tw[t]; x < std::min(w, (bx + 1) * tw[t]); ++x) ++seen[k][(size_t)y * w + x];
        }
      }
      for (int k = 0; k < m; ++k)
        if (std::count(seen[k].begin(), seen[k].end(), (uint8_t)1) != (long long)seen[k].size()) return fail(at + "a pixel not covered exactly once");
    }
  }
  if (next != n) return fail("the chunks do not cover the list");
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 4) % 2 != 0) {
    fprintf(stderr, "usage: composition_plan_harness <staged> <subject> <big|fit:i|short:i|bytes|cap:pixels> h w [h w ...]\n");
    return 2;
  }
  const bool staged = atoi(argv[1]) != 0, subject = atoi(argv[2]) != 0;
  std::vector<int32_t> hw;
  for (int a = 4; a < argc; ++a) hw.push_back(atoi(argv[a]));
  const int n = (int)hw.size() / 2;
  size_t arena = (size_t)8 << 30, max_pixels = kMaxChunkPixels;
  const std::string spec = argv[3];
  if (spec.compare(0, 4, "cap:") == 0) {
    max_pixels = (size_t)strtoull(spec.c_str() + 4, nullptr, 10);
  } else if (spec != "big") {
    const size_t colon = spec.find(':');
    if (colon == std::string::npos) {
      arena = (size_t)strtoull(spec.c_str(), nullptr, 10);
    } else {
      const int i = atoi(spec.c_str() + colon + 1);
      if (i < 0 || i >= n) { fprintf(stderr, "bad arena spec\n"); return 2; }
      const Plan alone = build(&hw[2 * i], 1, staged, subject, arena);
      if (alone.chunks.size() != 1) { fprintf(stderr, "image %d alone does not plan\n", i); return 1; }
      arena = alone.chunks[0].lay.total - (spec.compare(0, 6, "short:") == 0 ? 1 : 0);
    }
  }
  const Plan plan = build(hw.data(), n, staged, subject, arena, max_pixels);
  if (plan.bad_image >= 0) {
    if (!plan.chunks.empty() || plan.bad_bytes <= arena) { fprintf(stderr, "a plan that cannot fit must be empty and say what it needs\n"); return 1; }
  } else if (!check(plan, hw, staged, subject, arena, max_pixels)) {
    fprintf(stderr, "FAILED: %s\n", why.c_str());
    return 1;
  }
  printf("chunks=%zu bad=%d need=%zu\n", plan.chunks.size(), plan.bad_image, plan.bad_bytes);
  return 0;
}
