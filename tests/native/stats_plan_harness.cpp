// Checks the block plan of a mixed-size statistics call (facet_amd/csrc/stats_plan.h: what fe_image_stats_mixed executes) without a GPU
// (tests/test_stats_plan_host.py).
//
//   stats_plan_harness <staged> <segment_pixels> <arena> h w [h w ...]      prints "chunks=<k> bad=<i>"
//
// arena: "big" (8 GiB), "fit:<i>" (exactly what image i needs when it is alone in a chunk) or "short:<i>" (one byte less).
// A plan that reports an image that cannot fit (bad >= 0) must be empty. Checked for every other plan:
//   1. the chunks take the images in input order, each exactly once;
//   2. per chunk the regions of the allocation follow each other without overlap, the zeroed block is the accumulators plus the
//      histograms, a multiple of 16 bytes, and the whole does not exceed the arena;
//   3. walking pass 1 block by block (pass1_segment / pass1_half, as the kernel does), every pixel of every image is counted exactly once
//      per hue half; every segment starts at a multiple of 4 pixels, is at most segment_pixels long, and carries its ordinal; the list of
//      images with several segments is exact;
//   4. every row of every image lies in exactly one strip;
//   5. gray planes (and staged images) start on 256 bytes, lie inside their region and do not overlap.
#include "stats_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace fe::stats_plan;

namespace {
std::string why;
bool fail(const std::string& m) { why = m; return false; }

bool disjoint(std::vector<std::pair<size_t, size_t>> iv, size_t limit) {
  std::sort(iv.begin(), iv.end());
  size_t at = 0;
  for (const auto& v : iv) {
    if (v.first < at || v.first % kAlign != 0 || v.first + v.second > limit) return false;
    at = v.first + v.second;
  }
  return true;
}

bool check(const Plan& plan, const std::vector<int32_t>& hw, bool staged, int segment, size_t arena) {
  const int n = (int)hw.size() / 2;
  int next = 0;
  for (size_t c = 0; c < plan.chunks.size(); ++c) {
    const Chunk& ck = plan.chunks[c];
    const std::string at = "chunk " + std::to_string(c) + ": ";
    if (ck.first != next || ck.count < 1) return fail(at + "does not continue the list");
    next += ck.count;
    const size_t m = (size_t)ck.count;
    if (ck.gray_off.size() != m || ck.stage_off.size() != m || ck.nseg.size() != m) return fail(at + "per-image vectors");
    // 2. the layout
    const Layout L = layout(m, ck.segs.size(), ck.strips.size(), ck.multi.size(), ck.gray_bytes, ck.stage_bytes);
    if (memcmp(&L, &ck.lay, sizeof L) != 0) return fail(at + "layout differs from its own sizes");
    if (L.total > arena) return fail(at + "exceeds the arena");
    if (L.accum != 0 || L.accum + m * kAccumBytes > L.hist || L.hist + m * kHistBytes != L.zero_bytes || L.zero_bytes % 16 != 0 ||
        L.zero_bytes > L.records || L.records + m * kRecordBytes > L.blob || L.blob + L.blob_bytes > L.gray || L.gray + ck.gray_bytes != L.stage ||
        L.stage + ck.stage_bytes != L.total)
      return fail(at + "regions overlap");
    if (L.hist % kAlign || L.records % kAlign || L.blob % kAlign || L.gray % kAlign || L.stage % kAlign) return fail(at + "region off 256 bytes");
    if (L.blob_segs != m * sizeof(ImageDesc) || L.blob_strips != L.blob_segs + ck.segs.size() * sizeof(SegDesc) ||
        L.blob_multi != L.blob_strips + ck.strips.size() * sizeof(StripDesc) || L.blob_bytes != L.blob_multi + ck.multi.size() * sizeof(int32_t))
      return fail(at + "descriptor blob");
    // 3. pass 1, block by block
    std::vector<std::vector<uint8_t>> seen[2];
    std::vector<int> n_seg(m, 0);
    for (int half = 0; half < 2; ++half) {
      seen[half].resize(m);
      for (size_t k = 0; k < m; ++k) seen[half][k].assign((size_t)hw[2 * (ck.first + k)] * hw[2 * (ck.first + k) + 1], 0);
    }
    for (unsigned b = 0; b < 2u * ck.segs.size(); ++b) {
      const int s = pass1_segment(b), half = pass1_half(b);
      if (s < 0 || (size_t)s >= ck.segs.size() || half < 0 || half > 1) return fail(at + "block outside the segment list");
      const SegDesc& sg = ck.segs[s];
      if (sg.img < 0 || (size_t)sg.img >= m) return fail(at + "segment of no image");
      std::vector<uint8_t>& px = seen[half][sg.img];
      if (sg.p0 % 4 != 0) return fail(at + "segment starts off a 4-pixel boundary");
      if (sg.count < 1 || sg.count > (uint32_t)segment || (size_t)sg.p0 + sg.count > px.size()) return fail(at + "segment length");
      if (half == 0 && sg.index != n_seg[sg.img]++) return fail(at + "segment ordinal");
      for (size_t p = sg.p0; p < (size_t)sg.p0 + sg.count; ++p)
        if (px[p]++) return fail(at + "pixel in two segments of one hue half");
    }
    std::vector<int32_t> multi;
    for (size_t k = 0; k < m; ++k) {
      for (int half = 0; half < 2; ++half)
        if (std::find(seen[half][k].begin(), seen[half][k].end(), 0) != seen[half][k].end()) return fail(at + "pixel in no segment");
      if (n_seg[k] != ck.nseg[k]) return fail(at + "segment count of an image");
      if (n_seg[k] > 1) multi.push_back((int32_t)k);
    }
    if (multi != ck.multi) return fail(at + "list of images with several segments");
    // 4. pass 2
    std::vector<std::vector<uint8_t>> rows(m);
    for (size_t k = 0; k < m; ++k) rows[k].assign((size_t)hw[2 * (ck.first + k)], 0);
    for (const StripDesc& st : ck.strips) {
      if (st.img < 0 || (size_t)st.img >= m || st.y0 < 0 || st.y0 % kStripRows != 0 || (size_t)st.y0 >= rows[st.img].size()) return fail(at + "strip");
      for (size_t y = (size_t)st.y0; y < std::min(rows[st.img].size(), (size_t)st.y0 + kStripRows); ++y)
        if (rows[st.img][y]++) return fail(at + "row in two strips");
    }
    for (size_t k = 0; k < m; ++k)
      if (std::find(rows[k].begin(), rows[k].end(), 0) != rows[k].end()) return fail(at + "row in no strip");
    // 5. planes
    std::vector<std::pair<size_t, size_t>> gray, stage;
    for (size_t k = 0; k < m; ++k) {
      const size_t npx = seen[0][k].size();
      gray.emplace_back(ck.gray_off[k], npx);
      if (staged) stage.emplace_back(ck.stage_off[k], npx * 3);
    }
    if (!disjoint(gray, ck.gray_bytes)) return fail(at + "gray planes overlap");
    if (!disjoint(stage, ck.stage_bytes)) return fail(at + "staged images overlap");
    if (!staged && ck.stage_bytes != 0) return fail(at + "stage region without staging");
  }
  if (next != n) return fail("the chunks do not cover the list");
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 4) % 2 != 0) {
    fprintf(stderr, "usage: stats_plan_harness <staged> <segment_pixels> <big|fit:i|short:i> h w [h w ...]\n");
    return 2;
  }
  const bool staged = atoi(argv[1]) != 0;
  const int segment = atoi(argv[2]);
  std::vector<int32_t> hw;
  for (int a = 4; a < argc; ++a) hw.push_back(atoi(argv[a]));
  const int n = (int)hw.size() / 2;
  size_t arena = (size_t)8 << 30;
  const std::string spec = argv[3];
  if (spec != "big") {
    const size_t colon = spec.find(':');
    const int i = colon == std::string::npos ? -1 : atoi(spec.c_str() + colon + 1);
    if (i < 0 || i >= n) { fprintf(stderr, "bad arena spec\n"); return 2; }
    const Plan alone = build(&hw[2 * i], 1, staged, segment, arena);
    if (alone.chunks.size() != 1) { fprintf(stderr, "image %d alone does not plan\n", i); return 1; }
    arena = alone.chunks[0].lay.total - (spec.compare(0, 6, "short:") == 0 ? 1 : 0);
  }
  const Plan plan = build(hw.data(), n, staged, segment, arena);
  if (plan.bad_image >= 0) {
    if (!plan.chunks.empty() || plan.bad_bytes <= arena) { fprintf(stderr, "a plan that cannot fit must be empty and say what it needs\n"); return 1; }
  } else if (!check(plan, hw, staged, segment, arena)) {
    fprintf(stderr, "FAILED: %s\n", why.c_str());
    return 1;
  }
  printf("chunks=%zu bad=%d\n", plan.chunks.size(), plan.bad_image);
  return 0;
}
