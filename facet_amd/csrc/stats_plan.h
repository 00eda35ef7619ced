// The block plan of fe_image_stats_mixed as data. Host only (no HIP headers): capi_image.hip executes it, kernels_stats.hip reads its
// descriptors, tests/native/stats_plan_harness.cpp checks it without a GPU.
//
// A list of images of any sizes is cut, in input order, into chunks whose scratch fits the arena. Per chunk:
//   pass 1   one workgroup per (pixel segment, hue half): segments are runs of `segment_pixels` pixels of one image, the last one of an
//            image ragged; every segment starts at a multiple of 4 pixels, so its bytes start 12 k bytes behind the image's base.
//   entropy  one workgroup per (image with more than one segment, hue half); an image with one segment finishes inside pass 1.
//   pass 2   one workgroup per strip of kStripRows rows of one image's gray plane.
// One arena allocation per chunk, carved by Layout: the zeroed block (accumulators, then the per-image 180 x 256 hue-saturation
// histograms) first, then the records, the descriptor blob (one upload), the gray planes and, for host input, the staged pixels.
#pragma once
#include "mixed_list.h"
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fe {
namespace stats_plan {

constexpr int kSegmentUnit = 4096;            // fe_set_stats_segment takes multiples of this
// Pixels per pass-1 segment when fe_set_stats_segment was not called (or was called with 0). Measured (profiles/mixed_stats_perf.txt):
// of 65 536, 262 144 and 1 048 576 this is the fastest for 256 photos of 256 shapes (1.76 / 1.83 / 2.04 ms) and for one 24-megapixel
// photo (0.38 / 0.43 / 0.70 ms); for 256 photos of 1024 x 1024, where 1 048 576 makes every image one segment that needs no merge, it
// costs 0.08 ms (5 %) more than that size.
constexpr int kDefaultSegment = 262144;
constexpr int kStripRows = 16;
constexpr int kHistBins = 180 * 256;          // uint32 counts per image, both hue halves
constexpr size_t kHistBytes = (size_t)kHistBins * 4;
constexpr size_t kAccumBytes = 1072;          // sizeof(StatsAccum), asserted in kernels_stats.hip
constexpr size_t kRecordBytes = 264 * 8;      // FE_STATS_DOUBLES doubles
using mixed_list::kAlign;                     // the arena's own alignment; every region and every image's planes start on it
using mixed_list::align_up;

// what the kernels read, in device memory; `img` counts from the chunk's first image
struct ImageDesc { const uint8_t* src; uint8_t* gray; int32_t h, w, nseg, pad; };
struct SegDesc { int32_t img; uint32_t p0, count; int32_t index; };      // pixels [p0, p0 + count) of the image; index: which of its segments
struct StripDesc { int32_t img, y0; };                                   // rows [y0, min(h, y0 + kStripRows))

// pass 1 launches 2 * segments workgroups: workgroup b works on segment b / 2 for hue half b % 2 (hue [0, 90) and [90, 180))
constexpr int pass1_segment(unsigned block) { return (int)(block >> 1); }
constexpr int pass1_half(unsigned block) { return (int)(block & 1); }

// byte offsets of a chunk's regions inside its one allocation
struct Layout {
  size_t accum = 0, hist = 0, zero_bytes = 0;      // [accum, accum + zero_bytes) is cleared by one memset and holds both
  size_t records = 0;
  size_t blob = 0, blob_bytes = 0;                 // ImageDesc[n], SegDesc[segs], StripDesc[strips], int32 multi[n_multi], back to back
  size_t blob_segs = 0, blob_strips = 0, blob_multi = 0;      // offsets inside the blob
  size_t gray = 0, stage = 0, total = 0;
};
inline Layout layout(size_t n, size_t segs, size_t strips, size_t n_multi, size_t gray_bytes, size_t stage_bytes) {
  Layout L;
  L.accum = 0;
  L.hist = align_up(n * kAccumBytes);
  L.zero_bytes = L.hist + n * kHistBytes;           // a multiple of 16: kHistBytes is one, L.hist one of 256
  L.records = align_up(L.zero_bytes);
  L.blob = align_up(L.records + n * kRecordBytes);
  L.blob_segs = n * sizeof(ImageDesc);
  L.blob_strips = L.blob_segs + segs * sizeof(SegDesc);
  L.blob_multi = L.blob_strips + strips * sizeof(StripDesc);
  L.blob_bytes = L.blob_multi + n_multi * sizeof(int32_t);
  L.gray = align_up(L.blob + L.blob_bytes);
  L.stage = L.gray + gray_bytes;                    // gray_bytes and stage_bytes are sums of align_up()s
  L.total = L.stage + stage_bytes;
  return L;
}

struct Chunk {
  int first = 0, count = 0;                  // images [first, first + count) of the list
  std::vector<size_t> gray_off, stage_off;   // per image, inside the gray / stage region (stage_off: host input only)
  std::vector<int32_t> nseg;                 // per image
  std::vector<SegDesc> segs;
  std::vector<StripDesc> strips;
  std::vector<int32_t> multi;                // images with more than one segment
  size_t gray_bytes = 0, stage_bytes = 0;
  Layout lay;
};

struct Plan {
  std::vector<Chunk> chunks;
  int bad_image = -1;          // >= 0: this image's own scratch exceeds the arena; chunks is empty
  size_t bad_bytes = 0;        // what it would need
};

namespace detail {
inline size_t segments_of(size_t npx, int segment_pixels) { return (npx + (size_t)segment_pixels - 1) / (size_t)segment_pixels; }
inline size_t strips_of(int h) { return ((size_t)h + kStripRows - 1) / kStripRows; }
}  // namespace detail

// hw [n][2] = h, w, all >= 1 with h * w < 2^31; segment_pixels a positive multiple of kSegmentUnit; staged: the pixels go through the
// arena as well (host input)
inline Plan build(const int32_t* hw, int n, bool staged, int segment_pixels, size_t arena_bytes) {
  Plan plan;
  for (int i0 = 0; i0 < n;) {
    Chunk cur;
    size_t segs = 0, strips = 0;
    cur.first = i0;
    // the step: an image joins while the chunk's layout with it fits the arena
    const mixed_list::Cut c = mixed_list::cut_chunk(i0, n, [&](int i, int, size_t& need) {
      const int h = hw[2 * i], w = hw[2 * i + 1];
      const size_t npx = (size_t)h * (size_t)w;
      const size_t s = detail::segments_of(npx, segment_pixels), r = detail::strips_of(h);
      const size_t g = align_up(npx), st = staged ? align_up(npx * 3) : 0;
      need = layout((size_t)cur.count + 1, segs + s, strips + r, cur.multi.size() + (s > 1 ? 1 : 0), cur.gray_bytes + g, cur.stage_bytes + st).total;
      if (need > arena_bytes) return false;
      const int32_t k = cur.count++;
      cur.gray_off.push_back(cur.gray_bytes);
      cur.stage_off.push_back(cur.stage_bytes);
      cur.gray_bytes += g;
      cur.stage_bytes += st;
      cur.nseg.push_back((int32_t)s);
      for (size_t q = 0; q < s; ++q) {
        const size_t p0 = q * (size_t)segment_pixels, left = npx - p0;
        cur.segs.push_back(SegDesc{k, (uint32_t)p0, (uint32_t)(left < (size_t)segment_pixels ? left : (size_t)segment_pixels), (int32_t)q});
      }
      for (size_t q = 0; q < r; ++q) cur.strips.push_back(StripDesc{k, (int32_t)(q * kStripRows)});
      if (s > 1) cur.multi.push_back(k);
      segs += s;
      strips += r;
      return true;
    });
    if (c.bad_image >= 0) return Plan{{}, c.bad_image, c.bad_bytes};
    cur.lay = layout((size_t)cur.count, segs, strips, cur.multi.size(), cur.gray_bytes, cur.stage_bytes);
    plan.chunks.push_back(std::move(cur));
    i0 = c.end;
  }
  return plan;
}

}  // namespace stats_plan
}  // namespace fe
