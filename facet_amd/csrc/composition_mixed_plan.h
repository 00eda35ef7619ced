// The plan of fe_leading_lines_mixed and fe_subject_region_mixed as data. Host only (no HIP headers): capi_image.hip executes it,
// kernels_composition_mixed.hip reads its descriptors, tests/native/composition_plan_harness.cpp checks it without a GPU.
//
// A list of images of any sizes is cut, in input order, into chunks whose scratch fits the arena. The planes of a chunk (blur / gray,
// gradient, magnitude, map, and for the subject call the labelling planes) are the images' planes back to back, unpadded: image k starts
// `px` pixels into every plane, px being the sum of h * w of the chunk's images before it. That is also where its bytes lie in the
// caller's flat edge buffer, so a plane goes down in one copy.
// No tile is described: a kernel's grid is 1-D over the tiles of all images, and a workgroup finds its image by bisecting the cumulative
// tile counts (`prefix`, n + 1 entries per tiling), then its tile inside the image from the remainder. One ImageDesc per image.
// One arena allocation per chunk, carved by Layout; descriptors and prefix tables go up as one blob.
#pragma once
#include "mixed_list.h"
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fe {
namespace comp_plan {

using mixed_list::kAlign;                            // the arena's own alignment; every region starts on it
using mixed_list::align_up;
constexpr size_t kMaxChunkPixels = ((size_t)1 << 31) - 1;      // pixel offsets and tile counts of a chunk stay below 2^31
constexpr int kGrayRun = 8192;                       // pixels per workgroup of the subject call's gray + histogram pass
constexpr int kWalkLanes = 64;                       // work-list entries per workgroup of the border walk

// the tilings; the blur's, Sobel's and the labelling's sizes are asserted against the kernels' in kernels_composition_mixed.hip
enum Tiling : int { kBlur = 0, kSobel = 1, kCcl = 2, kWalk = 3, kGray = 4, kTilings = 5 };
constexpr int kTileW[3] = {32, 64, 16}, kTileH[3] = {8, 4, 16};

// roots of 8-connected components are never neighbours of each other: at most one per 2x2 cell (contour_work_cap)
constexpr int work_cap(int h, int w) { return ((h + 1) / 2) * ((w + 1) / 2); }

// workgroups image h x w takes in tiling t
inline int32_t tiles_of(int t, int h, int w) {
  if (t == kWalk) return (work_cap(h, w) + kWalkLanes - 1) / kWalkLanes;
  if (t == kGray) return (int32_t)(((size_t)h * (size_t)w + kGrayRun - 1) / kGrayRun);
  return ((w + kTileW[t] - 1) / kTileW[t]) * ((h + kTileH[t] - 1) / kTileH[t]);
}

// what the kernels read, in device memory
struct ImageDesc {
  const uint8_t* src;      // packed [h][w][3], any byte alignment
  int32_t h, w;
  uint32_t px;             // where the image's planes start in the chunk's planes, in pixels
  uint32_t work;           // subject: where its work list starts in the chunk's, in entries
  int32_t cap;             // subject: work_cap(h, w)
  int32_t pad;
};

// byte offsets of a chunk's regions inside its one allocation; a region the call does not use has offset 0 and takes nothing
struct Layout {
  size_t blob = 0, blob_bytes = 0;           // ImageDesc[n], then kTilings prefix tables of n + 1 int32 each
  size_t blob_prefix = 0;                    // offset of the first table inside the blob
  size_t gray = 0;                           // [P] the blurred gray (lines) / the gray plane (subject)
  size_t grad = 0, mag = 0, map = 0;         // [P] short2, [P] uint16, [P] uint8
  // subject only. [zero, zero + zero_bytes) is cleared by one memset: cnt, strong, outer, the gray histograms, the counters
  size_t zero = 0, zero_bytes = 0;
  size_t cnt = 0, strong = 0, outer = 0;     // [P] int, [P] int, [P] uint8
  size_t hist = 0;                           // [n][256] uint32
  size_t counters = 0;                       // int32: work_count [n], rec_count [n], error, records stored
  size_t fill = 0;                           // xmin [P] int (0x7F7F7F7F), then xmax [P] and ymax [P] (-1): one fill kernel
  size_t thr = 0;                            // [n][2] int
  size_t lab_fg = 0, lab_bg = 0, edge = 0;   // [P] int, [P] int, [P] uint8
  size_t work = 0;                           // [W] int, W the sum of the images' work_cap
  size_t recs = 0;                           // [W][8] long long: the chunk's records in the order the walks finished, field 0 tagged
  size_t stage = 0;                          // host input: the images' pixels back to back, image k at 3 * px bytes
  size_t total = 0;
};
constexpr size_t counter_ints(size_t n) { return 2 * n + 2; }

// n images, P pixels, W work-list entries
inline Layout layout(size_t n, size_t P, size_t W, bool staged, bool subject) {
  Layout L;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t r = at; at = align_up(at + bytes); return r; };
  L.blob = take(0);
  L.blob_prefix = n * sizeof(ImageDesc);
  L.blob_bytes = L.blob_prefix + (size_t)kTilings * (n + 1) * sizeof(int32_t);
  take(L.blob_bytes);
  L.gray = take(P);
  L.grad = take(P * 4);
  L.mag = take(P * 2);
  L.map = take(P);
  if (subject) {
    L.zero = L.cnt = take(P * 4);
    L.strong = take(P * 4);
    L.outer = take(P);
    L.hist = take(n * 256 * 4);
    L.counters = take(counter_ints(n) * 4);
    L.zero_bytes = at - L.zero;
    L.fill = take(P * 4 * 3);
    L.thr = take(n * 2 * 4);
    L.lab_fg = take(P * 4);
    L.lab_bg = take(P * 4);
    L.edge = take(P);
    L.work = take(W * 4);
    L.recs = take(W * 8 * 8);
  }
  if (staged) L.stage = take(P * 3);
  L.total = at;
  return L;
}

struct Chunk {
  int first = 0, count = 0;                    // images [first, first + count) of the list
  std::vector<ImageDesc> descs;                // src is filled in by the caller
  std::vector<int32_t> prefix[kTilings];       // count + 1 entries each, [0] = 0
  size_t pixels = 0, work = 0;                 // P and W
  Layout lay;
};

struct Plan {
  std::vector<Chunk> chunks;
  int bad_image = -1;          // >= 0: this image's own scratch exceeds the arena; chunks is empty
  size_t bad_bytes = 0;        // what it would need
};

// hw [n][2] = h, w, all >= 1 with h * w < 2^30; staged: the pixels go through the arena as well (host input); subject: the plan of
// fe_subject_region_mixed, else of fe_leading_lines_mixed; max_chunk_pixels (at most kMaxChunkPixels): a chunk of several images holds
// no more pixels than this (an image alone may: h * w < 2^30 keeps it below kMaxChunkPixels)
inline Plan build(const int32_t* hw, int n, bool staged, bool subject, size_t arena_bytes, size_t max_chunk_pixels = kMaxChunkPixels) {
  Plan plan;
  for (int i0 = 0; i0 < n;) {
    Chunk cur;
    cur.first = i0;
    for (auto& p : cur.prefix) p.assign(1, 0);
    // the step: an image joins while the chunk's layout with it fits the arena and, behind the first, the pixel limit
    const mixed_list::Cut c = mixed_list::cut_chunk(i0, n, [&](int i, int held, size_t& need) {
      const int h = hw[2 * i], w = hw[2 * i + 1];
      const size_t npx = (size_t)h * (size_t)w, cap = (size_t)work_cap(h, w);
      need = layout((size_t)cur.count + 1, cur.pixels + npx, cur.work + cap, staged, subject).total;
      if (need > arena_bytes || (held > 0 && cur.pixels + npx > max_chunk_pixels)) return false;
      ++cur.count;
      cur.descs.push_back(ImageDesc{nullptr, h, w, (uint32_t)cur.pixels, (uint32_t)cur.work, (int32_t)cap, 0});
      for (int t = 0; t < kTilings; ++t) cur.prefix[t].push_back(cur.prefix[t].back() + tiles_of(t, h, w));
      cur.pixels += npx;
      cur.work += cap;
      return true;
    });
    if (c.bad_image >= 0) return Plan{{}, c.bad_image, c.bad_bytes};
    cur.lay = layout((size_t)cur.count, cur.pixels, cur.work, staged, subject);
    plan.chunks.push_back(std::move(cur));
    i0 = c.end;
  }
  return plan;
}

}  // namespace comp_plan
}  // namespace fe
