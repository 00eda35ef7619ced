// The plan of the mixed-size face calls (fe_face_analyze_mixed and the calls beside it) as data. Host only (no HIP headers): capi_face.hip
// executes it, kernels_face_mixed.hip and kernels_face_thumb.hip read its descriptors, tests/native/face_plan_harness.cpp checks it without
// a GPU.
//
// One ImageDesc per image says where its pixels are and how SCRFD.detect fits it into the det_h x det_w canvas: the aspect-preserving
// size (new_h, new_w), which of cv2.resize's three INTER_LINEAR routes that is (the weighted one, the exact-2x box average, a plain
// copy), where its two weight tables start in the call's pool and the det_scale the decode divides by. The weight tables of a call, one
// per distinct (source length, target length, clamp), lie in one pool of int32 words: per table `dst` source offsets, then `dst` pairs
// of 11-bit weights (two shorts per word). The pool is made per call and uploaded into the arena; nothing is kept per size.
//
// A list is walked in input order in micro-batches of at most `max_images`; with host input a micro-batch also ends before the image
// whose staged bytes (each image on a 256-byte boundary) would pass `stage_room`.
#pragma once
#include "mixed_list.h"
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace fe {
namespace face_plan {

enum Mode : int32_t { kResize = 0, kBox2 = 1, kCopy = 2 };
using mixed_list::kAlign;           // the arena's alignment; every staged image starts on it
using mixed_list::align_up;
constexpr size_t staged_bytes(int h, int w) { return align_up((size_t)h * (size_t)w * 3); }

// what the kernels read, in device memory. The calls that do not run the detector (crops, ROIs, thumbnails) fill src, h and w only.
struct ImageDesc {
  const uint8_t* src;
  int32_t h, w, new_h, new_w, mode;
  int32_t xtab, ytab;      // int32 words into the pool: the column table (borders folded into the weights) and the row table
  float det_scale;
};

// SCRFD.detect's fit of an h x w image into the det_h x det_w canvas, in its fp32 arithmetic (insightface model_zoo/scrfd.py). false:
// the aspect ratio leaves an empty detector input (new_h or new_w is 0).
inline bool fit(int h, int w, int det_h, int det_w, int32_t& new_h, int32_t& new_w, float& det_scale, int32_t& mode) {
  const float im_ratio = (float)h / (float)w, model_ratio = (float)det_h / (float)det_w;
  if (im_ratio > model_ratio) { new_h = det_h; new_w = (int)((float)new_h / im_ratio); }
  else { new_w = det_w; new_h = (int)((float)new_w * im_ratio); }
  det_scale = new_h > 0 ? (float)new_h / (float)h : 0.f;
  mode = (h == new_h && w == new_w) ? kCopy : ((h == 2 * new_h && w == 2 * new_w) ? kBox2 : kResize);
  return new_h > 0 && new_w > 0;
}

// cv::resize's coefficient precomputation (kernels_face.hip: cv_resize_tables)
using TableFn = void (*)(int src, int dst, bool clamp_fx, std::vector<int>& ofs, std::vector<short>& coef);

// The weight tables of one call. add() returns the table's first word; a (src, dst, clamp) seen before costs nothing.
struct TablePool {
  std::vector<int32_t> words;
  std::map<std::pair<std::pair<int, int>, int>, int32_t> at;
  int32_t add(int src, int dst, bool clamp, TableFn make) {
    const auto key = std::make_pair(std::make_pair(src, dst), clamp ? 1 : 0);
    const auto it = at.find(key);
    if (it != at.end()) return it->second;
    std::vector<int> ofs;
    std::vector<short> coef;
    make(src, dst, clamp, ofs, coef);
    const int32_t first = (int32_t)words.size();
    words.insert(words.end(), ofs.begin(), ofs.end());
    for (int d = 0; d < dst; ++d) words.push_back((int32_t)((uint32_t)(uint16_t)coef[2 * d] | ((uint32_t)(uint16_t)coef[2 * d + 1] << 16)));
    return at[key] = first;
  }
  size_t tables() const { return at.size(); }
};

// Descriptor of image i of hw [n][2] = h, w (both >= 1) without its pointer; the tables of the weighted route go into `pool`. false:
// fit() failed.
inline bool describe(const int32_t* hw, int i, int det_h, int det_w, TablePool& pool, TableFn make, ImageDesc& d) {
  d.src = nullptr;
  d.h = hw[2 * i]; d.w = hw[2 * i + 1];
  d.xtab = d.ytab = 0;
  if (!fit(d.h, d.w, det_h, det_w, d.new_h, d.new_w, d.det_scale, d.mode)) return false;
  if (d.mode == kResize) {
    d.xtab = pool.add(d.w, d.new_w, true, make);
    d.ytab = pool.add(d.h, d.new_h, false, make);
  }
  return true;
}

// The micro-batch that starts at image i0: at most max_images images and, staged, at most stage_room bytes (*bytes, nullable, receives
// their sum). bad_image: image i0's staged bytes alone exceed stage_room.
inline mixed_list::Cut chunk(const int32_t* hw, int n, int i0, int max_images, bool staged, size_t stage_room, size_t* bytes) {
  size_t used = 0;
  const mixed_list::Cut c = mixed_list::cut_chunk(i0, n, [&](int i, int held, size_t& need) {
    need = staged ? staged_bytes(hw[2 * i], hw[2 * i + 1]) : 0;
    if (held >= max_images || used + need > stage_room) return false;
    used += need;
    return true;
  });
  if (bytes) *bytes = used;
  return c;
}

// The first image of the list whose staged bytes alone exceed stage_room, or -1. Resident input stages nothing.
inline int too_large(const int32_t* hw, int n, bool staged, size_t stage_room) {
  int bad = -1;
  for (int i0 = 0; staged && bad < 0 && i0 < n;) {
    const mixed_list::Cut c = chunk(hw, n, i0, n, staged, stage_room, nullptr);
    bad = c.bad_image;
    i0 = c.end;
  }
  return bad;
}

// The end i1 of the micro-batch that starts at image i0 (i0 < i1 <= n). offsets (nullable) receives the byte offset of every image of
// the micro-batch inside the stage region. Every image must pass too_large() first: then a micro-batch holds at least one image.
inline int cut(const int32_t* hw, int n, int i0, int max_images, bool staged, size_t stage_room, std::vector<size_t>* offsets, size_t* bytes) {
  const int i1 = chunk(hw, n, i0, max_images, staged, stage_room, bytes).end;
  if (offsets) {
    if (staged) mixed_list::staged_offsets(hw, i0, i1, true, *offsets);
    else offsets->assign((size_t)(i1 - i0), 0);
  }
  return i1;
}

}  // namespace face_plan
}  // namespace fe
