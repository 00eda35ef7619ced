// What the plans of the mixed-size calls share: the arena's alignment, the greedy cut of a list into chunks, the staged offsets of a
// chunk's host images and the pool of Pillow's resampling tables. Host only (no HIP headers): the plan headers build on it,
// capi_internal.h has the device half, tests/native/mixed_list_harness.cpp checks it without a GPU.
#pragma once
#include "resize_coeffs.h"
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

namespace fe {
namespace mixed_list {

constexpr size_t kAlign = 256;
constexpr size_t align_up(size_t v) { return (v + kAlign - 1) & ~(kAlign - 1); }
inline size_t image_bytes(const int32_t* hw, int i) { return (size_t)hw[2 * i] * (size_t)hw[2 * i + 1] * 3; }

// One chunk of a greedy cut: images [i0, end). bad_image >= 0 (then end == i0): image i0 does not fit a chunk of its own, which would
// take bad_bytes.
struct Cut { int end = 0, bad_image = -1; size_t bad_bytes = 0; };
// The chunk that starts at image i0 of n. fits(i, held, need) is asked for i = i0, i0 + 1, ... with `held` = i - i0 images in the chunk:
// true - image i joined (the step, which owns the running sums and limits, has added it); false - it did not and the chunk ends before
// it, the step's state unchanged. A step that refuses an image for an empty chunk stores what the image alone would take in `need`. So a
// chunk holds at least one image, or names the image that cannot stand alone.
template <class Fits>
Cut cut_chunk(int i0, int n, Fits&& fits) {
  Cut c;
  for (c.end = i0; c.end < n; ++c.end) {
    size_t need = 0;
    if (fits(c.end, c.end - i0, need)) continue;
    if (c.end == i0) { c.bad_image = i0; c.bad_bytes = need; }
    break;
  }
  return c;
}

// The ends of all chunks of a list, for the steps that keep no more per chunk: open(i0) resets the step's state before each. With a bad
// image `ends` is empty.
struct Cuts { std::vector<int> ends; int bad_image = -1; size_t bad_bytes = 0; };
template <class Open, class Fits>
Cuts cut_list(int n, Open&& open, Fits&& fits) {
  Cuts r;
  for (int i0 = 0; i0 < n; i0 = r.ends.back()) {
    open(i0);
    const Cut c = cut_chunk(i0, n, fits);
    if (c.bad_image >= 0) return Cuts{{}, c.bad_image, c.bad_bytes};
    r.ends.push_back(c.end);
  }
  return r;
}

// Where images [i0, i1) lie in a stage region, one behind the other: each on a kAlign boundary (aligned) or packed. off [i1 - i0];
// returns the bytes of the region.
inline size_t staged_offsets(const int32_t* hw, int i0, int i1, bool aligned, std::vector<size_t>& off) {
  off.resize((size_t)(i1 - i0));
  size_t at = 0;
  for (int i = i0; i < i1; ++i) {
    off[i - i0] = at;
    at += aligned ? align_up(image_bytes(hw, i)) : image_bytes(hw, i);
  }
  return at;
}

// The tables of one call: per distinct key one block of count x ksize coefficients, then one of count x 2 bounds. Descriptors address
// the pool by int32 offsets, so it lives in call-scoped memory and nothing is cached per size.
class PilTablePool {
 public:
  std::vector<int32_t> pool;
  size_t tables() const { return seen_.size(); }

  // Output samples [first, first + count) of pil_resize_coeffs(in, in0, in1, out, filter). false: the range leaves the table, a window
  // leaves the axis or the pool outgrows int32 offsets.
  bool add(int in, float in0, float in1, int out, int filter, int first, int count, int32_t& k_off, int32_t& b_off, int32_t& ksize) {
    uint32_t b0, b1;
    memcpy(&b0, &in0, 4); memcpy(&b1, &in1, 4);
    const Key key(in, b0, b1, out, filter, first, count);
    auto it = seen_.find(key);
    if (it == seen_.end()) {
      std::vector<int> kk, bounds;
      const int ks = pil_resize_coeffs(in, in0, in1, out, filter, kk, bounds);
      if (ks <= 0 || first < 0 || count < 0 || first + count > out) return false;
      it = store(key, in, count, ks, kk.data() + (size_t)first * ks, bounds.data() + (size_t)first * 2);
    }
    return give(it, k_off, b_off, ksize);
  }
  // `side` single taps of 1.0, each on its own sample: what a pass that PIL skips amounts to (a tap of 1.0 reproduces a byte exactly)
  bool add_identity(int side, int32_t& k_off, int32_t& b_off, int32_t& ksize) {
    const Key key(side, 0u, 0u, side, kIdentity, 0, side);
    auto it = seen_.find(key);
    if (it == seen_.end()) {
      std::vector<int> kk((size_t)side, 1 << kResizePrecisionBits), bounds((size_t)side * 2);
      for (int i = 0; i < side; ++i) { bounds[2 * i] = i; bounds[2 * i + 1] = 1; }
      it = store(key, side, side, 1, kk.data(), bounds.data());
    }
    return give(it, k_off, b_off, ksize);
  }

 private:
  static constexpr int kIdentity = -1;      // no FE_FILTER_* number
  struct Entry { int32_t k, b, ksize; };
  using Key = std::tuple<int, uint32_t, uint32_t, int, int, int, int>;      // in, the bits of in0 and in1, out, filter, first, count
  using Seen = std::map<Key, Entry>;
  // appends a checked table; seen_.end(): refused
  Seen::iterator store(const Key& key, int in, int count, int ks, const int* kk, const int* bounds) {
    for (int i = 0; i < count; ++i)
      if (bounds[i * 2] < 0 || bounds[i * 2 + 1] < 0 || bounds[i * 2 + 1] > ks || bounds[i * 2] + bounds[i * 2 + 1] > in) return seen_.end();
    if (pool.size() + (size_t)count * (ks + 2) > (size_t)INT32_MAX) return seen_.end();
    Entry e;
    e.ksize = ks;
    e.k = (int32_t)pool.size();
    pool.insert(pool.end(), kk, kk + (size_t)count * ks);
    e.b = (int32_t)pool.size();
    pool.insert(pool.end(), bounds, bounds + (size_t)count * 2);
    return seen_.emplace(key, e).first;
  }
  bool give(Seen::iterator it, int32_t& k_off, int32_t& b_off, int32_t& ksize) const {
    if (it == seen_.end()) return false;
    k_off = it->second.k; b_off = it->second.b; ksize = it->second.ksize;
    return true;
  }
  Seen seen_;
};

}  // namespace mixed_list
}  // namespace fe
