// Descriptors and coefficient pool of fe_phash_mixed as data. Host only (no HIP headers): capi_image.hip builds them, kernels_phash.hip
// reads them, tests/native/thumb_mixed_harness.cpp checks the pool without a GPU.
//
// One descriptor per image; stage 1 runs a wave per image row over the rows of all images of a chunk (`first_row` is the prefix sum of
// the heights, by which a wave finds its image), stage 2 one workgroup per image. The pool is one int32 array per call: for every
// distinct side length one block of 32 x ksize coefficients and one of 32 x 2 bounds - the (in, 32, LANCZOS) table of fe_phash, or the
// single-tap identity when the side is already 32 (PIL skips that pass; a tap of 1.0 reproduces a byte exactly). Descriptors address it
// by int32 offsets, two images with a side in common share a table, and nothing is cached per size.
#pragma once
#include "resize_coeffs.h"
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace fe {

constexpr int kPhashSide = 32;              // hash_size * highfreq_factor

// An image more than 100 times taller than wide: Image.resize makes two calls there, rows first ([h][w] -> [32][w]), then columns. Such an
// image has 32 rows of tmp instead of h: a kernel of its own runs both passes into them, and stage 2 applies the identity.
inline bool phash_tall(int h, int w) { return (long long)h > (long long)w * 100 && kPhashSide < h; }
inline int phash_tmp_rows(int h, int w) { return phash_tall(h, w) ? kPhashSide : h; }

struct PhashDesc {          // 64 bytes
  const uint8_t* src;       // [h][w][3], any alignment
  int32_t h, w;
  uint32_t first_row;       // tmp rows of the chunk's images before this one: row r of the image is row first_row + r of the chunk's tmp [rows][32]
  int32_t kh, bh, ksize_h;  // pool offsets of the horizontal coefficients [32][ksize_h] and bounds [32][2]
  int32_t kv, bv, ksize_v;  // the same for the vertical pass of stage 2; the identity for a tall image
  int32_t kt, bt, ksize_t;  // tall images: the (h, 32) table of the vertical pass that runs first
  int32_t tall;
};

class PhashTables {
 public:
  std::vector<int32_t> pool;
  size_t tables() const { return seen_.size(); }

  // the table of an axis of `in` samples; false: a window leaves the axis or the pool outgrows int32 offsets
  bool table(int in, int32_t& k_off, int32_t& b_off, int32_t& ksize) {
    auto it = seen_.find(in);
    if (it == seen_.end()) {
      std::vector<int> kk, bounds;
      int ks;
      if (in == kPhashSide) {
        ks = 1;
        kk.assign(kPhashSide, 1 << kResizePrecisionBits);
        bounds.resize(2 * kPhashSide);
        for (int i = 0; i < kPhashSide; ++i) { bounds[2 * i] = i; bounds[2 * i + 1] = 1; }
      } else {
        ks = pil_resize_coeffs(in, 0.0f, (float)in, kPhashSide, kFilterLanczos, kk, bounds);
      }
      if (ks <= 0) return false;
      for (int i = 0; i < kPhashSide; ++i)
        if (bounds[2 * i] < 0 || bounds[2 * i + 1] < 0 || bounds[2 * i + 1] > ks || bounds[2 * i] + bounds[2 * i + 1] > in) return false;
      if (pool.size() + (size_t)kPhashSide * (ks + 2) > (size_t)INT32_MAX) return false;
      Entry e;
      e.ksize = ks;
      e.k = (int32_t)pool.size();
      pool.insert(pool.end(), kk.begin(), kk.end());
      e.b = (int32_t)pool.size();
      pool.insert(pool.end(), bounds.begin(), bounds.end());
      it = seen_.emplace(in, e).first;
    }
    k_off = it->second.k; b_off = it->second.b; ksize = it->second.ksize;
    return true;
  }
  // both tables of an h x w image; src and first_row are the caller's
  bool describe(int h, int w, PhashDesc& d) {
    d = PhashDesc();
    d.h = h; d.w = w;
    if (h < 1 || w < 1 || !table(w, d.kh, d.bh, d.ksize_h)) return false;
    d.tall = phash_tall(h, w) ? 1 : 0;
    if (!d.tall) return table(h, d.kv, d.bv, d.ksize_v);
    return table(h, d.kt, d.bt, d.ksize_t) && table(kPhashSide, d.kv, d.bv, d.ksize_v);
  }

 private:
  struct Entry { int32_t k, b, ksize; };
  std::map<int, Entry> seen_;
};

}  // namespace fe
