// Descriptors and coefficient pool of fe_phash_mixed as data. Host only (no HIP headers): capi_image.hip builds them, kernels_phash.hip
// reads them, tests/native/thumb_mixed_harness.cpp checks the pool without a GPU.
//
// One descriptor per image; stage 1 runs a wave per image row over the rows of all images of a chunk (`first_row` is the prefix sum of
// the heights, by which a wave finds its image), stage 2 one workgroup per image. The pool is one int32 array per call: for every
// distinct side length one block of 32 x ksize coefficients and one of 32 x 2 bounds - the (in, 32, LANCZOS) table of fe_phash, or the
// single-tap identity when the side is already 32 (PIL skips that pass; a tap of 1.0 reproduces a byte exactly). Descriptors address it
// by int32 offsets, two images with a side in common share a table, and nothing is cached per size.
#pragma once
#include "mixed_list.h"
#include <cstddef>
#include <cstdint>
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

class PhashTables : public mixed_list::PilTablePool {
 public:
  // the table of an axis of `in` samples; false: a window leaves the axis or the pool outgrows int32 offsets
  bool table(int in, int32_t& k_off, int32_t& b_off, int32_t& ksize) {
    if (in == kPhashSide) return add_identity(kPhashSide, k_off, b_off, ksize);
    return add(in, 0.0f, (float)in, kPhashSide, kFilterLanczos, 0, kPhashSide, k_off, b_off, ksize);
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
};

// ---- the arena chunks of fe_phash_mixed ------------------------------------------------------------------------------------------
// what an image takes of a chunk besides the pool: its rows of tmp, its descriptor and outputs and, from the host, its staged pixels
inline size_t phash_need(int h, int w, bool small, bool dct, bool staged) {
  return (size_t)phash_tmp_rows(h, w) * kPhashSide + sizeof(PhashDesc) + sizeof(uint64_t) + (small ? 1024 : 0) + (dct ? 64 * sizeof(double) : 0) +
         (staged ? mixed_list::align_up((size_t)h * (size_t)w * 3) : 0);
}
// A chunk holds what fits the arena beside the pool (and 8 alignments of slack for the chunk's allocations), at most 2^30 rows of tmp and
// 65535 images. The ends of the chunks, or the image whose own need exceeds the arena.
inline mixed_list::Cuts phash_cuts(const int32_t* hw, int n, bool small, bool dct, bool staged, size_t pool_words, size_t arena_bytes) {
  const size_t fixed = mixed_list::align_up(pool_words * sizeof(int32_t)) + 8 * mixed_list::kAlign;
  const size_t room = arena_bytes > fixed ? arena_bytes - fixed : 0;
  size_t used = 0, rows = 0;
  return mixed_list::cut_list(n, [&](int) { used = rows = 0; }, [&](int i, int held, size_t& need) {
    const size_t b = phash_need(hw[2 * i], hw[2 * i + 1], small, dct, staged), r = (size_t)phash_tmp_rows(hw[2 * i], hw[2 * i + 1]);
    need = b + fixed;
    if (held == 0 ? b > room : (used + b > room || rows + r > ((size_t)1 << 30) || held >= 65535)) return false;
    used += b;
    rows += r;
    return true;
  });
}

}  // namespace fe
