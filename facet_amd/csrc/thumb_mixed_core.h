// Pillow's `Image.thumbnail` pixels for a LIST of images of any sizes: one descriptor per image, one launch per stage
// (kernels_jpeg.hip, fe_thumbnail_jpeg_mixed). Shared by host and device: the per-sample arithmetic below is what the kernels run, and
// tests/native/thumb_mixed_harness.cpp runs the same functions on the CPU from the same descriptors and table pool.
//
// Stages = thumbnail_run (capi_image.hip) per image: `Image.reduce` by integer factors over an integer box (libImaging/Reduce.c), then
// `Image.resize(size, LANCZOS, box)` with a fractional box (libImaging/Resample.c: 22-bit fixed-point coefficients, int32 accumulation
// from 1 << 21, a uint8 intermediate between the two passes). A pass whose axis keeps its size under a box that spans it is skipped, as
// ImagingResample skips it; an image more than 100 times taller than wide runs the vertical pass first (Image.resize's two calls).
//
// The table pool is one int32 array per call: for each distinct (input size, box start, box end, output size) one block of out x ksize
// coefficients and one of out x 2 bounds. Descriptors address it by int32 offsets, so the pool lives in call-scoped memory and nothing
// is cached per size.
#pragma once
#include "resize_coeffs.h"
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FE_THD __host__ __device__ __forceinline__
#else
#define FE_THD inline
#endif

namespace fe {

struct ThumbPass {          // one resampling pass over one axis; ksize = 0: skipped
  int32_t vertical;         // 0: along the rows (output oh = ih), 1: along the columns (output ow = iw)
  int32_t ih, iw, oh, ow;
  int32_t k, b, ksize;      // pool offsets of the coefficients [out][ksize] and the bounds [out][2] of the axis the pass works on
};

struct ThumbDesc {
  const uint8_t* src;       // [h][w][3], any alignment
  int32_t h, w;
  int32_t fx, fy;           // reduce factors; 1, 1: no reduce
  int32_t x0, y0, bw, bh;   // the reduce box: origin and size in source pixels
  int32_t rh, rw;           // size after the reduce (h, w without one)
  uint32_t m_in, m_col, m_row, m_cor;      // Reduce.c's multipliers: interior, last column, last row, corner
  ThumbPass pass[2];        // in the order they run
  int32_t oh, ow;           // size of the thumbnail
  uint8_t* red;             // [rh][rw][3], written by the reduce
  uint8_t* mid;             // output of pass[0] when pass[1] runs too
  uint8_t* pix;             // [oh][ow][3], output of the last pass that runs
};

FE_THD bool thumb_reduces(const ThumbDesc& d) { return d.fx > 1 || d.fy > 1; }
FE_THD const uint8_t* thumb_reduced(const ThumbDesc& d) { return thumb_reduces(d) ? d.red : d.src; }
FE_THD const uint8_t* thumb_pass_in(const ThumbDesc& d, int p) { return (p == 1 && d.pass[0].ksize) ? d.mid : thumb_reduced(d); }
FE_THD uint8_t* thumb_pass_out(const ThumbDesc& d, int p) { return (p == 0 && d.pass[1].ksize) ? d.mid : d.pix; }
// what the encoder reads: the source itself for an image that is encoded as it is
FE_THD const uint8_t* thumb_pixels(const ThumbDesc& d) { return (d.pass[0].ksize || d.pass[1].ksize) ? d.pix : thumb_reduced(d); }

// Reduce.c: the rounded mean of nx x ny samples from p on (rows row_stride bytes apart), ((sum + count / 2) * multiplier) >> 24
FE_THD void pil_reduce_pixel(const uint8_t* p, size_t row_stride, int nx, int ny, uint32_t mult, uint8_t out[3]) {
  uint32_t s0 = (uint32_t)(nx * ny) / 2, s1 = s0, s2 = s0;
  for (int yy = 0; yy < ny; ++yy) {
    const uint8_t* q = p + (size_t)yy * row_stride;
    for (int xx = 0; xx < nx; ++xx) { s0 += q[0]; s1 += q[1]; s2 += q[2]; q += 3; }
  }
  out[0] = (uint8_t)((s0 * mult) >> 24); out[1] = (uint8_t)((s1 * mult) >> 24); out[2] = (uint8_t)((s2 * mult) >> 24);
}

// Pixel (y, x) of the reduced image; the last column / row / corner average the samples that remain, with the count that remains
FE_THD void thumb_reduce_sample(const ThumbDesc& d, int y, int x, uint8_t out[3]) {
  const int xs = x * d.fx, ys = y * d.fy;
  const int nx = d.fx < d.bw - xs ? d.fx : d.bw - xs, ny = d.fy < d.bh - ys ? d.fy : d.bh - ys;      // > 0: rw = ceil(bw / fx)
  const uint32_t mult = nx == d.fx ? (ny == d.fy ? d.m_in : d.m_row) : (ny == d.fy ? d.m_col : d.m_cor);
  pil_reduce_pixel(d.src + ((size_t)(d.y0 + ys) * d.w + (d.x0 + xs)) * 3, (size_t)d.w * 3, nx, ny, mult, out);
}

// Output pixel (oy, ox) of a pass over `in` [ih][iw][3]
FE_THD void thumb_pass_sample(const ThumbPass& p, const int32_t* pool, const uint8_t* in, int oy, int ox, uint8_t out[3]) {
  const int o = p.vertical ? oy : ox;
  const int first = pool[p.b + o * 2], count = pool[p.b + o * 2 + 1];
  const int32_t* k = pool + p.k + (size_t)o * p.ksize;
  const uint8_t* q = p.vertical ? in + ((size_t)first * p.iw + ox) * 3 : in + ((size_t)oy * p.iw + first) * 3;
  const size_t stride = p.vertical ? (size_t)p.iw * 3 : 3;
  int s0 = 1 << (kResizePrecisionBits - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < count; ++t) {
    const int c = k[t];
    s0 += q[0] * c; s1 += q[1] * c; s2 += q[2] * c;
    q += stride;
  }
  out[0] = pil_clip8(s0); out[1] = pil_clip8(s1); out[2] = pil_clip8(s2);
}

}  // namespace fe

// ---- host side: descriptors and the table pool ------------------------------------------------------------------------------------
#include "mixed_list.h"
#include <algorithm>
#include <vector>

namespace fe {

// Reduce.c's multiplier of a mean over `count` samples: (uint32)(2^32 / (256 count)), the division taken in float
inline uint32_t pil_reduce_multiplier(int count) { return (uint32_t)(4294967296.0f / (float)(256u * (uint32_t)count)); }

// Builds the descriptors and the table pool of one call on the host. Tables are shared between images: a second image with the same
// (input size, box, output size) on an axis adds nothing to the pool.
class ThumbTables : public mixed_list::PilTablePool {
 public:
  // Geometry and tables of an h x w image under the plan of facet_amd.thumbnail.thumbnail_plan (fe_thumb_plan's fields); src and the
  // three buffers are the caller's. nullptr: described; otherwise what is wrong with the plan.
  const char* describe(int h, int w, int oh, int ow, int fx, int fy, const int32_t rbox[4], const float box[4], int tall, ThumbDesc& d) {
    d = ThumbDesc();
    if (h < 1 || w < 1) return "the image is empty";
    if (oh < 1 || ow < 1 || oh > 65535 || ow > 65535) return "the output size is not within 1 .. 65535";
    if (fx < 1 || fy < 1 || (long long)fx * fy > 65536) return "the reduce factors are not within 1 .. 65536 samples";      // 255 count + count / 2 < 2^32
    d.h = h; d.w = w; d.oh = oh; d.ow = ow; d.fx = fx; d.fy = fy; d.rh = h; d.rw = w; d.bw = w; d.bh = h;
    if (thumb_reduces(d)) {
      if (rbox[0] < 0 || rbox[1] < 0 || rbox[2] > w || rbox[3] > h || rbox[0] >= rbox[2] || rbox[1] >= rbox[3]) return "the reduce box is outside the image or empty";
      d.x0 = rbox[0]; d.y0 = rbox[1]; d.bw = rbox[2] - rbox[0]; d.bh = rbox[3] - rbox[1];
      d.rw = (d.bw + fx - 1) / fx; d.rh = (d.bh + fy - 1) / fy;
      const int rx = d.bw % fx ? d.bw % fx : fx, ry = d.bh % fy ? d.bh % fy : fy;
      d.m_in = pil_reduce_multiplier(fx * fy); d.m_col = pil_reduce_multiplier(rx * fy);
      d.m_row = pil_reduce_multiplier(fx * ry); d.m_cor = pil_reduce_multiplier(rx * ry);
    }
    const int rh = d.rh, rw = d.rw;
    if (oh == rh && ow == rw && box[0] == 0.0f && box[1] == 0.0f && box[2] == (float)rw && box[3] == (float)rh) return nullptr;      // no resize
    if (!(box[0] >= 0.0f && box[1] >= 0.0f && box[2] <= (float)rw && box[3] <= (float)rh && box[0] < box[2] && box[1] < box[3]))
      return "the resize box is outside the (reduced) image or empty";
    const bool need_h = ow != rw || box[0] != 0.0f || box[2] != (float)rw;
    const bool need_v = oh != rh || box[1] != 0.0f || box[3] != (float)rh;
    // Image.resize's two calls for a tall image: rows first, over all rw columns, then columns over the oh rows that gave
    ThumbPass hp = {0, tall ? oh : rh, rw, tall ? oh : rh, ow, 0, 0, 0};
    ThumbPass vp = {1, rh, tall ? rw : ow, oh, tall ? rw : ow, 0, 0, 0};
    if (need_h && !add(rw, box[0], box[2], ow, kFilterLanczos, 0, ow, hp.k, hp.b, hp.ksize)) return "a horizontal coefficient window leaves the axis";
    if (need_v && !add(rh, box[1], box[3], oh, kFilterLanczos, 0, oh, vp.k, vp.b, vp.ksize)) return "a vertical coefficient window leaves the axis";
    if (!need_v) { hp.ih = hp.oh = rh; }      // oh == rh then
    if (!need_h) { vp.iw = vp.ow = rw; }      // ow == rw then
    d.pass[0] = tall ? vp : hp;
    d.pass[1] = tall ? hp : vp;
    return nullptr;
  }
  // bytes of the three buffers of an image (0: not written)
  static size_t red_bytes(const ThumbDesc& d) { return thumb_reduces(d) ? (size_t)d.rh * d.rw * 3 : 0; }
  static size_t mid_bytes(const ThumbDesc& d) { return (d.pass[0].ksize && d.pass[1].ksize) ? (size_t)d.pass[0].oh * d.pass[0].ow * 3 : 0; }
  static size_t pix_bytes(const ThumbDesc& d) { return (d.pass[0].ksize || d.pass[1].ksize) ? (size_t)d.oh * d.ow * 3 : 0; }
};

// ---- the arena chunks of fe_thumbnail_jpeg_mixed ---------------------------------------------------------------------------------
// What the encoder takes per image, restated from jpeg_core.h so that this header stays free of it (kernels_jpeg.hip asserts the two
// constants): 6 blocks per 16 x 16 MCU, and per block 128 + 8 bytes of coefficients, bit length and offset plus its longest code in the
// bit buffer (a multiple of 16 bytes per image).
constexpr size_t kThumbItemBytes = 40, kThumbBlockCodeBytes = 208;      // sizeof(JpegItem), (BLOCK_MAX_BITS + 7) / 8
inline size_t thumb_jpeg_blocks(int oh, int ow) { return 6 * (size_t)((ow + 15) / 16) * (size_t)((oh + 15) / 16); }
// what thumbnails_mixed_launch carves from the arena for one image besides its output row
inline size_t thumb_mixed_scratch_bytes(const ThumbDesc& d) {
  using mixed_list::align_up;
  const size_t nblk = thumb_jpeg_blocks(d.oh, d.ow);
  return align_up(ThumbTables::red_bytes(d)) + align_up(ThumbTables::mid_bytes(d)) + align_up(ThumbTables::pix_bytes(d)) + nblk * (128 + 8) +
         ((nblk * kThumbBlockCodeBytes + 15) & ~(size_t)15) + sizeof(ThumbDesc) + kThumbItemBytes + 8;
}
// The chunks of the list (their ends) under the arena budget of thumbnail_run, pool_bytes of the arena being the call's tables. An image
// takes its output row of dcap bytes and its scratch (staged: its pixels too); when the chunk is done the scratch is dead and the
// gathered bytes (at most a row per image) take its place. At most 4096 images; an image alone whatever it needs (the arena refuses it
// if it must).
inline std::vector<int> thumb_mixed_cuts(const ThumbDesc* descs, int n, bool staged, size_t dcap, size_t arena_bytes, size_t pool_bytes) {
  const size_t whole = std::min<size_t>((size_t)1 << 30, arena_bytes - arena_bytes / 8), budget = whole > pool_bytes ? whole - pool_bytes : 0;
  size_t used = 0;
  return mixed_list::cut_list(n, [&](int) { used = 0; }, [&](int i, int held, size_t&) {
    const size_t stage = staged ? mixed_list::align_up((size_t)descs[i].h * descs[i].w * 3) : 0;
    const size_t need = dcap + std::max(thumb_mixed_scratch_bytes(descs[i]) + stage, dcap) + 4 * mixed_list::kAlign;
    if (held > 0 && (used + need > budget || held >= 4096)) return false;
    used += need;
    return true;
  }).ends;
}

}  // namespace fe
