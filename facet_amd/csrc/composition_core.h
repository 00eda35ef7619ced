// Device code the per-shape composition kernels (kernels_lines.hip, kernels_contours.hip) share with their mixed-size siblings
// (kernels_composition_mixed.hip): the per-pixel and per-tile bodies of the blur, Sobel, non-maximum suppression, union-find labelling,
// RETR_EXTERNAL test and border walk. Every function works on ONE image: the pointers it takes are that image's own planes and (x, y) or
// the tile index count inside it, so a border rule can only ever see the image's own edges. A kernel's job is to turn its block index
// into those pointers - from blockIdx.z and one shape there, from a descriptor found by bisection here.
#pragma once
#include "contour_core.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fe {

// ---- lines: gray, blur, Sobel, suppression ---------------------------------------------------------------------------------------------
// cv2 COLOR_BGR2GRAY in 15-bit fixed point (the weights kernels_stats.hip's gray_of uses as well)
__device__ __forceinline__ int lines_gray(int b, int g, int r) { return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15; }
__device__ __forceinline__ int lines_refl101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}
__device__ __forceinline__ int lines_clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

constexpr int LB_W = 32, LB_H = 8;      // the blur's tile; its block is LB_W x LB_H threads
constexpr int LS_W = 64, LS_H = 4;      // the tile of Sobel and suppression

// Tile (bx, by) of one image by a block of LB_W x LB_H threads: src [h][w][3] (kRgb: R,G,B bytes, else B,G,R) -> blur [h][w].
// Holds a __syncthreads: the whole block calls it.
template <bool kRgb>
__device__ __forceinline__ void lines_blur_tile(const uint8_t* __restrict__ src, int h, int w, int bx, int by, uint8_t* __restrict__ blur,
                                                int (&g)[LB_H + 4][LB_W + 4]) {
  const int x0 = bx * LB_W - 2, y0 = by * LB_H - 2;
  for (int i = threadIdx.y * LB_W + threadIdx.x; i < (LB_H + 4) * (LB_W + 4); i += LB_W * LB_H) {
    const int ty = i / (LB_W + 4), tx = i - ty * (LB_W + 4);
    const int y = lines_refl101(y0 + ty, h), x = lines_refl101(x0 + tx, w);
    const uint8_t* p = src + ((size_t)y * w + x) * 3;
    g[ty][tx] = kRgb ? lines_gray(p[2], p[1], p[0]) : lines_gray(p[0], p[1], p[2]);
  }
  __syncthreads();
  const int x = bx * LB_W + threadIdx.x, y = by * LB_H + threadIdx.y;
  if (x >= w || y >= h) return;
  const int k[5] = {1, 4, 6, 4, 1};
  int acc = 0;
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    int row = 0;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) row += k[dx] * g[threadIdx.y + dy][threadIdx.x + dx];
    acc += k[dy] * row;
  }
  blur[(size_t)y * w + x] = (uint8_t)((acc + 128) >> 8);
}

// pixel (x, y) of one image, x < w and y < h: 3x3 Sobel with a replicated border and the L1 magnitude
__device__ __forceinline__ void lines_sobel_px(const uint8_t* __restrict__ s, int h, int w, int x, int y, short2* __restrict__ grad,
                                               unsigned short* __restrict__ mag) {
  const int xm = lines_clampi(x - 1, w), xp = lines_clampi(x + 1, w), ym = lines_clampi(y - 1, h), yp = lines_clampi(y + 1, h);
  const int a = s[(size_t)ym * w + xm], b = s[(size_t)ym * w + x], c = s[(size_t)ym * w + xp];
  const int d = s[(size_t)y * w + xm], f = s[(size_t)y * w + xp];
  const int g = s[(size_t)yp * w + xm], hh = s[(size_t)yp * w + x], i = s[(size_t)yp * w + xp];
  const int dx = (c + 2 * f + i) - (a + 2 * d + g), dy = (g + 2 * hh + i) - (a + 2 * b + c);
  grad[(size_t)y * w + x] = make_short2((short)dx, (short)dy);
  mag[(size_t)y * w + x] = (unsigned short)(abs(dx) + abs(dy));
}

// pixel (x, y) of one image: non-maximum suppression along the quantised gradient direction and the two thresholds ->
// 2 = edge for sure, 0 = edge if connected to a 2, 1 = not an edge. The magnitude is zero outside the image.
__device__ __forceinline__ uint8_t lines_nms_px(const short2* __restrict__ grad, const unsigned short* __restrict__ mg, int h, int w, int x, int y,
                                                int low, int high) {
  auto M = [&](int yy, int xx) -> int { return (xx < 0 || xx >= w || yy < 0 || yy >= h) ? 0 : (int)mg[(size_t)yy * w + xx]; };   // zero outside
  const int m = mg[(size_t)y * w + x];
  uint8_t out = 1;
  if (m > low) {
    const short2 gr = grad[(size_t)y * w + x];
    const int xs = gr.x, ys = gr.y;
    const int ax = abs(xs), ay = abs(ys) << 15;
    const int tg22x = ax * 13573;                      // tan(22.5 deg) * 2^15, rounded
    bool peak;
    if (ay < tg22x) peak = m > M(y, x - 1) && m >= M(y, x + 1);                      // gradient ~horizontal
    else {
      const int tg67x = tg22x + (ax << 16);
      if (ay > tg67x) peak = m > M(y - 1, x) && m >= M(y + 1, x);                    // ~vertical
      else {
        const int s = (xs ^ ys) < 0 ? -1 : 1;                                        // diagonal the gradient points along
        peak = m > M(y - 1, x - s) && m > M(y + 1, x + s);
      }
    }
    if (peak) out = m > high ? 2 : 0;
  }
  return out;
}

// np.median of a uint8 image from its 256-bin histogram (counts of any arithmetic type), kept as twice the median (an even pixel count
// takes the mean of the two middle values), then lower = int(max(0, 0.5 median)) = m2 / 4 and upper = int(min(255, 1.5 median)) =
// min(255, 3 m2 / 4)
template <class Count>
__device__ __forceinline__ void median_thresholds_of(const Count* __restrict__ hist, long long npx, int* lower, int* upper) {
  const long long k_hi = npx / 2, k_lo = (npx & 1) ? k_hi : k_hi - 1;      // 0-based ranks of the middle values
  long long cum = 0;
  int v_lo = -1, v_hi = 255;
  for (int v = 0; v < 256; ++v) {
    cum += (long long)hist[v];
    if (v_lo < 0 && cum > k_lo) v_lo = v;
    if (cum > k_hi) { v_hi = v; break; }
  }
  if (v_lo < 0) v_lo = v_hi;
  const int m2 = v_lo + v_hi;
  *lower = m2 / 4;
  *upper = min(255, 3 * m2 / 4);
}

// smallest a with a * 5000 >= h * w: the reference keeps contours with area > h * w * 0.0001 (not strict here; subject_box is)
__host__ __device__ __forceinline__ long long subject_min_twice_area(long long npx) { return (npx + 4999) / 5000; }

// ---- contours: union-find labelling, the RETR_EXTERNAL test, the border walk ------------------------------------------------------------
constexpr int CT = 16;                                 // tile edge: 256 threads, 1 KB of LDS
enum { SET_CAND = 0, SET_FG = 1, SET_BG = 2 };         // which pixels are labelled: Canny candidates (!= 1), nonzero, zero

__device__ __forceinline__ bool in_set(int v, int mode) { return mode == SET_CAND ? v != 1 : (mode == SET_FG ? v != 0 : v == 0); }
__device__ __forceinline__ int ld(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ int find_root(const int* L, int i) {
  int p;
  while ((p = ld(L + i)) != i) i = p;                  // parents only ever decrease: the chain ends at a root
  return i;
}
// lock-free union, the larger root under the smaller one. When another thread re-parented `a` in between, what is left to join is
// a's previous parent and b.
__device__ __forceinline__ void unite(int* L, int a, int b) {
  for (;;) {
    a = find_root(L, a);
    b = find_root(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

// Tile (bx, by) of one image by a block of CT x CT threads: labels [h][w] <- the root of every pixel's component inside the tile as a
// pixel index of the image, -1 outside the set. L: CT * CT ints of LDS. Holds __syncthreads: the whole block calls it.
__device__ __forceinline__ void ccl_local_tile(const uint8_t* __restrict__ img, int h, int w, int mode, int conn8, int bx, int by,
                                               int* __restrict__ labels, int* L) {
  const int tx = threadIdx.x, ty = threadIdx.y, lid = ty * CT + tx;
  const int x = bx * CT + tx, y = by * CT + ty;
  const bool inside = x < w && y < h;
  const bool s = inside && in_set(img[(size_t)y * w + x], mode);
  L[lid] = s ? lid : -1;
  __syncthreads();
  if (s) {                                             // the neighbours that come before this pixel in raster order, inside the tile
    if (tx > 0 && ld(L + lid - 1) >= 0) unite(L, lid, lid - 1);
    if (ty > 0) {
      if (ld(L + lid - CT) >= 0) unite(L, lid, lid - CT);
      if (conn8) {
        if (tx > 0 && ld(L + lid - CT - 1) >= 0) unite(L, lid, lid - CT - 1);
        if (tx < CT - 1 && ld(L + lid - CT + 1) >= 0) unite(L, lid, lid - CT + 1);
      }
    }
  }
  __syncthreads();
  if (!inside) return;
  int out = -1;
  if (s) {                                             // tile order is raster order: the smallest local index is the smallest global one
    const int r = find_root(L, lid);
    out = (by * CT + r / CT) * w + bx * CT + r % CT;
  }
  labels[(size_t)y * w + x] = out;
}

// pixel (x, y) = tile (bx, by), thread (threadIdx.x, threadIdx.y): pixels on a tile edge unite with their neighbours across it
__device__ __forceinline__ void ccl_seam_px(int h, int w, int conn8, int bx, int by, int* __restrict__ L) {
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int x = bx * CT + tx, y = by * CT + ty;
  if (x >= w || y >= h) return;
  const int p = y * w + x;
  if (ld(L + p) < 0) return;
  if (tx == 0 && x > 0 && ld(L + p - 1) >= 0) unite(L, p, p - 1);
  if (y > 0) {
    if (ty == 0 && ld(L + p - w) >= 0) unite(L, p, p - w);
    if (conn8) {
      if ((tx == 0 || ty == 0) && x > 0 && ld(L + p - w - 1) >= 0) unite(L, p, p - w - 1);
      if ((tx == CT - 1 || ty == 0) && x + 1 < w && ld(L + p - w + 1) >= 0) unite(L, p, p - w + 1);
    }
  }
}

// every plane is the image's own [h][w]
__device__ __forceinline__ void ccl_flatten_fg_px(const uint8_t* __restrict__ img, int h, int w, int mode, int x, int y, int* __restrict__ L,
                                                  int* __restrict__ cnt, int* __restrict__ strong, int* __restrict__ xmin, int* __restrict__ xmax,
                                                  int* __restrict__ ymax) {
  if (x >= w || y >= h) return;
  const int p = y * w + x;
  if (ld(L + p) < 0) return;
  const int r = find_root(L, p);
  __atomic_store_n(L + p, r, __ATOMIC_RELAXED);        // a reader that still sees the old parent reaches the same root
  atomicAdd(cnt + r, 1);
  atomicMin(xmin + r, x);
  atomicMax(xmax + r, x);
  atomicMax(ymax + r, y);
  if (mode == SET_FG ? p == r : img[p] == 2) __atomic_store_n(strong + r, 1, __ATOMIC_RELAXED);
}

__device__ __forceinline__ void ccl_flatten_bg_px(int h, int w, int x, int y, int* __restrict__ L, uint8_t* __restrict__ outer) {
  if (x >= w || y >= h) return;
  const int p = y * w + x;
  if (ld(L + p) < 0) return;
  const int r = find_root(L, p);
  __atomic_store_n(L + p, r, __ATOMIC_RELAXED);
  if (x == 0 || y == 0 || x == w - 1 || y == h - 1) outer[r] = 1;      // every writer stores the same byte
}

__device__ __forceinline__ uint8_t contour_edge_px(const int* __restrict__ labels, const int* __restrict__ strong, size_t p) {
  const int l = labels[p];
  return (l >= 0 && strong[l]) ? 255 : 0;
}

// pixel (x, y) of one image: when it is the root of a kept component that is external and whose bounding box can hold min_twice_area,
// it takes a slot of the image's work list (work [work_cap], *work_count)
__device__ __forceinline__ void contour_candidate_px(int h, int w, int x, int y, long long min_twice_area, const int* __restrict__ lab_fg,
                                                     const int* __restrict__ lab_bg, const int* __restrict__ strong, const int* __restrict__ xmin,
                                                     const int* __restrict__ xmax, const int* __restrict__ ymax, const uint8_t* __restrict__ outer,
                                                     int* __restrict__ work, int* __restrict__ work_count, int work_cap, int* __restrict__ error) {
  if (x >= w || y >= h) return;
  const int p = y * w + x;
  if (lab_fg[p] != p || !strong[p]) return;                    // roots of kept components only
  bool external = x == 0;
  if (!external) {
    const int lb = lab_bg[p - 1];                               // the left neighbour of a first raster pixel is background
    external = lb >= 0 && outer[lb];
  }
  if (!external) return;
  // |a00| of a polygon is at most twice the area of its bounding rectangle through the pixel centres
  const long long bw = xmax[p] - xmin[p], bh = ymax[p] - y;
  if (2 * bw * bh < min_twice_area) return;
  const int slot = atomicAdd(work_count, 1);
  if (slot < work_cap) work[slot] = p;
  else atomicOr(error, 2);
}

// The border walk of the component rooted at pixel p of one image. true: the contour qualifies and r [8] holds its record
// (start_index, a00, a10, a01, x_min, y_min, x_max, y_max). A walk that does not close within 8 * pixels + 8 steps sets bit 0 of *error.
__device__ __forceinline__ bool contour_walk_one(const uint8_t* __restrict__ im, int h, int w, int p, long long min_twice_area,
                                                 const int* __restrict__ cnt, const int* __restrict__ xmin, const int* __restrict__ xmax,
                                                 const int* __restrict__ ymax, int* __restrict__ error, long long r[8]) {
  const int x0 = p % w, y0 = p / w;
  auto fg = [&](int x, int y) { return x >= 0 && x < w && y >= 0 && y < h && im[(size_t)y * w + x] != 0; };
  contour::Sums a;
  const long long steps = contour::follow_outer(fg, x0, y0, 8ll * cnt[p] + 8, &a);
  if (steps < 0) { atomicOr(error, 1); return false; }
  const long long twice = a.a00 < 0 ? -a.a00 : a.a00;
  if (twice < min_twice_area) return false;
  r[0] = p; r[1] = a.a00; r[2] = a.a10; r[3] = a.a01;
  r[4] = xmin[p]; r[5] = y0; r[6] = xmax[p]; r[7] = ymax[p];
  return true;
}

}  // namespace fe
