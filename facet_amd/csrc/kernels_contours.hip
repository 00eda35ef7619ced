// Subject-region detection (reference analyzers/composition.py:16-93: cv2.Canny(gray, 0.5 median, 1.5 median) ->
// cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) -> contourArea / moments / boundingRect of every contour). Nothing after the
// Canny map depends on an order, so all of it stays on the device and only a few records per image go back:
//   ccl_local_kernel      union-find labelling of one 16x16 tile in LDS; a component's root is its smallest pixel index
//   ccl_seam_kernel       joins the tiles: pixels on a tile edge unite with their neighbours across it (atomic min on the parent)
//   ccl_flatten_*_kernel  every pixel takes its root; foreground roots collect pixel count, bounding box and the has-a-strong-pixel
//                         flag (hysteresis = keep the components of the candidate map that own a strong pixel, which is what a
//                         flood fill from the strong pixels reaches); background roots note whether they touch the image frame
//   contour_candidates_kernel   RETR_EXTERNAL: a component is external iff the pixel left of its first raster pixel lies outside the
//                         image or in a 4-connected background region that reaches the frame; plus the bounding-box area bound
//   contour_walk_kernel   one lane per remaining component follows its outer border (contour_core.h) and sums a00, a10, a01
// [DEP-KNOWLEDGE] OpenCV is not available offline: these restate its documented algorithms; parity with cv2 is unpinned.
#include "contour_core.h"
#include "fe_common.h"

namespace fe {

namespace {

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

__global__ __launch_bounds__(CT * CT) void ccl_local_kernel(const uint8_t* __restrict__ img, int h, int w, int mode, int conn8,
                                                            int* __restrict__ labels) {
  __shared__ int L[CT * CT];
  const int tx = threadIdx.x, ty = threadIdx.y, lid = ty * CT + tx;
  const int x = blockIdx.x * CT + tx, y = blockIdx.y * CT + ty;
  const size_t base = (size_t)blockIdx.z * h * w;
  const bool inside = x < w && y < h;
  const bool s = inside && in_set(img[base + (size_t)y * w + x], mode);
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
    out = (blockIdx.y * CT + r / CT) * w + blockIdx.x * CT + r % CT;
  }
  labels[base + (size_t)y * w + x] = out;
}

__global__ __launch_bounds__(CT * CT) void ccl_seam_kernel(int h, int w, int conn8, int* __restrict__ labels) {
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int x = blockIdx.x * CT + tx, y = blockIdx.y * CT + ty;
  if (x >= w || y >= h) return;
  int* L = labels + (size_t)blockIdx.z * h * w;
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

__global__ __launch_bounds__(CT * CT) void ccl_flatten_fg_kernel(const uint8_t* __restrict__ img, int h, int w, int mode, int* __restrict__ labels,
                                                                 int* __restrict__ cnt, int* __restrict__ strong, int* __restrict__ xmin,
                                                                 int* __restrict__ xmax, int* __restrict__ ymax) {
  const int x = blockIdx.x * CT + threadIdx.x, y = blockIdx.y * CT + threadIdx.y;
  if (x >= w || y >= h) return;
  const size_t base = (size_t)blockIdx.z * h * w;
  int* L = labels + base;
  const int p = y * w + x;
  if (ld(L + p) < 0) return;
  const int r = find_root(L, p);
  __atomic_store_n(L + p, r, __ATOMIC_RELAXED);        // a reader that still sees the old parent reaches the same root
  atomicAdd(cnt + base + r, 1);
  atomicMin(xmin + base + r, x);
  atomicMax(xmax + base + r, x);
  atomicMax(ymax + base + r, y);
  if (mode == SET_FG ? p == r : img[base + p] == 2) __atomic_store_n(strong + base + r, 1, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(CT * CT) void ccl_flatten_bg_kernel(int h, int w, int* __restrict__ labels, uint8_t* __restrict__ outer) {
  const int x = blockIdx.x * CT + threadIdx.x, y = blockIdx.y * CT + threadIdx.y;
  if (x >= w || y >= h) return;
  const size_t base = (size_t)blockIdx.z * h * w;
  int* L = labels + base;
  const int p = y * w + x;
  if (ld(L + p) < 0) return;
  const int r = find_root(L, p);
  __atomic_store_n(L + p, r, __ATOMIC_RELAXED);
  if (x == 0 || y == 0 || x == w - 1 || y == h - 1) outer[base + r] = 1;      // every writer stores the same byte
}

__global__ void contour_edge_kernel(const int* __restrict__ labels, const int* __restrict__ strong, size_t npx, uint8_t* __restrict__ edge) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  const size_t base = (size_t)blockIdx.y * npx;
  const int l = labels[base + p];
  edge[base + p] = (l >= 0 && strong[base + l]) ? 255 : 0;
}

__global__ __launch_bounds__(CT * CT) void contour_candidates_kernel(int h, int w, long long min_twice_area, const int* __restrict__ lab_fg,
                                                                     const int* __restrict__ lab_bg, const int* __restrict__ strong,
                                                                     const int* __restrict__ xmin, const int* __restrict__ xmax,
                                                                     const int* __restrict__ ymax, const uint8_t* __restrict__ outer,
                                                                     int* __restrict__ work, int* __restrict__ work_count, int work_cap,
                                                                     int* __restrict__ error) {
  const int x = blockIdx.x * CT + threadIdx.x, y = blockIdx.y * CT + threadIdx.y;
  if (x >= w || y >= h) return;
  const int img = blockIdx.z;
  const size_t base = (size_t)img * h * w;
  const int p = y * w + x;
  if (lab_fg[base + p] != p || !strong[base + p]) return;      // roots of kept components only
  bool external = x == 0;
  if (!external) {
    const int lb = lab_bg[base + p - 1];                        // the left neighbour of a first raster pixel is background
    external = lb >= 0 && outer[base + lb];
  }
  if (!external) return;
  // |a00| of a polygon is at most twice the area of its bounding rectangle through the pixel centres
  const long long bw = xmax[base + p] - xmin[base + p], bh = ymax[base + p] - y;
  if (2 * bw * bh < min_twice_area) return;
  const int slot = atomicAdd(work_count + img, 1);
  if (slot < work_cap) work[(size_t)img * work_cap + slot] = p;
  else atomicOr(error, 2);
}

__global__ __launch_bounds__(64) void contour_walk_kernel(const uint8_t* __restrict__ fgimg, int h, int w, long long min_twice_area,
                                                          const int* __restrict__ cnt, const int* __restrict__ xmin, const int* __restrict__ xmax,
                                                          const int* __restrict__ ymax, const int* __restrict__ work,
                                                          const int* __restrict__ work_count, int work_cap, long long* __restrict__ recs,
                                                          int* __restrict__ rec_count, int* __restrict__ error) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, img = blockIdx.y;
  const int nwork = min(work_count[img], work_cap);
  if (j >= nwork) return;
  const size_t base = (size_t)img * h * w;
  const uint8_t* im = fgimg + base;
  const int p = work[(size_t)img * work_cap + j];
  const int x0 = p % w, y0 = p / w;
  auto fg = [&](int x, int y) { return x >= 0 && x < w && y >= 0 && y < h && im[(size_t)y * w + x] != 0; };
  contour::Sums a;
  const long long steps = contour::follow_outer(fg, x0, y0, 8ll * cnt[base + p] + 8, &a);
  if (steps < 0) { atomicOr(error, 1); return; }
  const long long twice = a.a00 < 0 ? -a.a00 : a.a00;
  if (twice < min_twice_area) return;
  const int slot = atomicAdd(rec_count + img, 1);
  if (slot >= work_cap) return;                                 // counted, not stored
  long long* r = recs + ((size_t)img * work_cap + slot) * FE_CONTOUR_RECORD;
  r[0] = p; r[1] = a.a00; r[2] = a.a10; r[3] = a.a01;
  r[4] = xmin[base + p]; r[5] = y0; r[6] = xmax[base + p]; r[7] = ymax[base + p];
}

// np.median of the uint8 image from its histogram, kept as twice the median (an even pixel count takes the mean of the two middle values),
// then lower = int(max(0, 0.5 median)) = m2 / 4 and upper = int(min(255, 1.5 median)) = min(255, 3 m2 / 4)
__global__ void median_thresholds_kernel(const double* __restrict__ stats, int n, long long npx, int* __restrict__ thr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* hist = stats + (size_t)i * FE_STATS_COUNT;
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
  thr[2 * i] = m2 / 4;
  thr[2 * i + 1] = min(255, 3 * m2 / 4);
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

// roots of 8-connected components are never neighbours of each other: at most one per 2x2 cell
int contour_work_cap(int h, int w) { return ((h + 1) / 2) * ((w + 1) / 2); }

size_t contour_scratch_bytes(int nb, int h, int w) {
  const size_t tot = (size_t)nb * h * w, cap = (size_t)nb * contour_work_cap(h, w);
  return 7 * up256(tot * sizeof(int)) + 2 * up256(tot) + up256(cap * sizeof(int)) + up256(cap * FE_CONTOUR_RECORD * sizeof(long long)) +
         2 * up256((size_t)nb * sizeof(int)) + up256(sizeof(int));
}

void contour_scratch_carve(ContourScratch& sc, void* base, int nb, int h, int w) {
  const size_t tot = (size_t)nb * h * w, cap = (size_t)nb * contour_work_cap(h, w);
  uint8_t* q = (uint8_t*)base;
  auto take = [&](size_t bytes) { void* r = q; q += up256(bytes); return r; };
  sc.lab_fg = (int*)take(tot * sizeof(int));
  sc.lab_bg = (int*)take(tot * sizeof(int));
  sc.cnt = (int*)take(tot * sizeof(int));
  sc.strong = (int*)take(tot * sizeof(int));
  sc.xmin = (int*)take(tot * sizeof(int));
  sc.xmax = (int*)take(tot * sizeof(int));
  sc.ymax = (int*)take(tot * sizeof(int));
  sc.outer = (uint8_t*)take(tot);
  sc.edge = (uint8_t*)take(tot);
  sc.work = (int*)take(cap * sizeof(int));
  sc.recs = (long long*)take(cap * FE_CONTOUR_RECORD * sizeof(long long));
  sc.work_count = (int*)take((size_t)nb * sizeof(int));
  sc.rec_count = (int*)take((size_t)nb * sizeof(int));
  sc.error = (int*)take(sizeof(int));
}

void launch_median_thresholds(const double* d_stats, int n, long long npx, int* d_thr, hipStream_t s) {
  hipLaunchKernelGGL(median_thresholds_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_stats, n, npx, d_thr);
  FE_HIP(hipGetLastError());
}

void launch_external_contours(const uint8_t* d_img, int nb, int h, int w, int candidates, long long min_twice_area, ContourScratch& sc,
                              hipStream_t s) {
  FE_CHECK(nb > 0 && nb <= 65535 && h > 0 && w > 0 && (size_t)h * w < (1ull << 31) && (h + CT - 1) / CT <= 65535, "contours: bad shape");
  const size_t npx = (size_t)h * w, tot = (size_t)nb * npx;
  FE_HIP(hipMemsetAsync(sc.cnt, 0, tot * sizeof(int), s));
  FE_HIP(hipMemsetAsync(sc.strong, 0, tot * sizeof(int), s));
  FE_HIP(hipMemsetAsync(sc.xmin, 0x7F, tot * sizeof(int), s));      // larger than any column
  FE_HIP(hipMemsetAsync(sc.xmax, 0xFF, tot * sizeof(int), s));      // -1
  FE_HIP(hipMemsetAsync(sc.ymax, 0xFF, tot * sizeof(int), s));
  FE_HIP(hipMemsetAsync(sc.outer, 0, tot, s));
  FE_HIP(hipMemsetAsync(sc.work_count, 0, (size_t)nb * sizeof(int), s));
  FE_HIP(hipMemsetAsync(sc.rec_count, 0, (size_t)nb * sizeof(int), s));
  FE_HIP(hipMemsetAsync(sc.error, 0, sizeof(int), s));
  const dim3 blk(CT, CT), grid((w + CT - 1) / CT, (h + CT - 1) / CT, nb);
  const int mode = candidates ? SET_CAND : SET_FG;
  hipLaunchKernelGGL(ccl_local_kernel, grid, blk, 0, s, d_img, h, w, mode, 1, sc.lab_fg);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_seam_kernel, grid, blk, 0, s, h, w, 1, sc.lab_fg);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_flatten_fg_kernel, grid, blk, 0, s, d_img, h, w, mode, sc.lab_fg, sc.cnt, sc.strong, sc.xmin, sc.xmax, sc.ymax);
  FE_HIP(hipGetLastError());
  const uint8_t* fgimg = d_img;
  if (candidates) {
    hipLaunchKernelGGL(contour_edge_kernel, dim3((unsigned)((npx + 255) / 256), nb), dim3(256), 0, s, sc.lab_fg, sc.strong, npx, sc.edge);
    FE_HIP(hipGetLastError());
    fgimg = sc.edge;
  }
  hipLaunchKernelGGL(ccl_local_kernel, grid, blk, 0, s, fgimg, h, w, (int)SET_BG, 0, sc.lab_bg);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_seam_kernel, grid, blk, 0, s, h, w, 0, sc.lab_bg);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_flatten_bg_kernel, grid, blk, 0, s, h, w, sc.lab_bg, sc.outer);
  FE_HIP(hipGetLastError());
  const int cap = contour_work_cap(h, w);
  hipLaunchKernelGGL(contour_candidates_kernel, grid, blk, 0, s, h, w, min_twice_area, sc.lab_fg, sc.lab_bg, sc.strong, sc.xmin, sc.xmax, sc.ymax,
                     sc.outer, sc.work, sc.work_count, cap, sc.error);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(contour_walk_kernel, dim3((cap + 63) / 64, nb), dim3(64), 0, s, fgimg, h, w, min_twice_area, sc.cnt, sc.xmin, sc.xmax, sc.ymax,
                     sc.work, sc.work_count, cap, sc.recs, sc.rec_count, sc.error);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
