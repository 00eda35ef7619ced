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
#include "composition_core.h"
#include "fe_common.h"

namespace fe {

namespace {

// the per-pixel and per-tile bodies are composition_core.h's, shared with the mixed-size kernels (kernels_composition_mixed.hip)
__global__ __launch_bounds__(CT * CT) void ccl_local_kernel(const uint8_t* __restrict__ img, int h, int w, int mode, int conn8,
                                                            int* __restrict__ labels) {
  __shared__ int L[CT * CT];
  const size_t base = (size_t)blockIdx.z * h * w;
  ccl_local_tile(img + base, h, w, mode, conn8, blockIdx.x, blockIdx.y, labels + base, L);
}

__global__ __launch_bounds__(CT * CT) void ccl_seam_kernel(int h, int w, int conn8, int* __restrict__ labels) {
  ccl_seam_px(h, w, conn8, blockIdx.x, blockIdx.y, labels + (size_t)blockIdx.z * h * w);
}

__global__ __launch_bounds__(CT * CT) void ccl_flatten_fg_kernel(const uint8_t* __restrict__ img, int h, int w, int mode, int* __restrict__ labels,
                                                                 int* __restrict__ cnt, int* __restrict__ strong, int* __restrict__ xmin,
                                                                 int* __restrict__ xmax, int* __restrict__ ymax) {
  const int x = blockIdx.x * CT + threadIdx.x, y = blockIdx.y * CT + threadIdx.y;
  const size_t base = (size_t)blockIdx.z * h * w;
  ccl_flatten_fg_px(img + base, h, w, mode, x, y, labels + base, cnt + base, strong + base, xmin + base, xmax + base, ymax + base);
}

__global__ __launch_bounds__(CT * CT) void ccl_flatten_bg_kernel(int h, int w, int* __restrict__ labels, uint8_t* __restrict__ outer) {
  const int x = blockIdx.x * CT + threadIdx.x, y = blockIdx.y * CT + threadIdx.y;
  const size_t base = (size_t)blockIdx.z * h * w;
  ccl_flatten_bg_px(h, w, x, y, labels + base, outer + base);
}

__global__ void contour_edge_kernel(const int* __restrict__ labels, const int* __restrict__ strong, size_t npx, uint8_t* __restrict__ edge) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npx) return;
  const size_t base = (size_t)blockIdx.y * npx;
  edge[base + p] = contour_edge_px(labels + base, strong + base, p);
}

__global__ __launch_bounds__(CT * CT) void contour_candidates_kernel(int h, int w, long long min_twice_area, const int* __restrict__ lab_fg,
                                                                     const int* __restrict__ lab_bg, const int* __restrict__ strong,
                                                                     const int* __restrict__ xmin, const int* __restrict__ xmax,
                                                                     const int* __restrict__ ymax, const uint8_t* __restrict__ outer,
                                                                     int* __restrict__ work, int* __restrict__ work_count, int work_cap,
                                                                     int* __restrict__ error) {
  const int x = blockIdx.x * CT + threadIdx.x, y = blockIdx.y * CT + threadIdx.y;
  const int img = blockIdx.z;
  const size_t base = (size_t)img * h * w;
  contour_candidate_px(h, w, x, y, min_twice_area, lab_fg + base, lab_bg + base, strong + base, xmin + base, xmax + base, ymax + base, outer + base,
                       work + (size_t)img * work_cap, work_count + img, work_cap, error);
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
  long long r[FE_CONTOUR_RECORD];
  if (!contour_walk_one(fgimg + base, h, w, work[(size_t)img * work_cap + j], min_twice_area, cnt + base, xmin + base, xmax + base, ymax + base,
                        error, r))
    return;
  const int slot = atomicAdd(rec_count + img, 1);
  if (slot >= work_cap) return;                                 // counted, not stored
  long long* o = recs + ((size_t)img * work_cap + slot) * FE_CONTOUR_RECORD;
  for (int k = 0; k < FE_CONTOUR_RECORD; ++k) o[k] = r[k];
}

__global__ void median_thresholds_kernel(const double* __restrict__ stats, int n, long long npx, int* __restrict__ thr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  median_thresholds_of(stats + (size_t)i * FE_STATS_COUNT, npx, thr + 2 * i, thr + 2 * i + 1);
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
