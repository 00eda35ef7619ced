// fe_leading_lines_mixed and fe_subject_region_mixed: the GPU stages of kernels_lines.hip and kernels_contours.hip for a list of images
// of any sizes, one launch per stage per chunk of the plan (composition_mixed_plan.h). The arithmetic is the per-shape kernels' own -
// both call the bodies of composition_core.h, which work on one image's planes - so every byte and record equals what the per-shape
// call gives for that image alone. What differs is how a workgroup finds its image: grids are 1-D over the tiles of all images, and
// the flat block index is bisected in the tiling's cumulative tile counts (n + 1 entries; block-uniform, so the loads are scalar).
// Labels stay pixel indices inside the image and every neighbour test uses the image's own h and w, so no seam, border rule or walk
// reaches the next image's planes.
//   lines     blur from R,G,B or B,G,R in place -> Sobel -> suppression with one pair of thresholds
//   subject   gray + 256-bin histogram (LDS counts, merged with atomics) -> median thresholds per image -> Sobel -> suppression with
//             per-image thresholds -> labelling, RETR_EXTERNAL test, border walks. The walks append to ONE record list per chunk, each
//             record tagged with its image in the upper half of field 0, so the records go down in one copy.
#include "composition_core.h"
#include "fe_common.h"

namespace fe {

namespace {

namespace cp = comp_plan;
static_assert(cp::kTileW[cp::kBlur] == LB_W && cp::kTileH[cp::kBlur] == LB_H, "composition_mixed_plan.h counts the blur's tiles");
static_assert(cp::kTileW[cp::kSobel] == LS_W && cp::kTileH[cp::kSobel] == LS_H, "composition_mixed_plan.h counts Sobel's tiles");
static_assert(cp::kTileW[cp::kCcl] == CT && cp::kTileH[cp::kCcl] == CT, "composition_mixed_plan.h counts the labelling's tiles");
static_assert(sizeof(cp::ImageDesc) == 32, "the descriptor blob is laid out by composition_mixed_plan.h");

// the image block `b` of a 1-D grid works on: prefix [n + 1] ascending from 0, prefix[k] <= b < prefix[k + 1]; *tile: b's place in it
__device__ __forceinline__ int image_of_block(const int32_t* __restrict__ prefix, int n, int b, int* tile) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b) lo = mid; else hi = mid;
  }
  *tile = b - prefix[lo];
  return lo;
}
// the same, and the tile's column and row in an image cut into tiles tw wide
__device__ __forceinline__ cp::ImageDesc image_tile(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix, int n, int tw, int* k,
                                                    int* bx, int* by) {
  int tile;
  *k = image_of_block(prefix, n, (int)blockIdx.x, &tile);
  const cp::ImageDesc im = descs[*k];
  const int across = (im.w + tw - 1) / tw;
  *by = tile / across;
  *bx = tile - *by * across;
  return im;
}

template <bool kRgb>
__global__ __launch_bounds__(LB_W * LB_H) void blur_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix, int n,
                                                                 uint8_t* __restrict__ blur) {
  __shared__ int g[LB_H + 4][LB_W + 4];
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, LB_W, &k, &bx, &by);
  lines_blur_tile<kRgb>(im.src, im.h, im.w, bx, by, blur + im.px, g);
}

__global__ __launch_bounds__(LS_W * LS_H) void sobel_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix, int n,
                                                                  const uint8_t* __restrict__ src, short2* __restrict__ grad,
                                                                  unsigned short* __restrict__ mag) {
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, LS_W, &k, &bx, &by);
  const int x = bx * LS_W + threadIdx.x, y = by * LS_H + threadIdx.y;
  if (x >= im.w || y >= im.h) return;
  lines_sobel_px(src + im.px, im.h, im.w, x, y, grad + im.px, mag + im.px);
}

// PER_IMAGE: the two thresholds of image k are thr[2 k], thr[2 k + 1] instead of low / high
template <bool PER_IMAGE>
__global__ __launch_bounds__(LS_W * LS_H) void nms_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix, int n,
                                                                const short2* __restrict__ grad, const unsigned short* __restrict__ mag, int low,
                                                                int high, const int* __restrict__ thr, uint8_t* __restrict__ map) {
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, LS_W, &k, &bx, &by);
  const int x = bx * LS_W + threadIdx.x, y = by * LS_H + threadIdx.y;
  if (x >= im.w || y >= im.h) return;
  if (PER_IMAGE) { low = thr[2 * k]; high = thr[2 * k + 1]; }
  map[im.px + (size_t)y * im.w + x] = lines_nms_px(grad + im.px, mag + im.px, im.h, im.w, x, y, low, high);
}

// One workgroup per run of kGrayRun pixels of one image: the gray plane and the image's 256 gray counts, which are all the subject call
// reads of the statistics pass the per-shape call runs (the same gray value per pixel, and a count does not depend on who counted).
template <bool kRgb>
__global__ __launch_bounds__(256) void gray_hist_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix, int n,
                                                              uint8_t* __restrict__ gray, unsigned int* __restrict__ hist) {
  __shared__ unsigned int gh[256];
  int run;
  const int k = image_of_block(prefix, n, (int)blockIdx.x, &run);
  const cp::ImageDesc im = descs[k];
  gh[threadIdx.x] = 0;
  __syncthreads();
  const size_t npx = (size_t)im.h * im.w, p0 = (size_t)run * cp::kGrayRun, p1 = min(npx, p0 + cp::kGrayRun);
  uint8_t* out = gray + im.px;
  for (size_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const uint8_t* s = im.src + p * 3;
    const int y = kRgb ? lines_gray(s[2], s[1], s[0]) : lines_gray(s[0], s[1], s[2]);
    out[p] = (uint8_t)y;
    atomicAdd(&gh[y], 1u);
  }
  __syncthreads();
  const unsigned int c = gh[threadIdx.x];
  if (c) atomicAdd(&hist[(size_t)k * 256 + threadIdx.x], c);
}

__global__ void thresholds_mixed_kernel(const cp::ImageDesc* __restrict__ descs, int n, const unsigned int* __restrict__ hist, int* __restrict__ thr) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  median_thresholds_of(hist + (size_t)k * 256, (long long)descs[k].h * descs[k].w, thr + 2 * k, thr + 2 * k + 1);
}

// xmin [P] <- larger than any column, xmax [P] and ymax [P] <- -1: the three planes lie back to back
__global__ void fill_bounds_kernel(int* __restrict__ planes, size_t P) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 * P) planes[i] = i < P ? 0x7F7F7F7F : -1;
}

__global__ __launch_bounds__(CT * CT) void ccl_local_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix, int n,
                                                                  const uint8_t* __restrict__ img, int mode, int conn8, int* __restrict__ labels) {
  __shared__ int L[CT * CT];
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, CT, &k, &bx, &by);
  ccl_local_tile(img + im.px, im.h, im.w, mode, conn8, bx, by, labels + im.px, L);
}

__global__ __launch_bounds__(CT * CT) void ccl_seam_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix, int n,
                                                                 int conn8, int* __restrict__ labels) {
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, CT, &k, &bx, &by);
  ccl_seam_px(im.h, im.w, conn8, bx, by, labels + im.px);
}

__global__ __launch_bounds__(CT * CT) void ccl_flatten_fg_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix,
                                                                       int n, const uint8_t* __restrict__ img, int mode, int* __restrict__ labels,
                                                                       int* __restrict__ cnt, int* __restrict__ strong, int* __restrict__ xmin,
                                                                       int* __restrict__ xmax, int* __restrict__ ymax) {
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, CT, &k, &bx, &by);
  ccl_flatten_fg_px(img + im.px, im.h, im.w, mode, bx * CT + threadIdx.x, by * CT + threadIdx.y, labels + im.px, cnt + im.px, strong + im.px,
                    xmin + im.px, xmax + im.px, ymax + im.px);
}

__global__ __launch_bounds__(CT * CT) void contour_edge_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix, int n,
                                                                     const int* __restrict__ labels, const int* __restrict__ strong,
                                                                     uint8_t* __restrict__ edge) {
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, CT, &k, &bx, &by);
  const int x = bx * CT + threadIdx.x, y = by * CT + threadIdx.y;
  if (x >= im.w || y >= im.h) return;
  const size_t p = (size_t)y * im.w + x;
  edge[im.px + p] = contour_edge_px(labels + im.px, strong + im.px, p);
}

__global__ __launch_bounds__(CT * CT) void ccl_flatten_bg_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix,
                                                                       int n, int* __restrict__ labels, uint8_t* __restrict__ outer) {
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, CT, &k, &bx, &by);
  ccl_flatten_bg_px(im.h, im.w, bx * CT + threadIdx.x, by * CT + threadIdx.y, labels + im.px, outer + im.px);
}

__global__ __launch_bounds__(CT * CT) void contour_candidates_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix,
                                                                           int n, const int* __restrict__ lab_fg, const int* __restrict__ lab_bg,
                                                                           const int* __restrict__ strong, const int* __restrict__ xmin,
                                                                           const int* __restrict__ xmax, const int* __restrict__ ymax,
                                                                           const uint8_t* __restrict__ outer, int* __restrict__ work,
                                                                           int* __restrict__ work_count, int* __restrict__ error) {
  int k, bx, by;
  const cp::ImageDesc im = image_tile(descs, prefix, n, CT, &k, &bx, &by);
  contour_candidate_px(im.h, im.w, bx * CT + threadIdx.x, by * CT + threadIdx.y, subject_min_twice_area((long long)im.h * im.w), lab_fg + im.px,
                       lab_bg + im.px, strong + im.px, xmin + im.px, xmax + im.px, ymax + im.px, outer + im.px, work + im.work, work_count + k, im.cap,
                       error);
}

// One lane per work-list entry. rec_count [n] counts every qualifying contour of its image; the record goes to the next free place of
// the chunk's list (room for `total_cap` = every image's work_cap, which no chunk can exceed), field 0 = image << 32 | start index.
__global__ __launch_bounds__(cp::kWalkLanes) void contour_walk_mixed_kernel(const cp::ImageDesc* __restrict__ descs, const int32_t* __restrict__ prefix,
                                                                            int n, const uint8_t* __restrict__ fgimg, const int* __restrict__ cnt,
                                                                            const int* __restrict__ xmin, const int* __restrict__ xmax,
                                                                            const int* __restrict__ ymax, const int* __restrict__ work,
                                                                            const int* __restrict__ work_count, long long* __restrict__ recs,
                                                                            int* __restrict__ rec_count, int* __restrict__ stored, unsigned total_cap,
                                                                            int* __restrict__ error) {
  int group;
  const int k = image_of_block(prefix, n, (int)blockIdx.x, &group);
  const cp::ImageDesc im = descs[k];
  const int j = group * cp::kWalkLanes + threadIdx.x;
  if (j >= min(work_count[k], im.cap)) return;
  long long r[FE_CONTOUR_RECORD];
  if (!contour_walk_one(fgimg + im.px, im.h, im.w, work[im.work + j], subject_min_twice_area((long long)im.h * im.w), cnt + im.px, xmin + im.px,
                        xmax + im.px, ymax + im.px, error, r))
    return;
  atomicAdd(rec_count + k, 1);
  const unsigned slot = (unsigned)atomicAdd(stored, 1);
  if (slot >= total_cap) { atomicOr(error, 2); return; }
  long long* o = recs + (size_t)slot * FE_CONTOUR_RECORD;
  o[0] = ((long long)k << 32) | r[0];
  for (int f = 1; f < FE_CONTOUR_RECORD; ++f) o[f] = r[f];
}

}  // namespace

// One chunk of fe_leading_lines_mixed. base: the chunk's allocation with the blob (descriptors with their pointers, prefix tables) in
// place; the map is left at base + lay.map, image k at its px.
void launch_canny_map_mixed(uint8_t* base, const comp_plan::Chunk& ck, int rgb, int low, int high, hipStream_t s) {
  const cp::Layout& L = ck.lay;
  const int n = ck.count;
  FE_CHECK(n > 0 && ck.pixels > 0 && ck.pixels <= cp::kMaxChunkPixels, "canny_mixed: bad plan");
  const cp::ImageDesc* descs = (const cp::ImageDesc*)(base + L.blob);
  auto prefix = [&](int t) { return (const int32_t*)(base + L.blob + L.blob_prefix) + (size_t)t * (n + 1); };
  uint8_t* blur = base + L.gray;
  short2* grad = (short2*)(base + L.grad);
  unsigned short* mag = (unsigned short*)(base + L.mag);
  const unsigned nb = (unsigned)ck.prefix[cp::kBlur].back(), ns = (unsigned)ck.prefix[cp::kSobel].back();
  if (rgb) hipLaunchKernelGGL(blur_mixed_kernel<true>, dim3(nb), dim3(LB_W, LB_H), 0, s, descs, prefix(cp::kBlur), n, blur);
  else hipLaunchKernelGGL(blur_mixed_kernel<false>, dim3(nb), dim3(LB_W, LB_H), 0, s, descs, prefix(cp::kBlur), n, blur);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(sobel_mixed_kernel, dim3(ns), dim3(LS_W, LS_H), 0, s, descs, prefix(cp::kSobel), n, (const uint8_t*)blur, grad, mag);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(nms_mixed_kernel<false>, dim3(ns), dim3(LS_W, LS_H), 0, s, descs, prefix(cp::kSobel), n, (const short2*)grad,
                     (const unsigned short*)mag, low, high, (const int*)nullptr, base + L.map);
  FE_HIP(hipGetLastError());
}

// One chunk of fe_subject_region_mixed, blob in place as above. Leaves the thresholds at lay.thr, the edge images at lay.edge, the
// counters (work_count [n], rec_count [n], error, records stored) at lay.counters and the tagged records at lay.recs.
void launch_subject_mixed(uint8_t* base, const comp_plan::Chunk& ck, int rgb, hipStream_t s) {
  const cp::Layout& L = ck.lay;
  const int n = ck.count;
  const size_t P = ck.pixels;
  FE_CHECK(n > 0 && P > 0 && P <= cp::kMaxChunkPixels && ck.work > 0 && ck.work < (1ull << 31), "subject_mixed: bad plan");
  const cp::ImageDesc* descs = (const cp::ImageDesc*)(base + L.blob);
  auto prefix = [&](int t) { return (const int32_t*)(base + L.blob + L.blob_prefix) + (size_t)t * (n + 1); };
  auto blocks = [&](int t) { return dim3((unsigned)ck.prefix[t].back()); };
  uint8_t* gray = base + L.gray;
  short2* grad = (short2*)(base + L.grad);
  unsigned short* mag = (unsigned short*)(base + L.mag);
  uint8_t* map = base + L.map;
  int *cnt = (int*)(base + L.cnt), *strong = (int*)(base + L.strong), *xmin = (int*)(base + L.fill), *xmax = xmin + P, *ymax = xmax + P;
  uint8_t *outer = base + L.outer, *edge = base + L.edge;
  unsigned int* hist = (unsigned int*)(base + L.hist);
  int *work_count = (int*)(base + L.counters), *rec_count = work_count + n, *error = rec_count + n, *stored = error + 1;
  int *thr = (int*)(base + L.thr), *lab_fg = (int*)(base + L.lab_fg), *lab_bg = (int*)(base + L.lab_bg), *work = (int*)(base + L.work);
  long long* recs = (long long*)(base + L.recs);

  FE_HIP(hipMemsetAsync(base + L.zero, 0, L.zero_bytes, s));
  hipLaunchKernelGGL(fill_bounds_kernel, dim3((unsigned)((3 * P + 255) / 256)), dim3(256), 0, s, xmin, P);
  FE_HIP(hipGetLastError());
  if (rgb) hipLaunchKernelGGL(gray_hist_mixed_kernel<true>, blocks(cp::kGray), dim3(256), 0, s, descs, prefix(cp::kGray), n, gray, hist);
  else hipLaunchKernelGGL(gray_hist_mixed_kernel<false>, blocks(cp::kGray), dim3(256), 0, s, descs, prefix(cp::kGray), n, gray, hist);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(thresholds_mixed_kernel, dim3((n + 63) / 64), dim3(64), 0, s, descs, n, (const unsigned int*)hist, thr);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(sobel_mixed_kernel, blocks(cp::kSobel), dim3(LS_W, LS_H), 0, s, descs, prefix(cp::kSobel), n, (const uint8_t*)gray, grad, mag);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(nms_mixed_kernel<true>, blocks(cp::kSobel), dim3(LS_W, LS_H), 0, s, descs, prefix(cp::kSobel), n, (const short2*)grad,
                     (const unsigned short*)mag, 0, 0, (const int*)thr, map);
  FE_HIP(hipGetLastError());
  const dim3 blk(CT, CT), grid = blocks(cp::kCcl);
  const int32_t* pc = prefix(cp::kCcl);
  hipLaunchKernelGGL(ccl_local_mixed_kernel, grid, blk, 0, s, descs, pc, n, (const uint8_t*)map, (int)SET_CAND, 1, lab_fg);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_seam_mixed_kernel, grid, blk, 0, s, descs, pc, n, 1, lab_fg);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_flatten_fg_mixed_kernel, grid, blk, 0, s, descs, pc, n, (const uint8_t*)map, (int)SET_CAND, lab_fg, cnt, strong, xmin, xmax, ymax);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(contour_edge_mixed_kernel, grid, blk, 0, s, descs, pc, n, (const int*)lab_fg, (const int*)strong, edge);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_local_mixed_kernel, grid, blk, 0, s, descs, pc, n, (const uint8_t*)edge, (int)SET_BG, 0, lab_bg);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_seam_mixed_kernel, grid, blk, 0, s, descs, pc, n, 0, lab_bg);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(ccl_flatten_bg_mixed_kernel, grid, blk, 0, s, descs, pc, n, lab_bg, outer);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(contour_candidates_mixed_kernel, grid, blk, 0, s, descs, pc, n, (const int*)lab_fg, (const int*)lab_bg, (const int*)strong,
                     (const int*)xmin, (const int*)xmax, (const int*)ymax, (const uint8_t*)outer, work, work_count, error);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(contour_walk_mixed_kernel, blocks(cp::kWalk), dim3(cp::kWalkLanes), 0, s, descs, prefix(cp::kWalk), n, (const uint8_t*)edge,
                     (const int*)cnt, (const int*)xmin, (const int*)xmax, (const int*)ymax, (const int*)work, (const int*)work_count, recs, rec_count,
                     stored, (unsigned)ck.work, error);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
