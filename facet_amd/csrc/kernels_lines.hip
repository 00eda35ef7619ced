// Leading-line detection (reference analyzers/composition.py:191-261: cv2.GaussianBlur(gray, (5,5), 0) ->
// cv2.Canny(50, 150) -> cv2.HoughLinesP(1, pi/180, 80, minLineLength, maxLineGap=20)).
//
// The pixel scans run on the GPU over the resident BGR batch (three small HBM-bound kernels, ~10 bytes of traffic per pixel):
//   lines_blur_kernel    BGR -> gray (OpenCV's 15-bit weights) -> 5x5 binomial blur, the fixed-point path OpenCV takes for
//                        8-bit images: kernel [1 4 6 4 1]/16 per axis, (sum + 128) >> 8, BORDER_REFLECT_101
//   lines_sobel_kernel   3x3 Sobel dx, dy (BORDER_REPLICATE, as cv::Canny asks for) and the L1 magnitude |dx| + |dy|
//   lines_nms_kernel     non-maximum suppression along the quantised gradient direction (tan 22.5 in 15-bit fixed point) and
//                        the two thresholds -> map: 2 = edge for sure, 0 = edge if connected to a 2, 1 = not an edge
// The rest (lines_host.cpp) is inherently sequential and runs on the host, one image per thread: hysteresis (flood fill from the 2s) and the
// progressive probabilistic Hough transform, whose result depends on the order a fixed pseudo-random generator visits the
// edge points in (vote, extract a segment as soon as a bin reaches the threshold, erase its points and un-vote them).
// [DEP-KNOWLEDGE] OpenCV is not available offline: these restate its documented algorithms; parity with cv2 is unpinned.
#include "composition_core.h"
#include "fe_common.h"

namespace fe {

// the per-pixel and per-tile bodies are composition_core.h's, shared with the mixed-size kernels (kernels_composition_mixed.hip)
__global__ __launch_bounds__(LB_W * LB_H) void lines_blur_kernel(const uint8_t* __restrict__ bgr, int h, int w, uint8_t* __restrict__ blur) {
  __shared__ int g[LB_H + 4][LB_W + 4];
  const size_t img = blockIdx.z;
  lines_blur_tile<false>(bgr + img * (size_t)h * w * 3, h, w, blockIdx.x, blockIdx.y, blur + img * (size_t)h * w, g);
}

__global__ void lines_sobel_kernel(const uint8_t* __restrict__ blur, int h, int w, short2* __restrict__ grad, unsigned short* __restrict__ mag) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const size_t base = (size_t)blockIdx.z * h * w;
  lines_sobel_px(blur + base, h, w, x, y, grad + base, mag + base);
}

// PER_IMAGE: the two thresholds of image blockIdx.z are read from thr[2 * blockIdx.z] (lower, upper) instead of low / high
template <bool PER_IMAGE>
__global__ void lines_nms_kernel(const short2* __restrict__ grad, const unsigned short* __restrict__ mag, int h, int w, int low, int high,
                                 const int* __restrict__ thr, uint8_t* __restrict__ map) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  if (PER_IMAGE) { low = thr[2 * blockIdx.z]; high = thr[2 * blockIdx.z + 1]; }
  const size_t base = (size_t)blockIdx.z * h * w;
  map[base + (size_t)y * w + x] = lines_nms_px(grad + base, mag + base, h, w, x, y, low, high);
}

// d_bgr [n][h][w][3] -> d_map [n][h][w]; d_blur / d_grad / d_mag: scratch of n*h*w elements each.
void launch_canny_map(const uint8_t* d_bgr, int n, int h, int w, int low, int high, uint8_t* d_blur, void* d_grad, void* d_mag, uint8_t* d_map,
                      hipStream_t s) {
  FE_CHECK(n > 0 && h > 0 && w > 0 && (size_t)h * w < (1ull << 31) && n <= 65535, "canny: bad shape");
  hipLaunchKernelGGL(lines_blur_kernel, dim3((w + LB_W - 1) / LB_W, (h + LB_H - 1) / LB_H, n), dim3(LB_W, LB_H), 0, s, d_bgr, h, w, d_blur);
  FE_HIP(hipGetLastError());
  const dim3 blk(LS_W, LS_H), grid((w + LS_W - 1) / LS_W, (h + LS_H - 1) / LS_H, n);
  hipLaunchKernelGGL(lines_sobel_kernel, grid, blk, 0, s, d_blur, h, w, (short2*)d_grad, (unsigned short*)d_mag);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(lines_nms_kernel<false>, grid, blk, 0, s, (const short2*)d_grad, (const unsigned short*)d_mag, h, w, low, high, (const int*)nullptr,
                     d_map);
  FE_HIP(hipGetLastError());
}

// Canny map of an image that is gray already and is NOT blurred (cv2.Canny(gray, lower, upper)), with one pair of thresholds per image in
// device memory: d_thr [n][2] = lower, upper. Same Sobel, same suppression as above.
void launch_canny_map_gray(const uint8_t* d_gray, int n, int h, int w, const int* d_thr, void* d_grad, void* d_mag, uint8_t* d_map, hipStream_t s) {
  FE_CHECK(n > 0 && h > 0 && w > 0 && (size_t)h * w < (1ull << 31) && n <= 65535, "canny: bad shape");
  const dim3 blk(LS_W, LS_H), grid((w + LS_W - 1) / LS_W, (h + LS_H - 1) / LS_H, n);
  hipLaunchKernelGGL(lines_sobel_kernel, grid, blk, 0, s, d_gray, h, w, (short2*)d_grad, (unsigned short*)d_mag);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(lines_nms_kernel<true>, grid, blk, 0, s, (const short2*)d_grad, (const unsigned short*)d_mag, h, w, 0, 0, d_thr, d_map);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
