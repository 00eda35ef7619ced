// The face-path pixel kernels of kernels_face.hip and roi_laplacian_kernel (kernels_stats.hip) for a list of images that each have
// their own size and address: every kernel takes the per-image descriptors of face_mixed_plan.h instead of one (base, h, w) and an
// `rgb` flag that says which byte of a source pixel is blue (0: B,G,R as cv2 holds them; 1: R,G,B). The arithmetic is that of the
// per-shape kernels, expression for expression, so the same pixels give the same bits.
//   det_input_mixed     SCRFD.detect's cv2.resize into the corner of the zero canvas + blobFromImage in one launch: reads the source
//                       images, writes the detector's NHWC4 fp32 input. No uint8 canvas, no memset.
//   scrfd_decode_mixed  scrfd_decode_kernel with the det_scale of the candidate's image; one record block per image (count, then rows)
//   warp_affine_mixed   warp_affine_kernel with source, h, w of the crop's image; writes the uint8 crops or, fused with u8_blob, the
//                       normalised NHWC4 fp32 input of the landmark / recognition graph
//   roi_laplacian_mixed roi_laplacian_kernel with source, h, w of the ROI's image
#include "fe_common.h"
#include "face_mixed_plan.h"

namespace fe {

using face_plan::ImageDesc;

// ---- detector input -----------------------------------------------------------------------------------------------------------------
// grid (ceil(det_h * det_w / 256), nb): thread t of block b writes pixel b * 256 + t of image blockIdx.y, so the float4 stores of a wave
// are 1 KiB of consecutive addresses. The descriptor is uniform over a block. Reads stay inside the image: the column table holds
// offsets in [0, w - 1] and sx + 1 is used only below w; rows are clamped into [0, h - 1]; the box route reads rows 2 dy, 2 dy + 1 < h
// and columns 2 dx, 2 dx + 1 < w because h = 2 new_h and w = 2 new_w there.
__global__ __launch_bounds__(256) void det_input_mixed_kernel(const ImageDesc* __restrict__ descs, const int32_t* __restrict__ pool, int det_h, int det_w,
                                                              int rgb, float4* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= det_h * det_w) return;
  const ImageDesc d = descs[blockIdx.y];
  const int dy = i / det_w, dx = i - dy * det_w;
  int c[3] = {0, 0, 0};      // the canvas pixel in the source's byte order; the padding is zero
  if (dy < d.new_h && dx < d.new_w) {
    const uint8_t* s = d.src;
    const size_t row = (size_t)d.w * 3;
    if (d.mode == face_plan::kCopy) {
      const uint8_t* p = s + (size_t)dy * row + (size_t)dx * 3;
      c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
    } else if (d.mode == face_plan::kBox2) {      // scale exactly 2 in both directions: OpenCV switches INTER_LINEAR to the 2x2 box average
      const uint8_t* p = s + (size_t)(2 * dy) * row + (size_t)(2 * dx) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = (p[k] + p[3 + k] + p[row + k] + p[row + 3 + k] + 2) >> 2;
    } else {
      const int32_t* xt = pool + d.xtab;
      const int32_t* yt = pool + d.ytab;
      const int sx = xt[dx], sy = yt[dy];
      const int32_t wa = xt[d.new_w + dx], wb = yt[d.new_h + dy];
      const int a0 = (short)(wa & 0xffff), a1 = (short)(wa >> 16), b0 = (short)(wb & 0xffff), b1 = (short)(wb >> 16);
      const int sx1 = sx + 1 < d.w ? sx + 1 : sx;
      const int sy0 = sy < 0 ? 0 : (sy > d.h - 1 ? d.h - 1 : sy), sy1 = sy + 1 < 0 ? 0 : (sy + 1 > d.h - 1 ? d.h - 1 : sy + 1);
      const uint8_t* r0 = s + (size_t)sy0 * row;
      const uint8_t* r1 = s + (size_t)sy1 * row;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int S0 = r0[sx * 3 + k] * a0 + r0[sx1 * 3 + k] * a1;
        const int S1 = r1[sx * 3 + k] * a0 + r1[sx1 * 3 + k] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        c[k] = v < 0 ? 0 : (v > 255 ? 255 : v);
      }
    }
  }
  // blobFromImage(canvas, 1/128, mean 127.5, swapRB): the graph takes R,G,B
  const float r = (float)(rgb ? c[0] : c[2]), g = (float)c[1], b = (float)(rgb ? c[2] : c[0]);
  const float scale = 1.0f / 128.0f;
  dst[(size_t)blockIdx.y * det_h * det_w + i] = make_float4((r - 127.5f) * scale, (g - 127.5f) * scale, (b - 127.5f) * scale, 0.f);
}
void launch_det_input_mixed(const ImageDesc* descs, int nb, const int32_t* pool, int det_h, int det_w, int rgb, float* dst, hipStream_t s) {
  if (nb <= 0) return;
  FE_CHECK(nb <= 65535 && det_h > 0 && det_w > 0, "det_input_mixed: %d images of %d x %d", nb, det_h, det_w);
  hipLaunchKernelGGL(det_input_mixed_kernel, dim3((unsigned)((det_h * det_w + 255) / 256), (unsigned)nb), dim3(256), 0, s, descs, pool, det_h, det_w, rgb,
                     (float4*)dst);
  FE_HIP(hipGetLastError());
}

// ---- SCRFD decode with a det_scale per image ------------------------------------------------------------------------------------------
// recs: per image 16 floats of header (word 0: the int count, zeroed by the caller) and max_cand candidate rows of 16 floats.
__global__ void scrfd_decode_mixed_kernel(const float* __restrict__ scores, const float* __restrict__ bbox, const float* __restrict__ kps, int n, int fh, int fw,
                                          int A, int K, int stride, float thresh, const ImageDesc* __restrict__ descs, int level, float* __restrict__ recs,
                                          int max_cand) {
  const size_t per = (size_t)fh * fw * A;
  const size_t total = (size_t)n * per;
  const size_t rec_floats = (size_t)(max_cand + 1) * 16;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float sc = scores[i];
    if (!(sc >= thresh)) continue;
    const int img = (int)(i / per);
    const size_t r = i - (size_t)img * per;
    const size_t cell = r / A;
    const float px = (float)((int)(cell % fw) * stride), py = (float)((int)(cell / fw) * stride);
    float* rec = recs + (size_t)img * rec_floats;
    const int slot = atomicAdd(reinterpret_cast<int*>(rec), 1);
    if (slot >= max_cand) continue;
    const float det_scale = descs[img].det_scale;
    float* o = rec + (size_t)(slot + 1) * 16;
    const float* b = bbox + i * 4;
    o[0] = sc;
    const float fs = (float)stride;
    o[1] = (px - b[0] * fs) / det_scale;
    o[2] = (py - b[1] * fs) / det_scale;
    o[3] = (px + b[2] * fs) / det_scale;
    o[4] = (py + b[3] * fs) / det_scale;
    for (int k = 0; k < 5; ++k) {
      o[5 + 2 * k] = k < K ? (px + kps[i * 2 * K + 2 * k] * fs) / det_scale : 0.f;
      o[6 + 2 * k] = k < K ? (py + kps[i * 2 * K + 2 * k + 1] * fs) / det_scale : 0.f;
    }
    o[15] = (float)level;
  }
}
void launch_scrfd_decode_mixed(const float* scores, const float* bbox, const float* kps, int n, int fh, int fw, int A, int K, int stride, float thresh,
                               const ImageDesc* descs, int level, float* recs, int max_cand, hipStream_t s) {
  const size_t total = (size_t)n * fh * fw * A;
  if (!total) return;
  const size_t g = std::min<size_t>(4096, (total + 255) / 256);
  hipLaunchKernelGGL(scrfd_decode_mixed_kernel, dim3((unsigned)g), dim3(256), 0, s, scores, bbox, kps, n, fh, fw, A, K, stride, thresh, descs, level, recs,
                     max_cand);
  FE_HIP(hipGetLastError());
}

// ---- warpAffine over crops of images of different sizes -------------------------------------------------------------------------------
// F32 = false: dst uint8 [m][S][S][3] in the source's byte order. F32 = true: dst float4 [m][S][S], (pixel - mean) * scale with the byte
// `first` (0 or 2) of the source pixel in channel 0 - what launch_u8_blob makes of the uint8 crop. Taps outside the image are 0.
template <bool F32>
__global__ void warp_affine_mixed_kernel(const ImageDesc* __restrict__ descs, const int* __restrict__ img_of, const double* __restrict__ Minv, int m, int S,
                                         const short* __restrict__ wtab, void* __restrict__ dst, float mean, float scale, int first) {
  const size_t total = (size_t)m * S * S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % S);
    const int y = (int)((i / S) % S);
    const int f = (int)(i / ((size_t)S * S));
    const double* M = Minv + (size_t)f * 6;
    const int adelta = __double2int_rn(M[0] * x * 1024.0), bdelta = __double2int_rn(M[3] * x * 1024.0);
    const int X0 = __double2int_rn((M[1] * y + M[2]) * 1024.0) + 16, Y0 = __double2int_rn((M[4] * y + M[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    int sx = X >> 5, sy = Y >> 5;
    sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
    sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
    const short* wt = wtab + (size_t)((Y & 31) * 32 + (X & 31)) * 4;
    const ImageDesc d = descs[img_of[f]];
    const uint8_t* s = d.src;
    const int h = d.h, w = d.w;
    const bool x0ok = sx >= 0 && sx < w, x1ok = sx + 1 >= 0 && sx + 1 < w, y0ok = sy >= 0 && sy < h, y1ok = sy + 1 >= 0 && sy + 1 < h;
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int p00 = (x0ok && y0ok) ? s[((size_t)sy * w + sx) * 3 + k] : 0;
      const int p01 = (x1ok && y0ok) ? s[((size_t)sy * w + sx + 1) * 3 + k] : 0;
      const int p10 = (x0ok && y1ok) ? s[((size_t)(sy + 1) * w + sx) * 3 + k] : 0;
      const int p11 = (x1ok && y1ok) ? s[((size_t)(sy + 1) * w + sx + 1) * 3 + k] : 0;
      const int v = (p00 * wt[0] + p01 * wt[1] + p10 * wt[2] + p11 * wt[3] + (1 << 14)) >> 15;
      c[k] = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
    if (F32) {
      const float c0 = (float)(first ? c[2] : c[0]), c2 = (float)(first ? c[0] : c[2]);
      reinterpret_cast<float4*>(dst)[i] = make_float4((c0 - mean) * scale, ((float)c[1] - mean) * scale, (c2 - mean) * scale, 0.f);
    } else {
      uint8_t* o = reinterpret_cast<uint8_t*>(dst) + i * 3;
      o[0] = (uint8_t)c[0]; o[1] = (uint8_t)c[1]; o[2] = (uint8_t)c[2];
    }
  }
}
static inline unsigned warp_grid(size_t work) { return (unsigned)std::max<size_t>(1, std::min<size_t>(4096, (work + 255) / 256)); }
void launch_warp_affine_mixed(const ImageDesc* descs, const int* img_of, const double* Minv, int m, int S, const short* wtab, uint8_t* dst, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(warp_affine_mixed_kernel<false>, dim3(warp_grid((size_t)m * S * S)), dim3(256), 0, s, descs, img_of, Minv, m, S, wtab, (void*)dst, 0.f, 1.f, 0);
  FE_HIP(hipGetLastError());
}
void launch_warp_affine_blob_mixed(const ImageDesc* descs, const int* img_of, const double* Minv, int m, int S, const short* wtab, float* dst, float mean,
                                   float scale, int first, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(warp_affine_mixed_kernel<true>, dim3(warp_grid((size_t)m * S * S)), dim3(256), 0, s, descs, img_of, Minv, m, S, wtab, (void*)dst, mean,
                     scale, first);
  FE_HIP(hipGetLastError());
}

// ---- ROI Laplacian over images of different sizes ---------------------------------------------------------------------------------------
// cv2's 8-bit BGR2GRAY (kernels_stats.hip: gray_of)
__device__ __forceinline__ int gray_of_bgr(int b, int g, int r) { return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15; }

// One block per ROI, as roi_laplacian_kernel. rois [m][4] = x1,y1,x2,y2 inside the ROI's image (checked on the host).
__global__ __launch_bounds__(256) void roi_laplacian_mixed_kernel(const ImageDesc* __restrict__ descs, int rgb, const int* __restrict__ img_of,
                                                                  const int* __restrict__ rois, int m, double* __restrict__ out) {
  const int f = blockIdx.x;
  if (f >= m) return;
  const int x1 = rois[4 * f], y1 = rois[4 * f + 1], x2 = rois[4 * f + 2], y2 = rois[4 * f + 3];
  const int rw = x2 - x1, rh = y2 - y1;
  __shared__ long long red[3][4];
  long long lsum = 0, lsq = 0, gsum = 0;
  if (rw > 0 && rh > 0) {
    const ImageDesc d = descs[img_of[f]];
    const uint8_t* src = d.src;
    const int w = d.w;
    auto G = [&](int yy, int xx) {
      const uint8_t* p = src + ((size_t)(y1 + yy) * w + (x1 + xx)) * 3;
      return rgb ? gray_of_bgr(p[2], p[1], p[0]) : gray_of_bgr(p[0], p[1], p[2]);
    };
    const int total = rw * rh;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int y = i / rw, x = i - y * rw;
      const int ym = rh > 1 ? (y - 1 < 0 ? 1 : y - 1) : 0, yp = rh > 1 ? (y + 1 >= rh ? rh - 2 : y + 1) : 0;
      const int xm = rw > 1 ? (x - 1 < 0 ? 1 : x - 1) : 0, xp = rw > 1 ? (x + 1 >= rw ? rw - 2 : x + 1) : 0;
      const int c = G(y, x);
      const int lap = G(ym, x) + G(yp, x) + G(y, xm) + G(y, xp) - 4 * c;
      lsum += lap; lsq += lap * lap; gsum += c;
    }
  }
  for (int o = 32; o > 0; o >>= 1) { lsum += __shfl_xor(lsum, o); lsq += __shfl_xor(lsq, o); gsum += __shfl_xor(gsum, o); }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wv] = lsum; red[1][wv] = lsq; red[2][wv] = gsum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = out + (size_t)f * 4;
    o[0] = (double)(red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    o[1] = (double)(red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    o[2] = (double)(red[2][0] + red[2][1] + red[2][2] + red[2][3]);
    o[3] = (rw > 0 && rh > 0) ? (double)rw * rh : 0.0;
  }
}
void launch_roi_laplacian_mixed(const ImageDesc* descs, int rgb, const int* img_of, const int* rois, int m, double* out, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(roi_laplacian_mixed_kernel, dim3(m), dim3(256), 0, s, descs, rgb, img_of, rois, m, out);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
