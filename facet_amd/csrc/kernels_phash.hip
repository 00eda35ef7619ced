// Perceptual hash (imagehash.phash, hash_size 8, highfreq_factor 4) of a resident uint8 batch, and the all-pairs Hamming search
// that duplicate detection runs over the stored hashes.
//
// The reference computes `str(imagehash.phash(pil_img))` per image on the CPU (processing/batch_processor.py:216,
// multi_pass.py:449, scorer.py:972): image.convert('L'), .resize((32, 32), LANCZOS), scipy.fftpack.dct over both axes, the
// 8x8 low-frequency block against its median. [DEP-KNOWLEDGE: imagehash is not importable offline -> parity with the package
// itself is unpinned; every stage is pinned against PIL + scipy, tests/golden/make_phash_golden.py.]
//   stage 1 (phash_rows_kernel, the whole cost: 3 B/pixel read once): a wave per image row. The row is fetched with aligned
//           dword loads - rows are 3*w bytes, so a row starts at any byte offset: the dwords are re-aligned in registers with
//           v_alignbyte - turned into PIL's 'L' gray in registers, and only the gray bytes (w per row) are parked in LDS. The
//           horizontal Lanczos pass (PIL's int32 fixed point, kernels_resize.hip's coefficient tables) then runs out of LDS:
//           16 lanes share one output sample and split its taps, four output samples per step, a 4-step butterfly ends each.
//           h rows of w pixels leave as h x 32 bytes.
//   stage 2 (phash_finish_kernel, one block per image): vertical pass -> 32x32, DCT-II over both axes in fp64 by direct
//           summation from a host-made cosine table (rows k < 8 only), median of the 64 values, bits packed first-bit-highest.
// fe_phash_mixed runs both stages from per-image descriptors (phash_mixed_plan.h) over a list of images of any sizes: the row and finish
// kernels below come in a uniform and a descriptor-driven form around the same device functions.
// fe_hamming_pairs: tiled upper triangle, i-tile in registers, j-tile in LDS (every lane reads the same word: a broadcast),
// hits appended with one atomic per wave, every store checked against the capacity.
#include "engine.h"
#include "phash_mixed_plan.h"
#include <cmath>

namespace fe {

constexpr int PH_BITS = 32 - 8 - 2;      // PIL's PRECISION_BITS
constexpr int PH_SIDE = 32;              // hash_size * highfreq_factor
constexpr int PH_WAVES = 4;              // rows in flight per block of stage 1

__device__ __forceinline__ int ph_clip8(int v) {
  v >>= PH_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One aligned dword of the batch; a dword that sticks out of [lo, hi) (only the first / last of an allocation can) is put
// together from the bytes that are inside.
__device__ __forceinline__ uint32_t ph_load_dword(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (p + b >= lo && p + b < hi) v |= (uint32_t)p[b] << (8 * b);
  return v;
}

// One image row by one wave, first half: the row's pixels as PIL's 'L' gray bytes in the wave's LDS strip `gray`. src: the row's first
// byte, [lo, hi): the bytes of the allocation (or of the image) the row lies in - no dword outside it is loaded whole.
__device__ __forceinline__ void ph_row_gray(const uint8_t* src, const uint8_t* lo, const uint8_t* hi, int w, int c0, int c2, int lane, uint8_t* gray) {
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
  const uint8_t* base = src - mis;                      // 4-byte aligned
  for (int px = lane * 4; px < w; px += 256) {          // 4 pixels = 12 bytes = 3 dwords per lane (+1 when the row is off-grid)
    const uint8_t* p = base + (size_t)px * 3;
    uint32_t d0 = ph_load_dword(p, lo, hi), d1 = ph_load_dword(p + 4, lo, hi), d2 = ph_load_dword(p + 8, lo, hi);
    if (mis) {                                          // wave-uniform
      const uint32_t d3 = ph_load_dword(p + 12, lo, hi);
      d0 = __builtin_amdgcn_alignbyte(d1, d0, mis);
      d1 = __builtin_amdgcn_alignbyte(d2, d1, mis);
      d2 = __builtin_amdgcn_alignbyte(d3, d2, mis);
    }
    const int b[12] = {(int)(d0 & 255), (int)((d0 >> 8) & 255), (int)((d0 >> 16) & 255), (int)(d0 >> 24),
                       (int)(d1 & 255), (int)((d1 >> 8) & 255), (int)((d1 >> 16) & 255), (int)(d1 >> 24),
                       (int)(d2 & 255), (int)((d2 >> 8) & 255), (int)((d2 >> 16) & 255), (int)(d2 >> 24)};
    uint32_t g = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)                         // pixels past w give bytes no tap reads (px + 3 < wpad: inside the wave's strip)
      g |= (uint32_t)((b[3 * k] * c0 + b[3 * k + 1] * 38470 + b[3 * k + 2] * c2 + 0x8000) >> 16) << (8 * k);
    *reinterpret_cast<uint32_t*>(gray + px) = g;
  }
}

// Second half: the horizontal Lanczos pass over the gray strip -> the 32 bytes of `outrow` (LDS)
__device__ __forceinline__ void ph_row_hpass(const uint8_t* gray, const int* __restrict__ kk, const int* __restrict__ bounds, int ksize, int lane,
                                             uint8_t* outrow) {
  const int osub = lane >> 4, tsub = lane & 15;
  for (int o = osub; o < PH_SIDE; o += 4) {
    const int xmin = bounds[2 * o], xn = bounds[2 * o + 1];   // xmin + xn <= w by construction of the table
    const int* k = kk + (size_t)o * ksize;
    const uint8_t* g = gray + xmin;
    int s = 0;
    for (int t = tsub; t < xn; t += 16) s += (int)g[t] * k[t];
    s += __shfl_xor(s, 8); s += __shfl_xor(s, 4); s += __shfl_xor(s, 2); s += __shfl_xor(s, 1);
    if (tsub == 0) outrow[o] = (uint8_t)ph_clip8(s + (1 << (PH_BITS - 1)));
  }
}

// img [rows][w][3] u8 -> tmp [rows][32] u8. kk [32][ksize] / bounds [32][2]: the horizontal coefficient table.
// c0 / c2: PIL's 'L' weights of the first and third byte of a pixel (R,B or B,R). LDS: PH_WAVES x (wpad gray bytes) + PH_WAVES x 32.
__global__ __launch_bounds__(PH_WAVES * 64) void phash_rows_kernel(const uint8_t* __restrict__ img, size_t rows, int w, int wpad, int c0, int c2,
                                                                   const int* __restrict__ kk, const int* __restrict__ bounds, int ksize,
                                                                   uint8_t* __restrict__ tmp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ph_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t* gray = ph_lds + (size_t)wave * wpad;
  uint8_t* outrow = ph_lds + (size_t)PH_WAVES * wpad + wave * PH_SIDE;
  const uint8_t* lo = img;
  const uint8_t* hi = img + rows * (size_t)w * 3;
  const size_t step = (size_t)gridDim.x * PH_WAVES;
  // every wave of a block makes the same number of trips (the barriers below); a wave without a row idles through them
  for (size_t row0 = (size_t)blockIdx.x * PH_WAVES; row0 < rows; row0 += step) {
    const size_t row = row0 + wave;
    const bool live = row < rows;
    if (live) ph_row_gray(img + row * (size_t)w * 3, lo, hi, w, c0, c2, lane, gray);
    __syncthreads();
    if (live) ph_row_hpass(gray, kk, bounds, ksize, lane, outrow);
    __syncthreads();
    if (live && lane < PH_SIDE / 4)
      reinterpret_cast<uint32_t*>(tmp + row * PH_SIDE)[lane] = reinterpret_cast<const uint32_t*>(outrow)[lane];
  }
}

// fe_phash_mixed's stage 1: the same wave per row, over the rows of all images of a chunk. A wave finds its image by bisection of the
// descriptors' first_row (rows: the chunk's total), takes the width, the table and the [lo, hi) guard from that image's descriptor -
// images lie at any byte offset, a dword that two of them share is put together from the bytes of the one being read - and the LDS
// strips are as wide as the widest image of the chunk (wpad).
__global__ __launch_bounds__(PH_WAVES * 64) void phash_rows_mixed_kernel(const PhashDesc* __restrict__ descs, int n, uint32_t rows, int wpad, int c0, int c2,
                                                                         const int* __restrict__ pool, uint8_t* __restrict__ tmp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ph_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t* gray = ph_lds + (size_t)wave * wpad;
  uint8_t* outrow = ph_lds + (size_t)PH_WAVES * wpad + wave * PH_SIDE;
  const uint32_t step = gridDim.x * PH_WAVES;
  for (uint32_t row0 = blockIdx.x * PH_WAVES; row0 < rows; row0 += step) {      // rows + step < 2^32: the launch function checks
    const uint32_t row = row0 + wave;
    int kh = 0, bh = 0, ksize = 0;
    bool live = row < rows;
    if (live) {
      int a = 0, b = n - 1;                               // the last image whose first_row <= row; wave-uniform
      while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (descs[m].first_row <= row) a = m; else b = m - 1;
      }
      const PhashDesc d = descs[a];
      live = !d.tall;                                     // the 32 rows of a tall image are phash_tall_kernel's
      if (live) {
        kh = d.kh; bh = d.bh; ksize = d.ksize_h;
        const size_t rb = (size_t)d.w * 3;
        ph_row_gray(d.src + (size_t)(row - d.first_row) * rb, d.src, d.src + (size_t)d.h * rb, d.w, c0, c2, lane, gray);
      }
    }
    __syncthreads();
    if (live) ph_row_hpass(gray, pool + kh, pool + bh, ksize, lane, outrow);
    __syncthreads();
    if (live && lane < PH_SIDE / 4)
      reinterpret_cast<uint32_t*>(tmp + (size_t)row * PH_SIDE)[lane] = reinterpret_cast<const uint32_t*>(outrow)[lane];
  }
}

// Tall images (phash_mixed_plan.h: more than 100 times taller than wide, where Image.resize runs the vertical pass first): grid
// (32 output rows, image), an image that is not tall leaves at once. Row oy of the [32][w] intermediate is made from gray computed on
// the fly and parked in LDS as bytes (w < 656: h <= 65536 and h > 100 w), then the horizontal pass over it gives row oy of the image's 32
// rows of tmp; stage 2 applies the identity to them.
constexpr int PH_TALL_W = 1024;
__global__ __launch_bounds__(256) void phash_tall_kernel(const PhashDesc* __restrict__ descs, int c0, int c2, const int* __restrict__ pool,
                                                         uint8_t* __restrict__ tmp) {
  __shared__ uint8_t vrow[PH_TALL_W];
  const PhashDesc d = descs[blockIdx.y];
  if (!d.tall || d.w > PH_TALL_W) return;
  const int oy = blockIdx.x;
  const int ymin = pool[d.bt + 2 * oy], yn = pool[d.bt + 2 * oy + 1];   // ymin + yn <= h
  const int* kv = pool + d.kt + (size_t)oy * d.ksize_t;
  for (int x = threadIdx.x; x < d.w; x += blockDim.x) {
    const uint8_t* p = d.src + ((size_t)ymin * d.w + x) * 3;
    int s = 1 << (PH_BITS - 1);
    for (int t = 0; t < yn; ++t) {
      s += (((int)p[0] * c0 + (int)p[1] * 38470 + (int)p[2] * c2 + 0x8000) >> 16) * kv[t];
      p += (size_t)d.w * 3;
    }
    vrow[x] = (uint8_t)ph_clip8(s);
  }
  __syncthreads();
  if (threadIdx.x < PH_SIDE) {
    const int o = threadIdx.x;
    const int xmin = pool[d.bh + 2 * o], xn = pool[d.bh + 2 * o + 1];   // xmin + xn <= w
    const int* k = pool + d.kh + (size_t)o * d.ksize_h;
    int s = 1 << (PH_BITS - 1);
    for (int t = 0; t < xn; ++t) s += (int)vrow[xmin + t] * k[t];
    tmp[((size_t)d.first_row + oy) * PH_SIDE + o] = (uint8_t)ph_clip8(s);
  }
}

// One image by one workgroup of 1024: tmp [h][32] -> small [32][32] (vertical pass), lo = dct(dct(small, axis 0), axis 1)[:8, :8], hash.
// cosv [8][32] doubles; hash / small_out (nullable) / dct_out (nullable) are this image's. Both finish kernels are this function, so
// their doubles are the same.
__device__ __forceinline__ void ph_finish(const uint8_t* __restrict__ tmp, const int* __restrict__ kk, const int* __restrict__ bounds, int ksize,
                                          const double* __restrict__ cosv, unsigned long long* __restrict__ hash, uint8_t* __restrict__ small_out,
                                          double* __restrict__ dct_out) {
  __shared__ double small[PH_SIDE][PH_SIDE + 1];
  __shared__ double cs[8][PH_SIDE];
  __shared__ double a0[8][PH_SIDE + 1];
  __shared__ double lo[64], sorted[64];
  const int tid = threadIdx.x;
  const int oy = tid >> 5, x = tid & 31;
  if (tid < 8 * PH_SIDE) cs[tid >> 5][tid & 31] = cosv[tid];
  {
    const int ymin = bounds[2 * oy], yn = bounds[2 * oy + 1];   // ymin + yn <= h
    const int* k = kk + (size_t)oy * ksize;
    const uint8_t* p = tmp + (size_t)ymin * PH_SIDE + x;
    int s = 1 << (PH_BITS - 1);
    for (int t = 0; t < yn; ++t) s += (int)p[(size_t)t * PH_SIDE] * k[t];
    const int v = ph_clip8(s);
    small[oy][x] = (double)v;
    if (small_out) small_out[tid] = (uint8_t)v;
  }
  __syncthreads();
  if (tid < 8 * PH_SIDE) {                 // axis 0: a0[k][x] = 2 sum_y small[y][x] cos(pi k (2y+1) / 64)
    const int k = tid >> 5;
    double s = 0.0;
    for (int y = 0; y < PH_SIDE; ++y) s += small[y][x] * cs[k][y];
    a0[k][x] = 2.0 * s;
  }
  __syncthreads();
  if (tid < 64) {                          // axis 1: lo[k][l] = 2 sum_x a0[k][x] cos(pi l (2x+1) / 64)
    const int k = tid >> 3, l = tid & 7;
    double s = 0.0;
    for (int xx = 0; xx < PH_SIDE; ++xx) s += a0[k][xx] * cs[l][xx];
    lo[tid] = 2.0 * s;
    if (dct_out) dct_out[tid] = 2.0 * s;
  }
  __syncthreads();
  if (tid < 64) {                          // rank sort of the 64 values (ties by index), numpy.median = mean of the two middle ones
    const double v = lo[tid];
    int r = 0;
    for (int j = 0; j < 64; ++j) r += (lo[j] < v || (lo[j] == v && j < tid)) ? 1 : 0;
    sorted[r] = v;
  }
  __syncthreads();
  if (tid < 64) {
    const double med = (sorted[31] + sorted[32]) / 2.0;
    const unsigned long long m = __ballot(lo[tid] > med);      // lane i = bit i of the row-major block; the string starts with bit 0
    if (tid == 0) *hash = __brevll(m);
  }
}

// tmp [n][h][32], one block per image
__global__ __launch_bounds__(1024) void phash_finish_kernel(const uint8_t* __restrict__ tmp, int h, const int* __restrict__ kk,
                                                            const int* __restrict__ bounds, int ksize, const double* __restrict__ cosv,
                                                            unsigned long long* __restrict__ hashes, uint8_t* __restrict__ small_out,
                                                            double* __restrict__ dct_out) {
  const int img = blockIdx.x;
  ph_finish(tmp + (size_t)img * h * PH_SIDE, kk, bounds, ksize, cosv, hashes + img, small_out ? small_out + (size_t)img * PH_SIDE * PH_SIDE : nullptr,
            dct_out ? dct_out + (size_t)img * 64 : nullptr);
}

// fe_phash_mixed's stage 2: one block per image, its rows of tmp and its vertical table from the descriptor
__global__ __launch_bounds__(1024) void phash_finish_mixed_kernel(const PhashDesc* __restrict__ descs, const int* __restrict__ pool,
                                                                  const uint8_t* __restrict__ tmp, const double* __restrict__ cosv,
                                                                  unsigned long long* __restrict__ hashes, uint8_t* __restrict__ small_out,
                                                                  double* __restrict__ dct_out) {
  const int img = blockIdx.x;
  const PhashDesc d = descs[img];
  ph_finish(tmp + (size_t)d.first_row * PH_SIDE, pool + d.kv, pool + d.bv, d.ksize_v, cosv, hashes + img,
            small_out ? small_out + (size_t)img * PH_SIDE * PH_SIDE : nullptr, dct_out ? dct_out + (size_t)img * 64 : nullptr);
}

static const ResizeCoeffsDev& phash_coeffs(Ctx& c, int in_size) {
  // stage 1 / 2's own tables, cached under FE_FILTER_KEY_PHASH: (in, 32, LANCZOS), or the identity when in == 32 - PIL skips a
  // pass whose axis already has the size, and a single tap of 1.0 reproduces a byte exactly
  const auto key = std::make_tuple(in_size, PH_SIDE, FE_FILTER_KEY_PHASH);
  auto it = c.resize_cache.find(key);
  if (it != c.resize_cache.end()) return it->second;
  ResizeCoeffs rc;
  if (in_size == PH_SIDE) {
    rc.ksize = 1; rc.out = PH_SIDE;
    rc.kk.assign(PH_SIDE, 1 << PH_BITS);
    rc.bounds.resize(2 * PH_SIDE);
    for (int i = 0; i < PH_SIDE; ++i) { rc.bounds[2 * i] = i; rc.bounds[2 * i + 1] = 1; }
  } else {
    build_resize_coeffs(in_size, PH_SIDE, FE_FILTER_LANCZOS, rc);
  }
  for (int i = 0; i < PH_SIDE; ++i)
    FE_CHECK(rc.bounds[2 * i] >= 0 && rc.bounds[2 * i + 1] >= 0 && rc.bounds[2 * i + 1] <= rc.ksize && rc.bounds[2 * i] + rc.bounds[2 * i + 1] <= in_size,
             "phash: coefficient window leaves the axis");
  return upload_resize_coeffs(c, key, rc);
}

void phash_cos_table(double* out) {      // [8][32]: cos(pi k (2n+1) / 64)
  for (int k = 0; k < 8; ++k)
    for (int n = 0; n < PH_SIDE; ++n) out[k * PH_SIDE + n] = std::cos(M_PI * (double)k * (double)(2 * n + 1) / 64.0);
}

size_t phash_tmp_bytes(int n, int h) { return (size_t)n * h * PH_SIDE; }

// d_img [n][h][w][3] device; d_tmp: phash_tmp_bytes scratch; d_cos [8][32]; d_hashes [n]; d_small [n][32][32] / d_dct [n][64] nullable
void launch_phash(Ctx& c, const uint8_t* d_img, int n, int h, int w, int bgr, uint8_t* d_tmp, const double* d_cos, uint64_t* d_hashes,
                  uint8_t* d_small, double* d_dct) {
  FE_CHECK(n > 0 && h > 0 && w > 0 && w <= 32768 && h <= 65536, "phash: bad shape %d x %d x %d", n, h, w);
  const ResizeCoeffsDev& ch = phash_coeffs(c, w);
  const ResizeCoeffsDev& cv = phash_coeffs(c, h);
  const int wpad = (w + 255) & ~255;
  const size_t lds = (size_t)PH_WAVES * wpad + PH_WAVES * PH_SIDE;
  static std::atomic<uint64_t> lds_set{0};
  ensure_dynamic_lds((const void*)phash_rows_kernel, (size_t)PH_WAVES * 32768 + PH_WAVES * PH_SIDE, lds_set);
  const size_t rows = (size_t)n * h;
  const size_t blocks = std::min<size_t>((rows + PH_WAVES - 1) / PH_WAVES, 8192);
  hipLaunchKernelGGL(phash_rows_kernel, dim3((unsigned)blocks), dim3(PH_WAVES * 64), lds, c.stream, d_img, rows, w, wpad, bgr ? 7471 : 19595,
                     bgr ? 19595 : 7471, ch.kk, ch.bounds, ch.ksize, d_tmp);
  FE_HIP(hipGetLastError());
  hipLaunchKernelGGL(phash_finish_kernel, dim3(n), dim3(1024), 0, c.stream, d_tmp, h, cv.kk, cv.bounds, cv.ksize, d_cos,
                     (unsigned long long*)d_hashes, d_small, d_dct);
  FE_HIP(hipGetLastError());
}

// One chunk of fe_phash_mixed. d_descs [n] (first_row ascending from 0), rows: the chunk's total, max_w: its widest image, d_pool: the
// call's tables, d_tmp [rows][32] scratch; any_tall: the chunk has a tall image (one more launch); outputs as launch_phash's.
void launch_phash_mixed(Ctx& c, const PhashDesc* d_descs, int n, size_t rows, int max_w, int any_tall, int bgr, const int32_t* d_pool, uint8_t* d_tmp,
                        const double* d_cos, uint64_t* d_hashes, uint8_t* d_small, double* d_dct) {
  FE_CHECK(n > 0 && rows >= (size_t)n && rows < ((size_t)1 << 31) && max_w > 0 && max_w <= 32768, "phash_mixed: bad chunk (%d images, %zu rows, width %d)", n,
           rows, max_w);
  const int wpad = (max_w + 255) & ~255;
  const size_t lds = (size_t)PH_WAVES * wpad + PH_WAVES * PH_SIDE;
  static std::atomic<uint64_t> lds_set{0};
  ensure_dynamic_lds((const void*)phash_rows_mixed_kernel, (size_t)PH_WAVES * 32768 + PH_WAVES * PH_SIDE, lds_set);
  const size_t blocks = std::min<size_t>((rows + PH_WAVES - 1) / PH_WAVES, 8192);
  hipLaunchKernelGGL(phash_rows_mixed_kernel, dim3((unsigned)blocks), dim3(PH_WAVES * 64), lds, c.stream, d_descs, n, (uint32_t)rows, wpad,
                     bgr ? 7471 : 19595, bgr ? 19595 : 7471, (const int*)d_pool, d_tmp);
  FE_HIP(hipGetLastError());
  if (any_tall) {
    FE_CHECK(n <= 65535, "phash_mixed: %d images in a chunk with a tall one (at most 65535)", n);
    hipLaunchKernelGGL(phash_tall_kernel, dim3(PH_SIDE, n), dim3(256), 0, c.stream, d_descs, bgr ? 7471 : 19595, bgr ? 19595 : 7471, (const int*)d_pool, d_tmp);
    FE_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(phash_finish_mixed_kernel, dim3(n), dim3(1024), 0, c.stream, d_descs, (const int*)d_pool, d_tmp, d_cos,
                     (unsigned long long*)d_hashes, d_small, d_dct);
  FE_HIP(hipGetLastError());
}

// ---- all pairs i < j with popcount(hash_i ^ hash_j) <= maxd --------------------------------------------------------------
constexpr int HP_TILE = 256;

// grid (i-tiles, strips): block (ti, s) walks the j-tiles ti + s, ti + s + strips, ... < tiles. Row ti of the triangle has
// tiles - ti tiles, so the blocks shrink with blockIdx.x: the longest are dispatched first and the short ones fill the tail
// (pairing each row with its mirror, equal work per block in a single resident wave, measured slower: profiles/phash_perf.txt).
// pairs [cap][2]; *count: all hits.
__global__ __launch_bounds__(HP_TILE) void hamming_pairs_kernel(const unsigned long long* __restrict__ hashes, int n, int tiles, int maxd,
                                                                unsigned long long cap, int* __restrict__ pairs,
                                                                unsigned long long* __restrict__ count) {
  __shared__ unsigned long long hj[HP_TILE];
  const int ti = blockIdx.x, lane = threadIdx.x & 63;
  const int i = ti * HP_TILE + threadIdx.x;
  const unsigned long long mine = i < n ? hashes[i] : 0ull;
  for (int tj = ti + blockIdx.y; tj < tiles; tj += gridDim.y) {
    const int j0 = tj * HP_TILE;
    __syncthreads();
    hj[threadIdx.x] = j0 + (int)threadIdx.x < n ? hashes[j0 + threadIdx.x] : 0ull;
    __syncthreads();
    const int jn = min(HP_TILE, n - j0);
    for (int jj = 0; jj < jn; jj += 4) {                          // the tile's tail is zero-filled and fails j < n
      bool hit[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = j0 + jj + k;
        hit[k] = i < j && j < n && __popcll(mine ^ hj[jj + k]) <= maxd;
      }
      if (__ballot(hit[0] | hit[1] | hit[2] | hit[3]) == 0) continue;   // wave-uniform: hits are rare, four columns per test
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned long long m = __ballot(hit[k]);
        if (!m) continue;
        unsigned long long base = 0;                              // one atomic for the wave's hits of this column
        const int lead = __ffsll((long long)m) - 1;
        if (lane == lead) base = atomicAdd(count, (unsigned long long)__popcll(m));
        base = __shfl(base, lead);
        if (hit[k]) {
          const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
          if (at < cap) { pairs[2 * at] = i; pairs[2 * at + 1] = j0 + jj + k; }
        }
      }
    }
  }
}

void launch_hamming_pairs(const uint64_t* d_hashes, int n, int maxd, int64_t cap, int* d_pairs, unsigned long long* d_count, hipStream_t s) {
  FE_CHECK(n >= 2 && cap >= 0 && (cap == 0 || d_pairs), "hamming_pairs: bad arguments");
  const int tiles = (n + HP_TILE - 1) / HP_TILE;
  const int strips = std::max(1, std::min(tiles, 4096 / tiles));
  FE_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(hamming_pairs_kernel, dim3(tiles, strips), dim3(HP_TILE), 0, s, (const unsigned long long*)d_hashes, n, tiles, maxd,
                     (unsigned long long)cap, d_pairs, d_count);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
