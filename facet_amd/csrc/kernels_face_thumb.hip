// Face thumbnails: Pillow's BOX resize and libjpeg's bytes for m crops of a resident BGR batch, every crop with its own rectangle and
// output size (reference analyzers/face.py:43-82; facet_amd.face.face_thumbnail_plan gives the rectangles and sizes).
//
// One descriptor per face (FaceThumb) carries the source image, the rectangle, the output size and the offsets of the face's slices
// of the shared buffers; three or four launches serve all faces of a call:
//   hpass:  grid (chunks, m): libImaging/Resample.c's horizontal pass over the crop taken as its own image -> uint8 [ch][ow][3]
//   vpass:  grid (chunks, m): the vertical pass over that -> uint8 [oh][ow][3] (still B,G,R)
//   encode: one workgroup per face runs the five passes of kernels_jpeg.hip (coeff, bits, scan, write, stuff) back to back with
//           barriers between them. Faces of up to FT_LDS_BLOCKS blocks (128 x 128 pixels) keep coefficients, bit lengths and the bit
//           buffer in LDS (face_jpeg_kernel<true>); larger ones run the same code over slices of arena scratch (<false>).
// BOX coefficients need no table: every tap inside the window weighs 1, so after normalisation all of them are 1 / count and the
// 22-bit integer is (int)(0.5 + (1.0 / count) * 2^22). The window is found with Resample.c's own double expressions; the scale, the
// support and 1 / filterscale come from the host, and this file is compiled without FMA contraction like the rest of the engine.
#include "engine.h"
#include "jpeg_core.h"

namespace fe {

using namespace jpeg;

const Tables* jpeg_tables(Ctx& c, int h, int w, int quality);      // kernels_jpeg.hip; (0, 0, q): the header's size fields are patched per face

constexpr int FT_THREADS = 256;
constexpr int FT_STRIP = 16;             // bytes per thread and trip of the stuffing pass
constexpr int FT_LDS_BLOCKS = 6 * 8 * 8; // 128 x 128 pixels: 48 KiB of coefficients, 1.5 KiB of bit lengths, 78 KiB of bit buffer
constexpr int FT_SOF_SIZE = 163;         // header bytes 163..166: height, width (big endian) of SOF0

struct FaceThumb {
  int img, x0, y0, cw, ch, ow, oh;       // source image, crop origin and size, output size
  uint32_t wcap;                         // words of the face's bit buffer (a multiple of 4)
  double sx, supx, ssx, sy, supy, ssy;   // per axis: scale, support, 1 / filterscale (Resample.c precompute_coeffs)
  size_t mid_off, pix_off;               // bytes into the intermediate [ch][ow][3] / pixel [oh][ow][3] buffers
  size_t coef_off, bits_off, bitbuf_off; // elements into the global coefficient (int16) / bit length (u32) / bit buffer (u32) scratch
};

static uint32_t bitbuf_words(int nblk) { return (uint32_t)((((size_t)nblk * ((BLOCK_MAX_BITS + 7) / 8) + 15) & ~(size_t)15) / 4); }

// ---- BOX resample ----------------------------------------------------------------------------------------------------------------
// Output sample xx of an axis of `in` samples: first tap and the common 22-bit coefficient of its window (count taps).
__device__ __forceinline__ void box_window(int xx, int in, double scale, double support, double ss, int& first, int& count, int& kc) {
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  first = xmin; count = 0;
  for (int x = 0; x < xmax; ++x) {
    const double a = (x + xmin - center + 0.5) * ss;
    if (a > -0.5 && a <= 0.5) { if (!count) first = xmin + x; ++count; }
  }
  kc = count ? (int)(0.5 + (1.0 / (double)count) * 4194304.0) : 0;
}

__device__ __forceinline__ uint8_t clip8_22(int v) { v >>= 22; return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// src rows of the crop inside the photo -> mid [ch][ow][3]
__global__ __launch_bounds__(FT_THREADS) void face_hpass_kernel(const uint8_t* __restrict__ bgr, int h, int w, const FaceThumb* __restrict__ descs,
                                                                uint8_t* __restrict__ mid) {
  const FaceThumb d = descs[blockIdx.y];
  const int total = d.ch * d.ow;
  const uint8_t* src = bgr + (((size_t)d.img * h + d.y0) * w + d.x0) * 3;
  uint8_t* dst = mid + d.mid_off;
  for (int i = blockIdx.x * FT_THREADS + threadIdx.x; i < total; i += gridDim.x * FT_THREADS) {
    const int xx = i % d.ow, yy = i / d.ow;
    int first, count, kc;
    box_window(xx, d.cw, d.sx, d.supx, d.ssx, first, count, kc);
    const uint8_t* p = src + ((size_t)yy * w + first) * 3;
    int s0 = 0, s1 = 0, s2 = 0;
    for (int x = 0; x < count; ++x) { s0 += p[0]; s1 += p[1]; s2 += p[2]; p += 3; }
    uint8_t* o = dst + (size_t)i * 3;
    o[0] = clip8_22((1 << 21) + s0 * kc); o[1] = clip8_22((1 << 21) + s1 * kc); o[2] = clip8_22((1 << 21) + s2 * kc);
  }
}

// The same pass for a list of images of any sizes (fe_face_thumbnails_mixed): source pointer and width of the face's image come from its
// descriptor (face_mixed_plan.h); rgb: the source pixels are R,G,B, and mid is written B,G,R as the passes after this one read it.
__global__ __launch_bounds__(FT_THREADS) void face_hpass_mixed_kernel(const face_plan::ImageDesc* __restrict__ imgs, int rgb, const FaceThumb* __restrict__ descs,
                                                                      uint8_t* __restrict__ mid) {
  const FaceThumb d = descs[blockIdx.y];
  const face_plan::ImageDesc im = imgs[d.img];
  const int total = d.ch * d.ow;
  const int w = im.w;
  const uint8_t* src = im.src + ((size_t)d.y0 * w + d.x0) * 3;
  uint8_t* dst = mid + d.mid_off;
  for (int i = blockIdx.x * FT_THREADS + threadIdx.x; i < total; i += gridDim.x * FT_THREADS) {
    const int xx = i % d.ow, yy = i / d.ow;
    int first, count, kc;
    box_window(xx, d.cw, d.sx, d.supx, d.ssx, first, count, kc);
    const uint8_t* p = src + ((size_t)yy * w + first) * 3;
    int s0 = 0, s1 = 0, s2 = 0;
    for (int x = 0; x < count; ++x) { s0 += p[0]; s1 += p[1]; s2 += p[2]; p += 3; }
    if (rgb) { const int t = s0; s0 = s2; s2 = t; }
    uint8_t* o = dst + (size_t)i * 3;
    o[0] = clip8_22((1 << 21) + s0 * kc); o[1] = clip8_22((1 << 21) + s1 * kc); o[2] = clip8_22((1 << 21) + s2 * kc);
  }
}

// mid [ch][ow][3] -> pix [oh][ow][3]
__global__ __launch_bounds__(FT_THREADS) void face_vpass_kernel(const FaceThumb* __restrict__ descs, const uint8_t* __restrict__ mid,
                                                                uint8_t* __restrict__ pix) {
  const FaceThumb d = descs[blockIdx.y];
  const int total = d.oh * d.ow;
  const uint8_t* src = mid + d.mid_off;
  uint8_t* dst = pix + d.pix_off;
  for (int i = blockIdx.x * FT_THREADS + threadIdx.x; i < total; i += gridDim.x * FT_THREADS) {
    const int xx = i % d.ow, yy = i / d.ow;
    int first, count, kc;
    box_window(yy, d.ch, d.sy, d.supy, d.ssy, first, count, kc);
    const uint8_t* p = src + ((size_t)first * d.ow + xx) * 3;
    int s0 = 0, s1 = 0, s2 = 0;
    for (int y = 0; y < count; ++y) { s0 += p[0]; s1 += p[1]; s2 += p[2]; p += (size_t)d.ow * 3; }
    uint8_t* o = dst + (size_t)i * 3;
    o[0] = clip8_22((1 << 21) + s0 * kc); o[1] = clip8_22((1 << 21) + s1 * kc); o[2] = clip8_22((1 << 21) + s2 * kc);
  }
}

// ---- encode: one workgroup per face ----------------------------------------------------------------------------------------------
// exclusive scan of v over the FT_THREADS lanes; *total receives the sum. buf: FT_THREADS words of LDS.
__device__ __forceinline__ uint32_t ft_exclusive_scan(uint32_t v, uint32_t* buf, uint32_t* total) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int d = 1; d < FT_THREADS; d <<= 1) {
    const uint32_t a = t >= d ? buf[t - d] : 0;
    __syncthreads();
    buf[t] += a;
    __syncthreads();
  }
  const uint32_t incl = buf[t];
  *total = buf[FT_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// big-endian bit writer as in kernels_jpeg.hip: bit p of the stream is bit 31 - (p & 31) of word p >> 5; neighbours share words
struct FtWordSink {
  uint32_t* words;
  uint32_t wi, wcap, acc;
  int fill;
  __device__ __forceinline__ void flush() {
    if (wi < wcap && acc) atomicOr(words + wi, acc);
    ++wi; acc = 0; fill = 0;
  }
  __device__ __forceinline__ void put(unsigned code, int len) {
    const int room = 32 - fill;
    if (len <= room) {
      acc |= len == 32 ? code : code << (room - len);
      fill += len;
      if (fill == 32) flush();
    } else {
      acc |= code >> (len - room);
      flush();
      acc = code << (32 - (len - room));
      fill = len - room;
    }
  }
};

// list[blockIdx.x]: the face this workgroup encodes. out [m][cap], lengths [m] as jpeg_stuff_kernel leaves them. LDS: the face has at most
// FT_LDS_BLOCKS blocks and its three work arrays live in the dynamic LDS of the launch; otherwise in the g* scratch at the descriptor's offsets.
template <bool LDS>
__global__ __launch_bounds__(FT_THREADS) void face_jpeg_kernel(const FaceThumb* __restrict__ descs, const int* __restrict__ list, const uint8_t* __restrict__ pix,
                                                               const Tables* __restrict__ tab, int16_t* __restrict__ gcoef, uint32_t* __restrict__ gbits,
                                                               uint32_t* __restrict__ gbitbuf, uint8_t* __restrict__ out, size_t cap, int32_t* __restrict__ lengths) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ft_lds[];
  __shared__ Huff H;
  __shared__ uint16_t q[128];
  __shared__ uint32_t sbuf[FT_THREADS];
  const int t = threadIdx.x;
  const int f = list[blockIdx.x];
  const FaceThumb d = descs[f];
  const Geom g = make_geom(d.oh, d.ow);
  const int nblk = g.nblk;
  uint32_t wcap = d.wcap;
  int16_t* coef;
  uint32_t *bits, *bitbuf;
  if (LDS) {
    if (nblk > FT_LDS_BLOCKS) {                                       // the host sorts faces by size; never taken
      if (t == 0) lengths[f] = INT32_MIN;
      return;
    }
    coef = reinterpret_cast<int16_t*>(ft_lds);
    bits = reinterpret_cast<uint32_t*>(ft_lds + (size_t)FT_LDS_BLOCKS * 128);
    bitbuf = bits + FT_LDS_BLOCKS;
    wcap = min(wcap, (uint32_t)(FT_LDS_BLOCKS * ((BLOCK_MAX_BITS + 7) / 8) / 4));
  } else {
    coef = gcoef + d.coef_off; bits = gbits + d.bits_off; bitbuf = gbitbuf + d.bitbuf_off;
  }
  for (int i = t; i < (int)(sizeof(Huff) / 4); i += FT_THREADS) reinterpret_cast<uint32_t*>(&H)[i] = reinterpret_cast<const uint32_t*>(&tab->huff)[i];
  if (t < 128) q[t] = (&tab->q[0][0])[t];
  for (uint32_t i = t; i < wcap; i += FT_THREADS) bitbuf[i] = 0;
  __syncthreads();
  // coeff
  const uint8_t* img = pix + d.pix_off;
  for (int b = t; b < nblk; b += FT_THREADS) {
    const int m = b / 6;
    int16_t zz[64];
    block_coeffs(img, g, 1, m / g.mw, m % g.mw, b % 6, q, zz);
    uint32_t* o = reinterpret_cast<uint32_t*>(coef + (size_t)b * 64);
#pragma unroll
    for (int v = 0; v < 32; ++v) o[v] = (uint16_t)zz[2 * v] | ((uint32_t)(uint16_t)zz[2 * v + 1] << 16);
  }
  __syncthreads();
  // bits, then their exclusive scan in place (tiles of FT_THREADS with a carry)
  for (int b = t; b < nblk; b += FT_THREADS) {
    CountSink s;
    encode_block(coef + (size_t)b * 64, dc_pred(coef, b), (b % 6) < 4 ? 0 : 1, H, s);
    bits[b] = s.bits;
  }
  __syncthreads();
  uint32_t carry = 0;
  for (int b0 = 0; b0 < nblk; b0 += FT_THREADS) {
    const int b = b0 + t;
    uint32_t tot;
    const uint32_t ex = ft_exclusive_scan(b < nblk ? bits[b] : 0, sbuf, &tot);
    if (b < nblk) bits[b] = carry + ex;
    carry += tot;
  }
  const uint32_t T = (carry + 7) >> 3;                                // unstuffed scan bytes after the final padding; uniform
  __syncthreads();
  // write
  for (int b = t; b < nblk; b += FT_THREADS) {
    const uint32_t off = bits[b];
    FtWordSink s;
    s.words = bitbuf; s.wcap = wcap; s.wi = off >> 5; s.acc = 0; s.fill = (int)(off & 31);
    encode_block(coef + (size_t)b * 64, dc_pred(coef, b), (b % 6) < 4 ? 0 : 1, H, s);
    if (b == nblk - 1) {                                              // the end of the scan is padded to a byte with 1-bits
      const int pad = (8 - (s.fill & 7)) & 7;
      if (pad) s.put((1u << pad) - 1, pad);
    }
    if (s.fill) s.flush();
  }
  __syncthreads();
  // stuff: header with this face's size, the scan with a 0x00 after every 0xFF, EOI; every store checked against cap
  uint8_t* o = out + (size_t)f * cap;
  if ((size_t)T > (size_t)wcap * 4) {                                 // uniform; the bit buffer's size rules it out
    if (t == 0) lengths[f] = INT32_MIN;
    return;
  }
  for (int i = t; i < HEADER_BYTES; i += FT_THREADS) {
    uint8_t v = tab->header[i];
    if (i == FT_SOF_SIZE) v = (uint8_t)(d.oh >> 8);
    else if (i == FT_SOF_SIZE + 1) v = (uint8_t)(d.oh & 255);
    else if (i == FT_SOF_SIZE + 2) v = (uint8_t)(d.ow >> 8);
    else if (i == FT_SOF_SIZE + 3) v = (uint8_t)(d.ow & 255);
    if ((size_t)i < cap) o[i] = v;
  }
  size_t pos0 = HEADER_BYTES;                                         // where the next unstuffed byte lands
  for (uint32_t s0 = 0; s0 < T; s0 += FT_THREADS * FT_STRIP) {
    const uint32_t first = s0 + (uint32_t)t * FT_STRIP;
    uint32_t w[4] = {0, 0, 0, 0};
    if (first < T) {                                                  // first / 4 + 3 < wcap: wcap is a multiple of 4 and T <= 4 wcap
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = bitbuf[first / 4 + j];
    }
    const int nb = first < T ? (int)min((uint32_t)FT_STRIP, T - first) : 0;
    uint32_t ff = 0;
#pragma unroll
    for (int j = 0; j < FT_STRIP; ++j) ff += (j < nb && ((w[j >> 2] >> (24 - 8 * (j & 3))) & 255u) == 255u) ? 1u : 0u;
    uint32_t tot;
    const uint32_t before = ft_exclusive_scan(ff, sbuf, &tot);
    size_t pos = pos0 + (first - s0) + before;
#pragma unroll
    for (int j = 0; j < FT_STRIP; ++j) {
      if (j < nb) {
        const uint32_t v = (w[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
        if (pos < cap) o[pos] = (uint8_t)v;
        ++pos;
        if (v == 255u) { if (pos < cap) o[pos] = 0; ++pos; }
      }
    }
    pos0 += (size_t)min((uint32_t)(FT_THREADS * FT_STRIP), T - s0) + tot;
  }
  if (t == 0) {
    const size_t len = pos0 + 2;
    if (len <= cap) { o[pos0] = 0xFF; o[pos0 + 1] = 0xD9; lengths[f] = (int32_t)len; }
    else lengths[f] = len < (size_t)INT32_MAX ? -(int32_t)len : INT32_MIN;
  }
}

static_assert(FT_LDS_BLOCKS == 6 * (FE_FACE_THUMB_FUSED_SIDE / 16) * (FE_FACE_THUMB_FUSED_SIDE / 16), "the header states the fused encoder's limit");

// img_index [m], crops [m][4], out_sizes [m][2] on the host and already validated. out [m][cap] and lengths [m] are host buffers with
// fe_jpeg_encode's contract. Returns false when a row was too small. Faces are served in groups whose scratch fits the arena; the
// scratch of a group is released (stream order) before the next one takes it. hpass(grid, d_desc, mid) launches the horizontal pass, the
// one kernel that reads the source images.
template <class HPass>
static bool face_thumbnails_run(Ctx& c, int m, const int32_t* img_index, const int32_t* crops, const int32_t* out_sizes, int quality, uint8_t* out, size_t cap,
                                int32_t* lengths, HPass&& hpass) {
  FE_CHECK(quality >= 1 && quality <= 100, "jpeg: quality %d (1 .. 100)", quality);
  const Tables* tab = jpeg_tables(c, 0, 0, quality);
  static std::atomic<uint64_t> lds_set{0};
  constexpr size_t LDS_BYTES = (size_t)FT_LDS_BLOCKS * (128 + 4) + (size_t)FT_LDS_BLOCKS * ((BLOCK_MAX_BITS + 7) / 8);
  static_assert(LDS_BYTES + sizeof(Huff) + 256 + FT_THREADS * 4 <= 160 * 1024, "the fused encoder's work arrays exceed the LDS of a CU");
  ensure_dynamic_lds((const void*)face_jpeg_kernel<true>, LDS_BYTES, lds_set);
  int max_oh = 1, max_ow = 1;
  for (int f = 0; f < m; ++f) { max_ow = std::max(max_ow, out_sizes[2 * f]); max_oh = std::max(max_oh, out_sizes[2 * f + 1]); }
  const size_t dcap = std::min(cap, jpeg_bound(max_oh, max_ow));        // no encode is longer, so the device rows need not be
  const size_t budget = std::min<size_t>((size_t)1 << 30, (c.arena.capacity() - c.arena.mark()) / 8 * 7);
  bool fits = true;
  std::vector<FaceThumb> descs;
  std::vector<int> list_lds, list_glb;
  std::vector<int32_t> lens;
  for (int f0 = 0; f0 < m;) {
    descs.clear(); list_lds.clear(); list_glb.clear();
    size_t mid_b = 0, pix_b = 0, coef_n = 0, bits_n = 0, bitbuf_n = 0, used = 0;
    int max_h = 1, max_v = 1, f1 = f0;
    for (; f1 < m; ++f1) {
      const int32_t* r = crops + 4 * f1;
      FaceThumb d;
      d.img = img_index[f1]; d.x0 = r[0]; d.y0 = r[1]; d.cw = r[2] - r[0]; d.ch = r[3] - r[1];
      d.ow = out_sizes[2 * f1]; d.oh = out_sizes[2 * f1 + 1];
      // Resample.c takes the box as C floats and the scale from their difference
      d.sx = (double)((float)r[2] - (float)r[0]) / d.ow; d.sy = (double)((float)r[3] - (float)r[1]) / d.oh;
      const double fx = d.sx < 1.0 ? 1.0 : d.sx, fy = d.sy < 1.0 ? 1.0 : d.sy;
      d.supx = 0.5 * fx; d.ssx = 1.0 / fx; d.supy = 0.5 * fy; d.ssy = 1.0 / fy;
      const int nblk = make_geom(d.oh, d.ow).nblk;
      d.wcap = bitbuf_words(nblk);
      const bool lds = nblk <= FT_LDS_BLOCKS;
      const size_t mid1 = ((size_t)d.ch * d.ow * 3 + 15) & ~(size_t)15, pix1 = ((size_t)d.oh * d.ow * 3 + 15) & ~(size_t)15;
      const size_t need = mid1 + pix1 + (lds ? 0 : (size_t)nblk * (128 + 4) + (size_t)d.wcap * 4) + dcap + sizeof(FaceThumb) + 16;
      if (f1 > f0 && (used + need > budget || f1 - f0 >= 32768)) break;      // 32768: gridDim.y
      used += need;
      d.mid_off = mid_b; d.pix_off = pix_b; d.coef_off = coef_n; d.bits_off = bits_n; d.bitbuf_off = bitbuf_n;
      mid_b += mid1; pix_b += pix1;
      if (!lds) { coef_n += (size_t)nblk * 64; bits_n += (size_t)nblk; bitbuf_n += d.wcap; }
      (lds ? list_lds : list_glb).push_back(f1 - f0);
      max_h = std::max(max_h, d.ch * d.ow); max_v = std::max(max_v, d.oh * d.ow);
      descs.push_back(d);
    }
    const int nb = f1 - f0;
    const size_t mark = c.arena.mark();
    FaceThumb* d_desc = (FaceThumb*)c.arena.alloc((size_t)nb * sizeof(FaceThumb));
    int* d_list = (int*)c.arena.alloc((size_t)nb * sizeof(int));
    uint8_t* mid = (uint8_t*)c.arena.alloc(mid_b);
    uint8_t* pix = (uint8_t*)c.arena.alloc(pix_b);
    int16_t* gcoef = (int16_t*)c.arena.alloc(std::max<size_t>(coef_n, 1) * 2);
    uint32_t* gbits = (uint32_t*)c.arena.alloc(std::max<size_t>(bits_n, 1) * 4);
    uint32_t* gbitbuf = (uint32_t*)c.arena.alloc(std::max<size_t>(bitbuf_n, 4) * 4);
    uint8_t* d_out = (uint8_t*)c.arena.alloc((size_t)nb * dcap);
    int32_t* d_len = (int32_t*)c.arena.alloc((size_t)nb * sizeof(int32_t));
    FE_HIP(hipMemcpyAsync(d_desc, descs.data(), (size_t)nb * sizeof(FaceThumb), hipMemcpyHostToDevice, c.stream));
    if (!list_lds.empty()) FE_HIP(hipMemcpyAsync(d_list, list_lds.data(), list_lds.size() * sizeof(int), hipMemcpyHostToDevice, c.stream));
    if (!list_glb.empty())
      FE_HIP(hipMemcpyAsync(d_list + list_lds.size(), list_glb.data(), list_glb.size() * sizeof(int), hipMemcpyHostToDevice, c.stream));
    hpass(dim3((unsigned)std::min((max_h + FT_THREADS - 1) / FT_THREADS, 64), nb), d_desc, mid);
    hipLaunchKernelGGL(face_vpass_kernel, dim3((unsigned)std::min((max_v + FT_THREADS - 1) / FT_THREADS, 64), nb), dim3(FT_THREADS), 0, c.stream, d_desc, mid,
                       pix);
    if (!list_lds.empty())
      hipLaunchKernelGGL(face_jpeg_kernel<true>, dim3((unsigned)list_lds.size()), dim3(FT_THREADS), LDS_BYTES, c.stream, d_desc, d_list, pix, tab, gcoef, gbits,
                         gbitbuf, d_out, dcap, d_len);
    if (!list_glb.empty())
      hipLaunchKernelGGL(face_jpeg_kernel<false>, dim3((unsigned)list_glb.size()), dim3(FT_THREADS), 0, c.stream, d_desc, d_list + list_lds.size(), pix, tab,
                         gcoef, gbits, gbitbuf, d_out, dcap, d_len);
    FE_HIP(hipGetLastError());
    lens.resize(nb);
    FE_HIP(hipMemcpyAsync(lens.data(), d_len, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    FE_HIP(hipStreamSynchronize(c.stream));
    for (int i = 0; i < nb; ++i) {
      const int32_t len = lens[i];
      lengths[f0 + i] = len;
      if (len <= 0 || (size_t)len > cap) { fits = false; continue; }
      FE_HIP(hipMemcpyAsync(out + (size_t)(f0 + i) * cap, d_out + (size_t)i * dcap, (size_t)len, hipMemcpyDeviceToHost, c.stream));
    }
    FE_HIP(hipStreamSynchronize(c.stream));      // the scratch is taken again by the next group
    c.arena.rewind(mark);
    f0 = f1;
  }
  return fits;
}

// d_bgr [n][h][w][3] on the device
bool face_thumbnails(Ctx& c, const uint8_t* d_bgr, int n, int h, int w, int m, const int32_t* img_index, const int32_t* crops, const int32_t* out_sizes,
                     int quality, uint8_t* out, size_t cap, int32_t* lengths) {
  return face_thumbnails_run(c, m, img_index, crops, out_sizes, quality, out, cap, lengths, [&](dim3 grid, const FaceThumb* d_desc, uint8_t* mid) {
    hipLaunchKernelGGL(face_hpass_kernel, grid, dim3(FT_THREADS), 0, c.stream, d_bgr, h, w, d_desc, mid);
  });
}

// d_imgs: device descriptors (src, h, w) of the images img_index refers to; rgb: their pixels are R,G,B
bool face_thumbnails_mixed(Ctx& c, const face_plan::ImageDesc* d_imgs, int rgb, int m, const int32_t* img_index, const int32_t* crops,
                           const int32_t* out_sizes, int quality, uint8_t* out, size_t cap, int32_t* lengths) {
  return face_thumbnails_run(c, m, img_index, crops, out_sizes, quality, out, cap, lengths, [&](dim3 grid, const FaceThumb* d_desc, uint8_t* mid) {
    hipLaunchKernelGGL(face_hpass_mixed_kernel, grid, dim3(FT_THREADS), 0, c.stream, d_imgs, rgb, d_desc, mid);
  });
}

}  // namespace fe
