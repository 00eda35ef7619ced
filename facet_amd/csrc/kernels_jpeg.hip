// Thumbnails: Pillow's integer box reduce (`Image.reduce`) and a baseline JPEG encoder that writes libjpeg's bytes.
//
// The reference stores `thumb.thumbnail((640, 640), LANCZOS); thumb.save(buf, "JPEG", quality=80)` per photo
// (utils/image_transforms.py:32-50, processing/scorer.py:1611-1617, :1680-1686). `Image.thumbnail` is reduce -> resize with a
// fractional box (kernels_resize.hip) -> libjpeg. The arithmetic of the encoder lives in jpeg_core.h; here are its passes over a batch:
//   coeff:  one lane per 8x8 block: colour conversion, h2v2 downsample, edge replication, DCT, quantiser, zigzag -> int16 [n][nblk][64]
//   bits:   one lane per block: the DC difference and the length of the block's Huffman code in bits
//   scan:   one workgroup per image: exclusive scan of the bit lengths (tiles of 1024 with a carry), pad to a byte
//   write:  one lane per block: the codes are OR-ed into a zeroed big-endian bit buffer at the block's offset (atomicOr: neighbours share words)
//   stuff:  one workgroup per image: counts the 0xFF bytes per 16-byte strip, scans, scatters the bytes behind the header with a 0x00
//           after every 0xFF, appends EOI and writes the length. Every store is checked against the caller's capacity.
//
// fe_thumbnail_jpeg_mixed (the last section) runs reduce, the two LANCZOS passes and the five encoder passes for a list of images of any
// sizes from per-image descriptors (thumb_mixed_core.h), one launch per stage.
#include "engine.h"
#include "jpeg_core.h"
#include "thumb_mixed_core.h"

namespace fe {

using namespace jpeg;

// ---- Image.reduce ----------------------------------------------------------------------------------------------------------------
// libImaging/Reduce.c rounds every mean as ((sum + count / 2) * multiplier) >> 24 with multiplier = (uint32)(2^32 / (256 count)) taken
// in float - its 2x2 / 4x4 / 1x2 / 2x1 shifts are that formula with an exact multiplier, the other special cases use it as it is -
// and the last column / row / corner (ImagingReduceCorners) average the samples that remain, with the count that remains.
// (pil_reduce_multiplier and pil_reduce_pixel: thumb_mixed_core.h, shared with the mixed-size path and its CPU harness.)
static uint32_t reduce_multiplier(int count) { return pil_reduce_multiplier(count); }

// src [n][h][w][3], box (x0, y0, bw, bh) -> dst [n][oh][ow][3]; mult[0..3]: interior, last column, last row, corner
__global__ void reduce_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, int h, int w, int x0, int y0, int bw, int bh,
                                 int fx, int fy, int oh, int ow, uint32_t m_in, uint32_t m_col, uint32_t m_row, uint32_t m_cor) {
  const size_t total = (size_t)n * oh * ow;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % ow, y = (i / ow) % oh;
    const size_t img = i / ((size_t)ow * oh);
    const int xs = x * fx, ys = y * fy;
    const int nx = min(fx, bw - xs), ny = min(fy, bh - ys);          // > 0: ow = ceil(bw / fx)
    const uint32_t mult = nx == fx ? (ny == fy ? m_in : m_row) : (ny == fy ? m_col : m_cor);
    pil_reduce_pixel(src + ((img * h + (y0 + ys)) * w + (x0 + xs)) * 3, (size_t)w * 3, nx, ny, mult, dst + i * 3);
  }
}

void reduce_u8(Ctx& c, const uint8_t* d_src, int n, int h, int w, int fx, int fy, const int box[4], uint8_t* d_dst) {
  const int bw = box[2] - box[0], bh = box[3] - box[1];
  FE_CHECK(n > 0 && fx >= 1 && fy >= 1 && box[0] >= 0 && box[1] >= 0 && bw > 0 && bh > 0 && box[2] <= w && box[3] <= h, "reduce: bad geometry");
  FE_CHECK((long long)fx * fy <= 65536, "reduce: factors %d x %d too large", fx, fy);      // 255 * count + count / 2 stays inside 32 bits
  const int ow = (bw + fx - 1) / fx, oh = (bh + fy - 1) / fy;
  const int rx = bw % fx ? bw % fx : fx, ry = bh % fy ? bh % fy : fy;
  const size_t work = (size_t)n * oh * ow;
  const size_t g = std::min<size_t>((work + 255) / 256, 8192);
  hipLaunchKernelGGL(reduce_u8_kernel, dim3((unsigned)std::max<size_t>(g, 1)), dim3(256), 0, c.stream, d_src, d_dst, n, h, w, box[0], box[1], bw, bh,
                     fx, fy, oh, ow, reduce_multiplier(fx * fy), reduce_multiplier(rx * fy), reduce_multiplier(fx * ry), reduce_multiplier(rx * ry));
  FE_HIP(hipGetLastError());
}

// ---- JPEG ------------------------------------------------------------------------------------------------------------------------
constexpr int JP_THREADS = 256;
constexpr int JP_SCAN = 1024;          // threads of the per-image scans
constexpr int JP_STRIP = 16;           // bytes per thread and trip of the stuffing pass

// block b of one image [g.h][g.w][3] -> its 64 quantised coefficients at coef (128 bytes, 16-byte aligned). q: [2][64] steps in LDS
__device__ __forceinline__ void jp_coeff_block(const uint8_t* img, const Geom& g, int bgr, int b, const uint16_t* q, int16_t* coef) {
  const int m = b / 6;
  int16_t zz[64];
  block_coeffs(img, g, bgr, m / g.mw, m % g.mw, b % 6, q, zz);
  uint4* o = reinterpret_cast<uint4*>(coef);
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    uint4 u;
    u.x = (uint16_t)zz[8 * v] | ((uint32_t)(uint16_t)zz[8 * v + 1] << 16);
    u.y = (uint16_t)zz[8 * v + 2] | ((uint32_t)(uint16_t)zz[8 * v + 3] << 16);
    u.z = (uint16_t)zz[8 * v + 4] | ((uint32_t)(uint16_t)zz[8 * v + 5] << 16);
    u.w = (uint16_t)zz[8 * v + 6] | ((uint32_t)(uint16_t)zz[8 * v + 7] << 16);
    o[v] = u;
  }
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_coeff_kernel(const uint8_t* __restrict__ img, int n, Geom g, int bgr, const Tables* __restrict__ tab,
                                                                int16_t* __restrict__ coef) {
  __shared__ uint16_t q[128];
  if (threadIdx.x < 128) q[threadIdx.x] = (&tab->q[0][0])[threadIdx.x];
  __syncthreads();
  const size_t total = (size_t)n * g.nblk;
  const size_t i = (size_t)blockIdx.x * JP_THREADS + threadIdx.x;
  if (i >= total) return;
  const size_t im = i / g.nblk;
  jp_coeff_block(img + im * (size_t)g.h * g.w * 3, g, bgr, (int)(i % g.nblk), q, coef + i * 64);
}

__device__ __forceinline__ void load_huff(Huff* dst, const Tables* tab) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&tab->huff);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (int t = threadIdx.x; t < (int)(sizeof(Huff) / 4); t += blockDim.x) d[t] = s[t];
  __syncthreads();
}
static_assert(sizeof(Huff) % 4 == 0 && offsetof(Tables, huff) % 4 == 0, "Huff is copied by dwords");

__global__ __launch_bounds__(JP_THREADS) void jpeg_bits_kernel(const int16_t* __restrict__ coef, int n, int nblk, const Tables* __restrict__ tab,
                                                               uint32_t* __restrict__ bits) {
  __shared__ Huff H;
  load_huff(&H, tab);
  const size_t i = (size_t)blockIdx.x * JP_THREADS + threadIdx.x;
  if (i >= (size_t)n * nblk) return;
  const size_t im = i / nblk;
  const int b = (int)(i % nblk);
  const int16_t* base = coef + im * (size_t)nblk * 64;
  CountSink s;
  encode_block(base + (size_t)b * 64, dc_pred(base, b), (b % 6) < 4 ? 0 : 1, H, s);
  bits[i] = s.bits;
}

// exclusive scan of v over the workgroup (JP_SCAN threads); *total receives the sum. buf: JP_SCAN words of LDS.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* buf, uint32_t* total) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int d = 1; d < JP_SCAN; d <<= 1) {
    const uint32_t a = t >= d ? buf[t - d] : 0;
    __syncthreads();
    buf[t] += a;
    __syncthreads();
  }
  const uint32_t incl = buf[t];
  *total = buf[JP_SCAN - 1];
  __syncthreads();
  return incl - v;
}

// One image by one workgroup of JP_SCAN: bits [nblk] -> offs [nblk] (bit offset of each block), *nbytes (unstuffed scan bytes after the
// final padding). Tiles of JP_SCAN with a carry. buf: JP_SCAN words of LDS.
__device__ __forceinline__ void jp_scan_image(const uint32_t* __restrict__ bits, int nblk, uint32_t* __restrict__ offs, uint32_t* __restrict__ nbytes,
                                              uint32_t* buf) {
  uint32_t carry = 0;
  for (int b0 = 0; b0 < nblk; b0 += JP_SCAN) {
    const int b = b0 + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan(b < nblk ? bits[b] : 0, buf, &tot);
    if (b < nblk) offs[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *nbytes = (carry + 7) >> 3;
}

// bits [n][nblk] -> offs [n][nblk] (bit offset of each block), nbytes[n] (unstuffed scan bytes after the final padding)
__global__ __launch_bounds__(JP_SCAN) void jpeg_scan_kernel(const uint32_t* __restrict__ bits, int nblk, uint32_t* __restrict__ offs,
                                                            uint32_t* __restrict__ nbytes) {
  __shared__ uint32_t buf[JP_SCAN];
  const size_t base = (size_t)blockIdx.x * nblk;
  jp_scan_image(bits + base, nblk, offs + base, nbytes + blockIdx.x, buf);
}

// big-endian bit writer into 32-bit words: bit p of the stream is bit 31 - (p & 31) of word p >> 5
struct WordSink {
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

// The Huffman code of block b of an image (coef: its [nblk][64] coefficients) OR-ed into its zeroed bit buffer `words` at bit `off`
__device__ __forceinline__ void jp_write_block(const int16_t* __restrict__ coef, int b, int nblk, uint32_t off, const Huff& H, uint32_t* __restrict__ words,
                                               uint32_t wcap) {
  WordSink s;
  s.words = words; s.wcap = wcap; s.wi = off >> 5; s.acc = 0; s.fill = (int)(off & 31);
  encode_block(coef + (size_t)b * 64, dc_pred(coef, b), (b % 6) < 4 ? 0 : 1, H, s);
  if (b == nblk - 1) {                                // the end of the scan is padded to a byte with 1-bits
    const int pad = (8 - (s.fill & 7)) & 7;
    if (pad) s.put((1u << pad) - 1, pad);
  }
  if (s.fill) s.flush();
}

// bitbuf [n][wcap] words, zeroed; wcap holds the longest possible scan, and a word index is still checked before every store.
__global__ __launch_bounds__(JP_THREADS) void jpeg_write_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ offs, int n, int nblk,
                                                                const Tables* __restrict__ tab, uint32_t* __restrict__ bitbuf, uint32_t wcap) {
  __shared__ Huff H;
  load_huff(&H, tab);
  const size_t i = (size_t)blockIdx.x * JP_THREADS + threadIdx.x;
  if (i >= (size_t)n * nblk) return;
  const size_t im = i / nblk;
  const int b = (int)(i % nblk);
  jp_write_block(coef + im * (size_t)nblk * 64, b, nblk, offs[i], H, bitbuf + im * (size_t)wcap, wcap);
}

constexpr int JP_SOF_SIZE = 163;       // header bytes 163..166: height, width (big endian) of SOF0

// One image by one workgroup of JP_SCAN: o [cap] <- header, stuffed scan, EOI. bits: the image's bit buffer of wcap words (a multiple of
// 4, 16-byte aligned) holding T bytes of scan. sof_h > 0: the header's size fields are written as sof_h x sof_w (tables made for (0, 0)).
// *length = the bytes written, or minus the bytes needed when that exceeds cap (nothing is stored at or past cap). INT32_MIN: the scan
// did not fit the bit buffer, which its size rules out. buf: JP_SCAN words of LDS.
__device__ __forceinline__ void jp_stuff_image(const uint32_t* __restrict__ bits, uint32_t wcap, uint32_t T, const Tables* __restrict__ tab, int sof_h,
                                               int sof_w, uint8_t* __restrict__ o, size_t cap, int32_t* __restrict__ length, uint32_t* buf) {
  const int t = threadIdx.x;
  if ((size_t)T > (size_t)wcap * 4) {                  // uniform over the workgroup
    if (t == 0) *length = INT32_MIN;
    return;
  }
  if (t < HEADER_BYTES && (size_t)t < cap) {
    uint8_t v = tab->header[t];
    if (sof_h > 0) {
      if (t == JP_SOF_SIZE) v = (uint8_t)(sof_h >> 8);
      else if (t == JP_SOF_SIZE + 1) v = (uint8_t)(sof_h & 255);
      else if (t == JP_SOF_SIZE + 2) v = (uint8_t)(sof_w >> 8);
      else if (t == JP_SOF_SIZE + 3) v = (uint8_t)(sof_w & 255);
    }
    o[t] = v;
  }
  const uint4* words = reinterpret_cast<const uint4*>(bits);
  size_t carry = HEADER_BYTES;                         // where the next unstuffed byte lands
  for (uint32_t s0 = 0; s0 < T; s0 += JP_SCAN * JP_STRIP) {
    const uint32_t first = s0 + (uint32_t)t * JP_STRIP;
    uint32_t w[4] = {0, 0, 0, 0};
    if (first < T) { const uint4 u = words[first / 16]; w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w; }
    const int nb = first < T ? (int)min((uint32_t)JP_STRIP, T - first) : 0;
    uint32_t ff = 0;
#pragma unroll
    for (int j = 0; j < JP_STRIP; ++j) ff += (j < nb && ((w[j >> 2] >> (24 - 8 * (j & 3))) & 255u) == 255u) ? 1u : 0u;
    uint32_t tot;
    const uint32_t before = block_exclusive_scan(ff, buf, &tot);
    size_t pos = carry + (first - s0) + before;
#pragma unroll
    for (int j = 0; j < JP_STRIP; ++j) {
      if (j < nb) {
        const uint32_t v = (w[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
        if (pos < cap) o[pos] = (uint8_t)v;
        ++pos;
        if (v == 255u) { if (pos < cap) o[pos] = 0; ++pos; }
      }
    }
    carry += (size_t)min((uint32_t)(JP_SCAN * JP_STRIP), T - s0) + tot;
  }
  if (t == 0) {
    const size_t len = carry + 2;
    if (len <= cap) { o[carry] = 0xFF; o[carry + 1] = 0xD9; *length = (int32_t)len; }
    else *length = len < (size_t)INT32_MAX ? -(int32_t)len : INT32_MIN;
  }
}

// out [n][cap], lengths [n]: jp_stuff_image per image; bitbuf [n][wcap]
__global__ __launch_bounds__(JP_SCAN) void jpeg_stuff_kernel(const uint32_t* __restrict__ bitbuf, uint32_t wcap, const uint32_t* __restrict__ nbytes,
                                                             const Tables* __restrict__ tab, uint8_t* __restrict__ out, size_t cap,
                                                             int32_t* __restrict__ lengths) {
  __shared__ uint32_t buf[JP_SCAN];
  const int im = blockIdx.x;
  jp_stuff_image(bitbuf + (size_t)im * wcap, wcap, nbytes[im], tab, 0, 0, out + (size_t)im * cap, cap, lengths + im, buf);
}

size_t jpeg_bound(int h, int w) { return encode_bound(h, w); }

// also used by kernels_face_thumb.hip, which patches the size fields of the header per image
const Tables* jpeg_tables(Ctx& c, int h, int w, int quality) {
  const auto key = std::make_tuple(h, w, quality);
  auto it = c.jpeg_cache.find(key);
  if (it != c.jpeg_cache.end()) return (const Tables*)it->second;
  Tables t;
  build_tables(h, w, quality, t);
  void* d = nullptr;
  FE_HIP(hipMalloc(&d, sizeof(Tables)));
  FE_HIP(hipMemcpy(d, &t, sizeof(Tables), hipMemcpyHostToDevice));
  c.jpeg_cache.emplace(key, d);
  return (const Tables*)d;
}

// words of an image's bit buffer: every block at its longest code, so the unstuffed scan always fits and an image that does not fit the
// caller's row can still be told how many bytes it needs
static uint32_t jpeg_bitbuf_words(const Geom& g) { return (uint32_t)((((size_t)g.nblk * ((BLOCK_MAX_BITS + 7) / 8) + 15) & ~(size_t)15) / 4); }

// bytes of arena the encode of one image takes besides its output row
size_t jpeg_scratch_bytes(int h, int w) {
  const Geom g = make_geom(h, w);
  return (size_t)g.nblk * (128 + 8) + (size_t)jpeg_bitbuf_words(g) * 4 + 1024;
}

// d_img [n][h][w][3] -> d_out [n][cap], d_lengths [n] (see jpeg_stuff_kernel); scratch from the arena, released on return (stream order)
void launch_jpeg_encode(Ctx& c, const uint8_t* d_img, int n, int h, int w, int bgr, int quality, uint8_t* d_out, size_t cap, int32_t* d_lengths) {
  FE_CHECK(n > 0 && h > 0 && w > 0 && h <= 65535 && w <= 65535, "jpeg: bad shape %d x %d x %d", n, h, w);
  FE_CHECK(quality >= 1 && quality <= 100, "jpeg: quality %d (1 .. 100)", quality);
  const Geom g = make_geom(h, w);
  FE_CHECK((double)g.nblk * BLOCK_MAX_BITS < 4.0e9 && (double)n * g.nblk < 2.0e9 * JP_THREADS, "jpeg: image too large");
  const Tables* tab = jpeg_tables(c, h, w, quality);
  const size_t mark = c.arena.mark();
  const size_t total = (size_t)n * g.nblk;
  const uint32_t wcap = jpeg_bitbuf_words(g);
  int16_t* coef = (int16_t*)c.arena.alloc(total * 128);
  uint32_t* bits = (uint32_t*)c.arena.alloc(total * 4);
  uint32_t* offs = (uint32_t*)c.arena.alloc(total * 4);
  uint32_t* nbytes = (uint32_t*)c.arena.alloc((size_t)n * 4);
  uint32_t* bitbuf = (uint32_t*)c.arena.alloc((size_t)n * wcap * 4);
  const unsigned blocks = (unsigned)((total + JP_THREADS - 1) / JP_THREADS);
  FE_HIP(hipMemsetAsync(bitbuf, 0, (size_t)n * wcap * 4, c.stream));
  hipLaunchKernelGGL(jpeg_coeff_kernel, dim3(blocks), dim3(JP_THREADS), 0, c.stream, d_img, n, g, bgr ? 1 : 0, tab, coef);
  hipLaunchKernelGGL(jpeg_bits_kernel, dim3(blocks), dim3(JP_THREADS), 0, c.stream, coef, n, g.nblk, tab, bits);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n), dim3(JP_SCAN), 0, c.stream, bits, g.nblk, offs, nbytes);
  hipLaunchKernelGGL(jpeg_write_kernel, dim3(blocks), dim3(JP_THREADS), 0, c.stream, coef, offs, n, g.nblk, tab, bitbuf, wcap);
  hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(n), dim3(JP_SCAN), 0, c.stream, bitbuf, wcap, nbytes, tab, d_out, cap, d_lengths);
  FE_HIP(hipGetLastError());
  c.arena.rewind(mark);
}

// ---- fe_thumbnail_jpeg_mixed: every stage from per-image descriptors, one launch per stage ------------------------------------------
// reduce and the two resampling passes: grid (sample chunks, image), the arithmetic of thumb_mixed_core.h; an image that skips a stage
// leaves its workgroups at once. The encoder passes above made ragged: coeff / bits / write take grid (block chunks, image) over the
// image's own Geom, scan / stuff stay one workgroup per image; every image has its slice of the coefficient, bit-length, offset and
// bit-buffer arrays (JpegItem), and the header's size fields are written per image (tables of (0, 0, quality)).
constexpr int TM_THREADS = 256;
constexpr unsigned TM_MAX_CHUNKS = 256;      // workgroups per image and stage; they stride over what is left

struct JpegItem {
  const uint8_t* pix;      // [h][w][3], what is encoded
  int32_t h, w;
  uint32_t wcap, pad;      // words of the image's bit buffer
  size_t blk0;             // its first block in the coefficient [.][64], bit-length and offset arrays
  size_t word0;            // its first word in the bit buffer (a multiple of 4)
};

__global__ __launch_bounds__(TM_THREADS) void thumb_reduce_mixed_kernel(const ThumbDesc* __restrict__ descs) {
  const ThumbDesc d = descs[blockIdx.y];
  if (!thumb_reduces(d)) return;
  const size_t total = (size_t)d.rh * d.rw;
  for (size_t i = (size_t)blockIdx.x * TM_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * TM_THREADS)
    thumb_reduce_sample(d, (int)(i / d.rw), (int)(i % d.rw), d.red + i * 3);
}

template <int P>
__global__ __launch_bounds__(TM_THREADS) void thumb_pass_mixed_kernel(const ThumbDesc* __restrict__ descs, const int32_t* __restrict__ pool) {
  const ThumbDesc d = descs[blockIdx.y];
  const ThumbPass p = d.pass[P];
  if (!p.ksize) return;
  const uint8_t* in = thumb_pass_in(d, P);
  uint8_t* out = thumb_pass_out(d, P);
  const size_t total = (size_t)p.oh * p.ow;
  for (size_t i = (size_t)blockIdx.x * TM_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * TM_THREADS)
    thumb_pass_sample(p, pool, in, (int)(i / p.ow), (int)(i % p.ow), out + i * 3);
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_coeff_ragged_kernel(const JpegItem* __restrict__ items, int bgr, const Tables* __restrict__ tab,
                                                                       int16_t* __restrict__ coef) {
  __shared__ uint16_t q[128];
  if (threadIdx.x < 128) q[threadIdx.x] = (&tab->q[0][0])[threadIdx.x];
  __syncthreads();
  const JpegItem it = items[blockIdx.y];
  const Geom g = make_geom(it.h, it.w);
  for (int b = blockIdx.x * JP_THREADS + threadIdx.x; b < g.nblk; b += gridDim.x * JP_THREADS)
    jp_coeff_block(it.pix, g, bgr, b, q, coef + (it.blk0 + b) * 64);
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_bits_ragged_kernel(const JpegItem* __restrict__ items, const int16_t* __restrict__ coef,
                                                                      const Tables* __restrict__ tab, uint32_t* __restrict__ bits) {
  __shared__ Huff H;
  load_huff(&H, tab);
  const JpegItem it = items[blockIdx.y];
  const int nblk = make_geom(it.h, it.w).nblk;
  const int16_t* base = coef + it.blk0 * 64;
  for (int b = blockIdx.x * JP_THREADS + threadIdx.x; b < nblk; b += gridDim.x * JP_THREADS) {
    CountSink s;
    encode_block(base + (size_t)b * 64, dc_pred(base, b), (b % 6) < 4 ? 0 : 1, H, s);
    bits[it.blk0 + b] = s.bits;
  }
}

__global__ __launch_bounds__(JP_SCAN) void jpeg_scan_ragged_kernel(const JpegItem* __restrict__ items, const uint32_t* __restrict__ bits,
                                                                   uint32_t* __restrict__ offs, uint32_t* __restrict__ nbytes) {
  __shared__ uint32_t buf[JP_SCAN];
  const JpegItem it = items[blockIdx.x];
  jp_scan_image(bits + it.blk0, make_geom(it.h, it.w).nblk, offs + it.blk0, nbytes + blockIdx.x, buf);
}

// bitbuf: every image's words, zeroed
__global__ __launch_bounds__(JP_THREADS) void jpeg_write_ragged_kernel(const JpegItem* __restrict__ items, const int16_t* __restrict__ coef,
                                                                       const uint32_t* __restrict__ offs, const Tables* __restrict__ tab,
                                                                       uint32_t* __restrict__ bitbuf) {
  __shared__ Huff H;
  load_huff(&H, tab);
  const JpegItem it = items[blockIdx.y];
  const int nblk = make_geom(it.h, it.w).nblk;
  for (int b = blockIdx.x * JP_THREADS + threadIdx.x; b < nblk; b += gridDim.x * JP_THREADS)
    jp_write_block(coef + it.blk0 * 64, b, nblk, offs[it.blk0 + b], H, bitbuf + it.word0, it.wcap);
}

__global__ __launch_bounds__(JP_SCAN) void jpeg_stuff_ragged_kernel(const JpegItem* __restrict__ items, const uint32_t* __restrict__ bitbuf,
                                                                    const uint32_t* __restrict__ nbytes, const Tables* __restrict__ tab,
                                                                    uint8_t* __restrict__ out, size_t cap, int32_t* __restrict__ lengths) {
  __shared__ uint32_t buf[JP_SCAN];
  const int im = blockIdx.x;
  const JpegItem it = items[im];
  jp_stuff_image(bitbuf + it.word0, it.wcap, nbytes[im], tab, it.h, it.w, out + (size_t)im * cap, cap, lengths + im, buf);
}

// rows [n][cap], lengths [n] as the stuff pass leaves them -> packed: the bytes of every row that fitted, back to back in row order.
// grid (byte chunks, row); every workgroup adds up the lengths in front of its row itself.
__global__ __launch_bounds__(TM_THREADS) void jpeg_gather_kernel(const uint8_t* __restrict__ rows, size_t cap, const int32_t* __restrict__ lengths,
                                                                 uint8_t* __restrict__ packed) {
  __shared__ unsigned long long part[TM_THREADS / 64];
  const int im = blockIdx.y;
  unsigned long long s = 0;
  for (int j = threadIdx.x; j < im; j += TM_THREADS) {
    const int32_t l = lengths[j];
    if (l > 0) s += (unsigned long long)l;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  size_t off = 0;
  for (int k = 0; k < TM_THREADS / 64; ++k) off += (size_t)part[k];
  const int32_t len = lengths[im];
  if (len <= 0 || (size_t)len > cap) return;
  const uint8_t* src = rows + (size_t)im * cap;
  for (size_t i = (size_t)blockIdx.x * TM_THREADS + threadIdx.x; i < (size_t)len; i += (size_t)gridDim.x * TM_THREADS) packed[off + i] = src[i];
}

// thumb_mixed_scratch_bytes (thumb_mixed_core.h) counts what thumbnails_mixed_launch carves from the arena per image
static_assert(sizeof(JpegItem) == kThumbItemBytes && (BLOCK_MAX_BITS + 7) / 8 == kThumbBlockCodeBytes, "thumb_mixed_core.h restates both");

// One chunk of fe_thumbnail_jpeg_mixed. descs [n]: host descriptors whose src is device memory; their three buffers are carved from the
// arena here, with everything else the stages need (the caller rewinds). host_blob: the descriptors as uploaded - the caller keeps it
// until the stream is synchronised. d_pool: the call's tables. d_out [n][cap] / d_lengths [n]: as launch_jpeg_encode leaves them.
void thumbnails_mixed_launch(Ctx& c, ThumbDesc* descs, int n, const int32_t* d_pool, int bgr, int quality, std::vector<uint8_t>& host_blob,
                             uint8_t* d_out, size_t cap, int32_t* d_lengths) {
  FE_CHECK(n > 0 && n <= 32768, "thumbnail_jpeg_mixed: %d images in a chunk (1 .. 32768)", n);
  FE_CHECK(quality >= 1 && quality <= 100, "jpeg: quality %d (1 .. 100)", quality);
  const Tables* tab = jpeg_tables(c, 0, 0, quality);
  std::vector<JpegItem> items(n);
  size_t blocks = 0, words = 0, max_red = 0, max_pass[2] = {0, 0};
  int max_nblk = 0;
  bool any_red = false, any_pass[2] = {false, false};
  for (int i = 0; i < n; ++i) {
    ThumbDesc& d = descs[i];
    const size_t rb = ThumbTables::red_bytes(d), mb = ThumbTables::mid_bytes(d), pb = ThumbTables::pix_bytes(d);
    d.red = rb ? (uint8_t*)c.arena.alloc(rb) : nullptr;
    d.mid = mb ? (uint8_t*)c.arena.alloc(mb) : nullptr;
    d.pix = pb ? (uint8_t*)c.arena.alloc(pb) : nullptr;
    if (rb) { any_red = true; max_red = std::max(max_red, (size_t)d.rh * d.rw); }
    for (int p = 0; p < 2; ++p)
      if (d.pass[p].ksize) { any_pass[p] = true; max_pass[p] = std::max(max_pass[p], (size_t)d.pass[p].oh * d.pass[p].ow); }
    const Geom g = make_geom(d.oh, d.ow);
    FE_CHECK((double)g.nblk * BLOCK_MAX_BITS < 4.0e9, "jpeg: image %d too large", i);
    JpegItem& it = items[i];
    it.pix = thumb_pixels(d); it.h = d.oh; it.w = d.ow; it.wcap = jpeg_bitbuf_words(g); it.pad = 0; it.blk0 = blocks; it.word0 = words;
    blocks += (size_t)g.nblk; words += it.wcap;
    max_nblk = std::max(max_nblk, g.nblk);
  }
  const size_t desc_b = mixed_list::align_up((size_t)n * sizeof(ThumbDesc));
  host_blob.resize(desc_b + (size_t)n * sizeof(JpegItem));
  memcpy(host_blob.data(), descs, (size_t)n * sizeof(ThumbDesc));
  memcpy(host_blob.data() + desc_b, items.data(), (size_t)n * sizeof(JpegItem));
  uint8_t* d_blob = (uint8_t*)c.arena.alloc(host_blob.size());
  const ThumbDesc* d_descs = (const ThumbDesc*)d_blob;
  const JpegItem* d_items = (const JpegItem*)(d_blob + desc_b);
  int16_t* coef = (int16_t*)c.arena.alloc(blocks * 128);
  uint32_t* bits = (uint32_t*)c.arena.alloc(blocks * 4);
  uint32_t* offs = (uint32_t*)c.arena.alloc(blocks * 4);
  uint32_t* nbytes = (uint32_t*)c.arena.alloc((size_t)n * 4);
  uint32_t* bitbuf = (uint32_t*)c.arena.alloc(words * 4);
  FE_HIP(hipMemcpyAsync(d_blob, host_blob.data(), host_blob.size(), hipMemcpyHostToDevice, c.stream));
  FE_HIP(hipMemsetAsync(bitbuf, 0, words * 4, c.stream));
  auto chunks = [](size_t work, int per) { return (unsigned)std::min<size_t>(std::max<size_t>((work + per - 1) / per, 1), TM_MAX_CHUNKS); };
  if (any_red) hipLaunchKernelGGL(thumb_reduce_mixed_kernel, dim3(chunks(max_red, TM_THREADS), n), dim3(TM_THREADS), 0, c.stream, d_descs);
  if (any_pass[0])
    hipLaunchKernelGGL(thumb_pass_mixed_kernel<0>, dim3(chunks(max_pass[0], TM_THREADS), n), dim3(TM_THREADS), 0, c.stream, d_descs, d_pool);
  if (any_pass[1])
    hipLaunchKernelGGL(thumb_pass_mixed_kernel<1>, dim3(chunks(max_pass[1], TM_THREADS), n), dim3(TM_THREADS), 0, c.stream, d_descs, d_pool);
  FE_HIP(hipGetLastError());
  const dim3 eg(chunks((size_t)max_nblk, JP_THREADS), n);
  hipLaunchKernelGGL(jpeg_coeff_ragged_kernel, eg, dim3(JP_THREADS), 0, c.stream, d_items, bgr ? 1 : 0, tab, coef);
  hipLaunchKernelGGL(jpeg_bits_ragged_kernel, eg, dim3(JP_THREADS), 0, c.stream, d_items, coef, tab, bits);
  hipLaunchKernelGGL(jpeg_scan_ragged_kernel, dim3(n), dim3(JP_SCAN), 0, c.stream, d_items, bits, offs, nbytes);
  hipLaunchKernelGGL(jpeg_write_ragged_kernel, eg, dim3(JP_THREADS), 0, c.stream, d_items, coef, offs, tab, bitbuf);
  hipLaunchKernelGGL(jpeg_stuff_ragged_kernel, dim3(n), dim3(JP_SCAN), 0, c.stream, d_items, bitbuf, nbytes, tab, d_out, cap, d_lengths);
  FE_HIP(hipGetLastError());
}

// rows [n][cap] / lengths [n] on the device -> d_packed (see jpeg_gather_kernel); max_len: the longest row that fitted
void jpeg_gather(Ctx& c, const uint8_t* d_rows, size_t cap, const int32_t* d_lengths, int n, size_t max_len, uint8_t* d_packed) {
  const unsigned gx = (unsigned)std::min<size_t>(std::max<size_t>((max_len + TM_THREADS * 16 - 1) / (TM_THREADS * 16), 1), 64);
  hipLaunchKernelGGL(jpeg_gather_kernel, dim3(gx, n), dim3(TM_THREADS), 0, c.stream, d_rows, cap, d_lengths, d_packed);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
