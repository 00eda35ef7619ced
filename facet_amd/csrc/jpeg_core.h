// Baseline JPEG arithmetic shared by the kernels of kernels_jpeg.hip and by host code: libjpeg's colour conversion, h2v2 downsample,
// integer slow DCT (jfdctint), quantiser and Huffman coder, restated per 8x8 block. Integer end to end, so the same functions give
// the same coefficients and bits on the device and on the host.
//
// Layout of a scan (YCbCr 4:2:0, one interleaved scan): MCU m = (my, mx) covers 16x16 pixels and holds the blocks Y0 Y1 / Y2 Y3, Cb, Cr
// in that order; block b of an image is (m, k) = (b / 6, b % 6). A luma block outside the component's own block grid
// (ceil(w/8) x ceil(h/8); the MCU grid can be one block wider / taller) is one of libjpeg's dummy blocks: all AC zero, DC copied from
// the block before it in the MCU (jccoefct.c compress_data).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define FE_JHD __host__ __device__ __forceinline__
#else
#define FE_JHD inline
#endif

namespace fe {
namespace jpeg {

constexpr int HEADER_BYTES = 623;        // SOI, APP0, 2 x DQT, SOF0, 4 x DHT, SOS
constexpr int BLOCK_MAX_BITS = 1658;     // 20 bits of DC + 63 x 26 bits of AC

struct Huff {                            // code / length by symbol, table 0 = luma, 1 = chroma
  uint16_t dc_code[2][12];
  uint16_t ac_code[2][256];
  uint8_t dc_len[2][12];
  uint8_t ac_len[2][256];
};

struct Tables {                          // one device block per (h, w, quality)
  uint8_t header[640];                   // HEADER_BYTES used
  uint16_t q[2][64];                     // quantiser steps, natural order, luma / chroma
  Huff huff;
};

struct Geom {
  int h, w;                              // pixels
  int mw, mh;                            // MCUs per row / column
  int wb, hb;                            // luma blocks per row / column that are real
  int ch2;                               // chroma rows that are real: ceil(h / 2)
  int nblk;                              // 6 * mw * mh
};

FE_JHD Geom make_geom(int h, int w) {
  Geom g;
  g.h = h; g.w = w;
  g.mw = (w + 15) / 16; g.mh = (h + 15) / 16;
  g.wb = (w + 7) / 8; g.hb = (h + 7) / 8;
  g.ch2 = (h + 1) / 2;
  g.nblk = 6 * g.mw * g.mh;
  return g;
}

// zigzag position -> natural (row-major) position
#define FE_JPEG_NATURAL_ORDER                                                                                                   \
  {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,  \
   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

FE_JHD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c's 1-D pass over d[0], d[s], ... d[7s]. first: the row pass (results scaled up by PASS1_BITS), else the column pass.
template <bool first>
FE_JHD void fdct_1d(int* d, const int s) {
  constexpr int CONST_BITS = 13, PASS1_BITS = 2;
  const int tmp0 = d[0] + d[7 * s], tmp7 = d[0] - d[7 * s];
  const int tmp1 = d[s] + d[6 * s], tmp6 = d[s] - d[6 * s];
  const int tmp2 = d[2 * s] + d[5 * s], tmp5 = d[2 * s] - d[5 * s];
  const int tmp3 = d[3 * s] + d[4 * s], tmp4 = d[3 * s] - d[4 * s];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int n = first ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
  if (first) {
    d[0] = (tmp10 + tmp11) << PASS1_BITS;
    d[4 * s] = (tmp10 - tmp11) << PASS1_BITS;
  } else {
    d[0] = descale(tmp10 + tmp11, PASS1_BITS);
    d[4 * s] = descale(tmp10 - tmp11, PASS1_BITS);
  }
  int z1 = (tmp12 + tmp13) * 4433;
  d[2 * s] = descale(z1 + tmp13 * 6270, n);
  d[6 * s] = descale(z1 + tmp12 * (-15137), n);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  d[7 * s] = descale(t4 + z1 + z3, n);
  d[5 * s] = descale(t5 + z2 + z4, n);
  d[3 * s] = descale(t6 + z2 + z3, n);
  d[s] = descale(t7 + z1 + z4, n);
}

// Block k of MCU (my, mx) of one image [h][w][3] -> 64 quantised coefficients in zigzag order.
FE_JHD void block_coeffs(const uint8_t* img, const Geom& g, int bgr, int my, int mx, int k, const uint16_t* q /* [2][64] */, int16_t* out) {
  int d[64];
  const int ir = bgr ? 2 : 0, ib = bgr ? 0 : 2;
  bool dummy = false;
  if (k < 4) {
    int bx = 2 * mx + (k & 1), by = 2 * my + (k >> 1);
    if (by >= g.hb) { by -= 1; bx = 2 * mx + 1; dummy = true; }      // bottom dummy row: DC of Y1 ...
    if (bx >= g.wb) { bx -= 1; dummy = true; }                       // ... which is Y0's when Y1 is a dummy itself
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int y = by * 8 + r < g.h ? by * 8 + r : g.h - 1;
      const uint8_t* row = img + (size_t)y * g.w * 3;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int x = bx * 8 + c < g.w ? bx * 8 + c : g.w - 1;
        const uint8_t* p = row + x * 3;
        d[r * 8 + c] = ((19595 * p[ir] + 38470 * p[1] + 7471 * p[ib] + 32768) >> 16) - 128;
      }
    }
  } else {
    // Cb: -0.16874 R - 0.33126 G + 0.5 B, Cr: 0.5 R - 0.41869 G - 0.08131 B, both + 128.0 + (0.5 - 1 ulp) in 16.16
    const int cr = k == 5;
    const int fr = cr ? 32768 : -11059, fg = cr ? -27439 : -21709, fb = cr ? -5329 : 32768;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int cy = my * 8 + r < g.ch2 ? my * 8 + r : g.ch2 - 1;      // rows past the component replicate the downsampled row
      const int y0 = 2 * cy, y1 = 2 * cy + 1 < g.h ? 2 * cy + 1 : g.h - 1;
      const uint8_t* r0 = img + (size_t)y0 * g.w * 3;
      const uint8_t* r1 = img + (size_t)y1 * g.w * 3;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int cx = mx * 8 + c;
        const int x0 = 2 * cx < g.w ? 2 * cx : g.w - 1, x1 = 2 * cx + 1 < g.w ? 2 * cx + 1 : g.w - 1;   // columns replicate the pixel
        int s = (c & 1) ? 2 : 1;
        const uint8_t* pp[4] = {r0 + x0 * 3, r0 + x1 * 3, r1 + x0 * 3, r1 + x1 * 3};
#pragma unroll
        for (int t = 0; t < 4; ++t) s += (fr * pp[t][ir] + fg * pp[t][1] + fb * pp[t][ib] + (128 << 16) + 32767) >> 16;
        d[r * 8 + c] = (s >> 2) - 128;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct_1d<true>(d + r * 8, 1);
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct_1d<false>(d + c, 8);
  const uint16_t* qt = q + (k < 4 ? 0 : 64);
  constexpr int nat[64] = FE_JPEG_NATURAL_ORDER;
#pragma unroll
  for (int z = 0; z < 64; ++z) {
    const int v = d[nat[z]];
    const int qv = (int)qt[nat[z]] << 3;            // the DCT output carries a factor 8
    const int a = ((v < 0 ? -v : v) + (qv >> 1)) / qv;
    out[z] = (int16_t)((dummy && z) ? 0 : (v < 0 ? -a : a));
  }
}

FE_JHD int bit_length(int v) { return v ? 32 - __builtin_clz((unsigned)v) : 0; }

// DC predictor of block b: the previous block of the same component in scan order, 0 at the start of the scan.
// coef: the image's [nblk][64] zigzag coefficients.
FE_JHD int dc_pred(const int16_t* coef, int b) {
  const int k = b % 6;
  int p;
  if (k == 0) p = b - 3;          // Y3 of the MCU before
  else if (k < 4) p = b - 1;
  else p = b - 6;
  return p < 0 ? 0 : coef[(size_t)p * 64];
}

// jchuff.c encode_one_block: sink.put(code, length) receives every code and every value field in order.
template <class Sink>
FE_JHD void encode_block(const int16_t* zz, int pred, int tbl, const Huff& H, Sink& sink) {
  int t = zz[0] - pred, t2 = t;
  if (t < 0) { t = -t; t2--; }
  int nb = bit_length(t);
  sink.put(H.dc_code[tbl][nb], H.dc_len[tbl][nb]);
  if (nb) sink.put((unsigned)t2 & ((1u << nb) - 1), nb);
  int r = 0;
  for (int k = 1; k < 64; ++k) {
    t = zz[k];
    if (t == 0) { ++r; continue; }
    while (r > 15) { sink.put(H.ac_code[tbl][0xF0], H.ac_len[tbl][0xF0]); r -= 16; }
    t2 = t;
    if (t < 0) { t = -t; t2--; }
    nb = bit_length(t);
    const int sym = (r << 4) + nb;
    sink.put(H.ac_code[tbl][sym], H.ac_len[tbl][sym]);
    sink.put((unsigned)t2 & ((1u << nb) - 1), nb);
    r = 0;
  }
  if (r > 0) sink.put(H.ac_code[tbl][0], H.ac_len[tbl][0]);
}

struct CountSink {
  uint32_t bits = 0;
  FE_JHD void put(unsigned, int len) { bits += (uint32_t)len; }
};


// ---- host: the tables and the 623 header bytes libjpeg writes for (h, w, quality) ---------------------------------------------
// ITU T.81 Annex K: the example quantisation tables (natural order) and the typical Huffman tables (bits per length, values)
static const uint8_t kStdLumaQ[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kStdChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
static const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t kAcVals[2][162] = {
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23,
     24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
     168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
     227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225,
     37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104,
     105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165,
     166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
     226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// canonical codes of a (bits, values) table, by symbol (jchuff.c jpeg_make_c_derived_tbl)
inline void derive_codes(const uint8_t* bits, const uint8_t* vals, uint16_t* code_of, uint8_t* len_of) {
  unsigned code = 0;
  int p = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++p) { code_of[vals[p]] = (uint16_t)code++; len_of[vals[p]] = (uint8_t)l; }
    code <<= 1;
  }
}

// jpeg_set_quality(quality, force_baseline = TRUE) + the markers of jpeg_start_compress for 8-bit YCbCr 4:2:0, JFIF 1.01, density 1x1
inline void build_tables(int h, int w, int quality, Tables& t) {
  t = Tables();
  int q = quality <= 0 ? 1 : (quality > 100 ? 100 : quality);
  const int scale = q < 50 ? 5000 / q : 200 - q * 2;
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 64; ++i) {
      long v = ((long)(c ? kStdChromaQ : kStdLumaQ)[i] * scale + 50L) / 100L;
      t.q[c][i] = (uint16_t)(v <= 0 ? 1 : (v > 255 ? 255 : v));
    }
  for (int c = 0; c < 2; ++c) {
    derive_codes(kDcBits[c], kDcVals, t.huff.dc_code[c], t.huff.dc_len[c]);
    derive_codes(kAcBits[c], kAcVals[c], t.huff.ac_code[c], t.huff.ac_len[c]);
  }
  const int nat[64] = FE_JPEG_NATURAL_ORDER;
  uint8_t* p = t.header;
  auto put = [&p](int v) { *p++ = (uint8_t)v; };
  auto put2 = [&put](int v) { put(v >> 8); put(v & 255); };
  put2(0xFFD8);
  put2(0xFFE0); put2(16); put('J'); put('F'); put('I'); put('F'); put(0); put(1); put(1); put(0); put2(1); put2(1); put(0); put(0);
  for (int c = 0; c < 2; ++c) {
    put2(0xFFDB); put2(67); put(c);
    for (int z = 0; z < 64; ++z) put(t.q[c][nat[z]]);
  }
  put2(0xFFC0); put2(17); put(8); put2(h); put2(w); put(3);
  put(1); put(0x22); put(0); put(2); put(0x11); put(1); put(3); put(0x11); put(1);
  for (int c = 0; c < 2; ++c) {
    put2(0xFFC4); put2(19 + 12); put(c);
    for (int i = 0; i < 16; ++i) put(kDcBits[c][i]);
    for (int i = 0; i < 12; ++i) put(kDcVals[i]);
    put2(0xFFC4); put2(19 + 162); put(0x10 | c);
    for (int i = 0; i < 16; ++i) put(kAcBits[c][i]);
    for (int i = 0; i < 162; ++i) put(kAcVals[c][i]);
  }
  put2(0xFFDA); put2(12); put(3); put(1); put(0x00); put(2); put(0x11); put(3); put(0x11); put(0); put(63); put(0);
}

// bytes no encode of an h x w image can exceed: every block at its longest, every byte stuffed, header, EOI
inline size_t encode_bound(int h, int w) {
  const Geom g = make_geom(h, w);
  return (size_t)g.nblk * ((BLOCK_MAX_BITS + 7) / 8) * 2 + HEADER_BYTES + 2;
}

}  // namespace jpeg
}  // namespace fe
