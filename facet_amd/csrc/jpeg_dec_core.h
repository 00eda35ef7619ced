// JPEG decoding arithmetic shared by the kernels of kernels_jpeg_dec.hip and by host code: the inverse of jpeg_core.h.
// libjpeg's Huffman decoders (jdhuff.c; jdphuff.c for the scans of a progressive file), dequantiser + integer slow IDCT (jidctint.c), fancy upsampling (jdsample.c) and YCbCr -> RGB
// (jdcolor.c), restated per segment / block / pixel. Integer end to end, so the same functions give the same pixels on the device and on
// the host, and those are the pixels of Pillow's `Image.open(f).convert('RGB')`.
//
// Layout of a decode: an image's entropy data is cut at its restart markers into segments (one when it has none); a segment decodes
// serially into int16 coefficient blocks in natural order, stored per component in that component's block grid padded to whole MCUs
// (DecGeom); every block is dequantised and transformed into its component's plane; a pixel takes its luma sample, its two chroma samples
// through the triangle filters and the colour conversion, and lands at the address its EXIF orientation gives it.
// A progressive file is a sequence of scans over that same coefficient buffer, each cut into segments of its own; once the last scan has
// run the buffer holds what a baseline file's single scan would have left, and everything behind the entropy stage is shared.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "jpeg_core.h"

namespace fe {
namespace jpegdec {

// status of an image: 0 decoded, > 0 a kind of file this decoder leaves to the caller, < 0 a corrupt stream (FE_JPEG_* of facet_engine.h)
enum Status : int32_t {
  ST_OK = 0,
  ST_PROGRESSIVE = 1,      // SOF2
  ST_ARITHMETIC = 2,       // SOF9 .. SOF15, DAC
  ST_PRECISION = 3,        // 12-bit (or any precision but 8)
  ST_COMPONENTS = 4,       // 4 components (CMYK / YCCK), 2 components
  ST_ADOBE_RGB = 5,        // 3 components stored as RGB (Adobe transform 0, or component ids 'R' 'G' 'B')
  ST_SAMPLING = 6,         // sampling factors other than luma 1x1 / 2x1 / 2x2 with chroma 1x1
  ST_MULTISCAN = 7,        // more than one scan
  ST_OTHER = 8,            // lossless / hierarchical frames, DNL, scan components out of frame order, EXIF blocks only Pillow should judge
  ST_BAD_MARKER = -1,
  ST_BAD_HUFFMAN = -2,
  ST_PREMATURE_END = -3,
  ST_BAD_RESTART = -4,
  ST_BAD_DIMENSIONS = -5,
  ST_BAD_COEFFICIENT = -6,   // samples so far out of range that libjpeg's own IDCT variants (C, SIMD) stop agreeing with each other
};

constexpr int LOOK_BITS = 9;

struct HuffDec {                       // jdhuff.c d_derived_tbl
  uint16_t look[1 << LOOK_BITS];       // next LOOK_BITS bits -> length << 8 | symbol; 0: the code is longer
  int32_t maxcode[17];                 // [l]: largest code of length l, -1 when there is none
  int32_t valoff[17];                  // [l]: index into vals of the first code of length l, minus that code
  uint8_t vals[256];
};

struct DecTables {                     // one per image
  uint16_t q[4][64];                   // natural order
  HuffDec huff[8];                     // 0 .. 3 DC, 4 .. 7 AC
};

struct DecGeom {
  int w, h, ncomp, hs, vs;             // hs, vs: luma sampling (1 for grayscale)
  int mw, mh;                          // MCUs per row / column
  int bw[3], bh[3];                    // blocks per row / column of each component's padded grid
  uint32_t blk_off[3];                 // first block of each component in the image's coefficient buffer
  uint32_t plane_off[3];               // first byte of each component in the image's plane buffer; a plane is [bh * 8][bw * 8]
  uint32_t nblk, plane_bytes;
  int cw, ch;                          // real extent of a chroma plane: ceil(w / hs), ceil(h / vs)
};

FE_JHD DecGeom make_dec_geom(int w, int h, int ncomp, int hs, int vs) {
  DecGeom g;
  g.w = w; g.h = h; g.ncomp = ncomp; g.hs = hs; g.vs = vs;
  g.mw = (w + 8 * hs - 1) / (8 * hs); g.mh = (h + 8 * vs - 1) / (8 * vs);
  uint32_t b = 0, p = 0;
  for (int c = 0; c < 3; ++c) {
    const bool on = c < ncomp;
    g.bw[c] = on ? g.mw * (c ? 1 : hs) : 0; g.bh[c] = on ? g.mh * (c ? 1 : vs) : 0;
    g.blk_off[c] = b; g.plane_off[c] = p;
    b += (uint32_t)g.bw[c] * g.bh[c]; p += (uint32_t)g.bw[c] * g.bh[c] * 64;
  }
  g.nblk = b; g.plane_bytes = p;
  g.cw = (w + hs - 1) / hs; g.ch = (h + vs - 1) / vs;
  return g;
}

// ---- bit reader over one segment ---------------------------------------------------------------------------------------------------
// The bytes of all files of a call sit in one buffer whose start is 16-byte aligned and whose size is a multiple of 16, so the aligned
// 16-byte chunk around any byte of a segment is inside it. A segment holds entropy-coded bytes only (the host cut it at the markers), so
// a 0xFF in it is followed by its stuffed 0x00, which is skipped. Past the segment's end the reader supplies zero bits, as libjpeg's
// jpeg_fill_bit_buffer does, and counts them: a decoder that consumed any has run past the end of its data.
struct Chunk16 { uint32_t w[4]; };

FE_JHD Chunk16 load16(const uint8_t* p) {
  Chunk16 c;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  c.w[0] = u.x; c.w[1] = u.y; c.w[2] = u.z; c.w[3] = u.w;
#else
  memcpy(c.w, p, 16);
#endif
  return c;
}

struct BitReader {
  const uint8_t* base;
  uint32_t pos, end, chunk;
  Chunk16 cur;
  uint64_t acc;
  int nbits, pad;
  FE_JHD void init(const uint8_t* b, uint32_t start, uint32_t stop) {
    base = b; pos = start; end = stop; chunk = 0xFFFFFFFFu; acc = 0; nbits = 0; pad = 0;
    cur.w[0] = cur.w[1] = cur.w[2] = cur.w[3] = 0;
  }
  FE_JHD uint32_t byte_at(uint32_t p) {
    if ((p >> 4) != chunk) { chunk = p >> 4; cur = load16(base + ((size_t)chunk << 4)); }
    const uint32_t j = p & 15u;
    const uint32_t word = j < 8 ? (j < 4 ? cur.w[0] : cur.w[1]) : (j < 12 ? cur.w[2] : cur.w[3]);
    return (word >> (8 * (j & 3u))) & 255u;
  }
  FE_JHD void fill() {                           // at least 57 bits afterwards
    while (nbits <= 56) {
      uint32_t b = 0;
      if (pos < end) {
        b = byte_at(pos++);
        if (b == 255u) ++pos;                    // the stuffed zero
      } else {
        pad += 8;
      }
      acc = (acc << 8) | b;
      nbits += 8;
    }
  }
  FE_JHD uint32_t peek(int n) const { return (uint32_t)(acc >> (nbits - n)) & ((1u << n) - 1u); }      // 1 <= n <= 16 <= nbits
  FE_JHD void skip(int n) { nbits -= n; }
  FE_JHD bool overread() const { return pad > nbits; }
};

// one Huffman symbol; < 0: no code matches (jdhuff.c jpeg_huff_decode's "corrupt JPEG data: bad Huffman code")
FE_JHD int decode_symbol(BitReader& br, const HuffDec& t) {
  const uint32_t v = br.peek(16);
  const uint32_t e = t.look[v >> (16 - LOOK_BITS)];
  if (e) { br.skip((int)(e >> 8)); return (int)(e & 255u); }
  for (int l = LOOK_BITS + 1; l <= 16; ++l) {
    const int32_t c = (int32_t)(v >> (16 - l));
    if (c <= t.maxcode[l]) { br.skip(l); return t.vals[(c + t.valoff[l]) & 255]; }
  }
  return -1;
}

FE_JHD int huff_extend(int r, int s) { return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r; }

// jdhuff.c decode_mcu for one block: blk (64 coefficients, natural order, zero on entry) receives the DC value and the non-zero AC values.
// nat: the zigzag -> natural table. Returns 0 or ST_BAD_HUFFMAN.
FE_JHD int decode_block(BitReader& br, const HuffDec& dc, const HuffDec& ac, int& pred, int16_t* blk, const uint8_t* nat) {
  br.fill();
  int s = decode_symbol(br, dc);
  if (s < 0 || s > 15) return ST_BAD_HUFFMAN;
  if (s) {
    const int r = (int)br.peek(s);
    br.skip(s);
    s = huff_extend(r, s);
  }
  pred = (int32_t)((uint32_t)pred + (uint32_t)s);
  blk[0] = (int16_t)pred;
  for (int k = 1; k < 64; ++k) {
    br.fill();
    s = decode_symbol(br, ac);
    if (s < 0) return ST_BAD_HUFFMAN;
    const int r = s >> 4;
    s &= 15;
    if (s) {
      k += r;
      const int v = (int)br.peek(s);
      br.skip(s);
      if (k >= 64) return ST_BAD_HUFFMAN;          // a run past the block: libjpeg would store it at 63, no encoder writes it
      blk[nat[k]] = (int16_t)huff_extend(v, s);
    } else {
      if (r != 15) break;                          // EOB
      k += 15;
    }
  }
  return 0;
}

// MCUs mcu0 .. mcu0 + nmcu - 1 of an image from one segment. huff: the image's 8 tables; td / ta: DC / AC table of each component;
// coef: the image's coefficient buffer. DC prediction starts at 0: a segment begins at the scan's start or behind a restart marker.
FE_JHD int decode_segment(BitReader& br, const DecGeom& g, const HuffDec* huff, const uint8_t* td, const uint8_t* ta, uint32_t mcu0, uint32_t nmcu,
                          int16_t* coef, const uint8_t* nat) {
  int pred[3] = {0, 0, 0};
  int my = (int)(mcu0 / (uint32_t)g.mw), mx = (int)(mcu0 % (uint32_t)g.mw);
  for (uint32_t m = 0; m < nmcu && my < g.mh; ++m) {
    for (int c = 0; c < g.ncomp; ++c) {
      const int ch = c ? 1 : g.hs, cv = c ? 1 : g.vs;
      for (int by = 0; by < cv; ++by)
        for (int bx = 0; bx < ch; ++bx) {
          const uint32_t b = g.blk_off[c] + (uint32_t)(my * cv + by) * g.bw[c] + (uint32_t)(mx * ch + bx);
          const int rc = decode_block(br, huff[td[c] & 3], huff[4 + (ta[c] & 3)], pred[c], coef + (size_t)b * 64, nat);
          if (rc) return rc;
        }
    }
    if (br.overread()) return ST_PREMATURE_END;
    if (++mx == g.mw) { mx = 0; ++my; }
  }
  return 0;
}

// ---- decoding inside one segment in parallel: self-synchronising Huffman decoding ------------------------------------------------------
// (Weissenberger & Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018.) A baseline segment is cut into subsequences of S raw
// bytes, S a power of two >= 16; a cut that lands on the stuffed 0x00 behind a 0xFF moves one byte on, which is exact because inside a
// segment a 0xFF is always followed by its stuffed zero and is never one itself. A lane decodes the symbols (a Huffman code with its
// extra bits) that START inside its subsequence, from an entry state: where in the MCU and in the block the decoder is, and at which bit.
//   step 1  every subsequence but the last is decoded from its first bit as if a block of component 0 began there; subsequence 0 really
//           does. Nothing is stored but the exit: the state at the first symbol that starts at or behind the next subsequence's first byte.
//   step 2  rounds: subsequence i is decoded again from the exit of i - 1 as the previous round left it, unless that is the entry it was last
//           decoded from. After round r the exits of 0 .. r are the true ones, by induction from subsequence 0, so at most as many rounds
//           as subsequences are run and what stands then is right: there is nothing to fall back from. A round that changes nothing ends it.
//   step 3  exclusive prefix sums over the blocks each subsequence completed and over the DC differences it decoded per component give
//           every subsequence the index of its first block in scan order and its entry predictions.
//   step 4  every subsequence decodes from its true entry and stores coefficients: a block that straddles a cut is written by two lanes,
//           to different int16 elements.
// Positions are kept in raw-byte terms: an exit is the number of (destuffed) bits behind the first byte of the next subsequence, which
// is a raw offset fixed by the cut, so two passes that stop at the same bit state the same number whatever their readers prefetched.
// A code in no table or a run past 63 in steps 1 and 2 is what a wrong guess looks like, not an error: the pass drops one bit, or ends
// the block at 63, and goes on, because any rule that is a function of the bits keeps the induction and this one lets a lane that guessed
// the component wrong find its way into step with the true decoder inside its own subsequence (giving up instead left a three-component
// file without restart markers one round per subsequence). Step 4 starts from true states, so there the same conditions are
// decode_segment's errors; the caller then zeroes the image and decodes it again with decode_segment for its exact status.
// SUB_INVALID is the exit of a pass that has not run; no pass starts from it.
// The exit of the last subsequence has no reader, so steps 1 and 2 leave it out.
constexpr uint32_t SUB_INVALID = 0xFFFFFFFFu;
constexpr uint32_t SUB_BYTES = 128;    // the device's S
// The most bits an exit can lie behind its cut: the longest symbol is a 16-bit code with 15 extra bits, and the symbol that crosses the cut
// began at least one bit in front of it. (The one-bit drop of a speculative pass is shorter.)
constexpr uint32_t SUB_MAX_PAST = 16 + 15 - 1;

FE_JHD uint32_t sub_count(uint32_t seg_bytes, uint32_t S) { return (seg_bytes + S - 1) / S; }

// raw offset of subsequence i's first byte; i * S is inside the segment [s0, s1)
FE_JHD uint32_t sub_start(const uint8_t* bytes, uint32_t s0, uint32_t i, uint32_t S) {
  const uint32_t c = s0 + i * S;
  return (i && bytes[c] == 0 && bytes[c - 1] == 255) ? c + 1 : c;
}

// BitReader that knows where the bit it hands out next lies relative to raw offset `limit`, a data byte or the segment's end
struct SubReader : BitReader {
  uint32_t limit, loaded, mark;        // loaded: bits taken into acc so far; mark: `loaded` when the byte at `limit` came in
  FE_JHD void start(const uint8_t* b, uint32_t from, uint32_t stop, uint32_t lim) {
    init(b, from, stop);
    limit = lim; loaded = 0; mark = SUB_INVALID;
  }
  FE_JHD void fill_marked() {          // BitReader::fill
    while (nbits <= 56) {
      uint32_t b = 0;
      if (pos >= limit && mark == SUB_INVALID) mark = loaded;
      if (pos < end) {
        b = byte_at(pos++);
        if (b == 255u) ++pos;
      } else {
        pad += 8;
      }
      acc = (acc << 8) | b;
      nbits += 8;
      loaded += 8;
    }
  }
  FE_JHD bool behind() const { return mark != SUB_INVALID && loaded - (uint32_t)nbits >= mark; }      // after fill_marked()
  FE_JHD uint32_t past() const { return loaded - (uint32_t)nbits - mark; }
};

// entry / exit state: bits behind the subsequence's first byte << 16 | block within the MCU << 8 | zigzag index (0: a DC code is next)
FE_JHD uint32_t sub_state(uint32_t bits, int b, int k) { return (bits << 16) | ((uint32_t)b << 8) | (uint32_t)k; }

struct SubResult {
  uint32_t exit;                       // SUB_INVALID: the pass did not reach its limit (step 4: ended with its blocks or an error)
  uint32_t nblk;                       // blocks whose last symbol it decoded
  int32_t dc[3];                       // sums of the DC differences it decoded, wrapping as decode_block's pred does
  int32_t err;                         // WRITE: 0, ST_BAD_HUFFMAN or ST_PREMATURE_END
};

// One pass over subsequence i of nsub of the segment [s0, s1) from `entry`. WRITE = false: steps 1 and 2. WRITE = true: step 4, which
// stores into coef (the image's buffer, zero on entry) for blocks first_blk .. of the segment's nmcu MCUs from mcu0 on, with predictions
// pred_in, stops at the segment's last block and, in the last subsequence, has no other end: it then runs until the MCU in which the
// data ran out. Every loop is bounded: a symbol takes at least one bit, so a pass with a limit sees at most 8 S + 32 of them, and the
// one without ends with its blocks or with the first MCU that consumed padding.
template <bool WRITE>
FE_JHD void sub_pass(const uint8_t* bytes, uint32_t s0, uint32_t s1, uint32_t S, uint32_t i, uint32_t nsub, uint32_t entry, const DecGeom& g,
                     const HuffDec* huff, const uint8_t* td, const uint8_t* ta, uint32_t first_blk, const int32_t* pred_in, uint32_t mcu0,
                     uint32_t nmcu, int16_t* coef, const uint8_t* nat, SubResult& R) {
  R.exit = SUB_INVALID; R.nblk = 0; R.dc[0] = R.dc[1] = R.dc[2] = 0; R.err = 0;
  const int eb = (int)((entry >> 8) & 255u), ek = (int)(entry & 255u);
  if (entry == SUB_INVALID || (entry >> 16) > SUB_MAX_PAST || ek >= 64 || eb >= (g.ncomp == 1 ? 1 : g.hs * g.vs + 2)) {
    if (WRITE) R.err = ST_BAD_HUFFMAN;       // no converged exit looks like this: step 4 never writes nothing without saying so
    return;
  }
  const int nl = g.ncomp == 1 ? 1 : g.hs * g.vs, bpm = g.ncomp == 1 ? 1 : nl + 2;      // luma blocks, all blocks of an MCU
  const uint32_t total = nmcu * (uint32_t)bpm;
  const bool last = i + 1 == nsub;
  int b = eb, k = ek;
  uint32_t blk = first_blk;
  int pred[3] = {0, 0, 0}, mx = 0, my = 0;
  int16_t* p = coef;
  auto block_at = [&]() {              // WRITE: block b of MCU (mx, my)
    const int c = b < nl ? 0 : b - nl + 1;
    const int ch = c ? 1 : g.hs, cv = c ? 1 : g.vs, by = c ? 0 : b / g.hs, bx = c ? 0 : b % g.hs;
    return coef + (size_t)(g.blk_off[c] + (uint32_t)(my * cv + by) * g.bw[c] + (uint32_t)(mx * ch + bx)) * 64;
  };
  if (WRITE) {
    if (blk >= total) return;
    b = (int)(blk % (uint32_t)bpm);    // the entry's, restated from the block index so that every address follows from blk < total alone
    const uint32_t m = mcu0 + blk / (uint32_t)bpm;
    my = (int)(m / (uint32_t)g.mw); mx = (int)(m % (uint32_t)g.mw);
    pred[0] = pred_in[0]; pred[1] = pred_in[1]; pred[2] = pred_in[2];
    p = block_at();
  }
  SubReader br;
  br.start(bytes, sub_start(bytes, s0, i, S), s1, last ? (WRITE ? SUB_INVALID : s1) : sub_start(bytes, s0, i + 1, S));
  br.fill_marked();
  br.skip((int)(entry >> 16));
  const uint32_t cap = (WRITE && last) ? SUB_INVALID : 8 * S + 64;
  for (uint32_t it = 0; it < cap; ++it) {
    br.fill_marked();
    if (br.behind()) { R.exit = sub_state(br.past(), b, k); return; }
    const int c = b < nl ? 0 : b - nl + 1;
    if (k == 0) {
      int s = decode_symbol(br, huff[td[c] & 3]);
      if (s < 0 || s > 15) {
        if (WRITE) { R.err = ST_BAD_HUFFMAN; return; }
        br.skip(1); continue;
      }
      if (s) {
        const int r = (int)br.peek(s);
        br.skip(s);
        s = huff_extend(r, s);
      }
      R.dc[c] = (int32_t)((uint32_t)R.dc[c] + (uint32_t)s);
      if (WRITE) {
        pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)s);
        p[0] = (int16_t)pred[c];
      }
      k = 1;
      continue;
    }
    int s = decode_symbol(br, huff[4 + (ta[c] & 3)]);
    if (s < 0) {
      if (WRITE) { R.err = ST_BAD_HUFFMAN; return; }
      br.skip(1); continue;
    }
    const int r = s >> 4;
    s &= 15;
    if (s) {
      k += r;
      const int v = (int)br.peek(s);
      br.skip(s);
      if (k >= 64) {
        if (WRITE) { R.err = ST_BAD_HUFFMAN; return; }
        k = 63;
      }
      if (WRITE) p[nat[k]] = (int16_t)huff_extend(v, s);
      ++k;
    } else {
      k = r == 15 ? k + 16 : 64;       // ZRL, which may run off the block's end as in decode_block; anything else is EOB
    }
    if (k < 64) continue;
    k = 0;                             // the block is complete
    ++R.nblk;
    if (++b == bpm) b = 0;
    if (WRITE) {
      if (b == 0) {
        if (br.overread()) { R.err = ST_PREMATURE_END; return; }
        if (++mx == g.mw) { mx = 0; ++my; }
      }
      if (++blk >= total) return;
      p = block_at();
    }
  }
}

// ---- dequantise + jidctint.c jpeg_idct_islow ------------------------------------------------------------------------------------------
// Two's complement arithmetic that wraps: coefficients a hostile stream chose may overflow 32 bits, which must stay defined behaviour.
FE_JHD int32_t wmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
FE_JHD int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
FE_JHD int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
FE_JHD int32_t wshl(int32_t a, int n) { return (int32_t)((uint32_t)a << n); }
FE_JHD int32_t wdescale(int32_t x, int n) { return wadd(x, 1 << (n - 1)) >> n; }

// ---- progressive scans (jdphuff.c) ----------------------------------------------------------------------------------------------------
// What belongs to one scan. A progressive file brings a fresh DHT in front of every Huffman scan and may change DRI between scans, so the
// tables, the restart interval and the segments are the scan's; quantisation tables, geometry and orientation stay the image's.
constexpr int MAX_SCANS = 32;          // libjpeg's default scripts have 10 (colour) and 6 (gray)
constexpr int FLAG_PROGRESSIVE = 1;    // parse(): take SOF2 files
constexpr int FLAG_PARALLEL = 0x100;   // the decode: baseline segments of at least two subsequences one lane per subsequence; parse() ignores it

struct ScanDesc {
  uint32_t seg_first, nseg;            // this scan's rows of the segment offset arrays
  uint32_t tab_first;                  // first of its Huffman tables in the table pool: ntab of them
  int32_t ri;                          // restart interval in units of this scan, 0: none
  uint8_t ns, comp[3];                 // components, ascending frame indices
  uint8_t tab[3];                      // table of component j, counted from tab_first (DC first); an AC scan has table 0
  uint8_t ntab, ss, se, ah, al;
};

// The units ("MCUs") a scan walks: whole MCUs when it interleaves components, else single blocks over the component's real extent,
// ceil(ceil(w * hs_c / hs_max) / 8) by the same in h, which is not the MCU-padded grid
FE_JHD void scan_extent(const DecGeom& g, const ScanDesc& s, int& uw, int& uh) {
  if (s.ns > 1) { uw = g.mw; uh = g.mh; return; }
  const bool luma = s.comp[0] == 0;    // a grayscale image has cw = w, ch = h
  uw = ((luma ? g.w : g.cw) + 7) >> 3; uh = ((luma ? g.h : g.ch) + 7) >> 3;
}

FE_JHD uint32_t take_bits(BitReader& br, int n) {      // 0 <= n <= 16 <= nbits
  if (n == 0) return 0;
  const uint32_t v = br.peek(n);
  br.skip(n);
  return v;
}
FE_JHD uint32_t take_bit(BitReader& br) {
  if (br.nbits < 16) br.fill();
  return take_bits(br, 1);
}

// decode_mcu_DC_first for one block
FE_JHD int prog_dc_first(BitReader& br, const HuffDec& t, int al, int& pred, int16_t* blk) {
  br.fill();
  int s = decode_symbol(br, t);
  if (s < 0 || s > 15) return ST_BAD_HUFFMAN;
  if (s) s = huff_extend((int)take_bits(br, s), s);
  pred = wadd(pred, s);
  blk[0] = (int16_t)wshl(pred, al);
  return 0;
}

// decode_mcu_AC_first for one block; eobrun: blocks still to be skipped, carried from block to block of a segment
FE_JHD int prog_ac_first(BitReader& br, const HuffDec& t, int ss, int se, int al, uint32_t& eobrun, int16_t* blk, const uint8_t* nat) {
  if (eobrun > 0) { --eobrun; return 0; }
  for (int k = ss; k <= se; ++k) {
    br.fill();
    int s = decode_symbol(br, t);
    if (s < 0) return ST_BAD_HUFFMAN;
    const int r = s >> 4;
    s &= 15;
    if (s) {
      k += r;
      const int v = (int)take_bits(br, s);
      if (k > se) return ST_BAD_HUFFMAN;             // a run past the band
      blk[nat[k & 63]] = (int16_t)wshl(huff_extend(v, s), al);
    } else if (r == 15) {
      k += 15;                                       // ZRL
    } else {
      eobrun = (1u << r) + take_bits(br, r) - 1u;    // this block ends here, and so do the next eobrun
      break;
    }
  }
  return 0;
}

// one correction bit for a coefficient that is already non-zero
FE_JHD void prog_correct(BitReader& br, int16_t* c, int p1) {
  if (take_bit(br) && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c - p1);
}

// decode_mcu_AC_refine for one block
FE_JHD int prog_ac_refine(BitReader& br, const HuffDec& t, int ss, int se, int al, uint32_t& eobrun, int16_t* blk, const uint8_t* nat) {
  const int p1 = 1 << al;
  int k = ss;
  if (eobrun == 0) {
    for (; k <= se; ++k) {
      br.fill();
      int s = decode_symbol(br, t);
      if (s < 0) return ST_BAD_HUFFMAN;
      int r = s >> 4;
      s &= 15;
      int val = 0;
      if (s) {
        if (s != 1) return ST_BAD_HUFFMAN;           // a new coefficient has magnitude 1 << al
        val = take_bits(br, 1) ? p1 : -p1;
      } else if (r != 15) {
        eobrun = (1u << r) + take_bits(br, r);       // this block included: the rest of its band is refined below
        break;
      }
      do {                                           // past r coefficients whose history is zero, correcting the others on the way
        int16_t* c = blk + nat[k & 63];
        if (*c != 0) prog_correct(br, c, p1);
        else if (--r < 0) break;
        ++k;
      } while (k <= se);
      if (val) {
        if (k > se) return ST_BAD_HUFFMAN;           // no zero-history position left in the band
        blk[nat[k & 63]] = (int16_t)val;
      }
    }
  }
  if (eobrun > 0) {
    for (; k <= se; ++k) {
      int16_t* c = blk + nat[k & 63];
      if (*c != 0) prog_correct(br, c, p1);
    }
    --eobrun;
  }
  return 0;
}

// Units u0 .. u0 + nu - 1 of one scan from one segment, in place on the image's coefficient buffer. huff: the scan's tables. The DC
// predictions and EOBRUN start at zero: a segment begins at the scan's start or behind a restart marker.
FE_JHD int decode_scan_segment(BitReader& br, const DecGeom& g, const ScanDesc& sc, const HuffDec* huff, uint32_t u0, uint32_t nu, int16_t* coef,
                               const uint8_t* nat) {
  int uw, uh;
  scan_extent(g, sc, uw, uh);
  int pred[3] = {0, 0, 0};
  uint32_t eobrun = 0;
  int uy = (int)(u0 / (uint32_t)uw), ux = (int)(u0 % (uint32_t)uw);
  for (uint32_t m = 0; m < nu && uy < uh; ++m) {
    if (sc.ss == 0) {
      for (int j = 0; j < sc.ns && j < 3; ++j) {
        const int c = sc.comp[j] < g.ncomp ? sc.comp[j] : 0;
        const int ch = (sc.ns > 1 && c == 0) ? g.hs : 1, cv = (sc.ns > 1 && c == 0) ? g.vs : 1;
        for (int by = 0; by < cv; ++by)
          for (int bx = 0; bx < ch; ++bx) {
            int16_t* blk = coef + (size_t)(g.blk_off[c] + (uint32_t)(uy * cv + by) * g.bw[c] + (uint32_t)(ux * ch + bx)) * 64;
            if (sc.ah == 0) {
              const int rc = prog_dc_first(br, huff[sc.tab[j] < 3 ? sc.tab[j] : 0], sc.al, pred[j], blk);
              if (rc) return rc;
            } else if (take_bit(br)) {               // decode_mcu_DC_refine
              blk[0] = (int16_t)(blk[0] | (1 << sc.al));
            }
          }
      }
    } else {
      const int c = sc.comp[0] < g.ncomp ? sc.comp[0] : 0;
      int16_t* blk = coef + (size_t)(g.blk_off[c] + (uint32_t)uy * g.bw[c] + (uint32_t)ux) * 64;
      const int rc = sc.ah == 0 ? prog_ac_first(br, huff[0], sc.ss, sc.se, sc.al, eobrun, blk, nat)
                                : prog_ac_refine(br, huff[0], sc.ss, sc.se, sc.al, eobrun, blk, nat);
      if (rc) return rc;
    }
    if (br.overread()) return ST_PREMATURE_END;
    if (++ux == uw) { ux = 0; ++uy; }
  }
  return 0;
}

// libjpeg's range_limit[x & RANGE_MASK] behind IDCT_range_limit: x + 128 clamped for the values an honest block gives, wrapped beyond
FE_JHD uint8_t idct_range_limit(int32_t x) {
  const int v = x & 1023;
  return (uint8_t)(v < 128 ? v + 128 : (v < 512 ? 255 : (v < 896 ? 0 : v - 896)));
}

// d[0], d[s], .. d[7s] -> the 1-D inverse transform in place, scaled up by 2^13; the caller descales
FE_JHD void idct_1d(int32_t* d, const int s, int32_t* o) {
  int32_t z2 = d[2 * s], z3 = d[6 * s];
  int32_t z1 = wmul(wadd(z2, z3), 4433);
  int32_t tmp2 = wadd(z1, wmul(z3, -15137));
  int32_t tmp3 = wadd(z1, wmul(z2, 6270));
  z2 = d[0]; z3 = d[4 * s];
  int32_t tmp0 = wshl(wadd(z2, z3), 13), tmp1 = wshl(wsub(z2, z3), 13);
  const int32_t tmp10 = wadd(tmp0, tmp3), tmp13 = wsub(tmp0, tmp3), tmp11 = wadd(tmp1, tmp2), tmp12 = wsub(tmp1, tmp2);
  tmp0 = d[7 * s]; tmp1 = d[5 * s]; tmp2 = d[3 * s]; tmp3 = d[s];
  z1 = wadd(tmp0, tmp3); z2 = wadd(tmp1, tmp2); z3 = wadd(tmp0, tmp2);
  int32_t z4 = wadd(tmp1, tmp3);
  const int32_t z5 = wmul(wadd(z3, z4), 9633);
  tmp0 = wmul(tmp0, 2446); tmp1 = wmul(tmp1, 16819); tmp2 = wmul(tmp2, 25172); tmp3 = wmul(tmp3, 12299);
  z1 = wmul(z1, -7373); z2 = wmul(z2, -20995); z3 = wadd(wmul(z3, -16069), z5); z4 = wadd(wmul(z4, -3196), z5);
  tmp0 = wadd(tmp0, wadd(z1, z3)); tmp1 = wadd(tmp1, wadd(z2, z4)); tmp2 = wadd(tmp2, wadd(z2, z3)); tmp3 = wadd(tmp3, wadd(z1, z4));
  o[0] = wadd(tmp10, tmp3); o[7] = wsub(tmp10, tmp3);
  o[1] = wadd(tmp11, tmp2); o[6] = wsub(tmp11, tmp2);
  o[2] = wadd(tmp12, tmp1); o[5] = wsub(tmp12, tmp1);
  o[3] = wadd(tmp13, tmp0); o[4] = wsub(tmp13, tmp0);
}

// 8 samples of a plane row, little-endian in two words; p is 8-byte aligned (planes are, and their strides are multiples of 8)
FE_JHD void store8(uint8_t* p, uint32_t lo, uint32_t hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
#else
  for (int i = 0; i < 4; ++i) { p[i] = (uint8_t)(lo >> (8 * i)); p[4 + i] = (uint8_t)(hi >> (8 * i)); }
#endif
}

// coef, q: natural order. out: 8 rows of `stride` bytes. Returns false when the block left the range in which libjpeg's C code (wrapping
// 32-bit sums, masked range-limit table) and libjpeg-turbo's SIMD code (16-bit products, saturating packs) give the same samples: a
// dequantised value or a first-pass value outside int16, or a sample before the table outside [-512, 511]. No encoder writes such a block.
FE_JHD bool idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, size_t stride) {
  int32_t ws[64];
  constexpr int CONST_BITS = 13, PASS1_BITS = 2;
  uint32_t wide = 0;                     // bits that are set only when some value v is outside [-lim, lim): (v + lim) >> shift != 0
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    ws[i] = wmul(coef[i], q[i]);
    wide |= (uint32_t)wadd(ws[i], 32768) >> 16;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int32_t o[8];
    idct_1d(ws + c, 8, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      ws[r * 8 + c] = wdescale(o[r], CONST_BITS - PASS1_BITS);
      wide |= (uint32_t)wadd(ws[r * 8 + c], 32768) >> 16;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int32_t o[8];
    idct_1d(ws + r * 8, 1, o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int32_t v = wdescale(o[c], CONST_BITS + PASS1_BITS + 3);
      wide |= (uint32_t)wadd(v, 512) >> 10;
      if (c < 4) lo |= (uint32_t)idct_range_limit(v) << (8 * c);
      else hi |= (uint32_t)idct_range_limit(v) << (8 * (c - 4));
    }
    store8(out + r * stride, lo, hi);
  }
  return wide == 0;
}

// ---- scaled decode: libjpeg's scale_num / scale_denom = 1 / scale, which is what Pillow's JpegImageFile.draft() asks for ------------------
// jdmaster.c: the image shrinks to ceil(w / scale) x ceil(h / scale) by transforming every luma block into 8 / scale samples a side
// instead of 8. A chroma component doubles its own transform size while that still divides the sampling ratio in both directions, so
// subsampled chroma is scaled up by its IDCT instead of by the upsampler:
//   scale   4:4:4 / gray   4:2:2 (Y, C, upsampling)        4:2:0 (Y, C, upsampling)
//     2     4              4, 4, h2v1 fancy                 4, 8, none
//     4     2              2, 2, h2v1 fancy                 2, 4, none
//     8     1              1, 1, h2v1 replicated            1, 2, none
// (jdsample.c switches the triangle filter off when the smallest transform is 1 x 1, and as ever for a component no wider than 2 samples.)
// The h2v2 upsamplers are never reached at scale > 1 with the samplings parse() takes.
// The reduced transforms are jidctred.c's: jpeg_idct_islow's fixed point (CONST_BITS 13, PASS1_BITS 2) over the coefficients that survive.
// 4x4 skips row 4 and column 4 of the block, 2x2 reads rows / columns 0, 1, 3, 5, 7 only, 1x1 is the DC term.
// Range rule, as idct_block's: libjpeg-turbo's SIMD 4x4 and 2x2 keep dequantised and first-pass values in 16 bits and saturate the
// samples, the C code wraps 32-bit sums and masks into its table, so a block with a dequantised coefficient (of those the transform
// reads) or a first-pass value outside int16, or a sample before the table outside [-512, 511], is reported (ST_BAD_COEFFICIENT). The 1x1
// transform exists in C only and int16 * uint16 cannot wrap: it reports nothing.
constexpr int UP_NONE = 0, UP_H2V1_FANCY = 1, UP_H2V1_REPLICATE = 2;

struct ScaledGeom {
  int scale, ow, oh;                   // output size before any EXIF transpose: ceil(w / scale), ceil(h / scale)
  int ss[3];                           // samples a side that a block of each component becomes
  int pack[3];                         // horizontally adjacent blocks one work item transforms, so that it stores whole dwords
  int gw[3];                           // work items per block row: ceil(bw / pack)
  uint32_t grp_off[4];                 // first work item of each component; [3]: their number
  int stride[3];                       // bytes per plane row: bw * ss rounded up to a dword
  uint32_t plane_off[3], plane_bytes;  // a plane is [bh * ss][stride], 16-byte aligned; never more than DecGeom's plane_bytes
  int cw;                              // real width of a chroma plane (jdmaster.c downsampled_width)
  int up;                              // UP_*
};

FE_JHD ScaledGeom make_scaled_geom(const DecGeom& g, int scale) {
  ScaledGeom s;
  s.scale = scale;
  s.ow = (g.w + scale - 1) / scale; s.oh = (g.h + scale - 1) / scale;
  const int mn = 8 / scale;
  uint32_t p = 0, n = 0;
  for (int c = 0; c < 3; ++c) {
    int ss = mn;
    const int ch = c ? 1 : g.hs, cv = c ? 1 : g.vs;        // this component's sampling factors
    while (ss < 8 && (g.hs * mn) % (ch * ss * 2) == 0 && (g.vs * mn) % (cv * ss * 2) == 0) ss *= 2;
    s.ss[c] = ss;
    s.pack[c] = ss >= 4 ? 1 : 4 / ss;
    s.gw[c] = (g.bw[c] + s.pack[c] - 1) / s.pack[c];
    s.grp_off[c] = n;
    n += (uint32_t)s.gw[c] * (uint32_t)g.bh[c];
    s.stride[c] = (g.bw[c] * ss + 3) & ~3;
    s.plane_off[c] = p;
    p += ((uint32_t)s.stride[c] * (uint32_t)(g.bh[c] * ss) + 15u) & ~15u;
  }
  s.grp_off[3] = n; s.plane_bytes = p;
  const int in_group = s.ss[1] / mn;                       // chroma samples per output group, against hs luma ones
  s.up = (g.ncomp == 1 || in_group == g.hs) ? UP_NONE : (mn > 1 ? UP_H2V1_FANCY : UP_H2V1_REPLICATE);
  s.cw = (g.w * s.ss[1] + g.hs * 8 - 1) / (g.hs * 8);
  return s;
}

// 8 coefficients of one block row
FE_JHD void load_coef_row(const int16_t* p, int32_t* r) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 u = *reinterpret_cast<const uint4*>(p);       // a block is 128 bytes, 16-byte aligned
  const uint32_t wds[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) { r[2 * j] = (int16_t)(wds[j] & 0xFFFFu); r[2 * j + 1] = (int16_t)(wds[j] >> 16); }
#else
  for (int j = 0; j < 8; ++j) r[j] = p[j];
#endif
}

FE_JHD void store4(uint8_t* p, uint32_t v) {                // p is 4-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<uint32_t*>(p) = v;
#else
  for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
#endif
}

// jidctred.c jpeg_idct_4x4's 1-D step on d[0 .. 7] without d[4] -> 4 values scaled up by 2^14
FE_JHD void idct4_1d(const int32_t* d, int32_t* o) {
  const int32_t tmp0 = wshl(d[0], 14);
  const int32_t tmp2 = wadd(wmul(d[2], 15137), wmul(d[6], -6270));
  const int32_t tmp10 = wadd(tmp0, tmp2), tmp12 = wsub(tmp0, tmp2);
  const int32_t a = wadd(wadd(wmul(d[7], -1730), wmul(d[5], 11893)), wadd(wmul(d[3], -17799), wmul(d[1], 8697)));
  const int32_t b = wadd(wadd(wmul(d[7], -4176), wmul(d[5], -4926)), wadd(wmul(d[3], 7373), wmul(d[1], 20995)));
  o[0] = wadd(tmp10, b); o[3] = wsub(tmp10, b);
  o[1] = wadd(tmp12, a); o[2] = wsub(tmp12, a);
}

// jpeg_idct_2x2's: d[0], d[1], d[3], d[5], d[7] -> 2 values scaled up by 2^15
FE_JHD void idct2_1d(const int32_t* d, int32_t* o) {
  const int32_t tmp10 = wshl(d[0], 15);
  const int32_t t = wadd(wadd(wmul(d[7], -5906), wmul(d[5], 6967)), wadd(wmul(d[3], -10426), wmul(d[1], 29692)));
  o[0] = wadd(tmp10, t); o[1] = wsub(tmp10, t);
}

// coef, q: natural order. out: 4 rows of 4 samples, one dword each. false: outside the range stated above.
FE_JHD bool idct_4x4(const int16_t* coef, const uint16_t* q, uint32_t* out) {
  int32_t ws[4][8];                      // [output row][column]
  int32_t in[8][8];
  uint32_t wide = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    if (r == 4) continue;
    load_coef_row(coef + 8 * r, in[r]);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c == 4) continue;
      in[r][c] = wmul(in[r][c], q[8 * r + c]);
      wide |= (uint32_t)wadd(in[r][c], 32768) >> 16;
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c == 4) continue;
    const int32_t d[8] = {in[0][c], in[1][c], in[2][c], in[3][c], 0, in[5][c], in[6][c], in[7][c]};
    int32_t o[4];
    idct4_1d(d, o);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ws[r][c] = wdescale(o[r], 12);     // CONST_BITS - PASS1_BITS + 1
      wide |= (uint32_t)wadd(ws[r][c], 32768) >> 16;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ws[r][4] = 0;
    int32_t o[4];
    idct4_1d(ws[r], o);
    uint32_t v4 = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int32_t v = wdescale(o[c], 19);      // CONST_BITS + PASS1_BITS + 3 + 1
      wide |= (uint32_t)wadd(v, 512) >> 10;
      v4 |= (uint32_t)idct_range_limit(v) << (8 * c);
    }
    out[r] = v4;
  }
  return wide == 0;
}

// out: samples (0,0), (0,1), (1,0), (1,1) in the bytes of one word, lowest first
FE_JHD bool idct_2x2(const int16_t* coef, const uint16_t* q, uint32_t* out) {
  constexpr int used[5] = {0, 1, 3, 5, 7};
  int32_t in[8][8];
  int32_t ws[2][8];
  uint32_t wide = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int r = used[i];
    load_coef_row(coef + 8 * r, in[r]);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int c = used[j];
      in[r][c] = wmul(in[r][c], q[8 * r + c]);
      wide |= (uint32_t)wadd(in[r][c], 32768) >> 16;
    }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int c = used[j];
    const int32_t d[8] = {in[0][c], in[1][c], 0, in[3][c], 0, in[5][c], 0, in[7][c]};
    int32_t o[2];
    idct2_1d(d, o);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      ws[r][c] = wdescale(o[r], 13);     // CONST_BITS - PASS1_BITS + 2
      wide |= (uint32_t)wadd(ws[r][c], 32768) >> 16;
    }
  }
  uint32_t v4 = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    ws[r][2] = ws[r][4] = ws[r][6] = 0;
    int32_t o[2];
    idct2_1d(ws[r], o);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int32_t v = wdescale(o[c], 20);      // CONST_BITS + PASS1_BITS + 3 + 2
      wide |= (uint32_t)wadd(v, 512) >> 10;
      v4 |= (uint32_t)idct_range_limit(v) << (8 * (2 * r + c));
    }
  }
  *out = v4;
  return wide == 0;
}

// jpeg_idct_1x1
FE_JHD uint8_t idct_1x1(int16_t dc, uint16_t q0) { return idct_range_limit(wdescale(wmul(dc, q0), 3)); }

// One work item of the scaled transform: blocks gx * pack .. of a block row whose first block is at `row` (bw blocks of 64 coefficients),
// each transformed into ss x ss samples of the plane rows starting at `out` (the block row's first sample). Blocks past bw give zero
// bytes inside the row's padding, so every store is a whole dword.
FE_JHD bool idct_group(const int16_t* row, int gx, int bw, int ss, const uint16_t* q, uint8_t* out, size_t stride) {
  if (ss == 8) return idct_block(row + (size_t)gx * 64, q, out + (size_t)gx * 8, stride);
  if (ss == 4) {
    uint32_t v[4];
    const bool ok = idct_4x4(row + (size_t)gx * 64, q, v);
#pragma unroll
    for (int r = 0; r < 4; ++r) store4(out + r * stride + (size_t)gx * 4, v[r]);
    return ok;
  }
  if (ss == 2) {
    uint32_t v[2] = {0, 0};
    bool ok = true;
    for (int j = 0; j < 2; ++j)
      if (2 * gx + j < bw) ok &= idct_2x2(row + (size_t)(2 * gx + j) * 64, q, v + j);
    store4(out + (size_t)gx * 4, (v[0] & 0xFFFFu) | (v[1] << 16));
    store4(out + stride + (size_t)gx * 4, (v[0] >> 16) | (v[1] & 0xFFFF0000u));
    return ok;
  }
  uint32_t v = 0;
  for (int j = 0; j < 4; ++j)
    if (4 * gx + j < bw) v |= (uint32_t)idct_1x1(row[(size_t)(4 * gx + j) * 64], q[0]) << (8 * j);
  store4(out + (size_t)gx * 4, v);
  return true;
}

// ---- upsampling (jdsample.c with do_fancy_upsampling) + jdcolor.c ---------------------------------------------------------------------
// Chroma sample for pixel (x, y) of a component subsampled hs x vs; p: its plane, stride bytes per row; cw x ch: its real extent.
// A component no wider than 2 samples is replicated (jinit_upsampler takes the fancy routines for downsampled_width > 2 only).
FE_JHD int chroma_at(const uint8_t* p, int stride, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(size_t)y * stride + x];      // vs == 1 as well
  const int cx = x >> 1;
  if (vs == 1) {                                      // h2v1
    const uint8_t* r = p + (size_t)y * stride;
    if (cw <= 2) return r[cx];
    if (x & 1) return cx == cw - 1 ? r[cx] : (3 * r[cx] + r[cx + 1] + 2) >> 2;
    return cx == 0 ? r[cx] : (3 * r[cx] + r[cx - 1] + 1) >> 2;
  }
  const int cy = y >> 1;                              // h2v2
  if (cw <= 2) return p[(size_t)cy * stride + cx];
  int fy = (y & 1) ? cy + 1 : cy - 1;                 // the nearer of the two neighbouring rows; the image's first / last row repeats
  fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
  const uint8_t* r0 = p + (size_t)cy * stride;
  const uint8_t* r1 = p + (size_t)fy * stride;
  const int cur = 3 * r0[cx] + r1[cx];
  if (x & 1) return cx == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

FE_JHD uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// jdcolor.c ycc_rgb_convert: 16.16 constants 1.40200, 1.77200, 0.71414, 0.34414 with ONE_HALF inside the tables
FE_JHD void ycc_to_rgb(int y, int cb, int cr, uint8_t* r, uint8_t* g, uint8_t* b) {
  cb -= 128; cr -= 128;
  *r = clamp_u8(y + ((91881 * cr + 32768) >> 16));
  *g = clamp_u8(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  *b = clamp_u8(y + ((116130 * cb + 32768) >> 16));
}

// pixel (x, y) of the decoded image from its planes -> rgb[3]
FE_JHD void pixel_rgb(const uint8_t* planes, const DecGeom& g, int x, int y, uint8_t* rgb) {
  const int yv = planes[g.plane_off[0] + (size_t)y * (g.bw[0] * 8) + x];
  if (g.ncomp == 1) { rgb[0] = rgb[1] = rgb[2] = (uint8_t)yv; return; }
  const int cb = chroma_at(planes + g.plane_off[1], g.bw[1] * 8, g.cw, g.ch, g.hs, g.vs, x, y);
  const int cr = chroma_at(planes + g.plane_off[2], g.bw[2] * 8, g.cw, g.ch, g.hs, g.vs, x, y);
  ycc_to_rgb(yv, cb, cr, rgb, rgb + 1, rgb + 2);
}

// pixel (x, y) of the ceil(w / scale) x ceil(h / scale) image from the planes of the scaled transform
FE_JHD void pixel_rgb_scaled(const uint8_t* planes, const DecGeom& g, const ScaledGeom& s, int x, int y, uint8_t* rgb) {
  const int yv = planes[s.plane_off[0] + (size_t)y * s.stride[0] + x];
  if (g.ncomp == 1) { rgb[0] = rgb[1] = rgb[2] = (uint8_t)yv; return; }
  int cc[2];
#pragma unroll
  for (int c = 1; c < 3; ++c) {
    const uint8_t* p = planes + s.plane_off[c];
    if (s.up == UP_NONE) cc[c - 1] = p[(size_t)y * s.stride[c] + x];
    else if (s.up == UP_H2V1_REPLICATE) cc[c - 1] = p[(size_t)y * s.stride[c] + (x >> 1)];
    else cc[c - 1] = chroma_at(p, s.stride[c], s.cw, 0, 2, 1, x, y);
  }
  ycc_to_rgb(yv, cc[0], cc[1], rgb, rgb + 1, rgb + 2);
}

// where pixel (x, y) of a w x h image lands under EXIF orientation o (ImageOps.exif_transpose): pixel index in the output, whose width is
// w for o <= 4 and h above
FE_JHD size_t oriented_index(int o, int w, int h, int x, int y) {
  switch (o) {
    case 2: return (size_t)y * w + (w - 1 - x);                    // FLIP_LEFT_RIGHT
    case 3: return (size_t)(h - 1 - y) * w + (w - 1 - x);          // ROTATE_180
    case 4: return (size_t)(h - 1 - y) * w + x;                    // FLIP_TOP_BOTTOM
    case 5: return (size_t)x * h + y;                              // TRANSPOSE
    case 6: return (size_t)x * h + (h - 1 - y);                    // ROTATE_270
    case 7: return (size_t)(w - 1 - x) * h + (h - 1 - y);          // TRANSVERSE
    case 8: return (size_t)(w - 1 - x) * h + y;                    // ROTATE_90
    default: return (size_t)y * w + x;
  }
}

// ---- host: marker parser, table builder, whole-image decode -----------------------------------------------------------------------------
static const uint8_t kNatural[64] = FE_JPEG_NATURAL_ORDER;

struct Component { uint8_t id, hs, vs, tq, td, ta; };

struct Parsed {
  int32_t status = ST_BAD_MARKER;
  int width = 0, height = 0, ncomp = 0, hs = 1, vs = 1, ri = 0, orientation = 1;
  Component comp[3] = {};
  uint16_t q[4][64] = {};
  uint8_t bits[8][16] = {}, vals[8][256] = {};
  bool q_set[4] = {}, h_set[8] = {};
  std::vector<uint32_t> seg_start, seg_end;      // byte offsets of the entropy-coded segments in the file; of all scans, in file order
  // a progressive file (FLAG_PROGRESSIVE): its scans, and the decoding tables each was written with (ri: the first scan's)
  bool progressive = false;
  bool incomplete = false;                       // status ST_OTHER because the scans stop short of all 64 coefficients at full precision
  std::vector<ScanDesc> scans;
  std::vector<HuffDec> scan_tabs;
};

// jdhuff.c jpeg_make_d_derived_tbl; false: the counts describe no prefix code
inline bool build_huff_dec(const uint8_t* bits, const uint8_t* vals, HuffDec& t) {
  memset(&t, 0, sizeof(t));
  int total = 0;
  for (int l = 1; l <= 16; ++l) total += bits[l - 1];
  if (total > 256) return false;
  uint32_t code = 0;
  int p = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = bits[l - 1];
    if (n == 0) { t.maxcode[l] = -1; t.valoff[l] = 0; code <<= 1; continue; }
    if (code + (uint32_t)n > (1u << l)) return false;
    t.valoff[l] = p - (int32_t)code;
    for (int i = 0; i < n; ++i, ++p, ++code) {
      t.vals[p] = vals[p];
      if (l <= LOOK_BITS) {
        const uint32_t first = code << (LOOK_BITS - l);
        for (uint32_t f = 0; f < (1u << (LOOK_BITS - l)); ++f) t.look[first + f] = (uint16_t)((l << 8) | vals[p]);
      }
    }
    t.maxcode[l] = (int32_t)code - 1;
    code <<= 1;
  }
  t.maxcode[0] = -1;
  return true;
}

namespace detail {
inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

// IFD0's orientation tag of an APP1/Exif payload (after "Exif\0\0"). 0: no tag; -1: a block this parser does not judge
inline int exif_orientation(const uint8_t* p, size_t n) {
  if (n < 8) return -1;
  const bool le = p[0] == 'I' && p[1] == 'I', be = p[0] == 'M' && p[1] == 'M';
  if (!le && !be) return -1;
  auto u16 = [&](size_t o) { return le ? (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) : ((uint32_t)p[o] << 8) | p[o + 1]; };
  auto u32 = [&](size_t o) { return le ? u16(o) | (u16(o + 2) << 16) : (u16(o) << 16) | u16(o + 2); };
  if (u16(2) != 42) return -1;
  const size_t ifd = u32(4);
  if (ifd > n || n - ifd < 2) return -1;
  const size_t cnt = u16(ifd);
  for (size_t i = 0; i < cnt; ++i) {
    const size_t e = ifd + 2 + 12 * i;
    if (e > n || n - e < 12) return -1;
    if (u16(e) != 0x0112) continue;
    const uint32_t type = u16(e + 2), count = u32(e + 4);
    if (count != 1) return -1;
    if (type == 3) return (int)u16(e + 8);
    if (type == 4) { const uint32_t v = u32(e + 8); return v > 65535 ? -1 : (int)v; }
    return -1;
  }
  return 0;
}

inline bool contains(const uint8_t* p, size_t n, const char* s) {
  const size_t m = strlen(s);
  for (size_t i = 0; i + m <= n; ++i)
    if (memcmp(p + i, s, m) == 0) return true;
  return false;
}
}  // namespace detail

// the payload of a DHT segment into P's current tables; 0 or the status
inline int32_t read_dht(const uint8_t* s, size_t n, Parsed& P) {
  size_t o = 0;
  while (o < n) {
    if (n - o < 17) return ST_BAD_MARKER;
    const int tc = s[o] >> 4, th = s[o] & 15;
    if (tc > 1 || th > 3) return ST_BAD_MARKER;
    int total = 0;
    for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
    if (total > 256 || (size_t)total > n - o - 17) return ST_BAD_MARKER;
    const int slot = tc * 4 + th;
    memcpy(P.bits[slot], s + o + 1, 16);
    memset(P.vals[slot], 0, 256);
    memcpy(P.vals[slot], s + o + 17, (size_t)total);
    P.h_set[slot] = true;
    o += 17 + (size_t)total;
  }
  return ST_OK;
}

// Entropy-coded data from `pos` on, cut at its restart markers into P.seg_start / seg_end; `want` segments belong there. Returns the
// marker that ends it (> 0) and sets `next` behind that marker, or the negative status of a stream that is cut wrongly.
inline int cut_segments(const uint8_t* d, size_t len, size_t pos, int ri, uint64_t want, Parsed& P, size_t& next) {
  const size_t seg0 = P.seg_start.size();
  size_t start = pos, i = pos;
  int marker = -1;
  while (i < len) {
    if (d[i] != 0xFF) { ++i; continue; }
    size_t j = i + 1;
    while (j < len && d[j] == 0xFF) ++j;                     // fill bytes before a marker
    if (j >= len) { i = len; break; }
    if (d[j] == 0x00) {
      if (j != i + 1) return ST_BAD_MARKER;                 // fill bytes in front of a stuffed zero
      i += 2;
      continue;
    }
    P.seg_start.push_back((uint32_t)start);
    P.seg_end.push_back((uint32_t)i);
    const size_t have = P.seg_start.size() - seg0;
    if (d[j] >= 0xD0 && d[j] <= 0xD7) {
      if (!ri || d[j] != 0xD0 + (int)((have - 1) & 7)) return ST_BAD_RESTART;
      if (have >= want) return ST_BAD_RESTART;              // a restart marker behind the last interval
      start = i = j + 1;
      continue;
    }
    marker = d[j];
    i = j + 1;
    break;
  }
  if (marker < 0) return ST_PREMATURE_END;
  if (P.seg_start.size() - seg0 < want) return ST_PREMATURE_END;
  next = i;
  return marker;
}
inline void parse_scans(const uint8_t* d, size_t len, size_t pos, Parsed& P);

// Reads the markers of one file. P.status: 0 when this decoder takes the file, then everything in P is set and the tables named by the
// scan exist and are prefix codes; otherwise the first reason found. Width, height and components are set whenever a frame header was read.
// flags: FLAG_PROGRESSIVE takes SOF2 files whose scans form a complete normal progression (parse_scans); without it they get ST_PROGRESSIVE.
inline void parse(const uint8_t* d, size_t len, Parsed& P, int flags = 0) {
  using detail::be16;
  P = Parsed();
  auto fail = [&P](int32_t s) { P.status = s; };
  if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(ST_BAD_MARKER);
  size_t pos = 2;
  bool have_sof = false, jfif = false, adobe = false, exif_seen = false, exif_odd = false, xmp_orient = false;
  int adobe_transform = -1, exif_orient = 0;
  for (;;) {
    if (pos + 2 > len) return fail(ST_PREMATURE_END);
    if (d[pos] != 0xFF) return fail(ST_BAD_MARKER);
    while (pos + 1 < len && d[pos + 1] == 0xFF) ++pos;      // fill bytes
    if (pos + 2 > len) return fail(ST_PREMATURE_END);
    const int m = d[pos + 1];
    pos += 2;
    if (m == 0x01) continue;                                 // TEM
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x00) return fail(ST_BAD_MARKER);
    if (m == 0xD9) return fail(ST_PREMATURE_END);            // EOI before any scan
    if (pos + 2 > len) return fail(ST_PREMATURE_END);
    const size_t L = be16(d + pos);
    if (L < 2) return fail(ST_BAD_MARKER);
    if (L > len - pos) return fail(ST_PREMATURE_END);
    const uint8_t* s = d + pos + 2;
    const size_t n = L - 2;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {      // a frame header
      if (have_sof) return fail(ST_BAD_MARKER);
      if (n < 6) return fail(ST_BAD_MARKER);
      have_sof = true;
      P.height = (int)be16(s + 1); P.width = (int)be16(s + 3); P.ncomp = s[5];
      if (m == 0xC2 && !(flags & FLAG_PROGRESSIVE)) return fail(ST_PROGRESSIVE);
      if (m >= 0xC9) return fail(ST_ARITHMETIC);
      if (m != 0xC0 && m != 0xC1 && m != 0xC2) return fail(ST_OTHER);
      P.progressive = m == 0xC2;
      if (s[0] != 8) return fail(ST_PRECISION);
      if (P.width == 0) return fail(ST_BAD_MARKER);
      if (P.height == 0) return fail(ST_OTHER);              // the height comes in a DNL marker
      if (P.ncomp != 1 && P.ncomp != 3) return fail(P.ncomp == 0 ? ST_BAD_MARKER : ST_COMPONENTS);
      if (n != (size_t)(6 + 3 * P.ncomp)) return fail(ST_BAD_MARKER);
      for (int c = 0; c < P.ncomp; ++c) {
        Component& k = P.comp[c];
        k.id = s[6 + 3 * c]; k.hs = s[7 + 3 * c] >> 4; k.vs = s[7 + 3 * c] & 15; k.tq = s[8 + 3 * c];
        if (k.hs < 1 || k.hs > 4 || k.vs < 1 || k.vs > 4 || k.tq > 3) return fail(ST_BAD_MARKER);
      }
      if (P.ncomp == 3) {
        const Component* k = P.comp;
        const bool luma_ok = (k[0].hs == 1 && k[0].vs == 1) || (k[0].hs == 2 && k[0].vs == 1) || (k[0].hs == 2 && k[0].vs == 2);
        if (!luma_ok || k[1].hs != 1 || k[1].vs != 1 || k[2].hs != 1 || k[2].vs != 1) return fail(ST_SAMPLING);
        P.hs = k[0].hs; P.vs = k[0].vs;
      } else {
        P.hs = P.vs = 1;                                     // a single-component scan is not interleaved: one block per MCU
      }
    } else if (m == 0xCC) {
      return fail(ST_ARITHMETIC);
    } else if (m == 0xC4) {
      const int32_t rc = read_dht(s, n, P);
      if (rc) return fail(rc);
    } else if (m == 0xDB) {
      size_t o = 0;
      while (o < n) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (pq > 1 || tq > 3) return fail(ST_BAD_MARKER);
        const size_t need = 1 + (pq ? 128 : 64);
        if (n - o < need) return fail(ST_BAD_MARKER);
        for (int z = 0; z < 64; ++z) P.q[tq][kNatural[z]] = (uint16_t)(pq ? be16(s + o + 1 + 2 * z) : s[o + 1 + z]);
        P.q_set[tq] = true;
        o += need;
      }
    } else if (m == 0xDD) {
      if (n != 2) return fail(ST_BAD_MARKER);
      P.ri = (int)be16(s);
    } else if (m == 0xE0) {
      if (n >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
    } else if (m == 0xE1) {
      if (n >= 6 && memcmp(s, "Exif\0\0", 6) == 0) {
        if (exif_seen) exif_odd = true;                      // a second block: Pillow joins them
        else {
          exif_seen = true;
          exif_orient = detail::exif_orientation(s + 6, n - 6);
          if (exif_orient < 0) exif_odd = true;
        }
      } else if (detail::contains(s, n, "tiff:Orientation")) {
        xmp_orient = true;                                   // Pillow reads it when the EXIF block has no orientation
      }
    } else if (m == 0xDA) {
      if (!have_sof) return fail(ST_BAD_MARKER);
      if (P.progressive) break;                              // pos stays at this first SOS: parse_scans reads every scan header
      if (n < 1) return fail(ST_BAD_MARKER);
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != (size_t)(4 + 2 * ns)) return fail(ST_BAD_MARKER);
      if (ns != P.ncomp) return fail(ST_MULTISCAN);
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != P.comp[c].id) return fail(ST_OTHER);
        P.comp[c].td = s[2 + 2 * c] >> 4; P.comp[c].ta = s[2 + 2 * c] & 15;
        if (P.comp[c].td > 3 || P.comp[c].ta > 3) return fail(ST_BAD_MARKER);
      }
      pos += L;
      break;
    }
    pos += L;
  }
  // what Pillow would see that this decoder does not reproduce
  if (exif_odd || (xmp_orient && exif_orient == 0)) return fail(ST_OTHER);
  P.orientation = exif_orient >= 2 && exif_orient <= 8 ? exif_orient : 1;
  if (P.ncomp == 3) {                                        // jdapimin.c default_decompress_parms
    bool ycc = true;
    if (jfif) ycc = true;
    else if (adobe) ycc = adobe_transform != 0;
    else ycc = !(P.comp[0].id == 'R' && P.comp[1].id == 'G' && P.comp[2].id == 'B');
    if (!ycc) return fail(ST_ADOBE_RGB);
  }
  if (P.progressive) return parse_scans(d, len, pos, P);
  for (int c = 0; c < P.ncomp; ++c) {
    if (!P.q_set[P.comp[c].tq] || !P.h_set[P.comp[c].td] || !P.h_set[4 + P.comp[c].ta]) return fail(ST_BAD_MARKER);
    HuffDec t;
    if (!build_huff_dec(P.bits[P.comp[c].td], P.vals[P.comp[c].td], t)) return fail(ST_BAD_HUFFMAN);
    for (int i = 0; i < 256; ++i)
      if (P.vals[P.comp[c].td][i] > 15) return fail(ST_BAD_HUFFMAN);
    if (!build_huff_dec(P.bits[4 + P.comp[c].ta], P.vals[4 + P.comp[c].ta], t)) return fail(ST_BAD_HUFFMAN);
  }
  // the entropy-coded data: cut at the restart markers
  const DecGeom g = make_dec_geom(P.width, P.height, P.ncomp, P.hs, P.vs);
  const uint64_t mcus = (uint64_t)g.mw * g.mh;
  const uint64_t want = P.ri ? (mcus + P.ri - 1) / P.ri : 1;
  if (len > 0xFFFFFFF0u) return fail(ST_OTHER);
  size_t i = pos;
  int marker = cut_segments(d, len, pos, P.ri, want, P, i);
  if (marker < 0) return fail(marker);
  while (marker != 0xD9) {                                   // what follows the scan: another scan makes the file multi-scan
    if (marker == 0xDA) return fail(ST_MULTISCAN);
    if (marker == 0xC4 || marker == 0xDB || marker == 0xDD || marker == 0xDC || marker == 0xFE || (marker >= 0xE0 && marker <= 0xEF)) {
      if (i + 2 > len) return fail(ST_PREMATURE_END);
      const size_t L = be16(d + i);
      if (L < 2) return fail(ST_BAD_MARKER);
      if (L > len - i) return fail(ST_PREMATURE_END);
      if (marker == 0xDC) return fail(ST_OTHER);
      i += L;
      if (i + 2 > len) return fail(ST_PREMATURE_END);
      if (d[i] != 0xFF) return fail(ST_BAD_MARKER);
      while (i + 1 < len && d[i + 1] == 0xFF) ++i;
      if (i + 2 > len) return fail(ST_PREMATURE_END);
      marker = d[i + 1];
      i += 2;
    } else {
      return fail(ST_BAD_MARKER);
    }
  }
  P.status = ST_OK;
}

// The scans of a progressive file, from its first SOS (pos: at that segment's length field) to EOI. Status 0 only for what libjpeg decodes
// without inter-block smoothing and exactly as a baseline file from there on: every scan within jdphuff.c's parameter rules, the scans
// in the normal progression (a coefficient's first scan has Ah = 0, every later one has Ah = the Al it was left at), and complete (all
// 64 coefficients of every component down to Al = 0). A file whose scans are in order but stop short is ST_OTHER with P.incomplete: its
// scans can still be run to tell whether the stream is corrupt as well.
inline void parse_scans(const uint8_t* d, size_t len, size_t pos, Parsed& P) {
  using detail::be16;
  auto fail = [&P](int32_t s) { P.status = s; };
  for (int c = 0; c < P.ncomp; ++c)
    if (!P.q_set[P.comp[c].tq]) return fail(ST_BAD_MARKER);
  if (len > 0xFFFFFFF0u) return fail(ST_OTHER);
  const DecGeom g = make_dec_geom(P.width, P.height, P.ncomp, P.hs, P.vs);
  int8_t left[3][64];                                        // the Al each coefficient was left at, -1: no scan has touched it
  memset(left, -1, sizeof(left));
  for (;;) {
    if (pos + 2 > len) return fail(ST_PREMATURE_END);
    const size_t L = be16(d + pos);
    if (L < 2) return fail(ST_BAD_MARKER);
    if (L > len - pos) return fail(ST_PREMATURE_END);
    const uint8_t* s = d + pos + 2;
    const size_t n = L - 2;
    if (n < 1) return fail(ST_BAD_MARKER);
    const int ns = s[0];
    if (ns < 1 || ns > 4 || n != (size_t)(4 + 2 * ns) || ns > P.ncomp) return fail(ST_BAD_MARKER);
    if (P.scans.size() >= (size_t)MAX_SCANS) return fail(ST_OTHER);
    ScanDesc sc;
    memset(&sc, 0, sizeof(sc));
    sc.ns = (uint8_t)ns;
    int td[3] = {0, 0, 0}, ta = 0, prev = -1;
    for (int j = 0; j < ns; ++j) {
      int c = prev + 1;
      while (c < P.ncomp && P.comp[c].id != s[1 + 2 * j]) ++c;
      if (c >= P.ncomp) return fail(ST_OTHER);               // not a component of the frame, or out of frame order
      prev = c;
      sc.comp[j] = (uint8_t)c;
      td[j] = s[2 + 2 * j] >> 4; ta = s[2 + 2 * j] & 15;
      if (td[j] > 3 || ta > 3) return fail(ST_BAD_MARKER);
    }
    const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ah = s[3 + 2 * ns] >> 4, al = s[3 + 2 * ns] & 15;
    // jdphuff.c start_pass_phuff_decoder
    if (ss == 0 ? se != 0 : (ss > se || se > 63 || ns != 1)) return fail(ST_BAD_MARKER);
    if ((ah != 0 && al != ah - 1) || al > 13) return fail(ST_BAD_MARKER);
    sc.ss = (uint8_t)ss; sc.se = (uint8_t)se; sc.ah = (uint8_t)ah; sc.al = (uint8_t)al;
    for (int j = 0; j < ns; ++j) {
      int8_t* l = left[sc.comp[j]];
      if (ss != 0 && l[0] < 0) return fail(ST_OTHER);        // AC before the component's DC
      for (int k = ss; k <= se; ++k) {
        if (ah == 0 ? l[k] != -1 : l[k] != ah) return fail(ST_OTHER);
        l[k] = (int8_t)al;
      }
    }
    // the tables this scan decodes with, as they stand now
    sc.tab_first = (uint32_t)P.scan_tabs.size();
    if (ss != 0 || ah == 0) {
      for (int j = 0; j < ns; ++j) {
        const int slot = ss ? 4 + ta : td[j];
        int same = 0;
        while (same < j && td[same] != td[j]) ++same;
        if (same < j) { sc.tab[j] = sc.tab[same]; continue; }
        if (!P.h_set[slot]) return fail(ST_BAD_MARKER);
        HuffDec t;
        if (!build_huff_dec(P.bits[slot], P.vals[slot], t)) return fail(ST_BAD_HUFFMAN);
        if (ss == 0)
          for (int i = 0; i < 256; ++i)
            if (P.vals[slot][i] > 15) return fail(ST_BAD_HUFFMAN);
        sc.tab[j] = sc.ntab++;
        P.scan_tabs.push_back(t);
      }
    }
    // its entropy-coded data
    sc.ri = P.ri;
    int uw, uh;
    scan_extent(g, sc, uw, uh);
    const uint64_t units = (uint64_t)uw * uh;
    sc.seg_first = (uint32_t)P.seg_start.size();
    size_t i = 0;
    int marker = cut_segments(d, len, pos + L, sc.ri, sc.ri ? (units + sc.ri - 1) / sc.ri : 1, P, i);
    if (marker < 0) return fail(marker);
    sc.nseg = (uint32_t)P.seg_start.size() - sc.seg_first;
    P.scans.push_back(sc);
    // what stands between two scans: tables and the restart interval of the next
    while (marker != 0xD9 && marker != 0xDA) {
      if (marker == 0xC4 || marker == 0xDB || marker == 0xDD || marker == 0xDC || marker == 0xFE || (marker >= 0xE0 && marker <= 0xEF)) {
        if (i + 2 > len) return fail(ST_PREMATURE_END);
        const size_t M = be16(d + i);
        if (M < 2) return fail(ST_BAD_MARKER);
        if (M > len - i) return fail(ST_PREMATURE_END);
        if (marker == 0xDC || marker == 0xDB) return fail(ST_OTHER);      // a quantisation table behind the first SOS is left to libjpeg
        if (marker == 0xC4) {
          const int32_t rc = read_dht(d + i + 2, M - 2, P);
          if (rc) return fail(rc);
        } else if (marker == 0xDD) {
          if (M != 4) return fail(ST_BAD_MARKER);
          P.ri = (int)be16(d + i + 2);
        }
        i += M;
        if (i + 2 > len) return fail(ST_PREMATURE_END);
        if (d[i] != 0xFF) return fail(ST_BAD_MARKER);
        while (i + 1 < len && d[i + 1] == 0xFF) ++i;
        if (i + 2 > len) return fail(ST_PREMATURE_END);
        marker = d[i + 1];
        i += 2;
      } else {
        return fail(ST_BAD_MARKER);
      }
    }
    if (marker == 0xD9) break;
    pos = i;
  }
  P.ri = P.scans[0].ri;
  for (int c = 0; c < P.ncomp; ++c)
    for (int k = 0; k < 64; ++k)
      if (left[c][k] != 0) { P.incomplete = true; return fail(ST_OTHER); }
  P.status = ST_OK;
}

inline void build_tables(const Parsed& P, DecTables& T) {
  memset(&T, 0, sizeof(T));
  for (int t = 0; t < 4; ++t)
    if (P.q_set[t]) memcpy(T.q[t], P.q[t], sizeof(T.q[t]));
  for (int c = 0; c < P.ncomp && !P.progressive; ++c) {      // a progressive file's Huffman tables are its scans' (P.scan_tabs)
    build_huff_dec(P.bits[P.comp[c].td], P.vals[P.comp[c].td], T.huff[P.comp[c].td]);
    build_huff_dec(P.bits[4 + P.comp[c].ta], P.vals[4 + P.comp[c].ta], T.huff[4 + P.comp[c].ta]);
  }
}

// Stages C and D on the host: the coefficients of a parsed file -> out. st: what the entropy stage gave; returns the image's status.
inline int32_t finish_host(const Parsed& P, const DecGeom& g, const ScaledGeom& sg, const DecTables& T, const std::vector<int16_t>& coef, int32_t st,
                           int scale, int bgr, int apply_orientation, uint8_t* out) {
  std::vector<uint8_t> planes(scale == 1 ? g.plane_bytes : sg.plane_bytes);
  if (st == ST_OK && scale == 1) {
    for (int c = 0; c < g.ncomp; ++c)
      for (int by = 0; by < g.bh[c]; ++by)
        for (int bx = 0; bx < g.bw[c]; ++bx)
          if (!idct_block(coef.data() + ((size_t)g.blk_off[c] + (size_t)by * g.bw[c] + bx) * 64, T.q[P.comp[c].tq],
                          planes.data() + g.plane_off[c] + ((size_t)by * 8 * g.bw[c] + bx) * 8, (size_t)g.bw[c] * 8))
            st = ST_BAD_COEFFICIENT;
  }
  if (st == ST_OK && scale != 1) {
    for (int c = 0; c < g.ncomp; ++c)
      for (int by = 0; by < g.bh[c]; ++by)
        for (int gx = 0; gx < sg.gw[c]; ++gx)
          if (!idct_group(coef.data() + ((size_t)g.blk_off[c] + (size_t)by * g.bw[c]) * 64, gx, g.bw[c], sg.ss[c], T.q[P.comp[c].tq],
                          planes.data() + sg.plane_off[c] + (size_t)by * sg.ss[c] * sg.stride[c], (size_t)sg.stride[c]))
            st = ST_BAD_COEFFICIENT;
  }
  if (st == ST_OK && P.incomplete) st = ST_OTHER;
  if (st == ST_OK) {
    const int o = apply_orientation ? P.orientation : 1;
    const int ow = scale == 1 ? g.w : sg.ow, oh = scale == 1 ? g.h : sg.oh;
    for (int y = 0; y < oh; ++y)
      for (int x = 0; x < ow; ++x) {
        uint8_t rgb[3];
        if (scale == 1) pixel_rgb(planes.data(), g, x, y, rgb);
        else pixel_rgb_scaled(planes.data(), g, sg, x, y, rgb);
        uint8_t* p = out + oriented_index(o, ow, oh, x, y) * 3;
        p[0] = rgb[bgr ? 2 : 0]; p[1] = rgb[1]; p[2] = rgb[bgr ? 0 : 2];
      }
  }
  return st;
}

// The whole decode of one parsed file on the host, stage by stage as the kernels run it. buf: the file copied into a 16-byte aligned
// buffer padded to a multiple of 16 bytes. scale: 1, 2, 4 or 8, which the caller has checked. out:
// [oh][ow][3] with (oh, ow) = (ceil(height / scale), ceil(width / scale)), exchanged for orientations 5 .. 8 when apply_orientation.
// Returns the status; out is written only for 0. An incomplete progression has its scans run and its blocks transformed all the same, so
// that a stream that is corrupt as well is reported as that; it keeps ST_OTHER when nothing is found.
inline int32_t decode_host_scaled(const Parsed& P, const uint8_t* buf, int scale, int bgr, int apply_orientation, uint8_t* out) {
  if (P.status != ST_OK && !P.incomplete) return P.status;
  const DecGeom g = make_dec_geom(P.width, P.height, P.ncomp, P.hs, P.vs);
  const ScaledGeom sg = make_scaled_geom(g, scale);
  DecTables* T = new DecTables;
  build_tables(P, *T);
  std::vector<int16_t> coef((size_t)g.nblk * 64, 0);
  uint8_t td[3], ta[3];
  for (int c = 0; c < 3; ++c) { td[c] = P.comp[c].td; ta[c] = P.comp[c].ta; }
  const uint32_t mcus = (uint32_t)g.mw * g.mh, per = P.ri ? (uint32_t)P.ri : mcus;
  int32_t st = ST_OK;
  for (size_t n = 0; n < P.scans.size() && st == ST_OK; ++n) {      // file order: a later scan refines what an earlier one left
    const ScanDesc& sc = P.scans[n];
    int uw, uh;
    scan_extent(g, sc, uw, uh);
    const uint32_t units = (uint32_t)uw * uh, each = sc.ri ? (uint32_t)sc.ri : units;
    for (uint32_t k = 0; k < sc.nseg && st == ST_OK; ++k) {
      BitReader br;
      br.init(buf, P.seg_start[sc.seg_first + k], P.seg_end[sc.seg_first + k]);
      const uint32_t u0 = k * each;
      st = decode_scan_segment(br, g, sc, P.scan_tabs.data() + sc.tab_first, u0, units - u0 < each ? units - u0 : each, coef.data(), kNatural);
    }
  }
  for (size_t k = 0; k < P.seg_start.size() && st == ST_OK && !P.progressive; ++k) {
    BitReader br;
    br.init(buf, P.seg_start[k], P.seg_end[k]);
    const uint32_t m0 = (uint32_t)k * per;
    st = decode_segment(br, g, T->huff, td, ta, m0, mcus - m0 < per ? mcus - m0 : per, coef.data(), kNatural);
  }
  st = finish_host(P, g, sg, *T, coef, st, scale, bgr, apply_orientation, out);
  delete T;
  return st;
}

inline int32_t decode_host(const Parsed& P, const uint8_t* buf, int bgr, int apply_orientation, uint8_t* out) {
  return decode_host_scaled(P, buf, 1, bgr, apply_orientation, out);
}

// Steps 1 to 4 of the parallel decode over one segment with the lanes as loops, in the order of the kernels: every pass of a round reads
// what the round before left. rounds: the largest count so far. Returns 0 or an error of step 4.
inline int32_t decode_segment_parallel(const uint8_t* buf, uint32_t s0, uint32_t s1, uint32_t S, const DecGeom& g, const HuffDec* huff,
                                       const uint8_t* td, const uint8_t* ta, uint32_t mcu0, uint32_t nmcu, int16_t* coef, uint32_t& rounds) {
  const uint32_t n = sub_count(s1 - s0, S);
  std::vector<uint32_t> cur(n, SUB_INVALID), nxt(n, SUB_INVALID), entry(n, 0), first(n, 0);
  std::vector<int32_t> dc[3] = {std::vector<int32_t>(n, 0), std::vector<int32_t>(n, 0), std::vector<int32_t>(n, 0)};
  SubResult R;
  auto sync_pass = [&](uint32_t i, uint32_t e) {
    sub_pass<false>(buf, s0, s1, S, i, n, e, g, huff, td, ta, 0, nullptr, 0, 0, nullptr, nullptr, R);
    entry[i] = e; first[i] = R.nblk;
    for (int c = 0; c < 3; ++c) dc[c][i] = R.dc[c];
  };
  for (uint32_t i = 0; i + 1 < n; ++i) {                     // step 1
    sync_pass(i, 0);
    cur[i] = R.exit;
  }
  uint32_t ran = 0;
  for (bool changed = true; changed && ran < n; ++ran) {   // step 2
    changed = false;
    nxt[0] = cur[0];
    for (uint32_t i = 1; i + 1 < n; ++i) {
      if (cur[i - 1] == entry[i]) { nxt[i] = cur[i]; continue; }
      sync_pass(i, cur[i - 1]);
      nxt[i] = R.exit;
      changed |= nxt[i] != cur[i];
    }
    cur.swap(nxt);
  }
  if (ran > rounds) rounds = ran;
  uint32_t blocks = 0;                                       // step 3
  int32_t pred[3] = {0, 0, 0};
  for (uint32_t i = 0; i < n; ++i) {
    if (i) entry[i] = cur[i - 1];
    const uint32_t nb = i + 1 < n ? first[i] : 0;
    first[i] = blocks;
    blocks += nb;
    for (int c = 0; c < 3; ++c) {
      const int32_t d = i + 1 < n ? dc[c][i] : 0;
      dc[c][i] = pred[c];
      pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)d);
    }
  }
  int32_t err = 0;
  for (uint32_t i = 0; i < n; ++i) {                         // step 4
    const int32_t pin[3] = {dc[0][i], dc[1][i], dc[2][i]};
    sub_pass<true>(buf, s0, s1, S, i, n, entry[i], g, huff, td, ta, first[i], pin, mcu0, nmcu, coef, kNatural, R);
    if (R.err && !err) err = R.err;
  }
  return err;
}

struct ParallelStats { uint32_t segments = 0, subsequences = 0, rounds = 0, redone = 0; };

// decode_host for a baseline file with every segment of at least two subsequences of S bytes decoded in parallel and the others by
// decode_segment; an image in which either met an error is zeroed and decoded again as decode_host decodes it, so status and pixels are
// decode_host's for every file.
inline int32_t decode_host_parallel(const Parsed& P, const uint8_t* buf, uint32_t S, int bgr, int apply_orientation, uint8_t* out, ParallelStats& ps) {
  if (P.status != ST_OK || P.progressive) return decode_host(P, buf, bgr, apply_orientation, out);
  const DecGeom g = make_dec_geom(P.width, P.height, P.ncomp, P.hs, P.vs);
  const ScaledGeom sg = make_scaled_geom(g, 1);
  DecTables* T = new DecTables;
  build_tables(P, *T);
  std::vector<int16_t> coef((size_t)g.nblk * 64, 0);
  uint8_t td[3], ta[3];
  for (int c = 0; c < 3; ++c) { td[c] = P.comp[c].td; ta[c] = P.comp[c].ta; }
  const uint32_t mcus = (uint32_t)g.mw * g.mh, per = P.ri ? (uint32_t)P.ri : mcus;
  int32_t st = ST_OK, perr = 0;
  for (size_t k = 0; k < P.seg_start.size(); ++k) {
    const uint32_t m0 = (uint32_t)k * per, nm = mcus - m0 < per ? mcus - m0 : per, nsub = sub_count(P.seg_end[k] - P.seg_start[k], S);
    if (nsub >= 2) {
      ++ps.segments; ps.subsequences += nsub;
      const int32_t e = decode_segment_parallel(buf, P.seg_start[k], P.seg_end[k], S, g, T->huff, td, ta, m0, nm, coef.data(), ps.rounds);
      if (e && !perr) perr = e;
    } else if (st == ST_OK) {
      BitReader br;
      br.init(buf, P.seg_start[k], P.seg_end[k]);
      st = decode_segment(br, g, T->huff, td, ta, m0, nm, coef.data(), kNatural);
    }
  }
  if (perr || st != ST_OK) {                                 // whichever decoder met the error, as the kernels do
    ++ps.redone;
    std::fill(coef.begin(), coef.end(), (int16_t)0);
    st = ST_OK;
    for (size_t k = 0; k < P.seg_start.size() && st == ST_OK; ++k) {
      BitReader br;
      br.init(buf, P.seg_start[k], P.seg_end[k]);
      const uint32_t m0 = (uint32_t)k * per;
      st = decode_segment(br, g, T->huff, td, ta, m0, mcus - m0 < per ? mcus - m0 : per, coef.data(), kNatural);
    }
  }
  st = finish_host(P, g, sg, *T, coef, st, 1, bgr, apply_orientation, out);
  delete T;
  return st;
}
}  // namespace jpegdec
}  // namespace fe
