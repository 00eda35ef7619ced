// JPEG decode: file bytes in, a resident uint8 [n][h][w][3] batch out, the pixels Pillow gives for
// `ImageOps.exif_transpose(Image.open(f)).convert('RGB')` (reference utils/image_loading.py:100-106). The arithmetic lives in
// jpeg_dec_core.h; here are its stages over a batch of files that may differ in everything but their output size:
//   A host:    parse every file (markers, tables, EXIF orientation), cut its entropy data at the restart markers into segments, and put
//              descriptors, tables, segment offsets and the compressed bytes of the whole chunk into one pinned block: one upload
//   B entropy: a lane decodes one segment serially into zeroed int16 coefficient blocks; a workgroup is one wave holding up to 64
//              segments of ONE image, whose Huffman tables sit in LDS. A file without restart markers is one segment: one lane of its wave.
//              A progressive file (FE_JPEG_PROGRESSIVE) has one such pass per scan, over the segments and with the tables of that scan:
//              launch s runs scan s of every image that has one, and the stream keeps an image's scans in file order.
//              With FE_JPEG_FLAG_PARALLEL a baseline segment of at least two subsequences (SUB_BYTES raw bytes each) is decoded by one
//              lane per subsequence instead (jpeg_dec_core.h, "decoding inside one segment in parallel"): a workgroup per segment finds
//              every subsequence's entry state in rounds separated by barriers and sums block counts and DC differences, a second
//              launch decodes every subsequence from its entry into the same coefficient blocks. An image in which that launch met an
//              error is zeroed and decoded again by the serial kernel in the same stream, so statuses are the serial decoder's.
//   C idct:    one lane per block: dequantise, integer slow IDCT, 8 rows of 8 samples into the component's plane (padded to the block grid)
//   D colour:  one lane per 4 pixels of a row: triangle-filter upsampling, YCbCr -> RGB, store as RGB or BGR at the address the EXIF
//              orientation gives (all 8 cases; there is no transpose pass)
// A scaled decode (fe_jpeg_decode_scaled, scale 2 / 4 / 8: libjpeg's 1/scale, which Pillow's draft() asks for) shares A and B and has a
// stage C of its own: a block becomes 4 x 4, 2 x 2 or 1 x 1 samples (chroma up to twice the luma's size, jpeg_dec_core.h's table), the
// planes are laid out per component, and a lane takes one block, two 2 x 2 blocks or four 1 x 1 blocks so that it stores whole dwords.
// Stage D is the same kernel instantiated over that layout.
// A segment's error (bad code, data that ends early) and a block outside the range honest coefficients reach become the image's negative
// status by atomicMin; stage D leaves the slot of such an image untouched.
#include <chrono>

#include "engine.h"
#include "jpeg_dec_core.h"

namespace fe {

using namespace jpegdec;

namespace {

struct DevImage {
  uint64_t coef_off;                     // int16 elements from the chunk's coefficient base
  uint64_t plane_off;                    // bytes from the chunk's plane base
  uint32_t seg_first, nseg;              // this image's rows of the segment offset arrays
  int32_t w, h, ncomp, hs, vs, ri, orientation;
  int32_t slot;                          // image index in the destination
  uint8_t td[4], ta[4], tq[4];
  uint32_t scan_first, nscan;            // a progressive image: its rows of the scan descriptors, and nseg = 0
};

constexpr int JD_WAVE = 64;
constexpr int JD_THREADS = 256;

// MODE 0: every segment of every image. With FE_JPEG_FLAG_PARALLEL, MODE 1: the segments that are not decoded in parallel (par[row] == 0),
// and an image with an error is flagged in redo as the parallel kernels flag theirs; MODE 2, behind those: every segment of the flagged
// images, whose blocks jpegdec_redo_zero_kernel has zeroed. So with the flag every baseline image whose entropy stage reports an error
// has been decoded by this kernel alone, start to end, whichever kernel met the error first.
constexpr int ENT_ALL = 0, ENT_SERIAL_ONLY = 1, ENT_REDO = 2;

template <int MODE>
__global__ __launch_bounds__(JD_WAVE) void jpegdec_entropy_kernel(const DevImage* __restrict__ imgs, const DecTables* __restrict__ tabs,
                                                                  const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_end,
                                                                  const uint8_t* __restrict__ bytes, int16_t* __restrict__ coef,
                                                                  int32_t* __restrict__ status, const uint32_t* __restrict__ par, int32_t* redo) {
  __shared__ HuffDec H[8];
  __shared__ uint8_t nat[64];
  const DevImage im = imgs[blockIdx.x];
  if (blockIdx.y * JD_WAVE >= im.nseg) return;               // uniform over the wave
  if (MODE == ENT_REDO && !redo[blockIdx.x]) return;         // as well
  {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(tabs[blockIdx.x].huff);
    uint32_t* d = reinterpret_cast<uint32_t*>(H);
    for (int t = threadIdx.x; t < (int)(sizeof(H) / 4); t += JD_WAVE) d[t] = s[t];
    constexpr uint8_t order[64] = FE_JPEG_NATURAL_ORDER;
    nat[threadIdx.x] = order[threadIdx.x];
  }
  __syncthreads();
  const uint32_t k = blockIdx.y * JD_WAVE + threadIdx.x;
  if (k >= im.nseg) return;
  if (MODE == ENT_SERIAL_ONLY && par[im.seg_first + k]) return;
  const DecGeom g = make_dec_geom(im.w, im.h, im.ncomp, im.hs, im.vs);
  const uint32_t mcus = (uint32_t)g.mw * (uint32_t)g.mh, per = im.ri ? (uint32_t)im.ri : mcus;
  const uint32_t m0 = k * per;                               // nseg = ceil(mcus / per): m0 < mcus
  BitReader br;
  br.init(bytes, seg_start[im.seg_first + k], seg_end[im.seg_first + k]);
  const int rc = decode_segment(br, g, H, im.td, im.ta, m0, min(per, mcus - m0), coef + im.coef_off, nat);
  if (rc) atomicMin(status + blockIdx.x, rc);
  if (MODE == ENT_SERIAL_ONLY && rc) redo[blockIdx.x] = 1;
}
static_assert(sizeof(HuffDec) % 4 == 0 && offsetof(DecTables, huff) % 4 == 0, "the tables are copied by dwords");

// ---- FE_JPEG_FLAG_PARALLEL: one lane per subsequence of a segment (jpeg_dec_core.h sub_pass) --------------------------------------------
struct ParSeg {                          // a segment that is decoded in parallel
  uint32_t img, seg;                     // its image in the chunk, its row of the segment offset arrays
  uint32_t mcu0, nmcu;
  uint32_t sub_first, nsub;              // its rows of the subsequence arrays; sub_first is a multiple of 64, so a wave of the write kernel has one segment
};
// The subsequence arrays, each T = all rows of the chunk long, one behind the other in arena scratch: the exits of this round and of the
// one before, the entry each exit was decoded from, blocks completed / first block, and per component DC sum / entry prediction.
constexpr int SUB_ARRAYS = 7;

__device__ __forceinline__ void load_huff(HuffDec* H, const DecTables* tabs, int nthreads) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(tabs->huff);
  uint32_t* d = reinterpret_cast<uint32_t*>(H);
  for (int t = threadIdx.x; t < (int)(8 * sizeof(HuffDec) / 4); t += nthreads) d[t] = s[t];
}

// Steps 1 to 3 for one segment per workgroup. The lanes stride over the subsequences; a round reads the exits the round before wrote and
// writes the other array, so its result does not depend on the order of the lanes, and rounds are separated by the workgroup's barrier,
// which also tells every lane whether any exit changed. No lane waits for another workgroup. At most nsub rounds run (after round r the
// exits 0 .. r are the true ones), so what stands at the end is right whether or not a quiet round was seen. stats[0]: most rounds of any segment.
__global__ __launch_bounds__(JD_THREADS) void jpegdec_sub_sync_kernel(const DevImage* __restrict__ imgs, const DecTables* __restrict__ tabs,
                                                                      const ParSeg* __restrict__ segs, const uint32_t* __restrict__ seg_start,
                                                                      const uint32_t* __restrict__ seg_end, const uint8_t* __restrict__ bytes,
                                                                      uint32_t* sub, uint32_t T, int32_t* stats) {
  __shared__ HuffDec H[8];
  __shared__ uint32_t part[4][JD_THREADS];
  const ParSeg ps = segs[blockIdx.x];
  const DevImage im = imgs[ps.img];
  load_huff(H, tabs + ps.img, JD_THREADS);
  __syncthreads();
  const DecGeom g = make_dec_geom(im.w, im.h, im.ncomp, im.hs, im.vs);
  const uint32_t s0 = seg_start[ps.seg], s1 = seg_end[ps.seg], n = ps.nsub, tid = threadIdx.x;
  uint32_t* cur = sub + ps.sub_first;
  uint32_t* nxt = cur + T;
  uint32_t* entry = sub + ps.sub_first + 2 * (size_t)T;
  uint32_t* first = entry + T;
  uint32_t* dc = first + T;              // [c * T + i]
  SubResult R;
  auto pass = [&](uint32_t i, uint32_t e) {
    sub_pass<false>(bytes, s0, s1, SUB_BYTES, i, n, e, g, H, im.td, im.ta, 0, nullptr, 0, 0, nullptr, nullptr, R);
    entry[i] = e; first[i] = R.nblk;
    for (int c = 0; c < 3; ++c) dc[c * (size_t)T + i] = (uint32_t)R.dc[c];
  };
  for (uint32_t i = tid; i + 1 < n; i += JD_THREADS) {       // step 1
    pass(i, 0);
    cur[i] = R.exit;
  }
  __syncthreads();
  uint32_t rounds = 0;
  for (uint32_t r = 0; r < n; ++r) {                         // step 2
    int changed = 0;
    for (uint32_t i = tid; i + 1 < n; i += JD_THREADS) {
      const uint32_t e = i ? cur[i - 1] : 0u;
      if (e == entry[i]) { nxt[i] = cur[i]; continue; }
      pass(i, e);
      nxt[i] = R.exit;
      changed |= R.exit != cur[i];
    }
    uint32_t* t = cur; cur = nxt; nxt = t;
    ++rounds;
    __syncthreads();                                         // the exits of this round, in global memory, before any lane of the next reads them
    if (!__syncthreads_or(changed)) break;
  }
  if (tid == 0) atomicMax(stats, (int32_t)rounds);
  // step 3: lane t sums rows t * per .. of the four quantities, the lanes' sums are scanned in LDS, and every lane writes its rows' offsets
  const uint32_t per = (n + JD_THREADS - 1) / JD_THREADS, lo = min(n, tid * per), hi = min(n, lo + per);
  uint32_t sum[4] = {0, 0, 0, 0};
  for (uint32_t i = lo; i < hi && i + 1 < n; ++i) {
    sum[0] += first[i];
    for (int c = 0; c < 3; ++c) sum[1 + c] += dc[c * (size_t)T + i];
  }
  for (int q = 0; q < 4; ++q) part[q][tid] = sum[q];
  __syncthreads();
  for (uint32_t d = 1; d < JD_THREADS; d <<= 1) {            // inclusive scan over the lanes
    uint32_t add[4];
    for (int q = 0; q < 4; ++q) add[q] = tid >= d ? part[q][tid - d] : 0u;
    __syncthreads();
    for (int q = 0; q < 4; ++q) part[q][tid] += add[q];
    __syncthreads();
  }
  uint32_t run[4];
  for (int q = 0; q < 4; ++q) run[q] = part[q][tid] - sum[q];
  for (uint32_t i = lo; i < hi; ++i) {
    const bool counted = i + 1 < n;                          // the last subsequence was not decoded: its rows hold nothing
    const uint32_t nb = counted ? first[i] : 0u;
    first[i] = run[0];
    run[0] += nb;
    for (int c = 0; c < 3; ++c) {
      const uint32_t v = counted ? dc[c * (size_t)T + i] : 0u;
      dc[c * (size_t)T + i] = run[1 + c];
      run[1 + c] += v;
    }
    entry[i] = i ? cur[i - 1] : 0u;
  }
}

// Step 4: a lane per subsequence, a wave per 64 rows of one segment (wave_seg[wave]: its ParSeg), the image's tables in LDS. A lane that
// meets an error flags its image in redo; statuses are left to the serial kernel that decodes such an image again.
__global__ __launch_bounds__(JD_WAVE) void jpegdec_sub_write_kernel(const DevImage* __restrict__ imgs, const DecTables* __restrict__ tabs,
                                                                    const ParSeg* __restrict__ segs, const uint32_t* __restrict__ wave_seg,
                                                                    const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_end,
                                                                    const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ sub, uint32_t T,
                                                                    int16_t* __restrict__ coef, int32_t* __restrict__ redo) {
  __shared__ HuffDec H[8];
  __shared__ uint8_t nat[64];
  const ParSeg ps = segs[wave_seg[blockIdx.x]];
  const DevImage im = imgs[ps.img];
  if (blockIdx.x * JD_WAVE - ps.sub_first >= ps.nsub) return;      // uniform over the wave; cannot happen by the way rows are handed out
  load_huff(H, tabs + ps.img, JD_WAVE);
  {
    constexpr uint8_t order[64] = FE_JPEG_NATURAL_ORDER;
    nat[threadIdx.x] = order[threadIdx.x];
  }
  __syncthreads();
  const uint32_t row = blockIdx.x * JD_WAVE + threadIdx.x, i = row - ps.sub_first;
  if (i >= ps.nsub) return;
  const DecGeom g = make_dec_geom(im.w, im.h, im.ncomp, im.hs, im.vs);
  const int32_t pred[3] = {(int32_t)sub[4 * (size_t)T + row], (int32_t)sub[5 * (size_t)T + row], (int32_t)sub[6 * (size_t)T + row]};
  SubResult R;
  sub_pass<true>(bytes, seg_start[ps.seg], seg_end[ps.seg], SUB_BYTES, i, ps.nsub, sub[2 * (size_t)T + row], g, H, im.td, im.ta, sub[3 * (size_t)T + row], pred,
                 ps.mcu0, ps.nmcu, coef + im.coef_off, nat, R);
  if (R.err) redo[ps.img] = 1;
}

// The coefficient blocks of every image flagged in redo back to zero; stats[1]: how many there were
__global__ __launch_bounds__(JD_THREADS) void jpegdec_redo_zero_kernel(const DevImage* __restrict__ imgs, const int32_t* __restrict__ redo,
                                                                       int16_t* __restrict__ coef, int32_t* stats) {
  if (!redo[blockIdx.y]) return;
  const DevImage im = imgs[blockIdx.y];
  const DecGeom g = make_dec_geom(im.w, im.h, im.ncomp, im.hs, im.vs);
  uint4* p = reinterpret_cast<uint4*>(coef + im.coef_off);   // 128 bytes per block, 16-byte aligned
  const size_t nv = (size_t)g.nblk * 8;
  for (size_t v = (size_t)blockIdx.x * JD_THREADS + threadIdx.x; v < nv; v += (size_t)gridDim.x * JD_THREADS) p[v] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(stats + 1, 1);
}

// Scan `scan` of every progressive image of the chunk that has that many: the shape of the kernel above with the scan's tables (at most
// one per component) and the scan's segments. It updates the coefficients earlier scans left, so the launches of a chunk follow each
// other on one stream in scan order; within a launch two lanes never share a block.
__global__ __launch_bounds__(JD_WAVE) void jpegdec_scan_entropy_kernel(const DevImage* __restrict__ imgs, const ScanDesc* __restrict__ scans,
                                                                       const HuffDec* __restrict__ pool, const uint32_t* __restrict__ seg_start,
                                                                       const uint32_t* __restrict__ seg_end, const uint8_t* __restrict__ bytes,
                                                                       int16_t* __restrict__ coef, int32_t* __restrict__ status, uint32_t scan) {
  __shared__ HuffDec H[3];
  __shared__ uint8_t nat[64];
  const DevImage im = imgs[blockIdx.x];
  if (scan >= im.nscan) return;                              // uniform over the wave, as are the next two
  const ScanDesc sc = scans[im.scan_first + scan];
  if (blockIdx.y * JD_WAVE >= sc.nseg) return;
  {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(pool + sc.tab_first);
    uint32_t* d = reinterpret_cast<uint32_t*>(H);
    const int nw = (int)(min((uint32_t)sc.ntab, 3u) * (sizeof(HuffDec) / 4));
    for (int t = threadIdx.x; t < nw; t += JD_WAVE) d[t] = s[t];
    constexpr uint8_t order[64] = FE_JPEG_NATURAL_ORDER;
    nat[threadIdx.x] = order[threadIdx.x];
  }
  __syncthreads();
  const uint32_t k = blockIdx.y * JD_WAVE + threadIdx.x;
  if (k >= sc.nseg) return;
  const DecGeom g = make_dec_geom(im.w, im.h, im.ncomp, im.hs, im.vs);
  int uw, uh;
  scan_extent(g, sc, uw, uh);
  const uint32_t units = (uint32_t)uw * (uint32_t)uh, per = sc.ri ? (uint32_t)sc.ri : units;
  const uint32_t u0 = k * per;                               // nseg = ceil(units / per): u0 < units
  BitReader br;
  br.init(bytes, seg_start[sc.seg_first + k], seg_end[sc.seg_first + k]);
  const int rc = decode_scan_segment(br, g, sc, H, u0, min(per, units - u0), coef + im.coef_off, nat);
  if (rc) atomicMin(status + blockIdx.x, rc);
}
static_assert(sizeof(ScanDesc) % 4 == 0, "scan descriptors are read as an array in the upload block");

__global__ __launch_bounds__(JD_THREADS) void jpegdec_idct_kernel(const DevImage* __restrict__ imgs, const DecTables* __restrict__ tabs,
                                                                  const int16_t* __restrict__ coef, uint8_t* __restrict__ planes,
                                                                  int32_t* __restrict__ status) {
  __shared__ uint16_t q[4][64];
  const DevImage im = imgs[blockIdx.y];
  const DecGeom g = make_dec_geom(im.w, im.h, im.ncomp, im.hs, im.vs);
  if (blockIdx.x * JD_THREADS >= g.nblk) return;             // uniform over the workgroup
  (&q[0][0])[threadIdx.x] = (&tabs[blockIdx.y].q[0][0])[threadIdx.x];
  __syncthreads();
  const uint32_t b = blockIdx.x * JD_THREADS + threadIdx.x;
  if (b >= g.nblk) return;
  const int c = (g.ncomp == 3 && b >= g.blk_off[1]) ? (b >= g.blk_off[2] ? 2 : 1) : 0;
  const uint32_t lb = b - g.blk_off[c];
  const uint32_t by = lb / (uint32_t)g.bw[c], bx = lb % (uint32_t)g.bw[c];
  int16_t blk[64];
  const uint4* src = reinterpret_cast<const uint4*>(coef + im.coef_off + (size_t)b * 64);      // 128 bytes per block, 16-byte aligned
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const uint4 u = src[v];
    const uint32_t wds[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { blk[8 * v + 2 * j] = (int16_t)(wds[j] & 0xFFFFu); blk[8 * v + 2 * j + 1] = (int16_t)(wds[j] >> 16); }
  }
  const size_t stride = (size_t)g.bw[c] * 8;
  if (!idct_block(blk, q[im.tq[c] & 3], planes + im.plane_off + g.plane_off[c] + ((size_t)by * 8 * g.bw[c] + bx) * 8, stride))
    atomicMin(status + blockIdx.y, (int32_t)ST_BAD_COEFFICIENT);
}

// Stage C of a scaled decode. Work items are numbered per component (ScaledGeom.grp_off); item (by, gx) of a component transforms blocks
// gx * pack .. gx * pack + pack - 1 of block row by into the rows by * ss .. of that component's plane (idct_group).
__global__ __launch_bounds__(JD_THREADS) void jpegdec_idct_scaled_kernel(const DevImage* __restrict__ imgs, const DecTables* __restrict__ tabs,
                                                                         const int16_t* __restrict__ coef, uint8_t* __restrict__ planes,
                                                                         int32_t* __restrict__ status, int scale) {
  __shared__ uint16_t q[4][64];
  const DevImage im = imgs[blockIdx.y];
  const DecGeom g = make_dec_geom(im.w, im.h, im.ncomp, im.hs, im.vs);
  const ScaledGeom sg = make_scaled_geom(g, scale);
  if (blockIdx.x * JD_THREADS >= sg.grp_off[3]) return;      // uniform over the workgroup
  (&q[0][0])[threadIdx.x] = (&tabs[blockIdx.y].q[0][0])[threadIdx.x];
  __syncthreads();
  const uint32_t i = blockIdx.x * JD_THREADS + threadIdx.x;
  if (i >= sg.grp_off[3]) return;
  const int c = (g.ncomp == 3 && i >= sg.grp_off[1]) ? (i >= sg.grp_off[2] ? 2 : 1) : 0;
  const uint32_t li = i - sg.grp_off[c];
  const uint32_t by = li / (uint32_t)sg.gw[c], gx = li % (uint32_t)sg.gw[c];
  const int16_t* row = coef + im.coef_off + ((size_t)g.blk_off[c] + (size_t)by * g.bw[c]) * 64;
  uint8_t* out = planes + im.plane_off + sg.plane_off[c] + (size_t)by * sg.ss[c] * sg.stride[c];
  if (!idct_group(row, (int)gx, g.bw[c], sg.ss[c], q[im.tq[c] & 3], out, (size_t)sg.stride[c]))
    atomicMin(status + blockIdx.y, (int32_t)ST_BAD_COEFFICIENT);
}

// dst [slots][oh][ow][3]. A lane takes pixels 4 t .. 4 t + 3 of a source row. SCALED: the source is the ceil(w / scale) x ceil(h / scale)
// image in ScaledGeom's planes; otherwise scale is 1 and unused. Where the destination keeps the source's row direction
// (orientation 1 or 4) and rows are a whole number of dwords, the 12 bytes go out as three dwords; otherwise byte by byte.
template <bool SCALED>
__global__ __launch_bounds__(JD_THREADS) void jpegdec_colour_kernel(const DevImage* __restrict__ imgs, const uint8_t* __restrict__ planes,
                                                                    const int32_t* __restrict__ status, uint8_t* __restrict__ dst, int oh, int ow,
                                                                    int bgr, int apply_orientation, int dst_aligned, int scale) {
  const DevImage im = imgs[blockIdx.y];
  if (status[blockIdx.y] != 0) return;
  const int sw = SCALED ? (im.w + scale - 1) / scale : im.w, sh = SCALED ? (im.h + scale - 1) / scale : im.h;
  const int w4 = (sw + 3) >> 2;
  const uint32_t i = blockIdx.x * JD_THREADS + threadIdx.x;
  if (i >= (uint32_t)w4 * (uint32_t)sh) return;
  const int y = (int)(i / (uint32_t)w4), x0 = (int)(i % (uint32_t)w4) * 4;
  const DecGeom g = make_dec_geom(im.w, im.h, im.ncomp, im.hs, im.vs);
  ScaledGeom sg;
  if constexpr (SCALED) sg = make_scaled_geom(g, scale);
  const uint8_t* pl = planes + im.plane_off;
  const int o = apply_orientation ? im.orientation : 1;
  uint8_t* out = dst + (size_t)im.slot * oh * ow * 3;
  const int ir = bgr ? 2 : 0, ib = bgr ? 0 : 2;
  uint8_t px[12];
  const int nx = min(4, sw - x0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint8_t rgb[3] = {0, 0, 0};
    if (j < nx) {
      if constexpr (SCALED) pixel_rgb_scaled(pl, g, sg, x0 + j, y, rgb);
      else pixel_rgb(pl, g, x0 + j, y, rgb);
    }
    px[3 * j + ir] = rgb[0]; px[3 * j + 1] = rgb[1]; px[3 * j + ib] = rgb[2];
  }
  if ((o == 1 || o == 4) && dst_aligned && (sw & 3) == 0) {
    uint32_t* p = reinterpret_cast<uint32_t*>(out + oriented_index(o, sw, sh, x0, y) * 3);
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = px[4 * j] | ((uint32_t)px[4 * j + 1] << 8) | ((uint32_t)px[4 * j + 2] << 16) | ((uint32_t)px[4 * j + 3] << 24);
  } else {
    for (int j = 0; j < nx; ++j) {
      uint8_t* p = out + oriented_index(o, sw, sh, x0 + j, y) * 3;
      p[0] = px[3 * j]; p[1] = px[3 * j + 1]; p[2] = px[3 * j + 2];
    }
  }
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct StageTimer {                      // with fe_profile_enable: one record per stage
  Ctx& c;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  explicit StageTimer(Ctx& ctx) : c(ctx) {
    if (c.profile) { FE_HIP(hipEventCreate(&e0)); FE_HIP(hipEventCreate(&e1)); }
  }
  ~StageTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  void begin() { if (c.profile) FE_HIP(hipEventRecord(e0, c.stream)); }
  void end(const char* name, double bytes) {
    if (!c.profile) return;
    FE_HIP(hipEventRecord(e1, c.stream));
    FE_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FE_HIP(hipEventElapsedTime(&ms, e0, e1));
    c.timings.push_back({name, 0.0, bytes, ms});
  }
};

}  // namespace

void jpeg_probe(const uint8_t* data, size_t len, int flags, int32_t out[10]) {
  Parsed P;
  parse(data, len, P, flags);
  out[8] = P.progressive ? 1 : 0; out[9] = (int32_t)P.scans.size();
  out[0] = P.width; out[1] = P.height; out[2] = P.ncomp; out[3] = P.hs; out[4] = P.vs; out[5] = P.ri; out[6] = P.orientation; out[7] = P.status;
}

void jpeg_scaled_size(int h, int w, int scale, int* sh, int* sw) {
  *sh = (h + scale - 1) / scale; *sw = (w + scale - 1) / scale;
}

// dst: [n][h][w][3] on the device or on the host; status: host [n]. scale: 1, 2, 4 or 8; h, w are the scaled size. See fe_jpeg_decode_scaled.
void jpeg_decode_batch(Ctx& c, const uint8_t* const* data, const size_t* len, int n, int h, int w, int scale, int bgr, int apply_orientation,
                       int dst_on_device, int flags, uint8_t* dst, int32_t* status) {
  FE_CHECK(n > 0 && h > 0 && w > 0 && h <= 65535 && w <= 65535, "jpeg_decode: bad shape %d x %d x %d", n, h, w);
  FE_CHECK(scale == 1 || scale == 2 || scale == 4 || scale == 8, "jpeg_decode: scale %d (1, 2, 4, 8)", scale);
  const bool par = (flags & FLAG_PARALLEL) != 0;
  for (int k = 0; k < 4; ++k) c.jpeg_entropy_stats[k] = 0;
  const auto t_parse = std::chrono::steady_clock::now();
  std::vector<Parsed> parsed((size_t)n);
  std::vector<int> todo;
  for (int i = 0; i < n; ++i) {
    Parsed& P = parsed[i];
    if (!data[i]) { P.status = ST_BAD_MARKER; status[i] = P.status; continue; }
    parse(data[i], len[i], P, flags);
    if (P.status == ST_OK || P.incomplete) {
      const bool swap = apply_orientation && P.orientation >= 5;
      int sh, sw;
      jpeg_scaled_size(P.height, P.width, scale, &sh, &sw);
      if ((swap ? sw : sh) != h || (swap ? sh : sw) != w) { P.status = ST_BAD_DIMENSIONS; P.incomplete = false; }
    }
    status[i] = P.status;
    if (P.status == ST_OK || P.incomplete) todo.push_back(i);      // an incomplete progression has its scans run: it may be corrupt as well
  }
  if (c.profile)
    c.timings.push_back({"jpeg_decode A: parse (host)", 0.0, 0.0,
                         std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_parse).count()});
  const size_t out_b = (size_t)h * w * 3;
  auto need = [&](const Parsed& P) {      // arena bytes of one image, alignment slack included
    const DecGeom g = make_dec_geom(P.width, P.height, P.ncomp, P.hs, P.vs);
    const size_t bytes = (size_t)(P.seg_end.back() - P.seg_start.front());
    size_t sub = 0;                       // FE_JPEG_FLAG_PARALLEL: descriptors and subsequence arrays of the segments decoded in parallel
    if (par && !P.progressive) {
      sub = P.seg_start.size() * 4 + 4;
      for (size_t s = 0; s < P.seg_start.size(); ++s) {
        const size_t ns = sub_count(P.seg_end[s] - P.seg_start[s], SUB_BYTES), rows = (ns + JD_WAVE - 1) / JD_WAVE * JD_WAVE;
        if (ns >= 2) sub += sizeof(ParSeg) + rows / JD_WAVE * 4 + rows * SUB_ARRAYS * 4;
      }
    }
    return sub + (size_t)g.nblk * 128 + up256(g.plane_bytes) + up256(bytes + 16) + sizeof(DevImage) + sizeof(DecTables) + P.seg_start.size() * 8 + 4 +
           P.scans.size() * sizeof(ScanDesc) + P.scan_tabs.size() * sizeof(HuffDec) + (dst_on_device ? 0 : out_b) + 64;
  };
  const size_t budget = c.arena.capacity() - c.arena.capacity() / 8;
  StageTimer tm(c);
  std::vector<int32_t> st_host;
  for (size_t first = 0; first < todo.size();) {
    // the images of this chunk: as many as the workspace holds
    size_t used = 17 * 256, last = first;                    // alignment slack of the upload block's regions and the arena allocations
    uint64_t comp_bytes = 0;
    while (last < todo.size() && last - first < 4096) {
      const Parsed& P = parsed[todo[last]];
      const size_t nb = need(P);
      if (last > first && (used + nb > budget || comp_bytes + (P.seg_end.back() - P.seg_start.front()) > 0xE0000000ull)) break;
      FE_CHECK(used + nb <= budget, "jpeg_decode: one %d x %d image needs %zu bytes of workspace, the arena holds %zu", P.width, P.height, nb, budget);
      used += nb; comp_bytes += P.seg_end.back() - P.seg_start.front();
      ++last;
    }
    const int nd = (int)(last - first);
    size_t nseg = 0, nscan = 0, npool = 0, npar = 0, nrow = 0;      // npar, nrow: segments decoded in parallel and their subsequence rows
    for (size_t k = first; k < last; ++k) {
      const Parsed& P = parsed[todo[k]];
      nseg += P.seg_start.size(); nscan += P.scans.size(); npool += P.scan_tabs.size();
      for (size_t s = 0; par && !P.progressive && s < P.seg_start.size(); ++s) {
        const size_t ns = sub_count(P.seg_end[s] - P.seg_start[s], SUB_BYTES);
        if (ns >= 2) { ++npar; nrow += (ns + JD_WAVE - 1) / JD_WAVE * JD_WAVE; }
      }
    }
    FE_CHECK(nrow < 0x7FFFFFC0ull, "jpeg_decode: too many subsequences in a chunk");
    // ---- stage A: one block of host memory -> one upload
    const size_t o_img = 0, o_tab = up256(o_img + (size_t)nd * sizeof(DevImage)), o_s0 = up256(o_tab + (size_t)nd * sizeof(DecTables)),
                 o_s1 = up256(o_s0 + nseg * 4), o_scan = up256(o_s1 + nseg * 4), o_pool = up256(o_scan + nscan * sizeof(ScanDesc)),
                 o_st0 = up256(o_pool + npool * sizeof(HuffDec)), o_par = up256(o_st0 + (size_t)(nd + 2) * 4),
                 o_wave = up256(o_par + npar * sizeof(ParSeg)), o_kind = up256(o_wave + nrow / JD_WAVE * 4),
                 o_bytes = up256(o_kind + (par ? nseg * 4 : 0));
    size_t blob = o_bytes;
    for (size_t k = first; k < last; ++k) blob += ((size_t)(parsed[todo[k]].seg_end.back() - parsed[todo[k]].seg_start.front()) + 15) & ~(size_t)15;
    blob += 16;                                              // 16-byte loads at the tail stay inside
    FE_CHECK(blob - o_bytes < 0xFFFFFFF0ull, "jpeg_decode: compressed bytes of a chunk exceed 32-bit offsets");
    if (blob > c.jpegdec_stage_cap) {
      if (c.jpegdec_stage) (void)hipHostFree(c.jpegdec_stage);
      c.jpegdec_stage = nullptr; c.jpegdec_stage_cap = 0;
      const size_t cap = blob + blob / 4;
      FE_HIP(hipHostMalloc(&c.jpegdec_stage, cap, hipHostMallocDefault));
      c.jpegdec_stage_cap = cap;
    }
    uint8_t* hb = (uint8_t*)c.jpegdec_stage;
    DevImage* h_img = (DevImage*)(hb + o_img);
    DecTables* h_tab = (DecTables*)(hb + o_tab);
    uint32_t* h_s0 = (uint32_t*)(hb + o_s0);
    uint32_t* h_s1 = (uint32_t*)(hb + o_s1);
    ScanDesc* h_scan = (ScanDesc*)(hb + o_scan);
    HuffDec* h_pool = (HuffDec*)(hb + o_pool);
    int32_t* h_st0 = (int32_t*)(hb + o_st0);                 // what each image's status starts from; behind them the two device counters
    h_st0[nd] = h_st0[nd + 1] = 0;
    ParSeg* h_par = (ParSeg*)(hb + o_par);
    uint32_t* h_wave = (uint32_t*)(hb + o_wave);             // [row / 64]: the ParSeg those rows belong to
    uint32_t* h_kind = (uint32_t*)(hb + o_kind);             // [segment row]: 1 when it is decoded in parallel
    size_t par_at = 0, row_at = 0;
    size_t coef_el = 0, plane_b = 0, seg_at = 0, byte_at = 0, scan_at = 0, pool_at = 0;
    uint32_t max_groups = 0, max_blk = 1;                    // max_blk: work items of stage C, which are blocks at scale 1
    uint32_t scan_groups[MAX_SCANS] = {};                    // [s]: workgroups per image of the launch for scan s, 0: no image has one
    bool held_back = false;
    for (int k = 0; k < nd; ++k) {
      const int src = todo[first + k];
      const Parsed& P = parsed[src];
      const DecGeom g = make_dec_geom(P.width, P.height, P.ncomp, P.hs, P.vs);
      DevImage& D = h_img[k];
      memset(&D, 0, sizeof(D));
      D.coef_off = coef_el; D.plane_off = plane_b;
      D.seg_first = (uint32_t)seg_at; D.nseg = (uint32_t)P.seg_start.size();
      D.w = P.width; D.h = P.height; D.ncomp = P.ncomp; D.hs = P.hs; D.vs = P.vs; D.ri = P.ri; D.orientation = P.orientation;
      D.slot = dst_on_device ? src : k;
      for (int cc = 0; cc < P.ncomp; ++cc) { D.td[cc] = P.comp[cc].td; D.ta[cc] = P.comp[cc].ta; D.tq[cc] = P.comp[cc].tq; }
      build_tables(P, h_tab[k]);
      h_st0[k] = P.incomplete ? (int32_t)ST_OTHER : (int32_t)ST_OK;
      held_back |= P.incomplete;
      if (P.progressive) {
        D.nseg = 0;                                          // nothing for the baseline kernel
        D.scan_first = (uint32_t)scan_at; D.nscan = (uint32_t)P.scans.size();
        for (size_t s = 0; s < P.scans.size(); ++s) {
          ScanDesc& S = h_scan[scan_at + s];
          S = P.scans[s];
          S.seg_first += (uint32_t)seg_at; S.tab_first += (uint32_t)pool_at;
          scan_groups[s] = std::max(scan_groups[s], (S.nseg + JD_WAVE - 1) / JD_WAVE);
        }
        if (!P.scan_tabs.empty()) memcpy(h_pool + pool_at, P.scan_tabs.data(), P.scan_tabs.size() * sizeof(HuffDec));
        scan_at += P.scans.size(); pool_at += P.scan_tabs.size();
      }
      const uint32_t s0 = P.seg_start.front(), nbytes = P.seg_end.back() - s0;
      memcpy(hb + o_bytes + byte_at, data[src] + s0, nbytes);
      const uint32_t mcus = (uint32_t)g.mw * (uint32_t)g.mh, per = P.ri ? (uint32_t)P.ri : mcus;
      for (size_t s = 0; s < P.seg_start.size(); ++s) {
        h_s0[seg_at + s] = (uint32_t)byte_at + (P.seg_start[s] - s0);
        h_s1[seg_at + s] = (uint32_t)byte_at + (P.seg_end[s] - s0);
        if (!par) continue;
        const uint32_t ns = sub_count(P.seg_end[s] - P.seg_start[s], SUB_BYTES);
        h_kind[seg_at + s] = (par && !P.progressive && ns >= 2) ? 1u : 0u;
        if (!h_kind[seg_at + s]) continue;
        const uint32_t m0 = (uint32_t)s * per;                 // parse() took the file with ceil(mcus / per) segments: m0 < mcus
        h_par[par_at] = ParSeg{(uint32_t)k, (uint32_t)(seg_at + s), m0, std::min(per, mcus - m0), (uint32_t)row_at, ns};
        const size_t rows = ((size_t)ns + JD_WAVE - 1) / JD_WAVE * JD_WAVE;
        for (size_t wv = 0; wv < rows / JD_WAVE; ++wv) h_wave[row_at / JD_WAVE + wv] = (uint32_t)par_at;
        ++par_at; row_at += rows;
        c.jpeg_entropy_stats[0] += 1; c.jpeg_entropy_stats[1] += (int32_t)ns;
      }
      const size_t padded = ((size_t)nbytes + 15) & ~(size_t)15;
      memset(hb + o_bytes + byte_at + nbytes, 0, padded - nbytes);
      byte_at += padded;
      seg_at += P.seg_start.size();
      coef_el += (size_t)g.nblk * 64;
      plane_b += up256(g.plane_bytes);
      max_groups = std::max(max_groups, (D.nseg + JD_WAVE - 1) / JD_WAVE);
      max_blk = std::max(max_blk, scale == 1 ? g.nblk : make_scaled_geom(g, scale).grp_off[3]);
    }
    memset(hb + o_bytes + byte_at, 0, 16);
    FE_CHECK(max_groups <= 65535, "jpeg_decode: an image has too many restart intervals");
    for (int s = 0; s < MAX_SCANS; ++s) FE_CHECK(scan_groups[s] <= 65535, "jpeg_decode: a scan has too many restart intervals");
    c.arena.reset();
    uint8_t* d_blob = (uint8_t*)c.arena.alloc(blob);
    int32_t* d_status = (int32_t*)c.arena.alloc((size_t)(nd + 2) * 4);      // [nd], [nd + 1]: most rounds of a segment, images decoded again
    int32_t* d_redo = par ? (int32_t*)c.arena.alloc((size_t)nd * 4) : nullptr;
    uint32_t* d_sub = npar ? (uint32_t*)c.arena.alloc(nrow * SUB_ARRAYS * 4) : nullptr;
    int16_t* d_coef = (int16_t*)c.arena.alloc(coef_el * 2);
    uint8_t* d_planes = (uint8_t*)c.arena.alloc(plane_b);
    uint8_t* d_out = dst_on_device ? dst : (uint8_t*)c.arena.alloc((size_t)nd * out_b);
    tm.begin();
    FE_HIP(hipMemcpyAsync(d_blob, hb, blob, hipMemcpyHostToDevice, c.stream));
    tm.end("jpeg_decode A: upload", (double)blob);
    const DevImage* d_img = (const DevImage*)(d_blob + o_img);
    const DecTables* d_tab = (const DecTables*)(d_blob + o_tab);
    tm.begin();
    if (held_back) FE_HIP(hipMemcpyAsync(d_status, d_blob + o_st0, (size_t)(nd + 2) * 4, hipMemcpyDeviceToDevice, c.stream));
    else FE_HIP(hipMemsetAsync(d_status, 0, (size_t)(nd + 2) * 4, c.stream));
    FE_HIP(hipMemsetAsync(d_coef, 0, coef_el * 2, c.stream));
    const uint32_t* d_s0 = (const uint32_t*)(d_blob + o_s0);
    const uint32_t* d_s1 = (const uint32_t*)(d_blob + o_s1);
    const uint8_t* d_bytes = (const uint8_t*)(d_blob + o_bytes);
    if (!par || !max_groups) {
      if (max_groups)
        hipLaunchKernelGGL(jpegdec_entropy_kernel<ENT_ALL>, dim3((unsigned)nd, max_groups), dim3(JD_WAVE), 0, c.stream, d_img, d_tab, d_s0, d_s1, d_bytes,
                           d_coef, d_status, (const uint32_t*)nullptr, (int32_t*)nullptr);
    } else {
      const ParSeg* d_par = (const ParSeg*)(d_blob + o_par);
      const uint32_t* d_kind = (const uint32_t*)(d_blob + o_kind);
      FE_HIP(hipMemsetAsync(d_redo, 0, (size_t)nd * 4, c.stream));
      hipLaunchKernelGGL(jpegdec_entropy_kernel<ENT_SERIAL_ONLY>, dim3((unsigned)nd, max_groups), dim3(JD_WAVE), 0, c.stream, d_img, d_tab, d_s0, d_s1,
                         d_bytes, d_coef, d_status, d_kind, d_redo);
      if (npar) {
        hipLaunchKernelGGL(jpegdec_sub_sync_kernel, dim3((unsigned)npar), dim3(JD_THREADS), 0, c.stream, d_img, d_tab, d_par, d_s0, d_s1, d_bytes, d_sub,
                           (uint32_t)nrow, d_status + nd);
        hipLaunchKernelGGL(jpegdec_sub_write_kernel, dim3((unsigned)(nrow / JD_WAVE)), dim3(JD_WAVE), 0, c.stream, d_img, d_tab, d_par,
                           (const uint32_t*)(d_blob + o_wave), d_s0, d_s1, d_bytes, (const uint32_t*)d_sub, (uint32_t)nrow, d_coef, d_redo);
      }
      // whatever either kernel flagged, zeroed and decoded by the serial kernel: both launches end at once for every other image
      hipLaunchKernelGGL(jpegdec_redo_zero_kernel, dim3(std::min((max_blk * 8 + JD_THREADS - 1) / JD_THREADS, 64u), (unsigned)nd), dim3(JD_THREADS), 0,
                         c.stream, d_img, (const int32_t*)d_redo, d_coef, d_status + nd);
      hipLaunchKernelGGL(jpegdec_entropy_kernel<ENT_REDO>, dim3((unsigned)nd, max_groups), dim3(JD_WAVE), 0, c.stream, d_img, d_tab, d_s0, d_s1, d_bytes,
                         d_coef, d_status, d_kind, d_redo);
    }
    for (int s = 0; s < MAX_SCANS && scan_groups[s]; ++s)    // every image's scan s before any image's scan s + 1
      hipLaunchKernelGGL(jpegdec_scan_entropy_kernel, dim3((unsigned)nd, scan_groups[s]), dim3(JD_WAVE), 0, c.stream, d_img,
                         (const ScanDesc*)(d_blob + o_scan), (const HuffDec*)(d_blob + o_pool), d_s0, d_s1, d_bytes, d_coef, d_status, (uint32_t)s);
    tm.end("jpeg_decode B: entropy", (double)(blob - o_bytes));
    tm.begin();
    if (scale == 1)
      hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((max_blk + JD_THREADS - 1) / JD_THREADS, (unsigned)nd), dim3(JD_THREADS), 0, c.stream, d_img, d_tab,
                         (const int16_t*)d_coef, d_planes, d_status);
    else
      hipLaunchKernelGGL(jpegdec_idct_scaled_kernel, dim3((max_blk + JD_THREADS - 1) / JD_THREADS, (unsigned)nd), dim3(JD_THREADS), 0, c.stream, d_img,
                         d_tab, (const int16_t*)d_coef, d_planes, d_status, scale);
    tm.end("jpeg_decode C: idct", (double)coef_el * 2);
    tm.begin();
    const unsigned quads = (unsigned)(((size_t)((std::max(h, w) + 3) / 4) * std::max(h, w) + JD_THREADS - 1) / JD_THREADS);      // either orientation
    const int aligned = (int)(((uintptr_t)d_out & 3) == 0 && (out_b & 3) == 0);
    if (scale == 1)
      hipLaunchKernelGGL(jpegdec_colour_kernel<false>, dim3(quads, (unsigned)nd), dim3(JD_THREADS), 0, c.stream, d_img, (const uint8_t*)d_planes,
                         (const int32_t*)d_status, d_out, h, w, bgr ? 1 : 0, apply_orientation ? 1 : 0, aligned, 1);
    else
      hipLaunchKernelGGL(jpegdec_colour_kernel<true>, dim3(quads, (unsigned)nd), dim3(JD_THREADS), 0, c.stream, d_img, (const uint8_t*)d_planes,
                         (const int32_t*)d_status, d_out, h, w, bgr ? 1 : 0, apply_orientation ? 1 : 0, aligned, scale);
    tm.end("jpeg_decode D: colour", (double)nd * out_b);
    FE_HIP(hipGetLastError());
    st_host.resize((size_t)nd + 2);
    FE_HIP(hipMemcpyAsync(st_host.data(), d_status, (size_t)(nd + 2) * 4, hipMemcpyDeviceToHost, c.stream));
    FE_HIP(hipStreamSynchronize(c.stream));
    c.jpeg_entropy_stats[2] = std::max(c.jpeg_entropy_stats[2], st_host[nd]);
    c.jpeg_entropy_stats[3] += st_host[nd + 1];
    for (int k = 0; k < nd; ++k) status[todo[first + k]] = st_host[k];
    if (!dst_on_device) {                                    // runs of decoded neighbours come down in one copy each
      for (int k = 0; k < nd;) {
        if (st_host[k] != 0) { ++k; continue; }
        int e = k + 1;
        while (e < nd && st_host[e] == 0 && todo[first + e] == todo[first + e - 1] + 1) ++e;
        FE_HIP(hipMemcpyAsync(dst + (size_t)todo[first + k] * out_b, d_out + (size_t)k * out_b, (size_t)(e - k) * out_b, hipMemcpyDeviceToHost, c.stream));
        k = e;
      }
      FE_HIP(hipStreamSynchronize(c.stream));
    }
    first = last;
  }
}

}  // namespace fe
