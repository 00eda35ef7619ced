// Tag selection on the device: per-tag max over the prompts, threshold and ranked top-k for every row of a similarity matrix
// (fe_tag_select, fe_tag_select_sims). The arithmetic is tag_select_core.h's, which restates models/tagger.py:103-114.
//
// tag_select_kernel: one wave per image row, TS_WAVES rows per block as far as the LDS reaches.
//   1. the row's T similarities go to LDS, lanes striding over t (coalesced);
//   2. lanes stride over the G tags; each folds its tag's prompts in prompt order through perm / goff (tagsel::fold) and leaves the
//      score and the keep flag in LDS;
//   3. the kept tags are counted (ballot), written = min(kept, max_tags);
//   4. lanes stride over the tags again: a kept tag's position is the number of kept tags that beat it (tagsel::beats); positions
//      below max_tags are stored, and the slots written .. max_tags-1 are padded by other stores to other addresses.
// There are no atomics and nothing depends on the order of lanes or launches. The block barriers are reached by every wave: a wave
// without a row (the last block) only skips the work between them, and T, G and max_tags are the same for all. No block waits for
// another. Rows are addressed with 64-bit offsets and a leading dimension.
//
// gather_rows_kernel: [n][d] rows that lie ld floats apart into a packed buffer, so that records can be read in place: columns
// 21 .. 788 of the 789-float ensemble record start 84 bytes into a row, which the GEMM's 16-byte loads cannot take.
#include "engine.h"
#include "tag_select_core.h"
#include <algorithm>

namespace fe {

constexpr int TS_WAVES = 4;                      // rows per block at most
constexpr size_t TS_LDS_BYTES = 64 * 1024;       // per block; one row of T = G = 4096 needs 36 KiB

static size_t ts_row_lds(int T, int G) { return ((size_t)T + G) * sizeof(float) + (((size_t)G + 3) & ~(size_t)3); }

// sims: rows ld floats apart, n rows of T; perm [T], goff [G + 1]; ids / scores [n][max_tags], counts [n].
// LDS per wave: T floats (the row), G floats (scores), G bytes rounded up to 4 (keep flags); `waves` waves per block.
__global__ __launch_bounds__(TS_WAVES * 64) void tag_select_kernel(const float* __restrict__ sims, long long ld, int n, int T, int G,
                                                                   const int32_t* __restrict__ perm, const int32_t* __restrict__ goff,
                                                                   double threshold, int max_tags, int waves, int32_t* __restrict__ ids,
                                                                   float* __restrict__ scores, int32_t* __restrict__ counts) {
  extern __shared__ float ts_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * waves + wave;
  const bool active = row < n;                   // wave-uniform
  float* s_sim = ts_lds + (size_t)wave * ((size_t)T + G);
  float* s_score = s_sim + T;
  uint8_t* s_keep = reinterpret_cast<uint8_t*>(ts_lds + (size_t)waves * ((size_t)T + G)) + (size_t)wave * (((size_t)G + 3) & ~(size_t)3);

  if (active) {
    const float* src = sims + row * ld;
    for (int t = lane; t < T; t += 64) s_sim[t] = src[t];
  }
  __syncthreads();
  if (active) {
    for (int g = lane; g < G; g += 64) {
      const float s = tagsel::fold(s_sim, perm, goff[g], goff[g + 1]);
      s_score[g] = s;
      s_keep[g] = tagsel::keep(s, threshold) ? 1 : 0;
    }
  }
  __syncthreads();
  if (!active) return;                           // no barrier below

  int kept = 0;
  for (int g0 = 0; g0 < G; g0 += 64) {           // every lane runs every iteration: the ballot sees the whole wave
    const int g = g0 + lane;
    kept += __popcll(__ballot(g < G && s_keep[g] != 0));
  }
  const int written = min(kept, max_tags);
  int32_t* o_ids = ids + row * max_tags;
  float* o_scores = scores + row * max_tags;
  for (int g = lane; g < G; g += 64) {
    if (!s_keep[g]) continue;
    const float s = s_score[g];
    int rank = 0;
    for (int h = 0; h < G; ++h) rank += (s_keep[h] && tagsel::beats(s_score[h], h, s, g)) ? 1 : 0;
    if (rank < max_tags) { o_ids[rank] = g; o_scores[rank] = s; }      // rank < written: ranks are 0 .. kept-1, each once
  }
  for (int k = written + lane; k < max_tags; k += 64) { o_ids[k] = -1; o_scores[k] = 0.f; }
  if (lane == 0) counts[row] = written;
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, long long ld, long long n, int d, float* __restrict__ dst) {
  const long long total = n * d;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / d;
    dst[i] = src[r * ld + (i - r * d)];
  }
}

void launch_gather_rows(const float* d_src, long long ld, int n, int d, float* d_dst, hipStream_t s) {
  FE_CHECK(d_src && d_dst && n > 0 && d > 0 && ld >= d, "gather_rows: bad arguments");
  const long long total = (long long)n * d;
  const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, s, d_src, ld, (long long)n, d, d_dst);
  FE_HIP(hipGetLastError());
}

// d_sims: n rows of T, ld floats apart (device); d_perm [T], d_goff [G + 1]; d_ids / d_scores [n][max_tags], d_counts [n] (device).
// The caller has checked 1 <= G <= T <= tagsel::kMaxPrompts and 1 <= max_tags <= G (capi_tags.hip).
void launch_tag_select(const float* d_sims, long long ld, int n, int T, int G, const int32_t* d_perm, const int32_t* d_goff, double threshold,
                       int max_tags, int32_t* d_ids, float* d_scores, int32_t* d_counts, hipStream_t s) {
  FE_CHECK(d_sims && d_perm && d_goff && d_ids && d_scores && d_counts && n > 0 && G >= 1 && G <= T && T <= tagsel::kMaxPrompts && ld >= T &&
               max_tags >= 1 && max_tags <= G,
           "tag_select: bad arguments");
  const size_t per_row = ts_row_lds(T, G);
  const int waves = (int)std::max<size_t>(1, std::min<size_t>(TS_WAVES, TS_LDS_BYTES / per_row));
  FE_CHECK(per_row * waves <= TS_LDS_BYTES, "tag_select: a row of T = %d, G = %d needs %zu bytes of LDS", T, G, per_row);
  const unsigned blocks = (unsigned)(((size_t)n + waves - 1) / waves);
  hipLaunchKernelGGL(tag_select_kernel, dim3(blocks), dim3(waves * 64), per_row * waves, s, d_sims, ld, n, T, G, d_perm, d_goff, threshold, max_tags,
                     waves, d_ids, d_scores, d_counts);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
