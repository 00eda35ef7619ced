// Burst detection over stored hashes: link[i] = the largest j < i that photo i is "similar" to, or -1 (fe_burst_links).
//
// The reference (processing/scorer.py:1880-1986, `process_bursts`) walks the photos in date order with one open burst and asks, per
// photo, whether it is similar to ANY member of that burst - a Python loop over the members with two strptime calls per comparison.
// The open burst is always the contiguous run [s, i-1], so "similar to any member" is L(i) >= s with L(i) the largest j < i that
// passes the pair test. L does not depend on s: it is one independent job per photo and the only part that runs here. The O(n)
// recurrence over L and the choice of the lead stay on the host (facet_amd/bursts.py).
//
// similar(i, j), both dates parsed, d = |t_i - t_j| in whole seconds, dist = popcount(h_i ^ h_j) (999 when either row has no hash):
//   slow rule:  d <= window_s and dist <= thr
//   rapid rule: d <= rapid_s and dist <= 2 thr and the rows share a person (either list empty, or the sorted lists intersect)
//
// burst_links_kernel: one wave per photo. The lanes take j = i-1, i-2, ... in chunks of 64 (lane 0 the nearest), a ballot finds the
// chunk's matches and its lowest set lane is the largest matching j; the wave stops at the first chunk with a match or at lo[i].
// lo[i] (host, burst_lower_bounds) is exact for any row order: the first j whose prefix maximum of parsed times reaches
// t_i - max(window_s, rapid_s). Every row below it is too old; later rows that are out of order merely fail the pair test.
// Times stay 64-bit throughout. No atomics, one int32 per photo out.
#include "engine.h"
#include <algorithm>
#include <vector>

namespace fe {

constexpr int BL_WAVES = 4;              // photos per block
constexpr int BL_NO_HASH_DIST = 999;     // the reference's distance for a pair with an empty hash string

// either list empty, or the two ascending lists have an element in common
__device__ __forceinline__ bool bl_share_person(const int* __restrict__ a, int na, const int* __restrict__ b, int nb) {
  if (na == 0 || nb == 0) return true;
  int x = 0, y = 0;
  while (x < na && y < nb) {
    const int u = a[x], v = b[y];
    if (u == v) return true;
    if (u < v) ++x; else ++y;
  }
  return false;
}

// hash / time / flags / lo [n]; person_off [n + 1] + person_ids, or both null; thr2 = 2 thr; link [n].
// 0 <= lo[i] <= i (burst_lower_bounds), so every j read lies in [0, i).
__global__ __launch_bounds__(BL_WAVES * 64) void burst_links_kernel(const unsigned long long* __restrict__ hash, const long long* __restrict__ time,
                                                                    const uint8_t* __restrict__ flags, const int* __restrict__ lo,
                                                                    const int* __restrict__ person_off, const int* __restrict__ person_ids, int n,
                                                                    int thr, int thr2, long long window_s, long long rapid_s, int* __restrict__ link) {
  const int lane = threadIdx.x & 63;
  const long long slot = (long long)blockIdx.x * BL_WAVES + (threadIdx.x >> 6);
  if (slot >= n) return;                                   // wave-uniform; the kernel has no barrier
  const int i = n - 1 - (int)slot;                         // the rows with the most predecessors are dispatched first
  const unsigned fi = flags[i];
  int best = -1;
  // a row without a hash meets only the distance 999
  if ((fi & FE_BURST_HAS_DATE) && ((fi & FE_BURST_HAS_HASH) || max(thr, thr2) >= BL_NO_HASH_DIST)) {
    const long long ti = time[i];
    const unsigned long long hi = hash[i];
    const int lo_i = lo[i];
    int pa = 0, na = 0;
    if (person_off) { pa = person_off[i]; na = person_off[i + 1] - pa; }
    for (int top = i - 1; top >= lo_i; top -= 64) {
      const int j = top - lane;
      bool hit = false;
      if (j >= lo_i) {
        const unsigned fj = flags[j];
        if (fj & FE_BURST_HAS_DATE) {
          const long long tj = time[j];
          const long long d = ti > tj ? ti - tj : tj - ti;  // |t| <= 2^61 (checked on the host): no overflow
          if (d <= window_s || d <= rapid_s) {
            const int dist = (fi & fj & FE_BURST_HAS_HASH) ? __popcll(hi ^ hash[j]) : BL_NO_HASH_DIST;
            hit = d <= window_s && dist <= thr;
            if (!hit && d <= rapid_s && dist <= thr2) {
              int pb = 0, nb = 0;
              if (person_off) { pb = person_off[j]; nb = person_off[j + 1] - pb; }
              hit = bl_share_person(person_ids + pa, na, person_ids + pb, nb);
            }
          }
        }
      }
      const unsigned long long m = __ballot(hit);
      if (m) { best = top - (__ffsll((long long)m) - 1); break; }
    }
  }
  if (lane == 0) link[i] = best;
}

// lo [n]: per row the first j <= i whose prefix maximum of parsed times is >= t_i - reach (reach = max(window_s, rapid_s)); i itself
// when reach < 0 (no pair passes) or the row has no date. pm is non-decreasing, so it is one bisection per row.
void burst_lower_bounds(const int64_t* times, const uint8_t* flags, int n, int64_t reach, int32_t* lo) {
  std::vector<int64_t> pm((size_t)n);
  int64_t run = INT64_MIN;
  for (int i = 0; i < n; ++i) {
    if ((flags[i] & FE_BURST_HAS_DATE) && times[i] > run) run = times[i];
    pm[i] = run;
  }
  for (int i = 0; i < n; ++i) {
    if (!(flags[i] & FE_BURST_HAS_DATE) || reach < 0) { lo[i] = i; continue; }
    lo[i] = (int32_t)(std::lower_bound(pm.begin(), pm.begin() + i, times[i] - reach) - pm.begin());
  }
}

// d_hash [n] device; times / flags [n], person_off [n + 1] / person_ids [n_ids] (both null: no person test), link [n]: host.
// The caller has checked the arrays (capi_search.hip); thr in [-1, 999], window_s / rapid_s in [-1, 2^62], |times| <= 2^61.
void burst_links(Ctx& c, const uint64_t* d_hash, const int64_t* times, const uint8_t* flags, int n, const int32_t* person_off, const int32_t* person_ids,
                 int n_ids, int thr, int64_t window_s, int64_t rapid_s, int32_t* link) {
  FE_CHECK(n >= 2 && d_hash && times && flags && link && thr >= -1 && thr <= BL_NO_HASH_DIST, "burst_links: bad arguments");
  std::vector<int32_t> lo((size_t)n);
  burst_lower_bounds(times, flags, n, std::max(window_s, rapid_s), lo.data());
  auto up = [&](const void* src, size_t bytes) {
    void* d = c.arena.alloc(bytes);
    FE_HIP(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, c.stream));
    return d;
  };
  const long long* d_time = (const long long*)up(times, (size_t)n * sizeof(int64_t));
  const int* d_lo = (const int*)up(lo.data(), (size_t)n * sizeof(int32_t));
  const uint8_t* d_flags = (const uint8_t*)up(flags, (size_t)n);
  const int* d_off = nullptr;
  const int* d_ids = nullptr;
  if (person_off) {
    d_off = (const int*)up(person_off, ((size_t)n + 1) * sizeof(int32_t));
    d_ids = n_ids > 0 ? (const int*)up(person_ids, (size_t)n_ids * sizeof(int32_t)) : (const int*)c.arena.alloc(sizeof(int32_t));   // never read when every list is empty
  }
  int* d_link = (int*)c.arena.alloc((size_t)n * sizeof(int32_t));
  const unsigned blocks = (unsigned)(((size_t)n + BL_WAVES - 1) / BL_WAVES);
  hipLaunchKernelGGL(burst_links_kernel, dim3(blocks), dim3(BL_WAVES * 64), 0, c.stream, (const unsigned long long*)d_hash, d_time, d_flags, d_lo, d_off,
                     d_ids, n, thr, 2 * thr, (long long)window_s, (long long)rapid_s, d_link);
  FE_HIP(hipGetLastError());
  FE_HIP(hipMemcpyAsync(link, d_link, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipStreamSynchronize(c.stream));                  // lo (pageable host memory) is read by the copy above until here
}

}  // namespace fe
