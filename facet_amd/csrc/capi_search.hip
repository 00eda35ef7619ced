// C ABI: near-duplicate pairs, the clustering sweeps, similarity search.
#include "capi_internal.h"

namespace {
/* shapes the clustering sweeps accept; anything else is FE_ERR_INVALID with a message, never a launch */
bool cluster_shape_ok(fe_ctx* ctx, const char* who, int n, int n_min, int d) {
  char b[160];
  if (n < n_min || n > 262144) { snprintf(b, sizeof(b), "%s: %d rows (supported: %d .. 262144)", who, n, n_min); ctx->c.err = b; return false; }
  if (d < 32 || d > 1024 || d % 32 != 0) { snprintf(b, sizeof(b), "%s: d = %d (supported: multiples of 32 in 32 .. 1024)", who, d); ctx->c.err = b; return false; }
  return true;
}
bool cluster_k_ok(fe_ctx* ctx, const char* who, int n, int k) {
  char b[160];
  if (k < 1 || k > 32 || k > n) { snprintf(b, sizeof(b), "%s: k = %d (supported: 1 .. min(32, n = %d))", who, k, n); ctx->c.err = b; return false; }
  return true;
}

/* one side of fe_similar_topk / fe_similar_pairs */
bool sim_rows_ok(fe_ctx* ctx, const char* who, const fe_sim_rows* r, int d) {
  char b[200];
  if (!r || !r->emb) { snprintf(b, sizeof(b), "%s: null rows", who); ctx->c.err = b; return false; }
  if (!cluster_shape_ok(ctx, who, r->n, 1, d)) return false;
  if (r->n_person_ids < 0 || ((r->person_off == nullptr) != (r->person_ids == nullptr) && r->n_person_ids > 0)) {
    snprintf(b, sizeof(b), "%s: person_off and person_ids go together (n_person_ids = %d)", who, r->n_person_ids); ctx->c.err = b; return false;
  }
  return true;
}
bool sim_common_ok(fe_ctx* ctx, const char* who, const fe_sim_rows* q, const fe_sim_rows* c, int d, int kind, const float* weights) {
  if (!sim_rows_ok(ctx, who, q, d) || !sim_rows_ok(ctx, who, c, d)) return false;
  if (kind != FE_SIM_FUSED && kind != FE_SIM_COSINE) { ctx->c.err = std::string(who) + ": score_kind must be FE_SIM_FUSED or FE_SIM_COSINE"; return false; }
  if (kind == FE_SIM_FUSED && !weights) { ctx->c.err = std::string(who) + ": the fused score needs weights [4]"; return false; }
  return true;
}
}  // namespace

extern "C" {

/* every i < j with popcount(hashes[i] ^ hashes[j]) <= max_distance, ascending (reference utils/duplicate.py:89-119) */
int fe_hamming_pairs(fe_ctx* ctx, const uint64_t* hashes, int n, int on_device, int max_distance, int64_t max_pairs, int32_t* pairs,
                     int64_t* count) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(count && n >= 0 && (n == 0 || hashes) && max_distance >= 0 && max_pairs >= 0 && (max_pairs == 0 || pairs), "bad arguments");
    *count = 0;
    if (n < 2) return FE_OK;
    C.arena.reset();
    const uint64_t* d_h = resident(C, hashes, (size_t)n, on_device);
    // one block: pairs [max_pairs][2], then the hit counter, then a canary word. A store past the capacity would land on the counter
    // first and on the canary next, so the kernel's own bounds check is visible from outside (exact count + intact canary).
    const unsigned long long canary = 0xA5A5A5A5A5A5A5A5ull;
    uint8_t* d_block = (uint8_t*)C.arena.alloc((size_t)max_pairs * 2 * sizeof(int) + 2 * sizeof(unsigned long long));
    int* d_pairs = max_pairs ? (int*)d_block : nullptr;
    unsigned long long* d_count = (unsigned long long*)(d_block + (size_t)max_pairs * 2 * sizeof(int));
    FE_HIP(hipMemsetAsync(d_count + 1, 0xA5, sizeof(unsigned long long), C.stream));
    launch_hamming_pairs(d_h, n, std::min(max_distance, 64), max_pairs, d_pairs, d_count, C.stream);
    unsigned long long tail[2] = {0, 0};
    FE_HIP(hipMemcpyAsync(tail, d_count, sizeof(tail), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    FE_CHECK(tail[1] == canary, "hamming_pairs: the word after the pair buffer was overwritten");
    const unsigned long long found = tail[0];
    *count = (int64_t)found;
    if (found && found <= (unsigned long long)max_pairs) {
      FE_HIP(hipMemcpyAsync(pairs, d_pairs, (size_t)found * 2 * sizeof(int), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
      // the order of arrival is the order the waves ran in; the caller gets ascending (i, j)
      struct P { int32_t i, j; };
      P* p = reinterpret_cast<P*>(pairs);
      std::sort(p, p + found, [](const P& a, const P& b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
    }
    return FE_OK;
  });
}

/* per row the largest earlier row it is similar to: the pair test of process_bursts (reference processing/scorer.py:1943-1968) */
int fe_burst_links(fe_ctx* ctx, const uint64_t* hashes, int on_device, const int64_t* times, const uint8_t* flags, int n, const int32_t* person_off,
                   const int32_t* person_ids, int n_person_ids, int thr, int64_t window_s, int64_t rapid_s, int32_t* link) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    char b[200];
    auto invalid = [&](const char* msg) { ctx->c.err = std::string("fe_burst_links: ") + msg; return FE_ERR_INVALID; };
    if (n < 0) return invalid("negative n");
    if (n == 0) return FE_OK;
    if (!hashes || !times || !flags || !link) return invalid("null pointer");
    if (n_person_ids < 0 || (person_off == nullptr) != (person_ids == nullptr)) return invalid("person_off and person_ids go together, n_person_ids >= 0");
    const int64_t t_max = (int64_t)1 << 61;
    for (int i = 0; i < n; ++i) {
      if (flags[i] & ~(FE_BURST_HAS_HASH | FE_BURST_HAS_DATE)) { snprintf(b, sizeof(b), "flags[%d] = %d has bits outside FE_BURST_HAS_HASH | FE_BURST_HAS_DATE", i, (int)flags[i]); return invalid(b); }
      if ((flags[i] & FE_BURST_HAS_DATE) && (times[i] < -t_max || times[i] > t_max)) { snprintf(b, sizeof(b), "times[%d] = %lld is outside +-2^61", i, (long long)times[i]); return invalid(b); }
    }
    if (person_off) {
      if (person_off[0] < 0 || person_off[n] > n_person_ids) { snprintf(b, sizeof(b), "person_off runs from %d to %d with %d ids", person_off[0], person_off[n], n_person_ids); return invalid(b); }
      for (int i = 0; i < n; ++i)
        if (person_off[i] > person_off[i + 1]) { snprintf(b, sizeof(b), "person_off[%d] = %d > person_off[%d] = %d", i, person_off[i], i + 1, person_off[i + 1]); return invalid(b); }
      for (int i = 0; i < n; ++i)                                      // every offset is now known to lie in 0 .. n_person_ids
        for (int k = person_off[i] + 1; k < person_off[i + 1]; ++k)
          if (person_ids[k - 1] >= person_ids[k]) { snprintf(b, sizeof(b), "person ids of row %d are not ascending and distinct", i); return invalid(b); }
    }
    if (n == 1) { link[0] = -1; return FE_OK; }
    // dist is 0 .. 64 or 999 and d is below 2^62: beyond these the settings change nothing
    const int thr_c = std::max(-1, std::min(thr, 999));
    const int64_t s_max = (int64_t)1 << 62;
    const int64_t window_c = std::max<int64_t>(-1, std::min(window_s, s_max)), rapid_c = std::max<int64_t>(-1, std::min(rapid_s, s_max));
    C.arena.reset();
    const uint64_t* d_h = resident(C, hashes, (size_t)n, on_device);
    burst_links(C, d_h, times, flags, n, person_off, person_ids, n_person_ids, thr_c, window_c, rapid_c, link);
    return FE_OK;
  });
}

/* core distance (distance to the k-th nearest row, the row itself counted) of every row: HDBSCAN's first stage (reference faces/clusterer.py:188-197) */
int fe_knn_core_distances(fe_ctx* ctx, const float* x, int n, int d, int on_device, int normalise, int k, double* core, int32_t* core_idx) {
  return fe_api(ctx, [&] {
    if (!x || !core) { ctx->c.err = "fe_knn_core_distances: null pointer"; return FE_ERR_INVALID; }
    if (!cluster_shape_ok(ctx, "fe_knn_core_distances", n, 2, d) || !cluster_k_ok(ctx, "fe_knn_core_distances", n, k)) return FE_ERR_INVALID;
    cluster_core_distances(ctx->c, x, n, d, on_device, normalise, k, core, core_idx);
    return FE_OK;
  });
}

/* minimum spanning tree of the mutual-reachability graph: HDBSCAN's second stage (reference faces/clusterer.py:188-197) */
int fe_mreach_mst(fe_ctx* ctx, const float* x, int n, int d, int on_device, int normalise, int k, int32_t* edge_u, int32_t* edge_v, double* edge_w,
                  double* core, int32_t* rounds) {
  return fe_api(ctx, [&] {
    if (!x || !edge_u || !edge_v || !edge_w) { ctx->c.err = "fe_mreach_mst: null pointer"; return FE_ERR_INVALID; }
    if (!cluster_shape_ok(ctx, "fe_mreach_mst", n, 2, d) || !cluster_k_ok(ctx, "fe_mreach_mst", n, k)) return FE_ERR_INVALID;
    cluster_mreach_mst(ctx->c, x, n, d, on_device, normalise, k, edge_u, edge_v, edge_w, core, rounds);
    return FE_OK;
  });
}

/* best cosine match of every query row among the candidate rows (reference faces/clusterer.py:399-405, :508-518) */
int fe_cosine_best_match(fe_ctx* ctx, const float* q, int nq, const float* c, int nc, int d, float* best_sim, int32_t* best_idx) {
  return fe_api(ctx, [&] {
    if (!q || !c || !best_sim || !best_idx) { ctx->c.err = "fe_cosine_best_match: null pointer"; return FE_ERR_INVALID; }
    if (!cluster_shape_ok(ctx, "fe_cosine_best_match", nq, 1, d) || !cluster_shape_ok(ctx, "fe_cosine_best_match", nc, 1, d)) return FE_ERR_INVALID;
    cluster_best_match(ctx->c, q, nq, c, nc, d, best_sim, best_idx);
    return FE_OK;
  });
}

/* top-k similar candidates per query (reference api/routers/gallery.py:410-539) */
int fe_similar_topk(fe_ctx* ctx, const fe_sim_rows* q, const fe_sim_rows* c, int d, int score_kind, const float* weights, const int32_t* q_self,
                    const uint8_t* visible, int k, int32_t* idx, float* score) {
  return fe_api(ctx, [&] {
    if (!idx || !score) { ctx->c.err = "fe_similar_topk: null pointer"; return FE_ERR_INVALID; }
    if (!sim_common_ok(ctx, "fe_similar_topk", q, c, d, score_kind, weights)) return FE_ERR_INVALID;
    if (k < 1 || k > FE_SIM_K_MAX) { char b[120]; snprintf(b, sizeof(b), "fe_similar_topk: k = %d (supported: 1 .. %d)", k, FE_SIM_K_MAX); ctx->c.err = b; return FE_ERR_INVALID; }
    similar_topk(ctx->c, *q, *c, d, score_kind == FE_SIM_COSINE, weights, q_self, visible, k, idx, score);
    return FE_OK;
  });
}

/* every (query, candidate) at or above a threshold (similar photos' tie sets; reference faces/merge_analyzer.py:64-72) */
int fe_similar_pairs(fe_ctx* ctx, const fe_sim_rows* q, const fe_sim_rows* c, int d, int score_kind, const float* weights, const int32_t* q_self,
                     const uint8_t* visible, const float* thr, int n_thr, int upper, int64_t max_pairs, int32_t* pairs, float* scores, int64_t* count) {
  return fe_api(ctx, [&] {
    if (!count || !thr || max_pairs < 0 || (max_pairs > 0 && (!pairs || !scores))) { ctx->c.err = "fe_similar_pairs: null pointer or negative max_pairs"; return FE_ERR_INVALID; }
    if (!sim_common_ok(ctx, "fe_similar_pairs", q, c, d, score_kind, weights)) return FE_ERR_INVALID;
    if (n_thr != 1 && n_thr != q->n) { ctx->c.err = "fe_similar_pairs: n_thr must be 1 or the number of queries"; return FE_ERR_INVALID; }
    if (upper && q->n != c->n) { ctx->c.err = "fe_similar_pairs: upper = 1 needs as many queries as candidates"; return FE_ERR_INVALID; }
    *count = 0;
    similar_pairs(ctx->c, *q, *c, d, score_kind == FE_SIM_COSINE, weights, q_self, visible, thr, n_thr, upper, max_pairs, pairs, scores, count);
    return FE_OK;
  });
}

}  // extern "C"
