// C ABI: the tag vocabulary of a context and the tag selection over it (per-tag max, threshold, ranked top-k; kernels_tags.hip).
#include "capi_internal.h"
#include "tag_select_core.h"

namespace {

constexpr int kTagChunkMax = 131072;      // rows per chunk at most: rows * T stays below 2^30

fe_status tags_invalid(fe_ctx* ctx, const char* who, const char* msg) {
  ctx->c.err = std::string(who) + ": " + msg;
  return FE_ERR_INVALID;
}

// rows [r0, r0 + rows) of a host matrix whose rows lie ld floats apart, packed into dst (device)
void upload_rows(Ctx& C, const float* src, int ld, int width, int rows, float* dst) {
  if (ld == width) FE_HIP(hipMemcpyAsync(dst, src, (size_t)rows * width * sizeof(float), hipMemcpyHostToDevice, C.stream));
  else FE_HIP(hipMemcpy2DAsync(dst, (size_t)width * sizeof(float), src, (size_t)ld * sizeof(float), (size_t)width * sizeof(float), (size_t)rows, hipMemcpyHostToDevice, C.stream));
}

// fe_tag_select (from_sims = false: src is [n][d] embeddings) and fe_tag_select_sims (true: src is [n][T] similarities)
fe_status tag_select_run(fe_ctx* ctx, const char* who, bool from_sims, const float* src, int n, int ld, int on_device, double threshold, int max_tags,
                   int32_t* ids, float* scores, int32_t* counts) {
  Ctx& C = ctx->c;
  char b[240];
  if (!ctx->tag_vocab) {
    C.err = std::string(who) + ": no tag vocabulary is set (fe_tag_vocab_set)";
    return FE_ERR_NOT_LOADED;
  }
  const fe_ctx::TagVocab& v = *ctx->tag_vocab;
  const int width = from_sims ? v.T : v.d;
  if (n < 0) return tags_invalid(ctx, who, "negative n");
  if (max_tags < 1 || max_tags > v.G) { snprintf(b, sizeof b, "max_tags = %d (supported: 1 .. G = %d, the tags of the vocabulary)", max_tags, v.G); return tags_invalid(ctx, who, b); }
  if (n == 0) return FE_OK;
  if (!src || !ids || !scores || !counts) return tags_invalid(ctx, who, "null pointer");
  if (ld < width) { snprintf(b, sizeof b, "ld = %d is smaller than a row of %d floats", ld, width); return tags_invalid(ctx, who, b); }

  // what a row takes of the arena: its packed input, its similarities, its outputs (each allocation is rounded up to 256 bytes once)
  const size_t per_row = (size_t)width * sizeof(float) + (from_sims ? 0 : (size_t)v.T * sizeof(float)) + (size_t)max_tags * 8 + 4;
  const size_t room = C.arena.capacity() / 2;            // the other half is the GEMM's (split-K partials, when they fit)
  if (room < per_row + 4096) { snprintf(b, sizeof b, "%s: one row needs %zu bytes of the arena, which holds %zu", who, per_row, C.arena.capacity()); throw CapacityError(b); }
  const size_t fit = std::min<size_t>((room - 4096) / per_row, (size_t)kTagChunkMax);
  const int chunk = (int)(ctx->tag_chunk > 0 ? std::min<size_t>((size_t)ctx->tag_chunk, fit) : fit);

  for (int r0 = 0; r0 < n; r0 += chunk) {
    const int rows = std::min(chunk, n - r0);
    C.arena.reset();
    const float* at = src + (size_t)r0 * ld;
    const float* d_in = at;                               // resident rows are read in place where the consumer can take them
    long long ld_in = ld;
    // the selection kernel reads single floats at any leading dimension; the GEMM wants packed rows on a 16-byte boundary
    const bool in_place = on_device && (from_sims || (ld == width && ((uintptr_t)at & 15) == 0));
    if (!in_place) {
      float* d_p = (float*)C.arena.alloc((size_t)rows * width * sizeof(float));
      if (on_device) launch_gather_rows(at, ld, rows, width, d_p, C.stream);
      else upload_rows(C, at, ld, width, rows, d_p);
      d_in = d_p;
      ld_in = width;
    }
    const float* d_s = d_in;
    long long ld_s = ld_in;
    if (!from_sims) {
      float* d_y = (float*)C.arena.alloc((size_t)rows * v.T * sizeof(float));
      linear_forward(C, v.w, d_in, v.d, rows, d_y, v.T, ACT_NONE);
      d_s = d_y;
      ld_s = v.T;
    }
    int32_t* d_ids = (int32_t*)C.arena.alloc((size_t)rows * max_tags * sizeof(int32_t));
    float* d_scores = (float*)C.arena.alloc((size_t)rows * max_tags * sizeof(float));
    int32_t* d_counts = (int32_t*)C.arena.alloc((size_t)rows * sizeof(int32_t));
    launch_tag_select(d_s, ld_s, rows, v.T, v.G, v.perm, v.goff, threshold, max_tags, d_ids, d_scores, d_counts, C.stream);
    FE_HIP(hipMemcpyAsync(ids + (size_t)r0 * max_tags, d_ids, (size_t)rows * max_tags * sizeof(int32_t), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(scores + (size_t)r0 * max_tags, d_scores, (size_t)rows * max_tags * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(counts + r0, d_counts, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));               // the next chunk recycles the arena
  }
  return FE_OK;
}

}  // namespace

extern "C" {

/* the context's tag vocabulary: text rows packed once for the GEMM, prompts grouped by tag */
int fe_tag_vocab_set(fe_ctx* ctx, const float* text, int T, int d, const int32_t* tag_of_prompt, int G) {
  return fe_api(ctx, [&] {
    const char* who = "fe_tag_vocab_set";
    char b[240];
    FE_HIP(hipStreamSynchronize(ctx->c.stream));
    if (T == 0) { ctx->tag_vocab.reset(); return FE_OK; }
    if (G < 1 || G > T || T > tagsel::kMaxPrompts) {
      snprintf(b, sizeof b, "T = %d prompts, G = %d tags (supported: 1 <= G <= T <= %d)", T, G, tagsel::kMaxPrompts);
      return tags_invalid(ctx, who, b);
    }
    if (d < 4 || d > 8192 || d % 4 != 0) { snprintf(b, sizeof b, "d = %d (supported: multiples of 4 in 4 .. 8192)", d); return tags_invalid(ctx, who, b); }
    if (!text || !tag_of_prompt) return tags_invalid(ctx, who, "null pointer");
    std::vector<int32_t> perm((size_t)T), goff((size_t)G + 1);
    int where = 0;
    switch (tagsel::build_groups(tag_of_prompt, T, G, perm.data(), goff.data(), &where)) {
      case tagsel::GROUPS_OK: break;
      case tagsel::GROUPS_ID_RANGE:
        snprintf(b, sizeof b, "tag_of_prompt[%d] = %d is outside 0 .. G-1 = %d", where, tag_of_prompt[where], G - 1);
        return tags_invalid(ctx, who, b);
      case tagsel::GROUPS_ID_ORDER:
        snprintf(b, sizeof b, "tag_of_prompt[%d] = %d appears before any prompt has tag id %d: ids are numbered by first appearance, none skipped", where,
                 tag_of_prompt[where], tag_of_prompt[where] - 1);
        return tags_invalid(ctx, who, b);
      case tagsel::GROUPS_ID_UNUSED:
        snprintf(b, sizeof b, "no prompt has tag id %d: every id of 0 .. G-1 = %d must be used", where, G - 1);
        return tags_invalid(ctx, who, b);
    }
    auto v = std::make_unique<fe_ctx::TagVocab>();
    HostTensor w;
    w.shape = {T, d};
    w.data.assign(text, text + (size_t)T * d);
    v->w = build_linear_rows(v->dw, w, nullptr, 0, T);
    v->perm = (int32_t*)v->dw.upload_raw(perm.data(), perm.size() * sizeof(int32_t));
    v->goff = (int32_t*)v->dw.upload_raw(goff.data(), goff.size() * sizeof(int32_t));
    v->T = T; v->G = G; v->d = d;
    ctx->tag_vocab = std::move(v);                        // a second vocabulary replaces the first
    return FE_OK;
  });
}

int fe_set_tag_chunk(fe_ctx* ctx, int rows) {
  return fe_api(ctx, [&] {
    if (rows < 0) {
      char b[120];
      snprintf(b, sizeof b, "%d rows (0 for the size the arena gives, or a positive count)", rows);
      return tags_invalid(ctx, "fe_set_tag_chunk", b);
    }
    ctx->tag_chunk = rows;
    return FE_OK;
  });
}

/* embeddings -> similarities on the cached text rows -> selection, chunk by chunk; the similarities stay on the device */
int fe_tag_select(fe_ctx* ctx, const float* emb, int n, int ld, int on_device, double threshold, int max_tags, int32_t* ids, float* scores,
                  int32_t* counts) {
  return fe_api(ctx, OnError::Capacity, [&] { return tag_select_run(ctx, "fe_tag_select", false, emb, n, ld, on_device, threshold, max_tags, ids, scores, counts); });
}

/* the selection alone on a given [n][T] matrix */
int fe_tag_select_sims(fe_ctx* ctx, const float* sims, int n, int ld, int on_device, double threshold, int max_tags, int32_t* ids, float* scores,
                       int32_t* counts) {
  return fe_api(ctx, OnError::Capacity, [&] { return tag_select_run(ctx, "fe_tag_select_sims", true, sims, n, ld, on_device, threshold, max_tags, ids, scores, counts); });
}

}  // extern "C"
