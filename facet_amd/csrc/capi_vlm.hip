// C ABI: the three VLM families (Qwen2.5-VL, Qwen2-VL, Qwen3-VL) - configure, preprocess, vision encode, prefill, decode.
#include "capi_internal.h"
#include "fp8_core.h"

namespace {
// ---- the blocks every vision encode entry point repeats ----
// room for `rows` merged embeddings in m.img_embeds
void vlm_grow_img_embeds(VlmModel& m, int rows) {
  if (rows <= m.img_cap) return;
  if (m.img_embeds) (void)hipFree(m.img_embeds);
  m.img_embeds = nullptr; m.img_cap = 0;
  FE_HIP(hipMalloc((void**)&m.img_embeds, (size_t)rows * m.hidden * sizeof(bf16)));
  m.img_cap = rows;
}
// every segment of cu [n + 1] holds a row (`what` names the segments in the error); returns the longest
int vlm_longest_segment(const int32_t* cu, int n, const char* what) {
  int longest = 0;
  for (int i = 0; i < n; ++i) { FE_CHECK(cu[i + 1] > cu[i], "empty %s segment", what); longest = std::max(longest, cu[i + 1] - cu[i]); }
  return longest;
}
// n bf16 embedding values as fp32 to the host through the arena buffer d_f (copied on the stream: the caller synchronises)
void vlm_download_f32(Ctx& C, const bf16* src, size_t n, float* d_f, float* dst) {
  launch_convert(src, d_f, n, C.stream);
  FE_HIP(hipMemcpyAsync(dst, d_f, n * sizeof(float), hipMemcpyDeviceToHost, C.stream));
}
// shared by fe_vlm_encode_images (fp32 rows from the host) and fe_vlm_encode_preprocessed (pixel_values == nullptr: the bf16 rows the last
// fe_vlm_preprocess_rgb left on the device)
void vlm_encode(fe_ctx* ctx, const float* pixel_values, int n_patches, const int32_t* patch_pos_hw, const int32_t* window_index,
                const int32_t* cu_window_seqlens, int n_windows, const int32_t* cu_seqlens, int n_images, float* embeds) {
  Ctx& C = ctx->c;
  VlmModel& m = *C.vlm;
  FE_CHECK(patch_pos_hw && window_index && cu_window_seqlens && cu_seqlens && n_patches > 0 && n_patches % 4 == 0 && n_windows > 0 && n_images > 0,
           "bad arguments");
  FE_CHECK(cu_window_seqlens[0] == 0 && cu_window_seqlens[n_windows] == n_patches && cu_seqlens[0] == 0 && cu_seqlens[n_images] == n_patches, "segment bounds must cover the patches");
  const int max_win = vlm_longest_segment(cu_window_seqlens, n_windows, "window"), max_full = vlm_longest_segment(cu_seqlens, n_images, "image");
  for (int i = 0; i < n_patches / 4; ++i) FE_CHECK(window_index[i] >= 0 && window_index[i] < n_patches / 4, "window_index out of range");
  const int rows = n_patches / 4;
  vlm_grow_img_embeds(m, rows);
  C.arena.reset();
  float* d_pv = upload(C, pixel_values, (size_t)n_patches * m.vis.patch_dim);
  int* d_pos = upload(C, patch_pos_hw, (size_t)n_patches * 2);
  int* d_widx = upload(C, window_index, (size_t)rows);
  int* d_cw = upload(C, cu_window_seqlens, (size_t)n_windows + 1);
  int* d_cf = upload(C, cu_seqlens, (size_t)n_images + 1);
  vlm_vision_forward(C, m, d_pv, n_patches, d_pos, d_widx, d_cw, n_windows, max_win, d_cf, n_images, max_full, m.img_embeds,
                     pixel_values ? (const bf16*)nullptr : (const bf16*)m.pre_pv);
  m.img_rows = rows;
  const size_t per = (size_t)rows * m.hidden;
  if (embeds) vlm_download_f32(C, m.img_embeds, per, (float*)C.arena.alloc(per * sizeof(float)), embeds);
  FE_HIP(hipStreamSynchronize(C.stream));
}
// shared by fe_vlm2_encode_images and fe_vlm3_encode_images: the LayerNorm tower. `fn` names the entry point in the errors; Qwen2-VL has
// no interpolation taps (interp_idx == interp_w == nullptr) and no DeepStack blocks
void vlm_ln_encode(fe_ctx* ctx, const char* fn, const float* pixel_values, int n_patches, const int32_t* patch_pos_hw, const int32_t* interp_idx,
                   const float* interp_w, const int32_t* cu_seqlens, int n_seg, float* embeds, float* deepstack) {
  Ctx& C = ctx->c;
  VlmModel& m = *C.vlm;
  const VlmLnVisionW& v = m.vis_ln;
  const bool taps = m.cfg.qwen3;
  if (!pixel_values) {
    FE_CHECK(m.pre_pv && m.pre_rows > 0, "%s: no pixel_values and no rows of a fe_vlm_preprocess_rgb", fn);
    FE_CHECK(n_patches == m.pre_rows, "%s: %d patches but the last fe_vlm_preprocess_rgb left %d rows", fn, n_patches, m.pre_rows);
  }
  FE_CHECK(patch_pos_hw && (!taps || (interp_idx && interp_w)) && cu_seqlens && n_patches > 0 && n_patches % 4 == 0 && n_seg > 0, "bad arguments");
  FE_CHECK(cu_seqlens[0] == 0 && cu_seqlens[n_seg] == n_patches, "segment bounds must cover the patches");
  const int max_seg = vlm_longest_segment(cu_seqlens, n_seg, "image");
  for (size_t i = 0; taps && i < (size_t)n_patches * 4; ++i) FE_CHECK(interp_idx[i] >= 0 && interp_idx[i] < v.n_pos, "interp_idx out of range (%d position embeddings)", v.n_pos);
  const int rows = n_patches / 4, nds = (int)v.ds_blocks.size();
  vlm_grow_img_embeds(m, rows);
  if (nds > 0 && rows > m.ds_cap) {
    if (m.ds_feats) (void)hipFree(m.ds_feats);
    m.ds_feats = nullptr; m.ds_cap = 0; m.ds_n = 0;
    FE_HIP(hipMalloc((void**)&m.ds_feats, (size_t)nds * rows * m.hidden * sizeof(bf16)));
    m.ds_cap = rows;
  }
  m.img_rows = 0; m.ds_n = 0;
  C.arena.reset();
  float* d_pv = upload(C, pixel_values, (size_t)n_patches * v.patch_dim);
  int* d_pos = upload(C, patch_pos_hw, (size_t)n_patches * 2);
  int* d_ii = taps ? upload(C, interp_idx, (size_t)n_patches * 4) : nullptr;
  float* d_iw = taps ? upload(C, interp_w, (size_t)n_patches * 4) : nullptr;
  int* d_cu = upload(C, cu_seqlens, (size_t)n_seg + 1);
  vlm_ln_vision_forward(C, m, d_pv, pixel_values ? (const bf16*)nullptr : (const bf16*)m.pre_pv, n_patches, d_pos, d_ii, d_iw, d_cu, n_seg, max_seg, m.img_embeds,
                        nds > 0 ? m.ds_feats : (bf16*)nullptr);
  m.img_rows = rows; m.ds_n = nds;
  const size_t per = (size_t)rows * m.hidden;
  if (embeds || (deepstack && nds > 0)) {
    float* d_f = (float*)C.arena.alloc(per * sizeof(float));
    if (embeds) {
      vlm_download_f32(C, m.img_embeds, per, d_f, embeds);
      FE_HIP(hipStreamSynchronize(C.stream));      // d_f is reused: each copy drains before the next
    }
    for (int k = 0; deepstack && k < nds; ++k) {
      vlm_download_f32(C, m.ds_feats + (size_t)k * m.ds_cap * m.hidden, per, d_f, deepstack + (size_t)k * per);
      FE_HIP(hipStreamSynchronize(C.stream));
    }
  }
  FE_HIP(hipStreamSynchronize(C.stream));
}

// The decoder geometry that the configure call of every family takes, under the caller's lock on the context: checked, then stored.
// `who` prefixes the messages; own_ok and own_rule are the family's own condition and what it adds to the message. sum64: the mrope
// sections must sum to head_dim / 2 (fe_vlm_configure has never asked for that). Returns the configuration for the family's own fields.
VlmConfig& vlm_set_geometry(Ctx& c, const char* who, bool own_ok, const char* own_rule, bool sum64, int n_heads, int n_kv_heads, int head_dim,
                            float rope_theta, float rms_eps, const int* mrope_section) {
  FE_CHECK(n_heads > 0 && n_kv_heads > 0 && n_heads % n_kv_heads == 0 && head_dim == 128 && rope_theta > 0.f && rms_eps > 0.f && mrope_section && own_ok,
           "%s: bad geometry (head_dim must be 128%s)", who, own_rule);
  FE_CHECK(!sum64 || (mrope_section[0] + mrope_section[1] + mrope_section[2] == 64 && mrope_section[0] >= 0 && mrope_section[1] >= 0 && mrope_section[2] >= 0),
           "%s: mrope sections must sum to head_dim / 2", who);
  VlmConfig& g = c.vlm_cfg;
  g.n_heads = n_heads; g.n_kv_heads = n_kv_heads; g.head_dim = head_dim; g.rope_theta = rope_theta; g.rms_eps = rms_eps;
  for (int i = 0; i < 3; ++i) g.mrope[i] = mrope_section[i];
  return g;
}

// tokens (+ optional replacement rows for image tokens) -> embeddings -> decoder -> next tokens; shared by prefill and decode
// pad: a prefill's left padding per sequence (nullptr: none; a prefill always sets the model's pad array, a decode step never touches it)
void vlm_step(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int len, int32_t* next_tokens, float* logits,
              const int32_t* image_rows = nullptr, int n_image_rows = 0, const int32_t* pad = nullptr, bool prefill = true) {
  Ctx& C = ctx->c;
  VlmModel& m = *C.vlm;
  const int rows = n_seq * len;
  C.arena.reset();
  int* d_tok = upload(C, tokens, (size_t)rows);
  int* d_pos = upload(C, position_ids, (size_t)3 * rows);
  int* d_next = (int*)C.arena.alloc((size_t)n_seq * sizeof(int));
  float* d_logits = logits ? (float*)C.arena.alloc((size_t)n_seq * m.vocab * sizeof(float)) : nullptr;
  bf16* x = C.arena.array<bf16>((size_t)rows * m.hidden);
  if (prefill) {
    if (pad) FE_HIP(hipMemcpyAsync(m.pad, pad, (size_t)n_seq * sizeof(int), hipMemcpyHostToDevice, C.stream));
    else FE_HIP(hipMemsetAsync(m.pad, 0, (size_t)n_seq * sizeof(int), C.stream));
  }
  vlm_embed(C, m, d_tok, rows, x);
  if (n_image_rows > 0) {      // inputs_embeds.masked_scatter(image_mask, image_embeds): the merged image embeddings replace the placeholder rows, in order
    int* d_idx = upload(C, image_rows, (size_t)n_image_rows);
    vlm_put_rows(C, x, m.img_embeds, d_idx, n_image_rows, m.hidden);
  }
  // Qwen3-VL prefill: the DeepStack features of the last image encode go to the image rows after the first decoder layers (row -> slot map)
  struct SlotReset { VlmModel& m; ~SlotReset() { m.ds_slot = nullptr; } } slot_reset{m};
  std::vector<int> slot;      // (host source of the copy: alive until the synchronisation below)
  if (prefill && m.cfg.qwen3 && n_image_rows > 0 && m.ds_n > 0) {
    slot.assign((size_t)rows, -1);
    for (int i = 0; i < n_image_rows; ++i) slot[image_rows[i]] = i;
    m.ds_slot = upload(C, slot.data(), (size_t)rows);
  }
  vlm_forward(C, m, x, d_pos, n_seq, len, d_next, d_logits, nullptr, m.last_lp);      // (the chosen tokens' log-probs: fe_vlm_last_logprobs)
  FE_HIP(hipMemcpyAsync(next_tokens, d_next, (size_t)n_seq * sizeof(int), hipMemcpyDeviceToHost, C.stream));
  if (logits) FE_HIP(hipMemcpyAsync(logits, d_logits, (size_t)n_seq * m.vocab * sizeof(float), hipMemcpyDeviceToHost, C.stream));
  FE_HIP(hipStreamSynchronize(C.stream));
}

// fe_vlm_generate and fe_vlm_generate_scored: out_logprobs == nullptr takes the plain selection kernels
int vlm_generate_impl(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int n_steps, int32_t* out_tokens, float* out_logprobs) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    Ctx& C = ctx->c;
    VlmModel& m = *C.vlm;
    FE_CHECK(tokens && position_ids && out_tokens && n_steps > 0 && n_seq == m.cache_B && m.cur_len > 0, "generate: call fe_vlm_prefill for these %d sequences first", n_seq);
    C.arena.reset();
    int* d_tok = upload(C, tokens, (size_t)n_seq);
    int* d_pos = upload(C, position_ids, (size_t)3 * n_seq);
    int* d_out = (int*)C.arena.alloc((size_t)n_steps * n_seq * sizeof(int));
    float* d_lp = out_logprobs ? (float*)C.arena.alloc((size_t)n_steps * n_seq * sizeof(float)) : nullptr;
    vlm_decode_steps(C, m, d_tok, d_pos, n_seq, n_steps, d_out, d_lp);
    FE_HIP(hipMemcpyAsync(out_tokens, d_out, (size_t)n_steps * n_seq * sizeof(int), hipMemcpyDeviceToHost, C.stream));
    if (d_lp) FE_HIP(hipMemcpyAsync(out_logprobs, d_lp, (size_t)n_steps * n_seq * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}
}  // namespace

extern "C" {

// ---- VLM tagger: text decoder of Qwen2.5-VL (models/vlm_tagger.py:163-184 load, :250-259 / :355-360 greedy generate) ----------------
int fe_vlm_vision_configure(fe_ctx* ctx, int n_heads, const int* fullatt_block_indexes, int n_fullatt) {
  return fe_api(ctx, [&] {
    FE_CHECK(n_heads > 0 && n_fullatt >= 0 && n_fullatt <= 8 && (n_fullatt == 0 || fullatt_block_indexes), "vlm_vision_configure: bad arguments (at most 8 full-attention blocks)");
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    VlmConfig& g = ctx->c.vlm_cfg;
    g.vis_heads = n_heads; g.n_fullatt = n_fullatt;
    for (int i = 0; i < n_fullatt; ++i) g.fullatt[i] = fullatt_block_indexes[i];
  });
}

int fe_vlm_encode_images(fe_ctx* ctx, const float* pixel_values, int n_patches, const int32_t* patch_pos_hw, const int32_t* window_index, const int32_t* cu_window_seqlens,
                         int n_windows, const int32_t* cu_seqlens, int n_images, float* embeds) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm || !ctx->c.vlm->vis.present) { ctx->c.err = "vlm vision tower not loaded (checkpoint had no model.visual.* tensors)"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(pixel_values, "bad arguments");
    vlm_encode(ctx, pixel_values, n_patches, patch_pos_hw, window_index, cu_window_seqlens, n_windows, cu_seqlens, n_images, embeds);
    return FE_OK;
  });
}
int fe_vlm_encode_preprocessed(fe_ctx* ctx, const int32_t* patch_pos_hw, const int32_t* window_index, const int32_t* cu_window_seqlens, int n_windows,
                               const int32_t* cu_seqlens, int n_images, float* embeds) {
  return fe_api(ctx, OnError::VlmCapacity, [&] {
    if (!ctx->c.vlm || !ctx->c.vlm->vis.present) { ctx->c.err = "vlm vision tower not loaded (checkpoint had no model.visual.* tensors)"; return FE_ERR_NOT_LOADED; }
    VlmModel& m = *ctx->c.vlm;
    FE_CHECK(m.pre_pv && m.pre_rows > 0 && cu_seqlens && n_images > 0, "encode_preprocessed: call fe_vlm_preprocess_rgb first");
    vlm_encode(ctx, nullptr, m.pre_rows, patch_pos_hw, window_index, cu_window_seqlens, n_windows, cu_seqlens, n_images, embeds);
    return FE_OK;
  });
}
int fe_vlm_preprocess_rgb(fe_ctx* ctx, const uint8_t* rgb, int n_images, const int32_t* sizes, const float* mean, const float* stdv, float* pixel_values) {
  return fe_api(ctx, OnError::VlmCapacity, [&] {
    const bool q3 = ctx->c.vlm && ctx->c.vlm->cfg.qwen3;      // Qwen3-VL: 16-pixel patches (32-pixel merge blocks)
    const bool q2 = ctx->c.vlm && ctx->c.vlm->cfg.qwen2;      // Qwen2-VL: the 14-pixel patches of Qwen2.5-VL
    if (!ctx->c.vlm || !(q3 || q2 ? ctx->c.vlm->vis_ln.present : ctx->c.vlm->vis.present)) { ctx->c.err = "vlm vision tower not loaded (checkpoint had no model.visual.* tensors)"; return FE_ERR_NOT_LOADED; }
    Ctx& C = ctx->c;
    VlmModel& m = *C.vlm;
    FE_CHECK(rgb && sizes && mean && stdv && n_images > 0, "bad arguments");
    const int P = q3 ? 16 : 14, F = 2 * P, PD = 6 * P * P;
    const int tower_pd = q3 || q2 ? m.vis_ln.patch_dim : m.vis.patch_dim;
    FE_CHECK(tower_pd == PD, "preprocess_rgb: the vision tower takes %d-value patches (3 x 2 x %d x %d built)", tower_pd, P, P);
    size_t in_b = 0, rows = 0, px_max = 0;
    for (int i = 0; i < n_images; ++i) {
      const int h = sizes[4 * i], w = sizes[4 * i + 1], oh = sizes[4 * i + 2], ow = sizes[4 * i + 3];
      FE_CHECK(h > 0 && w > 0 && oh >= F && ow >= F && oh % F == 0 && ow % F == 0 && (size_t)oh * ow <= ((size_t)1 << 26),
               "preprocess_rgb: image %d: %dx%d -> %dx%d (target sides must be positive multiples of %d)", i, h, w, oh, ow, F);
      in_b += (size_t)h * w * 3;
      rows += (size_t)(oh / P) * (ow / P);
      px_max = std::max(px_max, (size_t)oh * ow * 3);
    }
    FE_CHECK(rows < ((size_t)1 << 31) / PD, "preprocess_rgb: %zu patches", rows);
    // the processor's arithmetic, once per (channel, value): float32(float64(u) * (1 / 255)), then float32 (x - mean) / std
    std::vector<float> lut(3 * 256);
    for (int c = 0; c < 3; ++c)
      for (int u = 0; u < 256; ++u) {
        const float x = (float)((double)u * (1.0 / 255.0));
        lut[c * 256 + u] = (x - mean[c]) / stdv[c];
      }
    if ((int)rows > m.pre_cap) {
      if (m.pre_pv) (void)hipFree(m.pre_pv);
      m.pre_pv = nullptr; m.pre_cap = 0; m.pre_rows = 0;
      FE_HIP(hipMalloc((void**)&m.pre_pv, rows * PD * sizeof(bf16)));
      m.pre_cap = (int)rows;
    }
    m.pre_rows = 0;
    C.arena.reset();
    uint8_t* d_in = upload(C, rgb, in_b);
    float* d_lut = upload(C, lut.data(), lut.size());
    uint8_t* d_img = (uint8_t*)C.arena.alloc(px_max);
    float* d_f = pixel_values ? (float*)C.arena.alloc(rows * PD * sizeof(float)) : nullptr;
    size_t off = 0, row0 = 0;
    for (int i = 0; i < n_images; ++i) {      // one resample pair and one patchify launch per image (tagger batches are a few images)
      const int h = sizes[4 * i], w = sizes[4 * i + 1], oh = sizes[4 * i + 2], ow = sizes[4 * i + 3];
      resize_u8(C, d_in + off, 1, h, w, oh, ow, FE_BICUBIC, 0, oh, 0, ow, d_img);
      if (q3) vlm_patchify16(C, d_img, oh, ow, d_lut, m.pre_pv + row0 * PD, d_f ? d_f + row0 * PD : nullptr);
      else vlm_patchify(C, d_img, oh, ow, d_lut, m.pre_pv + row0 * PD, d_f ? d_f + row0 * PD : nullptr);
      off += (size_t)h * w * 3;
      row0 += (size_t)(oh / P) * (ow / P);
    }
    if (pixel_values) FE_HIP(hipMemcpyAsync(pixel_values, d_f, rows * PD * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    m.pre_rows = (int)rows;
    return FE_OK;
  });
}
int fe_vlm_configure(fe_ctx* ctx, int n_heads, int n_kv_heads, int head_dim, float rope_theta, float rms_eps, const int* mrope_section) {
  return fe_api(ctx, [&] {
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    VlmConfig& g = vlm_set_geometry(ctx->c, "vlm_configure", true, "", false, n_heads, n_kv_heads, head_dim, rope_theta, rms_eps, mrope_section);
    g.qwen3 = false; g.qwen2 = false; g.n_deepstack = 0;      // (the Qwen2.5-VL family: what a context builds unless fe_vlm2_ / fe_vlm3_configure said otherwise)
  });
}
int fe_vlm_set_weight_format(fe_ctx* ctx, int format) {
  return fe_api(ctx, [&] {
    FE_CHECK(format == FE_VLM_WEIGHTS_BF16 || format == FE_VLM_WEIGHTS_E4M3, "vlm_set_weight_format: %d (FE_VLM_WEIGHTS_BF16 or FE_VLM_WEIGHTS_E4M3)", format);
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    ctx->c.vlm_weight_format = format;
  });
}
int fe_vlm_weight_info(fe_ctx* ctx, int64_t* info4) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(info4, "bad arguments");
    const VlmModel& m = *ctx->c.vlm;
    info4[0] = m.weight_format; info4[1] = m.weight_bytes; info4[2] = m.scale_bytes; info4[3] = m.quant_rows;
    return FE_OK;
  });
}
int fe_vlm_set_kv_format(fe_ctx* ctx, int format) {
  return fe_api(ctx, [&] {
    FE_CHECK(format == FE_VLM_KV_BF16 || format == FE_VLM_KV_E4M3 || format == FE_VLM_KV_BF16_E4M3,
             "vlm_set_kv_format: %d (FE_VLM_KV_BF16, FE_VLM_KV_E4M3 or FE_VLM_KV_BF16_E4M3)", format);
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    ctx->c.vlm_kv_format = format;
    // a live cache in another format is gone: decode calls fail until the next prefill
    if (ctx->c.vlm && ctx->c.vlm->cache_B > 0 && ctx->c.vlm->kv_format != format) {
      FE_HIP(hipStreamSynchronize(ctx->c.stream));
      ctx->c.vlm->release_cache();
    }
  });
}
int fe_vlm_kv_info(fe_ctx* ctx, int64_t* info4) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(info4, "bad arguments");
    const VlmModel& m = *ctx->c.vlm;
    info4[0] = ctx->c.vlm_kv_format; info4[1] = m.kv_token_bytes(ctx->c.vlm_kv_format); info4[2] = m.cache_bytes; info4[3] = m.max_seq;
    return FE_OK;
  });
}
int fe_vlm_kv_rows(fe_ctx* ctx, int layer, int seq, int kv_head, int pos0, int n, float* k, float* v) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    Ctx& C = ctx->c;
    const VlmModel& m = *C.vlm;
    FE_CHECK(m.cache_B > 0 && m.cur_len > 0, "kv_rows: call fe_vlm_prefill first");
    FE_CHECK(k && v && layer >= 0 && layer < (int)m.layers.size() && seq >= 0 && seq < m.cache_B && kv_head >= 0 && kv_head < m.cfg.n_kv_heads && pos0 >= 0 && n > 0 &&
             pos0 + n <= m.cur_len, "kv_rows: layer %d, sequence %d, kv head %d, positions %d .. %d outside the live cache (%d positions)", layer, seq, kv_head, pos0,
             pos0 + n - 1, m.cur_len);
    const size_t row0 = ((size_t)seq * m.cfg.n_kv_heads + kv_head) * m.max_seq + pos0, cnt = (size_t)n * 128;
    for (int which = 0; which < 2; ++which) {
      float* out = which ? v : k;
      const bf16* src = which ? m.vcache[layer] : m.kcache[layer];
      if (m.kv_format == FE_VLM_KV_E4M3) {      // codes and scales to the host, decoded by fp8_core.h
        std::vector<uint8_t> codes(cnt);
        std::vector<float> sc((size_t)n);
        FE_HIP(hipMemcpyAsync(codes.data(), (const uint8_t*)src + row0 * 128, cnt, hipMemcpyDeviceToHost, C.stream));
        FE_HIP(hipMemcpyAsync(sc.data(), (which ? m.vscale[layer] : m.kscale[layer]) + row0, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, C.stream));
        FE_HIP(hipStreamSynchronize(C.stream));
        for (size_t i = 0; i < cnt; ++i) out[i] = fp8::e4m3_decode(codes[i]) * sc[i / 128];
      } else {
        std::vector<uint16_t> h(cnt);
        FE_HIP(hipMemcpyAsync(h.data(), src + row0 * 128, cnt * sizeof(uint16_t), hipMemcpyDeviceToHost, C.stream));
        FE_HIP(hipStreamSynchronize(C.stream));
        for (size_t i = 0; i < cnt; ++i) { const uint32_t u = (uint32_t)h[i] << 16; memcpy(&out[i], &u, 4); }
      }
    }
    return FE_OK;
  });
}
// ---- Qwen3-VL: the same decoder entry points serve the family the next commit builds --------------------------------------------------------
int fe_vlm3_configure(fe_ctx* ctx, int n_heads, int n_kv_heads, int head_dim, float rope_theta, float rms_eps, const int* mrope_section, int vis_heads,
                      const int* deepstack_indexes, int n_deepstack) {
  return fe_api(ctx, [&] {
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    VlmConfig& g = vlm_set_geometry(ctx->c, "vlm3_configure", vis_heads > 0 && n_deepstack >= 0 && n_deepstack <= 8 && (n_deepstack == 0 || deepstack_indexes),
                                    ", at most 8 DeepStack levels", true, n_heads, n_kv_heads, head_dim, rope_theta, rms_eps, mrope_section);
    g.vis_heads = vis_heads;
    g.qwen3 = true; g.qwen2 = false;
    g.n_deepstack = n_deepstack;
    for (int i = 0; i < n_deepstack; ++i) g.deepstack[i] = deepstack_indexes[i];
  });
}
int fe_vlm3_encode_images(fe_ctx* ctx, const float* pixel_values, int n_patches, const int32_t* patch_pos_hw, const int32_t* interp_idx, const float* interp_w,
                          const int32_t* cu_seqlens, int n_seg, float* embeds, float* deepstack) {
  return fe_api(ctx, OnError::VlmCapacity, [&] {
    if (!ctx->c.vlm || !ctx->c.vlm->cfg.qwen3 || !ctx->c.vlm->vis_ln.present) {
      ctx->c.err = "qwen3-vl vision tower not loaded (fe_vlm3_configure before the commit; the checkpoint needs model.visual.*)";
      return FE_ERR_NOT_LOADED;
    }
    vlm_ln_encode(ctx, "vlm3_encode_images", pixel_values, n_patches, patch_pos_hw, interp_idx, interp_w, cu_seqlens, n_seg, embeds, deepstack);
    return FE_OK;
  });
}
// ---- Qwen2-VL (the composition model, models/vlm_composition.py): the Qwen2.5-VL decoder entry points, a tower of its own ---------------------
int fe_vlm2_configure(fe_ctx* ctx, int n_heads, int n_kv_heads, int head_dim, float rope_theta, float rms_eps, const int* mrope_section, int vis_heads) {
  return fe_api(ctx, [&] {
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    VlmConfig& g = vlm_set_geometry(ctx->c, "vlm2_configure", vis_heads > 0, "", true, n_heads, n_kv_heads, head_dim, rope_theta, rms_eps, mrope_section);
    g.vis_heads = vis_heads;
    g.qwen2 = true; g.qwen3 = false; g.n_deepstack = 0;
  });
}
int fe_vlm2_encode_images(fe_ctx* ctx, const float* pixel_values, int n_patches, const int32_t* patch_pos_hw, const int32_t* cu_seqlens, int n_seg, float* embeds) {
  return fe_api(ctx, OnError::VlmCapacity, [&] {
    if (!ctx->c.vlm || !ctx->c.vlm->cfg.qwen2 || !ctx->c.vlm->vis_ln.present) {
      ctx->c.err = "qwen2-vl vision tower not loaded (fe_vlm2_configure before the commit; the checkpoint needs model.visual.*)";
      return FE_ERR_NOT_LOADED;
    }
    vlm_ln_encode(ctx, "vlm2_encode_images", pixel_values, n_patches, patch_pos_hw, nullptr, nullptr, cu_seqlens, n_seg, embeds, nullptr);
    return FE_OK;
  });
}
int fe_vlm_vision_dims(fe_ctx* ctx, int* dims) {
  return fe_api(ctx, [&] {
    const bool q3 = ctx->c.vlm && ctx->c.vlm->cfg.qwen3, q2 = ctx->c.vlm && ctx->c.vlm->cfg.qwen2;
    if (!ctx->c.vlm || !(q3 || q2 ? ctx->c.vlm->vis_ln.present : ctx->c.vlm->vis.present)) { ctx->c.err = "vlm vision tower not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(dims, "bad arguments");
    const VlmModel& m = *ctx->c.vlm;
    if (q3) {
      int side = 0;
      while ((side + 1) * (side + 1) <= m.vis_ln.n_pos) ++side;
      dims[0] = m.vis_ln.patch_side; dims[1] = m.vis_ln.patch_dim; dims[2] = (int)m.vis_ln.ds_blocks.size(); dims[3] = side * side == m.vis_ln.n_pos ? side : 0;
    } else {
      dims[0] = 14; dims[1] = q2 ? m.vis_ln.patch_dim : m.vis.patch_dim; dims[2] = 0; dims[3] = 0;
    }
    return FE_OK;
  });
}
int fe_vlm_dims(fe_ctx* ctx, int* dims) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(dims, "bad arguments");
    const VlmModel& m = *ctx->c.vlm;
    dims[0] = m.vocab; dims[1] = m.hidden; dims[2] = (int)m.layers.size(); dims[3] = m.cfg.n_heads; dims[4] = m.cfg.n_kv_heads; dims[5] = m.inter;
    dims[6] = m.max_seq; dims[7] = m.cur_len;
    return FE_OK;
  });
}

int fe_vlm_prefill(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int len, int max_seq, int32_t* next_tokens, float* logits) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(tokens && position_ids && next_tokens && n_seq > 0 && len > 0 && max_seq >= len && max_seq <= 8192, "bad arguments (max_seq <= 8192)");
    ctx->c.vlm->reserve_cache(n_seq, max_seq, ctx->c.vlm_kv_format);
    ctx->c.vlm->cur_len = 0;
    vlm_step(ctx, tokens, position_ids, n_seq, len, next_tokens, logits);
    return FE_OK;
  });
}
int fe_vlm_prefill_images(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int len, int max_seq, const int32_t* image_rows, int n_image_rows,
                          int32_t* next_tokens, float* logits) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    VlmModel& m = *ctx->c.vlm;
    FE_CHECK(tokens && position_ids && next_tokens && n_seq > 0 && len > 0 && max_seq >= len && max_seq <= 8192, "bad arguments (max_seq <= 8192)");
    FE_CHECK(n_image_rows == 0 || (image_rows && n_image_rows == m.img_rows), "prefill_images: %d placeholder rows but the last fe_vlm_encode_images left %d embeddings",
             n_image_rows, m.img_rows);
    for (int i = 0; i < n_image_rows; ++i) FE_CHECK(image_rows[i] >= 0 && image_rows[i] < n_seq * len, "prefill_images: row index out of range");
    m.reserve_cache(n_seq, max_seq, ctx->c.vlm_kv_format);
    m.cur_len = 0;
    vlm_step(ctx, tokens, position_ids, n_seq, len, next_tokens, logits, image_rows, n_image_rows);
    return FE_OK;
  });
}
int fe_vlm_prefill_images_padded(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int len, int max_seq, const int32_t* pad,
                                 const int32_t* image_rows, int n_image_rows, int32_t* next_tokens, float* logits) {
  return fe_api(ctx, OnError::VlmCapacity, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    VlmModel& m = *ctx->c.vlm;
    FE_CHECK(tokens && position_ids && pad && next_tokens && n_seq > 0 && len > 0 && max_seq >= len && max_seq <= 8192, "bad arguments (max_seq <= 8192)");
    for (int b = 0; b < n_seq; ++b) FE_CHECK(pad[b] >= 0 && pad[b] < len, "prefill_images_padded: sequence %d: pad %d of %d positions (at least one real token)", b, pad[b], len);
    FE_CHECK(n_image_rows == 0 || (image_rows && n_image_rows == m.img_rows), "prefill_images_padded: %d placeholder rows but the last image encode left %d embeddings",
             n_image_rows, m.img_rows);
    for (int i = 0; i < n_image_rows; ++i)
      FE_CHECK(image_rows[i] >= 0 && image_rows[i] < n_seq * len && image_rows[i] % len >= pad[image_rows[i] / len], "prefill_images_padded: row index %d out of range or in the pad", image_rows[i]);
    m.reserve_cache(n_seq, max_seq, ctx->c.vlm_kv_format);
    m.cur_len = 0;
    vlm_step(ctx, tokens, position_ids, n_seq, len, next_tokens, logits, image_rows, n_image_rows, pad);
    return FE_OK;
  });
}

// fe_vlm_generate(_scored) that stops: the same device loop, with the stop rule of VlmUntil (model_vlm.hip). Steps that were not run are
// filled in here with what they would have held: each sequence's EOS id, NaN log-probs.
int fe_vlm_generate_until(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int max_steps, const int32_t* eos_ids, int n_eos, int poll,
                          int32_t* out_tokens, float* out_logprobs, int* steps_run) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    Ctx& C = ctx->c;
    VlmModel& m = *C.vlm;
    FE_CHECK(tokens && position_ids && out_tokens && steps_run && max_steps > 0 && n_seq == m.cache_B && m.cur_len > 0, "generate_until: call fe_vlm_prefill for these %d sequences first", n_seq);
    FE_CHECK(n_eos >= 0 && n_eos <= 8 && (n_eos == 0 || eos_ids) && poll >= 1, "generate_until: at most 8 eos ids, poll >= 1");
    *steps_run = 0;
    VlmUntil u;
    u.n_eos = n_eos; u.poll = poll;
    for (int e = 0; e < n_eos; ++e) u.eos[e] = eos_ids[e];
    std::vector<int> fin((size_t)n_seq + 1, -1);      // [n_seq] the EOS id of a finished sequence, then the running count
    int live = 0;
    for (int b = 0; b < n_seq; ++b) {      // a first token that already is an EOS id: finished before the first step
      for (int e = 0; e < n_eos; ++e) if (tokens[b] == eos_ids[e]) fin[b] = tokens[b];
      live += fin[b] < 0;
    }
    fin[n_seq] = live;
    C.arena.reset();
    int* d_tok = upload(C, tokens, (size_t)n_seq);
    int* d_pos = upload(C, position_ids, (size_t)3 * n_seq);
    int* d_out = (int*)C.arena.alloc((size_t)max_steps * n_seq * sizeof(int));
    float* d_lp = out_logprobs ? (float*)C.arena.alloc((size_t)max_steps * n_seq * sizeof(float)) : nullptr;
    int* d_fin = upload(C, fin.data(), fin.size());
    u.fin_dev = d_fin; u.live_dev = d_fin + n_seq;
    vlm_decode_steps(C, m, d_tok, d_pos, n_seq, max_steps, d_out, d_lp, &u);
    const int ran = u.steps_run;
    FE_HIP(hipMemcpyAsync(out_tokens, d_out, (size_t)ran * n_seq * sizeof(int), hipMemcpyDeviceToHost, C.stream));
    if (d_lp) FE_HIP(hipMemcpyAsync(out_logprobs, d_lp, (size_t)ran * n_seq * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(fin.data(), d_fin, (size_t)n_seq * sizeof(int), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    for (int s = ran; s < max_steps; ++s)      // (reached only when every sequence has finished)
      for (int b = 0; b < n_seq; ++b) {
        out_tokens[(size_t)s * n_seq + b] = fin[b];
        if (out_logprobs) out_logprobs[(size_t)s * n_seq + b] = NAN;
      }
    *steps_run = ran;
    return FE_OK;
  });
}
int fe_vlm_generate(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int n_steps, int32_t* out_tokens) {
  return vlm_generate_impl(ctx, tokens, position_ids, n_seq, n_steps, out_tokens, nullptr);
}
int fe_vlm_generate_scored(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int n_steps, int32_t* out_tokens, float* out_logprobs) {
  if (ctx && !out_logprobs) { ctx->c.err = "generate_scored: out_logprobs is null (fe_vlm_generate takes no scores)"; return FE_ERR_INVALID; }
  return vlm_generate_impl(ctx, tokens, position_ids, n_seq, n_steps, out_tokens, out_logprobs);
}
int fe_vlm_last_logprobs(fe_ctx* ctx, float* out) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    Ctx& C = ctx->c;
    const VlmModel& m = *C.vlm;
    FE_CHECK(out && m.cache_B > 0 && m.last_lp, "last_logprobs: no prefill yet");
    FE_HIP(hipMemcpyAsync(out, m.last_lp, (size_t)m.cache_B * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}
int fe_vlm_decode_step(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int32_t* next_tokens, float* logits) {
  return fe_api(ctx, [&] {
    if (!ctx->c.vlm) { ctx->c.err = "vlm weights not loaded"; return FE_ERR_NOT_LOADED; }
    VlmModel& m = *ctx->c.vlm;
    FE_CHECK(tokens && position_ids && next_tokens && n_seq == m.cache_B && m.cur_len > 0, "decode_step: call fe_vlm_prefill for these %d sequences first", n_seq);
    FE_CHECK(m.cur_len < m.max_seq, "decode_step: the KV cache is full (%d positions)", m.max_seq);
    vlm_step(ctx, tokens, position_ids, n_seq, 1, next_tokens, logits, nullptr, 0, nullptr, false);
    return FE_OK;
  });
}

}  // extern "C"
