// C ABI: image-level work without a model - PIL resize and reduce, thumbnails, JPEG encode / probe / decode, pHash, statistics, lines,
// contours, subject region.
#include "capi_internal.h"
#include "lines_host.h"
#include "phash_mixed_plan.h"
#include "thumb_mixed_core.h"
#include <chrono>
#include <thread>

namespace {
// What fe_resize_u8, fe_resize_u8_box and fe_reduce_u8 do around their launch: a host batch goes through the arena, in and out.
template <class Launch>
void resize_staged(Ctx& C, const uint8_t* src, size_t in_b, uint8_t* dst, size_t out_b, int on_device, Launch&& launch) {
  C.arena.reset();
  const uint8_t* d_in = resident(C, src, in_b, on_device);
  uint8_t* d_out = on_device ? dst : (uint8_t*)C.arena.alloc(out_b);
  launch(d_in, d_out);
  if (!on_device) FE_HIP(hipMemcpyAsync(dst, d_out, out_b, hipMemcpyDeviceToHost, C.stream));
  FE_HIP(hipStreamSynchronize(C.stream));
}

// ---- thumbnails: reduce -> boxed LANCZOS resize -> baseline JPEG, one chain on the device ----------------------------------------
struct ThumbPlan { int oh, ow, fx, fy; int rbox[4]; float box[4]; int tall; };
ThumbPlan make_thumb_plan(int oh, int ow, int fx, int fy, const int32_t* reduce_box, const float* resize_box, int tall) {
  ThumbPlan p;
  p.oh = oh; p.ow = ow; p.fx = fx; p.fy = fy; p.tall = tall;
  for (int i = 0; i < 4; ++i) { p.rbox[i] = reduce_box ? reduce_box[i] : 0; p.box[i] = resize_box[i]; }
  return p;
}
// plan NULL: the images are encoded as they are. out [n][cap] and lengths [n] are host buffers.
void thumbnail_run(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device, const ThumbPlan* plan, int quality,
                   uint8_t* out, size_t cap, int32_t* lengths) {
  Ctx& C = ctx->c;
  int rh = h, rw = w, oh = h, ow = w;
  bool do_reduce = false, do_resize = false;
  if (plan) {
    oh = plan->oh; ow = plan->ow;
    do_reduce = plan->fx > 1 || plan->fy > 1;
    if (do_reduce) {
      FE_CHECK(plan->rbox[0] >= 0 && plan->rbox[1] >= 0 && plan->rbox[2] <= w && plan->rbox[3] <= h && plan->rbox[0] < plan->rbox[2] && plan->rbox[1] < plan->rbox[3],
               "thumbnail: reduce box outside the image or empty");
      rw = (plan->rbox[2] - plan->rbox[0] + plan->fx - 1) / plan->fx;
      rh = (plan->rbox[3] - plan->rbox[1] + plan->fy - 1) / plan->fy;
    }
    do_resize = oh != rh || ow != rw || plan->box[0] != 0.0f || plan->box[1] != 0.0f || plan->box[2] != (float)rw || plan->box[3] != (float)rh;
  }
  FE_CHECK(oh > 0 && ow > 0 && oh <= 65535 && ow <= 65535, "thumbnail: bad output size %d x %d", ow, oh);
  const size_t dcap = std::min(cap, jpeg_bound(oh, ow));      // no encode is longer, so the device rows need not be
  const size_t per_in = (size_t)h * w * 3;
  const size_t per = (do_reduce ? (size_t)rh * rw * 3 : 0) + (do_resize ? (size_t)rh * ow * 3 + (size_t)rw * oh * 3 + (size_t)oh * ow * 3 : 0) +
                     jpeg_scratch_bytes(oh, ow) + dcap + 2048;
  const size_t budget = std::min<size_t>((size_t)1 << 30, C.arena.capacity() - C.arena.capacity() / 8);
  int mb = (int)std::max<size_t>(1, std::min<size_t>(256, budget / per));
  if (!on_device) mb = (int)std::max<size_t>(1, std::min<size_t>(mb, ((size_t)1 << 30) / per_in));
  std::vector<int32_t> lens(n);
  ImageStager st(ctx, img, n, per_in, mb, on_device);
  bool overflow = false;
  for (int k = 0; k < st.chunks(); ++k) {
    const int i0 = k * mb, nb = st.count(k);
    C.arena.reset();
    const uint8_t* cur = st.get(k);
    if (do_reduce) {
      uint8_t* d = (uint8_t*)C.arena.alloc((size_t)nb * rh * rw * 3);
      reduce_u8(C, cur, nb, h, w, plan->fx, plan->fy, plan->rbox, d);
      cur = d;
    }
    if (do_resize) {
      uint8_t* d = (uint8_t*)C.arena.alloc((size_t)nb * oh * ow * 3);
      if (plan->tall) {      // Image.resize's two calls for images more than 100 times taller than wide: rows first, then columns
        uint8_t* mid = (uint8_t*)C.arena.alloc((size_t)nb * oh * rw * 3);
        const float b1[4] = {0.0f, plan->box[1], (float)rw, plan->box[3]}, b2[4] = {plan->box[0], 0.0f, plan->box[2], (float)oh};
        resize_u8_box(C, cur, nb, rh, rw, oh, rw, FE_FILTER_LANCZOS, b1, mid);
        resize_u8_box(C, mid, nb, oh, rw, oh, ow, FE_FILTER_LANCZOS, b2, d);
      } else {
        resize_u8_box(C, cur, nb, rh, rw, oh, ow, FE_FILTER_LANCZOS, plan->box, d);
      }
      cur = d;
    }
    uint8_t* d_out = (uint8_t*)C.arena.alloc((size_t)nb * dcap);
    int32_t* d_len = (int32_t*)C.arena.alloc((size_t)nb * sizeof(int32_t));
    launch_jpeg_encode(C, cur, nb, oh, ow, bgr ? 1 : 0, quality, d_out, dcap, d_len);
    st.done(k);
    FE_HIP(hipMemcpyAsync(lens.data() + i0, d_len, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    for (int i = 0; i < nb; ++i) {
      const int32_t len = lens[i0 + i];
      lengths[i0 + i] = len;
      if (len <= 0 || (size_t)len > cap) { overflow = true; continue; }
      FE_HIP(hipMemcpyAsync(out + (size_t)(i0 + i) * cap, d_out + (size_t)i * dcap, (size_t)len, hipMemcpyDeviceToHost, C.stream));
    }
    FE_HIP(hipStreamSynchronize(C.stream));   // the arena is recycled by the next chunk
  }
  if (overflow) {
    char b[160];
    snprintf(b, sizeof(b), "jpeg: an image needs more than the %zu bytes of its output row (fe_jpeg_bound(%d, %d) = %zu always fits)", cap, oh, ow, jpeg_bound(oh, ow));
    throw CapacityError(b);
  }
}

bool jpeg_scale_ok(int scale) { return scale == 1 || scale == 2 || scale == 4 || scale == 8; }

// the two division tables of cv2's 8-bit HSV conversion, made once per context (fe_image_stats, fe_subject_region)
void ensure_hsv_tables(fe_ctx* ctx) {
  if (ctx->hsv_sdiv) return;
  std::vector<int> sd, hd;
  cv_hsv_tables(sd, hd);
  FE_HIP(hipMalloc((void**)&ctx->hsv_sdiv, 256 * sizeof(int)));
  ctx->misc_allocs.push_back(ctx->hsv_sdiv);
  FE_HIP(hipMalloc((void**)&ctx->hsv_hdiv, 256 * sizeof(int)));
  ctx->misc_allocs.push_back(ctx->hsv_hdiv);
  FE_HIP(hipMemcpy(ctx->hsv_sdiv, sd.data(), 256 * sizeof(int), hipMemcpyHostToDevice));
  FE_HIP(hipMemcpy(ctx->hsv_hdiv, hd.data(), 256 * sizeof(int), hipMemcpyHostToDevice));
}

// the DCT-II cosine table of the pHash entry points, made once per context
void ensure_phash_cos(fe_ctx* ctx) {
  if (ctx->phash_cos) return;
  double tab[8 * 32];
  phash_cos_table(tab);
  FE_HIP(hipMalloc((void**)&ctx->phash_cos, sizeof(tab)));
  ctx->misc_allocs.push_back(ctx->phash_cos);
  FE_HIP(hipMemcpy(ctx->phash_cos, tab, sizeof(tab), hipMemcpyHostToDevice));
}

// fe_phash_mixed behind its argument checks: descriptors and pool of the whole list, then chunk by chunk through the arena
void phash_mixed_run(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, uint64_t* hashes, uint8_t* small_out,
                     double* dct_out) {
  Ctx& C = ctx->c;
  PhashTables tables;
  std::vector<PhashDesc> descs(n);
  for (int i = 0; i < n; ++i) FE_CHECK(tables.describe(hw[2 * i], hw[2 * i + 1], descs[i]), "fe_phash_mixed: image %d: a coefficient window leaves the axis", i);
  const mixed_list::Cuts cuts = phash_cuts(hw, n, small_out != nullptr, dct_out != nullptr, !on_device, tables.pool.size(), C.arena.capacity());
  if (cuts.bad_image >= 0) throw_image_too_large("fe_phash_mixed", cuts.bad_image, hw, cuts.bad_bytes, C.arena.capacity());
  ensure_phash_cos(ctx);
  C.arena.reset();
  const int32_t* d_pool = upload(C, tables.pool.data(), tables.pool.size());
  const size_t mark = C.arena.mark();
  std::vector<size_t> offs;
  int i0 = 0;
  for (const int i1 : cuts.ends) {
    size_t rows = 0;
    int max_w = 1, any_tall = 0;
    for (int i = i0; i < i1; ++i) {
      descs[i].first_row = (uint32_t)rows;
      rows += (size_t)phash_tmp_rows(hw[2 * i], hw[2 * i + 1]);
      any_tall |= descs[i].tall;
      max_w = std::max(max_w, (int)hw[2 * i + 1]);
    }
    const int nb = i1 - i0;
    const size_t stage_b = on_device ? 0 : mixed_list::staged_offsets(hw, i0, i1, true, offs);
    C.arena.rewind(mark);
    PhashDesc* d_desc = (PhashDesc*)C.arena.alloc((size_t)nb * sizeof(PhashDesc));
    uint8_t* d_tmp = (uint8_t*)C.arena.alloc(rows * kPhashSide);
    uint64_t* d_hash = (uint64_t*)C.arena.alloc((size_t)nb * sizeof(uint64_t));
    uint8_t* d_small = small_out ? (uint8_t*)C.arena.alloc((size_t)nb * 1024) : nullptr;
    double* d_dct = dct_out ? (double*)C.arena.alloc((size_t)nb * 64 * sizeof(double)) : nullptr;
    uint8_t* d_stage = on_device ? nullptr : (uint8_t*)C.arena.alloc(stage_b);
    stage_images(C, images, hw, i0, i1, on_device, d_stage, offs.data(), [&](int i, const uint8_t* src) { descs[i].src = src; });
    FE_HIP(hipMemcpyAsync(d_desc, descs.data() + i0, (size_t)nb * sizeof(PhashDesc), hipMemcpyHostToDevice, C.stream));
    launch_phash_mixed(C, d_desc, nb, rows, max_w, any_tall, order == FE_ORDER_BGR, d_pool, d_tmp, ctx->phash_cos, d_hash, d_small, d_dct);
    FE_HIP(hipMemcpyAsync(hashes + i0, d_hash, (size_t)nb * sizeof(uint64_t), hipMemcpyDeviceToHost, C.stream));
    if (small_out) FE_HIP(hipMemcpyAsync(small_out + (size_t)i0 * 1024, d_small, (size_t)nb * 1024, hipMemcpyDeviceToHost, C.stream));
    if (dct_out) FE_HIP(hipMemcpyAsync(dct_out + (size_t)i0 * 64, d_dct, (size_t)nb * 64 * sizeof(double), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));   // the arena is recycled by the next chunk
    i0 = i1;
  }
}

// Brings the contour records of one micro-batch to the host: counts [nb] exact; records [nb][max_contours][8], per image the first
// max_contours in descending start_index order. The device list holds every qualifying contour (its capacity is the largest number
// of components an image can have), in the order the walks finished, so the order is made here.
void collect_contours(fe_ctx* ctx, const ContourScratch& sc, int nb, int h, int w, int max_contours, long long* records, int* counts) {
  Ctx& C = ctx->c;
  const int cap = contour_work_cap(h, w);
  std::vector<int> found(nb), listed(nb);
  int err = 0;
  FE_HIP(hipMemcpyAsync(found.data(), sc.rec_count, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, C.stream));
  FE_HIP(hipMemcpyAsync(listed.data(), sc.work_count, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, C.stream));
  FE_HIP(hipMemcpyAsync(&err, sc.error, sizeof(int), hipMemcpyDeviceToHost, C.stream));
  FE_HIP(hipStreamSynchronize(C.stream));
  FE_CHECK(!(err & 1), "contours: a border walk did not close within 8 * pixels + 8 steps");
  FE_CHECK(!(err & 2), "contours: more component roots than an image can hold");
  std::vector<std::vector<long long>> got(nb);
  for (int i = 0; i < nb; ++i) {
    FE_CHECK(found[i] >= 0 && found[i] <= listed[i] && listed[i] <= cap, "contours: inconsistent counts (%d of %d, room %d)", found[i], listed[i], cap);
    counts[i] = found[i];
  }
  for (int i = 0; i < nb; ++i) {      // nothing below throws while a copy into `got` is in flight
    if (!found[i]) continue;
    got[i].resize((size_t)found[i] * FE_CONTOUR_RECORD);
    FE_HIP(hipMemcpyAsync(got[i].data(), sc.recs + (size_t)i * cap * FE_CONTOUR_RECORD, got[i].size() * sizeof(long long), hipMemcpyDeviceToHost,
                          C.stream));
  }
  FE_HIP(hipStreamSynchronize(C.stream));
  struct Rec { long long f[FE_CONTOUR_RECORD]; };
  for (int i = 0; i < nb; ++i) {
    if (!found[i]) continue;
    Rec* r = reinterpret_cast<Rec*>(got[i].data());
    std::sort(r, r + found[i], [](const Rec& a, const Rec& b) { return a.f[0] > b.f[0]; });
    const size_t keep = (size_t)std::min(found[i], max_contours);
    memcpy(records + (size_t)i * max_contours * FE_CONTOUR_RECORD, r, keep * sizeof(Rec));
  }
}

// images per micro-batch such that `per_image` bytes each fit the arena with room to spare
int contour_microbatch(fe_ctx* ctx, int n, size_t per_image) {
  const size_t room = ctx->c.arena.capacity() / 8 * 7;
  FE_CHECK(per_image + 4096 <= room, "contours: one image needs %zu bytes of workspace, the arena holds %zu", per_image, ctx->c.arena.capacity());
  return (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, (size_t)64, room / (per_image + 4096)}));
}

// ---- what fe_leading_lines_mixed and fe_subject_region_mixed share ------------------------------------------------------------------
// what the composition calls accept of an image: the per-shape calls' own bound, h * w below 2^30
constexpr MixedLimits kCompositionLimits = {1, INT32_MAX, INT32_MAX, ((size_t)1 << 30) - 1, "below 2^30"};
// the plan of the list, or the capacity error that names the image whose own scratch exceeds the arena
comp_plan::Plan composition_plan(Ctx& C, const char* who, const int32_t* hw, int n, int on_device, bool subject,
                                 size_t max_chunk_pixels = comp_plan::kMaxChunkPixels) {
  comp_plan::Plan plan = comp_plan::build(hw, n, !on_device, subject, C.arena.capacity(), max_chunk_pixels);
  if (plan.bad_image >= 0) throw_image_too_large(who, plan.bad_image, hw, plan.bad_bytes, C.arena.capacity());
  return plan;
}
// A chunk's allocation with its blob (descriptors with their pointers, prefix tables) uploaded; host images are staged back to back,
// image k at 3 * px bytes. `blob` must outlive the copy: the caller keeps it until it has synchronised.
uint8_t* composition_stage_chunk(Ctx& C, const comp_plan::Chunk& ck, const uint8_t* const* images, const int32_t* hw, int on_device, std::vector<uint8_t>& blob) {
  const comp_plan::Layout& L = ck.lay;
  C.arena.reset();
  uint8_t* base = (uint8_t*)C.arena.alloc(L.total);
  blob.assign(L.blob_bytes, 0);
  comp_plan::ImageDesc* im = (comp_plan::ImageDesc*)blob.data();
  std::vector<size_t> offs;
  if (!on_device) mixed_list::staged_offsets(hw, ck.first, ck.first + ck.count, false, offs);
  stage_images(C, images, hw, ck.first, ck.first + ck.count, on_device, base + L.stage, offs.data(), [&](int i, const uint8_t* src) {
    im[i - ck.first] = ck.descs[i - ck.first];
    im[i - ck.first].src = src;
  });
  for (int t = 0; t < comp_plan::kTilings; ++t)
    memcpy(blob.data() + L.blob_prefix + (size_t)t * (ck.count + 1) * sizeof(int32_t), ck.prefix[t].data(), (size_t)(ck.count + 1) * sizeof(int32_t));
  FE_HIP(hipMemcpyAsync(base + L.blob, blob.data(), L.blob_bytes, hipMemcpyHostToDevice, C.stream));
  return base;
}
}  // namespace

extern "C" {

// device u8 batch -> device u8 batch resized like PIL (+ crop)
int fe_resize_u8(fe_ctx* ctx, const uint8_t* src, int n, int h, int w, int oh, int ow, int filter, int on_device,
                 uint8_t* dst) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(src && dst && n > 0, "bad arguments");
    resize_staged(C, src, (size_t)n * h * w * 3, dst, (size_t)n * oh * ow * 3, on_device,
                  [&](const uint8_t* d_in, uint8_t* d_out) { resize_u8(C, d_in, n, h, w, oh, ow, filter, 0, oh, 0, ow, d_out); });
  });
}

/* PIL `resize((ow, oh), filter, box)` with a fractional source box (x0, y0, x1, y1); box NULL = the whole image */
int fe_resize_u8_box(fe_ctx* ctx, const uint8_t* src, int n, int h, int w, int oh, int ow, int filter, const float* box, int on_device,
                     uint8_t* dst) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(src && dst && n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "bad arguments");
    const float whole[4] = {0.0f, 0.0f, (float)w, (float)h};
    resize_staged(C, src, (size_t)n * h * w * 3, dst, (size_t)n * oh * ow * 3, on_device,
                  [&](const uint8_t* d_in, uint8_t* d_out) { resize_u8_box(C, d_in, n, h, w, oh, ow, filter, box ? box : whole, d_out); });
  });
}

/* PIL `reduce((fx, fy), box)`: dst [n, ceil(bh / fy), ceil(bw / fx), 3]; box (x0, y0, x1, y1) in pixels, NULL = the whole image */
int fe_reduce_u8(fe_ctx* ctx, const uint8_t* src, int n, int h, int w, int fx, int fy, const int32_t* box, int on_device, uint8_t* dst) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(src && dst && n > 0 && h > 0 && w > 0 && fx >= 1 && fy >= 1, "bad arguments");
    const int b[4] = {box ? box[0] : 0, box ? box[1] : 0, box ? box[2] : w, box ? box[3] : h};
    FE_CHECK(b[0] >= 0 && b[1] >= 0 && b[2] <= w && b[3] <= h && b[0] < b[2] && b[1] < b[3], "reduce: box outside the image or empty");
    const int ow = (b[2] - b[0] + fx - 1) / fx, oh = (b[3] - b[1] + fy - 1) / fy;
    resize_staged(C, src, (size_t)n * h * w * 3, dst, (size_t)n * oh * ow * 3, on_device,
                  [&](const uint8_t* d_in, uint8_t* d_out) { reduce_u8(C, d_in, n, h, w, fx, fy, b, d_out); });
  });
}

size_t fe_jpeg_bound(int h, int w) { return (h > 0 && w > 0) ? jpeg_bound(h, w) : 0; }

/* what Pillow's `Image.save(buf, "JPEG", quality=q)` writes for each RGB (bgr = 1: B,G,R bytes) image of the batch */
int fe_jpeg_encode(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device, int quality, uint8_t* out, size_t cap,
                   int32_t* lengths) {
  return fe_api(ctx, OnError::Capacity, [&] {
    FE_CHECK(img && out && lengths && n > 0 && h > 0 && w > 0, "bad arguments");
    thumbnail_run(ctx, img, n, h, w, bgr, on_device, nullptr, quality, out, cap, lengths);
  });
}

/* the reference's generate_photo_thumbnail (utils/image_transforms.py:32-50) for a batch, with the plan of facet_amd.thumbnail.thumbnail_plan */
int fe_thumbnail_jpeg(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device, int oh, int ow, int fx, int fy,
                      const int32_t* reduce_box, const float* resize_box, int tall, int quality, uint8_t* out, size_t cap, int32_t* lengths) {
  return fe_api(ctx, OnError::Capacity, [&] {
    FE_CHECK(img && out && lengths && resize_box && n > 0 && h > 0 && w > 0 && fx >= 1 && fy >= 1, "bad arguments");
    FE_CHECK((fx == 1 && fy == 1) || reduce_box, "thumbnail: reduce factors without a reduce box");
    const ThumbPlan p = make_thumb_plan(oh, ow, fx, fy, reduce_box, resize_box, tall);
    thumbnail_run(ctx, img, n, h, w, bgr, on_device, &p, quality, out, cap, lengths);
  });
}

/* ---- JPEG decode: what `ImageOps.exif_transpose(Image.open(f)).convert('RGB')` gives, from the file's bytes ---- */
int fe_jpeg_probe_ex(const uint8_t* data, size_t len, int flags, fe_jpeg_info_ex* info) {
  if (!info || (flags & ~(FE_JPEG_PROGRESSIVE | FE_JPEG_FLAG_PARALLEL))) return FE_ERR_INVALID;      // the parser has no use for the second
  try {
    int32_t v[10];
    static const uint8_t none[1] = {0};
    jpeg_probe(data ? data : none, data ? len : 0, flags, v);
    info->width = v[0]; info->height = v[1]; info->components = v[2]; info->hsamp = v[3]; info->vsamp = v[4];
    info->restart_interval = v[5]; info->orientation = v[6]; info->status = v[7]; info->progressive = v[8]; info->scans = v[9];
  } catch (const std::exception&) {
    return FE_ERR_RUNTIME;
  }
  return FE_OK;
}

int fe_jpeg_probe(const uint8_t* data, size_t len, fe_jpeg_info* info) {
  if (!info) return FE_ERR_INVALID;
  fe_jpeg_info_ex x;
  const int rc = fe_jpeg_probe_ex(data, len, 0, &x);
  if (rc != FE_OK) return rc;
  info->width = x.width; info->height = x.height; info->components = x.components; info->hsamp = x.hsamp; info->vsamp = x.vsamp;
  info->restart_interval = x.restart_interval; info->orientation = x.orientation; info->status = x.status;
  return FE_OK;
}

int fe_jpeg_decode(fe_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, int h, int w, int bgr, int apply_orientation, int dst_on_device,
                   uint8_t* dst, int32_t* status) {
  return fe_api(ctx, [&] {
    FE_CHECK(data && len && dst && status && n > 0 && h > 0 && w > 0, "bad arguments");
    jpeg_decode_batch(ctx->c, data, len, n, h, w, 1, bgr, apply_orientation, dst_on_device, 0, dst, status);
  });
}

int fe_jpeg_decode_ex(fe_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, int h, int w, int bgr, int apply_orientation, int dst_on_device,
                      int flags, uint8_t* dst, int32_t* status) {
  return fe_api(ctx, [&] {
    FE_CHECK(data && len && dst && status && n > 0 && h > 0 && w > 0 && !(flags & ~(FE_JPEG_PROGRESSIVE | FE_JPEG_FLAG_PARALLEL)), "bad arguments");
    jpeg_decode_batch(ctx->c, data, len, n, h, w, 1, bgr, apply_orientation, dst_on_device, flags, dst, status);
  });
}

/* what the entropy stage of the context's last decode call did; read back with that call's statuses, so nothing is waited for here */
int fe_jpeg_entropy_stats(fe_ctx* ctx, int32_t out[4]) {
  if (!ctx || !out) return FE_ERR_INVALID;
  for (int k = 0; k < 4; ++k) out[k] = ctx->c.jpeg_entropy_stats[k];
  return FE_OK;
}

int fe_jpeg_scaled_size(int h, int w, int scale, int32_t* sh, int32_t* sw) {
  if (!sh || !sw || h <= 0 || w <= 0 || !jpeg_scale_ok(scale)) return FE_ERR_INVALID;
  int a, b;
  jpeg_scaled_size(h, w, scale, &a, &b);
  *sh = a; *sw = b;
  return FE_OK;
}

/* libjpeg's 1/scale decode, which is what Pillow's JpegImageFile.draft() switches on: scale 1 is fe_jpeg_decode_ex */
int fe_jpeg_decode_scaled(fe_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, int h, int w, int scale, int bgr, int apply_orientation,
                          int dst_on_device, int flags, uint8_t* dst, int32_t* status) {
  return fe_api(ctx, [&] {
    if (!jpeg_scale_ok(scale)) {
      ctx->c.err = "jpeg_decode_scaled: scale " + std::to_string(scale) + " (1, 2, 4 or 8)";
      return FE_ERR_INVALID;
    }
    FE_CHECK(data && len && dst && status && n > 0 && h > 0 && w > 0 && !(flags & ~(FE_JPEG_PROGRESSIVE | FE_JPEG_FLAG_PARALLEL)), "bad arguments");
    jpeg_decode_batch(ctx->c, data, len, n, h, w, scale, bgr, apply_orientation, dst_on_device, flags, dst, status);
    return FE_OK;
  });
}

/* stored JPEG bytes -> smaller JPEG bytes: `Image.open(f)`, `thumbnail((size, size), LANCZOS)`, `save("JPEG", quality)` (reference
 * db/maintenance.py:182-272, api/routers/thumbnails.py:54-64) as scaled decode -> reduce -> boxed LANCZOS -> encode on one resident buffer */
int fe_jpeg_thumbnail(fe_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, int h, int w, int scale, int flags, int oh, int ow, int fx,
                      int fy, const int32_t* reduce_box, const float* resize_box, int tall, int quality, uint8_t* out, size_t cap, int32_t* lengths,
                      int32_t* status) {
  return fe_api(ctx, OnError::Capacity, [&] {
    if (!jpeg_scale_ok(scale)) {
      ctx->c.err = "jpeg_thumbnail: scale " + std::to_string(scale) + " (1, 2, 4 or 8)";
      return FE_ERR_INVALID;
    }
    FE_CHECK(data && len && out && lengths && status && resize_box && n > 0 && h > 0 && w > 0 && fx >= 1 && fy >= 1 && !(flags & ~(FE_JPEG_PROGRESSIVE | FE_JPEG_FLAG_PARALLEL)),
             "bad arguments");
    FE_CHECK((fx == 1 && fy == 1) || reduce_box, "jpeg_thumbnail: reduce factors without a reduce box");
    const ThumbPlan p = make_thumb_plan(oh, ow, fx, fy, reduce_box, resize_box, tall);
    Ctx& C = ctx->c;
    struct DevBuf {
      uint8_t* p = nullptr;
      ~DevBuf() { if (p) (void)hipFree(p); }
    } px;                                                      // the decoded batch: outside the arena, which both stages recycle
    const size_t per = (size_t)h * w * 3;
    FE_HIP(hipMalloc((void**)&px.p, (size_t)n * per));
    jpeg_decode_batch(C, data, len, n, h, w, scale, 0, 0, 1, flags, px.p, status);      // no EXIF transpose: Image.open + thumbnail does none
    std::vector<int> good;
    for (int i = 0; i < n; ++i) {
      lengths[i] = 0;
      if (status[i] == 0) good.push_back(i);
    }
    const int ng = (int)good.size();
    for (int k = 0; k < ng; ++k)                               // close the holes files with a status left: slot good[k] >= k moves down to k
      if (good[k] != k) FE_HIP(hipMemcpyAsync(px.p + (size_t)k * per, px.p + (size_t)good[k] * per, per, hipMemcpyDeviceToDevice, C.stream));
    auto spread = [&]() {                                      // rows and lengths 0 .. ng - 1 back to their files' places, last first
      for (int k = ng - 1; k >= 0; --k) {
        if (good[k] == k) continue;
        if (lengths[k] > 0 && (size_t)lengths[k] <= cap) memmove(out + (size_t)good[k] * cap, out + (size_t)k * cap, (size_t)lengths[k]);
        lengths[good[k]] = lengths[k];
        lengths[k] = 0;
      }
    };
    if (ng) {
      try {
        thumbnail_run(ctx, px.p, ng, h, w, 0, 1, &p, quality, out, cap, lengths);
      } catch (const CapacityError&) {
        spread();
        throw;
      }
      spread();
    }
    return FE_OK;
  });
}

/* External contours of binary images: labelling, RETR_EXTERNAL test and border sums on the device (kernels_contours.hip) */
int fe_external_contours(fe_ctx* ctx, const uint8_t* binary, int n, int h, int w, int on_device, long long min_twice_area, int max_contours,
                         long long* records, int* counts) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(binary && records && counts && n > 0 && h > 0 && w > 0 && (size_t)h * w < (1ull << 30) && max_contours > 0 && min_twice_area >= 0,
             "bad arguments");
    const size_t npx = (size_t)h * w;
    const int mb = contour_microbatch(ctx, n, contour_scratch_bytes(1, h, w));
    ImageStager st(ctx, binary, n, npx, mb, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int i0 = k * mb, nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      ContourScratch sc;
      contour_scratch_carve(sc, C.arena.alloc(contour_scratch_bytes(nb, h, w)), nb, h, w);
      launch_external_contours(d_in, nb, h, w, 0, min_twice_area, sc, C.stream);
      st.done(k);
      collect_contours(ctx, sc, nb, h, w, max_contours, records + (size_t)i0 * max_contours * FE_CONTOUR_RECORD, counts + i0);
    }
  });
}

/* Subject region (reference analyzers/composition.py:16-93): median thresholds, Canny, hysteresis, external contours - all on the device */
int fe_subject_region(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int max_contours, long long* records, int* counts,
                      int* thresholds, uint8_t* edges_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(bgr && records && counts && n > 0 && h > 0 && w > 0 && (size_t)h * w < (1ull << 30) && max_contours > 0, "bad arguments");
    ensure_hsv_tables(ctx);
    const size_t npx = (size_t)h * w, per = npx * 3;
    const long long min_twice_area = ((long long)npx + 4999) / 5000;      // smallest a with a * 5000 >= h * w  (area > h * w * 0.0001, not strict)
    const size_t per_image = contour_scratch_bytes(1, h, w) + 8 * npx + stats_accum_bytes(1) + FE_STATS_COUNT * sizeof(double) + 2048;
    const int mb = contour_microbatch(ctx, n, per_image);
    ImageStager st(ctx, bgr, n, per, mb, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int i0 = k * mb, nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      uint8_t* d_gray = (uint8_t*)C.arena.alloc((size_t)nb * npx);
      void* d_acc = C.arena.alloc(stats_accum_bytes(nb));
      double* d_stats = (double*)C.arena.alloc((size_t)nb * FE_STATS_COUNT * sizeof(double));
      int* d_thr = (int*)C.arena.alloc((size_t)nb * 2 * sizeof(int));
      void* d_grad = C.arena.alloc((size_t)nb * npx * 4);
      void* d_mag = C.arena.alloc((size_t)nb * npx * 2);
      uint8_t* d_map = (uint8_t*)C.arena.alloc((size_t)nb * npx);
      ContourScratch sc;
      contour_scratch_carve(sc, C.arena.alloc(contour_scratch_bytes(nb, h, w)), nb, h, w);
      // gray and its histogram come from the statistics pass, so the conversion exists once
      launch_image_stats(d_in, nb, h, w, d_gray, nullptr, ctx->hsv_sdiv, ctx->hsv_hdiv, d_acc, d_stats, C.stream);
      st.done(k);
      launch_median_thresholds(d_stats, nb, (long long)npx, d_thr, C.stream);
      launch_canny_map_gray(d_gray, nb, h, w, d_thr, d_grad, d_mag, d_map, C.stream);
      launch_external_contours(d_map, nb, h, w, 1, min_twice_area, sc, C.stream);
      if (thresholds) FE_HIP(hipMemcpyAsync(thresholds + (size_t)i0 * 2, d_thr, (size_t)nb * 2 * sizeof(int), hipMemcpyDeviceToHost, C.stream));
      if (edges_out) FE_HIP(hipMemcpyAsync(edges_out + (size_t)i0 * npx, sc.edge, (size_t)nb * npx, hipMemcpyDeviceToHost, C.stream));
      collect_contours(ctx, sc, nb, h, w, max_contours, records + (size_t)i0 * max_contours * FE_CONTOUR_RECORD, counts + i0);
    }
  });
}

/* Per-image technical statistics of a BGR batch (reference analyzers/image_cache.py:28-33 + analyzers/technical.py) */
int fe_image_stats(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, double* stats, uint8_t* gray_out, uint8_t* hsv_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(bgr && stats && n > 0 && h > 0 && w > 0, "bad arguments");
    ensure_hsv_tables(ctx);
    const size_t per = (size_t)h * w * 3, npx = (size_t)h * w;
    // two blocks per image in pass 1: large chunks keep all 256 CUs busy (the footprint is only ~2-5 bytes per pixel)
    const int mb = std::max(1, std::max(ctx->microbatch, 256));
    ImageStager st(ctx, bgr, n, per, mb, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int i0 = k * mb, nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      uint8_t* d_gray = (uint8_t*)C.arena.alloc((size_t)nb * npx);
      uint8_t* d_hsv = hsv_out ? (uint8_t*)C.arena.alloc((size_t)nb * per) : nullptr;
      void* d_acc = C.arena.alloc(stats_accum_bytes(nb));
      double* d_out = (double*)C.arena.alloc((size_t)nb * FE_STATS_COUNT * sizeof(double));
      launch_image_stats(d_in, nb, h, w, d_gray, d_hsv, ctx->hsv_sdiv, ctx->hsv_hdiv, d_acc, d_out, C.stream);
      st.done(k);
      FE_HIP(hipMemcpyAsync(stats + (size_t)i0 * FE_STATS_COUNT, d_out, (size_t)nb * FE_STATS_COUNT * sizeof(double), hipMemcpyDeviceToHost, C.stream));
      if (gray_out) FE_HIP(hipMemcpyAsync(gray_out + (size_t)i0 * npx, d_gray, (size_t)nb * npx, hipMemcpyDeviceToHost, C.stream));
      if (hsv_out) FE_HIP(hipMemcpyAsync(hsv_out + (size_t)i0 * per, d_hsv, (size_t)nb * per, hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));   // the arena is recycled by the next micro-batch
    }
  });
}

/* The records of fe_image_stats for a list of images of any sizes: the plan of stats_plan.h, chunk by chunk */
int fe_image_stats_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, double* stats) {
  return fe_api(ctx, OnError::Capacity, [&]() -> int {
    namespace sp = fe::stats_plan;
    Ctx& C = ctx->c;
    const char* who = "fe_image_stats_mixed";
    if (!mixed_list_ok(C, who, (images && stats) ? images : nullptr, hw, n, order, images, kAnySideBelow2_31)) return FE_ERR_INVALID;
    const sp::Plan plan = sp::build(hw, n, !on_device, ctx->stats_segment ? ctx->stats_segment : sp::kDefaultSegment, C.arena.capacity());
    if (plan.bad_image >= 0) throw_image_too_large(who, plan.bad_image, hw, plan.bad_bytes, C.arena.capacity());
    ensure_hsv_tables(ctx);
    std::vector<uint8_t> blob;
    for (const sp::Chunk& ck : plan.chunks) {
      const sp::Layout& L = ck.lay;
      C.arena.reset();
      uint8_t* base = (uint8_t*)C.arena.alloc(L.total);
      blob.assign(L.blob_bytes, 0);
      sp::ImageDesc* im = (sp::ImageDesc*)blob.data();
      stage_images(C, images, hw, ck.first, ck.first + ck.count, on_device, base + L.stage, ck.stage_off.data(), [&](int i, const uint8_t* src) {
        const int k = i - ck.first;
        im[k] = sp::ImageDesc{src, base + L.gray + ck.gray_off[k], hw[2 * i], hw[2 * i + 1], ck.nseg[k], 0};
      });
      memcpy(blob.data() + L.blob_segs, ck.segs.data(), ck.segs.size() * sizeof(sp::SegDesc));
      memcpy(blob.data() + L.blob_strips, ck.strips.data(), ck.strips.size() * sizeof(sp::StripDesc));
      if (!ck.multi.empty()) memcpy(blob.data() + L.blob_multi, ck.multi.data(), ck.multi.size() * sizeof(int32_t));
      uint8_t* d_blob = base + L.blob;
      FE_HIP(hipMemcpyAsync(d_blob, blob.data(), L.blob_bytes, hipMemcpyHostToDevice, C.stream));
      double* d_out = (double*)(base + L.records);
      launch_image_stats_mixed((const sp::ImageDesc*)d_blob, ck.count, (const sp::SegDesc*)(d_blob + L.blob_segs), (int)ck.segs.size(),
                               (const sp::StripDesc*)(d_blob + L.blob_strips), (int)ck.strips.size(), (const int32_t*)(d_blob + L.blob_multi),
                               (int)ck.multi.size(), order == FE_ORDER_RGB, ctx->hsv_sdiv, ctx->hsv_hdiv, base + L.accum, L.zero_bytes,
                               (unsigned int*)(base + L.hist), d_out, C.stream);
      FE_HIP(hipMemcpyAsync(stats + (size_t)ck.first * FE_STATS_COUNT, d_out, (size_t)ck.count * FE_STATS_COUNT * sizeof(double), hipMemcpyDeviceToHost,
                            C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));   // the arena and the blob are recycled by the next chunk
    }
    return FE_OK;
  });
}

int fe_set_stats_segment(fe_ctx* ctx, int pixels) {
  return fe_api(ctx, [&]() -> int {
    if (pixels != 0 && (pixels < fe::stats_plan::kSegmentUnit || pixels % fe::stats_plan::kSegmentUnit != 0)) {
      char b[160];
      snprintf(b, sizeof b, "fe_set_stats_segment: %d pixels (0 for the default, or a multiple of %d that is at least %d)", pixels,
               fe::stats_plan::kSegmentUnit, fe::stats_plan::kSegmentUnit);
      ctx->c.err = b;
      return FE_ERR_INVALID;
    }
    ctx->stats_segment = pixels;
    return FE_OK;
  });
}

/* RGB <-> BGR copy of a packed uint8 batch into device memory */
int fe_swap_rb_u8(fe_ctx* ctx, const uint8_t* src, int on_device, size_t pixels, uint8_t* dst_device) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(src && dst_device && pixels > 0, "bad arguments");
    if (on_device) {
      FE_CHECK(src != dst_device, "swap_rb: in-place is not supported");
      launch_swap_rb_u8(src, dst_device, pixels, C.stream);
    } else {                                   // stage through the destination: upload, then swap each pixel's ends in a second buffer-free pass
      C.arena.reset();
      launch_swap_rb_u8(upload(C, src, pixels * 3), dst_device, pixels, C.stream);
    }
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

/* Leading lines (reference analyzers/composition.py:191-261): blur + Canny map on the GPU, hysteresis + probabilistic Hough per image on host threads */
int fe_leading_lines(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int canny_low, int canny_high, int threshold,
                     int min_line_length, int max_line_gap, int max_lines, int* lines, int* counts, uint8_t* edges_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(bgr && n > 0 && h > 0 && w > 0 && (size_t)h * w < (1ull << 30), "bad arguments");
    FE_CHECK((lines != nullptr) == (counts != nullptr) && (lines || edges_out), "pass lines AND counts, and / or edges_out");
    FE_CHECK(!lines || max_lines > 0, "max_lines must be positive");
    FE_CHECK(canny_low >= 0 && canny_high >= canny_low && threshold > 0 && min_line_length >= 0 && max_line_gap >= 0, "bad thresholds");
    const size_t npx = (size_t)h * w, per = npx * 3;
    const int mb = std::max(1, std::min(n, 64));
    const int threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<uint8_t> scratch;
    if (!edges_out) scratch.resize((size_t)mb * npx);
    ctx->lines_host_ms = 0.0;
    ImageStager st(ctx, bgr, n, per, mb, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int i0 = k * mb, nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      uint8_t* d_blur = (uint8_t*)C.arena.alloc((size_t)nb * npx);
      void* d_grad = C.arena.alloc((size_t)nb * npx * 4);
      void* d_mag = C.arena.alloc((size_t)nb * npx * 2);
      uint8_t* d_map = (uint8_t*)C.arena.alloc((size_t)nb * npx);
      launch_canny_map(d_in, nb, h, w, canny_low, canny_high, d_blur, d_grad, d_mag, d_map, C.stream);
      st.done(k);
      uint8_t* maps = edges_out ? edges_out + (size_t)i0 * npx : scratch.data();
      FE_HIP(hipMemcpyAsync(maps, d_map, (size_t)nb * npx, hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
      const auto t0 = std::chrono::steady_clock::now();
      lines_host_stage(maps, nb, h, w, threshold, min_line_length, max_line_gap, max_lines, lines ? lines + (size_t)i0 * max_lines * 4 : nullptr,
                       counts ? counts + i0 : nullptr, threads);
      ctx->lines_host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  });
}

/* fe_leading_lines for a list of images of any sizes: three launches and one map copy per arena chunk, the host stage over the chunk */
int fe_leading_lines_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int canny_low, int canny_high,
                           int threshold, const int32_t* min_line_length, int max_line_gap, int max_lines, int* lines, int* counts, uint8_t* edges_out) {
  return fe_api(ctx, OnError::Capacity, [&]() -> int {
    Ctx& C = ctx->c;
    char b[240];
    if (!mixed_list_ok(C, "fe_leading_lines_mixed", images, hw, n, order, images, kCompositionLimits)) return FE_ERR_INVALID;
    const char* why = nullptr;
    if ((lines != nullptr) != (counts != nullptr) || !(lines || edges_out)) why = "pass lines AND counts, and / or edges_out";
    else if (lines && max_lines <= 0) why = "max_lines must be positive";
    else if (lines && !min_line_length) why = "min_line_length is a null pointer";
    else if (canny_low < 0 || canny_high < canny_low || threshold <= 0 || max_line_gap < 0) why = "bad thresholds";
    if (why) { snprintf(b, sizeof b, "fe_leading_lines_mixed: %s", why); C.err = b; return FE_ERR_INVALID; }
    for (int i = 0; lines && i < n; ++i)
      if (min_line_length[i] < 0) {
        snprintf(b, sizeof b, "fe_leading_lines_mixed: image %d: min_line_length %d is negative", i, min_line_length[i]);
        C.err = b;
        return FE_ERR_INVALID;
      }
    // Without edges_out the maps of a chunk come down into a pinned buffer the context keeps (a fresh pageable one costs more than
    // the kernels: page faults, and a copy at a fraction of the link's rate), so a chunk of several images holds at most 2^28 pixels
    constexpr size_t kHostMapPixels = (size_t)1 << 28;
    const comp_plan::Plan plan = composition_plan(C, "fe_leading_lines_mixed", hw, n, on_device, false, kHostMapPixels);
    const int threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<uint8_t> blob;
    std::vector<size_t> offsets;
    std::vector<int32_t> no_len;
    size_t first_px = 0;      // of the chunk, in the caller's flat edge buffer
    ctx->lines_host_ms = 0.0;
    for (const comp_plan::Chunk& ck : plan.chunks) {
      uint8_t* base = composition_stage_chunk(C, ck, images, hw, on_device, blob);
      launch_canny_map_mixed(base, ck, order == FE_ORDER_RGB, canny_low, canny_high, C.stream);
      if (!edges_out && ctx->lines_maps_cap < ck.pixels) {
        if (ctx->lines_maps) (void)hipHostFree(ctx->lines_maps);
        ctx->lines_maps = nullptr; ctx->lines_maps_cap = 0;
        FE_HIP(hipHostMalloc((void**)&ctx->lines_maps, ck.pixels, hipHostMallocDefault));
        ctx->lines_maps_cap = ck.pixels;
      }
      uint8_t* maps = edges_out ? edges_out + first_px : ctx->lines_maps;
      FE_HIP(hipMemcpyAsync(maps, base + ck.lay.map, ck.pixels, hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));   // the arena and the blob are recycled by the next chunk
      offsets.resize(ck.count);
      for (int k = 0; k < ck.count; ++k) offsets[k] = ck.descs[k].px;
      if (!lines) no_len.assign(ck.count, 0);
      const auto t0 = std::chrono::steady_clock::now();
      lines_host_stage_mixed(maps, offsets.data(), hw + 2 * (size_t)ck.first, ck.count, threshold, lines ? min_line_length + ck.first : no_len.data(),
                             max_line_gap, max_lines, lines ? lines + (size_t)ck.first * max_lines * 4 : nullptr, counts ? counts + ck.first : nullptr,
                             threads);
      ctx->lines_host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      first_px += ck.pixels;
    }
    return FE_OK;
  });
}

/* how long the host stage (hysteresis and Hough, all chunks) of the context's last fe_leading_lines / fe_leading_lines_mixed call took */
int fe_lines_host_ms(fe_ctx* ctx, double* ms) {
  if (!ctx || !ms) return FE_ERR_INVALID;
  *ms = ctx->lines_host_ms;
  return FE_OK;
}

/* fe_subject_region for a list of images of any sizes: one memset, a fixed number of launches and two read-backs per arena chunk */
int fe_subject_region_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int max_contours,
                            long long* records, int* counts, int* thresholds, uint8_t* edges_out) {
  return fe_api(ctx, OnError::Capacity, [&]() -> int {
    Ctx& C = ctx->c;
    if (!mixed_list_ok(C, "fe_subject_region_mixed", (records && counts) ? images : nullptr, hw, n, order, images, kCompositionLimits)) return FE_ERR_INVALID;
    if (max_contours <= 0) { C.err = "fe_subject_region_mixed: max_contours must be positive"; return FE_ERR_INVALID; }
    const comp_plan::Plan plan = composition_plan(C, "fe_subject_region_mixed", hw, n, on_device, true);
    struct Rec { long long f[FE_CONTOUR_RECORD]; };
    std::vector<uint8_t> blob;
    std::vector<int> ctr;
    std::vector<Rec> got;
    std::vector<size_t> at;
    size_t first_px = 0;
    for (const comp_plan::Chunk& ck : plan.chunks) {
      const comp_plan::Layout& L = ck.lay;
      const int nb = ck.count;
      uint8_t* base = composition_stage_chunk(C, ck, images, hw, on_device, blob);
      launch_subject_mixed(base, ck, order == FE_ORDER_RGB, C.stream);
      if (thresholds) FE_HIP(hipMemcpyAsync(thresholds + 2 * (size_t)ck.first, base + L.thr, (size_t)nb * 2 * sizeof(int), hipMemcpyDeviceToHost, C.stream));
      if (edges_out) FE_HIP(hipMemcpyAsync(edges_out + first_px, base + L.edge, ck.pixels, hipMemcpyDeviceToHost, C.stream));
      // one copy of the counters (listed [nb], found [nb], error, stored), then one of the chunk's records
      ctr.resize(comp_plan::counter_ints(nb));
      FE_HIP(hipMemcpyAsync(ctr.data(), base + L.counters, ctr.size() * sizeof(int), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
      const int *listed = ctr.data(), *found = listed + nb, err = found[nb], stored = found[nb + 1];
      FE_CHECK(!(err & 1), "contours: a border walk did not close within 8 * pixels + 8 steps");
      FE_CHECK(!(err & 2), "contours: more component roots than an image can hold");
      size_t total = 0;
      at.assign((size_t)nb + 1, 0);
      for (int k = 0; k < nb; ++k) {
        FE_CHECK(found[k] >= 0 && found[k] <= listed[k] && listed[k] <= ck.descs[k].cap, "contours: inconsistent counts of image %d (%d of %d, room %d)",
                 ck.first + k, found[k], listed[k], ck.descs[k].cap);
        counts[ck.first + k] = found[k];
        total += (size_t)found[k];
        at[k + 1] = total;
      }
      FE_CHECK((size_t)stored == total, "contours: %d records stored, %zu counted", stored, total);
      got.resize(total);
      if (total) FE_HIP(hipMemcpyAsync(got.data(), base + L.recs, total * sizeof(Rec), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));   // the arena and the blob are recycled by the next chunk
      // the list is in the order the walks finished: by image, and in descending start_index order within one, as collect_contours leaves them
      std::sort(got.begin(), got.end(), [](const Rec& a, const Rec& b) {
        const long long ia = a.f[0] >> 32, ib = b.f[0] >> 32;
        return ia != ib ? ia < ib : a.f[0] > b.f[0];
      });
      for (int k = 0; k < nb; ++k) {
        const size_t keep = (size_t)std::min(found[k], max_contours);
        Rec* out = reinterpret_cast<Rec*>(records + (size_t)(ck.first + k) * max_contours * FE_CONTOUR_RECORD);
        for (size_t q = 0; q < keep; ++q) {
          const Rec& r = got[at[k] + q];
          FE_CHECK((r.f[0] >> 32) == k, "contours: a record of image %d where image %d's were counted", (int)(r.f[0] >> 32) + ck.first, ck.first + k);
          out[q] = r;
          out[q].f[0] = r.f[0] & 0xffffffffll;
        }
      }
      first_px += ck.pixels;
    }
    return FE_OK;
  });
}

/* imagehash.phash (hash_size 8, highfreq_factor 4) of every image of an RGB / BGR batch (reference batch_processor.py:216) */
int fe_phash(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device, uint64_t* hashes, uint8_t* small_out, double* dct_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(img && hashes && n > 0 && h > 0 && w > 0, "bad arguments");
    const size_t per = (size_t)h * w * 3;
    if (phash_tall(h, w)) {      // Image.resize's vertical-pass-first case: the descriptor path has the kernel for it
      FE_CHECK(w <= 32768 && h <= 65536, "phash: bad shape %d x %d x %d", n, h, w);
      std::vector<const uint8_t*> ptrs(n);
      std::vector<int32_t> sizes(2 * (size_t)n);
      for (int i = 0; i < n; ++i) { ptrs[i] = img + (size_t)i * per; sizes[2 * i] = h; sizes[2 * i + 1] = w; }
      phash_mixed_run(ctx, ptrs.data(), sizes.data(), n, on_device, bgr ? FE_ORDER_BGR : FE_ORDER_RGB, hashes, small_out, dct_out);
      return;
    }
    ensure_phash_cos(ctx);
    // chunks of up to 256 images whatever the model micro-batch (a wave per row: large chunks fill the chip, scratch is 32 B per
    // row), but at most 1 GiB of pixels: host input is staged through two device buffers of one chunk each
    const int mb = (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)1 << 30) / per));
    ImageStager st(ctx, img, n, per, mb, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int i0 = k * mb, nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      uint8_t* d_tmp = (uint8_t*)C.arena.alloc(phash_tmp_bytes(nb, h));
      uint64_t* d_hash = (uint64_t*)C.arena.alloc((size_t)nb * sizeof(uint64_t));
      uint8_t* d_small = small_out ? (uint8_t*)C.arena.alloc((size_t)nb * 1024) : nullptr;
      double* d_dct = dct_out ? (double*)C.arena.alloc((size_t)nb * 64 * sizeof(double)) : nullptr;
      launch_phash(C, d_in, nb, h, w, bgr ? 1 : 0, d_tmp, ctx->phash_cos, d_hash, d_small, d_dct);
      st.done(k);
      FE_HIP(hipMemcpyAsync(hashes + i0, d_hash, (size_t)nb * sizeof(uint64_t), hipMemcpyDeviceToHost, C.stream));
      if (small_out) FE_HIP(hipMemcpyAsync(small_out + (size_t)i0 * 1024, d_small, (size_t)nb * 1024, hipMemcpyDeviceToHost, C.stream));
      if (dct_out) FE_HIP(hipMemcpyAsync(dct_out + (size_t)i0 * 64, d_dct, (size_t)nb * 64 * sizeof(double), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));   // the arena is recycled by the next micro-batch
    }
  });
}

/* fe_phash for a list of images of any sizes: two launches per arena chunk of the list, all tables in one call-scoped pool */
int fe_phash_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, uint64_t* hashes, uint8_t* small_out,
                   double* dct_out) {
  return fe_api(ctx, OnError::Capacity, [&]() -> int {
    constexpr MixedLimits lim = {1, 65536, 32768, SIZE_MAX, nullptr};
    if (!mixed_list_ok(ctx->c, "fe_phash_mixed", (images && hashes) ? images : nullptr, hw, n, order, images, lim)) return FE_ERR_INVALID;
    phash_mixed_run(ctx, images, hw, n, on_device, order, hashes, small_out, dct_out);
    return FE_OK;
  });
}

/* fe_thumbnail_jpeg for a list of images of any sizes, each with its own plan: one launch per stage per arena chunk of the list */
int fe_thumbnail_jpeg_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, const fe_thumb_plan* plans,
                            int quality, uint8_t* out, size_t cap, int32_t* lengths) {
  return fe_api(ctx, OnError::Capacity, [&]() -> int {
    Ctx& C = ctx->c;
    char b[240];
    if (!mixed_list_ok(C, "fe_thumbnail_jpeg_mixed", (images && plans && out && lengths) ? images : nullptr, hw, n, order, images, kAnySideBelow2_31))
      return FE_ERR_INVALID;
    if (quality < 1 || quality > 100) {
      snprintf(b, sizeof b, "fe_thumbnail_jpeg_mixed: quality %d (1 .. 100)", quality);
      C.err = b;
      return FE_ERR_INVALID;
    }
    ThumbTables tables;
    std::vector<ThumbDesc> descs(n);
    int max_oh = 1, max_ow = 1;
    for (int i = 0; i < n; ++i) {
      const fe_thumb_plan& p = plans[i];
      if (const char* why = tables.describe(hw[2 * i], hw[2 * i + 1], p.oh, p.ow, p.fx, p.fy, p.reduce_box, p.resize_box, p.tall, descs[i])) {
        snprintf(b, sizeof b, "fe_thumbnail_jpeg_mixed: image %d (%d x %d): %s", i, hw[2 * i], hw[2 * i + 1], why);
        C.err = b;
        return FE_ERR_INVALID;
      }
      max_oh = std::max(max_oh, (int)p.oh); max_ow = std::max(max_ow, (int)p.ow);
    }
    const size_t dcap = std::min(cap, jpeg_bound(max_oh, max_ow));      // no encode is longer, so the device rows need not be
    C.arena.reset();
    const int32_t* d_pool = upload(C, tables.pool.data(), tables.pool.size());
    const size_t mark = C.arena.mark();
    const std::vector<int> ends = thumb_mixed_cuts(descs.data(), n, !on_device, dcap, C.arena.capacity(), mark);
    std::vector<uint8_t> blob, packed;
    std::vector<int32_t> lens;
    std::vector<size_t> offs;
    bool overflow = false;
    int i0 = 0;
    for (const int i1 : ends) {
      const int nb = i1 - i0;
      C.arena.rewind(mark);
      uint8_t* d_out = (uint8_t*)C.arena.alloc((size_t)nb * dcap);
      int32_t* d_len = (int32_t*)C.arena.alloc((size_t)nb * sizeof(int32_t));
      const size_t scratch = C.arena.mark();
      uint8_t* d_stage = on_device ? nullptr : (uint8_t*)C.arena.alloc(mixed_list::staged_offsets(hw, i0, i1, true, offs));
      stage_images(C, images, hw, i0, i1, on_device, d_stage, offs.data(), [&](int i, const uint8_t* src) { descs[i].src = src; });
      thumbnails_mixed_launch(C, descs.data() + i0, nb, d_pool, order == FE_ORDER_BGR, quality, blob, d_out, dcap, d_len);
      lens.resize(nb);
      FE_HIP(hipMemcpyAsync(lens.data(), d_len, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
      size_t total = 0, longest = 0;
      for (int i = 0; i < nb; ++i) {
        const int32_t len = lens[i];
        lengths[i0 + i] = len;
        if (len <= 0 || (size_t)len > cap) { overflow = true; continue; }
        total += (size_t)len;
        longest = std::max(longest, (size_t)len);
      }
      if (total) {      // one gather of the used bytes into the dead scratch, one copy down, and the rows are dealt out on the host
        C.arena.rewind(scratch);
        uint8_t* d_packed = (uint8_t*)C.arena.alloc(total);
        jpeg_gather(C, d_out, dcap, d_len, nb, longest, d_packed);
        packed.resize(total);
        FE_HIP(hipMemcpyAsync(packed.data(), d_packed, total, hipMemcpyDeviceToHost, C.stream));
        FE_HIP(hipStreamSynchronize(C.stream));   // the arena is recycled by the next chunk
        size_t at = 0;
        for (int i = 0; i < nb; ++i) {
          const int32_t len = lens[i];
          if (len <= 0 || (size_t)len > cap) continue;
          memcpy(out + (size_t)(i0 + i) * cap, packed.data() + at, (size_t)len);
          at += (size_t)len;
        }
      }
      i0 = i1;
    }
    if (overflow) {
      snprintf(b, sizeof b, "jpeg: an image needs more than the %zu bytes of its output row (fe_jpeg_bound(%d, %d) = %zu always fits)", cap, max_oh, max_ow,
               jpeg_bound(max_oh, max_ow));
      throw CapacityError(b);
    }
    return FE_OK;
  });
}

/* how many per-size coefficient tables the context has cached (fe_resize_u8 / fe_resize_u8_box / fe_phash / fe_thumbnail_jpeg add one or two per
 * new size; the mixed-size entry points add none) */
int fe_resize_cache_entries(fe_ctx* ctx, int32_t* entries) {
  if (!ctx || !entries) return FE_ERR_INVALID;
  *entries = (int32_t)(ctx->c.resize_cache.size() + ctx->c.resize_box_cache.size());
  return FE_OK;
}

}  // extern "C"
