// C ABI: the face path (InsightFace FaceAnalysis: detection -> landmark_2d_106 -> recognition), cv2 resize, ROI Laplacian, face thumbnails.
#include "capi_internal.h"

namespace {
void ensure_warp_wtab(fe_ctx* ctx);
void invert_crop_matrices(const double* M, int m, std::vector<double>& inv);

fe_ctx::CvResizeTab cv_resize_tab(fe_ctx* ctx, int src, int dst, bool clamp) {
  auto key = std::make_tuple(src, dst, clamp ? 1 : 0);
  auto it = ctx->cvresize.find(key);
  if (it != ctx->cvresize.end()) return it->second;
  std::vector<int> ofs;
  std::vector<short> coef;
  cv_resize_tables(src, dst, clamp, ofs, coef);
  fe_ctx::CvResizeTab t{};
  FE_HIP(hipMalloc((void**)&t.ofs, ofs.size() * sizeof(int)));
  ctx->misc_allocs.push_back(t.ofs);
  FE_HIP(hipMalloc((void**)&t.coef, coef.size() * sizeof(short)));
  ctx->misc_allocs.push_back(t.coef);
  FE_HIP(hipMemcpy(t.ofs, ofs.data(), ofs.size() * sizeof(int), hipMemcpyHostToDevice));
  FE_HIP(hipMemcpy(t.coef, coef.data(), coef.size() * sizeof(short), hipMemcpyHostToDevice));
  return ctx->cvresize[key] = t;
}

// Warps `m` crops out of device-resident images and (optionally) runs graph `gs` on them. d_out: device [m][out_dim] or null;
// crops_out: host [m][size][size][3] or null. Does not reset the arena; allocates above the caller's mark.
void run_face_crops(fe_ctx* ctx, GraphSlot* gs, const uint8_t* d_img, int n, int h, int w, int m, const int* img_index,
                    const double* M, int size, float mean, float scale, int swap_rb, float* d_out, int out_dim, uint8_t* crops_out) {
  Ctx& C = ctx->c;
  if (m <= 0) return;
  ensure_warp_wtab(ctx);
  for (int f = 0; f < m; ++f) FE_CHECK(img_index[f] >= 0 && img_index[f] < n, "crop %d refers to image %d of %d", f, img_index[f], n);
  std::vector<double> inv;
  invert_crop_matrices(M, m, inv);
  double* d_inv = upload(C, inv.data(), inv.size());
  int* d_idx = upload(C, img_index, (size_t)m);
  FE_HIP(hipStreamSynchronize(C.stream));   // inv is a local; the copies above must finish before it goes away
  const size_t base = C.arena.mark();
  const int mb = std::max(1, ctx->microbatch * 8);   // crops are small (112^2 / 192^2): large batches fill the chip
  for (int f0 = 0; f0 < m; f0 += mb) {
    const int fb = std::min(mb, m - f0);
    C.arena.rewind(base);
    uint8_t* crops = (uint8_t*)C.arena.alloc((size_t)fb * size * size * 3);
    launch_warp_affine(d_img, h, w, d_idx + f0, d_inv + (size_t)f0 * 6, fb, size, ctx->warp_wtab, crops, C.stream);
    if (crops_out)
      FE_HIP(hipMemcpyAsync(crops_out + (size_t)f0 * size * size * 3, crops, (size_t)fb * size * size * 3, hipMemcpyDeviceToHost, C.stream));
    if (d_out) {
      Tensor x = C.arena.tensor(fb, size, size, 4);
      launch_u8_blob(crops, x.p, (size_t)fb * size * size, mean, scale, swap_rb, C.stream);
      std::vector<GraphOutput> outs;
      gs->g.run(C, x, 3, outs);
      FE_CHECK(outs[0].numel == (size_t)fb * out_dim, "graph output has %zu values for %d crops, expected %d each", outs[0].numel, fb, out_dim);
      FE_HIP(hipMemcpyAsync(d_out + (size_t)f0 * out_dim, outs[0].dev, outs[0].numel * sizeof(float), hipMemcpyDeviceToDevice, C.stream));
    }
  }
}

struct Cand { float v[16]; };
// insightface SCRFD.nms on rows sorted by score (fp32 arithmetic like numpy's): returns kept indices in score order
std::vector<int> face_nms(const std::vector<Cand>& c, float thresh) {
  const int n = (int)c.size();
  std::vector<float> area(n);
  for (int i = 0; i < n; ++i) area[i] = (c[i].v[3] - c[i].v[1] + 1.f) * (c[i].v[4] - c[i].v[2] + 1.f);
  std::vector<char> dead(n, 0);
  std::vector<int> keep;
  for (int i = 0; i < n; ++i) {
    if (dead[i]) continue;
    keep.push_back(i);
    for (int j = i + 1; j < n; ++j) {
      if (dead[j]) continue;
      const float xx1 = std::max(c[i].v[1], c[j].v[1]), yy1 = std::max(c[i].v[2], c[j].v[2]);
      const float xx2 = std::min(c[i].v[3], c[j].v[3]), yy2 = std::min(c[i].v[4], c[j].v[4]);
      const float ww = std::max(0.0f, xx2 - xx1 + 1.f), hh = std::max(0.0f, yy2 - yy1 + 1.f);
      const float inter = ww * hh;
      const float ovr = inter / (area[i] + area[j] - inter);
      if (!(ovr <= thresh)) dead[j] = 1;
    }
  }
  return keep;
}
// least-squares similarity src(5 pts, fp32) -> dst, closed form of Umeyama in 2-D (double); false when degenerate
bool similarity5(const float* src, const double* dst, double* M) {
  double sm[2] = {0, 0}, dm[2] = {0, 0};
  for (int k = 0; k < 5; ++k) { sm[0] += src[2 * k]; sm[1] += src[2 * k + 1]; dm[0] += dst[2 * k]; dm[1] += dst[2 * k + 1]; }
  for (int a = 0; a < 2; ++a) { sm[a] /= 5.0; dm[a] /= 5.0; }
  double A[2][2] = {{0, 0}, {0, 0}}, var = 0;
  for (int k = 0; k < 5; ++k) {
    const double sx = src[2 * k] - sm[0], sy = src[2 * k + 1] - sm[1], dx = dst[2 * k] - dm[0], dy = dst[2 * k + 1] - dm[1];
    A[0][0] += dx * sx; A[0][1] += dx * sy; A[1][0] += dy * sx; A[1][1] += dy * sy;
    var += sx * sx + sy * sy;
  }
  for (auto& r : A) for (auto& v : r) v /= 5.0;
  var /= 5.0;
  const double p = A[0][0] + A[1][1], q = A[1][0] - A[0][1], r = std::hypot(p, q);
  if (r == 0.0 || var == 0.0) return false;
  const double sc = r / var, c = p / r * sc, s = q / r * sc;
  M[0] = c; M[1] = -s; M[2] = dm[0] - (c * sm[0] - s * sm[1]);
  M[3] = s; M[4] = c;  M[5] = dm[1] - (s * sm[0] + c * sm[1]);
  return true;
}
const float kArcfaceDst[10] = {38.2946f, 51.6963f, 73.5318f, 51.5014f, 56.0252f, 71.7366f, 41.5493f, 92.3655f, 70.7299f, 92.2041f};

// ---- what fe_face_analyze and fe_face_analyze_mixed share: the graphs' layouts and the host glue between the three networks ----------
struct DetLayout { int fmc, K, A; const int* strides; };
DetLayout det_layout(GraphSlot& det) {
  const size_t no = det.g.model().outputs.size();
  DetLayout L{0, 0, 0, nullptr};
  if (no == 6) { L.fmc = 3; L.A = 2; }
  else if (no == 9) { L.fmc = 3; L.A = 2; L.K = 5; }
  else if (no == 10) { L.fmc = 5; L.A = 1; }
  else if (no == 15) { L.fmc = 5; L.A = 1; L.K = 5; }
  else FE_CHECK(false, "detector graph has %zu outputs; SCRFD layouts have 6, 9, 10 or 15", no);
  static const int kS3[3] = {8, 16, 32}, kS5[5] = {8, 16, 32, 64, 128};
  L.strides = L.fmc == 3 ? kS3 : kS5;
  return L;
}

// the landmark and recognition graphs of the context (null when not loaded) with the input normalisation insightface picks for them
struct FaceNets {
  GraphSlot *lmk = nullptr, *rec = nullptr;
  float lm_mean = 0, lm_scale = 1, rc_mean = 0, rc_scale = 1;
  int lm_size = 192, rc_size = 112;
};
FaceNets face_nets(fe_ctx* ctx) {
  FaceNets N;
  N.lmk = ctx->c.graphs[FE_GRAPH_FACE_LMK].get();
  N.rec = ctx->c.graphs[FE_GRAPH_FACE_REC].get();
  auto graph_norm = [](GraphSlot* g, float dflt_std, float* mean, float* scale, int* size, int dflt_size) {
    const bool self = g->g.head_has_sub() && g->g.head_has_mul();
    *mean = self ? 0.f : 127.5f;
    *scale = 1.0f / (self ? 1.0f : dflt_std);
    const auto& d = g->g.model().inputs[0].dims;
    *size = (d.size() == 4 && d[2] > 0) ? (int)d[2] : dflt_size;
  };
  if (N.lmk) graph_norm(N.lmk, 128.0f, &N.lm_mean, &N.lm_scale, &N.lm_size, 192);
  if (N.rec) graph_norm(N.rec, 127.5f, &N.rc_mean, &N.rc_scale, &N.rc_size, 112);
  const auto& lo = N.lmk ? N.lmk->g.model().outputs[0].dims : std::vector<int64_t>();
  const int lm_dim = (N.lmk && !lo.empty() && lo.back() > 0) ? (int)lo.back() : 212;
  FE_CHECK(!N.lmk || lm_dim == 212, "landmark graph yields %d values per face; the record layout holds 106 x 2", lm_dim);
  const auto& ro = N.rec ? N.rec->g.model().outputs[0].dims : std::vector<int64_t>();
  const int rc_dim = (N.rec && !ro.empty() && ro.back() > 0) ? (int)ro.back() : 512;
  FE_CHECK(!N.rec || rc_dim == 512, "recognition graph yields %d values per face; the record layout holds 512", rc_dim);
  return N;
}

// The faces of one micro-batch on the host, between the detector and the two crop graphs.
struct FaceBatch {
  std::vector<int> img;            // per face: its image inside the micro-batch
  std::vector<Cand> c;             // per face: its candidate row
  std::vector<double> Ml, Mr;      // per face: the landmark crop matrix and the recognition crop matrix (forward, 2 x 3)
  std::vector<char> rec_ok;        // per face: the 5-point similarity exists
  int m() const { return (int)c.size(); }
};
// cand: candidate rows of image b at cand + b * stride (floats), n_cand[b] of them. Sort by score (ties: level, x1, y1 - deterministic),
// NMS, keep the best max_faces; counts[b] receives the number that survived NMS.
void select_faces(const float* cand, size_t stride, const int* n_cand, int nb, float nms_thresh, int max_faces, int* counts, FaceBatch& F) {
  F.img.clear(); F.c.clear();
  for (int b = 0; b < nb; ++b) {
    std::vector<Cand> c(n_cand[b]);
    for (int q = 0; q < n_cand[b]; ++q) memcpy(c[q].v, cand + (size_t)b * stride + (size_t)q * 16, 16 * sizeof(float));
    std::sort(c.begin(), c.end(), [](const Cand& a, const Cand& b2) {
      if (a.v[0] != b2.v[0]) return a.v[0] > b2.v[0];
      if (a.v[15] != b2.v[15]) return a.v[15] < b2.v[15];
      if (a.v[1] != b2.v[1]) return a.v[1] < b2.v[1];
      return a.v[2] < b2.v[2];
    });
    std::vector<int> keep = face_nms(c, nms_thresh);
    counts[b] = (int)keep.size();
    for (int q = 0; q < (int)keep.size() && q < max_faces; ++q) { F.img.push_back(b); F.c.push_back(c[keep[q]]); }
  }
}
// Landmark.get: face_align.transform(img, center, size, size / (max(w,h) * 1.5), 0)
void landmark_matrices(FaceBatch& F, int lm_size) {
  const int m = F.m();
  F.Ml.assign((size_t)m * 6, 0.0);
  for (int f = 0; f < m; ++f) {
    const double x1 = F.c[f].v[1], y1 = F.c[f].v[2], x2 = F.c[f].v[3], y2 = F.c[f].v[4];
    const double bw = x2 - x1, bh = y2 - y1, cx = (x2 + x1) / 2, cy = (y2 + y1) / 2;
    const double sc = lm_size / (std::max(bw, bh) * 1.5);
    double* M = &F.Ml[(size_t)f * 6];
    M[0] = sc; M[1] = 0; M[2] = -cx * sc + lm_size / 2.0;
    M[3] = 0; M[4] = sc; M[5] = -cy * sc + lm_size / 2.0;
  }
}
// face_align.norm_crop: the similarity of the five keypoints onto the ArcFace template; the identity where it does not exist
void recognition_matrices(FaceBatch& F, int rc_size) {
  const int m = F.m();
  F.Mr.assign((size_t)m * 6, 0.0);
  F.rec_ok.assign(m, 0);
  double dst[10];
  for (int q = 0; q < 10; ++q) dst[q] = (double)kArcfaceDst[q] * ((double)rc_size / 112.0);
  for (int f = 0; f < m; ++f) {
    F.rec_ok[f] = similarity5(&F.c[f].v[5], dst, &F.Mr[(size_t)f * 6]) ? 1 : 0;
    if (!F.rec_ok[f]) { double* M = &F.Mr[(size_t)f * 6]; M[0] = M[4] = 1; M[1] = M[2] = M[3] = M[5] = 0; }
  }
}
// faces: the records of the micro-batch's first image. h_lmk [m][212] / h_emb [m][512]: the graphs' outputs, null when the graph did not run.
void write_face_records(const FaceBatch& F, int nb, int max_faces, int lm_size, const float* h_lmk, const float* h_emb, float* faces) {
  std::vector<int> slot_of(nb, 0);
  for (int f = 0; f < F.m(); ++f) {
    const int b = F.img[f];
    float* o = faces + ((size_t)b * max_faces + slot_of[b]++) * FE_FACE_FLOATS;
    o[0] = F.c[f].v[1]; o[1] = F.c[f].v[2]; o[2] = F.c[f].v[3]; o[3] = F.c[f].v[4]; o[4] = F.c[f].v[0];
    memcpy(o + 5, &F.c[f].v[5], 10 * sizeof(float));
    if (h_lmk) {   // pred in [-1,1] -> crop pixels -> image through the inverse crop matrix (trans_points2d)
      const double* M = &F.Ml[(size_t)f * 6];
      const double D = 1.0 / (M[0] * M[4]);   // rotation 0: diagonal matrix
      const double i00 = M[4] * D, i11 = M[0] * D, i02 = -i00 * M[2], i12 = -i11 * M[5];
      for (int q = 0; q < 106; ++q) {
        const float px = (h_lmk[(size_t)f * 212 + 2 * q] + 1.f) * (float)(lm_size / 2);
        const float py = (h_lmk[(size_t)f * 212 + 2 * q + 1] + 1.f) * (float)(lm_size / 2);
        o[15 + 2 * q] = (float)(i00 * (double)px + 0.0 * (double)py + i02);
        o[16 + 2 * q] = (float)(0.0 * (double)px + i11 * (double)py + i12);
      }
    }
    if (h_emb && F.rec_ok[f]) memcpy(o + 15 + 212, &h_emb[(size_t)f * 512], 512 * sizeof(float));
  }
}

// ---- the mixed-size calls ---------------------------------------------------------------------------------------------------------
using face_plan::ImageDesc;
constexpr MixedLimits kFaceLimits = {1, 65535, 65535, ((size_t)1 << 31) - 1, "below 2^31"};

// src of every descriptor: the caller's pointer when the images are resident, else a copy in the arena on a 256-byte boundary. An image
// that does not fit with `reserve` bytes left for the call's own scratch is a CapacityError that names it.
void place_images(Ctx& C, const char* who, const uint8_t* const* images, const int32_t* hw, int n, int on_device, size_t reserve, ImageDesc* descs) {
  std::vector<size_t> offs;
  const size_t total = on_device ? 0 : mixed_list::staged_offsets(hw, 0, n, true, offs), first = mixed_list::align_up(C.arena.mark());
  for (int i = 0; i < n && !on_device; ++i) {
    const size_t bytes = mixed_list::image_bytes(hw, i), at = first + offs[i];
    if (at + bytes + reserve > C.arena.capacity()) {
      char b[200];
      snprintf(b, sizeof b, "%s: image %d (%d x %d) does not fit: %zu bytes at %zu with %zu reserved, the arena holds %zu", who, i, hw[2 * i], hw[2 * i + 1],
               bytes, at, reserve, C.arena.capacity());
      throw CapacityError(b);
    }
  }
  uint8_t* d_stage = on_device ? nullptr : (uint8_t*)C.arena.alloc(total);
  stage_images(C, images, hw, 0, n, on_device, d_stage, offs.data(), [&](int i, const uint8_t* src) { descs[i].src = src; });
}
// descriptors that carry only src, h, w (crops, ROIs, thumbnails), placed and uploaded
const ImageDesc* plain_descs(Ctx& C, const char* who, const uint8_t* const* images, const int32_t* hw, int n, int on_device, size_t reserve,
                             std::vector<ImageDesc>& descs) {
  descs.assign(n, ImageDesc{});
  for (int i = 0; i < n; ++i) { descs[i].h = hw[2 * i]; descs[i].w = hw[2 * i + 1]; }
  place_images(C, who, images, hw, n, on_device, reserve + (size_t)n * sizeof(ImageDesc) + 4096, descs.data());
  return upload(C, descs.data(), descs.size());
}
bool det_size_ok(Ctx& C, const char* who, int det_h, int det_w) {
  if (det_h >= 32 && det_w >= 32 && det_h % 32 == 0 && det_w % 32 == 0) return true;
  char b[160];
  snprintf(b, sizeof b, "%s: detector input %d x %d; both sides must be multiples of 32, at least 32", who, det_h, det_w);
  C.err = b;
  return false;
}
// The detector descriptors of the whole list and the call's weight tables; false (FE_ERR_INVALID, message stored) names the image whose
// aspect ratio leaves an empty detector input.
bool describe_list(Ctx& C, const char* who, const int32_t* hw, int n, int det_h, int det_w, std::vector<ImageDesc>& descs, face_plan::TablePool& pool) {
  descs.assign(n, ImageDesc{});
  for (int i = 0; i < n; ++i)
    if (!face_plan::describe(hw, i, det_h, det_w, pool, cv_resize_tables, descs[i])) {
      char b[200];
      snprintf(b, sizeof b, "%s: image %d is %d x %d (h x w): its aspect ratio leaves an empty detector input (%d x %d)", who, i, hw[2 * i], hw[2 * i + 1],
               descs[i].new_h, descs[i].new_w);
      C.err = b;
      return false;
    }
  return true;
}
void ensure_warp_wtab(fe_ctx* ctx) {
  if (ctx->warp_wtab) return;
  std::vector<short> wt;
  cv_warp_weight_table(wt);
  FE_HIP(hipMalloc((void**)&ctx->warp_wtab, wt.size() * sizeof(short)));
  ctx->misc_allocs.push_back(ctx->warp_wtab);
  FE_HIP(hipMemcpy(ctx->warp_wtab, wt.data(), wt.size() * sizeof(short), hipMemcpyHostToDevice));
}
// cv::warpAffine inverts the forward matrix in double before walking the destination
void invert_crop_matrices(const double* M, int m, std::vector<double>& inv) {
  inv.assign((size_t)m * 6, 0.0);
  for (int f = 0; f < m; ++f) {
    const double* a = M + (size_t)f * 6;
    double D = a[0] * a[4] - a[1] * a[3];
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A11 = a[4] * D, A22 = a[0] * D;
    double* o = &inv[(size_t)f * 6];
    o[0] = A11; o[1] = a[1] * (-D); o[3] = a[3] * (-D); o[4] = A22;
    o[2] = -o[0] * a[2] - o[1] * a[5];
    o[5] = -o[3] * a[2] - o[4] * a[5];
  }
}
// run_face_crops for crops of images of different sizes: d_descs are the device descriptors img_index (host, already checked) refers to.
// Without crops_out the warp writes the graph's fp32 input directly. rev: the byte order of the source is the reverse of what the graph
// takes in channel 0 .. 2. inv is the caller's: it and img_index must outlive the stream's work (nothing here synchronises).
void run_face_crops_mixed(fe_ctx* ctx, GraphSlot* gs, const ImageDesc* d_descs, int m, const int* img_index, const double* M, int size, float mean,
                          float scale, int rev, float* d_out, int out_dim, uint8_t* crops_out, std::vector<double>& inv) {
  Ctx& C = ctx->c;
  if (m <= 0) return;
  ensure_warp_wtab(ctx);
  invert_crop_matrices(M, m, inv);
  double* d_inv = upload(C, inv.data(), inv.size());
  int* d_idx = upload(C, img_index, (size_t)m);
  const size_t base = C.arena.mark();
  const int mb = std::max(1, ctx->microbatch * 8);   // as run_face_crops
  for (int f0 = 0; f0 < m; f0 += mb) {
    const int fb = std::min(mb, m - f0);
    C.arena.rewind(base);
    uint8_t* crops = nullptr;
    if (crops_out) {
      crops = (uint8_t*)C.arena.alloc((size_t)fb * size * size * 3);
      launch_warp_affine_mixed(d_descs, d_idx + f0, d_inv + (size_t)f0 * 6, fb, size, ctx->warp_wtab, crops, C.stream);
      FE_HIP(hipMemcpyAsync(crops_out + (size_t)f0 * size * size * 3, crops, (size_t)fb * size * size * 3, hipMemcpyDeviceToHost, C.stream));
    }
    if (d_out) {
      Tensor x = C.arena.tensor(fb, size, size, 4);
      if (crops) launch_u8_blob(crops, x.p, (size_t)fb * size * size, mean, scale, rev, C.stream);
      else launch_warp_affine_blob_mixed(d_descs, d_idx + f0, d_inv + (size_t)f0 * 6, fb, size, ctx->warp_wtab, x.p, mean, scale, rev ? 2 : 0, C.stream);
      std::vector<GraphOutput> outs;
      gs->g.run(C, x, 3, outs);
      FE_CHECK(outs[0].numel == (size_t)fb * out_dim, "graph output has %zu values for %d crops, expected %d each", outs[0].numel, fb, out_dim);
      FE_HIP(hipMemcpyAsync(d_out + (size_t)f0 * out_dim, outs[0].dev, outs[0].numel * sizeof(float), hipMemcpyDeviceToDevice, C.stream));
    }
  }
}
}  // namespace

extern "C" {

int fe_face_detect(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int det_h, int det_w, float thresh,
                   int max_cand, float* cand, int* counts, float* det_scale_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    GraphSlot& gs = graph_slot(ctx, FE_GRAPH_FACE_DET);
    FE_CHECK(bgr && cand && counts && n > 0 && h > 0 && w > 0 && det_h >= 32 && det_w >= 32 && det_h % 32 == 0 && det_w % 32 == 0 &&
                 max_cand > 0, "bad arguments");
    // SCRFD.detect: keep the aspect ratio, fill the top-left of the det canvas (insightface model_zoo/scrfd.py [DEP-KNOWLEDGE])
    const float im_ratio = (float)h / (float)w, model_ratio = (float)det_h / (float)det_w;
    int new_h, new_w;
    if (im_ratio > model_ratio) { new_h = det_h; new_w = (int)((float)new_h / im_ratio); }
    else { new_w = det_w; new_h = (int)((float)new_w * im_ratio); }
    FE_CHECK(new_h > 0 && new_w > 0, "image aspect ratio leaves an empty detector input");
    const float det_scale = (float)new_h / (float)h;
    if (det_scale_out) *det_scale_out = det_scale;
    const bool area2 = (h == 2 * new_h && w == 2 * new_w);
    const bool copy_only = (h == new_h && w == new_w);
    auto tx = cv_resize_tab(ctx, w, new_w, true), ty = cv_resize_tab(ctx, h, new_h, false);

    const size_t no = gs.g.model().outputs.size();
    int fmc, K = 0, A;
    if (no == 6) { fmc = 3; A = 2; }
    else if (no == 9) { fmc = 3; A = 2; K = 5; }
    else if (no == 10) { fmc = 5; A = 1; }
    else if (no == 15) { fmc = 5; A = 1; K = 5; }
    else FE_CHECK(false, "detector graph has %zu outputs; SCRFD layouts have 6, 9, 10 or 15", no);
    static const int kStrides3[3] = {8, 16, 32}, kStrides5[5] = {8, 16, 32, 64, 128};
    const int* strides = fmc == 3 ? kStrides3 : kStrides5;

    const size_t per = (size_t)h * w * 3;
    float* d_cand = ctx->out_buf((size_t)n * max_cand * 16 + (size_t)n + 16);
    int* d_counts = (int*)(d_cand + (size_t)n * max_cand * 16);
    FE_HIP(hipMemsetAsync(d_counts, 0, (size_t)n * sizeof(int), C.stream));
    const int mbn = ctx->microbatch * 2;   // see fe_face_analyze
    ImageStager st(ctx, bgr, n, per, mbn, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int i0 = k * mbn, nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      uint8_t* canvas = (uint8_t*)C.arena.alloc((size_t)nb * det_h * det_w * 3);
      FE_HIP(hipMemsetAsync(canvas, 0, (size_t)nb * det_h * det_w * 3, C.stream));
      if (copy_only) {
        for (int b = 0; b < nb; ++b)
          FE_HIP(hipMemcpy2DAsync(canvas + (size_t)b * det_h * det_w * 3, (size_t)det_w * 3, d_in + (size_t)b * per, (size_t)w * 3, (size_t)w * 3, h,
                                  hipMemcpyDeviceToDevice, C.stream));
      } else {
        launch_cv_resize_linear(d_in, nb, h, w, canvas, det_h, det_w, new_h, new_w, tx.ofs, tx.coef, ty.ofs, ty.coef, area2 ? 1 : 0, C.stream);
      }
      st.done(k);
      Tensor x = C.arena.tensor(nb, det_h, det_w, 4);
      launch_u8_blob(canvas, x.p, (size_t)nb * det_h * det_w, 127.5f, 1.0f / 128.0f, 1, C.stream);
      std::vector<GraphOutput> outs;
      gs.g.run(C, x, 3, outs);
      for (int l = 0; l < fmc; ++l) {
        const int s = strides[l], fh = det_h / s, fw = det_w / s;
        const size_t rows = (size_t)nb * fh * fw * A;
        FE_CHECK(outs[l].numel == rows && outs[l + fmc].numel == rows * 4 && (!K || outs[l + 2 * fmc].numel == rows * 2 * K),
                 "detector output %d has %zu values, expected %zu rows for stride %d", l, outs[l].numel, rows, s);
        launch_scrfd_decode(outs[l].dev, outs[l + fmc].dev, K ? outs[l + 2 * fmc].dev : nullptr, nb, fh, fw, A, K, s, thresh, det_scale, l,
                            d_cand + (size_t)i0 * max_cand * 16, d_counts + i0, max_cand, C.stream);
      }
    }
    FE_HIP(hipMemcpyAsync(counts, d_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(cand, d_cand, (size_t)n * max_cand * 16 * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

int fe_face_crops_run(fe_ctx* ctx, int slot, const uint8_t* bgr, int n, int h, int w, int on_device, int m, const int* img_index,
                      const double* M, int size, float mean, float scale, int swap_rb, float* out, int out_dim, uint8_t* crops_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(bgr && n > 0 && h > 0 && w > 0 && m >= 0 && size > 0 && (m == 0 || (img_index && M)), "bad arguments");
    FE_CHECK(out || crops_out, "nothing to compute: both outputs are null");
    GraphSlot* gs = out ? &graph_slot(ctx, slot) : nullptr;
    if (m == 0) return FE_OK;
    C.arena.reset();
    const uint8_t* d_img = resident(C, bgr, (size_t)n * h * w * 3, on_device);
    float* d_out = out ? ctx->out_buf((size_t)m * out_dim) : nullptr;
    run_face_crops(ctx, gs, d_img, n, h, w, m, img_index, M, size, mean, scale, swap_rb, d_out, out_dim, crops_out);
    if (out) FE_HIP(hipMemcpyAsync(out, d_out, (size_t)m * out_dim * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

// ---- FaceAnalysis.get for a whole batch, host glue in C++ ---------------------------------------------------------------
int fe_face_analyze(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int det_h, int det_w, float det_thresh,
                    float nms_thresh, int max_faces, float* faces, int* counts, int* models_run) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    GraphSlot& det = graph_slot(ctx, FE_GRAPH_FACE_DET);
    GraphSlot* lmk = ctx->c.graphs[FE_GRAPH_FACE_LMK].get();
    GraphSlot* rec = ctx->c.graphs[FE_GRAPH_FACE_REC].get();
    FE_CHECK(bgr && faces && counts && n > 0 && h > 0 && w > 0 && max_faces > 0 && det_h >= 32 && det_w >= 32 && det_h % 32 == 0 &&
                 det_w % 32 == 0, "bad arguments");
    if (models_run) *models_run = 1 | (lmk ? 2 : 0) | (rec ? 4 : 0);
    int32_t new_h, new_w, mode;
    float det_scale;
    FE_CHECK(face_plan::fit(h, w, det_h, det_w, new_h, new_w, det_scale, mode), "image aspect ratio leaves an empty detector input");
    const bool area2 = mode == face_plan::kBox2, copy_only = mode == face_plan::kCopy;
    auto tx = cv_resize_tab(ctx, w, new_w, true), ty = cv_resize_tab(ctx, h, new_h, false);
    const DetLayout L = det_layout(det);
    const int fmc = L.fmc, K = L.K, A = L.A;
    const int* strides = L.strides;
    const FaceNets N = face_nets(ctx);

    const int max_cand = 4096;
    const size_t per = (size_t)h * w * 3;
    const int mbn = ctx->microbatch * 2;   // the detector's footprint at 640^2 is ~10x below TOPIQ's at 1024^2: larger chunks fill the chip better
    memset(faces, 0, (size_t)n * max_faces * FE_FACE_FLOATS * sizeof(float));
    std::vector<float> h_cand((size_t)mbn * max_cand * 16), h_lmk, h_emb;
    std::vector<int> h_counts(mbn);
    FaceBatch F;
    // device image access for the crop stage: resident input is used in place; host input is staged per micro-batch
    ImageStager st(ctx, bgr, n, per, mbn, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int i0 = k * mbn, nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      float* d_cand = (float*)C.arena.alloc((size_t)nb * max_cand * 16 * sizeof(float));
      int* d_counts = (int*)C.arena.alloc((size_t)nb * sizeof(int));
      FE_HIP(hipMemsetAsync(d_counts, 0, (size_t)nb * sizeof(int), C.stream));
      const size_t keep_mark = C.arena.mark();
      uint8_t* canvas = (uint8_t*)C.arena.alloc((size_t)nb * det_h * det_w * 3);
      FE_HIP(hipMemsetAsync(canvas, 0, (size_t)nb * det_h * det_w * 3, C.stream));
      if (copy_only) {
        for (int b = 0; b < nb; ++b)
          FE_HIP(hipMemcpy2DAsync(canvas + (size_t)b * det_h * det_w * 3, (size_t)det_w * 3, d_in + (size_t)b * per, (size_t)w * 3, (size_t)w * 3, h,
                                  hipMemcpyDeviceToDevice, C.stream));
      } else {
        launch_cv_resize_linear(d_in, nb, h, w, canvas, det_h, det_w, new_h, new_w, tx.ofs, tx.coef, ty.ofs, ty.coef, area2 ? 1 : 0, C.stream);
      }
      Tensor x = C.arena.tensor(nb, det_h, det_w, 4);
      launch_u8_blob(canvas, x.p, (size_t)nb * det_h * det_w, 127.5f, 1.0f / 128.0f, 1, C.stream);
      std::vector<GraphOutput> outs;
      det.g.run(C, x, 3, outs);
      for (int l = 0; l < fmc; ++l) {
        const int s = strides[l], fh = det_h / s, fw = det_w / s;
        const size_t rows = (size_t)nb * fh * fw * A;
        FE_CHECK(outs[l].numel == rows && outs[l + fmc].numel == rows * 4 && (!K || outs[l + 2 * fmc].numel == rows * 2 * K),
                 "detector output %d has %zu values, expected %zu rows for stride %d", l, outs[l].numel, rows, s);
        launch_scrfd_decode(outs[l].dev, outs[l + fmc].dev, K ? outs[l + 2 * fmc].dev : nullptr, nb, fh, fw, A, K, s, det_thresh, det_scale, l,
                            d_cand, d_counts, max_cand, C.stream);
      }
      FE_HIP(hipMemcpyAsync(h_counts.data(), d_counts, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
      int maxc = 0;
      for (int b = 0; b < nb; ++b) { h_counts[b] = std::min(h_counts[b], max_cand); maxc = std::max(maxc, h_counts[b]); }
      if (maxc > 0) {
        FE_HIP(hipMemcpy2DAsync(h_cand.data(), (size_t)maxc * 16 * sizeof(float), d_cand, (size_t)max_cand * 16 * sizeof(float),
                                (size_t)maxc * 16 * sizeof(float), nb, hipMemcpyDeviceToHost, C.stream));
        FE_HIP(hipStreamSynchronize(C.stream));
      }
      select_faces(h_cand.data(), (size_t)maxc * 16, h_counts.data(), nb, nms_thresh, max_faces, counts + i0, F);
      const int m = F.m();
      C.arena.rewind(keep_mark);   // detector activations are no longer needed; candidates were copied out
      float *d_lmk = nullptr, *d_emb = nullptr;
      if (m > 0 && lmk) {
        landmark_matrices(F, N.lm_size);
        d_lmk = (float*)C.arena.alloc((size_t)m * 212 * sizeof(float));
        run_face_crops(ctx, lmk, d_in, nb, h, w, m, F.img.data(), F.Ml.data(), N.lm_size, N.lm_mean, N.lm_scale, 1, d_lmk, 212, nullptr);
        h_lmk.resize((size_t)m * 212);
        FE_HIP(hipMemcpyAsync(h_lmk.data(), d_lmk, h_lmk.size() * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      }
      if (m > 0 && rec && K == 5) {
        recognition_matrices(F, N.rc_size);
        d_emb = (float*)C.arena.alloc((size_t)m * 512 * sizeof(float));
        run_face_crops(ctx, rec, d_in, nb, h, w, m, F.img.data(), F.Mr.data(), N.rc_size, N.rc_mean, N.rc_scale, 1, d_emb, 512, nullptr);
        h_emb.resize((size_t)m * 512);
        FE_HIP(hipMemcpyAsync(h_emb.data(), d_emb, h_emb.size() * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      }
      FE_HIP(hipStreamSynchronize(C.stream));
      st.done(k);
      write_face_records(F, nb, max_faces, N.lm_size, d_lmk ? h_lmk.data() : nullptr, d_emb ? h_emb.data() : nullptr,
                         faces + (size_t)i0 * max_faces * FE_FACE_FLOATS);
    }
  });
}

/* cv2.resize(img, (ow, oh)) INTER_LINEAR on uint8 HWC images (restated fixed-point path); exposed for the parity tests */
int fe_cv_resize_linear_u8(fe_ctx* ctx, const uint8_t* src, int n, int h, int w, int oh, int ow, uint8_t* dst) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(src && dst && n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "bad arguments");
    C.arena.reset();
    uint8_t* d_src = upload(C, src, (size_t)n * h * w * 3);
    uint8_t* d_dst = (uint8_t*)C.arena.alloc((size_t)n * oh * ow * 3);
    auto tx = cv_resize_tab(ctx, w, ow, true), ty = cv_resize_tab(ctx, h, oh, false);
    if (h == oh && w == ow) FE_HIP(hipMemcpyAsync(d_dst, d_src, (size_t)n * h * w * 3, hipMemcpyDeviceToDevice, C.stream));
    else launch_cv_resize_linear(d_src, n, h, w, d_dst, oh, ow, oh, ow, tx.ofs, tx.coef, ty.ofs, ty.coef, (h == 2 * oh && w == 2 * ow) ? 1 : 0, C.stream);
    FE_HIP(hipMemcpyAsync(dst, d_dst, (size_t)n * oh * ow * 3, hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

/* Laplacian statistics of m rectangular ROIs of a BGR batch (reference analyzers/face.py:160-176, 272-279) */
int fe_roi_laplacian(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int m, const int* img_index, const int* rois,
                     double* out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(bgr && n > 0 && h > 0 && w > 0 && m >= 0 && (m == 0 || (img_index && rois && out)), "bad arguments");
    if (m == 0) return FE_OK;
    for (int f = 0; f < m; ++f) {
      FE_CHECK(img_index[f] >= 0 && img_index[f] < n, "roi %d refers to image %d of %d", f, img_index[f], n);
      const int* r = rois + 4 * f;
      FE_CHECK(r[0] >= 0 && r[1] >= 0 && r[2] <= w && r[3] <= h, "roi %d = [%d,%d,%d,%d] leaves the %dx%d image", f, r[0], r[1], r[2], r[3], w, h);
    }
    C.arena.reset();
    const uint8_t* d_img = resident(C, bgr, (size_t)n * h * w * 3, on_device);
    int* d_idx = upload(C, img_index, (size_t)m);
    int* d_roi = upload(C, rois, (size_t)m * 4);
    double* d_out = (double*)C.arena.alloc((size_t)m * 4 * sizeof(double));
    launch_roi_laplacian(d_img, h, w, d_idx, d_roi, m, d_out, C.stream);
    FE_HIP(hipMemcpyAsync(out, d_out, (size_t)m * 4 * sizeof(double), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

/* face thumbnails: m crops of a BGR batch, each BOX-resized to its own size and encoded (reference analyzers/face.py:43-82) */
int fe_face_thumbnails(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int m, const int32_t* img_index, const int32_t* crops,
                       const int32_t* out_sizes, int quality, uint8_t* out, size_t cap, int32_t* lengths) {
  return fe_api(ctx, OnError::Capacity, [&] {
    char msg[200] = "";
    if (!(bgr && n > 0 && h > 0 && w > 0 && h <= 65535 && w <= 65535 && m >= 0 && (m == 0 || (img_index && crops && out_sizes && out && lengths))))
      snprintf(msg, sizeof msg, "face_thumbnails: bad arguments");
    else if (quality < 1 || quality > 100)
      snprintf(msg, sizeof msg, "face_thumbnails: quality %d (1 .. 100)", quality);
    for (int f = 0; f < m && !msg[0]; ++f) {
      const int32_t* r = crops + 4 * f;
      const int32_t ow = out_sizes[2 * f], oh = out_sizes[2 * f + 1];
      if (img_index[f] < 0 || img_index[f] >= n) snprintf(msg, sizeof msg, "face_thumbnails: face %d refers to image %d of %d", f, img_index[f], n);
      else if (r[0] < 0 || r[1] < 0 || r[2] > w || r[3] > h || r[0] >= r[2] || r[1] >= r[3])
        snprintf(msg, sizeof msg, "face_thumbnails: crop %d = [%d,%d,%d,%d] is empty or leaves the %dx%d image", f, r[0], r[1], r[2], r[3], w, h);
      else if (ow < 1 || oh < 1 || ow > FE_FACE_THUMB_MAX_SIDE || oh > FE_FACE_THUMB_MAX_SIDE)
        snprintf(msg, sizeof msg, "face_thumbnails: output size %d x %d of face %d (1 .. %d)", ow, oh, f, FE_FACE_THUMB_MAX_SIDE);
    }
    if (msg[0]) { ctx->c.err = msg; return FE_ERR_INVALID; }
    if (m == 0) return FE_OK;
    Ctx& C = ctx->c;
    C.arena.reset();
    const uint8_t* d_img = resident(C, bgr, (size_t)n * h * w * 3, on_device);
    if (!face_thumbnails(C, d_img, n, h, w, m, img_index, crops, out_sizes, quality, out, cap, lengths)) {
      char b[200];
      snprintf(b, sizeof(b), "face_thumbnails: a face needs more than the %zu bytes of its output row (fe_jpeg_bound(max oh, max ow) always fits)", cap);
      throw CapacityError(b);
    }
    return FE_OK;
  });
}

/* ---- the face calls for a list of images that each have their own size ---------------------------------------------------------------- */

int fe_face_cache_entries(fe_ctx* ctx, int32_t* entries) {
  return fe_api(ctx, [&] {
    FE_CHECK(entries, "bad arguments");
    *entries = (int32_t)ctx->cvresize.size();
  });
}

/* the detector input of every image of the list, as fe_face_analyze_mixed feeds it to the graph: out [n][det_h][det_w][4] fp32 (host) */
int fe_face_det_input_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int det_h, int det_w, float* out) {
  return fe_api(ctx, OnError::Capacity, [&] {
    Ctx& C = ctx->c;
    const char* who = "fe_face_det_input_mixed";
    if (!mixed_list_ok(C, who, (images && out) ? images : nullptr, hw, n, order, images, kFaceLimits)) return FE_ERR_INVALID;
    if (!det_size_ok(C, who, det_h, det_w)) return FE_ERR_INVALID;
    std::vector<ImageDesc> descs;
    face_plan::TablePool pool;
    if (!describe_list(C, who, hw, n, det_h, det_w, descs, pool)) return FE_ERR_INVALID;
    C.arena.reset();
    const int32_t* d_pool = pool.words.empty() ? nullptr : upload(C, pool.words.data(), pool.words.size());
    const int mbn = std::max(1, ctx->microbatch * 2);
    const size_t px = (size_t)det_h * det_w, mark = C.arena.mark();
    for (int i0 = 0; i0 < n; i0 += mbn) {
      const int nb = std::min(mbn, n - i0);
      C.arena.rewind(mark);
      float* x = (float*)C.arena.alloc((size_t)nb * px * 4 * sizeof(float));
      place_images(C, who, images + i0, hw + 2 * (size_t)i0, nb, on_device, (size_t)nb * sizeof(ImageDesc) + 4096, descs.data() + i0);
      const ImageDesc* d_desc = upload(C, descs.data() + i0, (size_t)nb);
      launch_det_input_mixed(d_desc, nb, d_pool, det_h, det_w, order == FE_ORDER_RGB, x, C.stream);
      FE_HIP(hipMemcpyAsync(out + (size_t)i0 * px * 4, x, (size_t)nb * px * 4 * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));      // the arena is recycled by the next micro-batch
    }
    return FE_OK;
  });
}

/* fe_face_crops_run over a list of images of any sizes */
int fe_face_crops_run_mixed(fe_ctx* ctx, int slot, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int m,
                            const int* img_index, const double* M, int size, float mean, float scale, int swap_rb, float* out, int out_dim,
                            uint8_t* crops_out) {
  return fe_api(ctx, OnError::Capacity, [&] {
    Ctx& C = ctx->c;
    const char* who = "fe_face_crops_run_mixed";
    if (!mixed_list_ok(C, who, images, hw, n, order, images, kFaceLimits)) return FE_ERR_INVALID;
    FE_CHECK(m >= 0 && size > 0 && (m == 0 || (img_index && M)), "bad arguments");
    FE_CHECK(out || crops_out, "nothing to compute: both outputs are null");
    for (int f = 0; f < m; ++f) FE_CHECK(img_index[f] >= 0 && img_index[f] < n, "crop %d refers to image %d of %d", f, img_index[f], n);
    GraphSlot* gs = out ? &graph_slot(ctx, slot) : nullptr;
    if (m == 0) return FE_OK;
    C.arena.reset();
    std::vector<ImageDesc> descs;
    std::vector<double> inv;
    const int mb = std::max(1, ctx->microbatch * 8);
    const ImageDesc* d_desc = plain_descs(C, who, images, hw, n, on_device, (size_t)std::min(m, mb) * size * size * 3 + (size_t)m * 64, descs);
    float* d_out = out ? ctx->out_buf((size_t)m * out_dim) : nullptr;
    run_face_crops_mixed(ctx, gs, d_desc, m, img_index, M, size, mean, scale, (swap_rb ? 1 : 0) ^ (order == FE_ORDER_RGB ? 1 : 0), d_out, out_dim, crops_out, inv);
    if (out) FE_HIP(hipMemcpyAsync(out, d_out, (size_t)m * out_dim * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

/* FaceAnalysis.get for a list of images of any sizes in ONE call: every graph runs over full micro-batches whatever the shapes */
int fe_face_analyze_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int det_h, int det_w,
                          float det_thresh, float nms_thresh, int max_faces, float* faces, int* counts, int* models_run) {
  return fe_api(ctx, OnError::Capacity, [&] {
    Ctx& C = ctx->c;
    const char* who = "fe_face_analyze_mixed";
    if (!mixed_list_ok(C, who, (images && faces && counts) ? images : nullptr, hw, n, order, images, kFaceLimits))
      return FE_ERR_INVALID;
    if (!det_size_ok(C, who, det_h, det_w)) return FE_ERR_INVALID;
    if (max_faces <= 0) { C.err = "fe_face_analyze_mixed: max_faces must be positive"; return FE_ERR_INVALID; }
    std::vector<ImageDesc> descs;
    face_plan::TablePool pool;
    if (!describe_list(C, who, hw, n, det_h, det_w, descs, pool)) return FE_ERR_INVALID;
    const bool staged = !on_device;
    const size_t stage_room = C.arena.capacity() / 4;      // the rest is the graphs'
    const int bad = face_plan::too_large(hw, n, staged, stage_room);
    if (bad >= 0) {
      char b[200];
      snprintf(b, sizeof b, "%s: image %d (%d x %d) needs %zu bytes of staging, the arena (%zu bytes) gives staged pixels %zu", who, bad, hw[2 * bad],
               hw[2 * bad + 1], face_plan::staged_bytes(hw[2 * bad], hw[2 * bad + 1]), C.arena.capacity(), stage_room);
      throw CapacityError(b);
    }
    GraphSlot& det = graph_slot(ctx, FE_GRAPH_FACE_DET);
    const DetLayout L = det_layout(det);
    const FaceNets N = face_nets(ctx);
    if (models_run) *models_run = 1 | (N.lmk ? 2 : 0) | (N.rec ? 4 : 0);
    const int rgb = order == FE_ORDER_RGB ? 1 : 0;

    const int max_cand = 4096, head_rows = 255;      // head_rows: candidate rows that come down with the counts
    const size_t rec_floats = (size_t)(max_cand + 1) * 16, head_floats = (size_t)(head_rows + 1) * 16;
    const int mbn = std::max(1, ctx->microbatch * 2);   // as fe_face_analyze
    memset(faces, 0, (size_t)n * max_faces * FE_FACE_FLOATS * sizeof(float));
    std::vector<float> h_head((size_t)mbn * head_floats), h_full, h_lmk, h_emb;
    std::vector<int> h_counts(mbn);
    std::vector<size_t> offs;
    std::vector<double> inv_l, inv_r;
    FaceBatch F;
    C.arena.reset();
    const int32_t* d_pool = pool.words.empty() ? nullptr : upload(C, pool.words.data(), pool.words.size());
    const size_t base = C.arena.mark();
    for (int i0 = 0; i0 < n;) {
      size_t stage_b = 0;
      const int i1 = face_plan::cut(hw, n, i0, mbn, staged, stage_room, &offs, &stage_b);
      const int nb = i1 - i0;
      C.arena.rewind(base);
      ImageDesc* d_desc = (ImageDesc*)C.arena.alloc((size_t)nb * sizeof(ImageDesc));
      uint8_t* d_stage = staged ? (uint8_t*)C.arena.alloc(stage_b) : nullptr;
      stage_images(C, images, hw, i0, i1, on_device, d_stage, offs.data(), [&](int i, const uint8_t* src) { descs[i].src = src; });
      FE_HIP(hipMemcpyAsync(d_desc, descs.data() + i0, (size_t)nb * sizeof(ImageDesc), hipMemcpyHostToDevice, C.stream));
      float* d_rec = (float*)C.arena.alloc((size_t)nb * rec_floats * sizeof(float));
      FE_HIP(hipMemset2DAsync(d_rec, rec_floats * sizeof(float), 0, 16 * sizeof(float), nb, C.stream));      // the counts
      const size_t keep_mark = C.arena.mark();
      Tensor x = C.arena.tensor(nb, det_h, det_w, 4);
      launch_det_input_mixed(d_desc, nb, d_pool, det_h, det_w, rgb, x.p, C.stream);
      std::vector<GraphOutput> outs;
      det.g.run(C, x, 3, outs);
      for (int l = 0; l < L.fmc; ++l) {
        const int s = L.strides[l], fh = det_h / s, fw = det_w / s;
        const size_t rows = (size_t)nb * fh * fw * L.A;
        FE_CHECK(outs[l].numel == rows && outs[l + L.fmc].numel == rows * 4 && (!L.K || outs[l + 2 * L.fmc].numel == rows * 2 * L.K),
                 "detector output %d has %zu values, expected %zu rows for stride %d", l, outs[l].numel, rows, s);
        launch_scrfd_decode_mixed(outs[l].dev, outs[l + L.fmc].dev, L.K ? outs[l + 2 * L.fmc].dev : nullptr, nb, fh, fw, L.A, L.K, s, det_thresh, d_desc, l,
                                  d_rec, max_cand, C.stream);
      }
      // one copy brings the counts and the first head_rows candidates of every image; only an image with more costs a second one
      FE_HIP(hipMemcpy2DAsync(h_head.data(), head_floats * sizeof(float), d_rec, rec_floats * sizeof(float), head_floats * sizeof(float), nb,
                              hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
      int maxc = 0;
      for (int b = 0; b < nb; ++b) {
        int cnt;
        memcpy(&cnt, &h_head[(size_t)b * head_floats], sizeof(int));
        h_counts[b] = std::min(cnt, max_cand);
        maxc = std::max(maxc, h_counts[b]);
      }
      const float* cand = h_head.data() + 16;
      size_t stride = head_floats;
      if (maxc > head_rows) {
        stride = (size_t)(maxc + 1) * 16;
        h_full.resize((size_t)nb * stride);
        FE_HIP(hipMemcpy2DAsync(h_full.data(), stride * sizeof(float), d_rec, rec_floats * sizeof(float), stride * sizeof(float), nb, hipMemcpyDeviceToHost,
                                C.stream));
        FE_HIP(hipStreamSynchronize(C.stream));
        cand = h_full.data() + 16;
      }
      select_faces(cand, stride, h_counts.data(), nb, nms_thresh, max_faces, counts + i0, F);
      const int m = F.m();
      C.arena.rewind(keep_mark);   // detector activations are no longer needed; candidates were copied out
      float *d_lmk = nullptr, *d_emb = nullptr;
      if (m > 0 && N.lmk) {
        landmark_matrices(F, N.lm_size);
        d_lmk = (float*)C.arena.alloc((size_t)m * 212 * sizeof(float));
        run_face_crops_mixed(ctx, N.lmk, d_desc, m, F.img.data(), F.Ml.data(), N.lm_size, N.lm_mean, N.lm_scale, 1 ^ rgb, d_lmk, 212, nullptr, inv_l);
        h_lmk.resize((size_t)m * 212);
        FE_HIP(hipMemcpyAsync(h_lmk.data(), d_lmk, h_lmk.size() * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      }
      if (m > 0 && N.rec && L.K == 5) {
        recognition_matrices(F, N.rc_size);
        d_emb = (float*)C.arena.alloc((size_t)m * 512 * sizeof(float));
        run_face_crops_mixed(ctx, N.rec, d_desc, m, F.img.data(), F.Mr.data(), N.rc_size, N.rc_mean, N.rc_scale, 1 ^ rgb, d_emb, 512, nullptr, inv_r);
        h_emb.resize((size_t)m * 512);
        FE_HIP(hipMemcpyAsync(h_emb.data(), d_emb, h_emb.size() * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      }
      FE_HIP(hipStreamSynchronize(C.stream));
      write_face_records(F, nb, max_faces, N.lm_size, d_lmk ? h_lmk.data() : nullptr, d_emb ? h_emb.data() : nullptr,
                         faces + (size_t)i0 * max_faces * FE_FACE_FLOATS);
      i0 = i1;
    }
    return FE_OK;
  });
}

/* fe_roi_laplacian over a list of images of any sizes */
int fe_roi_laplacian_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int m, const int* img_index,
                           const int* rois, double* out) {
  return fe_api(ctx, OnError::Capacity, [&] {
    Ctx& C = ctx->c;
    const char* who = "fe_roi_laplacian_mixed";
    if (!mixed_list_ok(C, who, images, hw, n, order, images, kFaceLimits)) return FE_ERR_INVALID;
    FE_CHECK(m >= 0 && (m == 0 || (img_index && rois && out)), "bad arguments");
    if (m == 0) return FE_OK;
    for (int f = 0; f < m; ++f) {
      FE_CHECK(img_index[f] >= 0 && img_index[f] < n, "roi %d refers to image %d of %d", f, img_index[f], n);
      const int* r = rois + 4 * f;
      const int h = hw[2 * img_index[f]], w = hw[2 * img_index[f] + 1];
      FE_CHECK(r[0] >= 0 && r[1] >= 0 && r[2] <= w && r[3] <= h, "roi %d = [%d,%d,%d,%d] leaves the %dx%d image %d", f, r[0], r[1], r[2], r[3], w, h, img_index[f]);
    }
    C.arena.reset();
    std::vector<ImageDesc> descs;
    const ImageDesc* d_desc = plain_descs(C, who, images, hw, n, on_device, (size_t)m * 64 + 4096, descs);
    int* d_idx = upload(C, img_index, (size_t)m);
    int* d_roi = upload(C, rois, (size_t)m * 4);
    double* d_out = (double*)C.arena.alloc((size_t)m * 4 * sizeof(double));
    launch_roi_laplacian_mixed(d_desc, order == FE_ORDER_RGB, d_idx, d_roi, m, d_out, C.stream);
    FE_HIP(hipMemcpyAsync(out, d_out, (size_t)m * 4 * sizeof(double), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

/* fe_face_thumbnails over a list of images of any sizes */
int fe_face_thumbnails_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int m,
                             const int32_t* img_index, const int32_t* crops, const int32_t* out_sizes, int quality, uint8_t* out, size_t cap,
                             int32_t* lengths) {
  return fe_api(ctx, OnError::Capacity, [&] {
    Ctx& C = ctx->c;
    const char* who = "fe_face_thumbnails_mixed";
    if (!mixed_list_ok(C, who, images, hw, n, order, images, kFaceLimits)) return FE_ERR_INVALID;
    char msg[200] = "";
    if (!(m >= 0 && (m == 0 || (img_index && crops && out_sizes && out && lengths)))) snprintf(msg, sizeof msg, "%s: bad arguments", who);
    else if (quality < 1 || quality > 100) snprintf(msg, sizeof msg, "%s: quality %d (1 .. 100)", who, quality);
    for (int f = 0; f < m && !msg[0]; ++f) {
      const int32_t* r = crops + 4 * f;
      const int32_t ow = out_sizes[2 * f], oh = out_sizes[2 * f + 1];
      if (img_index[f] < 0 || img_index[f] >= n) { snprintf(msg, sizeof msg, "%s: face %d refers to image %d of %d", who, f, img_index[f], n); break; }
      const int h = hw[2 * img_index[f]], w = hw[2 * img_index[f] + 1];
      if (r[0] < 0 || r[1] < 0 || r[2] > w || r[3] > h || r[0] >= r[2] || r[1] >= r[3])
        snprintf(msg, sizeof msg, "%s: crop %d = [%d,%d,%d,%d] is empty or leaves the %dx%d image %d", who, f, r[0], r[1], r[2], r[3], w, h, img_index[f]);
      else if (ow < 1 || oh < 1 || ow > FE_FACE_THUMB_MAX_SIDE || oh > FE_FACE_THUMB_MAX_SIDE)
        snprintf(msg, sizeof msg, "%s: output size %d x %d of face %d (1 .. %d)", who, ow, oh, f, FE_FACE_THUMB_MAX_SIDE);
    }
    if (msg[0]) { C.err = msg; return FE_ERR_INVALID; }
    if (m == 0) return FE_OK;
    C.arena.reset();
    std::vector<ImageDesc> descs;
    const ImageDesc* d_desc = plain_descs(C, who, images, hw, n, on_device, C.arena.capacity() / 8, descs);
    if (!face_thumbnails_mixed(C, d_desc, order == FE_ORDER_RGB, m, img_index, crops, out_sizes, quality, out, cap, lengths)) {
      char b[200];
      snprintf(b, sizeof(b), "%s: a face needs more than the %zu bytes of its output row (fe_jpeg_bound(max oh, max ow) always fits)", who, cap);
      throw CapacityError(b);
    }
    return FE_OK;
  });
}

}  // extern "C"
