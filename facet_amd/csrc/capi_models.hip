// C ABI: the scoring models - TOPIQ, U2-Net-P + SAMP-Net, CLIP image and text, the aesthetic head, tag similarities, the ensemble.
#include "capi_internal.h"
#include "ensemble_plan.h"
#include "resize_mixed_core.h"

namespace {
const float kImagenetMean[3] = {0.485f, 0.456f, 0.406f};
const float kImagenetStd[3] = {0.229f, 0.224f, 0.225f};
const float kClipMean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
const float kClipStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};

int py_round_half_even(double v) {
  const double f = std::floor(v);
  const double d = v - f;
  if (d > 0.5) return (int)f + 1;
  if (d < 0.5) return (int)f;
  return ((long long)f % 2 == 0) ? (int)f : (int)f + 1;
}

// Runs the backbone on images [i0, i0+nb) of a device-resident u8 batch.
// Long edge > 1024 is first reduced with PIL-exact LANCZOS to (int(w*s), int(h*s)), s = 1024/long_edge, exactly as
// PyIQAScorer._preprocess_image does on the host (reference models/pyiqa_scorer.py:131-153).
template <class T>
void topiq_backbone_chunk(fe_ctx* ctx, const uint8_t* d_rgb, int nb, int h, int w, std::vector<TensorT<T>>& feats) {
  Ctx& C = ctx->c;
  const int long_edge = h > w ? h : w;
  if (long_edge > 1024) {
    const double sc = 1024.0 / long_edge;
    const int nw = (int)(w * sc), nh = (int)(h * sc);
    uint8_t* small = (uint8_t*)C.arena.alloc((size_t)nb * nh * nw * 3);
    resize_u8(C, d_rgb, nb, h, w, nh, nw, FE_FILTER_LANCZOS, 0, nh, 0, nw, small);
    d_rgb = small; h = nh; w = nw;
  }
  Tensor x = C.arena.tensor(nb, h, w, 4);
  launch_u8_to_nhwc4_norm(d_rgb, x.p, (size_t)nb * h * w, kImagenetMean, kImagenetStd, 0, C.stream);
  resnet_forward<T>(C, ctx->c.topiq->backbone, x, &feats, ctx->c.topiq->dw.res32);      // RES32: fp32 skip stream in the backbone
}
// backbone + head of one micro-batch in the precision the model was committed under; scores are fp32 either way
// fe_topiq_f32_below: images with fewer pixels run on the model's fp32 weights even when it was committed under a 2-byte precision.
// With a few dozen tokens per pyramid level the rounding noise of a 2-byte pass is not averaged down (fp16 TOPIQ on 33 x 500 and
// 97 x 131 inputs: 4e-4 .. 1.2e-3 from the oracle, against <= 6e-4 from 512 x 512 up, tests/test_precision_policy_gpu.py), and such an
// image costs under a sixteenth of a 1024 x 1024 one. The PARITY policy (facet_amd/precision.py) sets 256 x 256; the default is 0.
// (Every 2-byte model keeps its fp32 weights: pack_conv only drops them for half_only models, which TOPIQ is not.)
void topiq_chunk_score(fe_ctx* ctx, const uint8_t* d_in, int nb, int h, int w, float* d_scores) {
  Ctx& C = ctx->c;
  const bool small = (size_t)h * (size_t)w < C.topiq_f32_below && !C.topiq->dw.half_only && !C.topiq->dw.res32;
  if (C.topiq->dw.prec != PREC_F32 && small) {
    std::vector<Tensor> feats;
    topiq_backbone_chunk<float>(ctx, d_in, nb, h, w, feats);
    topiq_head_forward<float>(C, *C.topiq, feats, d_scores);
  } else if (C.topiq->dw.prec == PREC_BF16) {
    std::vector<TensorH> feats;
    topiq_backbone_chunk<bf16>(ctx, d_in, nb, h, w, feats);
    topiq_head_forward<bf16>(C, *C.topiq, feats, d_scores);
  } else if (C.topiq->dw.prec == PREC_F16) {
    std::vector<TensorF16> feats;
    topiq_backbone_chunk<f16>(ctx, d_in, nb, h, w, feats);
    topiq_head_forward<f16>(C, *C.topiq, feats, d_scores);
  } else {
    std::vector<Tensor> feats;
    topiq_backbone_chunk<float>(ctx, d_in, nb, h, w, feats);
    topiq_head_forward<float>(C, *C.topiq, feats, d_scores);
  }
}

// uint8 images -> the model's normalised NHWC4 input, preprocessing exactly like the reference's PIL/torchvision path
Tensor preprocess_square224(Ctx& C, const uint8_t* d_rgb, int nb, int h, int w, int filter, bool shorter_side_crop,
                            const float mean[3], const float stdv[3], int bgr) {
  int oh = 224, ow = 224, y0 = 0, x0 = 0;
  if (shorter_side_crop) {  // torchvision Resize(224) + CenterCrop(224)
    if (w <= h) { ow = 224; oh = (int)(224.0 * h / w); } else { oh = 224; ow = (int)(224.0 * w / h); }
    y0 = py_round_half_even((oh - 224) / 2.0);
    x0 = py_round_half_even((ow - 224) / 2.0);
  }
  uint8_t* small = (uint8_t*)C.arena.alloc((size_t)nb * 224 * 224 * 3);
  resize_u8(C, d_rgb, nb, h, w, oh, ow, filter, y0, 224, x0, 224, small);
  Tensor x = C.arena.tensor(nb, 224, 224, 4);
  launch_u8_to_nhwc4_norm(small, x.p, (size_t)nb * 224 * 224, mean, stdv, bgr, C.stream);
  return x;
}

// saliency (and optionally the SAMP-Net scores) of one chunk of normalised fp32 NHWC4 crops, in the precision the models were
// committed under. d_sal (nullable): fp32 device [n][h][w] copy of the saliency map.
void samp_chunk(fe_ctx* ctx, const Tensor& x, bool with_samp, float* pw, float* at, float* sd, float* d_sal) {
  Ctx& C = ctx->c;
  // the two networks may be committed under different precisions (the saliency map crosses in U2-Net-P's type)
  auto samp_on = [&](auto sal) {
    typedef decltype(sal.p) SP;
    typedef std::remove_pointer_t<SP> TS;
    if (!with_samp) return;
    if (C.samp->dw.prec == PREC_BF16) sampnet_forward<bf16, TS>(C, *C.samp, x, sal, pw, at, sd);
    else if (C.samp->dw.prec == PREC_F16) sampnet_forward<f16, TS>(C, *C.samp, x, sal, pw, at, sd);
    else sampnet_forward<float, TS>(C, *C.samp, x, sal, pw, at, sd);
  };
  const int prec = C.u2netp->dw.prec;
  if (prec == PREC_BF16) {
    TensorH sal = C.arena.tensor_t<bf16>(x.n, x.h, x.w, 1);
    u2netp_forward<bf16>(C, *C.u2netp, x, sal);
    samp_on(sal);
    if (d_sal) launch_convert(sal.p, d_sal, sal.numel(), C.stream);
  } else if (prec == PREC_F16) {
    TensorF16 sal = C.arena.tensor_t<f16>(x.n, x.h, x.w, 1);
    u2netp_forward<f16>(C, *C.u2netp, x, sal);
    samp_on(sal);
    if (d_sal) launch_convert(sal.p, d_sal, sal.numel(), C.stream);
  } else {
    Tensor sal = C.arena.tensor(x.n, x.h, x.w, 1);
    u2netp_forward<float>(C, *C.u2netp, x, sal);
    samp_on(sal);
    if (d_sal) FE_HIP(hipMemcpyAsync(d_sal, sal.p, sal.numel() * sizeof(float), hipMemcpyDeviceToDevice, C.stream));
  }
}

// x: fp32 NCHW [n,3,224,224] as open_clip's eval transform yields (host, or device when on_device).
// features [n,768] un-normalised (= model.encode_image); emb_norm (nullable) = F.normalize(features);
// aesthetic_raw (nullable, needs FE_MODEL_AESTHETIC) = aesthetic_head(features) before the (x+1)*5 clamp.
// The ViT tower wants more images per launch than the 1024^2 models can hold in flight: its GEMMs have rows = images x 257
// tokens in 128-row tiles x (width / 128) column tiles over 256 CUs, and a partially filled last round of workgroups costs up
// to a third of a launch. tools/clip_mb_sweep.py: 621 img/s at 32 images per launch, ~700 at 95-127. So crops (602 KB each)
// are collected across micro-batches and the tower runs on `chunk` of them, chunk chosen for full rounds.
// Moves the `left` crops behind the `c` just consumed to the front of a batcher buffer. left can exceed c (micro-batch larger than
// the tower chunk), where one copy would have overlapping source and destination ranges: the move is cut into pieces of at most c
// crops, each with disjoint ranges, issued in ascending order on the one stream.
void compact_crops(float* buf, size_t per, int c, int left, hipStream_t s) {
  for (int done = 0; done < left; done += c) {
    const int n = std::min(c, left - done);
    FE_HIP(hipMemcpyAsync(buf + (size_t)done * per, buf + (size_t)(c + done) * per, (size_t)n * per * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
}
void clip_tower(Ctx& C, const Tensor& x, float* feat) {   // in the precision the tower was committed under
  const bool r32 = C.clip->dw.res32;      // fp32 token stream around the 2-byte GEMMs
  if (C.clip->split3) { clip_forward_split3(C, *C.clip, x, feat); return; }
  if (C.clip->dw.prec == PREC_BF16) { if (r32) clip_forward<bf16, float>(C, *C.clip, x, feat); else clip_forward<bf16>(C, *C.clip, x, feat); }
  else if (C.clip->dw.prec == PREC_F16) { if (r32) clip_forward<f16, float>(C, *C.clip, x, feat); else clip_forward<f16>(C, *C.clip, x, feat); }
  else clip_forward<float>(C, *C.clip, x, feat);
}
// Both batchers enqueue on ctx->c.stream and take scratch from ctx->c.arena as they find them at the call (the main pair, or the side
// lane's under a LaneScope). stage / run / compact are the three steps; push / finish sequence them for the single-model entry points,
// ensemble_run follows its plan (ensemble_plan.h), which sequences them the same way.
class ClipBatcher {
 public:
  ClipBatcher(fe_ctx* ctx, int n_total, int max_push, float* d_feat, float* d_norm, float* d_aes)
      : x_(ctx), feat_(d_feat), norm_(d_norm), aes_(d_aes) {
    const ClipModel& m = *ctx->c.clip;
    hw_ = m.patch_size * (int)std::lround(std::sqrt((double)(m.tokens - 1)));
    od_ = m.out_dim;
    per_ = (size_t)hw_ * hw_ * 4;
    chunk_ = clip_tower_chunk(m.width, m.tokens, n_total);
    const size_t need = (size_t)(chunk_ + max_push) * per_;
    if (ctx->clip_in_cap < need) {
      FE_HIP(hipStreamSynchronize(ctx->c.stream));
      if (ctx->clip_in) FE_HIP(hipFree(ctx->clip_in));
      ctx->clip_in = nullptr; ctx->clip_in_cap = 0;
      FE_HIP(hipMalloc((void**)&ctx->clip_in, need * sizeof(float)));
      ctx->clip_in_cap = need;
    }
  }
  int chunk() const { return chunk_; }
  // xt: dense NHWC4 crops of one micro-batch (arena memory; copied out before the arena is recycled) -> slots [slot, slot + xt.n)
  void stage(const Tensor& xt, int slot) {
    FE_CHECK(xt.c == 4 && xt.ld == 4 && xt.h == hw_ && xt.w == hw_, "clip batcher: crop layout");
    FE_CHECK((size_t)(slot + xt.n) * per_ <= x_->clip_in_cap, "clip batcher: slot %d + %d past the staging buffer", slot, xt.n);
    FE_HIP(hipMemcpyAsync(x_->clip_in + (size_t)slot * per_, xt.p, (size_t)xt.n * per_ * sizeof(float), hipMemcpyDeviceToDevice, x_->c.stream));
  }
  // tower, L2 normalise and aesthetic head on slots [0, c): the results of images [done, done + c)
  void run(int c, int done) {
    Ctx& C = x_->c;
    const size_t mark = C.arena.mark();
    Tensor x;
    x.p = x_->clip_in; x.n = c; x.h = hw_; x.w = hw_; x.c = 4; x.ld = 4;
    clip_tower(C, x, feat_ + (size_t)done * od_);
    if (norm_) l2_normalize(C, feat_ + (size_t)done * od_, norm_ + (size_t)done * od_, c, od_);
    if (aes_) aesthetic_forward(C, *C.aesthetic, feat_ + (size_t)done * od_, c, aes_ + done);
    C.arena.rewind(mark);
  }
  void compact(int c, int left) { compact_crops(x_->clip_in, per_, c, left, x_->c.stream); }
  // slots [slot, slot + count) themselves, for a producer that writes the normalised crops in place (the mixed-size preprocessing)
  float* slots(int slot, int count) {
    FE_CHECK(hw_ == 224, "clip batcher: in-place crops are 224 x 224");
    FE_CHECK(slot >= 0 && count > 0 && (size_t)(slot + count) * per_ <= x_->clip_in_cap, "clip batcher: slot %d + %d past the staging buffer", slot, count);
    return x_->clip_in + (size_t)slot * per_;
  }
  void push(const Tensor& xt) {
    stage(xt, count_);
    count_ += xt.n;
    while (count_ >= chunk_) consume(chunk_);
  }
  void finish() {
    while (count_ > 0) consume(std::min(count_, chunk_));
  }
 private:
  void consume(int c) {
    run(c, done_);
    compact(c, count_ - c);
    done_ += c;
    count_ -= c;
  }
  fe_ctx* x_;
  float *feat_, *norm_, *aes_;
  int hw_ = 224, od_ = 768, chunk_ = 1, count_ = 0, done_ = 0;
  size_t per_ = 0;
};
// SAMP-Net + U2-Net-P see 224^2 crops too, and most of their ~130 convolutions run on 7x7 .. 56x56 maps: at 32 images per launch
// they are launch- and tile-quantisation-bound (tools/samp_mb_sweep.py: 2216 img/s at 32 per launch, 2903 at 128). Crops are
// collected across micro-batches like the CLIP ones; the chunk is bounded by what the arena can hold (~150 MB per image).
// The chunk is sized from the arena of the Ctx at construction: construct it outside any LaneScope, so the policy follows the main arena.
constexpr size_t kSampBytesPerImage = (size_t)150 << 20;
class SampBatcher {
 public:
  SampBatcher(fe_ctx* ctx, int n_total, int max_push, float* pw, float* at, float* sd) : x_(ctx), pw_(pw), at_(at), sd_(sd) {
    const size_t room = ctx->c.arena.capacity() > ((size_t)8 << 30) ? ctx->c.arena.capacity() - ((size_t)8 << 30) : ctx->c.arena.capacity() / 4;
    const int fit = (int)std::min<size_t>(128, std::max<size_t>(1, room / kSampBytesPerImage));
    chunk_ = std::max(1, std::min(n_total, std::max(fit, std::min(max_push, 32))));
    per_ = (size_t)224 * 224 * 4;
    const size_t need = (size_t)(chunk_ + max_push) * per_;
    if (ctx->samp_in_cap < need) {
      FE_HIP(hipStreamSynchronize(ctx->c.stream));
      if (ctx->samp_in) FE_HIP(hipFree(ctx->samp_in));
      ctx->samp_in = nullptr; ctx->samp_in_cap = 0;
      FE_HIP(hipMalloc((void**)&ctx->samp_in, need * sizeof(float)));
      ctx->samp_in_cap = need;
    }
  }
  int chunk() const { return chunk_; }
  void stage(const Tensor& xt, int slot) {
    FE_CHECK(xt.c == 4 && xt.ld == 4 && xt.h == 224 && xt.w == 224, "samp batcher: crop layout");
    FE_CHECK((size_t)(slot + xt.n) * per_ <= x_->samp_in_cap, "samp batcher: slot %d + %d past the staging buffer", slot, xt.n);
    FE_HIP(hipMemcpyAsync(x_->samp_in + (size_t)slot * per_, xt.p, (size_t)xt.n * per_ * sizeof(float), hipMemcpyDeviceToDevice, x_->c.stream));
  }
  void run(int c, int done) {
    Ctx& C = x_->c;
    const size_t mark = C.arena.mark();
    Tensor x;
    x.p = x_->samp_in; x.n = c; x.h = 224; x.w = 224; x.c = 4; x.ld = 4;
    samp_chunk(x_, x, true, pw_ + (size_t)done * 8, at_ + (size_t)done * 6, sd_ + (size_t)done * 5, nullptr);
    C.arena.rewind(mark);
  }
  void compact(int c, int left) { compact_crops(x_->samp_in, per_, c, left, x_->c.stream); }
  float* slots(int slot, int count) {
    FE_CHECK(slot >= 0 && count > 0 && (size_t)(slot + count) * per_ <= x_->samp_in_cap, "samp batcher: slot %d + %d past the staging buffer", slot, count);
    return x_->samp_in + (size_t)slot * per_;
  }
  void push(const Tensor& xt) {
    stage(xt, count_);
    count_ += xt.n;
    while (count_ >= chunk_) consume(chunk_);
  }
  void finish() {
    while (count_ > 0) consume(std::min(count_, chunk_));
  }
 private:
  void consume(int c) {
    run(c, done_);
    compact(c, count_ - c);
    done_ += c;
    count_ -= c;
  }
  fe_ctx* x_;
  float *pw_, *at_, *sd_;
  int chunk_ = 1, count_ = 0, done_ = 0;
  size_t per_ = 0;
};

// SoA result planes (what the model heads write) -> [n][ld] records, one thread per record float.
__global__ void records_interleave_kernel(const float* __restrict__ planes, size_t n4, int n, float* __restrict__ rec, int ld) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n * FE_RECORD_FLOATS) return;
  const int img = (int)(i / FE_RECORD_FLOATS), f = (int)(i - (size_t)img * FE_RECORD_FLOATS);
  const size_t o_aes = n4, o_pw = 2 * n4, o_at = o_pw + 8 * n4, o_sd = o_at + 6 * n4, o_emb = o_sd + 5 * n4;
  float v;
  if (f == 0) v = planes[img];
  else if (f == 1) v = planes[o_aes + img];
  else if (f < 10) v = planes[o_pw + (size_t)img * 8 + (f - 2)];
  else if (f < 16) v = planes[o_at + (size_t)img * 6 + (f - 10)];
  else if (f < 21) v = planes[o_sd + (size_t)img * 5 + (f - 16)];
  else v = planes[o_emb + (size_t)img * 768 + (f - 21)];
  rec[(size_t)img * ld + f] = v;
}

// The side lane's stream, events and an arena of at least `need` bytes. false: something could not be had (device memory, most
// likely) and the call runs on the one lane; that is no error.
bool side_lane_ready(fe_ctx* ctx, size_t need) {
  auto& s = ctx->side;
  try {
    if (!s.stream) FE_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&s.ev_start, &s.ev_join, &s.ev_read[0], &s.ev_read[1]})
      if (!*e) FE_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    if (s.arena.capacity() < need) {
      FE_HIP(hipStreamSynchronize(s.stream));
      s.arena.init(need);
    }
    return true;
  } catch (const std::exception&) {
    (void)hipGetLastError();
    return false;
  }
}
// Scratch of the side lane: the larger of its two models on a chunk (each step resets the arena, and they alternate on the one stream)
// plus the 224^2 preprocessing of a micro-batch. CLIP: ~13 token-stream-sized buffers of 257 x 1024 x 4 B per image in either
// precision, taken as 32 MB. Never more than the main arena, in which the one-lane path runs the same steps.
size_t side_arena_bytes(fe_ctx* ctx, int mb, int h, int w, int clip_chunk, int samp_chunk) {
  const size_t tower = std::max((size_t)clip_chunk * ((size_t)32 << 20), (size_t)samp_chunk * kSampBytesPerImage);
  const size_t ow = w <= h ? 224 : (size_t)(224.0 * w / h) + 1;
  const size_t pre = (size_t)mb * ((size_t)h * ow * 3 + (size_t)224 * 224 * (3 + 16) + 1024);
  return std::min(ctx->c.arena.capacity(), tower + pre + ((size_t)64 << 20));
}

// Runs every selected model over the batch and leaves the interleaved records in device memory d_rec [n][ld].
// With a 224^2 model selected the call runs on two lanes: TOPIQ on the context's stream and arena, SAMP (and a 2-byte CLIP tower) on
// the side lane beside it (ensemble_plan.h has the schedule and its edges; DESIGN.md section 5 the reasons). One lane when
// per-launch profiling is on (event pairs with a sync mean nothing across lanes), when the side arena could not be allocated, and
// when FE_NO_OVERLAP is in the environment (A/B hook, read per call). Both ways every launch has the same arguments.
int ensemble_run(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* d_rec, int ld) {
  using namespace fe::plan;
  Ctx& C = ctx->c;
  const size_t per = (size_t)h * w * 3;
  // SoA planes on the device (every plane 16-B aligned), interleaved into records by a last small kernel
  const size_t n4 = ((size_t)n + 3) & ~(size_t)3;
  const size_t o_aes = n4, o_pw = 2 * n4, o_at = o_pw + 8 * n4, o_sd = o_at + 6 * n4, o_emb = o_sd + 5 * n4,
               o_feat = o_emb + 768 * n4, total = o_feat + 768 * n4;
  float* d_pl = ctx->out_buf(total);
  const int sel = ctx->ensemble_mask;
  const bool do_topiq = (sel & 1) && C.topiq && C.topiq->has_head, do_clip = (sel & 2) && C.clip, do_samp = (sel & 4) && C.samp && C.u2netp;
  float* p_topiq = d_pl;  float* p_aes = d_pl + o_aes;  float* p_pw = d_pl + o_pw;  float* p_at = d_pl + o_at;
  float* p_sd = d_pl + o_sd;  float* p_emb = d_pl + o_emb;  float* d_feat = d_pl + o_feat;
  std::unique_ptr<ClipBatcher> tower;
  if (do_clip) tower = std::make_unique<ClipBatcher>(ctx, n, ctx->microbatch, d_feat, p_emb, C.aesthetic ? p_aes : nullptr);
  std::unique_ptr<SampBatcher> samp;
  if (do_samp) samp = std::make_unique<SampBatcher>(ctx, n, ctx->microbatch, p_pw, p_at, p_sd);
  if (!on_device) ImageStager::prepare(ctx, (size_t)std::min(ctx->microbatch, n) * per);

  Shape sh;
  sh.n = n; sh.mb = ctx->microbatch; sh.on_device = on_device != 0;
  sh.topiq = do_topiq; sh.clip = do_clip; sh.samp = do_samp;
  sh.clip_chunk = tower ? tower->chunk() : 1;
  sh.samp_chunk = samp ? samp->chunk() : 1;
  // An fp32 CLIP tower stays on the main lane: its GEMMs and TOPIQ's want the same matrix pipes, and beside TOPIQ it measured 0 to -0.2 %
  // (profiles/overlap_perf.txt: topiq_clip, and CLIP alone on the side lane of the full workload). A 2-byte tower rides the side lane with
  // SAMP: under the parity and bf16 policies the pairing is worth 5 %. Keyed on the precision the model was committed under.
  sh.clip_side = do_clip && C.clip->dw.prec != PREC_F32;
  if (const char* v = getenv("FE_OVERLAP_LANES")) {   // A/B hook, read per call: "clip" / "samp" = only that model on the side lane; "both"; "samp_first"
    sh.samp_side = strcmp(v, "clip") != 0;
    sh.clip_side = strcmp(v, "samp") != 0;
    sh.samp_first = strcmp(v, "samp_first") == 0;
  }
  const bool side_clip = do_clip && sh.clip_side, side_samp = do_samp && sh.samp_side;
  sh.overlap = (side_clip || side_samp) && !C.profile && getenv("FE_NO_OVERLAP") == nullptr &&
               side_lane_ready(ctx, side_arena_bytes(ctx, std::min(ctx->microbatch, n), h, w, side_clip ? sh.clip_chunk : 0, side_samp ? sh.samp_chunk : 0));

  // the streams and events by the plan's names, read before any LaneScope swaps the Ctx's members
  const hipStream_t lane[N_LANES] = {C.stream, ctx->side.stream, ctx->copy_stream};
  hipEvent_t event[N_EVENTS];
  event[EV_START] = ctx->side.ev_start; event[EV_JOIN] = ctx->side.ev_join;
  for (int b = 0; b < 2; ++b) {
    event[EV_COPIED0 + b] = ctx->ev_copied[b]; event[EV_CONSUMED0 + b] = ctx->ev_consumed[b]; event[EV_SIDE_READ0 + b] = ctx->side.ev_read[b];
  }
  auto input = [&](int k) { return on_device ? rgb + (size_t)k * ctx->microbatch * per : (const uint8_t*)ctx->stage_buf[k & 1]; };
  for (const Op& o : build(sh)) {
    LaneScope scope(ctx, o.lane == LANE_SIDE);
    switch (o.kind) {
      case OP_CLEAR:
        FE_HIP(hipMemsetAsync(d_pl, 0, total * sizeof(float), lane[LANE_MAIN]));
        break;
      case OP_COPY_IN:
        FE_HIP(hipMemcpyAsync(ctx->stage_buf[o.mb & 1], rgb + (size_t)o.img0 * per, (size_t)o.count * per, hipMemcpyHostToDevice, lane[LANE_COPY]));
        break;
      case OP_RECORD:
        FE_HIP(hipEventRecord(event[o.event], lane[o.lane]));
        break;
      case OP_WAIT:
        FE_HIP(hipStreamWaitEvent(lane[o.lane], event[o.event], 0));
        break;
      case OP_TOPIQ:
        C.arena.reset();
        topiq_chunk_score(ctx, input(o.mb), o.count, h, w, p_topiq + o.img0);
        break;
      case OP_CLIP_PRE:
        C.arena.reset();
        tower->stage(preprocess_square224(C, input(o.mb), o.count, h, w, FE_FILTER_BICUBIC, true, kClipMean, kClipStd, 0), o.slot);
        break;
      case OP_CLIP_TOWER:   // the ViT tower runs once enough crops have gathered for full rounds of workgroups
        C.arena.reset();
        tower->run(o.count, o.img0);
        break;
      case OP_CLIP_COMPACT:
        tower->compact(o.count, o.left);
        break;
      case OP_SAMP_PRE:
        C.arena.reset();
        samp->stage(preprocess_square224(C, input(o.mb), o.count, h, w, FE_FILTER_BILINEAR, false, kImagenetMean, kImagenetStd, 0), o.slot);
        break;
      case OP_SAMP_NETS:    // U2-Net-P + SAMP-Net run once enough crops have gathered
        C.arena.reset();
        samp->run(o.count, o.img0);
        break;
      case OP_SAMP_COMPACT:
        samp->compact(o.count, o.left);
        break;
      case OP_INTERLEAVE: {
        const size_t work = (size_t)n * FE_RECORD_FLOATS;
        hipLaunchKernelGGL(records_interleave_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, lane[LANE_MAIN], d_pl, n4, n, d_rec, ld);
        FE_HIP(hipGetLastError());
        break;
      }
    }
  }
  return (do_topiq ? 1 : 0) | (do_clip ? 2 : 0) | (do_samp ? 4 : 0);
}

// ---- images of mixed sizes --------------------------------------------------------------------------------------------------------
// records_interleave_kernel for a mixed call: the planes are in position order, pos [n] = position of input image i.
__global__ void records_interleave_mixed_kernel(const float* __restrict__ planes, size_t n4, int n, const int32_t* __restrict__ pos,
                                                float* __restrict__ rec, int ld) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n * FE_RECORD_FLOATS) return;
  const int img = (int)(i / FE_RECORD_FLOATS), f = (int)(i - (size_t)img * FE_RECORD_FLOATS);
  const size_t p = (size_t)pos[img];
  const size_t o_aes = n4, o_pw = 2 * n4, o_at = o_pw + 8 * n4, o_sd = o_at + 6 * n4, o_emb = o_sd + 5 * n4;
  float v;
  if (f == 0) v = planes[p];
  else if (f == 1) v = planes[o_aes + p];
  else if (f < 10) v = planes[o_pw + p * 8 + (f - 2)];
  else if (f < 16) v = planes[o_at + p * 6 + (f - 10)];
  else if (f < 21) v = planes[o_sd + p * 5 + (f - 16)];
  else v = planes[o_emb + p * 768 + (f - 21)];
  rec[(size_t)img * ld + f] = v;
}

// Puts the scoped resize tables into the Ctx for the lifetime of a mixed call
struct ScopedTables {
  Ctx& c;
  ScopedTables(Ctx& ctx, const std::map<std::tuple<int, int, int>, ResizeCoeffsDev>* t) : c(ctx) { c.resize_scoped = t; }
  ~ScopedTables() { c.resize_scoped = nullptr; }
};

// what the mixed entry points here accept of an image, from a shortest side on: at most 2^28 pixels
constexpr MixedLimits mixed_limits(int min_side) { return {min_side, INT32_MAX, INT32_MAX, (size_t)1 << 28, "at most 2^28"}; }

// ensemble_run for images of mixed sizes: the same plan over cut_mixed's micro-batches (ensemble_plan.h), the 224^2 crops from the
// descriptor-driven kernels (resize_mixed_core.h) straight into the batchers' slots. Descriptors, the table pool (LANCZOS tables of
// TOPIQ's > 1024 cap included) and the position map go up once, into ctx->mixed_buf: nothing is allocated or cached per image size.
int ensemble_run_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, float* d_rec, int ld) {
  using namespace fe::plan;
  Ctx& C = ctx->c;
  const size_t n4 = ((size_t)n + 3) & ~(size_t)3;
  const size_t o_aes = n4, o_pw = 2 * n4, o_at = o_pw + 8 * n4, o_sd = o_at + 6 * n4, o_emb = o_sd + 5 * n4,
               o_feat = o_emb + 768 * n4, total = o_feat + 768 * n4;
  float* d_pl = ctx->out_buf(total);
  const int sel = ctx->ensemble_mask;
  const bool do_topiq = (sel & 1) && C.topiq && C.topiq->has_head, do_clip = (sel & 2) && C.clip, do_samp = (sel & 4) && C.samp && C.u2netp;
  float* p_topiq = d_pl;  float* p_aes = d_pl + o_aes;  float* p_pw = d_pl + o_pw;  float* p_at = d_pl + o_at;
  float* p_sd = d_pl + o_sd;  float* p_emb = d_pl + o_emb;  float* d_feat = d_pl + o_feat;
  std::unique_ptr<ClipBatcher> tower;
  if (do_clip) tower = std::make_unique<ClipBatcher>(ctx, n, ctx->microbatch, d_feat, p_emb, C.aesthetic ? p_aes : nullptr);
  std::unique_ptr<SampBatcher> samp;
  if (do_samp) samp = std::make_unique<SampBatcher>(ctx, n, ctx->microbatch, p_pw, p_at, p_sd);

  // the cuts: positions, micro-batches, and where every image lies inside its micro-batch
  std::vector<uintptr_t> addr(n);
  for (int i = 0; i < n; ++i) addr[i] = (uintptr_t)images[i];
  const MixedCuts mc = cut_mixed(hw, n, ctx->microbatch, do_topiq, on_device ? addr.data() : nullptr);
  const int chunks = (int)mc.cuts.size();
  std::vector<int> first(chunks + 1, 0), cut_of(n);
  std::vector<size_t> off(n), bytes(n);
  size_t stage_need = 0;
  for (int k = 0; k < chunks; ++k) {
    first[k + 1] = first[k] + mc.cuts[k].count;
    size_t run = 0;
    for (int p = first[k]; p < first[k + 1]; ++p) {
      const int i = mc.order[p];
      cut_of[p] = k; off[p] = run; bytes[p] = (size_t)hw[2 * i] * hw[2 * i + 1] * 3;
      run += bytes[p];
    }
    if (!on_device || mc.cuts[k].gather) stage_need = std::max(stage_need, run);
  }
  if (stage_need) ImageStager::prepare(ctx, stage_need);

  // descriptors per mode in position order, the pool, TOPIQ's LANCZOS tables, the position map: one blob
  MixedTables tables;
  std::vector<MixedDesc> desc[2];
  std::vector<size_t> inter_need[2];
  std::vector<int> max_nr[2];
  const bool mode_on[2] = {do_clip, do_samp};
  size_t max_inter = 0;
  for (int m = 0; m < 2; ++m) {
    if (!mode_on[m]) continue;
    desc[m].resize(n); inter_need[m].assign(chunks, 0); max_nr[m].assign(chunks, 0);
    for (int p = 0; p < n; ++p) {
      const int i = mc.order[p], k = cut_of[p];
      MixedDesc& d = desc[m][p];
      FE_CHECK(tables.describe(m, hw[2 * i], hw[2 * i + 1], d), "ensemble_score_mixed: image %d (%d x %d) cannot be resampled to 224 x 224", i, hw[2 * i], hw[2 * i + 1]);
      d.src = on_device ? images[i] : (const uint8_t*)ctx->stage_buf[k & 1] + off[p];
      d.slot = p - first[k];
      FE_CHECK(inter_need[m][k] + MixedTables::inter_bytes(d) < ((size_t)1 << 32), "ensemble_score_mixed: intermediates of a micro-batch exceed 4 GiB");
      d.inter = (uint32_t)inter_need[m][k];
      inter_need[m][k] += MixedTables::inter_bytes(d);
      if (d.ksize_h) max_nr[m][k] = std::max(max_nr[m][k], (int)d.nr);
      max_inter = std::max(max_inter, inter_need[m][k]);
    }
  }
  struct Lz { std::tuple<int, int, int> key; size_t kk, bounds; int ksize; };
  std::vector<Lz> lz;
  if (do_topiq) {
    std::map<std::tuple<int, int, int>, int> have;
    for (int k = 0; k < chunks; ++k) {
      const int i = mc.order[first[k]], h = hw[2 * i], w = hw[2 * i + 1], long_edge = std::max(h, w);
      if (long_edge <= 1024) continue;
      const double sc = 1024.0 / long_edge;      // topiq_backbone_chunk's arithmetic
      const int nw = (int)(w * sc), nh = (int)(h * sc);
      for (const auto& ax : {std::make_pair(w, nw), std::make_pair(h, nh)}) {
        const auto key = std::make_tuple(ax.first, ax.second, (int)FE_FILTER_LANCZOS);
        if (ax.first == ax.second || ax.second < 1 || !have.emplace(key, 1).second) continue;
        ResizeCoeffs rc;
        build_resize_coeffs(ax.first, ax.second, FE_FILTER_LANCZOS, rc);
        Lz e{key, tables.pool.size(), tables.pool.size() + rc.kk.size(), rc.ksize};
        tables.pool.insert(tables.pool.end(), rc.kk.begin(), rc.kk.end());
        tables.pool.insert(tables.pool.end(), rc.bounds.begin(), rc.bounds.end());
        lz.push_back(e);
      }
    }
  }
  const size_t desc_bytes = (size_t)n * sizeof(MixedDesc), pool_bytes = tables.pool.size() * sizeof(int32_t), pos_bytes = (size_t)n * sizeof(int32_t);
  const size_t o_pool = 2 * desc_bytes, o_pos = o_pool + pool_bytes, blob_bytes = o_pos + pos_bytes;
  std::vector<uint8_t> blob(blob_bytes, 0);
  for (int m = 0; m < 2; ++m)
    if (mode_on[m]) memcpy(blob.data() + m * desc_bytes, desc[m].data(), desc_bytes);
  if (pool_bytes) memcpy(blob.data() + o_pool, tables.pool.data(), pool_bytes);
  {
    int32_t* pos = (int32_t*)(blob.data() + o_pos);
    for (int p = 0; p < n; ++p) pos[mc.order[p]] = p;
  }
  if (ctx->mixed_cap < blob_bytes) {
    fe_drain(ctx);
    if (ctx->mixed_buf) FE_HIP(hipFree(ctx->mixed_buf));
    ctx->mixed_buf = nullptr; ctx->mixed_cap = 0;
    FE_HIP(hipMalloc(&ctx->mixed_buf, blob_bytes + blob_bytes / 2));
    ctx->mixed_cap = blob_bytes + blob_bytes / 2;
  }
  uint8_t* d_blob = (uint8_t*)ctx->mixed_buf;
  FE_HIP(hipMemcpyAsync(d_blob, blob.data(), blob_bytes, hipMemcpyHostToDevice, C.stream));
  FE_HIP(hipStreamSynchronize(C.stream));      // the blob is host memory of this frame; the stream is idle between calls
  const MixedDesc* d_desc[2] = {(const MixedDesc*)d_blob, (const MixedDesc*)(d_blob + desc_bytes)};
  int32_t* d_pool = (int32_t*)(d_blob + o_pool);
  const int32_t* d_pos = (const int32_t*)(d_blob + o_pos);
  std::map<std::tuple<int, int, int>, ResizeCoeffsDev> lanczos;
  for (const Lz& e : lz) {
    ResizeCoeffsDev t;
    t.kk = d_pool + e.kk; t.bounds = d_pool + e.bounds; t.ksize = e.ksize;
    lanczos.emplace(e.key, t);
  }
  ScopedTables scoped(C, &lanczos);

  Shape sh;
  sh.n = n; sh.mb = ctx->microbatch; sh.on_device = on_device != 0;
  sh.topiq = do_topiq; sh.clip = do_clip; sh.samp = do_samp;
  sh.clip_chunk = tower ? tower->chunk() : 1;
  sh.samp_chunk = samp ? samp->chunk() : 1;
  sh.clip_side = do_clip && C.clip->dw.prec != PREC_F32;      // as in ensemble_run
  if (const char* v = getenv("FE_OVERLAP_LANES")) {
    sh.samp_side = strcmp(v, "clip") != 0;
    sh.clip_side = strcmp(v, "samp") != 0;
    sh.samp_first = strcmp(v, "samp_first") == 0;
  }
  const bool side_clip = do_clip && sh.clip_side, side_samp = do_samp && sh.samp_side;
  // side arena: the larger tower chunk plus the intermediates of the largest micro-batch of the call, in steps of 64 MiB so that calls
  // whose sizes differ a little do not each regrow it
  const size_t inter_room = (max_inter + (((size_t)64 << 20) - 1)) & ~(((size_t)64 << 20) - 1);
  const size_t side_need = std::min(C.arena.capacity(), std::max((size_t)(side_clip ? sh.clip_chunk : 0) * ((size_t)32 << 20),
                                                                 (size_t)(side_samp ? sh.samp_chunk : 0) * kSampBytesPerImage) + inter_room + ((size_t)64 << 20));
  sh.overlap = (side_clip || side_samp) && !C.profile && getenv("FE_NO_OVERLAP") == nullptr && side_lane_ready(ctx, side_need);

  const hipStream_t lane[N_LANES] = {C.stream, ctx->side.stream, ctx->copy_stream};
  hipEvent_t event[N_EVENTS];
  event[EV_START] = ctx->side.ev_start; event[EV_JOIN] = ctx->side.ev_join;
  for (int b = 0; b < 2; ++b) {
    event[EV_COPIED0 + b] = ctx->ev_copied[b]; event[EV_CONSUMED0 + b] = ctx->ev_consumed[b]; event[EV_SIDE_READ0 + b] = ctx->side.ev_read[b];
  }
  auto crops = [&](const Op& o, int m, float* out, const float* mean, const float* stdv) {
    uint8_t* scratch = inter_need[m][o.mb] ? (uint8_t*)C.arena.alloc(inter_need[m][o.mb]) : nullptr;
    resize_mixed224(C, d_desc[m] + o.img0, o.count, max_nr[m][o.mb], d_pool, scratch, nullptr, out, mean, stdv);
  };
  for (const Op& o : build(sh, mc.cuts)) {
    LaneScope scope(ctx, o.lane == LANE_SIDE);
    switch (o.kind) {
      case OP_CLEAR:
        FE_HIP(hipMemsetAsync(d_pl, 0, total * sizeof(float), lane[LANE_MAIN]));
        break;
      case OP_COPY_IN:      // image by image: the host images lie anywhere
        for (int p = o.img0; p < o.img0 + o.count; ++p)
          FE_HIP(hipMemcpyAsync(ctx->stage_buf[o.mb & 1] + off[p], images[mc.order[p]], bytes[p], hipMemcpyHostToDevice, lane[LANE_COPY]));
        break;
      case OP_GATHER:
        for (int p = o.img0; p < o.img0 + o.count; ++p)
          FE_HIP(hipMemcpyAsync(ctx->stage_buf[o.mb & 1] + off[p], images[mc.order[p]], bytes[p], hipMemcpyDeviceToDevice, lane[LANE_MAIN]));
        break;
      case OP_RECORD:
        FE_HIP(hipEventRecord(event[o.event], lane[o.lane]));
        break;
      case OP_WAIT:
        FE_HIP(hipStreamWaitEvent(lane[o.lane], event[o.event], 0));
        break;
      case OP_TOPIQ: {
        const int i = mc.order[o.img0];
        const uint8_t* in = (!on_device || mc.cuts[o.mb].gather) ? (const uint8_t*)ctx->stage_buf[o.mb & 1] : images[i];
        C.arena.reset();
        topiq_chunk_score(ctx, in, o.count, hw[2 * i], hw[2 * i + 1], p_topiq + o.img0);
        break;
      }
      case OP_CLIP_PRE:
        C.arena.reset();
        crops(o, MIXED_CLIP, tower->slots(o.slot, o.count), kClipMean, kClipStd);
        break;
      case OP_CLIP_TOWER:
        C.arena.reset();
        tower->run(o.count, o.img0);
        break;
      case OP_CLIP_COMPACT:
        tower->compact(o.count, o.left);
        break;
      case OP_SAMP_PRE:
        C.arena.reset();
        crops(o, MIXED_SAMP, samp->slots(o.slot, o.count), kImagenetMean, kImagenetStd);
        break;
      case OP_SAMP_NETS:
        C.arena.reset();
        samp->run(o.count, o.img0);
        break;
      case OP_SAMP_COMPACT:
        samp->compact(o.count, o.left);
        break;
      case OP_INTERLEAVE: {
        const size_t work = (size_t)n * FE_RECORD_FLOATS;
        hipLaunchKernelGGL(records_interleave_mixed_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, lane[LANE_MAIN], d_pl, n4, n, d_pos, d_rec, ld);
        FE_HIP(hipGetLastError());
        break;
      }
    }
  }
  return (do_topiq ? 1 : 0) | (do_clip ? 2 : 0) | (do_samp ? 4 : 0);
}
}  // namespace

extern "C" {

int fe_topiq_feature_shape(int h, int w, int level, int dims[3]) {
  if (!dims || h < 32 || w < 32 || level < 0 || level > 4) return FE_ERR_INVALID;
  const int long_edge = h > w ? h : w;
  if (long_edge > 1024) {   // the LANCZOS cap of PyIQAScorer._preprocess_image, as topiq_backbone_chunk applies it
    const double sc = 1024.0 / long_edge;
    w = (int)(w * sc); h = (int)(h * sc);
  }
  static const int ch[5] = {64, 256, 512, 1024, 2048};
  int fh = conv_out_dim(h, 7, 2, 3, 1), fw = conv_out_dim(w, 7, 2, 3, 1);              // stem 7x7 / 2
  if (level >= 1) { fh = conv_out_dim(fh, 3, 2, 1, 1); fw = conv_out_dim(fw, 3, 2, 1, 1); }   // max pool 3x3 / 2
  for (int l = 2; l <= level; ++l) { fh = conv_out_dim(fh, 3, 2, 1, 1); fw = conv_out_dim(fw, 3, 2, 1, 1); }   // stride-2 3x3 of layer l
  dims[0] = ch[level]; dims[1] = fh; dims[2] = fw;
  return FE_OK;
}

int fe_topiq_features(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, int level, float* out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.topiq) { C.err = "topiq weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(rgb && out && n > 0 && h >= 32 && w >= 32 && level >= 0 && level <= 4, "bad arguments");
    const size_t img_bytes = (size_t)h * w * 3;
    size_t out_per_img = 0;
    for (int i0 = 0; i0 < n; i0 += ctx->microbatch) {
      const int nb = std::min(ctx->microbatch, n - i0);
      C.arena.reset();
      const uint8_t* d_in = resident(C, rgb + (size_t)i0 * img_bytes, nb * img_bytes, on_device);
      if (C.topiq->dw.prec == PREC_BF16) {
        std::vector<TensorH> feats;
        topiq_backbone_chunk<bf16>(ctx, d_in, nb, h, w, feats);
        const TensorH& f = feats[level];
        out_per_img = (size_t)f.c * f.h * f.w;
        download_nchw(C, f, f.c, out + (size_t)i0 * out_per_img);
      } else if (C.topiq->dw.prec == PREC_F16) {
        std::vector<TensorF16> feats;
        topiq_backbone_chunk<f16>(ctx, d_in, nb, h, w, feats);
        const TensorF16& f = feats[level];
        out_per_img = (size_t)f.c * f.h * f.w;
        download_nchw(C, f, f.c, out + (size_t)i0 * out_per_img);
      } else {
        std::vector<Tensor> feats;
        topiq_backbone_chunk<float>(ctx, d_in, nb, h, w, feats);
        const Tensor& f = feats[level];
        out_per_img = (size_t)f.c * f.h * f.w;
        download_nchw(C, f, f.c, out + (size_t)i0 * out_per_img);
      }
    }
    return FE_OK;
  });
}

int fe_topiq_score(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* scores) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.topiq || !C.topiq->has_head) { C.err = "topiq weights (backbone + head) not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(rgb && scores && n > 0 && h >= 32 && w >= 32, "bad arguments");
    const size_t img_bytes = (size_t)h * w * 3;
    // scores of all micro-batches accumulate in a small device buffer outside the arena; one D2H at the end
    float* d_scores = ctx->out_buf((size_t)n);
    {
      ImageStager st(ctx, rgb, n, img_bytes, ctx->microbatch, on_device);
      for (int k = 0; k < st.chunks(); ++k) {
        const int i0 = k * ctx->microbatch, nb = st.count(k);
        C.arena.reset();
        const uint8_t* d_in = st.get(k);
        topiq_chunk_score(ctx, d_in, nb, h, w, d_scores + i0);
        st.done(k);
      }
      FE_HIP(hipMemcpyAsync(scores, d_scores, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
    }
    return FE_OK;
  });
}

// x: host fp32 NCHW [n,3,h,w], already ImageNet-normalised (what SAMPNetScorer.preprocess yields, samp_net.py:904-928)
int fe_u2netp_saliency(fe_ctx* ctx, const float* x, int n, int h, int w, float* sal_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.u2netp) { C.err = "u2netp weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(x && sal_out && n > 0 && h >= 32 && w >= 32, "bad arguments");
    const size_t per = (size_t)3 * h * w;
    for (int i0 = 0; i0 < n; i0 += ctx->microbatch) {
      const int nb = std::min(ctx->microbatch, n - i0);
      C.arena.reset();
      Tensor xt = upload_nchw(C, x + (size_t)i0 * per, nb, 3, h, w, 4);
      float* d_sal = C.arena.array<float>((size_t)nb * h * w);
      samp_chunk(ctx, xt, false, nullptr, nullptr, nullptr, d_sal);
      FE_HIP(hipMemcpyAsync(sal_out + (size_t)i0 * h * w, d_sal, (size_t)nb * h * w * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
    }
    return FE_OK;
  });
}

// SAMPNetScorer.score_batch's model part (samp_net.py:1005-1010): saliency = U2NETP(x); SAMPNet(x, saliency).
// Outputs (host): pattern_weights [n,8] (logits), attributes [n,6], score_dist [n,5]; sal_out optional [n,224,224].
int fe_samp_forward(fe_ctx* ctx, const float* x, int n, float* pattern_weights, float* attributes, float* score_dist,
                    float* sal_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.u2netp || !C.samp) { C.err = "samp_net / u2netp weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(x && n > 0 && pattern_weights && attributes && score_dist, "bad arguments");
    const int h = 224, w = 224;
    const size_t per = (size_t)3 * h * w;
    float* d_out = ctx->out_buf((size_t)n * 19);
    for (int i0 = 0; i0 < n; i0 += ctx->microbatch) {
      const int nb = std::min(ctx->microbatch, n - i0);
      C.arena.reset();
      Tensor xt = upload_nchw(C, x + (size_t)i0 * per, nb, 3, h, w, 4);
      float* d_sal = sal_out ? C.arena.array<float>((size_t)nb * h * w) : nullptr;
      samp_chunk(ctx, xt, true, d_out + (size_t)i0 * 8, d_out + (size_t)n * 8 + (size_t)i0 * 6, d_out + (size_t)n * 14 + (size_t)i0 * 5, d_sal);
      if (sal_out) FE_HIP(hipMemcpyAsync(sal_out + (size_t)i0 * h * w, d_sal, (size_t)nb * h * w * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
    }
    FE_HIP(hipMemcpyAsync(pattern_weights, d_out, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(attributes, d_out + (size_t)n * 8, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(score_dist, d_out + (size_t)n * 14, (size_t)n * 5 * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

/* aesthetic_head on given feature / embedding vectors (reference Facet.score_from_embedding, processing/scorer.py:619-629) */
int fe_aesthetic_score(fe_ctx* ctx, const float* feats, int n, float* aesthetic_raw) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.aesthetic) { C.err = "aesthetic head weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(feats && aesthetic_raw && n > 0, "bad arguments");
    const int d = 768;
    for (int i0 = 0; i0 < n; i0 += 65536) {
      const int nb = std::min(65536, n - i0);
      C.arena.reset();
      float* d_in = upload(C, feats + (size_t)i0 * d, (size_t)nb * d);
      float* d_out = (float*)C.arena.alloc((size_t)nb * sizeof(float));
      aesthetic_forward(C, *C.aesthetic, d_in, nb, d_out);
      FE_HIP(hipMemcpyAsync(aesthetic_raw + i0, d_out, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
    }
    return FE_OK;
  });
}

int fe_clip_encode_image(fe_ctx* ctx, const float* x, int n, int on_device, float* features, float* emb_norm,
                         float* aesthetic_raw) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.clip) { C.err = "clip weights not loaded"; return FE_ERR_NOT_LOADED; }
    if (aesthetic_raw && !C.aesthetic) { C.err = "aesthetic head weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(x && n > 0 && (features || emb_norm || aesthetic_raw), "bad arguments");
    const int hw = C.clip->patch_size * (int)std::lround(std::sqrt((double)(C.clip->tokens - 1)));
    const int od = C.clip->out_dim;
    const size_t per = (size_t)3 * hw * hw;
    float* d_out = ctx->out_buf((size_t)n * (2 * od + 1));
    float* d_feat = d_out; float* d_norm = d_out + (size_t)n * od; float* d_aes = d_out + (size_t)n * 2 * od;
    const int step = clip_tower_chunk(C.clip->width, C.clip->tokens, n);   // inputs are already 224^2: batch the tower for full rounds of workgroups
    for (int i0 = 0; i0 < n; i0 += step) {
      const int nb = std::min(step, n - i0);
      C.arena.reset();
      Tensor xt;
      if (on_device) {
        xt = C.arena.tensor(nb, hw, hw, 4);
        launch_nchw_to_nhwc(x + (size_t)i0 * per, xt.p, nb, 3, hw, hw, 4, C.stream);
      } else {
        xt = upload_nchw(C, x + (size_t)i0 * per, nb, 3, hw, hw, 4);
      }
      clip_tower(C, xt, d_feat + (size_t)i0 * od);
      if (emb_norm) l2_normalize(C, d_feat + (size_t)i0 * od, d_norm + (size_t)i0 * od, nb, od);
      if (aesthetic_raw) aesthetic_forward(C, *C.aesthetic, d_feat + (size_t)i0 * od, nb, d_aes + i0);
    }
    if (features) FE_HIP(hipMemcpyAsync(features, d_feat, (size_t)n * od * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    if (emb_norm) FE_HIP(hipMemcpyAsync(emb_norm, d_norm, (size_t)n * od * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    if (aesthetic_raw) FE_HIP(hipMemcpyAsync(aesthetic_raw, d_aes, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

// CLIP from raw images: open_clip eval transform (bicubic shorter-side 224, center crop, CLIP mean/std) + tower.
int fe_clip_encode_images(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* features,
                          float* emb_norm, float* aesthetic_raw) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.clip) { C.err = "clip weights not loaded"; return FE_ERR_NOT_LOADED; }
    if (aesthetic_raw && !C.aesthetic) { C.err = "aesthetic head weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(rgb && n > 0 && h > 0 && w > 0, "bad arguments");
    const int od = C.clip->out_dim;
    const size_t per = (size_t)h * w * 3;
    float* d_out = ctx->out_buf((size_t)n * (2 * od + 1));
    float* d_feat = d_out; float* d_norm = d_out + (size_t)n * od; float* d_aes = d_out + (size_t)n * 2 * od;
    ClipBatcher tower(ctx, n, ctx->microbatch, d_feat, emb_norm ? d_norm : nullptr, aesthetic_raw ? d_aes : nullptr);
    ImageStager st(ctx, rgb, n, per, ctx->microbatch, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int i0 = k * ctx->microbatch, nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      Tensor xt = preprocess_square224(C, d_in, nb, h, w, FE_FILTER_BICUBIC, true, kClipMean, kClipStd, 0);
      st.done(k);   // the raw images are consumed by the resize kernels queued above
      (void)i0;
      tower.push(xt);
    }
    tower.finish();
    if (features) FE_HIP(hipMemcpyAsync(features, d_feat, (size_t)n * od * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    if (emb_norm) FE_HIP(hipMemcpyAsync(emb_norm, d_norm, (size_t)n * od * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    if (aesthetic_raw) FE_HIP(hipMemcpyAsync(aesthetic_raw, d_aes, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

// SAMPNetScorer.score_batch from raw images (samp_net.py:904-928, 991-1010): BGR->RGB if bgr, PIL bilinear
// Resize((224,224)), ToTensor, ImageNet Normalize, U2NETP saliency, SAMPNet.
int fe_samp_score_images(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device,
                         float* pattern_weights, float* attributes, float* score_dist) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.u2netp || !C.samp) { C.err = "samp_net / u2netp weights not loaded"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(img && n > 0 && pattern_weights && attributes && score_dist, "bad arguments");
    const size_t per = (size_t)h * w * 3;
    float* d_out = ctx->out_buf((size_t)n * 19);
    SampBatcher batch(ctx, n, ctx->microbatch, d_out, d_out + (size_t)n * 8, d_out + (size_t)n * 14);
    ImageStager st(ctx, img, n, per, ctx->microbatch, on_device);
    for (int k = 0; k < st.chunks(); ++k) {
      const int nb = st.count(k);
      C.arena.reset();
      const uint8_t* d_in = st.get(k);
      Tensor xt = preprocess_square224(C, d_in, nb, h, w, FE_FILTER_BILINEAR, false, kImagenetMean, kImagenetStd, bgr);
      st.done(k);
      batch.push(xt);
    }
    batch.finish();
    FE_HIP(hipMemcpyAsync(pattern_weights, d_out, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(attributes, d_out + (size_t)n * 8, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(score_dist, d_out + (size_t)n * 14, (size_t)n * 5 * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

// CLIP text tower: tokens int32 [n][ctx_len] (host) -> un-normalised text features [n][768].
// Reference: `self.model.encode_text(text_tokens)` in CLIPTagger._precompute_text_embeddings (models/tagger.py:69-75).
int fe_clip_encode_text(fe_ctx* ctx, const int32_t* tokens, int n, int ctx_len, float* features) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    if (!C.clip_text) { C.err = "clip text tower not loaded (checkpoint had no token_embedding.weight)"; return FE_ERR_NOT_LOADED; }
    FE_CHECK(tokens && features && n > 0 && ctx_len == C.clip_text->ctx, "bad arguments (context length must be %d)", C.clip_text->ctx);
    const int od = C.clip_text->out_dim;
    std::vector<int> eot(n);
    for (int b = 0; b < n; ++b) {   // text.argmax(dim=-1): first position of the largest token id (the EOT token)
      int best = 0;
      for (int t = 1; t < ctx_len; ++t)
        if (tokens[(size_t)b * ctx_len + t] > tokens[(size_t)b * ctx_len + best]) best = t;
      eot[b] = best;
    }
    float* d_out = ctx->out_buf((size_t)n * od);
    const int mb = std::max(1, ctx->microbatch * 4);
    for (int i0 = 0; i0 < n; i0 += mb) {
      const int nb = std::min(mb, n - i0);
      C.arena.reset();
      int* d_tok = upload(C, tokens + (size_t)i0 * ctx_len, (size_t)nb * ctx_len);
      int* d_eot = upload(C, eot.data() + i0, (size_t)nb);
      clip_text_forward(C, *C.clip_text, d_tok, d_eot, nb, d_out + (size_t)i0 * od);
      FE_HIP(hipStreamSynchronize(C.stream));
    }
    FE_HIP(hipMemcpyAsync(features, d_out, (size_t)n * od * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

// Batched zero-shot tag scoring: sims[n][T] = emb[n][d] . text[T][d]^T on the matrix cores (both host, row-major).
// Replaces the per-image `image_features @ text_embeddings.T` + python loop of models/tagger.py:100-106.
int fe_tag_similarities(fe_ctx* ctx, const float* emb, int n, const float* text, int T, int d, float* sims) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(emb && text && sims && n > 0 && T > 0 && d > 0 && d % 4 == 0, "bad arguments");
    C.arena.reset();
    DeviceWeights dw;
    HostTensor w; w.shape = {T, d}; w.data.assign(text, text + (size_t)T * d);
    ConvW tw = build_linear_rows(dw, w, nullptr, 0, T);
    float* d_e = (float*)C.arena.alloc((size_t)n * tw.CinPad * sizeof(float));
    float* d_s = (float*)C.arena.alloc((size_t)n * T * sizeof(float));
    FE_HIP(hipMemcpyAsync(d_e, emb, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, C.stream));
    linear_forward(C, tw, d_e, d, n, d_s, T, ACT_NONE);
    FE_HIP(hipMemcpyAsync(sims, d_s, (size_t)n * T * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

// One call per batch for the whole ensemble (what processing/batch_processor.py:169-360 sequences per image):
// record[i] = [topiq_raw, aesthetic_raw, pattern_weights(8), attributes(6), score_dist(5), clip_emb_norm(768)] = 789 floats.
// Models that are not loaded leave their fields at 0 (mask bit i of *models_run: 1 topiq, 2 clip, 4 samp).
int fe_ensemble_select(fe_ctx* ctx, int models) {
  return fe_api(ctx, [&] {
    FE_CHECK(models > 0 && models <= 7, "ensemble_select: mask %d (1 topiq | 2 clip | 4 samp)", models);
    ctx->ensemble_mask = models;
  });
}

int fe_ensemble_score(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* records, int* models_run) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(rgb && records && n > 0 && h >= 32 && w >= 32, "bad arguments");
    const size_t floats = (size_t)n * FE_RECORD_FLOATS;
    if (floats > ctx->d_rec_cap) {
      if (ctx->d_rec) FE_HIP(hipFree(ctx->d_rec));
      ctx->d_rec = nullptr; ctx->d_rec_cap = 0;
      FE_HIP(hipMalloc((void**)&ctx->d_rec, floats * sizeof(float)));
      ctx->d_rec_cap = floats;
    }
    const int ran = ensemble_run(ctx, rgb, n, h, w, on_device, ctx->d_rec, FE_RECORD_FLOATS);
    FE_HIP(hipMemcpyAsync(records, ctx->d_rec, floats * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    if (models_run) *models_run = ran;
  });
}

// Same, with the records left in DEVICE memory: d_records [n][ld_records] floats (ld_records >= FE_RECORD_FLOATS; the columns past
// 789 are not touched, so a caller can keep its face slots beside them). Returns after the engine stream has drained, so the
// buffer can be handed to a collective on another stream (the multi-GPU all-gather reads it in place: facet_amd/sharding.py).
int fe_ensemble_score_dev(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* d_records, int ld_records,
                          int* models_run) {
  return fe_api(ctx, [&] {
    FE_CHECK(rgb && d_records && n > 0 && h >= 32 && w >= 32 && ld_records >= FE_RECORD_FLOATS, "bad arguments");
    const int ran = ensemble_run(ctx, rgb, n, h, w, on_device, d_records, ld_records);
    FE_HIP(hipStreamSynchronize(ctx->c.stream));
    if (models_run) *models_run = ran;
  });
}

// fe_ensemble_score on a list of images that each have their own size (include/facet_engine.h has the contract, ensemble_run_mixed the schedule).
int fe_ensemble_score_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, float* records,
                            int* models_run) {
  return fe_api(ctx, [&]() -> int {
    Ctx& C = ctx->c;
    if (!records) { C.err = "fe_ensemble_score_mixed: bad arguments (null records)"; return FE_ERR_INVALID; }
    if (!mixed_list_ok(C, "fe_ensemble_score_mixed", images, hw, n, FE_ORDER_RGB, images, mixed_limits(32))) return FE_ERR_INVALID;
    const size_t floats = (size_t)n * FE_RECORD_FLOATS;
    if (floats > ctx->d_rec_cap) {
      if (ctx->d_rec) FE_HIP(hipFree(ctx->d_rec));
      ctx->d_rec = nullptr; ctx->d_rec_cap = 0;
      FE_HIP(hipMalloc((void**)&ctx->d_rec, floats * sizeof(float)));
      ctx->d_rec_cap = floats;
    }
    const int ran = ensemble_run_mixed(ctx, images, hw, n, on_device, ctx->d_rec, FE_RECORD_FLOATS);
    FE_HIP(hipMemcpyAsync(records, ctx->d_rec, floats * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    if (models_run) *models_run = ran;
    return FE_OK;
  });
}

// The mixed-size preprocessing kernels alone: uint8 crops to the host. Works through the list in pieces of fe_set_microbatch images, each with
// its descriptors, table pool, (host input) images and intermediates in the arena.
int fe_preprocess224_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int mode, uint8_t* crops) {
  return fe_api(ctx, [&]() -> int {
    Ctx& C = ctx->c;
    if (!crops || (mode != FE_MIXED_CLIP && mode != FE_MIXED_SAMP)) { C.err = "fe_preprocess224_mixed: bad arguments (null crops, or mode not 0 / 1)"; return FE_ERR_INVALID; }
    if (!mixed_list_ok(C, "fe_preprocess224_mixed", images, hw, n, FE_ORDER_RGB, images, mixed_limits(1))) return FE_ERR_INVALID;
    const size_t crop_bytes = (size_t)kMixedSide * kMixedSide * 3;
    std::vector<size_t> offs;
    for (int i0 = 0; i0 < n; i0 += ctx->microbatch) {
      const int nb = std::min(ctx->microbatch, n - i0);
      C.arena.reset();
      MixedTables tables;
      std::vector<MixedDesc> desc(nb);
      size_t inter = 0;
      int max_nr = 0;
      for (int j = 0; j < nb; ++j) {
        const int i = i0 + j;
        MixedDesc& d = desc[j];
        FE_CHECK(tables.describe(mode, hw[2 * i], hw[2 * i + 1], d), "preprocess224_mixed: image %d (%d x %d) cannot be resampled to 224 x 224", i, hw[2 * i], hw[2 * i + 1]);
        d.slot = j;
        FE_CHECK(inter + MixedTables::inter_bytes(d) < ((size_t)1 << 32), "preprocess224_mixed: intermediates exceed 4 GiB");
        d.inter = (uint32_t)inter;
        inter += MixedTables::inter_bytes(d);
        if (d.ksize_h) max_nr = std::max(max_nr, (int)d.nr);
      }
      uint8_t* d_src = on_device ? nullptr : (uint8_t*)C.arena.alloc(mixed_list::staged_offsets(hw, i0, i0 + nb, false, offs));
      stage_images(C, images, hw, i0, i0 + nb, on_device, d_src, offs.data(), [&](int i, const uint8_t* src) { desc[i - i0].src = src; });
      if (tables.pool.empty()) tables.pool.push_back(0);      // every image 224 x 224: no pass, but the kernel still takes a pool
      const MixedDesc* d_desc = upload(C, desc.data(), desc.size());
      const int32_t* d_pool = upload(C, tables.pool.data(), tables.pool.size());
      uint8_t* d_inter = inter ? (uint8_t*)C.arena.alloc(inter) : nullptr;
      uint8_t* d_crops = (uint8_t*)C.arena.alloc((size_t)nb * crop_bytes);
      resize_mixed224(C, d_desc, nb, max_nr, d_pool, d_inter, d_crops, nullptr, nullptr, nullptr);
      FE_HIP(hipMemcpyAsync(crops + (size_t)i0 * crop_bytes, d_crops, (size_t)nb * crop_bytes, hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));      // descriptors and pool are host memory of this iteration
    }
    return FE_OK;
  });
}

}  // extern "C"
