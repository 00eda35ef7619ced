// C ABI of libfacet_engine.so (declared in include/facet_engine.h): the context and its runtime - lifetime, memory, timers, profile, weights.
// The other entry points are in capi_<domain>.hip; capi_internal.h holds what they share.
#include "capi_internal.h"

static std::string g_create_err;   // fe_create has no context to leave its message in

extern "C" {

const char* fe_version(void) { return "facet_amd 0.1 (gfx950)"; }

int fe_create(int device, size_t arena_bytes, fe_ctx** out) {
  if (!out) return FE_ERR_INVALID;
  *out = nullptr;
  try {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) throw Error(std::string("no HIP device available: ") + hipGetErrorString(e));
    FE_CHECK(device >= 0 && device < ndev, "device %d out of range (%d devices)", device, ndev);
    FE_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    FE_HIP(hipGetDeviceProperties(&prop, device));
    FE_CHECK(std::string(prop.gcnArchName).rfind("gfx950", 0) == 0, "device %d is %s; this engine is built for gfx950 only",
             device, prop.gcnArchName);
    auto* x = new fe_ctx();
    x->c.device = device;
    FE_HIP(hipStreamCreateWithFlags(&x->c.stream, hipStreamNonBlocking));
    if (!arena_bytes) {
      // default workspace: a quarter of the free HBM, capped at 64 GiB (8 x 1024^2 images of TOPIQ in flight need ~13 GB,
      // 128 SAMP crops ~20 GB); on a 288 GB MI355X that is 64 GiB. Pass an explicit size to override.
      size_t free_b = 0, total_b = 0;
      FE_HIP(hipMemGetInfo(&free_b, &total_b));
      arena_bytes = std::min<size_t>((size_t)64 << 30, std::max<size_t>((size_t)2 << 30, free_b / 4));
    }
    x->c.arena.init(arena_bytes);
    FE_HIP(hipEventCreate(&x->t0));
    FE_HIP(hipEventCreate(&x->t1));
    *out = x;
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return FE_ERR_RUNTIME;
  }
  return FE_OK;
}

void fe_destroy(fe_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->c.device);
  (void)hipStreamSynchronize(ctx->c.stream);
  if (ctx->t0) (void)hipEventDestroy(ctx->t0);
  if (ctx->t1) (void)hipEventDestroy(ctx->t1);
  if (ctx->d_out) (void)hipFree(ctx->d_out);
  if (ctx->d_rec) (void)hipFree(ctx->d_rec);
  if (ctx->mixed_buf) (void)hipFree(ctx->mixed_buf);
  for (int i = 0; i < 2; ++i) {
    if (ctx->stage_buf[i]) (void)hipFree(ctx->stage_buf[i]);
    if (ctx->ev_copied[i]) (void)hipEventDestroy(ctx->ev_copied[i]);
    if (ctx->ev_consumed[i]) (void)hipEventDestroy(ctx->ev_consumed[i]);
  }
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  if (ctx->side.stream) {
    (void)hipStreamSynchronize(ctx->side.stream);
    (void)hipStreamDestroy(ctx->side.stream);
  }
  for (hipEvent_t e : {ctx->side.ev_start, ctx->side.ev_join, ctx->side.ev_read[0], ctx->side.ev_read[1]})
    if (e) (void)hipEventDestroy(e);
  ctx->side.arena.release();
  for (void* q : ctx->misc_allocs) (void)hipFree(q);
  if (ctx->lines_maps) (void)hipHostFree(ctx->lines_maps);
  if (ctx->clip_in) (void)hipFree(ctx->clip_in);
  if (ctx->samp_in) (void)hipFree(ctx->samp_in);
  delete ctx;
}

const char* fe_last_error(fe_ctx* ctx) { return ctx ? ctx->c.err.c_str() : g_create_err.c_str(); }

int fe_sync(fe_ctx* ctx) {
  return fe_api(ctx, [&] {
    FE_HIP(hipStreamSynchronize(ctx->c.stream));
  });
}

int fe_set_microbatch(fe_ctx* ctx, int n) {
  return fe_api(ctx, [&] {
    FE_CHECK(n >= 1 && n <= 256, "microbatch %d out of range", n);
    ctx->microbatch = n;
  });
}

int fe_set_conv_variant(fe_ctx* ctx, int variant) {
  return fe_api(ctx, [&] {
    ctx->c.force_variant = variant;
  });
}

int fe_dev_alloc(fe_ctx* ctx, size_t bytes, void** d_out) {
  return fe_api(ctx, [&] {
    FE_CHECK(d_out != nullptr, "null out");
    FE_HIP(hipSetDevice(ctx->c.device));
    FE_HIP(hipMalloc(d_out, bytes ? bytes : 16));
  });
}
int fe_dev_free(fe_ctx* ctx, void* d_ptr) {
  return fe_api(ctx, [&] {
    FE_HIP(hipFree(d_ptr));
  });
}
int fe_memcpy_h2d(fe_ctx* ctx, void* d_dst, const void* src, size_t bytes) {
  return fe_api(ctx, [&] {
    FE_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->c.stream));
    FE_HIP(hipStreamSynchronize(ctx->c.stream));
  });
}
int fe_memcpy_d2h(fe_ctx* ctx, void* dst, const void* d_src, size_t bytes) {
  return fe_api(ctx, [&] {
    FE_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->c.stream));
    FE_HIP(hipStreamSynchronize(ctx->c.stream));
  });
}

int fe_timer_start(fe_ctx* ctx) {
  return fe_api(ctx, [&] {
    FE_HIP(hipEventRecord(ctx->t0, ctx->c.stream));
  });
}
int fe_timer_stop(fe_ctx* ctx, float* ms_out) {
  return fe_api(ctx, [&] {
    FE_HIP(hipEventRecord(ctx->t1, ctx->c.stream));
    FE_HIP(hipEventSynchronize(ctx->t1));
    FE_HIP(hipEventElapsedTime(ms_out, ctx->t0, ctx->t1));
  });
}
int fe_profile_enable(fe_ctx* ctx, int on) {
  return fe_api(ctx, [&] {
    ctx->c.profile = on != 0;
    ctx->c.timings.clear();
  });
}
int fe_profile_count(fe_ctx* ctx) { return ctx ? (int)ctx->c.timings.size() : 0; }
int fe_profile_get(fe_ctx* ctx, int i, char* name, int name_cap, double* flops, double* bytes, float* ms) {
  return fe_api(ctx, [&] {
    FE_CHECK(i >= 0 && i < (int)ctx->c.timings.size(), "profile index %d", i);
    const OpTiming& t = ctx->c.timings[i];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", t.name.c_str());
    if (flops) *flops = t.flops;
    if (bytes) *bytes = t.bytes;
    if (ms) *ms = t.ms;
  });
}
int fe_flops_reset(fe_ctx* ctx) {
  return fe_api(ctx, [&] {
    ctx->c.flops_accum = 0.0;
    ctx->c.flops_saved = 0.0;
    ctx->c.flops_half = 0.0;
  });
}
int fe_flops_get_half(fe_ctx* ctx, double* flops) {
  return fe_api(ctx, [&] {
    FE_CHECK(flops, "bad arguments");
    *flops = ctx->c.flops_half;
  });
}
int fe_flops_get_executed(fe_ctx* ctx, double* flops) {
  return fe_api(ctx, [&] {
    FE_CHECK(flops, "bad arguments");
    *flops = ctx->c.flops_accum - ctx->c.flops_saved;
  });
}
int fe_flops_get(fe_ctx* ctx, double* flops) {
  return fe_api(ctx, [&] {
    *flops = ctx->c.flops_accum;
  });
}

// ---- weights ------------------------------------------------------------------------------------
int fe_weights_begin(fe_ctx* ctx, int model) {
  return fe_api(ctx, [&] {
    FE_CHECK(model >= 0 && model < 8, "model id %d", model);
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    ctx->c.staging[model].clear();
  });
}
int fe_weights_set(fe_ctx* ctx, int model, const char* name, const float* data, const int64_t* shape, int ndim) {
  return fe_api(ctx, [&] {
    FE_CHECK(model >= 0 && model < 8 && name && data && shape && ndim >= 0 && ndim <= 6, "bad arguments");
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    ctx->c.staging[model].set(name, data, shape, ndim);
  });
}
int fe_set_precision(fe_ctx* ctx, int precision) {
  return fe_api(ctx, [&] {
    const int base = precision & ~(FE_PRECISION_RES32 | FE_PRECISION_SPLIT3);
    FE_CHECK(!(precision & FE_PRECISION_SPLIT3) || base == FE_PRECISION_F16, "set_precision: FE_PRECISION_SPLIT3 qualifies FE_PRECISION_F16");
    FE_CHECK(base == FE_PRECISION_F32 || base == FE_PRECISION_BF16 || base == FE_PRECISION_F16, "set_precision: %d", precision);
    FE_CHECK(base != FE_PRECISION_F32 || !(precision & FE_PRECISION_RES32), "set_precision: FE_PRECISION_RES32 qualifies a 2-byte precision");
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    ctx->c.precision = base;
    ctx->c.res32 = (precision & (FE_PRECISION_RES32 | FE_PRECISION_SPLIT3)) != 0;      // split operands imply fp32 streams
    ctx->c.split3 = (precision & FE_PRECISION_SPLIT3) != 0;
  });
}
int fe_model_precision(fe_ctx* ctx, int model) {
  if (!ctx) return -1;
  auto code = [](const DeviceWeights& dw) { return dw.prec | (dw.res32 ? FE_PRECISION_RES32 : 0) | (dw.split3 ? FE_PRECISION_SPLIT3 : 0); };
  if (model == FE_MODEL_TOPIQ && ctx->c.topiq) return code(ctx->c.topiq->dw);
  if (model == FE_MODEL_U2NETP && ctx->c.u2netp) return code(ctx->c.u2netp->dw);
  if (model == FE_MODEL_SAMP && ctx->c.samp) return code(ctx->c.samp->dw);
  if (model == FE_MODEL_CLIP && ctx->c.clip) return code(ctx->c.clip->dw);
  if (model == FE_MODEL_AESTHETIC && ctx->c.aesthetic) return FE_PRECISION_F32;
  if (model == FE_MODEL_VLM && ctx->c.vlm) return FE_PRECISION_BF16;
  return -1;
}

int fe_topiq_f32_below(fe_ctx* ctx, long long pixels) {
  return fe_api(ctx, [&] {
    FE_CHECK(pixels >= 0, "topiq_f32_below: negative pixel count");
    ctx->c.topiq_f32_below = (size_t)pixels;
  });
}

int fe_topiq_configure(fe_ctx* ctx, int gate_act, int weight_blk_act) {
  return fe_api(ctx, [&] {
    auto ok = [](int a) { return a == FE_ACT_RELU || a == FE_ACT_GELU || a == FE_ACT_SOFTPLUS; };
    FE_CHECK(ok(gate_act) && ok(weight_blk_act), "topiq_configure: activations must be relu, gelu or softplus");
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    ctx->c.topiq_gate_act = gate_act;
    ctx->c.topiq_wblk_act = weight_blk_act;
  });
}

int fe_weights_commit(fe_ctx* ctx, int model) {
  return fe_api(ctx, [&] {
    FE_CHECK(model >= 0 && model < 8, "model id %d", model);
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    FE_HIP(hipSetDevice(ctx->c.device));
    WeightStore& ws = ctx->c.staging[model];
    if (model == FE_MODEL_TOPIQ) {
      auto m = std::make_unique<TopiqModel>();
      m->dw.prec = ctx->c.precision; m->dw.res32 = ctx->c.res32;
      m->gate_act = ctx->c.topiq_gate_act;
      m->wblk_act = ctx->c.topiq_wblk_act;
      const int blocks[4] = {3, 4, 6, 3};
      build_resnet(m->backbone, m->dw, ws, "semantic_model.", true, blocks, false);
      if (ws.has("weight_pool.0.splitconv.weight")) build_topiq_head(*m, ws);
      ctx->c.topiq = std::move(m);
    } else if (model == FE_MODEL_U2NETP) {
      auto m = std::make_unique<U2NetPModel>();
      m->dw.prec = ctx->c.precision; m->dw.res32 = ctx->c.res32;
      build_u2netp(*m, ws);
      ctx->c.u2netp = std::move(m);
    } else if (model == FE_MODEL_CLIP) {
      auto m = std::make_unique<ClipModel>();
      m->dw.prec = ctx->c.precision; m->dw.res32 = ctx->c.res32; m->dw.split3 = ctx->c.split3;      // the image tower; the text tower (built below, run once per vocabulary) stays fp32
      build_clip(*m, ws);
      ctx->c.clip = std::move(m);
      if (ws.has("token_embedding.weight")) {   // full CLIP checkpoint: also build the text tower
        auto t = std::make_unique<ClipTextModel>();
        build_clip_text(*t, ws);
        ctx->c.clip_text = std::move(t);
      } else {
        ctx->c.clip_text.reset();
      }
    } else if (model == FE_MODEL_AESTHETIC) {
      auto m = std::make_unique<AestheticModel>();
      build_aesthetic(*m, ws);
      ctx->c.aesthetic = std::move(m);
    } else if (model == FE_MODEL_SAMP) {
      auto m = std::make_unique<SampModel>();
      m->dw.prec = ctx->c.precision; m->dw.res32 = ctx->c.res32;
      build_sampnet(*m, ws);
      ctx->c.samp = std::move(m);
    } else if (model == FE_MODEL_VLM) {
      auto m = std::make_unique<VlmModel>();
      // bf16 arithmetic always: the precision the reference loads it in (models/vlm_tagger.py:155-156); the weights' storage is the caller's choice
      build_vlm(*m, ws, ctx->c.vlm_cfg, ctx->c.vlm_weight_format);
      ctx->c.vlm = std::move(m);
    } else {
      throw Error("fe_weights_commit: model " + std::to_string(model) + " not implemented");
    }
    ws.clear();
  });
}
int fe_model_unload(fe_ctx* ctx, int model) {
  return fe_api(ctx, [&] {
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    FE_HIP(hipStreamSynchronize(ctx->c.stream));
    if (model == FE_MODEL_TOPIQ) ctx->c.topiq.reset();
    if (model == FE_MODEL_U2NETP) ctx->c.u2netp.reset();
    if (model == FE_MODEL_SAMP) ctx->c.samp.reset();
    if (model == FE_MODEL_CLIP) { ctx->c.clip.reset(); ctx->c.clip_text.reset(); }
    if (model == FE_MODEL_AESTHETIC) ctx->c.aesthetic.reset();
    if (model == FE_MODEL_VLM) ctx->c.vlm.reset();
  });
}
int fe_model_loaded(fe_ctx* ctx, int model) {
  if (!ctx) return 0;
  if (model == FE_MODEL_TOPIQ) return ctx->c.topiq != nullptr;
  if (model == FE_MODEL_U2NETP) return ctx->c.u2netp != nullptr;
  if (model == FE_MODEL_SAMP) return ctx->c.samp != nullptr;
  if (model == FE_MODEL_CLIP) return ctx->c.clip != nullptr;
  if (model == FE_MODEL_AESTHETIC) return ctx->c.aesthetic != nullptr;
  if (model == FE_MODEL_VLM) return ctx->c.vlm != nullptr;
  return 0;
}

// Developer hook: time one conv shape on random data (device-resident), `iters` launches, forced tile variant.
int fe_bench_conv(fe_ctx* ctx, int n, int h, int w, int cin, int cout, int k, int stride, int pad, int with_res, int act,
                  int variant, int iters, float* ms_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    C.arena.reset();
    DeviceWeights dw;
    WeightStore ws;
    std::vector<float> hw((size_t)cout * cin * k * k);
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xFFFF) / 65536.0f - 0.5f; };
    for (auto& v : hw) v = rnd() * 0.1f;
    const int64_t wshape[4] = {cout, cin, k, k};
    ws.set("w.weight", hw.data(), wshape, 4);
    ConvW cw = build_conv(dw, ws, "w", "", false);
    std::vector<float> sc(cout, 1.01f), sh(cout, 0.1f);
    cw.scale = dw.upload(sc); cw.shift = dw.upload(sh);
    Tensor x = C.arena.tensor(n, h, w, cw.CinPad);
    {
      std::vector<float> hx((size_t)1 << 20);
      for (auto& v : hx) v = rnd();
      for (size_t off = 0; off < x.numel(); off += hx.size())
        FE_HIP(hipMemcpyAsync(x.p + off, hx.data(), std::min(hx.size(), x.numel() - off) * sizeof(float), hipMemcpyHostToDevice, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
    }
    ConvOpts o; o.sh = o.sw = stride; o.ph = o.pw = pad; o.act = act;
    Tensor y = C.arena.tensor(n, conv_out_dim(h, k, stride, pad, 1), conv_out_dim(w, k, stride, pad, 1), cout);
    Tensor r;
    if (with_res) { r = C.arena.tensor(y.n, y.h, y.w, y.c); FE_HIP(hipMemsetAsync(r.p, 0, r.numel() * sizeof(float), C.stream)); o.res = &r; }
    C.force_variant = variant;
    conv_forward(C, cw, x, y, o);  // warm
    FE_HIP(hipEventRecord(ctx->t0, C.stream));
    for (int i = 0; i < iters; ++i) conv_forward(C, cw, x, y, o);
    FE_HIP(hipEventRecord(ctx->t1, C.stream));
    FE_HIP(hipEventSynchronize(ctx->t1));
    C.force_variant = 0;
    float ms = 0.f;
    FE_HIP(hipEventElapsedTime(&ms, ctx->t0, ctx->t1));
    *ms_out = ms / iters;
  });
}

}  // extern "C"
