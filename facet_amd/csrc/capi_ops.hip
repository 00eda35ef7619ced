// C ABI: single operators and kernels launched alone, the test hooks of the suite.
#include "capi_internal.h"
#include "fp8_core.h"
#include "wino64_maps.h"

// ---- staging of the element-typed test hooks (fe_op_plane, fe_op_rowpass, fe_op_gemm_skinny) ---------------------------------------------
// n host floats -> n values of type E in the arena, rounded on the device; the array starts `off` elements past a 256-byte boundary
template <class E>
static E* hook_up(Ctx& C, const float* src, size_t n, int off = 0) {
  if (!src) return nullptr;
  if constexpr (std::is_same_v<E, float>) {
    float* d = C.arena.array<float>(n + off) + off;
    FE_HIP(hipMemcpyAsync(d, src, n * sizeof(float), hipMemcpyHostToDevice, C.stream));
    return d;
  } else {
    const float* d32 = upload(C, src, n);
    E* d = C.arena.array<E>(n + off) + off;
    launch_convert(d32, d, n, C.stream);
    return d;
  }
}
// n values of `fill`, placed the same way
template <class E>
static E* hook_filled(Ctx& C, size_t n, float fill, int off = 0) {
  const std::vector<float> v(n, fill);
  E* d = hook_up<E>(C, v.data(), n, off);
  FE_HIP(hipStreamSynchronize(C.stream));      // (v dies with this block)
  return d;
}
// n values of type E in device memory -> host floats (synchronises)
template <class E>
static void hook_down(Ctx& C, const E* src, size_t n, float* dst) {
  const float* d32;
  if constexpr (std::is_same_v<E, float>) {
    d32 = src;
  } else {
    float* t = C.arena.array<float>(n);
    launch_convert(src, t, n, C.stream);
    d32 = t;
  }
  FE_HIP(hipMemcpyAsync(dst, d32, n * sizeof(float), hipMemcpyDeviceToHost, C.stream));
  FE_HIP(hipStreamSynchronize(C.stream));
}
template <class TI, class TO>
static void hook_layernorm(Ctx& C, const float* x, int rows, int d, int ldx, int ldy, int off_x, int off_y, const float* g, const float* b, int off_gb,
                           float eps, float fill, float* y) {
  const size_t ny = (size_t)rows * ldy;
  const TI* dx = hook_up<TI>(C, x, (size_t)rows * ldx, off_x);
  TO* dy = hook_filled<TO>(C, ny, fill, off_y);
  const float *dg = hook_up<float>(C, g, (size_t)d, off_gb), *db = hook_up<float>(C, b, (size_t)d, off_gb);
  launch_layernorm(dx, ldx, dy, ldy, dg, db, rows, d, eps, C.stream);
  hook_down(C, dy, ny, y);
}
template <class TI, class TO>
static void hook_convert(Ctx& C, const float* x, size_t n, float fill, float* y) {
  const TI* dx = hook_up<TI>(C, x, n);
  TO* dy = hook_filled<TO>(C, n, fill);
  launch_convert(dx, dy, n, C.stream);
  hook_down(C, dy, n, y);
}
template <class TI, class TW, class TO>
static void hook_gemm_skinny(Ctx& C, const float* x, int M, int K, int ldx, const float* w, int N, int ldw, const float* scale, const float* shift, int act,
                             int ldy, float fill, float* y, const float* res = nullptr, int ldr = 0) {
  const size_t ny = (size_t)M * ldy;
  const TO* dr = hook_up<TO>(C, res, (size_t)M * ldr);
  const TI* dx = hook_up<TI>(C, x, (size_t)M * ldx);
  const TW* dw = hook_up<TW>(C, w, (size_t)N * ldw);
  const float *ds = hook_up<float>(C, scale, (size_t)N), *dh = hook_up<float>(C, shift, (size_t)N);
  TO* dy = hook_filled<TO>(C, ny, fill);
  launch_gemm_skinny(dx, ldx, dw, ldw, ds, dh, dy, ldy, M, N, K, act, C.stream, dr, ldr);
  hook_down(C, dy, ny, y);
}

extern "C" {

int fe_op_conv2d(fe_ctx* ctx, const float* x, int n, int c, int h, int w, const float* weight, int cout, int kh, int kw,
                 const float* scale, const float* shift, const float* res, int res_after_act, int stride, int pad,
                 int dil, int act, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(x && weight && y && n > 0 && c > 0 && h > 0 && w > 0 && cout > 0 && kh > 0 && kw > 0 && stride > 0 && dil > 0,
             "bad conv arguments");
    C.arena.reset();
    DeviceWeights dw;
    dw.prec = C.precision;      // FE_PRECISION_BF16: the same op on the bf16 kernel (inputs rounded to bf16 on upload, fp32 back)
    WeightStore ws;
    const int64_t wshape[4] = {cout, c, kh, kw};
    ws.set("w.weight", weight, wshape, 4);
    ConvW cw = build_conv(dw, ws, "w", "", false);
    std::vector<float> v;
    if (scale) { v.assign(scale, scale + cout); cw.scale = dw.upload(v); }
    if (shift) { v.assign(shift, shift + cout); cw.shift = dw.upload(v); }
    const int ho = conv_out_dim(h, kh, stride, pad, dil), wo = conv_out_dim(w, kw, stride, pad, dil);
    FE_CHECK(ho > 0 && wo > 0, "conv output is empty");
    auto half_op = [&](auto* tag) {      // the same op on the 2-byte kernel (inputs rounded on upload, fp32 back)
      typedef std::remove_pointer_t<decltype(tag)> E;
      FE_CHECK(cw.wh, "fe_op_conv2d(2-byte): Cin must be a multiple of 8 (16 for spatial kernels)");
      TensorT<E> xt = upload_nchw<E>(C, x, n, c, h, w, cw.CinPadH);
      ConvOptsT<E> o;
      o.sh = o.sw = stride; o.ph = o.pw = pad; o.dh = o.dw = dil; o.act = act; o.res_after_act = res_after_act;
      TensorT<E> rt;
      if (C.res32) {
        // FE_PRECISION_RES32: the fp32-stream form of the layer - residual read as fp32, result written both as fp32 rows (returned)
        // and as 2-byte rows, which must be the rounding of the fp32 ones (checked here: this entry point is the kernels' test hook)
        Tensor r32, y32 = C.arena.tensor(n, ho, wo, cout);
        if (res) { r32 = upload_nchw(C, res, n, cout, ho, wo, cout); o.res32 = &r32; }
        o.y32 = &y32;
        TensorT<E> yt = C.arena.tensor_t<E>(n, ho, wo, cout);
        conv_forward(C, cw, xt, yt, o);
        download_nchw(C, y32, cout, y);
        std::vector<float> y16((size_t)n * cout * ho * wo);
        download_nchw(C, yt, cout, y16.data());
        for (size_t i = 0; i < y16.size(); ++i) {
          const float a = std::fmin(std::fmax(y[i], -65504.f), 65504.f);
          FE_CHECK(std::fabs(y16[i] - a) <= std::fabs(a) * (PrecOf<E>::value == PREC_F16 ? 4.9e-4f : 3.95e-3f) + 6.2e-5f,
                   "fe_op_conv2d(res32): 2-byte output %g is not the rounding of the fp32 output %g at %zu", y16[i], y[i], i);
        }
        return;
      }
      if (res) { rt = upload_nchw<E>(C, res, n, cout, ho, wo, cout); o.res = &rt; }
      TensorT<E> yt = conv_new(C, cw, xt, o);
      download_nchw(C, yt, cout, y);
    };
    if (C.precision == PREC_BF16) {
      half_op((bf16*)nullptr);
    } else if (C.precision == PREC_F16) {
      half_op((f16*)nullptr);
    } else {
      Tensor xt = upload_nchw(C, x, n, c, h, w, cw.CinPad);
      ConvOpts o;
      o.sh = o.sw = stride; o.ph = o.pw = pad; o.dh = o.dw = dil; o.act = act; o.res_after_act = res_after_act;
      Tensor rt;
      if (res) { rt = upload_nchw(C, res, n, cout, ho, wo, cout); o.res = &rt; }
      Tensor yt = conv_new(C, cw, xt, o);
      download_nchw(C, yt, cout, y);
    }
  });
}

int fe_op_gate_rowpool(fe_ctx* ctx, const float* x, int n, int h, int w, int cin, int ldx, const float* weight, const float* bias, int cout,
                       const float* gate, int act, int th, int tw, int fused, float* y, int* routed) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(x && weight && gate && y && n > 0 && h > 0 && w > 0 && cin > 0 && ldx >= cin && cout > 0 && th > 0 && tw > 0 && th <= h && tw <= w,
             "bad gate_rowpool arguments");
    FE_CHECK(C.precision == PREC_F32, "fe_op_gate_rowpool: fp32 contexts only");
    C.arena.reset();
    DeviceWeights dw;
    dw.prec = PREC_F32;
    HostTensor W, B;
    W.shape = {cout, cin}; W.data.assign(weight, weight + (size_t)cout * cin);
    if (bias) { B.shape = {cout}; B.data.assign(bias, bias + cout); }
    ConvW cw = build_linear_rows(dw, W, bias ? &B : nullptr, 0, cout);
    FE_CHECK(cw.CinPad <= ldx, "fe_op_gate_rowpool: ldx below the packed channel count %d", cw.CinPad);
    Tensor xt = C.arena.tensor(n, h, w, ldx);
    FE_HIP(hipMemcpyAsync(xt.p, x, xt.numel() * sizeof(float), hipMemcpyHostToDevice, C.stream));
    Tensor gt = C.arena.tensor(n, h, w, 1);
    FE_HIP(hipMemcpyAsync(gt.p, gate, gt.numel() * sizeof(float), hipMemcpyHostToDevice, C.stream));
    ConvOpts og; og.act = act; og.gate = &gt;
    int took = 0;
    Tensor pooled = topiq_gate_pool(C, cw, xt.slice(0, cw.CinPad), og, th, tw, fused != 0, &took);
    FE_CHECK(pooled.h == th && pooled.w == tw && pooled.ld == cout, "fe_op_gate_rowpool: unexpected result shape");
    FE_HIP(hipMemcpyAsync(y, pooled.p, pooled.numel() * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    if (routed) *routed = took;
  });
}

int fe_op_wino64(fe_ctx* ctx, const float* x, int n, int c, int h, int w, const float* weight, int cout, const float* scale, const float* shift,
                 const float* res, int res_after_act, int act, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(x && weight && y && n > 0 && h > 0 && w > 0 && c > 0 && c <= 64 && c % 4 == 0 && cout > 0 && cout <= 64 && cout % 4 == 0, "bad wino64 arguments");
    FE_CHECK(C.precision == PREC_F32, "fe_op_wino64: fp32 contexts only");
    C.arena.reset();
    std::vector<float> U(w64::U_FLOATS);
    w64::pack_u(weight, cout, c, U.data());
    const float* dU = upload(C, U.data(), U.size());
    const float *ds = upload(C, scale, (size_t)cout), *dh = upload(C, shift, (size_t)cout);
    Tensor xt = upload_nchw(C, x, n, c, h, w, c);
    Tensor rt;
    if (res) rt = upload_nchw(C, res, n, cout, h, w, cout);
    Tensor yt = C.arena.tensor(n, h, w, cout);
    launch_wino64(xt, yt, dU, ds, dh, nullptr, act, res ? &rt : nullptr, res_after_act, C.stream);
    download_nchw(C, yt, cout, y);      // synchronises: U is read by then
  });
}

int fe_op_topiq_gate64(fe_ctx* ctx, const float* x, int n, int h, int w, const float* w0, const float* b0, const float* w2, const float* b2,
                       const float* w4, float b4, const float* wx, const float* bx, int wblk_act, int gate_act, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(x && w0 && b0 && w2 && b2 && w4 && wx && bx && y && n > 0 && h > 0 && w > 0 && h % 16 == 0 && w % 16 == 0, "bad gate64 arguments");
    FE_CHECK(C.precision == PREC_BF16 || C.precision == PREC_F16, "fe_op_topiq_gate64: the fused gate exists for the 2-byte element types only");
    C.arena.reset();
    DeviceWeights dw;
    dw.prec = C.precision;
    GatedConvW g;
    build_gate64_fragments(dw, g, w0, b0, w2, b2, w4, b4, wx, bx);
    auto run = [&](auto* tag) {
      typedef std::remove_pointer_t<decltype(tag)> E;
      TensorT<E> xt = upload_nchw<E>(C, x, n, 64, h, w, 64);
      TensorT<E> yt = C.arena.tensor_t<E>(n, h / 16, w / 16, 64);
      launch_topiq_gate64(xt, yt, g.fused, g.fused_bias, wblk_act, gate_act, C.stream);
      download_nchw(C, yt, 64, y);
    };
    if (C.precision == PREC_BF16) run((bf16*)nullptr); else run((f16*)nullptr);
  });
}

int fe_op_conv3x3_c64(fe_ctx* ctx, const float* x, int n, int h, int w, const float* w2, const float* scale2, const float* shift2, int act2,
                      const float* w3, const float* scale3, const float* shift3, const float* res, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(x && w2 && y && n > 0 && h > 0 && w > 0 && (!w3 || res), "bad conv3x3_c64 arguments");
    FE_CHECK(C.precision == PREC_BF16 || C.precision == PREC_F16, "fe_op_conv3x3_c64: the halo-tiled kernel exists for the 2-byte element types only");
    C.arena.reset();
    DeviceWeights dw;
    dw.prec = C.precision;
    void *f2 = nullptr, *f3 = nullptr;
    build_c64_fragments(dw, w2, w3, &f2, &f3);
    std::vector<float> v;
    auto up = [&](const float* a, int cnt) -> float* { if (!a) return nullptr; v.assign(a, a + cnt); return dw.upload(v); };
    float *s2 = up(scale2, 64), *h2 = up(shift2, 64), *s3 = up(scale3, 256), *h3 = up(shift3, 256);
    const int cout = w3 ? 256 : 64;
    auto run = [&](auto* tag) {
      typedef std::remove_pointer_t<decltype(tag)> E;
      TensorT<E> xt = upload_nchw<E>(C, x, n, 64, h, w, 64);
      TensorT<E> yt = C.arena.tensor_t<E>(n, h, w, cout);
      TensorT<E> rt;
      if (w3) rt = upload_nchw<E>(C, res, n, 256, h, w, 256);
      launch_conv3x3_c64(xt, yt, w3 ? &rt : nullptr, f2, f3, s2, h2, s3, h3, act2, C.stream);
      download_nchw(C, yt, cout, y);
    };
    if (C.precision == PREC_BF16) run((bf16*)nullptr); else run((f16*)nullptr);
  });
}

int fe_op_maxpool2d(fe_ctx* ctx, const float* x, int n, int c, int h, int w, int k, int stride, int pad, int ceil_mode,
                    float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    C.arena.reset();
    Tensor xt = upload_nchw(C, x, n, c, h, w, c);
    auto od = [&](int in) {
      int o = ceil_mode ? (in + 2 * pad - k + stride - 1) / stride + 1 : (in + 2 * pad - k) / stride + 1;
      if (ceil_mode && (o - 1) * stride >= in + pad) --o;
      return o;
    };
    Tensor yt = C.arena.tensor(n, od(h), od(w), c);
    launch_maxpool(xt, yt, k, stride, pad, C.stream);
    download_nchw(C, yt, c, y);
  });
}

int fe_op_bilinear(fe_ctx* ctx, const float* x, int n, int c, int h, int w, int ho, int wo, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    C.arena.reset();
    Tensor xt = upload_nchw(C, x, n, c, h, w, c);
    Tensor yt = C.arena.tensor(n, ho, wo, c);
    launch_bilinear(xt, yt, C.stream);
    download_nchw(C, yt, c, y);
  });
}

int fe_op_adaptive_avgpool(fe_ctx* ctx, const float* x, int n, int c, int h, int w, int ho, int wo, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    C.arena.reset();
    Tensor xt = upload_nchw(C, x, n, c, h, w, c);
    Tensor yt = C.arena.tensor(n, ho, wo, c);
    launch_adaptive_avgpool(xt, yt, C.stream);
    download_nchw(C, yt, c, y);
  });
}

int fe_op_layernorm(fe_ctx* ctx, const float* x, int rows, int d, const float* g, const float* b, float eps, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    C.arena.reset();
    const size_t n = (size_t)rows * d;
    float* dx = upload(C, x, n);
    float* dy = C.arena.array<float>(n);
    float* dg = upload(C, g, (size_t)d);
    float* db = upload(C, b, (size_t)d);
    launch_layernorm(dx, d, dy, d, dg, db, rows, d, eps, C.stream);
    FE_HIP(hipMemcpyAsync(y, dy, n * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

// ---- test hooks of kernels_misc.hip on explicit element types (independent of the context's precision): upload, launch, download ----------
int fe_op_plane(fe_ctx* ctx, int route, int elem, const float* x, int n, int c, int h, int w, int ctot_in, int c0_in, int ctot_out, int c0_out,
                int k, int stride, int pad, int ceil_mode, int ho, int wo, float poison, float fill, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    enum { MAXPOOL = 0, BILINEAR = 1, AVGPOOL = 2 };
    FE_CHECK(x && y && route >= MAXPOOL && route <= AVGPOOL && n > 0 && c > 0 && h > 0 && w > 0 && ho > 0 && wo > 0, "bad plane arguments");
    FE_CHECK(c0_in >= 0 && c0_in + c <= ctot_in && c0_out >= 0 && c0_out + c <= ctot_out, "fe_op_plane: channels %d + %d of %d, %d + %d of %d", c0_in, c, ctot_in,
             c0_out, c, ctot_out);
    FE_CHECK((size_t)n * ctot_in * h * w <= (1u << 24) && (size_t)n * ctot_out * ho * wo <= (1u << 24), "fe_op_plane: up to 2^24 values a tensor");
    if (route == MAXPOOL) {
      FE_CHECK(k > 0 && stride > 0 && pad >= 0 && 2 * pad <= k, "fe_op_plane: max pool k %d stride %d pad %d", k, stride, pad);
      auto od = [&](int in) {
        int o = ceil_mode ? (in + 2 * pad - k + stride - 1) / stride + 1 : (in + 2 * pad - k) / stride + 1;
        if (ceil_mode && (o - 1) * stride >= in + pad) --o;
        return o;
      };
      FE_CHECK(ho == od(h) && wo == od(w), "fe_op_plane: max pool output %d x %d, expected %d x %d", ho, wo, od(h), od(w));
    }
    C.arena.reset();
    const size_t hw = (size_t)h * w;
    std::vector<float> xin((size_t)n * ctot_in * hw, poison);
    const std::vector<float> yin((size_t)n * ctot_out * ho * wo, fill);
    for (int img = 0; img < n; ++img)
      for (int ch = 0; ch < c; ++ch) memcpy(&xin[((size_t)img * ctot_in + c0_in + ch) * hw], x + ((size_t)img * c + ch) * hw, hw * sizeof(float));
    auto run = [&](auto* tag) {
      typedef std::remove_pointer_t<decltype(tag)> E;
      const TensorT<E> xt = upload_nchw<E>(C, xin.data(), n, ctot_in, h, w, ctot_in);
      const TensorT<E> yt = upload_nchw<E>(C, yin.data(), n, ctot_out, ho, wo, ctot_out);
      const TensorT<E> xv = xt.slice(c0_in, c), yv = yt.slice(c0_out, c);
      if (route == MAXPOOL) launch_maxpool(xv, yv, k, stride, pad, C.stream);
      else if (route == BILINEAR) launch_bilinear(xv, yv, C.stream);
      else launch_adaptive_avgpool(xv, yv, C.stream);
      download_nchw(C, yt, ctot_out, y);
    };
    if (elem == FE_ELEM_F32) run((float*)nullptr);
    else if (elem == FE_ELEM_BF16) run((bf16*)nullptr);
    else if (elem == FE_ELEM_F16) run((f16*)nullptr);
    else FE_CHECK(false, "fe_op_plane: element type %d", elem);
  });
}

int fe_op_rowpass(fe_ctx* ctx, int route, int elem_in, int elem_out, const float* x, int rows, int d, int ldx, int ldy, int off_x, int off_y,
                  const float* g, const float* b, int off_gb, int L, float eps, float fill, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    enum { LAYERNORM = 0, LAYERNORM_SPLIT = 1, SOFTMAX = 2, SOFTMAX_PAD = 3, ADD_ROWS = 4, SPLIT_HI_LO = 5, CONVERT = 6 };
    const int F = FE_ELEM_F32, B = FE_ELEM_BF16, H = FE_ELEM_F16;
    FE_CHECK(x && y && route >= LAYERNORM && route <= CONVERT && rows > 0 && d > 0 && ldx >= d && ldy >= d, "bad rowpass arguments");
    FE_CHECK((size_t)rows * ldx <= (1u << 24) && (size_t)rows * ldy <= (1u << 24), "fe_op_rowpass: up to 2^24 values an array");
    FE_CHECK(off_x >= 0 && off_x <= 3 && off_y >= 0 && off_y <= 3 && off_gb >= 0 && off_gb <= 3, "fe_op_rowpass: offsets %d, %d, %d (0 .. 3)", off_x, off_y, off_gb);
    const bool in_place = route == SOFTMAX || route == SOFTMAX_PAD || route == ADD_ROWS;
    FE_CHECK(!in_place || (ldy == ldx && off_y == off_x && elem_in == elem_out), "fe_op_rowpass: route %d runs in place (one stride, offset and type)", route);
    FE_CHECK((route == LAYERNORM || route == LAYERNORM_SPLIT) ? (g && b) : route == ADD_ROWS ? (g && !b && L > 0) : (!g && !b), "fe_op_rowpass: g / b of route %d", route);
    auto pair = [&](int a, int o) { return elem_in == a && elem_out == o; };
    const size_t nx = (size_t)rows * ldx, ny = (size_t)rows * ldy;
    C.arena.reset();
    if (route == LAYERNORM) {
      if (pair(F, F)) hook_layernorm<float, float>(C, x, rows, d, ldx, ldy, off_x, off_y, g, b, off_gb, eps, fill, y);
      else if (pair(B, B)) hook_layernorm<bf16, bf16>(C, x, rows, d, ldx, ldy, off_x, off_y, g, b, off_gb, eps, fill, y);
      else if (pair(H, H)) hook_layernorm<f16, f16>(C, x, rows, d, ldx, ldy, off_x, off_y, g, b, off_gb, eps, fill, y);
      else if (pair(F, B)) hook_layernorm<float, bf16>(C, x, rows, d, ldx, ldy, off_x, off_y, g, b, off_gb, eps, fill, y);
      else if (pair(F, H)) hook_layernorm<float, f16>(C, x, rows, d, ldx, ldy, off_x, off_y, g, b, off_gb, eps, fill, y);
      else FE_CHECK(false, "fe_op_rowpass: no LayerNorm from element type %d to %d", elem_in, elem_out);
    } else if (route == LAYERNORM_SPLIT) {
      FE_CHECK(pair(F, H) && ldy >= 2 * d, "fe_op_rowpass: layernorm_split is f32 -> f16 with ldy >= 2 d");
      const float* dx = hook_up<float>(C, x, nx, off_x);
      f16* dy = hook_filled<f16>(C, ny, fill, off_y);
      const float *dg = hook_up<float>(C, g, (size_t)d, off_gb), *db = hook_up<float>(C, b, (size_t)d, off_gb);
      launch_layernorm_split(dx, ldx, dy, ldy, dg, db, rows, d, eps, C.stream);
      hook_down(C, dy, ny, y);
    } else if (route == SOFTMAX || route == SOFTMAX_PAD) {
      FE_CHECK(pair(F, F), "fe_op_rowpass: the softmax kernels are fp32");
      float* dy = hook_up<float>(C, x, nx, off_x);
      if (route == SOFTMAX) launch_softmax_rows(dy, ldx, rows, d, C.stream);
      else launch_softmax_rows_pad(dy, ldx, rows, d, C.stream);
      hook_down(C, dy, nx, y);
    } else if (route == ADD_ROWS) {
      const float* dpos = hook_up<float>(C, g, (size_t)L * d, off_gb);
      auto run = [&](auto* tag) {
        typedef std::remove_pointer_t<decltype(tag)> E;
        E* dy = hook_up<E>(C, x, nx, off_x);
        launch_add_rows_bcast(dy, ldx, dpos, rows, L, d, C.stream);
        hook_down(C, dy, nx, y);
      };
      if (elem_in == F) run((float*)nullptr);
      else if (elem_in == B) run((bf16*)nullptr);
      else if (elem_in == H) run((f16*)nullptr);
      else FE_CHECK(false, "fe_op_rowpass: element type %d", elem_in);
    } else if (route == SPLIT_HI_LO) {
      FE_CHECK(pair(F, H) && ldx == d && ldy == 2 * d && off_x == 0 && off_y == 0, "fe_op_rowpass: split_hi_lo is dense f32 [rows][d] -> f16 [rows][2 d]");
      const float* dx = hook_up<float>(C, x, nx);
      f16* dy = hook_filled<f16>(C, ny, fill);
      launch_split_hi_lo(dx, dy, (size_t)rows, d, C.stream);
      hook_down(C, dy, ny, y);
    } else {
      FE_CHECK(ldx == d && ldy == d && off_x == 0 && off_y == 0, "fe_op_rowpass: convert takes dense arrays");
      if (pair(F, B)) hook_convert<float, bf16>(C, x, nx, fill, y);
      else if (pair(B, F)) hook_convert<bf16, float>(C, x, nx, fill, y);
      else if (pair(F, H)) hook_convert<float, f16>(C, x, nx, fill, y);
      else if (pair(H, F)) hook_convert<f16, float>(C, x, nx, fill, y);
      else FE_CHECK(false, "fe_op_rowpass: no conversion from element type %d to %d", elem_in, elem_out);
    }
  });
}

int fe_op_gemm_skinny(fe_ctx* ctx, int ti, int tw, int to, const float* x, int M, int K, int ldx, const float* w, int N, int ldw,
                      const float* scale, const float* shift, int act, int ldy, float fill, float* y) {
  if (M > 32) return fe_api(ctx, [&] { FE_CHECK(false, "bad skinny GEMM arguments"); });
  return fe_op_gemm_skinny_res(ctx, ti, tw, to, x, M, K, ldx, w, N, ldw, scale, shift, nullptr, 0, act, ldy, fill, y);
}

int fe_op_gemm_skinny_res(fe_ctx* ctx, int ti, int tw, int to, const float* x, int M, int K, int ldx, const float* w, int N, int ldw,
                          const float* scale, const float* shift, const float* res, int ldr, int act, int ldy, float fill, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    const int F = FE_ELEM_F32, B = FE_ELEM_BF16, H = FE_ELEM_F16;
    FE_CHECK(x && w && y && M > 0 && M <= 4096 && N > 0 && N <= 65536 && K > 0 && K <= 65536 && ldx >= K && ldx <= 2 * K + 64 && ldw >= K && ldw <= 2 * K + 64 && ldy >= N &&
             ldy <= 2 * N + 64 && (!res || (ldr >= N && ldr <= 2 * N + 64)), "bad skinny GEMM arguments");
    FE_CHECK(act >= ACT_NONE && act <= ACT_QUICKGELU && act != ACT_PRELU, "fe_op_gemm_skinny: activation %d", act);
    auto is = [&](int a, int b, int c) { return ti == a && tw == b && to == c; };
    C.arena.reset();
    if (is(F, F, F)) hook_gemm_skinny<float, float, float>(C, x, M, K, ldx, w, N, ldw, scale, shift, act, ldy, fill, y, res, ldr);
    else if (is(B, B, B)) hook_gemm_skinny<bf16, bf16, bf16>(C, x, M, K, ldx, w, N, ldw, scale, shift, act, ldy, fill, y, res, ldr);
    else if (is(B, B, F)) hook_gemm_skinny<bf16, bf16, float>(C, x, M, K, ldx, w, N, ldw, scale, shift, act, ldy, fill, y, res, ldr);
    else if (is(H, H, H)) hook_gemm_skinny<f16, f16, f16>(C, x, M, K, ldx, w, N, ldw, scale, shift, act, ldy, fill, y, res, ldr);
    else if (is(H, H, F)) hook_gemm_skinny<f16, f16, float>(C, x, M, K, ldx, w, N, ldw, scale, shift, act, ldy, fill, y, res, ldr);
    else if (is(F, B, F)) hook_gemm_skinny<float, bf16, float>(C, x, M, K, ldx, w, N, ldw, scale, shift, act, ldy, fill, y, res, ldr);
    else if (is(F, H, F)) hook_gemm_skinny<float, f16, float>(C, x, M, K, ldx, w, N, ldw, scale, shift, act, ldy, fill, y, res, ldr);
    else FE_CHECK(false, "fe_op_gemm_skinny: no kernel for element types (%d, %d, %d)", ti, tw, to);
  });
}

// Test hook of the fused head_dim-64 attention kernels, launched alone: o = softmax(q k^T) v + bv per (batch, head), q taken as the
// kernel receives it (already scaled). v is transposed on the host into the kernel's V^T layout [B][d][roundup32(Lk)], zero padded.
// form 0: the kernel of the context's precision (operands rounded on upload); form 1: the split-f16 kernel on hi | lo pairs.
int fe_op_attention(fe_ctx* ctx, const float* q, const float* k, const float* v, const float* bv, int B, int H, int Lq, int Lk, int causal,
                    int form, float* o) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(q && k && v && bv && o && B > 0 && H > 0 && Lq > 0 && Lk > 0 && (form == 0 || form == 1), "bad attention arguments");
    FE_CHECK(form == 0 || C.precision == PREC_F16, "fe_op_attention: the split form (form 1) runs on f16 pairs - set f16 precision");
    FE_CHECK(form == 0 || !causal, "fe_op_attention: the split form (form 1) has no causal mask");
    C.arena.reset();
    const int d = H * 64, Lp = (Lk + 31) / 32 * 32;
    const size_t nq = (size_t)B * Lq * d, nk = (size_t)B * Lk * d, nv = (size_t)B * d * Lp;
    std::vector<float> vt(nv, 0.f);
    for (int b = 0; b < B; ++b)
      for (int j = 0; j < Lk; ++j)
        for (int c = 0; c < d; ++c) vt[((size_t)b * d + c) * Lp + j] = v[((size_t)b * Lk + j) * d + c];
    float *dq = upload(C, q, nq), *dk = upload(C, k, nk), *dvt = upload(C, vt.data(), nv), *dbv = upload(C, bv, (size_t)d);
    if (form == 1) {
      f16* q2 = C.arena.array<f16>(2 * nq);      // rows [hi d | lo d]
      f16* k2 = C.arena.array<f16>(2 * nk);
      f16* v2 = C.arena.array<f16>(2 * nv);      // rows [hi Lp | lo Lp]: V^T hi and lo interleaved by row, row stride 2 Lp
      f16* o2 = C.arena.array<f16>(2 * nq);
      float* o32 = C.arena.array<float>(2 * nq);
      launch_split_hi_lo(dq, q2, (size_t)B * Lq, d, C.stream);
      launch_split_hi_lo(dk, k2, (size_t)B * Lk, d, C.stream);
      launch_split_hi_lo(dvt, v2, (size_t)B * d, Lp, C.stream);
      launch_attention_split(q2, k2, 2 * d, d, v2, v2 + Lp, 2 * Lp, o2, 2 * d, d, B, H, Lq, Lk, d, C.stream);
      launch_convert(o2, o32, 2 * nq, C.stream);
      std::vector<float> pair(2 * nq);
      FE_HIP(hipMemcpyAsync(pair.data(), o32, 2 * nq * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
      for (size_t row = 0; row < (size_t)B * Lq; ++row)
        for (int c = 0; c < d; ++c) o[row * d + c] = (pair[row * 2 * d + c] + pair[row * 2 * d + d + c]) + bv[c];
      return FE_OK;
    }
    auto half_op = [&](auto* tag) {
      typedef std::remove_pointer_t<decltype(tag)> E;
      E *hq = C.arena.array<E>(nq), *hk = C.arena.array<E>(nk), *hv = C.arena.array<E>(nv), *ho = C.arena.array<E>(nq);
      launch_convert(dq, hq, nq, C.stream);
      launch_convert(dk, hk, nk, C.stream);
      launch_convert(dvt, hv, nv, C.stream);
      launch_attention(hq, d, hk, d, hv, Lp, dbv, ho, d, B, H, Lq, Lk, d, causal ? 1 : 0, C.stream);
      launch_convert(ho, dq, nq, C.stream);      // dq is free again: the fp32 copy of the output
      return dq;
    };
    float* dout;
    if (C.precision == PREC_BF16) {
      dout = half_op((bf16*)nullptr);
    } else if (C.precision == PREC_F16) {
      dout = half_op((f16*)nullptr);
    } else {
      dout = C.arena.array<float>(nq);
      launch_attention(dq, d, dk, d, dvt, Lp, dbv, dout, d, B, H, Lq, Lk, d, causal ? 1 : 0, C.stream);
    }
    FE_HIP(hipMemcpyAsync(o, dout, nq * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    return FE_OK;
  });
}

// Test hook of the attention wiring (build_mha + mha_forward in engine.hip) with nn.MultiheadAttention's parameters: the q / k
// projections with the folded 1/sqrt(head_dim), the role-swapped V^T GEMM, the kernel (or the unfused route for head_dim != 64), the
// out-projection and the residual, in the context's precision.
int fe_op_mha(fe_ctx* ctx, const float* x_q, const float* x_kv, int B, int Lq, int Lk, int d, int heads, const float* in_proj_weight,
              const float* in_proj_bias, const float* out_proj_weight, const float* out_proj_bias, const float* res, int causal, float* y) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(x_q && x_kv && in_proj_weight && in_proj_bias && out_proj_weight && out_proj_bias && y && B > 0 && Lq > 0 && Lk > 0 && d > 0 && heads > 0,
             "bad mha arguments");
    C.arena.reset();
    DeviceWeights dw;
    dw.prec = C.precision;
    WeightStore ws;
    const int64_t s_in[2] = {3 * d, d}, s_out[2] = {d, d}, s_inb[1] = {3 * d}, s_outb[1] = {d};
    ws.set("a.in_proj_weight", in_proj_weight, s_in, 2);
    ws.set("a.in_proj_bias", in_proj_bias, s_inb, 1);
    ws.set("a.out_proj.weight", out_proj_weight, s_out, 2);
    ws.set("a.out_proj.bias", out_proj_bias, s_outb, 1);
    const MHAW m = build_mha(dw, ws, "a", heads);
    const size_t nq = (size_t)B * Lq * d, nk = (size_t)B * Lk * d;
    float *dq = upload(C, x_q, nq), *dkv = upload(C, x_kv, nk), *dres = upload(C, res, nq), *dy = C.arena.array<float>(nq);
    auto half_op = [&](auto* tag) {
      typedef std::remove_pointer_t<decltype(tag)> E;
      E *hq = C.arena.array<E>(nq), *hkv = C.arena.array<E>(nk), *hres = res ? C.arena.array<E>(nq) : nullptr, *hy = C.arena.array<E>(nq);
      launch_convert(dq, hq, nq, C.stream);
      launch_convert(dkv, hkv, nk, C.stream);
      if (res) launch_convert(dres, hres, nq, C.stream);
      mha_forward<E, E>(C, m, hq, d, hkv, d, B, Lq, Lk, hres, d, hy, d, causal != 0);
      launch_convert(hy, dy, nq, C.stream);
    };
    if (C.precision == PREC_BF16) half_op((bf16*)nullptr);
    else if (C.precision == PREC_F16) half_op((f16*)nullptr);
    else mha_forward<float, float>(C, m, dq, d, dkv, d, B, Lq, Lk, dres, d, dy, d, causal != 0);
    FE_HIP(hipMemcpyAsync(y, dy, nq * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

// Bring-up hook: the VLM decoder's greedy selection (vlm_select) on caller logits [rows][vocab], rounded to bf16 first as in the decoder.
// ids [rows]; logprobs [rows] (nullable: the plain kernels) the log-probability of each chosen id.
int fe_op_vlm_select(fe_ctx* ctx, const float* logits, int rows, int vocab, int32_t* ids, float* logprobs) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(logits && ids && rows > 0 && rows <= 65535 && vocab > 0, "bad arguments (1 <= rows <= 65535, vocab > 0)");
    C.arena.reset();
    float* d_lg = upload(C, logits, (size_t)rows * vocab);
    int* d_ids = (int*)C.arena.alloc((size_t)rows * sizeof(int));
    float* d_lp = logprobs ? (float*)C.arena.alloc((size_t)rows * sizeof(float)) : nullptr;
    vlm_select(C, d_lg, rows, vocab, d_ids, d_lp);
    FE_HIP(hipMemcpyAsync(ids, d_ids, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, C.stream));
    if (d_lp) FE_HIP(hipMemcpyAsync(logprobs, d_lp, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

// Test hook of the VLM decode attention (vlm_decode_attention in model_vlm.hip, with the cache built by vlm_kv_fill), launched alone.
int fe_op_vlm_decode_attention(fe_ctx* ctx, const float* q, const float* k, const float* v, int B, int nh, int nkv, int Lk, const int32_t* pad, int kv_format,
                               int len_from_device, float* out, float* k_image, float* v_image) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(q && k && v && pad && out && B > 0 && nkv > 0 && nh > 0 && nh % nkv == 0 && nh / nkv <= 8 && Lk > 0 && Lk <= 8192, "bad decode attention arguments");
    FE_CHECK(kv_format == FE_VLM_KV_BF16 || kv_format == FE_VLM_KV_E4M3 || kv_format == FE_VLM_KV_BF16_E4M3, "fe_op_vlm_decode_attention: kv format %d", kv_format);
    for (int b = 0; b < B; ++b) FE_CHECK(pad[b] >= 0 && pad[b] < Lk, "fe_op_vlm_decode_attention: pad %d of %d keys", pad[b], Lk);
    C.arena.reset();
    // graph-replay form: the grid covers a cache longer than Lk (whole chunks past the length, and one that starts inside it)
    const int max_seq = len_from_device ? Lk + 2 * 128 + 37 : Lk;
    const size_t nq = (size_t)B * nh * 128, rows = (size_t)B * nkv * Lk, nk = rows * 128, crow = (size_t)B * nkv * max_seq;
    float *dq = upload(C, q, nq), *dk = upload(C, k, nk), *dv = upload(C, v, nk);
    int* dpad = upload(C, pad, (size_t)B);
    bf16 *hq = C.arena.array<bf16>(nq), *hk = C.arena.array<bf16>(nk), *hv = C.arena.array<bf16>(nk), *ho = C.arena.array<bf16>(nq);
    launch_convert(dq, hq, nq, C.stream);
    launch_convert(dk, hk, nk, C.stream);
    launch_convert(dv, hv, nk, C.stream);
    const bool f8 = kv_format == FE_VLM_KV_E4M3;
    VlmKv kv;
    kv.format = kv_format; kv.max_seq = max_seq;
    kv.k = (bf16*)C.arena.alloc(crow * 128 * (f8 ? 1 : sizeof(bf16)));
    kv.v = (bf16*)C.arena.alloc(crow * 128 * (f8 ? 1 : sizeof(bf16)));
    if (f8) { kv.ks = C.arena.array<float>(crow); kv.vs = C.arena.array<float>(crow); }
    vlm_kv_fill(C, kv, hk, hv, B * nkv, Lk);
    int* dlen = nullptr;
    if (len_from_device) { const int last = Lk - 1; dlen = upload(C, &last, 1); FE_HIP(hipStreamSynchronize(C.stream)); }
    const int nsplit = (max_seq + 127) / 128;
    float *po = C.arena.array<float>(nq * nsplit), *pm = C.arena.array<float>((size_t)B * nh * nsplit), *pl = C.arena.array<float>((size_t)B * nh * nsplit);
    vlm_decode_attention(C, kv, hq, B, nh, nkv, Lk, dlen, dpad, po, pm, pl, nsplit, ho);
    launch_convert(ho, dq, nq, C.stream);      // dq is free again: the fp32 copy of the output
    FE_HIP(hipMemcpyAsync(out, dq, nq * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    // the cache rows as the kernel read them, dequantised on the host (fp8_core.h)
    for (int which = 0; which < 2; ++which) {
      float* img = which ? v_image : k_image;
      if (!img) continue;
      const bf16* src = which ? kv.v : kv.k;
      const size_t esz = f8 ? 1 : sizeof(uint16_t);
      std::vector<uint8_t> raw(crow * 128 * esz);
      std::vector<float> sc(f8 ? crow : 0);
      FE_HIP(hipMemcpyAsync(raw.data(), src, raw.size(), hipMemcpyDeviceToHost, C.stream));
      if (f8) FE_HIP(hipMemcpyAsync(sc.data(), which ? kv.vs : kv.ks, crow * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipStreamSynchronize(C.stream));
      for (size_t r = 0; r < rows; ++r) {
        const size_t cr = (r / Lk) * max_seq + r % Lk;
        for (int d = 0; d < 128; ++d) {
          if (f8) img[r * 128 + d] = fp8::e4m3_decode(raw[cr * 128 + d]) * sc[cr];
          else { uint16_t h; memcpy(&h, &raw[(cr * 128 + d) * 2], 2); const uint32_t u = (uint32_t)h << 16; memcpy(&img[r * 128 + d], &u, 4); }
        }
      }
    }
    return FE_OK;
  });
}

// Test hook of the VLM decode projections (vlm_linear, vlm_logits and the fused steps of vlm_forward in model_vlm.hip), launched alone on
// weights packed as build_vlm packs them. The weights live in a DeviceWeights of the call: freed when it returns, on every path.
int fe_op_vlm_linear(fe_ctx* ctx, const float* x, int M, int ldx, const float* w, const float* bias, int N, int K, int weight_format, const float* w2,
                     const float* xres, const float* g, float eps, const int32_t* slot, const float* ds, int n_ds, int route, int kernel, float* y,
                     float* y2, int32_t* info) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(x && w && y && info && M > 0 && M <= 4096 && N > 0 && K > 0 && ldx >= K && ldx % 8 == 0, "bad vlm linear arguments");
    FE_CHECK(weight_format == FE_VLM_WEIGHTS_BF16 || weight_format == FE_VLM_WEIGHTS_E4M3, "fe_op_vlm_linear: weight format %d", weight_format);
    FE_CHECK(route >= 0 && route <= 3 && kernel >= VLM_LIN_AUTO && kernel <= VLM_LIN_FORCE_GEMM32, "fe_op_vlm_linear: route %d, kernel %d", route, kernel);
    FE_CHECK(route < 2 || (!bias && N % 4 == 0 && kernel != VLM_LIN_FORCE_GEMV), "fe_op_vlm_linear: the fused routes take the GEMM, no bias and N %% 4 == 0");
    FE_CHECK(route != 2 || (xres && g && y2 && !slot == !ds && (!ds || n_ds > 0)), "fe_op_vlm_linear: route 2 takes xres, g, y2 and slot with ds");
    FE_CHECK(route != 3 || w2, "fe_op_vlm_linear: route 3 takes w2");
    if (route == 2 && slot)
      for (int m = 0; m < M; ++m) FE_CHECK(slot[m] >= -1 && slot[m] < n_ds, "fe_op_vlm_linear: slot %d of %d rows", slot[m], n_ds);
    C.arena.reset();
    DeviceWeights dw;
    dw.prec = PREC_BF16; dw.half_only = true;      // as build_vlm
    const size_t mn = (size_t)M * N;
    auto pack = [&](const float* src, const HostTensor* b) {
      HostTensor W;
      W.shape = {N, K};
      W.data.assign(src, src + (size_t)N * K);
      return vlm_pack_linear(dw, weight_format, W, b, "w");
    };
    HostTensor Bv;
    if (bias) { Bv.shape = {N}; Bv.data.assign(bias, bias + N); }
    const ConvW cw = pack(w, bias ? &Bv : nullptr);
    auto to_bf16 = [&](const float* src, size_t n) {
      float* d32 = upload(C, src, n);
      bf16* d16 = C.arena.array<bf16>(n);
      launch_convert(d32, d16, n, C.stream);
      return d16;
    };
    const bf16* hx = to_bf16(x, (size_t)M * ldx);
    float* out32 = C.arena.array<float>(mn);
    bf16* out16 = C.arena.array<bf16>(mn);
    VlmLinearInfo li;
    if (route == 0) {
      vlm_linear(C, cw, hx, ldx, M, out16, N, kernel, &li);
      launch_convert(out16, out32, mn, C.stream);
    } else if (route == 1) {
      vlm_logits(C, cw, hx, ldx, M, out32, N, kernel, &li);
    } else if (route == 2) {
      bf16* hres = to_bf16(xres, mn);
      const bf16* hg = to_bf16(g, (size_t)N);
      const bf16* hds = ds ? to_bf16(ds, (size_t)n_ds * N) : nullptr;
      const int* dslot = ds ? upload(C, slot, (size_t)M) : nullptr;
      li = VlmLinearInfo{VLM_LIN_GEMM32, 0, vlm_proj_add_rmsnorm(C, cw, hx, ldx, M, hres, hg, out16, eps, dslot, hds), 0};
      float* n32 = C.arena.array<float>(mn);
      launch_convert(out16, n32, mn, C.stream);
      launch_convert(hres, out32, mn, C.stream);
      FE_HIP(hipMemcpyAsync(y2, n32, mn * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    } else {
      const ConvW cw2 = pack(w2, nullptr);
      li = VlmLinearInfo{VLM_LIN_GEMM32, 0, vlm_gate_up_silu_mul(C, cw, cw2, hx, ldx, M, out16), 0};
      launch_convert(out16, out32, mn, C.stream);
    }
    FE_HIP(hipMemcpyAsync(y, out32, mn * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipStreamSynchronize(C.stream));
    info[0] = li.family; info[1] = li.mr; info[2] = li.splits; info[3] = li.direct;
  });
}

// ---- test hooks of the VLM decoders' row passes: each runs the launch function vlm_forward (or a vision tower) calls, alone ----------------
// n host floats -> bf16 in the arena
static bf16* vlm_hook_bf16(Ctx& C, const float* src, size_t n) {
  if (!src) return nullptr;
  float* d32 = upload(C, src, n);
  bf16* d16 = C.arena.array<bf16>(n);
  launch_convert(d32, d16, n, C.stream);
  return d16;
}
// n bf16 values in device memory -> host floats (queued on the stream; the caller synchronises)
static void vlm_hook_f32(Ctx& C, const bf16* src, size_t n, float* dst) {
  if (!dst) return;
  float* d32 = C.arena.array<float>(n);
  launch_convert(src, d32, n, C.stream);
  FE_HIP(hipMemcpyAsync(dst, d32, n * sizeof(float), hipMemcpyDeviceToHost, C.stream));
}

int fe_op_vlm_rope_cache(fe_ctx* ctx, const float* qkv, const int32_t* pos, const float* inv_freq, int family, const float* qn, const float* kn, float eps,
                         int sa, int sb, int B, int L, int nh, int nkv, int start, int start_from_device, int max_seq, int kv_format, int max_blocks, int fill,
                         float* q_out, uint8_t* k_raw, uint8_t* v_raw, float* k_scale, float* v_scale) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(qkv && pos && inv_freq && q_out && k_raw && v_raw && B > 0 && L > 0 && nh > 0 && nkv > 0 && (size_t)B * L * (nh + 2 * nkv) <= (1u << 20),
             "bad rope arguments");
    FE_CHECK(family == 0 || (family == 1 && qn && kn), "fe_op_vlm_rope_cache: family %d (0 Qwen2.5-VL, 1 Qwen3-VL with qn and kn)", family);
    FE_CHECK(kv_format == FE_VLM_KV_BF16 || kv_format == FE_VLM_KV_E4M3 || kv_format == FE_VLM_KV_BF16_E4M3, "fe_op_vlm_rope_cache: kv format %d", kv_format);
    FE_CHECK(sa >= 0 && sb >= 0 && sa + sb <= 64 && fill >= 0 && fill <= 255 && max_blocks >= 0, "fe_op_vlm_rope_cache: sections %d, %d, fill %d", sa, sb, fill);
    // (the launch function checks a start passed by value; the one the kernel reads from device memory is checked here)
    FE_CHECK(max_seq > 0 && max_seq <= 8192 && start >= 0 && start + L <= max_seq, "fe_op_vlm_rope_cache: positions %d .. %d of a cache of %d", start, start + L - 1,
             max_seq);
    const bool f8 = kv_format == FE_VLM_KV_E4M3;
    FE_CHECK(!f8 || (k_scale && v_scale), "fe_op_vlm_rope_cache: the e4m3 format returns its scales");
    C.arena.reset();
    const size_t rows = (size_t)B * L, crow = (size_t)B * nkv * max_seq, cbytes = crow * 128 * (f8 ? 1 : sizeof(bf16));
    const bf16* hqkv = vlm_hook_bf16(C, qkv, rows * (nh + 2 * nkv) * 128);
    const int* dpos = upload(C, pos, 3 * rows);
    const float* dfreq = upload(C, inv_freq, (size_t)64);
    VlmKv kv;
    kv.format = kv_format; kv.max_seq = max_seq;
    kv.k = (bf16*)C.arena.alloc(cbytes);
    kv.v = (bf16*)C.arena.alloc(cbytes);
    FE_HIP(hipMemsetAsync(kv.k, fill, cbytes, C.stream));
    FE_HIP(hipMemsetAsync(kv.v, fill, cbytes, C.stream));
    if (f8) {
      kv.ks = C.arena.array<float>(crow); kv.vs = C.arena.array<float>(crow);
      FE_HIP(hipMemsetAsync(kv.ks, fill, crow * sizeof(float), C.stream));
      FE_HIP(hipMemsetAsync(kv.vs, fill, crow * sizeof(float), C.stream));
    }
    bf16* hq = C.arena.array<bf16>(rows * nh * 128);
    VlmRope r;
    r.qwen3 = family == 1;
    r.qn = vlm_hook_bf16(C, r.qwen3 ? qn : nullptr, 128); r.kn = vlm_hook_bf16(C, r.qwen3 ? kn : nullptr, 128); r.eps = eps;
    if (r.qwen3) { r.s1 = sa; r.s2 = sb; } else { r.s0 = sa; r.s1 = sb; r.s2 = 64 - sa - sb; }
    r.B = B; r.L = L; r.nh = nh; r.nkv = nkv; r.max_blocks = max_blocks;
    if (start_from_device) { r.start = 0; r.start_dev = upload(C, &start, 1); FE_HIP(hipStreamSynchronize(C.stream)); }
    else r.start = start;
    vlm_rope_cache(C, r, kv, hqkv, dpos, dfreq, hq);
    vlm_hook_f32(C, hq, rows * nh * 128, q_out);
    FE_HIP(hipMemcpyAsync(k_raw, kv.k, cbytes, hipMemcpyDeviceToHost, C.stream));
    FE_HIP(hipMemcpyAsync(v_raw, kv.v, cbytes, hipMemcpyDeviceToHost, C.stream));
    if (f8) {
      FE_HIP(hipMemcpyAsync(k_scale, kv.ks, crow * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      FE_HIP(hipMemcpyAsync(v_scale, kv.vs, crow * sizeof(float), hipMemcpyDeviceToHost, C.stream));
    }
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

int fe_op_vlm_rows(fe_ctx* ctx, int route, const float* x, const float* y, const float* w, const int32_t* slot, const float* ds, int n_ds, int rows, int d,
                   int ldx, int ldy, float eps, int alias, int max_blocks, float* out_x, float* out_n) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    enum { RMSNORM = 0, ADD = 1, ADD_NORM = 2, ADD_NORM_NO_W = 3, ADD_NORM_DS = 4, FEW_ROWS = 5, SILU_MUL = 6 };
    FE_CHECK(route >= RMSNORM && route <= SILU_MUL && x && rows > 0 && rows <= 65536 && d > 0 && d <= 65536 && d % 4 == 0 && max_blocks >= 0, "bad vlm rows arguments");
    FE_CHECK(route == RMSNORM ? (ldx >= d && ldy >= d && ldx <= 2 * d + 64 && ldy <= 2 * d + 64) : (ldx == d && ldy == d), "fe_op_vlm_rows: strides %d, %d of %d values", ldx,
             ldy, d);
    const bool takes_y = route != RMSNORM && route != FEW_ROWS, takes_w = route == RMSNORM || route == ADD_NORM || route == ADD_NORM_DS || route == FEW_ROWS;
    const bool gives_x = route != RMSNORM;
    FE_CHECK(!takes_y == !y && !takes_w == !w && !gives_x == !out_x && !takes_w == !out_n, "fe_op_vlm_rows: route %d takes other operands", route);
    FE_CHECK(route == ADD_NORM_DS ? (slot && ds && n_ds > 0) : (!slot && !ds), "fe_op_vlm_rows: slot and ds belong to route %d", (int)ADD_NORM_DS);
    if (route == ADD_NORM_DS)
      for (int m = 0; m < rows; ++m) FE_CHECK(slot[m] >= -1 && slot[m] < n_ds, "fe_op_vlm_rows: slot %d of %d rows", slot[m], n_ds);
    FE_CHECK(route != FEW_ROWS || rows <= 64, "fe_op_vlm_rows: the few-rows form takes up to 64 rows");
    C.arena.reset();
    const size_t n = (size_t)rows * d;
    bf16* hx = vlm_hook_bf16(C, x, (size_t)rows * ldx);
    const bf16* hy = vlm_hook_bf16(C, y, n);
    const bf16* hw = vlm_hook_bf16(C, w, (size_t)d);
    const bf16* hds = vlm_hook_bf16(C, ds, (size_t)(ds ? n_ds : 0) * d);
    const int* dslot = slot ? upload(C, slot, (size_t)rows) : nullptr;
    bf16* hn = nullptr;
    if (takes_w) {      // the columns past d of a padded output keep the fill
      const size_t no = (size_t)rows * ldy;
      std::vector<float> pad(no, 768.f);      // (a bf16 value)
      hn = vlm_hook_bf16(C, pad.data(), no);
      FE_HIP(hipStreamSynchronize(C.stream));      // (pad dies with this block)
    }
    const bf16* hout = hx;
    if (route == RMSNORM) vlm_rmsnorm(C, hx, ldx, hw, hn, ldy, rows, d, eps, max_blocks);
    else if (route == ADD) vlm_add(C, hx, hy, n, max_blocks);
    else if (route == FEW_ROWS) vlm_few_rows_rmsnorm(C, hx, hw, hn, rows, d, eps);
    else if (route == SILU_MUL) {
      bf16* hh = alias ? hx : C.arena.array<bf16>(n);
      vlm_silu_mul(C, hx, hy, hh, n, max_blocks);
      hout = hh;
    } else vlm_add_rmsnorm(C, hx, hy, hw, hn, rows, d, eps, dslot, hds, max_blocks);
    if (gives_x) vlm_hook_f32(C, hout, n, out_x);
    if (takes_w) vlm_hook_f32(C, hn, (size_t)rows * ldy, out_n);
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

int fe_op_vlm_vis_rope(fe_ctx* ctx, const float* qkv, const int32_t* pos, const float* inv_freq, int hd, int rows, int heads, int max_blocks, float* q_out,
                       float* k_out) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(qkv && pos && inv_freq && q_out && k_out && (hd == 64 || hd == 80) && rows > 0 && rows <= 65536 && heads > 0 && heads <= 64 && max_blocks >= 0,
             "bad vision rope arguments (hd 64 or 80)");
    C.arena.reset();
    const size_t n = (size_t)rows * heads * hd;
    const bf16* hqkv = vlm_hook_bf16(C, qkv, 3 * n);
    const int* dpos = upload(C, pos, (size_t)2 * rows);
    const float* dfreq = upload(C, inv_freq, (size_t)(hd / 4));
    bf16 *hq = C.arena.array<bf16>(n), *hk = C.arena.array<bf16>(n);
    vlm_vis_rope(C, hd, hqkv, dpos, dfreq, hq, hk, rows, heads, max_blocks);
    vlm_hook_f32(C, hq, n, q_out);
    vlm_hook_f32(C, hk, n, k_out);
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

// ---- test hooks of the attention tile (vlm_attn_tile.h) under its two kernels, each through the one function that launches it ---------------
// n bf16 values in the arena, all 768 (a bf16 value): a row the kernel leaves unwritten shows
static bf16* vlm_hook_768(Ctx& C, size_t n) {
  const std::vector<float> fill(n, 768.f);
  bf16* d = vlm_hook_bf16(C, fill.data(), n);
  FE_HIP(hipStreamSynchronize(C.stream));      // (fill dies here)
  return d;
}

int fe_op_vlm_vis_attention(fe_ctx* ctx, const float* q, const float* k, const float* v, const int32_t* cu, int n_seg, int max_seg, int hd, int heads, float* o) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(q && k && v && cu && o && (hd == 64 || hd == 80) && heads >= 1 && heads <= 64 && n_seg >= 1 && n_seg <= 65535,
             "bad vision attention arguments (hd 64 or 80, 1 .. 64 heads, 1 .. 65535 segments)");
    FE_CHECK(cu[0] == 0, "fe_op_vlm_vis_attention: cu[0] = %d (0)", cu[0]);
    int longest = 0;
    for (int s = 0; s < n_seg; ++s) {
      FE_CHECK(cu[s + 1] > cu[s] && cu[s + 1] <= 65536, "fe_op_vlm_vis_attention: segment %d is rows %d .. %d (at least one row, 65536 in all)", s, cu[s], cu[s + 1]);
      longest = std::max(longest, cu[s + 1] - cu[s]);
    }
    FE_CHECK(max_seg == longest, "fe_op_vlm_vis_attention: max_seg %d, the longest segment has %d rows", max_seg, longest);
    C.arena.reset();
    const size_t N = (size_t)cu[n_seg], d = (size_t)heads * hd, n = N * d;
    const bf16* hq = vlm_hook_bf16(C, q, n);
    const bf16* hk = vlm_hook_bf16(C, k, n);
    // the fused projection rows: v in the last third, a large finite value in the q and k thirds (a read from the wrong third is gross)
    std::vector<float> fused(3 * n, 1.0e4f);
    for (size_t r = 0; r < N; ++r) memcpy(&fused[r * 3 * d + 2 * d], v + r * d, d * sizeof(float));
    const bf16* hqkv = vlm_hook_bf16(C, fused.data(), 3 * n);
    const int* dcu = upload(C, cu, (size_t)n_seg + 1);
    bf16* ho = vlm_hook_768(C, n);
    vlm_vis_attention(C, hd, hq, hk, hqkv, ho, dcu, n_seg, max_seg, heads);
    vlm_hook_f32(C, ho, n, o);
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

int fe_op_vlm_prefill_attention(fe_ctx* ctx, const float* q, const float* k, const float* v, int B, int nh, int nkv, int Lq, int qpos0, int max_seq, const int32_t* pad,
                                float* o) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    FE_CHECK(q && k && v && pad && o && B > 0 && nh > 0 && nkv > 0 && nh % nkv == 0 && (size_t)B * nh <= 65535, "bad prefill attention arguments (nh %% nkv == 0, B nh <= 65535)");
    FE_CHECK(Lq >= 1 && qpos0 >= 0 && qpos0 <= 8192 && Lq <= 8192 && qpos0 + Lq <= max_seq && max_seq <= 8192,
             "fe_op_vlm_prefill_attention: %d queries from position %d in a cache of %d rows (8192 at most)", Lq, qpos0, max_seq);
    const int Lk = qpos0 + Lq;
    for (int b = 0; b < B; ++b) FE_CHECK(pad[b] >= 0 && pad[b] < Lk, "fe_op_vlm_prefill_attention: pad %d of %d keys", pad[b], Lk);
    C.arena.reset();
    const size_t nq = (size_t)B * Lq * nh * 128, nk = (size_t)B * nkv * Lk * 128, cbytes = (size_t)B * nkv * max_seq * 128 * sizeof(bf16);
    const bf16* hq = vlm_hook_bf16(C, q, nq);
    const bf16* hk = vlm_hook_bf16(C, k, nk);
    const bf16* hv = vlm_hook_bf16(C, v, nk);
    const int* dpad = upload(C, pad, (size_t)B);
    // the caches: rows Lk .. max_seq - 1 hold bf16 NaNs (the kernel clamps its loads to row Lk - 1: they must never reach a result)
    VlmKv kv;
    kv.format = FE_VLM_KV_BF16; kv.max_seq = max_seq;
    kv.k = (bf16*)C.arena.alloc(cbytes);
    kv.v = (bf16*)C.arena.alloc(cbytes);
    FE_HIP(hipMemsetAsync(kv.k, 0xFF, cbytes, C.stream));
    FE_HIP(hipMemsetAsync(kv.v, 0xFF, cbytes, C.stream));
    vlm_kv_fill(C, kv, hk, hv, B * nkv, Lk);
    bf16* ho = vlm_hook_768(C, nq);
    vlm_prefill_attention(C, hq, kv.k, kv.v, max_seq, B, nh, nkv, Lq, Lk, qpos0, dpad, ho);
    vlm_hook_f32(C, ho, nq, o);
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}

}  // extern "C"
