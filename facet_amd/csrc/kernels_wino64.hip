// fp32 3x3 convolution, stride 1, padding 1, up to 64 input and 64 output channels, as Winograd F(2x2,3x3) in ONE launch: neither the
// transformed input V nor the products M reach HBM. The three-launch Winograd forms (kernels_winograd.hip) are HBM-bound on their plane
// buffers at K = 64, so these layers ran on the direct implicit-GEMM kernel (36 multiplies per output where this kernel issues 16).
//
// Index maps, transforms and the U packing: wino64_maps.h (shared with the host model in tests/test_wino64_host.py).
//   * transposed products (A = U, B = V) on v_mfma_f32_32x32x2_f32: a lane owns ONE tile and 16 output channels in every plane;
//   * a wave holds all 16 planes of its 32 tiles x 32 channels as accumulators (256 registers, one wave per SIMD);
//   * input transform in-lane: a lane reads the 4 x 4 patch of its tile for its channel pair from the LDS patch (16 8-byte reads per two
//     K-steps), forms the 16 plane values with adds, and issues 16 matrix instructions per K-step into 16 independent accumulators;
//   * output transform in-lane, then scale / shift / residual / ReLU, PReLU or GELU (fe_apply_act, as the direct kernel) and 16-byte stores;
//   * persistent workgroups, one per CU; the K loop runs in stages of 8 input channels (4 K-steps). A stage's patch chunk (11.5 KB) sits
//     in LDS, double buffered: the next one - of this block or the next block - is fetched into registers under the current stage's
//     matrix instructions and stored behind them;
//   * U (262 KB per layer, prepared at pack time, L2 resident, shared by all workgroups) goes straight to registers as four coalesced
//     16-byte loads per K-step, a whole stage ahead of its use. (One K-step ahead, its latency under 256 CUs was longer than the step and
//     the kernel ran at a quarter of the pipe; staged through LDS, the LDS traffic of 4 waves held it at 0.4: profiles/wino64_perf.txt.)
#include "fe_common.h"
#include "wino64_maps.h"

namespace fe {

struct W64Params {
  const float* x; int ldx, cin;       // [N][H][W][ldx], cin <= 64 channels read per pixel (cin % 4 == 0)
  int N, H, W;
  float* y; int ldy, cout;            // [N][H][W][ldy], cout <= 64, cout % 4 == 0
  const float* U;                     // w64::pack_u
  const float *scale, *shift, *slope; // nullable
  const float* res; int ldr;          // nullable
  int res_after_act;
  int bx, by, nblocks;                // blocks of 16 x 16 output pixels per image row / column, in all
};

constexpr int W64_PATCH_FLOATS = w64::CHUNK_UNITS * 2;

// A: the activation - ACT_NONE, ACT_RELU, ACT_PRELU or ACT_GELU. With one wave per SIMD nothing hides the epilogue's vector work behind another
// wave's matrix instructions. ocml's erff or an exp with its division per output (GELU, sigmoid) made the kernel slower than the direct one, so
// conv_forward keeps those there; with the branch-free fe_erf (erf_core.h) the GELU form is the faster one on large maps, and the TOPIQ fp32 head
// calls it for its 64 -> 64 layers (conv_wino64, engine.hip; profiles/erf_gelu_perf.txt).
template <int A>
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) void wino64_kernel(const W64Params p) {
  using namespace w64;
  __shared__ __attribute__((aligned(16))) float sP[2 * W64_PATCH_FLOATS];      // two stages of the patch chunk
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int tg = wave & 1, half = wave >> 1;
  const int tl = lane & 31, kk = lane >> 5;
  const int ty = tile_y(tg, tl), tx = tile_x(tl);
  constexpr int act = A;

  // the thread's pieces of a patch chunk (16 bytes = 4 channels of one patch pixel)
  int pc_py[PIECES_PER_THREAD], pc_px[PIECES_PER_THREAD], pc_dst[PIECES_PER_THREAD];
#pragma unroll
  for (int i = 0; i < PIECES_PER_THREAD; ++i) {
    const int idx = t + 256 * i, pixel = idx / PARTS, part = idx % PARTS;
    pc_py[i] = pixel / PATCH; pc_px[i] = pixel - pc_py[i] * PATCH;
    pc_dst[i] = idx < PIECES ? 2 * patch_unit(2 * part, pc_py[i], pc_px[i]) : -1;
  }
  const int part4 = (t % PARTS) * 4;
  auto block_origin = [&](const int v, int& b, int& y0, int& x0) {
    const int per = p.bx * p.by;
    b = v / per;
    const int rem = v - b * per, byi = rem / p.bx;
    y0 = byi * BLOCK; x0 = (rem - byi * p.bx) * BLOCK;
  };
  // A stage = chunk c of block v: 8 input channels of the 18 x 18 patch (zeros outside the image and past cin) and the 4 K-steps of U
  // that multiply them. Fetched into registers under the matrix instructions of the stage before, stored to LDS behind them.
  // The patch pieces come through buffer loads on a descriptor of the block's image: an offset past its end (pieces outside the image,
  // channels past cin, blocks past the last one) returns zeros, so nothing selects on - and waits for - a loaded value before the store.
  fe_v4f pf[PIECES_PER_THREAD];
  typedef unsigned w64_v4u __attribute__((ext_vector_type(4)));
  constexpr unsigned OOB = 0xFFFFFFF0u;      // as conv_bf16_kernel.h: 16-byte aligned, offset + 16 does not wrap
  const unsigned img_bytes = (unsigned)p.H * (unsigned)p.W * (unsigned)p.ldx * 4u;      // < 2^32: checked by the launcher
  auto fetch_stage = [&](const int v, const int c) __attribute__((always_inline)) {
    const bool live = v < p.nblocks;
    int b, y0, x0;
    block_origin(live ? v : 0, b, y0, x0);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x + (size_t)b * p.H * p.W * p.ldx), 0, (int)img_bytes, 0x00020000);
    const bool ch_in = live && c * CHUNK_CH + part4 < p.cin;
#pragma unroll
    for (int i = 0; i < PIECES_PER_THREAD; ++i) {
      const int gy = y0 - 1 + pc_py[i], gx = x0 - 1 + pc_px[i];
      const bool in = pc_dst[i] >= 0 && ch_in && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
      const unsigned off = in ? ((unsigned)(gy * p.W + gx) * (unsigned)p.ldx + (unsigned)(c * CHUNK_CH + part4)) * 4u : OOB;
      pf[i] = __builtin_bit_cast(fe_v4f, (w64_v4u)__builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
    }
  };
  auto store_stage = [&](const int buf) __attribute__((always_inline)) {
    float* const pd = sP + buf * W64_PATCH_FLOATS;
#pragma unroll
    for (int i = 0; i < PIECES_PER_THREAD; ++i)
      if (pc_dst[i] >= 0) {
        *reinterpret_cast<float2*>(pd + pc_dst[i]) = make_float2(pf[i].x, pf[i].y);
        *reinterpret_cast<float2*>(pd + pc_dst[i] + 2 * PAIR_UNITS) = make_float2(pf[i].z, pf[i].w);
      }
  };

  // The lane's U fragments of one stage: [K-step][plane quad], four coalesced 16-byte loads per K-step (1 KB per wave and quad). The
  // registers of a K-step are reloaded with the same step of the NEXT stage as soon as its matrix instructions are issued, so a load has
  // a whole stage to come back from L2.
  const float* const ubase = p.U + u_index(0, half, 0, lane, 0);
  fe_v4f ua[STEPS_PER_CHUNK][4];
  auto fetch_u = [&](const int step, fe_v4f (&u)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = *reinterpret_cast<const fe_v4f*>(ubase + step * U_STEP_FLOATS + q * 256);
  };
#pragma unroll
  for (int s0 = 0; s0 < STEPS_PER_CHUNK; ++s0) fetch_u(s0, ua[s0]);
  fetch_stage(blockIdx.x, 0);
  store_stage(0);
  __syncthreads();

  const int lane_unit = patch_unit(kk, 2 * ty, 2 * tx);      // 2 tx is even: + (dx & 1) * 10 + (dx >> 1) below stays exact
  for (int v = blockIdx.x; v < p.nblocks; v += gridDim.x) {
    fe_f32x16 acc[16];
#pragma unroll
    for (int pl = 0; pl < 16; ++pl)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[pl][e] = 0.f;

#pragma unroll 1
    for (int c = 0; c < NCHUNK; ++c) {
      if (c + 1 < NCHUNK) fetch_stage(v, c + 1);
      else fetch_stage(v + (int)gridDim.x, 0);
      const float* const buf = sP + (c & 1) * W64_PATCH_FLOATS + 2 * lane_unit;
      // the patch reads of a step pair run one pair ahead of the matrix instructions that use them (the scheduling barrier keeps them
      // there: placed next to their use, every read's latency stood between two matrix instructions)
      float2 dq[2][16];
      auto read_pair = [&](const int j, float2 (&d)[16]) __attribute__((always_inline)) {
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
          for (int dx = 0; dx < 4; ++dx)
            d[4 * dy + dx] = *reinterpret_cast<const float2*>(buf + 2 * (2 * j * PAIR_UNITS + dy * ROW_UNITS + (dx & 1) * (ROW_UNITS / 2) + (dx >> 1)));
      };
      const int nstage = ((c + 1) & (NCHUNK - 1)) * STEPS_PER_CHUNK;      // behind the last stage: stage 0 of the next block
      read_pair(0, dq[0]);
#pragma unroll
      for (int j = 0; j < STEPS_PER_CHUNK / 2; ++j) {
        if (j + 1 < STEPS_PER_CHUNK / 2) read_pair(j + 1, dq[(j + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          float d[16], vv[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) d[i] = s2 ? dq[j & 1][i].y : dq[j & 1][i].x;
          input_transform(d, vv);
#pragma unroll
          for (int pl = 0; pl < 16; ++pl) acc[pl] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[2 * j + s2][pl >> 2][pl & 3], vv[pl], acc[pl], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          fetch_u(nstage + 2 * j + s2, ua[2 * j + s2]);
        }
      }
      store_stage((c + 1) & 1);      // free since the barrier that ended stage c - 1
      __syncthreads();
    }

    // ---- output transform + epilogue: the lane's tile (2 x 2 pixels) x 16 channels --------------------------------------------------------
    int b, y0, x0;
    block_origin(v, b, y0, x0);
    const int oy = y0 + 2 * ty, ox = x0 + 2 * tx;
    size_t pix[4]; bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int yy = oy + (i >> 1), xx = ox + (i & 1);
      ok[i] = yy < p.H && xx < p.W;
      pix[i] = ok[i] ? ((size_t)b * p.H + yy) * p.W + xx : 0;
    }
    float4 scv[4], sfv[4], slv[4];      // requested together: one load latency per block, not one per channel group
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cb = acc_channel(half, lane, 4 * g), cl = cb < p.cout ? cb : 0;
      scv[g] = p.scale ? *reinterpret_cast<const float4*>(p.scale + cl) : make_float4(1.f, 1.f, 1.f, 1.f);
      sfv[g] = p.shift ? *reinterpret_cast<const float4*>(p.shift + cl) : make_float4(0.f, 0.f, 0.f, 0.f);
      slv[g] = act == ACT_PRELU ? *reinterpret_cast<const float4*>(p.slope + cl) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cb = acc_channel(half, lane, 4 * g);
      if (cb >= p.cout) continue;
      float o[4][4];      // [pixel][channel]
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float m[16], yq[4];
#pragma unroll
        for (int pl = 0; pl < 16; ++pl) m[pl] = acc[pl][4 * g + e];
        output_transform(m, yq);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i][e] = yq[i];
      }
      const float4 sc = scv[g], sf = sfv[g], sl = slv[g];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!ok[i]) continue;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.res) r = *reinterpret_cast<const float4*>(p.res + pix[i] * p.ldr + cb);
        float4 q;
        q.x = o[i][0] * sc.x + sf.x; q.y = o[i][1] * sc.y + sf.y; q.z = o[i][2] * sc.z + sf.z; q.w = o[i][3] * sc.w + sf.w;
        if (p.res && !p.res_after_act) { q.x += r.x; q.y += r.y; q.z += r.z; q.w += r.w; }
        if (act == ACT_PRELU) {
          q.x = q.x > 0.f ? q.x : q.x * sl.x; q.y = q.y > 0.f ? q.y : q.y * sl.y;
          q.z = q.z > 0.f ? q.z : q.z * sl.z; q.w = q.w > 0.f ? q.w : q.w * sl.w;
        } else {
          q.x = fe_apply_act(q.x, act); q.y = fe_apply_act(q.y, act); q.z = fe_apply_act(q.z, act); q.w = fe_apply_act(q.w, act);
        }
        if (p.res && p.res_after_act) { q.x += r.x; q.y += r.y; q.z += r.z; q.w += r.w; }
        *reinterpret_cast<float4*>(p.y + pix[i] * p.ldy + cb) = q;
      }
    }
  }
}

void launch_wino64(const Tensor& x, const Tensor& y, const float* U, const float* scale, const float* shift, const float* slope, int act,
                   const Tensor* res, int res_after_act, hipStream_t s) {
  FE_CHECK(x.c > 0 && x.c <= 64 && x.c % 4 == 0 && y.c > 0 && y.c <= 64 && y.c % 4 == 0 && y.n == x.n && y.h == x.h && y.w == x.w, "wino64: %dx%dx%d -> %dx%dx%d", x.h,
           x.w, x.c, y.h, y.w, y.c);
  FE_CHECK(x.ld % 4 == 0 && y.ld % 4 == 0 && (((uintptr_t)x.p | (uintptr_t)y.p | (uintptr_t)U) & 15) == 0, "wino64: operands must be 16-byte aligned");
  FE_CHECK(!res || (res->ld % 4 == 0 && ((uintptr_t)res->p & 15) == 0 && res->c == y.c && res->pixels() == y.pixels()), "wino64: residual view");
  FE_CHECK(act == ACT_NONE || act == ACT_RELU || act == ACT_GELU || (act == ACT_PRELU && slope), "wino64: activation %d (PReLU needs slopes)", act);
  FE_CHECK((unsigned long long)x.h * x.w * x.ld * 4ull < 0xF0000000ull, "wino64: one image must stay below 4 GiB (32-bit buffer offsets)");
  W64Params p{};
  p.x = x.p; p.ldx = x.ld; p.cin = x.c; p.N = x.n; p.H = x.h; p.W = x.w;
  p.y = y.p; p.ldy = y.ld; p.cout = y.c;
  p.U = U; p.scale = scale; p.shift = shift; p.slope = slope;
  p.res = res ? res->p : nullptr; p.ldr = res ? res->ld : 0;
  p.res_after_act = res_after_act;
  p.bx = (x.w + w64::BLOCK - 1) / w64::BLOCK; p.by = (x.h + w64::BLOCK - 1) / w64::BLOCK;
  const long long nb = (long long)x.n * p.bx * p.by;
  FE_CHECK(nb < (1ll << 30), "wino64: too many blocks");
  p.nblocks = (int)nb;
  const int grid = p.nblocks < 256 ? p.nblocks : 256;      // one workgroup per CU
  if (act == ACT_NONE) hipLaunchKernelGGL(wino64_kernel<ACT_NONE>, dim3(grid), dim3(256), 0, s, p);
  else if (act == ACT_RELU) hipLaunchKernelGGL(wino64_kernel<ACT_RELU>, dim3(grid), dim3(256), 0, s, p);
  else if (act == ACT_GELU) hipLaunchKernelGGL(wino64_kernel<ACT_GELU>, dim3(grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(wino64_kernel<ACT_PRELU>, dim3(grid), dim3(256), 0, s, p);
  FE_HIP(hipGetLastError());
}

}  // namespace fe
