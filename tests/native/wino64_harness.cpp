// CPU model of facet_amd/csrc/kernels_wino64.hip (built with -fsanitize=address,undefined by tests/test_wino64_host.py): the kernel's
// algorithm as loops over workgroups, waves and lanes, on the index maps, transforms and U packing of wino64_maps.h - the same header
// the device code is compiled from - against a plain direct convolution. Inputs are small integers, so every product and sum of the
// Winograd form is exact in fp32 (U holds quarters of integers, V integer sums) and the two results must be EQUAL.
//
//   wino64_harness N Cin Cout H W     exit status 0: equal; 1: differences (the first few are printed)
#include "wino64_maps.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fe::w64;

// the kernel: x [N][H][W][cinp] (cinp = Cin rounded up to 4, zero channels behind Cin), U from pack_u, y [N][H][W][Cout]
static void kernel_model(const std::vector<float>& x, int N, int H, int W, int cinp, const std::vector<float>& U, int Cout, std::vector<float>& y) {
  const int bx = (W + BLOCK - 1) / BLOCK, by = (H + BLOCK - 1) / BLOCK, nblocks = N * bx * by;
  std::vector<float> lds(2 * CHUNK_UNITS * 2);
  std::vector<float> acc(4 * 64 * 16 * 16);      // [wave][lane][plane][e]
  std::vector<float> A(16 * 64), B(16 * 64);     // one matrix instruction's operands: [plane][lane]
  for (int v = 0; v < nblocks; ++v) {
    const int b = v / (bx * by), rem = v - b * (bx * by), y0 = rem / bx * BLOCK, x0 = rem % bx * BLOCK;
    std::fill(acc.begin(), acc.end(), 0.f);
    for (int c = 0; c < NCHUNK; ++c) {
      float* const buf = lds.data() + (c & 1) * CHUNK_UNITS * 2;
      for (int t = 0; t < 256; ++t)      // staging: thread t, piece i
        for (int i = 0; i < PIECES_PER_THREAD; ++i) {
          const int idx = t + 256 * i, pixel = idx / PARTS, part = idx % PARTS;
          if (idx >= PIECES) continue;
          const int py = pixel / PATCH, px = pixel - py * PATCH, gy = y0 - 1 + py, gx = x0 - 1 + px, ch = c * CHUNK_CH + part * 4;
          const bool in = ch < cinp && gy >= 0 && gy < H && gx >= 0 && gx < W;
          float q[4] = {0.f, 0.f, 0.f, 0.f};
          if (in)
            for (int e = 0; e < 4; ++e) q[e] = x[(((size_t)b * H + gy) * W + gx) * cinp + ch + e];
          const int dst = 2 * patch_unit(2 * part, py, px);
          buf[dst] = q[0]; buf[dst + 1] = q[1];
          buf[dst + 2 * PAIR_UNITS] = q[2]; buf[dst + 2 * PAIR_UNITS + 1] = q[3];
        }
      for (int wave = 0; wave < 4; ++wave) {
        const int tg = wave & 1, half = wave >> 1;
        for (int s = 0; s < STEPS_PER_CHUNK; ++s) {
          const int step = c * STEPS_PER_CHUNK + s, j = s >> 1, s2 = s & 1;
          for (int lane = 0; lane < 64; ++lane) {
            const int tl = lane & 31, kk = lane >> 5, ty = tile_y(tg, tl), tx = tile_x(tl);
            const int lane_unit = patch_unit(kk, 2 * ty, 2 * tx);
            float d[16], vv[16];
            for (int dy = 0; dy < 4; ++dy)
              for (int dx = 0; dx < 4; ++dx)
                d[4 * dy + dx] = buf[2 * (lane_unit + 2 * j * PAIR_UNITS + dy * ROW_UNITS + (dx & 1) * (ROW_UNITS / 2) + (dx >> 1)) + s2];
            input_transform(d, vv);
            for (int pl = 0; pl < 16; ++pl) {
              B[pl * 64 + lane] = vv[pl];
              A[pl * 64 + lane] = U[u_index(step, half, pl >> 2, lane, pl & 3)];
            }
          }
          // v_mfma_f32_32x32x2_f32 per plane: D[i][j] += sum_k A[i][k] B[k][j]; lane L gives A[L % 32][L / 32] and B[L / 32][L % 32] and
          // holds D[acc_channel(0, L, e)][L % 32]
          for (int pl = 0; pl < 16; ++pl)
            for (int lane = 0; lane < 64; ++lane)
              for (int e = 0; e < 16; ++e) {
                const int row = acc_channel(0, lane, e), col = lane & 31;
                float& a = acc[((wave * 64 + lane) * 16 + pl) * 16 + e];
                for (int k = 0; k < 2; ++k) a += A[pl * 64 + row + 32 * k] * B[pl * 64 + col + 32 * k];
              }
        }
      }
    }
    for (int wave = 0; wave < 4; ++wave)
      for (int lane = 0; lane < 64; ++lane) {
        const int tg = wave & 1, half = wave >> 1, tl = lane & 31, oy = y0 + 2 * tile_y(tg, tl), ox = x0 + 2 * tile_x(tl);
        for (int e = 0; e < 16; ++e) {
          const int co = acc_channel(half, lane, e);
          if (co >= Cout) continue;
          float m[16], yq[4];
          for (int pl = 0; pl < 16; ++pl) m[pl] = acc[((wave * 64 + lane) * 16 + pl) * 16 + e];
          output_transform(m, yq);
          for (int i = 0; i < 4; ++i) {
            const int yy = oy + (i >> 1), xx = ox + (i & 1);
            if (yy < H && xx < W) y[(((size_t)b * H + yy) * W + xx) * Cout + co] = yq[i];
          }
        }
      }
  }
}

int main(int argc, char** argv) {
  if (argc != 6) { fprintf(stderr, "usage: wino64_harness N Cin Cout H W\n"); return 2; }
  const int N = atoi(argv[1]), Cin = atoi(argv[2]), Cout = atoi(argv[3]), H = atoi(argv[4]), W = atoi(argv[5]);
  if (N < 1 || Cin < 1 || Cin > 64 || Cout < 1 || Cout > 64 || Cout % 4 || H < 1 || W < 1) { fprintf(stderr, "bad shape\n"); return 2; }
  const int cinp = (Cin + 3) & ~3;
  uint32_t seed = 12345u + (uint32_t)(N * 7 + Cin * 131 + Cout * 17 + H * 1009 + W * 31);
  auto rnd = [&](int lo, int hi) { seed = seed * 1664525u + 1013904223u; return (float)(lo + (int)((seed >> 8) % (uint32_t)(hi - lo + 1))); };
  std::vector<float> x((size_t)N * H * W * cinp, 0.f), w((size_t)Cout * Cin * 9), y((size_t)N * H * W * Cout, -12345.f), ref((size_t)N * H * W * Cout);
  for (size_t px = 0; px < (size_t)N * H * W; ++px)
    for (int ci = 0; ci < Cin; ++ci) x[px * cinp + ci] = rnd(-3, 3);
  for (auto& e : w) e = rnd(-2, 2);
  std::vector<float> U(U_FLOATS);
  pack_u(w.data(), Cout, Cin, U.data());
  kernel_model(x, N, H, W, cinp, U, Cout, y);
  for (int b = 0; b < N; ++b)
    for (int oy = 0; oy < H; ++oy)
      for (int ox = 0; ox < W; ++ox)
        for (int co = 0; co < Cout; ++co) {
          float a = 0.f;
          for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
              const int iy = oy - 1 + ky, ix = ox - 1 + kx;
              if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
              for (int ci = 0; ci < Cin; ++ci) a += x[(((size_t)b * H + iy) * W + ix) * cinp + ci] * w[((size_t)co * Cin + ci) * 9 + ky * 3 + kx];
            }
          ref[(((size_t)b * H + oy) * W + ox) * Cout + co] = a;
        }
  size_t bad = 0;
  for (size_t i = 0; i < ref.size(); ++i)
    if (y[i] != ref[i] && bad++ < 8) fprintf(stderr, "at %zu: kernel model %g, direct %g\n", i, y[i], ref[i]);
  printf("%zu values, %zu differ\n", ref.size(), bad);
  return bad ? 1 : 0;
}
