// Index maps, transforms and weight packing of the in-register Winograd F(2x2,3x3) kernel (kernels_wino64.hip), shared by the device
// code, the host packing in engine.hip and the stand-alone host model of the kernel in tests/test_wino64_host.py. Plain C++: no HIP
// headers, so the host model compiles with any compiler under sanitizers.
//
// One workgroup (4 waves) computes a block of 16 x 16 output pixels = 8 x 8 tiles of 2 x 2 for 64 output channels. Wave w owns tile
// rows 4 (w & 1) .. + 4 (32 tiles) and output channels 32 (w >> 1) .. + 32. Per K-step one v_mfma_f32_32x32x2_f32 per Winograd plane:
//   A (one float per lane) = U[plane][row = lane % 32 of the wave's channel half][k = lane / 32]
//   B (one float per lane) = V[plane][k = lane / 32][tile = lane % 32]
//   D (16 floats per lane) = M[plane][channel = w64_acc_channel(e)][tile = lane % 32]
// The 64 input channels are walked in 8 chunks of 8 (the unit the input patch is staged in), 4 K-steps per chunk.
#pragma once

#if defined(__HIPCC__)
#define W64_HD __host__ __device__ __forceinline__
#else
#define W64_HD inline
#endif

namespace fe {
namespace w64 {

constexpr int BLOCK = 16;                    // output pixels per block side
constexpr int PATCH = BLOCK + 2;             // input patch side (halo of 1)
constexpr int CHUNK_CH = 8;                  // input channels per staged chunk
constexpr int NCHUNK = 64 / CHUNK_CH;
constexpr int STEPS_PER_CHUNK = CHUNK_CH / 2;
constexpr int NSTEPS = NCHUNK * STEPS_PER_CHUNK;
// LDS image of one chunk, in 8-byte units (a channel pair of one pixel): [pair 4][patch row 18][column parity 2][10]. Splitting the
// columns by parity makes the 32 tiles of a wave (column step 2, row step 2) hit 32 different 8-byte bank pairs.
constexpr int ROW_UNITS = 20;
constexpr int PAIR_UNITS = PATCH * ROW_UNITS;              // 360
constexpr int CHUNK_UNITS = (CHUNK_CH / 2) * PAIR_UNITS;   // 1440 units = 11520 bytes
constexpr int PARTS = CHUNK_CH / 4;                        // 16-byte pieces (4 channels) of one patch pixel in a chunk
constexpr int PIECES = PATCH * PATCH * PARTS;              // pieces of one chunk: 648
constexpr int PIECES_PER_THREAD = (PIECES + 255) / 256;    // 3
constexpr int U_STEP_FLOATS = 2 * 4 * 64 * 4;              // one K-step of U: [half][plane quad][lane][4] = 8 KB
constexpr int U_FLOATS = NSTEPS * U_STEP_FLOATS;           // 65536 floats = 262144 bytes per layer

// tile (row, column) inside the block of lane % 32 = tl of a wave in tile group tg
W64_HD int tile_y(int tg, int tl) { return 4 * tg + (tl >> 3); }
W64_HD int tile_x(int tl) { return tl & 7; }
// K permutation: input channel that lane half k (= lane / 32) multiplies in K-step `step`. Steps 2 j and 2 j + 1 of a chunk take the two
// floats of ONE 8-byte LDS read (channel pair 2 j + k of the chunk).
W64_HD int channel(int step, int k) { return 4 * (step >> 1) + 2 * k + (step & 1); }
// output channel of accumulator element e (0..15) of a lane in channel half `half`
W64_HD int acc_channel(int half, int lane, int e) { return half * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3); }
// U fragment layout [K-step][half][plane quad q][lane][4]: plane 4 q + j; a wave's load of one quad is 1 KB contiguous
W64_HD int u_index(int step, int half, int q, int lane, int j) { return ((((step * 2 + half) * 4 + q) * 64 + lane) << 2) + j; }
// 8-byte unit of (channel pair, patch row, patch column) in the LDS image of a chunk
W64_HD int patch_unit(int pair, int py, int px) { return pair * PAIR_UNITS + py * ROW_UNITS + (px & 1) * (ROW_UNITS / 2) + (px >> 1); }

// V = B^T d B for one 4 x 4 patch d (row major); plane order 4 a + b. B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]: adds only.
W64_HD void input_transform(const float d[16], float v[16]) {
  float t[16];
  for (int c = 0; c < 4; ++c) {
    t[0 + c] = d[0 + c] - d[8 + c];
    t[4 + c] = d[4 + c] + d[8 + c];
    t[8 + c] = d[8 + c] - d[4 + c];
    t[12 + c] = d[4 + c] - d[12 + c];
  }
  for (int a = 0; a < 4; ++a) {
    v[4 * a + 0] = t[4 * a + 0] - t[4 * a + 2];
    v[4 * a + 1] = t[4 * a + 1] + t[4 * a + 2];
    v[4 * a + 2] = t[4 * a + 2] - t[4 * a + 1];
    v[4 * a + 3] = t[4 * a + 1] - t[4 * a + 3];
  }
}
// Y = A^T M A for the 16 planes of one (tile, channel); y = [row 0: col 0, col 1; row 1: col 0, col 1]. A^T = [1 1 1 0; 0 1 -1 -1].
W64_HD void output_transform(const float m[16], float y[4]) {
  float s[8];
  for (int b = 0; b < 4; ++b) {
    s[b] = (m[b] + m[4 + b]) + m[8 + b];
    s[4 + b] = (m[4 + b] - m[8 + b]) - m[12 + b];
  }
  for (int i = 0; i < 2; ++i) {
    y[2 * i + 0] = (s[4 * i + 0] + s[4 * i + 1]) + s[4 * i + 2];
    y[2 * i + 1] = (s[4 * i + 1] - s[4 * i + 2]) - s[4 * i + 3];
  }
}

// U = G g G^T per (output channel, input channel), in double, into the fragment layout; rows >= Cout and channels >= Cin stay zero.
// w: [Cout][Cin][3][3]; U: U_FLOATS floats.
inline void pack_u(const float* w, int Cout, int Cin, float* U) {
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  for (int i = 0; i < U_FLOATS; ++i) U[i] = 0.f;
  for (int step = 0; step < NSTEPS; ++step)
    for (int half = 0; half < 2; ++half)
      for (int lane = 0; lane < 64; ++lane) {
        const int co = half * 32 + (lane & 31), ci = channel(step, lane >> 5);
        if (co >= Cout || ci >= Cin) continue;
        const float* g = w + ((long long)co * Cin + ci) * 9;
        double tmp[4][3];
        for (int a = 0; a < 4; ++a)
          for (int q = 0; q < 3; ++q) tmp[a][q] = G[a][0] * g[q] + G[a][1] * g[3 + q] + G[a][2] * g[6 + q];
        for (int a = 0; a < 4; ++a)
          for (int b = 0; b < 4; ++b) {
            const double u = tmp[a][0] * G[b][0] + tmp[a][1] * G[b][1] + tmp[a][2] * G[b][2];
            U[u_index(step, half, a, lane, b)] = (float)u;
          }
      }
}

}  // namespace w64
}  // namespace fe
