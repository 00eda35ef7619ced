// Outer-border following and the Green sums of a border polygon, shared by the kernels of kernels_contours.hip and by host code.
// Suzuki & Abe 1985 (algorithm 1) as cv2.findContours follows an outer border: from the component's first pixel in raster order, the
// neighbourhood is searched clockwise starting at the left neighbour for the first foreground pixel; from then on every step searches
// counter-clockwise, starting one past the direction it came from. The walk ends when it steps from the pixel found first back onto
// the start pixel. Directions: 0 = E, 1 = NE, 2 = N, 3 = NW, 4 = W, 5 = SW, 6 = S, 7 = SE (y grows downwards).
// The sums are those of cv2.moments / cv2.contourArea over the closed polygon through the pixel centres, left as exact integers:
// with consecutive points p, q and d = p.x q.y - q.x p.y: a00 += d, a10 += d (p.x + q.x), a01 += d (p.y + q.y).
// contourArea = |a00| / 2, m00 = a00 / 2, m10 = a10 / 6, m01 = a01 / 6 (all three negated when a00 < 0). Collinear points add nothing
// that their end points do not, so the full chain gives what CHAIN_APPROX_SIMPLE gives. [DEP-KNOWLEDGE: OpenCV contours.cpp, moments.cpp]
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FE_CHD __host__ __device__ __forceinline__
#else
#define FE_CHD inline
#endif

namespace fe {
namespace contour {

struct Sums {
  long long a00, a10, a01;
};

FE_CHD int dir_dx(int s) { return s == 0 || s == 1 || s == 7 ? 1 : (s >= 3 && s <= 5 ? -1 : 0); }
FE_CHD int dir_dy(int s) { return s >= 1 && s <= 3 ? -1 : (s >= 5 ? 1 : 0); }

FE_CHD void add_edge(Sums& a, int px, int py, int qx, int qy) {
  const long long d = (long long)px * qy - (long long)qx * py;
  a.a00 += d;
  a.a10 += d * (px + qx);
  a.a01 += d * (py + qy);
}

// the state a step of the walk depends on: where it stands and the direction it looks in first
struct Walk {
  int x, y, s;
};

// One step: from w (standing on a foreground pixel) to the next border pixel. fg(x, y) must answer false outside the image.
// Returns false when the pixel has no foreground neighbour at all (only the start pixel of a one-pixel component can).
template <class Fg>
FE_CHD bool step(const Fg& fg, Walk& w) {
  for (int k = 0; k < 8; ++k) {
    const int s = (w.s + 1 + k) & 7;
    const int nx = w.x + dir_dx(s), ny = w.y + dir_dy(s);
    if (fg(nx, ny)) {
      w.x = nx;
      w.y = ny;
      w.s = (s + 4) & 7;      // the next search starts one past the pixel just left
      return true;
    }
  }
  return false;
}

// Follows the outer border that starts at (x0, y0), the first pixel of its component in raster order (so its W, NW, N and NE
// neighbours are background). Returns the number of steps taken, or -1 when `max_steps` steps did not close the border; a state
// (pixel, direction) never repeats before the end, so 8 * pixel count + 8 is always enough.
template <class Fg>
FE_CHD long long follow_outer(const Fg& fg, int x0, int y0, long long max_steps, Sums* out) {
  Sums a = {0, 0, 0};
  *out = a;
  int s = 4;
  bool found = false;
  for (int k = 0; k < 7 && !found; ++k) {      // clockwise from the left neighbour: NW, N, NE, E, SE, S, SW
    s = (s + 7) & 7;
    found = fg(x0 + dir_dx(s), y0 + dir_dy(s));
  }
  if (!found) return 0;                         // a single pixel: one point, all sums zero
  const int x1 = x0 + dir_dx(s), y1 = y0 + dir_dy(s);
  Walk w = {x0, y0, s};
  for (long long n = 1; n <= max_steps; ++n) {
    const int px = w.x, py = w.y;
    if (!step(fg, w)) return -1;
    add_edge(a, px, py, w.x, w.y);
    if (w.x == x0 && w.y == y0 && px == x1 && py == y1) {
      *out = a;
      return n;
    }
  }
  return -1;
}

}  // namespace contour
}  // namespace fe
