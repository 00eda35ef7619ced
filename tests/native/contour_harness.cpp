// Host harness for facet_amd/csrc/contour_core.h: follows the outer border of every external component of binary images with the
// functions the kernel uses, under AddressSanitizer + UBSan (tests/test_subject_host.py). Components and the external test are found
// here with plain flood fills (8-connected foreground; 4-connected background grown from the frame), the image in a buffer of exactly
// h * w bytes so that a walk that leaves it is reported.
//   in:  int32 n; n x { int32 h, w; h * w bytes }
//   out: n x { int32 k; k x { int64 record[8], steps, bound } }   records in descending start_index order
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "contour_core.h"

using namespace fe::contour;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n;
  if (fread(&n, 4, 1, f) != 1) return 2;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (int i = 0; i < n; ++i) {
    int32_t hw[2];
    if (fread(hw, 4, 2, f) != 2) return 2;
    const int h = hw[0], w = hw[1];
    uint8_t* im = (uint8_t*)malloc((size_t)h * w);
    if (fread(im, 1, (size_t)h * w, f) != (size_t)h * w) return 2;
    // background reachable from the frame, 4-connected
    std::vector<uint8_t> outer((size_t)h * w, 0);
    std::vector<int> stack;
    auto push_bg = [&](int y, int x) {
      if (y < 0 || y >= h || x < 0 || x >= w || im[y * w + x] || outer[y * w + x]) return;
      outer[y * w + x] = 1;
      stack.push_back(y * w + x);
    };
    for (int x = 0; x < w; ++x) { push_bg(0, x); push_bg(h - 1, x); }
    for (int y = 0; y < h; ++y) { push_bg(y, 0); push_bg(y, w - 1); }
    while (!stack.empty()) {
      const int p = stack.back();
      stack.pop_back();
      push_bg(p / w - 1, p % w); push_bg(p / w + 1, p % w); push_bg(p / w, p % w - 1); push_bg(p / w, p % w + 1);
    }
    std::vector<uint8_t> seen((size_t)h * w, 0);
    std::vector<std::vector<int64_t>> recs;
    auto fg = [&](int x, int y) { return x >= 0 && x < w && y >= 0 && y < h && im[y * w + x] != 0; };
    for (int p = 0; p < h * w; ++p) {
      if (!im[p] || seen[p]) continue;
      long long count = 0;
      int x0 = p % w, y0 = p / w, xmin = x0, xmax = x0, ymax = y0;
      seen[p] = 1;
      stack.push_back(p);
      while (!stack.empty()) {
        const int q = stack.back();
        stack.pop_back();
        ++count;
        const int qx = q % w, qy = q / w;
        xmin = qx < xmin ? qx : xmin; xmax = qx > xmax ? qx : xmax; ymax = qy > ymax ? qy : ymax;
        for (int s = 0; s < 8; ++s) {
          const int nx = qx + dir_dx(s), ny = qy + dir_dy(s);
          if (fg(nx, ny) && !seen[ny * w + nx]) { seen[ny * w + nx] = 1; stack.push_back(ny * w + nx); }
        }
      }
      if (x0 > 0 && !outer[p - 1]) continue;      // inside a hole of another component
      Sums a;
      const long long bound = 8 * count + 8;
      const long long steps = follow_outer(fg, x0, y0, bound, &a);
      recs.push_back({p, a.a00, a.a10, a.a01, xmin, y0, xmax, ymax, steps, bound});
    }
    const int32_t k = (int32_t)recs.size();
    fwrite(&k, 4, 1, o);
    for (int j = k - 1; j >= 0; --j) fwrite(recs[j].data(), 8, 10, o);
    free(im);
  }
  fclose(o);
  fclose(f);
  return 0;
}
