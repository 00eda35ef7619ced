// Host harness of tag_select_core.h (tests/test_tag_select_host.py builds it with -fsanitize=address,undefined).
//   tag_select_harness in.bin out.bin
// in.bin:  int32 cases, then per case: int32 n, T, G, max_tags, ld; double threshold; int32 tag_of_prompt[T]; float sims[n][ld]
// out.bin: per case: int32 status (tagsel::GroupsStatus), int32 where; when status is 0: int32 perm[T], goff[G + 1], then
//          int32 ids[n][max_tags], float scores[n][max_tags], int32 counts[n]
// Every buffer has exactly the size the header documents, so a read or store outside it is a sanitizer report.
#include "tag_select_core.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}
template <class T>
static void wr(FILE* f, const T* p, size_t n) {
  if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "short output\n"); exit(2); }
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
  int32_t cases = 0;
  rd(fi, &cases, 1);
  for (int c = 0; c < cases; ++c) {
    int32_t h[5];
    double threshold;
    rd(fi, h, 5);
    rd(fi, &threshold, 1);
    const int n = h[0], T = h[1], G = h[2], max_tags = h[3], ld = h[4];
    std::vector<int32_t> top((size_t)T), perm((size_t)T), goff((size_t)G + 1);
    std::vector<float> sims((size_t)n * ld);
    rd(fi, top.data(), top.size());
    rd(fi, sims.data(), sims.size());
    int where = -1;
    const int32_t status = fe::tagsel::build_groups(top.data(), T, G, perm.data(), goff.data(), &where);
    const int32_t where32 = where;
    wr(fo, &status, 1);
    wr(fo, &where32, 1);
    if (status != 0) continue;
    wr(fo, perm.data(), perm.size());
    wr(fo, goff.data(), goff.size());
    std::vector<int32_t> ids((size_t)n * max_tags), counts((size_t)n);
    std::vector<float> scores((size_t)n * max_tags), score((size_t)G);
    std::vector<uint8_t> kept((size_t)G);
    for (int i = 0; i < n; ++i) {
      // the row alone in a buffer of its own size: nothing past T floats may be read
      std::vector<float> row(sims.begin() + (size_t)i * ld, sims.begin() + (size_t)i * ld + T);
      counts[i] = fe::tagsel::select_row(row.data(), perm.data(), goff.data(), G, threshold, max_tags, ids.data() + (size_t)i * max_tags,
                                         scores.data() + (size_t)i * max_tags, score.data(), kept.data());
    }
    wr(fo, ids.data(), ids.size());
    wr(fo, scores.data(), scores.size());
    wr(fo, counts.data(), counts.size());
  }
  fclose(fi);
  fclose(fo);
  return 0;
}
