// Tag selection for one row of prompt similarities: the arithmetic shared by tag_select_kernel (kernels_tags.hip) and the host
// (tests/native/tag_select_harness.cpp compiles this file alone, under the sanitizers).
//
// It restates the reference's selection (models/tagger.py:103-114) exactly:
//   tag_scores = {}
//   for tag_name, sim in zip(self.tag_names, similarities):            # sim: np.float32
//       if tag_name not in tag_scores or sim > tag_scores[tag_name]:
//           tag_scores[tag_name] = float(sim)
//   filtered = [(tag, score) for tag, score in tag_scores.items() if score >= threshold]
//   filtered.sort(key=lambda x: x[1], reverse=True)
//   return [tag for tag, _ in filtered[:max_tags]]
//
// score:     the tag's prompts folded in prompt order: the first prompt's similarity, replaced only by a later one that is `>` the
//            current value. A NaN in first place stays (nothing is > NaN), a NaN later is skipped (NaN > x is false).
// threshold: kept iff (double)score >= threshold. The reference compares float(sim) with a Python float, so the compare is in double:
//            np.float32(0.22) < 0.22. NaN never passes.
// order:     descending score, ties by ascending tag id (the tag's first appearance in the prompt list: list.sort(reverse=True) is
//            stable on the dict's insertion order). A kept tag's position is the number of kept tags that beat it: `beats` is a strict
//            total order on kept tags (no kept score is NaN), so the positions are 0 .. kept-1, each once, whatever the order of
//            evaluation. The first max_tags positions are written.
//
// Groups: prompts of one tag need not be contiguous. perm [T] lists the prompts sorted by (tag, prompt index) and goff [G + 1] are
// the CSR offsets of the tags in perm, both made once per vocabulary (build_groups).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FE_TSHD __host__ __device__ __forceinline__
#else
#define FE_TSHD inline
#endif

namespace fe {
namespace tagsel {

constexpr int kMaxPrompts = 4096;      // 1 <= G <= T <= kMaxPrompts: a row and its scores fit the kernel's LDS

// the score of the tag whose prompts are perm[begin .. end), begin < end
FE_TSHD float fold(const float* sims, const int32_t* perm, int begin, int end) {
  float best = sims[perm[begin]];
  for (int k = begin + 1; k < end; ++k) {
    const float s = sims[perm[k]];
    if (s > best) best = s;
  }
  return best;
}

FE_TSHD bool keep(float score, double threshold) { return (double)score >= threshold; }

// kept tag a (score sa) comes before kept tag b (score sb)
FE_TSHD bool beats(float sa, int a, float sb, int b) { return sa > sb || (sa == sb && a < b); }

// ---- host only ---------------------------------------------------------------------------------------------------------------------
// perm [T] and goff [G + 1] from tag_of_prompt [T], 1 <= G <= T. Every id of 0 .. G-1 must be used, and the ids must first appear
// in ascending order: the tag id is the tie-break of the order above, so it has to be the reference's dict insertion order.
// GROUPS_OK, or what is wrong, with *where the prompt (GROUPS_ID_RANGE, GROUPS_ID_ORDER) or the id (GROUPS_ID_UNUSED) it is about.
enum GroupsStatus { GROUPS_OK = 0, GROUPS_ID_RANGE, GROUPS_ID_ORDER, GROUPS_ID_UNUSED };
inline GroupsStatus build_groups(const int32_t* tag_of_prompt, int T, int G, int32_t* perm, int32_t* goff, int* where) {
  for (int g = 0; g <= G; ++g) goff[g] = 0;
  int seen = 0;                                   // ids 0 .. seen-1 have appeared
  for (int t = 0; t < T; ++t) {
    const int g = tag_of_prompt[t];
    *where = t;
    if (g < 0 || g >= G) return GROUPS_ID_RANGE;
    if (g > seen) return GROUPS_ID_ORDER;
    if (g == seen) ++seen;
    ++goff[g + 1];
  }
  *where = seen;
  if (seen != G) return GROUPS_ID_UNUSED;
  for (int g = 0; g < G; ++g) goff[g + 1] += goff[g];
  // a counting sort in prompt order (ascending prompt index within a tag): goff[g] is tag g's cursor, then shifted back
  for (int t = 0; t < T; ++t) perm[goff[tag_of_prompt[t]]++] = t;
  for (int g = G; g > 0; --g) goff[g] = goff[g - 1];
  goff[0] = 0;
  return GROUPS_OK;
}

// One row on the host, the kernel's steps in sequence. score / kept: scratch [G]. ids / scores [max_tags] are padded with -1 / 0.
// Returns the entries written.
inline int select_row(const float* sims, const int32_t* perm, const int32_t* goff, int G, double threshold, int max_tags, int32_t* ids,
                      float* scores, float* score, uint8_t* kept) {
  for (int g = 0; g < G; ++g) {
    score[g] = fold(sims, perm, goff[g], goff[g + 1]);
    kept[g] = keep(score[g], threshold) ? 1 : 0;
  }
  for (int k = 0; k < max_tags; ++k) { ids[k] = -1; scores[k] = 0.f; }
  int n = 0;
  for (int g = 0; g < G; ++g) {
    if (!kept[g]) continue;
    int rank = 0;
    for (int h = 0; h < G; ++h) rank += (kept[h] && beats(score[h], h, score[g], g)) ? 1 : 0;
    if (rank < max_tags) { ids[rank] = g; scores[rank] = score[g]; ++n; }
  }
  return n;
}

}  // namespace tagsel
}  // namespace fe
