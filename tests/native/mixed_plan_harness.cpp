// Replays the plans of a mixed-size ensemble call (facet_amd/csrc/ensemble_plan.h: cut_mixed + build(Shape, cuts), what
// ensemble_run_mixed executes) on simulated in-order queues (tests/test_mixed_plan_host.py).
//
//   mixed_plan_harness check <on_device> <overlap>     every case below under the model masks 7, 6, 5 and 1; prints "<plans> plans ok"
//
// Cases: all images of one shape; two shapes alternating; every image different; n = 1; 70 images in 3 shapes at micro-batch 16. Mask 6
// is TOPIQ deselected. Device images lie back to back in input order, so only a group whose members are neighbours is taken in place.
// As in ensemble_plan_harness.cpp each queue carries a vector clock, an event keeps the clock of its last record and a wait merges it in.
// Checked for every plan:
//   1. two operations on different queues that touch overlapping parts of a region, at least one writing, are ordered, and every
//      operation of the side queue is ordered before the interleave;
//   2. every image passes through each selected model exactly once, read from where the plan says it lies (its own address, the
//      staging buffer a copy or a gather filled), and the interleave's position map returns every record to its input index;
//   3. with TOPIQ on a micro-batch holds one shape, and is gathered exactly when its images are not consecutive in memory or start
//      off a 4-byte boundary;
//   4. for uniform input the operation list equals build(Shape) element by element.
#include "ensemble_plan.h"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace fe::plan;

namespace {
typedef std::array<int, N_LANES> Clock;

struct Case {
  const char* name;
  int mb;
  std::vector<int32_t> hw;   // [n][2]
  int n() const { return (int)hw.size() / 2; }
};

bool same(const Op& a, const Op& b) {
  if (a.kind != b.kind || a.lane != b.lane || a.mb != b.mb || a.img0 != b.img0 || a.count != b.count || a.slot != b.slot || a.left != b.left ||
      a.event != b.event || a.n_acc != b.n_acc)
    return false;
  for (int i = 0; i < a.n_acc; ++i)
    if (a.acc[i].region != b.acc[i].region || a.acc[i].lo != b.acc[i].lo || a.acc[i].hi != b.acc[i].hi || a.acc[i].write != b.acc[i].write) return false;
  return true;
}

struct Checker {
  const Shape& s;
  const Case& c;
  const MixedCuts& mc;
  const std::vector<Op>& ops;
  const std::vector<uintptr_t>& addr;
  std::string why;
  bool fail(const std::string& m) { why = m; return false; }
  static bool before(const Op& a, const Clock& ca, const Clock& cb) { return ca[a.lane] <= cb[a.lane]; }

  bool run() {
    const int n_ops = (int)ops.size(), n = s.n;
    // the cuts themselves
    std::vector<int> first(mc.cuts.size() + 1, 0);
    for (size_t k = 0; k < mc.cuts.size(); ++k) {
      if (mc.cuts[k].count < 1 || mc.cuts[k].count > s.mb) return fail("cut outside 1 .. micro-batch");
      first[k + 1] = first[k] + mc.cuts[k].count;
    }
    if (first.back() != n || (int)mc.order.size() != n) return fail("the cuts do not cover the images");
    std::vector<int> pos(n, -1);
    for (int p = 0; p < n; ++p) {
      if (mc.order[p] < 0 || mc.order[p] >= n || pos[mc.order[p]] != -1) return fail("order is no permutation");
      pos[mc.order[p]] = p;
    }
    auto shape_of = [&](int i) { return std::make_pair(c.hw[2 * i], c.hw[2 * i + 1]); };
    if (s.topiq)
      for (size_t k = 0; k < mc.cuts.size(); ++k) {
        bool apart = (addr[mc.order[first[k]]] & 3) != 0;      // TOPIQ reads 4-byte words: an odd start is gathered too
        for (int p = first[k]; p < first[k + 1]; ++p) {
          if (shape_of(mc.order[p]) != shape_of(mc.order[first[k]])) return fail("a micro-batch mixes shapes with TOPIQ on");
          if (p > first[k] && addr[mc.order[p]] != addr[mc.order[p - 1]] + (uintptr_t)c.hw[2 * mc.order[p]] * c.hw[2 * mc.order[p] + 1] * 3) apart = true;
        }
        if (mc.cuts[k].gather != (s.on_device && apart)) return fail("gather flag of micro-batch " + std::to_string(k));
      }
    else if (mc.order != [&] { std::vector<int> id(n); for (int i = 0; i < n; ++i) id[i] = i; return id; }())
      return fail("without TOPIQ the micro-batches are slices of the list");
    // clocks
    std::vector<Clock> stamp(n_ops);
    Clock lane[N_LANES] = {};
    Clock ev[N_EVENTS] = {};
    bool recorded[N_EVENTS] = {};
    for (int i = 0; i < n_ops; ++i) {
      const Op& o = ops[i];
      if (o.lane < 0 || o.lane >= N_LANES) return fail("lane out of range");
      if (!s.overlap && o.lane == LANE_SIDE) return fail("side lane used with overlap off");
      if (s.on_device && o.lane == LANE_COPY) return fail("copy lane used with device input");
      if (o.kind == OP_WAIT) {
        if (o.event < 0 || o.event >= N_EVENTS || !recorded[o.event]) return fail("wait on an event never recorded");
        for (int l = 0; l < N_LANES; ++l) lane[o.lane][l] = std::max(lane[o.lane][l], ev[o.event][l]);
      }
      lane[o.lane][o.lane] += 1;
      stamp[i] = lane[o.lane];
      if (o.kind == OP_RECORD) {
        if (o.event < 0 || o.event >= N_EVENTS) return fail("event out of range");
        ev[o.event] = stamp[i];
        recorded[o.event] = true;
      }
    }
    // 1. hazards
    std::vector<std::pair<int, int>> touch[R_ARENA_SIDE + 1];
    for (int i = 0; i < n_ops; ++i)
      for (int a = 0; a < ops[i].n_acc; ++a) {
        const Access& x = ops[i].acc[a];
        if (x.region < 0 || x.region > R_ARENA_SIDE || x.lo < 0 || x.hi < x.lo) return fail("bad access");
        touch[x.region].push_back({i, a});
      }
    for (int r = 0; r <= R_ARENA_SIDE; ++r)
      for (size_t q = 1; q < touch[r].size(); ++q) {
        const Op& b = ops[touch[r][q].first];
        const Access& xb = b.acc[touch[r][q].second];
        for (size_t p = 0; p < q; ++p) {
          const Op& a = ops[touch[r][p].first];
          if (a.lane == b.lane) continue;
          const Access& xa = a.acc[touch[r][p].second];
          if (!(xa.write || xb.write) || xa.hi <= xb.lo || xb.hi <= xa.lo) continue;
          if (!before(a, stamp[touch[r][p].first], stamp[touch[r][q].first]))
            return fail("unordered access to region " + std::to_string(r) + ": operations " + std::to_string(touch[r][p].first) + " and " +
                        std::to_string(touch[r][q].first));
        }
      }
    if (ops.empty() || ops.back().kind != OP_INTERLEAVE || ops.back().lane != LANE_MAIN) return fail("the plan does not end with the interleave");
    for (int i = 0; i + 1 < n_ops; ++i)
      if (ops[i].lane == LANE_SIDE && !before(ops[i], stamp[i], stamp[n_ops - 1])) return fail("side operation " + std::to_string(i) + " not joined");
    // 2. contents, in list order: stage buffers and crop slots hold input indices, the planes [model][position] too
    std::vector<int> stage[2], slots[2], plane[3];
    stage[0].assign(s.mb, -1); stage[1].assign(s.mb, -1);
    slots[0].assign(s.clip_chunk + s.mb, -1); slots[1].assign(s.samp_chunk + s.mb, -1);
    for (auto& v : plane) v.assign(n, -1);
    std::vector<int> seen[3];
    for (auto& v : seen) v.assign(n, 0);
    bool cleared = false;
    auto in_cut = [&](const Op& o) {
      return o.mb >= 0 && o.mb < (int)mc.cuts.size() && o.img0 == first[o.mb] && o.count == mc.cuts[o.mb].count;
    };
    for (const Op& o : ops) {
      if (o.kind == OP_CLEAR) { cleared = true; continue; }
      if (o.kind == OP_RECORD || o.kind == OP_WAIT) continue;
      if (!cleared) return fail("work before the clear of the result planes");
      if (o.kind == OP_COPY_IN || o.kind == OP_GATHER) {
        if (!in_cut(o) || (o.kind == OP_COPY_IN) == s.on_device) return fail("bad copy / gather");
        if (o.kind == OP_GATHER && !mc.cuts[o.mb].gather) return fail("gather of a micro-batch that lies back to back");
        for (int i = 0; i < s.mb; ++i) stage[o.mb & 1][i] = i < o.count ? mc.order[o.img0 + i] : -1;
      } else if (o.kind == OP_TOPIQ) {
        if (!in_cut(o)) return fail("topiq range is no micro-batch");
        const bool staged = !s.on_device || mc.cuts[o.mb].gather;
        for (int i = 0; i < o.count; ++i) {
          const int img = mc.order[o.img0 + i];
          if (staged ? stage[o.mb & 1][i] != img : (addr[img] != addr[mc.order[o.img0]] + (uintptr_t)i * c.hw[2 * img] * c.hw[2 * img + 1] * 3)) return fail("topiq reads the wrong image");
          seen[0][img] += 1;
          plane[0][o.img0 + i] = img;
        }
      } else if (o.kind == OP_CLIP_PRE || o.kind == OP_SAMP_PRE) {
        std::vector<int>& sl = slots[o.kind == OP_SAMP_PRE];
        if (!in_cut(o) || o.slot < 0 || o.slot + o.count > (int)sl.size()) return fail("bad crop range");
        for (int i = 0; i < o.count; ++i) {
          const int img = mc.order[o.img0 + i];      // device input: the descriptor holds the image's own address
          if (!s.on_device && stage[o.mb & 1][i] != img) return fail("crops read the wrong image");
          if (sl[o.slot + i] != -1) return fail("crop written over a waiting crop");
          sl[o.slot + i] = img;
        }
      } else if (o.kind == OP_CLIP_TOWER || o.kind == OP_SAMP_NETS) {
        const bool sp = o.kind == OP_SAMP_NETS;
        std::vector<int>& sl = slots[sp];
        if (o.count < 1 || o.count > (sp ? s.samp_chunk : s.clip_chunk) || o.img0 < 0 || o.img0 + o.count > n) return fail("bad model range");
        for (int i = 0; i < o.count; ++i) {
          if (sl[i] < 0 || sl[i] != mc.order[o.img0 + i]) return fail("model result lands at another image's position");
          seen[sp ? 2 : 1][sl[i]] += 1;
          plane[sp ? 2 : 1][o.img0 + i] = sl[i];
          sl[i] = -1;
        }
      } else if (o.kind == OP_CLIP_COMPACT || o.kind == OP_SAMP_COMPACT) {
        std::vector<int>& sl = slots[o.kind == OP_SAMP_COMPACT];
        if (o.count < 1 || o.left < 1 || o.count + o.left > (int)sl.size()) return fail("bad compaction");
        for (int i = 0; i < o.left; ++i) {
          if (sl[i] != -1) return fail("compaction over a waiting crop");
          sl[i] = sl[o.count + i];
          sl[o.count + i] = -1;
        }
      } else if (o.kind == OP_INTERLEAVE) {
        const bool on[3] = {s.topiq, s.clip, s.samp};
        for (int m = 0; m < 3; ++m)
          for (int i = 0; i < n; ++i) {
            if (seen[m][i] != (on[m] ? 1 : 0)) return fail("image " + std::to_string(i) + " went through model " + std::to_string(m) + " " + std::to_string(seen[m][i]) + " times");
            if (on[m] && plane[m][pos[i]] != i) return fail("record " + std::to_string(i) + " does not come back to its input index");
          }
      } else {
        return fail("unknown operation");
      }
    }
    return true;
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4 || std::string(argv[1]) != "check") { fprintf(stderr, "usage: %s check <on_device> <overlap>\n", argv[0]); return 2; }
  const bool on_device = atoi(argv[2]) != 0, overlap = atoi(argv[3]) != 0;
  std::vector<Case> cases;
  auto add = [&](const char* name, int mb, int n, auto shape) {
    Case c{name, mb, {}};
    for (int i = 0; i < n; ++i) { const std::pair<int, int> s = shape(i); c.hw.push_back(s.first); c.hw.push_back(s.second); }
    cases.push_back(c);
  };
  add("one shape", 8, 37, [](int) { return std::make_pair(64, 96); });
  add("one shape, n a multiple of the micro-batch", 8, 32, [](int) { return std::make_pair(64, 96); });
  add("two shapes alternating", 8, 20, [](int i) { return i % 2 ? std::make_pair(96, 64) : std::make_pair(64, 96); });
  add("every image different", 4, 13, [](int i) { return std::make_pair(40 + i, 300 - 7 * i); });
  add("every image different, micro-batch 3", 3, 8, [](int i) { return std::make_pair(33 + 5 * i, 47 + i); });
  add("n = 1", 8, 1, [](int) { return std::make_pair(48, 1100); });
  add("70 images in 3 shapes", 16, 70, [](int i) { const int k = (i * 7 + i / 5) % 3; return std::make_pair(64 + 16 * k, 96 - 8 * k); });
  int plans = 0;
  for (const Case& c : cases)
    for (int mask : {7, 6, 5, 1})
      for (int variant = 0; variant < (overlap ? 4 : 1); ++variant)
        for (int sc : {5, 128}) {
          Shape s;
          s.clip_side = variant != 2; s.samp_side = variant != 1; s.samp_first = variant == 3;
          s.n = c.n(); s.mb = c.mb; s.on_device = on_device; s.overlap = overlap;
          s.topiq = mask & 1; s.clip = mask & 2; s.samp = mask & 4;
          s.clip_chunk = fe::clip_tower_chunk(1024, 257, s.n);
          s.samp_chunk = std::min(s.n, sc);
          std::vector<uintptr_t> addr(s.n);
          uintptr_t at = 4096;
          for (int i = 0; i < s.n; ++i) { addr[i] = at; at += (uintptr_t)c.hw[2 * i] * c.hw[2 * i + 1] * 3; }
          const MixedCuts mc = cut_mixed(c.hw.data(), s.n, s.mb, s.topiq, on_device ? addr.data() : nullptr);
          const std::vector<Op> ops = build(s, mc.cuts);
          Checker ck{s, c, mc, ops, addr, {}};
          if (!ck.run()) {
            printf("FAILED %s: mask=%d on_device=%d overlap=%d variant=%d samp_chunk=%d: %s\n", c.name, mask, (int)on_device, (int)overlap, variant, sc, ck.why.c_str());
            return 1;
          }
          bool uniform = true;
          for (int i = 1; i < s.n; ++i) uniform = uniform && c.hw[2 * i] == c.hw[0] && c.hw[2 * i + 1] == c.hw[1];
          if (uniform) {
            const std::vector<Op> ref = build(s);
            bool eq = ref.size() == ops.size();
            for (size_t i = 0; eq && i < ref.size(); ++i) eq = same(ref[i], ops[i]);
            if (!eq) { printf("FAILED %s: mask=%d: the plan of uniform input differs from build(Shape)\n", c.name, mask); return 1; }
          }
          ++plans;
        }
  printf("%d plans ok\n", plans);
  return 0;
}
