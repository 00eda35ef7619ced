// Replays the schedule of facet_amd/csrc/ensemble_plan.h on simulated in-order queues (tests/test_overlap_host.py).
//
//   ensemble_plan_harness check <on_device>                      every case of the grid below; prints "<plans> plans ok"
//   ensemble_plan_harness drop <n> <mb> <samp_chunk> <on_device> removes each wait of that plan in turn and counts how many removals
//                                                                the checks notice; prints "waits <W> detected <D>"
//
// Each queue carries a vector clock; an event keeps the clock of its last record, a wait merges it into the waiting queue. Operation
// a is ordered before b when b's clock has reached a's tick on a's queue. Checked for every plan:
//   1. every image goes through every selected model exactly once, from the staging slots the plan says, into its own result rows;
//   2. two operations on different queues that touch overlapping parts of a region, at least one writing, are ordered;
//   3. every operation of the side queue is ordered before the interleave.
#include "ensemble_plan.h"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace fe::plan;

namespace {
typedef std::array<int, N_LANES> Clock;

struct Checker {
  const Shape& s;
  const std::vector<Op>& ops;
  std::string why;
  Checker(const Shape& shape, const std::vector<Op>& list) : s(shape), ops(list) {}

  bool fail(const std::string& m) { why = m; return false; }
  static bool before(const Op& a, const Clock& ca, const Clock& cb) { return ca[a.lane] <= cb[a.lane]; }

  bool run() {
    const int n_ops = (int)ops.size();
    std::vector<Clock> stamp(n_ops);
    Clock lane[N_LANES] = {};
    Clock ev[N_EVENTS] = {};
    bool recorded[N_EVENTS] = {};
    for (int i = 0; i < n_ops; ++i) {
      const Op& o = ops[i];
      if (o.lane < 0 || o.lane >= N_LANES) return fail("lane out of range");
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
    // 2. hazards, region by region
    std::vector<std::pair<int, int>> touch[R_ARENA_SIDE + 1];   // (operation, access)
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
    // 3. the join
    if (ops.empty() || ops.back().kind != OP_INTERLEAVE || ops.back().lane != LANE_MAIN) return fail("the plan does not end with the interleave");
    for (int i = 0; i + 1 < n_ops; ++i)
      if (ops[i].lane == LANE_SIDE && !before(ops[i], stamp[i], stamp[n_ops - 1])) return fail("side operation " + std::to_string(i) + " not joined");
    // 1. contents: which image sits where, in list order (the ordering itself was checked above)
    std::vector<int> stage[2], slots[2];
    stage[0].assign(s.mb, -1); stage[1].assign(s.mb, -1);
    slots[0].assign(s.clip_chunk + s.mb, -1); slots[1].assign(s.samp_chunk + s.mb, -1);
    std::vector<int> seen[3];
    for (auto& v : seen) v.assign(s.n, 0);
    bool cleared = false;
    auto source = [&](const Op& o, int i) { return s.on_device ? o.img0 + i : stage[o.mb & 1][i]; };
    for (const Op& o : ops) {
      if (o.kind == OP_CLEAR) { cleared = true; continue; }
      if (o.kind == OP_RECORD || o.kind == OP_WAIT) continue;
      if (!cleared) return fail("work before the clear of the result planes");
      if (o.kind == OP_COPY_IN) {
        if (s.on_device || o.count < 1 || o.count > s.mb || o.img0 != o.mb * s.mb || o.img0 + o.count > s.n) return fail("bad copy");
        for (int i = 0; i < s.mb; ++i) stage[o.mb & 1][i] = i < o.count ? o.img0 + i : -1;
      } else if (o.kind == OP_TOPIQ) {
        if (o.count < 1 || o.count > s.mb || o.img0 < 0 || o.img0 + o.count > s.n) return fail("bad topiq range");
        for (int i = 0; i < o.count; ++i) {
          if (source(o, i) != o.img0 + i) return fail("topiq reads the wrong image");
          seen[0][o.img0 + i] += 1;
        }
      } else if (o.kind == OP_CLIP_PRE || o.kind == OP_SAMP_PRE) {
        std::vector<int>& sl = slots[o.kind == OP_SAMP_PRE];
        if (o.count < 1 || o.count > s.mb || o.img0 < 0 || o.img0 + o.count > s.n || o.slot < 0 || o.slot + o.count > (int)sl.size()) return fail("bad crop range");
        for (int i = 0; i < o.count; ++i) {
          if (source(o, i) != o.img0 + i) return fail("crops read the wrong image");
          if (sl[o.slot + i] != -1) return fail("crop written over a waiting crop");
          sl[o.slot + i] = o.img0 + i;
        }
      } else if (o.kind == OP_CLIP_TOWER || o.kind == OP_SAMP_NETS) {
        const bool sp = o.kind == OP_SAMP_NETS;
        std::vector<int>& sl = slots[sp];
        if (o.count < 1 || o.count > (sp ? s.samp_chunk : s.clip_chunk) || o.img0 < 0 || o.img0 + o.count > s.n) return fail("bad model range");
        for (int i = 0; i < o.count; ++i) {
          if (sl[i] != o.img0 + i) return fail("model result lands at another image's offset");
          seen[sp ? 2 : 1][o.img0 + i] += 1;
          sl[i] = -1;
        }
      } else if (o.kind == OP_CLIP_COMPACT || o.kind == OP_SAMP_COMPACT) {
        std::vector<int>& sl = slots[o.kind == OP_SAMP_COMPACT];
        if (o.count < 1 || o.left < 1 || o.count + o.left > (int)sl.size()) return fail("bad compaction");
        for (int i = 0; i < o.left; ++i) {   // ascending pieces, as the copies are issued
          if (sl[i] != -1) return fail("compaction over a waiting crop");
          sl[i] = sl[o.count + i];
          sl[o.count + i] = -1;
        }
      } else if (o.kind == OP_INTERLEAVE) {
        const bool on[3] = {s.topiq, s.clip, s.samp};
        for (int m = 0; m < 3; ++m)
          for (int i = 0; i < s.n; ++i)
            if (seen[m][i] != (on[m] ? 1 : 0)) return fail("image " + std::to_string(i) + " went through model " + std::to_string(m) + " " + std::to_string(seen[m][i]) + " times");
      } else {
        return fail("unknown operation");
      }
    }
    return true;
  }
};

bool check(const Shape& s, const std::vector<Op>& ops, std::string* why) {
  Checker c(s, ops);
  const bool ok = c.run();
  if (why) *why = c.why;
  return ok;
}

Shape shape(int n, int mb, int samp_chunk, bool on_device, int mask, bool overlap, int variant = 0) {
  Shape s;
  s.clip_side = variant != 2; s.samp_side = variant != 1; s.samp_first = variant == 3;   // 0: both on the side lane, CLIP first
  s.n = n; s.mb = mb; s.on_device = on_device; s.overlap = overlap;
  s.topiq = mask & 1; s.clip = mask & 2; s.samp = mask & 4;
  s.clip_chunk = fe::clip_tower_chunk(1024, 257, n);      // ViT-L/14
  s.samp_chunk = std::min(n, samp_chunk);
  return s;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "check" && argc == 3) {
    const bool on_device = atoi(argv[2]) != 0;
    const int ns[] = {1, 2, 31, 32, 33, 45, 127, 128, 129, 256, 300}, mbs[] = {1, 8, 32, 64, 200}, scs[] = {1, 27, 128};
    int plans = 0;
    for (int n : ns)
      for (int mb : mbs)
        for (int sc : scs)
          for (int mask : {7, 3, 5})
            for (int v = 0; v < 5; ++v) {      // one lane; two lanes in the four variants of Shape
              const int overlap = v > 0;
              const Shape s = shape(n, mb, sc, on_device, mask, overlap != 0, v > 0 ? v - 1 : 0);
              const std::vector<Op> ops = build(s);
              std::string why;
              if (!check(s, ops, &why)) {
                printf("FAILED n=%d mb=%d samp_chunk=%d on_device=%d mask=%d lanes variant=%d: %s\n", n, mb, sc, (int)on_device, mask, v, why.c_str());
                return 1;
              }
              bool side = false;
              for (const Op& o : ops) side = side || o.lane == LANE_SIDE;
              if (side != (overlap != 0 && ((s.clip && s.clip_side) || (s.samp && s.samp_side)))) { printf("FAILED: side lane use does not follow the overlap switch\n"); return 1; }
              ++plans;
            }
    printf("%d plans ok\n", plans);
    return 0;
  }
  if (mode == "drop" && argc == 6) {
    const Shape s = shape(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) != 0, 7, true);
    const std::vector<Op> ops = build(s);
    if (!check(s, ops, nullptr)) { printf("the whole plan fails\n"); return 1; }
    int waits = 0, detected = 0;
    for (size_t i = 0; i < ops.size(); ++i) {
      if (ops[i].kind != OP_WAIT) continue;
      std::vector<Op> cut = ops;
      cut.erase(cut.begin() + (long)i);
      std::string why;
      ++waits;
      if (!check(s, cut, &why)) ++detected;
      else printf("not noticed: wait %zu (lane %d, event %d)\n", i, ops[i].lane, ops[i].event);
    }
    printf("waits %d detected %d\n", waits, detected);
    return waits == detected ? 0 : 1;
  }
  fprintf(stderr, "usage: %s check <on_device> | drop <n> <mb> <samp_chunk> <on_device>\n", argv[0]);
  return 2;
}
