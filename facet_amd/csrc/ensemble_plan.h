// The schedule of one ensemble call as data. Host only (no HIP headers): ensemble_run (capi_models.hip) executes the list,
// tests/native/ensemble_plan_harness.cpp replays it on simulated in-order queues and checks every cross-queue hazard.
//
// Three in-order queues: MAIN (TOPIQ, the clear of the result planes, the final interleave), SIDE (the 224^2 models: CLIP tower +
// aesthetic head, U2-Net-P + SAMP-Net; its own stream and arena) and COPY (host input only: H2D of the ping-pong staging buffers).
// With `overlap` off every SIDE operation is issued on MAIN instead and the start / join edges disappear: the serial path.
// An event wait orders the waiting queue behind the LAST record of that event issued before the wait, in list (= host issue) order.
#pragma once
#include <algorithm>
#include <vector>

namespace fe {

// Images per launch of the CLIP ViT tower: the largest count in (hi - 40, hi] whose GEMM rows (count x tokens, 128-row tiles x
// width / 128 column tiles) fill whole rounds of 256 workgroups best; small batches go as one launch.
inline int clip_tower_chunk(int width, int tokens, int n) {
  if (n <= 40) return n;
  const int hi = std::min(n, 128), lo = std::max(32, hi - 40), ntile = std::max(1, width / 128);
  int best = hi;
  double best_eff = 0.0;
  for (int c = hi; c >= lo; --c) {
    const long wgs = (((long)c * tokens + 127) / 128) * ntile;
    const double eff = (double)wgs / (double)(((wgs + 255) / 256) * 256);
    if (eff > best_eff + 1e-9) { best_eff = eff; best = c; }
  }
  return best;
}

namespace plan {

enum Lane : int { LANE_MAIN = 0, LANE_SIDE = 1, LANE_COPY = 2, N_LANES = 3 };
enum Kind : int {
  OP_CLEAR,         // zero the result planes
  OP_COPY_IN,       // host input: H2D of micro-batch `mb` into its ping-pong buffer
  OP_TOPIQ,         // TOPIQ on micro-batch `mb`: images [img0, img0 + count)
  OP_CLIP_PRE,      // 224^2 CLIP crops of micro-batch `mb` into staging slots [slot, slot + count)
  OP_CLIP_TOWER,    // tower + normalise + aesthetic head on staging slots [0, count): results of images [img0, img0 + count)
  OP_CLIP_COMPACT,  // staging slots [count, count + left) move to [0, left)
  OP_SAMP_PRE, OP_SAMP_NETS, OP_SAMP_COMPACT,   // the same three for U2-Net-P + SAMP-Net
  OP_RECORD, OP_WAIT,                           // `event` on `lane`
  OP_INTERLEAVE     // result planes -> records
};
enum Region : int { R_STAGE0, R_STAGE1, R_CLIP_IN, R_SAMP_IN, R_OUT_TOPIQ, R_OUT_CLIP, R_OUT_SAMP, R_ARENA_MAIN, R_ARENA_SIDE };
enum Event : int { EV_START, EV_JOIN, EV_COPIED0, EV_COPIED1, EV_CONSUMED0, EV_CONSUMED1, EV_SIDE_READ0, EV_SIDE_READ1, N_EVENTS };

// [lo, hi) of a region: images of the micro-batch (stage buffers), crop slots (staging), image indices (result planes), {0, 1} (arenas)
struct Access { int region, lo, hi; bool write; };
struct Op {
  int kind = OP_CLEAR, lane = LANE_MAIN;
  int mb = 0, img0 = 0, count = 0;   // micro-batch index; first image / crop count (see Kind)
  int slot = 0, left = 0;            // OP_*_PRE: first staging slot written; OP_*_COMPACT: crops moved
  int event = -1;
  Access acc[3];
  int n_acc = 0;
  void touch(int region, int lo, int hi, bool write) { acc[n_acc++] = Access{region, lo, hi, write}; }
};

struct Shape {
  int n = 0, mb = 1;                       // images, micro-batch
  int clip_chunk = 1, samp_chunk = 1;      // crops per tower / per U2-Net-P + SAMP-Net launch
  bool on_device = true;                   // device-resident input (no COPY queue)
  bool topiq = true, clip = true, samp = true;
  bool overlap = true;
  // which of the two 224^2 models ride the side lane when `overlap` is on (the other stays on MAIN), and which is issued first
  bool clip_side = true, samp_side = true, samp_first = false;
};

class Builder {
 public:
  explicit Builder(const Shape& s) : s_(s), side_(s.overlap && ((s.clip && s.clip_side) || (s.samp && s.samp_side)) ? LANE_SIDE : LANE_MAIN) {}
  std::vector<Op> build() {
    const bool two = side_ == LANE_SIDE;
    const int chunks = (s_.n + s_.mb - 1) / s_.mb;
    Op clr = op(OP_CLEAR, LANE_MAIN);
    clr.touch(R_OUT_TOPIQ, 0, s_.n, true); clr.touch(R_OUT_CLIP, 0, s_.n, true); clr.touch(R_OUT_SAMP, 0, s_.n, true);
    ops_.push_back(clr);
    if (two) { sync(OP_RECORD, LANE_MAIN, EV_START); sync(OP_WAIT, LANE_SIDE, EV_START); }
    if (!s_.on_device) copy_in(0);
    for (int k = 0; k < chunks; ++k) {
      const int b = k & 1;
      if (!s_.on_device) {
        sync(OP_WAIT, LANE_MAIN, EV_COPIED0 + b);
        if (two) sync(OP_WAIT, LANE_SIDE, EV_COPIED0 + b);
      }
      // two lanes: the side work of a micro-batch is issued first, so the side queue fills while MAIN still holds the previous
      // micro-batch and (device-resident input) its crops run ahead of TOPIQ's loop; one lane: the order TOPIQ, CLIP, SAMP
      if (!two) topiq(k);
      if (s_.samp && s_.samp_first) crops(k, OP_SAMP_PRE, R_SAMP_IN, R_OUT_SAMP, s_.samp_chunk, samp_);
      if (s_.clip) crops(k, OP_CLIP_PRE, R_CLIP_IN, R_OUT_CLIP, s_.clip_chunk, clip_);
      if (s_.samp && !s_.samp_first) crops(k, OP_SAMP_PRE, R_SAMP_IN, R_OUT_SAMP, s_.samp_chunk, samp_);
      if (two && !s_.on_device) sync(OP_RECORD, LANE_SIDE, EV_SIDE_READ0 + b);
      if (two) topiq(k);
      if (!s_.on_device) {
        sync(OP_RECORD, LANE_MAIN, EV_CONSUMED0 + b);
        if (k + 1 < chunks) copy_in(k + 1);
      }
    }
    if (s_.samp && s_.samp_first) while (samp_.count > 0) run(OP_SAMP_PRE, R_SAMP_IN, R_OUT_SAMP, std::min(samp_.count, s_.samp_chunk), samp_);
    if (s_.clip) while (clip_.count > 0) run(OP_CLIP_PRE, R_CLIP_IN, R_OUT_CLIP, std::min(clip_.count, s_.clip_chunk), clip_);
    if (s_.samp && !s_.samp_first) while (samp_.count > 0) run(OP_SAMP_PRE, R_SAMP_IN, R_OUT_SAMP, std::min(samp_.count, s_.samp_chunk), samp_);
    if (two) { sync(OP_RECORD, LANE_SIDE, EV_JOIN); sync(OP_WAIT, LANE_MAIN, EV_JOIN); }
    Op il = op(OP_INTERLEAVE, LANE_MAIN);
    il.count = s_.n;
    il.touch(R_OUT_TOPIQ, 0, s_.n, false); il.touch(R_OUT_CLIP, 0, s_.n, false); il.touch(R_OUT_SAMP, 0, s_.n, false);
    ops_.push_back(il);
    return ops_;
  }

 private:
  struct Gather { int count = 0, done = 0; };   // crops waiting in a staging buffer, images already through the model
  Op op(int kind, int lane) const { Op o; o.kind = kind; o.lane = lane; return o; }
  int nb(int k) const { return std::min(s_.mb, s_.n - k * s_.mb); }
  int arena(int lane) const { return lane == LANE_SIDE ? R_ARENA_SIDE : R_ARENA_MAIN; }
  int lane_of(int pre) const { return (pre == OP_CLIP_PRE ? s_.clip_side : s_.samp_side) ? side_ : (int)LANE_MAIN; }
  void sync(int kind, int lane, int event) { Op o = op(kind, lane); o.event = event; ops_.push_back(o); }
  void copy_in(int k) {
    const int b = k & 1;
    if (k >= 2) {   // the buffer still holds micro-batch k - 2: behind its last reader on every lane that reads it
      sync(OP_WAIT, LANE_COPY, EV_CONSUMED0 + b);
      if (side_ == LANE_SIDE) sync(OP_WAIT, LANE_COPY, EV_SIDE_READ0 + b);
    }
    Op o = op(OP_COPY_IN, LANE_COPY);
    o.mb = k; o.img0 = k * s_.mb; o.count = nb(k);
    o.touch(R_STAGE0 + b, 0, nb(k), true);
    ops_.push_back(o);
    sync(OP_RECORD, LANE_COPY, EV_COPIED0 + b);
  }
  void topiq(int k) {
    if (!s_.topiq) return;
    Op o = op(OP_TOPIQ, LANE_MAIN);
    o.mb = k; o.img0 = k * s_.mb; o.count = nb(k);
    if (!s_.on_device) o.touch(R_STAGE0 + (k & 1), 0, nb(k), false);
    o.touch(R_OUT_TOPIQ, o.img0, o.img0 + o.count, true);
    o.touch(R_ARENA_MAIN, 0, 1, true);
    ops_.push_back(o);
  }
  // pre: OP_CLIP_PRE or OP_SAMP_PRE; the model and compaction kinds follow it in Kind
  void crops(int k, int pre, int staging, int out, int chunk, Gather& g) {
    const int lane = lane_of(pre);
    Op o = op(pre, lane);
    o.mb = k; o.img0 = k * s_.mb; o.count = nb(k); o.slot = g.count;
    if (!s_.on_device) o.touch(R_STAGE0 + (k & 1), 0, nb(k), false);
    o.touch(staging, g.count, g.count + o.count, true);
    o.touch(arena(lane), 0, 1, true);
    ops_.push_back(o);
    g.count += o.count;
    while (g.count >= chunk) run(pre, staging, out, chunk, g);
  }
  void run(int pre, int staging, int out, int c, Gather& g) {
    const int lane = lane_of(pre);
    Op o = op(pre + 1, lane);
    o.img0 = g.done; o.count = c;
    o.touch(staging, 0, c, false);
    o.touch(out, g.done, g.done + c, true);
    o.touch(arena(lane), 0, 1, true);
    ops_.push_back(o);
    const int left = g.count - c;
    if (left > 0) {
      Op m = op(pre + 2, lane);
      m.count = c; m.left = left;
      m.touch(staging, c, c + left, false);
      m.touch(staging, 0, left, true);
      ops_.push_back(m);
    }
    g.done += c;
    g.count = left;
  }
  Shape s_;
  int side_;
  Gather clip_, samp_;
  std::vector<Op> ops_;
};

inline std::vector<Op> build(const Shape& s) { return Builder(s).build(); }

}  // namespace plan
}  // namespace fe
