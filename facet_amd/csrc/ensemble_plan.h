// The schedule of one ensemble call as data. Host only (no HIP headers): ensemble_run (capi_models.hip) executes the list,
// tests/native/ensemble_plan_harness.cpp replays it on simulated in-order queues and checks every cross-queue hazard.
//
// Three in-order queues: MAIN (TOPIQ, the clear of the result planes, the final interleave), SIDE (the 224^2 models: CLIP tower +
// aesthetic head, U2-Net-P + SAMP-Net; its own stream and arena) and COPY (host input only: H2D of the ping-pong staging buffers).
// With `overlap` off every SIDE operation is issued on MAIN instead and the start / join edges disappear: the serial path.
// An event wait orders the waiting queue behind the LAST record of that event issued before the wait, in list (= host issue) order.
//
// A call on images of mixed sizes (fe_ensemble_score_mixed) is the same schedule over a list of micro-batch cuts (cut_mixed): the images
// are taken in grouped order ("positions": by shape in order of first appearance when TOPIQ runs, the input order otherwise), every
// image index of an operation below is a position, and the interleave puts the records back into input order. build(Shape) is
// build(Shape, cuts) with the uniform cuts of ceil(n / mb) micro-batches, operation for operation.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
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
  OP_INTERLEAVE,    // result planes -> records (a mixed call: position -> input order)
  OP_GATHER         // mixed call, device input: the images of TOPIQ's micro-batch `mb` do not lie back to back, D2D into its staging buffer
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

// One micro-batch of a cut list: `count` images (1 .. Shape::mb) from the position where the previous cut ended. gather: device input whose
// images TOPIQ cannot take in place.
struct Cut { int count = 0; bool gather = false; };

class Builder {
 public:
  explicit Builder(const Shape& s, const std::vector<Cut>* cuts = nullptr)
      : s_(s), side_(s.overlap && ((s.clip && s.clip_side) || (s.samp && s.samp_side)) ? LANE_SIDE : LANE_MAIN) {
    if (cuts) cuts_ = *cuts;
    else for (int i = 0; i < s.n; i += s.mb) cuts_.push_back(Cut{std::min(s.mb, s.n - i), false});
    first_.assign(cuts_.size() + 1, 0);
    for (size_t k = 0; k < cuts_.size(); ++k) first_[k + 1] = first_[k] + cuts_[k].count;
  }
  std::vector<Op> build() {
    const bool two = side_ == LANE_SIDE;
    const int chunks = (int)cuts_.size();
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
  int nb(int k) const { return cuts_[k].count; }
  int first(int k) const { return first_[k]; }
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
    o.mb = k; o.img0 = first(k); o.count = nb(k);
    o.touch(R_STAGE0 + b, 0, nb(k), true);
    ops_.push_back(o);
    sync(OP_RECORD, LANE_COPY, EV_COPIED0 + b);
  }
  void topiq(int k) {
    if (!s_.topiq) return;
    const bool gathered = s_.on_device && cuts_[k].gather;   // MAIN is the only queue that touches the staging buffers of device input
    if (gathered) {
      Op g = op(OP_GATHER, LANE_MAIN);
      g.mb = k; g.img0 = first(k); g.count = nb(k);
      g.touch(R_STAGE0 + (k & 1), 0, nb(k), true);
      ops_.push_back(g);
    }
    Op o = op(OP_TOPIQ, LANE_MAIN);
    o.mb = k; o.img0 = first(k); o.count = nb(k);
    if (!s_.on_device || gathered) o.touch(R_STAGE0 + (k & 1), 0, nb(k), false);
    o.touch(R_OUT_TOPIQ, o.img0, o.img0 + o.count, true);
    o.touch(R_ARENA_MAIN, 0, 1, true);
    ops_.push_back(o);
  }
  // pre: OP_CLIP_PRE or OP_SAMP_PRE; the model and compaction kinds follow it in Kind
  void crops(int k, int pre, int staging, int out, int chunk, Gather& g) {
    const int lane = lane_of(pre);
    Op o = op(pre, lane);
    o.mb = k; o.img0 = first(k); o.count = nb(k); o.slot = g.count;
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
  std::vector<Cut> cuts_;
  std::vector<int> first_;   // position of the first image of each cut, and n
  std::vector<Op> ops_;
};

inline std::vector<Op> build(const Shape& s) { return Builder(s).build(); }
// the cuts must cover s.n images, each with 1 .. s.mb of them
inline std::vector<Op> build(const Shape& s, const std::vector<Cut>& cuts) { return Builder(s, &cuts).build(); }

// The cut list of a call on images of mixed sizes. hw [n][2] = (h, w) of every image; addr (nullable) = the device address of every image.
// by_shape (TOPIQ selected): the images are grouped by shape in order of first appearance, input order kept within a group, and a
// micro-batch never crosses a group; its gather flag is set when addr is given and its images are not consecutive in memory (or do not
// start on a 4-byte boundary). Otherwise
// the micro-batches are plain slices of the list, mixed shapes and all. order [position] = input index.
struct MixedCuts {
  std::vector<int> order;
  std::vector<Cut> cuts;
};
inline MixedCuts cut_mixed(const int32_t* hw, int n, int mb, bool by_shape, const uintptr_t* addr) {
  MixedCuts m;
  std::vector<std::vector<int>> groups;
  if (by_shape) {
    std::map<std::pair<int32_t, int32_t>, size_t> seen;
    for (int i = 0; i < n; ++i) {
      auto it = seen.emplace(std::make_pair(hw[2 * i], hw[2 * i + 1]), groups.size());
      if (it.second) groups.emplace_back();
      groups[it.first->second].push_back(i);
    }
  } else {
    groups.emplace_back();
    for (int i = 0; i < n; ++i) groups[0].push_back(i);
  }
  for (const std::vector<int>& g : groups)
    for (size_t i0 = 0; i0 < g.size(); i0 += (size_t)mb) {
      Cut c;
      c.count = (int)std::min<size_t>((size_t)mb, g.size() - i0);
      for (int j = 0; j < c.count; ++j) {
        const int i = g[i0 + j];
        // TOPIQ's first kernel reads its batch in 4-byte words: a micro-batch that starts at an odd address is gathered too
        if (by_shape && addr && (j > 0 ? addr[i] != addr[g[i0 + j - 1]] + (uintptr_t)hw[2 * i] * (uintptr_t)hw[2 * i + 1] * 3 : (addr[i] & 3) != 0)) c.gather = true;
        m.order.push_back(i);
      }
      m.cuts.push_back(c);
    }
  return m;
}

}  // namespace plan
}  // namespace fe
