// What the translation units of the C ABI (capi.hip, capi_<domain>.hip) share: the context, the entry-point guard, the staging helpers.
#pragma once
#include "../../include/facet_engine.h"
#include "engine.h"
#include "mixed_list.h"
#include "onnx_graph.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <tuple>
#include <type_traits>

using namespace fe;

// Below the first group, each group of fields is kept by the one file named above it; fe_destroy (capi.hip) releases them all.
struct fe_ctx {
  Ctx c;
  int microbatch = 8;
  hipEvent_t t0 = nullptr, t1 = nullptr;   // capi.hip: fe_timer_*, fe_bench_conv
  // double-buffered H2D staging of uint8 micro-batches on a copy stream (host-buffer entry points): the copy of
  // micro-batch k+1 is issued right after the kernels of micro-batch k were queued, so PCIe overlaps compute (ImageStager)
  hipStream_t copy_stream = nullptr;
  uint8_t* stage_buf[2] = {nullptr, nullptr};
  size_t stage_cap[2] = {0, 0};
  hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
  // capi_face.hip: device copies of OpenCV's interpolation tables (built once / per size)
  short* warp_wtab = nullptr;
  struct CvResizeTab { int* ofs; short* coef; };
  std::map<std::tuple<int, int, int>, CvResizeTab> cvresize;   // (src, dst, clamp) -> tables
  // capi_image.hip
  int* hsv_sdiv = nullptr; int* hsv_hdiv = nullptr;   // cv2 HSV division tables
  double* phash_cos = nullptr;                        // DCT-II cosine table of fe_phash
  uint8_t* lines_maps = nullptr; size_t lines_maps_cap = 0;   // fe_leading_lines_mixed: pinned host buffer of a chunk's maps (grow-only, at most 256 MiB)
  double lines_host_ms = 0.0;                         // fe_lines_host_ms: what the host stage of the last leading-lines call took
  int stats_segment = 0;                              // fe_set_stats_segment: pixels per pass-1 segment of fe_image_stats_mixed, 0 = default
  std::vector<void*> misc_allocs;                     // these tables and capi_face.hip's, for fe_destroy
  // capi_models.hip
  float* clip_in = nullptr;  // preprocessed CLIP crops waiting for a full tower batch (ClipBatcher)
  size_t clip_in_cap = 0;
  float* samp_in = nullptr;  // same for the SAMP-Net / U2-Net-P crops (SampBatcher)
  size_t samp_in_cap = 0;
  float* d_rec = nullptr;   // interleaved ensemble records of the host-output entry point
  size_t d_rec_cap = 0;
  void* mixed_buf = nullptr;   // descriptors and table pool of the mixed-size call on the stack (fe_ensemble_score_mixed,
  size_t mixed_cap = 0;        // fe_preprocess224_mixed); grows to the largest call, never per image size
  int ensemble_mask = 7;    // models fe_ensemble_score runs when loaded: 1 topiq | 2 clip | 4 samp (fe_ensemble_select)
  // the side lane of ensemble_run: a second stream with an arena of its own, on which the 224^2 models run beside TOPIQ. Created on
  // first use; idle whenever ensemble_run is not on the stack (it joins before it returns)
  struct SideLane {
    hipStream_t stream = nullptr;
    Arena arena;
    hipEvent_t ev_start = nullptr, ev_join = nullptr, ev_read[2] = {nullptr, nullptr};   // ev_read: its last read of a ping-pong buffer
  } side;
  // capi_tags.hip: the one tag vocabulary of the context (fe_tag_vocab_set), packed once; freed with the context
  struct TagVocab {
    DeviceWeights dw;                 // owns w's rows, perm and goff
    ConvW w;                          // the text rows [T][d] as a Linear without bias
    int32_t* perm = nullptr;          // device [T]: prompts sorted by (tag, prompt index)
    int32_t* goff = nullptr;          // device [G + 1]: CSR offsets of the tags in perm
    int T = 0, G = 0, d = 0;
  };
  std::unique_ptr<TagVocab> tag_vocab;
  int tag_chunk = 0;                  // fe_set_tag_chunk: rows per chunk of fe_tag_select / fe_tag_select_sims, 0 = sized from the arena
  // capi_models.hip and capi_face.hip, through out_buf()
  float* d_out = nullptr;   // persistent device staging for per-image results
  size_t d_out_cap = 0;
  float* out_buf(size_t floats) {
    if (floats > d_out_cap) {
      if (d_out) (void)hipFree(d_out);
      d_out = nullptr; d_out_cap = 0;
      FE_HIP(hipMalloc((void**)&d_out, floats * sizeof(float)));
      d_out_cap = floats;
    }
    return d_out;
  }
};

// Walks a uint8 image batch micro-batch by micro-batch. Device-resident input: pointer arithmetic. Host input: ping-pong
// device buffers filled on the copy stream; get(k) makes the compute stream wait for chunk k, done(k) marks its last
// consumer and starts the copy of chunk k+1 (which then runs under the kernels just queued for chunk k).
class ImageStager {
 public:
  ImageStager(fe_ctx* ctx, const uint8_t* imgs, int n, size_t per_image, int mb, int on_device)
      : x_(ctx), imgs_(imgs), n_(n), per_(per_image), mb_(mb), dev_(on_device) {
    if (!dev_) {
      prepare(x_, (size_t)std::min(mb_, n_) * per_);
      issue(0);
    }
  }
  // the copy stream, its events and two staging buffers of at least `need` bytes (ensemble_run issues its copies itself)
  static void prepare(fe_ctx* x, size_t need) {
    if (!x->copy_stream) {
      FE_HIP(hipStreamCreateWithFlags(&x->copy_stream, hipStreamNonBlocking));
      for (int i = 0; i < 2; ++i) {
        FE_HIP(hipEventCreateWithFlags(&x->ev_copied[i], hipEventDisableTiming));
        FE_HIP(hipEventCreateWithFlags(&x->ev_consumed[i], hipEventDisableTiming));
      }
    }
    for (int i = 0; i < 2; ++i)
      if (x->stage_cap[i] < need) {
        FE_HIP(hipStreamSynchronize(x->c.stream));
        if (x->stage_buf[i]) FE_HIP(hipFree(x->stage_buf[i]));
        x->stage_buf[i] = nullptr; x->stage_cap[i] = 0;
        FE_HIP(hipMalloc((void**)&x->stage_buf[i], need));
        x->stage_cap[i] = need;
      }
  }
  int chunks() const { return (n_ + mb_ - 1) / mb_; }
  int count(int k) const { return std::min(mb_, n_ - k * mb_); }
  const uint8_t* get(int k) {
    if (dev_) return imgs_ + (size_t)k * mb_ * per_;
    FE_HIP(hipStreamWaitEvent(x_->c.stream, x_->ev_copied[k & 1], 0));
    return x_->stage_buf[k & 1];
  }
  void done(int k) {
    if (dev_) return;
    FE_HIP(hipEventRecord(x_->ev_consumed[k & 1], x_->c.stream));
    consumed_[k & 1] = true;
    if (k + 1 < chunks()) issue(k + 1);
  }
 private:
  void issue(int k) {
    const int b = k & 1;
    if (consumed_[b]) FE_HIP(hipStreamWaitEvent(x_->copy_stream, x_->ev_consumed[b], 0));
    FE_HIP(hipMemcpyAsync(x_->stage_buf[b], imgs_ + (size_t)k * mb_ * per_, (size_t)count(k) * per_, hipMemcpyHostToDevice,
                          x_->copy_stream));
    FE_HIP(hipEventRecord(x_->ev_copied[b], x_->copy_stream));
  }
  fe_ctx* x_; const uint8_t* imgs_; int n_; size_t per_; int mb_, dev_;
  bool consumed_[2] = {false, false};
};

// ---- the guard of every entry point that takes a context -------------------------------------------------------------------------
// On the error path nothing may stay in flight: queued async copies read the caller's host buffers and write into host
// vectors local to the entry point, both of which die when it returns.
// The side lane's kernels also run in an arena that the next call recycles. (By the time an exception reaches the guard, LaneScope has
// put the main stream and arena back into the Ctx.)
inline void fe_drain(fe_ctx* ctx) {
  if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
  if (ctx->side.stream) (void)hipStreamSynchronize(ctx->side.stream);
  if (ctx->c.stream) (void)hipStreamSynchronize(ctx->c.stream);
}

// While it lives, the Ctx enqueues on the side lane: c.stream and c.arena are the side lane's, and the main pair waits in ctx->side.
// The model code reads both members of the Ctx it is handed; all enqueueing happens on one host thread in program order.
class LaneScope {
 public:
  explicit LaneScope(fe_ctx* ctx, bool on_side) : x_(on_side ? ctx : nullptr) { flip(); }
  ~LaneScope() { flip(); }
  LaneScope(const LaneScope&) = delete;
  LaneScope& operator=(const LaneScope&) = delete;
 private:
  void flip() {
    if (!x_) return;
    std::swap(x_->c.stream, x_->side.stream);
    x_->c.arena.swap(x_->side.arena);
  }
  fe_ctx* x_;
};

// thrown by the JPEG writers when an output row is too small for its image
struct CapacityError : std::runtime_error { using std::runtime_error::runtime_error; };

// Which failures of an entry point are FE_ERR_CAPACITY; every other exception is FE_ERR_RUNTIME.
enum class OnError {
  Runtime,       // none
  Capacity,      // a thrown CapacityError (the thumbnail and JPEG encode entry points)
  VlmCapacity    // a failure to fit (arena, device memory, KV-cache capacity) by its message: the padded-batch image path of the VLM
                 // families, so a caller can retry with fewer images
};
inline bool vlm_capacity_error(const char* msg) {
  return strstr(msg, "arena exhausted") || strstr(msg, "out of memory") || strstr(msg, "do not fit") || strstr(msg, "max_seq <= 8192");
}

// Runs `body` as the entry point's work. A null context is FE_ERR_INVALID. Every entry point re-selects the context's device: the
// calling thread may share the process with torch / RCCL. body returns nothing (FE_OK) or an fe_status (an early `return FE_OK;`, or
// FE_ERR_NOT_LOADED / FE_ERR_INVALID after storing the message in ctx->c.err). An exception leaves what() in ctx->c.err, drains the
// streams and returns the code `policy` gives it.
template <class F>
int fe_api(fe_ctx* ctx, OnError policy, F&& body) {
  if (!ctx) return FE_ERR_INVALID;
  try {
    (void)hipSetDevice(ctx->c.device);
    if constexpr (std::is_void_v<decltype(body())>) {
      body();
      return FE_OK;
    } else {
      return body();
    }
  } catch (const std::exception& e) {
    ctx->c.err = e.what();
    fe_drain(ctx);
    const bool capacity = (policy == OnError::Capacity && dynamic_cast<const CapacityError*>(&e)) ||
                          (policy == OnError::VlmCapacity && vlm_capacity_error(e.what()));
    return capacity ? FE_ERR_CAPACITY : FE_ERR_RUNTIME;
  }
}
template <class F>
int fe_api(fe_ctx* ctx, F&& body) { return fe_api(ctx, OnError::Runtime, body); }

// ---- host data into the arena ---------------------------------------------------------------------------------------------------
// n elements of a host array into the arena, copied on the stream (src == nullptr: nothing, nullptr)
template <class T>
T* upload(Ctx& C, const T* src, size_t n) {
  if (!src) return nullptr;
  T* d = (T*)C.arena.alloc(n * sizeof(T));
  FE_HIP(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, C.stream));
  return d;
}
// p itself when it is device memory, its arena copy otherwise
template <class T>
const T* resident(Ctx& C, const T* p, size_t n, int on_device) { return on_device ? p : upload(C, p, n); }

// host fp32 NCHW -> arena NHWC tensor of element type T with cpad channels, and back (synchronises)
template <class T = float>
TensorT<T> upload_nchw(Ctx& c, const float* x, int n, int ch, int h, int w, int cpad) {
  const size_t elems = (size_t)n * ch * h * w;
  float* tmp = (float*)c.arena.alloc(elems * sizeof(float));
  FE_HIP(hipMemcpyAsync(tmp, x, elems * sizeof(float), hipMemcpyHostToDevice, c.stream));
  TensorT<T> t = c.arena.tensor_t<T>(n, h, w, cpad);
  launch_nchw_to_nhwc(tmp, t.p, n, ch, h, w, cpad, c.stream);
  return t;
}
template <class T>
void download_nchw(Ctx& c, const TensorT<T>& t, int ch, float* y) {
  const size_t elems = (size_t)t.n * ch * t.h * t.w;
  float* tmp = (float*)c.arena.alloc(elems * sizeof(float));
  launch_nhwc_to_nchw(t.p, t.ld, tmp, t.n, ch, t.h, t.w, c.stream);
  FE_HIP(hipMemcpyAsync(y, tmp, elems * sizeof(float), hipMemcpyDeviceToHost, c.stream));
  FE_HIP(hipStreamSynchronize(c.stream));
}

// ---- the list front end of the mixed-size entry points: check, stage, refuse (mixed_list.h has the host half) ---------------------------
// What an entry point accepts of an image: min_side <= h <= max_h, min_side <= w <= max_w, h * w <= max_pixels (`pixels` says that
// bound in the message; nullptr: there is none).
struct MixedLimits {
  int min_side, max_h, max_w;
  size_t max_pixels;
  const char* pixels;
};
constexpr MixedLimits kAnySideBelow2_31 = {1, INT32_MAX, INT32_MAX, ((size_t)1 << 31) - 1, "below 2^31"};

// What the mixed-size entry points check alike: the list (`list` is null when it or an output of the call is), the order and every
// image's pointer and size. false: FE_ERR_INVALID with the message in the context.
inline bool mixed_list_ok(Ctx& C, const char* who, const void* list, const int32_t* hw, int n, int order, const uint8_t* const* images, const MixedLimits& lim) {
  char b[240];
  if (!list || !hw || n <= 0) {
    snprintf(b, sizeof b, "%s: bad arguments (null list, null output or n <= 0)", who);
    C.err = b;
    return false;
  }
  if (order != FE_ORDER_BGR && order != FE_ORDER_RGB) {
    snprintf(b, sizeof b, "%s: order %d is neither FE_ORDER_BGR (0) nor FE_ORDER_RGB (1)", who, order);
    C.err = b;
    return false;
  }
  for (int i = 0; i < n; ++i) {
    const int h = hw[2 * i], w = hw[2 * i + 1];
    if (!images[i]) { snprintf(b, sizeof b, "%s: image %d is a null pointer", who, i); C.err = b; return false; }
    if (h < lim.min_side || w < lim.min_side || h > lim.max_h || w > lim.max_w || (size_t)h * (size_t)w > lim.max_pixels) {
      snprintf(b, sizeof b, "%s: image %d is %d x %d (h x w); h must be within %d .. %d and w within %d .. %d%s%s", who, i, h, w, lim.min_side, lim.max_h,
               lim.min_side, lim.max_w, lim.pixels ? ", h * w " : "", lim.pixels ? lim.pixels : "");
      C.err = b;
      return false;
    }
  }
  return true;
}

// Images [i0, i1) of the list where the kernels read them, handed to put(i, pointer): the caller's own pointer when the images are
// resident; else the host images lie anywhere, so one copy each on the stream, to base + off[i - i0] (mixed_list::staged_offsets).
template <class Put>
void stage_images(Ctx& C, const uint8_t* const* images, const int32_t* hw, int i0, int i1, int on_device, uint8_t* base, const size_t* off, Put&& put) {
  for (int i = i0; i < i1; ++i) {
    const uint8_t* src = images[i];
    if (!on_device) {
      uint8_t* d = base + off[i - i0];
      FE_HIP(hipMemcpyAsync(d, src, mixed_list::image_bytes(hw, i), hipMemcpyHostToDevice, C.stream));
      src = d;
    }
    put(i, src);
  }
}

// the FE_ERR_CAPACITY of an image whose own scratch exceeds the arena
[[noreturn]] inline void throw_image_too_large(const char* who, int i, const int32_t* hw, size_t bytes, size_t capacity) {
  char b[240];
  snprintf(b, sizeof b, "%s: image %d (%d x %d) needs %zu bytes of scratch, the arena holds %zu", who, i, hw[2 * i], hw[2 * i + 1], bytes, capacity);
  throw CapacityError(b);
}

// capi_graph.hip: the loaded graph of a slot, or an exception that names the slot
GraphSlot& graph_slot(fe_ctx* ctx, int slot);
