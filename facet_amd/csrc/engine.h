// Engine-side runtime: context, weight store, layer builders and the model graphs of the hot path.
#pragma once
#include "fe_common.h"
#include "../../include/facet_engine.h"   // fe_sim_rows
#include <memory>
#include <tuple>

namespace fe {

// Host copy of one named checkpoint tensor (fp32, contiguous, PyTorch layout).
struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
  size_t numel() const { size_t n = 1; for (auto d : shape) n *= (size_t)d; return n; }
};

class WeightStore {
 public:
  void clear() { t_.clear(); }
  void set(const std::string& name, const float* data, const int64_t* shape, int ndim);
  bool has(const std::string& name) const { return t_.count(name) != 0; }
  const HostTensor& get(const std::string& name) const;
  size_t size() const { return t_.size(); }
 private:
  std::map<std::string, HostTensor> t_;
};

// Owns device copies of packed weights for one model; freed together.
class DeviceWeights {
 public:
  int prec = 0;   // Precision the owning model is built for: pack_conv also emits the 2-byte forms (bf16 / f16) when it is not PREC_F32
  bool res32 = false;   // FE_PRECISION_RES32: the model keeps its residual / skip streams in fp32 around 2-byte GEMM operands
  bool split3 = false;  // FE_PRECISION_SPLIT3 (CLIP image tower only)
  bool half_only = false;   // 2-byte models whose every layer has a 2-byte form (the VLM decoder): no fp32 / Winograd / tap copies uploaded
  ~DeviceWeights() { release(); }
  float* upload(const std::vector<float>& v);
  void* upload_raw(const void* data, size_t bytes);   // any element type (bf16 weights)
  void release();
  size_t bytes() const { return bytes_; }
 private:
  std::vector<void*> ptrs_;
  size_t bytes_ = 0;
};

struct Linear {  // y = x W^T + b, stored as a 1x1 ConvW
  ConvW w;
};

struct LayerNormW {
  float* g = nullptr; float* b = nullptr; int d = 0; float eps = 1e-5f;
};

// Precision of a model's activations / weights, chosen per context before fe_weights_commit (fe_set_precision).
enum Precision : int { PREC_F32 = 0, PREC_BF16 = 1, PREC_F16 = 2 };
constexpr int PREC_RES32_FLAG = 16;   // or-ed into fe_set_precision's argument (include/facet_engine.h FE_PRECISION_RES32)
constexpr int PREC_SPLIT3_FLAG = 32;  // FE_PRECISION_SPLIT3: split-operand fp16 GEMMs (the ViT tower; implies fp32 streams)
template <class T> struct PrecOf { static constexpr int value = PREC_F32; };
template <> struct PrecOf<bf16> { static constexpr int value = PREC_BF16; };
template <> struct PrecOf<f16> { static constexpr int value = PREC_F16; };
// round-to-nearest-even float -> bf16 bits on the host (NaN stays NaN)
inline uint16_t f32_to_bf16_bits(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
// round-to-nearest-even float -> fp16 bits on the host, saturating at +-65504 like the device stores (NaN stays NaN)
inline uint16_t f32_to_f16_bits(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7FFFFFFFu;
  if (u > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);
  if (u >= 0x477FF000u) return (uint16_t)(sign | 0x7BFFu);           // >= 65520 rounds past the largest finite value: saturate
  if (u < 0x38800000u) {                                             // below 2^-14: subnormal half (or zero)
    if (u < 0x33000000u) return (uint16_t)sign;                      // < 2^-25 rounds to zero
    const int shift = 126 - (int)(u >> 23);                          // 14 .. 24
    const uint32_t m = (u & 0x7FFFFFu) | 0x800000u;
    const uint32_t h = m >> shift, rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    return (uint16_t)(sign | (h + ((rem > half || (rem == half && (h & 1))) ? 1 : 0)));
  }
  const uint32_t h = ((u - 0x38000000u) >> 13), rem = u & 0x1FFFu;
  return (uint16_t)(sign | (h + ((rem > 0x1000u || (rem == 0x1000u && (h & 1))) ? 1 : 0)));
}
inline uint16_t f32_to_half_bits(float f, int prec) { return prec == PREC_F16 ? f32_to_f16_bits(f) : f32_to_bf16_bits(f); }
// Adds the bf16 forms (ConvW.wh / wtap_h) of a weight to an already packed ConvW; a no-op for layers the bf16 kernel cannot take
// (3-channel first layers: those run on the fp32 stem / generic kernels and hand a bf16 tensor to the next layer).
void pack_conv_bf16(DeviceWeights& dw, const HostTensor& w, ConvW& c);

// Build helpers ------------------------------------------------------------------------------------
// `bf16` below: also build the bf16 form (models committed under PREC_BF16).
// packs an OIHW (or [out][in]) weight for the conv kernels; scale/shift are per-Cout epilogue vectors (nullable)
ConvW pack_conv(DeviceWeights& dw, const HostTensor& w, const std::vector<float>* scale, const std::vector<float>* shift);
// conv (OIHW) with optional bias and optional eval-mode BatchNorm folded into per-channel scale/shift.
ConvW build_conv(DeviceWeights& dw, const WeightStore& ws, const std::string& conv_prefix,
                 const std::string& bn_prefix, bool conv_bias, float bn_eps = 1e-5f);
// nn.Linear weight [out][in] (+bias) as a 1x1 conv
ConvW build_linear(DeviceWeights& dw, const WeightStore& ws, const std::string& prefix, bool bias);
// same from explicit tensor names / row ranges (for fused in_proj splits)
ConvW build_linear_rows(DeviceWeights& dw, const HostTensor& w, const HostTensor* b, int row0, int rows);
LayerNormW build_ln(DeviceWeights& dw, const WeightStore& ws, const std::string& prefix, float eps = 1e-5f);

struct Ctx;

// nn.MultiheadAttention (batch_first irrelevant: tokens of one image are contiguous rows).
struct MHAW {
  ConvW q, k;          // projections with bias; q carries the 1/sqrt(head_dim) scaling in scale/shift
  float* wv = nullptr; // raw [d][d] V weight: used as the A operand so the GEMM emits V^T directly
  void* wv_h = nullptr; // the same in the model's 2-byte type (bf16 / f16 models)
  float* bv = nullptr; // [d] V bias, added after P.V (softmax rows sum to 1)
  ConvW out;           // out_proj
  int d = 0, heads = 0;
};
MHAW build_mha(DeviceWeights& dw, const WeightStore& ws, const std::string& prefix, int heads);
// The layer wrappers below exist for T = float (fp32 path) and T = bf16 (models committed under PREC_BF16): same call shapes,
// overloads / explicit instantiations in engine.hip.
// y[B*Lq][d] = res + out_proj(softmax(q k^T / sqrt(hd)) v); q from q_in, k/v from kv_in (rows = tokens).
// RT = type of the residual / output rows: T, or float around 2-byte projections (fp32 token stream, FE_PRECISION_RES32)
template <class T, class RT>
void mha_forward(Ctx& c, const MHAW& m, const T* q_in, int ldq, const T* kv_in, int ldkv, int B, int Lq,
                 int Lk, const RT* res, int ldr, RT* y, int ldy, bool causal = false, bool out_by_image = false);
// (out_by_image, fp32: the out-projection goes through linear_tokens - for callers whose B*Lq rows must not pick the route, Lq <= 32)
// y[M][N] = act(x[M][K] W^T + b) (+res). fp32: M <= 32 rows without a residual take the few-row kernel; by_image (linear_tokens sets it:
// the rows are the tokens of images of at most 32 each) sends any M and a residual there too, where the layer fits that kernel.
void linear_forward(Ctx& c, const ConvW& w, const float* x, int ldx, int M, float* y, int ldy, int act,
                    const float* res = nullptr, int ldr = 0, bool by_image = false);
void linear_forward(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, bf16* y, int ldy, int act,
                    const bf16* res = nullptr, int ldr = 0);
void linear_forward(Ctx& c, const ConvW& w, const f16* x, int ldx, int M, f16* y, int ldy, int act,
                    const f16* res = nullptr, int ldr = 0);
// fp32 rows that are the tokens of B images, L each (the transformer layers of the TOPIQ head). linear_forward picks its few-row kernel by
// the row count, so an image's route - and the last bits of its score - would depend on what it is batched with; here the route follows L:
// images of at most 32 tokens take the few-row kernel, which works in chunks of 32 rows, whatever B is (a row's sum does not depend on its
// chunk), larger ones never reach it. res (nullable): residual rows, added before the activation on either route.
void linear_tokens(Ctx& c, const ConvW& w, const float* x, int ldx, int B, int L, float* y, int ldy, int act, const float* res = nullptr, int ldr = 0);
template <class T>
inline void linear_tokens(Ctx& c, const ConvW& w, const T* x, int ldx, int B, int L, T* y, int ldy, int act) { linear_forward(c, w, x, ldx, B * L, y, ldy, act); }
// 2-byte operand rows, fp32 residual rows (nullable) and fp32 result rows (the projections that write an fp32 token stream)
void linear_forward_s32(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, float* y, int ldy, int act, const float* res = nullptr, int ldr = 0);
void linear_forward_s32(Ctx& c, const ConvW& w, const f16* x, int ldx, int M, float* y, int ldy, int act, const float* res = nullptr, int ldr = 0);
// y = act(x W^T + b) + res with y / res of the caller's stream type: (T, T) = linear_forward, (2-byte, float) = linear_forward_s32
void linear_forward_res(Ctx& c, const ConvW& w, const float* x, int ldx, int M, float* y, int ldy, int act, const float* res, int ldr);
void linear_forward_res(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, bf16* y, int ldy, int act, const bf16* res, int ldr);
void linear_forward_res(Ctx& c, const ConvW& w, const f16* x, int ldx, int M, f16* y, int ldy, int act, const f16* res, int ldr);
void linear_forward_res(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, float* y, int ldy, int act, const float* res, int ldr);
void linear_forward_res(Ctx& c, const ConvW& w, const f16* x, int ldx, int M, float* y, int ldy, int act, const float* res, int ldr);
// same with fp32 outputs whatever the activation type (the last layer of a head: scores / features leave the engine in fp32)
void linear_forward_f32(Ctx& c, const ConvW& w, const float* x, int ldx, int M, float* y, int ldy, int act);
void linear_forward_f32(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, float* y, int ldy, int act);
void linear_forward_f32(Ctx& c, const ConvW& w, const f16* x, int ldx, int M, float* y, int ldy, int act);
// fp32 rows in, fp32 rows out, on the 2-byte copy of the weights (type `prec` = the model's): weight rows streamed once per 32 rows,
// activations never rounded (per-image head vectors of a FE_PRECISION_RES32 model)
void linear_forward_xf32(Ctx& c, const ConvW& w, int prec, const float* x, int ldx, int M, float* y, int ldy, int act);
template <class T>
inline TensorT<T> mat_view(const T* p, int rows, int cols, int ld) {
  TensorT<T> t; t.p = const_cast<T*>(p); t.n = 1; t.h = 1; t.w = rows; t.c = cols; t.ld = ld; return t;
}

// Runs conv on views; allocates nothing. Output spatial dims must already be set on y.
void conv_forward(Ctx& c, const ConvW& w, const Tensor& x, const Tensor& y, const ConvOpts& o);
void conv_forward(Ctx& c, const ConvW& w, const TensorH& x, const TensorH& y, const ConvOptsT<bf16>& o);
void conv_forward(Ctx& c, const ConvW& w, const TensorF16& x, const TensorF16& y, const ConvOptsT<f16>& o);
// fp32: whether this layer can run with the row-pooling epilogue (ConvOpts::pool_kw = kw, ConvOpts::pool); conv_forward asserts it
bool conv_rowpool_ok(const Ctx& c, const ConvW& w, const Tensor& x, const ConvOpts& o, int kw);
// fp32: the layer on the in-register Winograd kernel (3x3, stride 1, pad 1, a packed ConvW::wino64 operand), with its profile record
// "wino64 3x3 M= K= N=" and FLOP accounting. false = not launched: the layer or the views do not fit. The caller decides on the activation.
bool conv_wino64(Ctx& c, const ConvW& w, const Tensor& x, const Tensor& y, const ConvOpts& o);
// Allocates the output from the arena with the standard conv output size.
template <class T>
TensorT<T> conv_new(Ctx& c, const ConvW& w, const TensorT<T>& x, const ConvOptsT<T>& o);
// First layer of a network: fp32 NHWC4 pixels in, activations of type T out (the 3-channel layers always run on the fp32 stem /
// generic kernels; with T = bf16 their epilogue - or one conversion pass - hands bf16 to the rest of the network).
template <class T>
TensorT<T> first_conv(Ctx& c, const ConvW& w, const Tensor& x, const ConvOpts& o);
inline int conv_out_dim(int in, int k, int s, int p, int d) { return (in + 2 * p - d * (k - 1) - 1) / s + 1; }

// ---- ResNet (timm resnet50 features_only / torchvision resnet18 children[:-2]) -------------------
struct ResBlock {
  ConvW c1, c2, c3, down;
  bool has_down = false, bottleneck = true;
  int stride = 1;
  // stride-1 bottlenecks with a 64-channel 3x3 of a 2-byte model: conv2 + conv3 + identity + ReLU as one launch (kernels_c64.hip)
  void* frag2 = nullptr;
  void* frag3 = nullptr;
};
// kernels_n16.hip: fp32 3x3 convolution to 16 output channels (U2-Net-P's REBNCONV mid layers)
float* build_n16_weights(DeviceWeights& dw, const float* W, int cin);
void launch_conv3x3_n16_f32(const Tensor& x, const Tensor& y, const float* wt, const float* scale, const float* shift, int act, hipStream_t s);
// fragment blobs of kernels_c64.hip (W2 [64][64][3][3]; W3 [256][64] or null: the plain 3x3)
void build_c64_fragments(DeviceWeights& dw, const float* W2, const float* W3, void** frag2, void** frag3);
template <class E>
void launch_conv3x3_c64(const TensorT<E>& x, const TensorT<E>& y, const TensorT<E>* res, const void* frag2, const void* frag3, const float* scale2, const float* shift2,
                        const float* scale3, const float* shift3, int act2, hipStream_t s);
struct ResNet {
  ConvW stem;
  std::vector<std::vector<ResBlock>> layers;
  bool bottleneck = true;
};
// keys: prefix + {conv1,bn1,layer1.0.conv1,...} (timm/torchvision naming) or the Sequential numbering
// of reference models/samp_net.py:652-662 when `seq_names` is true (0=conv1,1=bn1,4..7=layer1..4).
void build_resnet(ResNet& r, DeviceWeights& dw, const WeightStore& ws, const std::string& prefix,
                  bool bottleneck, const int blocks[4], bool seq_names);
// feats (optional) receives [stem-relu, layer1..layer4]; returns layer4 output. x is always the fp32 NHWC4 image tensor.
// res32 (2-byte T only; FE_PRECISION_RES32): the skip stream of the network is kept in fp32 - every block's output leaves its
// last convolution both as fp32 (the next block's identity / the downsample branch's output) and as T (the operand of the next
// convolutions); last32 (optional) receives the fp32 form of the returned map.
template <class T>
TensorT<T> resnet_forward(Ctx& c, const ResNet& r, const Tensor& x_nhwc4, std::vector<TensorT<T>>* feats, bool res32 = false, Tensor* last32 = nullptr);

// ---- PIL-exact uint8 resampling (kernels_resize.hip) --------------------------------------------------
enum ResizeFilter : int { FE_FILTER_LANCZOS = 1, FE_FILTER_BILINEAR = 2, FE_FILTER_BICUBIC = 3 };  // PIL's enum values
struct ResizeCoeffs { std::vector<int> kk, bounds; int ksize = 0, out = 0; };
struct ResizeCoeffsDev { int* kk = nullptr; int* bounds = nullptr; int ksize = 0; };
// in0 / in1: the source interval the outputs cover (PIL passes the box as C floats); the whole axis is (0, in_size)
void build_resize_coeffs(int in_size, int out_size, int filter, ResizeCoeffs& rc);
void build_resize_coeffs(int in_size, float in0, float in1, int out_size, int filter, ResizeCoeffs& rc);
// third member of a Ctx::resize_cache key that is no PIL filter: fe_phash's tables to 32 samples (LANCZOS, or the identity for a skipped pass)
constexpr int FE_FILTER_KEY_PHASH = -1;
struct Ctx;
const ResizeCoeffsDev& upload_resize_coeffs(Ctx& c, const std::tuple<int, int, int>& key, const ResizeCoeffs& rc);
void resize_u8(Ctx& c, const uint8_t* d_src, int n, int h, int w, int oh, int ow, int filter, int y0, int ch, int x0,
               int cw, uint8_t* d_dst);
// PIL `resize((ow, oh), filter, box)`: box = (x0, y0, x1, y1) in source pixels, fractional; the support is clamped to the image, not the box
void resize_u8_box(Ctx& c, const uint8_t* d_src, int n, int h, int w, int oh, int ow, int filter, const float box[4], uint8_t* d_dst);
// 224 x 224 crops of a list of images of any sizes, one launch per pass (kernels_resize_mixed.hip; descriptors and pool: resize_mixed_core.h)
struct MixedDesc;
void resize_mixed224(Ctx& c, const MixedDesc* d_desc, int count, int max_nr, const int32_t* d_pool, uint8_t* d_scratch, uint8_t* out_u8,
                     float* out_f, const float mean[3], const float stdv[3]);

// ---- thumbnails: Pillow's box reduce + baseline JPEG encoder (kernels_jpeg.hip, jpeg_core.h) ------------
// PIL `reduce((fx, fy), box)`: d_dst [n][ceil(bh / fy)][ceil(bw / fx)][3]
void reduce_u8(Ctx& c, const uint8_t* d_src, int n, int h, int w, int fx, int fy, const int box[4], uint8_t* d_dst);
size_t jpeg_bound(int h, int w);                          // bytes no encode of an h x w image exceeds
size_t jpeg_scratch_bytes(int h, int w);      // arena bytes per image of launch_jpeg_encode
// d_out [n][cap]; d_lengths [n]: bytes written, or < 0 when the image needs more than cap (nothing is stored past cap)
void launch_jpeg_encode(Ctx& c, const uint8_t* d_img, int n, int h, int w, int bgr, int quality, uint8_t* d_out, size_t cap, int32_t* d_lengths);
// face thumbnails (kernels_face_thumb.hip): m crops of a resident BGR batch, each BOX-resized to its own size and encoded; out [m][cap] and
// lengths [m] are host buffers with fe_jpeg_encode's contract, the index / rectangle / size arrays are host arrays the caller has checked.
// Returns false when a row was too small for its face.
bool face_thumbnails(Ctx& c, const uint8_t* d_bgr, int n, int h, int w, int m, const int32_t* img_index, const int32_t* crops, const int32_t* out_sizes,
                     int quality, uint8_t* out, size_t cap, int32_t* lengths);
// the same for images of any sizes: d_imgs device descriptors (face_mixed_plan.h: src, h, w) of the images img_index refers to; rgb: R,G,B pixels
bool face_thumbnails_mixed(Ctx& c, const face_plan::ImageDesc* d_imgs, int rgb, int m, const int32_t* img_index, const int32_t* crops,
                           const int32_t* out_sizes, int quality, uint8_t* out, size_t cap, int32_t* lengths);

// thumbnails of a list of images of any sizes (kernels_jpeg.hip; descriptors and pool: thumb_mixed_core.h): one chunk's reduce, resize
// and encode, one launch per stage. descs [n] host descriptors with device sources; their buffers and every scratch array come from the
// arena (the caller rewinds); host_blob must outlive the stream's work. d_out [n][cap] / d_lengths [n] as launch_jpeg_encode leaves them.
struct ThumbDesc;
void thumbnails_mixed_launch(Ctx& c, ThumbDesc* descs, int n, const int32_t* d_pool, int bgr, int quality, std::vector<uint8_t>& host_blob,
                             uint8_t* d_out, size_t cap, int32_t* d_lengths);
// the bytes of every row that fitted (0 < length <= cap), back to back in row order, into d_packed; max_len: the longest of them
void jpeg_gather(Ctx& c, const uint8_t* d_rows, size_t cap, const int32_t* d_lengths, int n, size_t max_len, uint8_t* d_packed);

// ---- JPEG decode: file bytes -> resident uint8 batch, Pillow's pixels (kernels_jpeg_dec.hip, jpeg_dec_core.h) ----
void jpeg_probe(const uint8_t* data, size_t len, int flags, int32_t out[10]);      // the fields of fe_jpeg_info_ex, host only
void jpeg_scaled_size(int h, int w, int scale, int* sh, int* sw);                  // ceil(h / scale), ceil(w / scale): what a scaled decode gives
void jpeg_decode_batch(Ctx& c, const uint8_t* const* data, const size_t* len, int n, int h, int w, int scale, int bgr, int apply_orientation, int dst_on_device, int flags,
                       uint8_t* dst, int32_t* status);

// ---- perceptual hash + all-pairs Hamming search (kernels_phash.hip) ------------------------------------
void phash_cos_table(double* out);                       // [8][32] = cos(pi k (2n+1) / 64), host
size_t phash_tmp_bytes(int n, int h);
void launch_phash(Ctx& c, const uint8_t* d_img, int n, int h, int w, int bgr, uint8_t* d_tmp, const double* d_cos, uint64_t* d_hashes,
                  uint8_t* d_small, double* d_dct);
// one chunk of a list of images of any sizes (descriptors and pool: phash_mixed_plan.h): d_descs [n] with first_row ascending from 0,
// rows their total, max_w the widest, any_tall: one of them is tall (Image.resize's vertical-pass-first case), d_tmp [rows][32] scratch;
// outputs as launch_phash's
struct PhashDesc;
void launch_phash_mixed(Ctx& c, const PhashDesc* d_descs, int n, size_t rows, int max_w, int any_tall, int bgr, const int32_t* d_pool, uint8_t* d_tmp,
                        const double* d_cos, uint64_t* d_hashes, uint8_t* d_small, double* d_dct);
void launch_hamming_pairs(const uint64_t* d_hashes, int n, int maxd, int64_t cap, int* d_pairs, unsigned long long* d_count, hipStream_t s);

// ---- burst links over stored hashes (kernels_burst.hip; arguments as fe_burst_links, already checked and clamped) ----
void burst_lower_bounds(const int64_t* times, const uint8_t* flags, int n, int64_t reach, int32_t* lo);   // host
void burst_links(Ctx& c, const uint64_t* d_hash, const int64_t* times, const uint8_t* flags, int n, const int32_t* person_off, const int32_t* person_ids,
                 int n_ids, int thr, int64_t window_s, int64_t rapid_s, int32_t* link);

// ---- tag selection over prompt similarities (kernels_tags.hip; arguments as fe_tag_select_sims, already checked) ----
void launch_tag_select(const float* d_sims, long long ld, int n, int T, int G, const int32_t* d_perm, const int32_t* d_goff, double threshold,
                       int max_tags, int32_t* d_ids, float* d_scores, int32_t* d_counts, hipStream_t s);
void launch_gather_rows(const float* d_src, long long ld, int n, int d, float* d_dst, hipStream_t s);   // [n][d] rows ld floats apart -> packed

// ---- face clustering sweeps: core distances, mutual-reachability MST, best cosine match (kernels_cluster.hip) ----
int cluster_max_rounds(int n);                           // ceil(log2 n) + 1: the Boruvka round bound
void cluster_core_distances(Ctx& c, const float* x, int n, int d, int on_device, int normalise, int k, double* core, int32_t* core_idx);
void cluster_mreach_mst(Ctx& c, const float* x, int n, int d, int on_device, int normalise, int k, int32_t* edge_u, int32_t* edge_v,
                        double* edge_w, double* core, int32_t* rounds_out);
void cluster_best_match(Ctx& c, const float* q, int nq, const float* cc, int nc, int d, float* best_sim, int32_t* best_idx);
// ---- similar photos / merge suggestions: two more epilogues of the same sweep (kernels_cluster.hip; arguments as fe_similar_topk / fe_similar_pairs) ----
void similar_topk(Ctx& c, const fe_sim_rows& q, const fe_sim_rows& cand, int d, int cosine, const float* w, const int32_t* q_self, const uint8_t* visible,
                  int k, int32_t* idx, float* score);
void similar_pairs(Ctx& c, const fe_sim_rows& q, const fe_sim_rows& cand, int d, int cosine, const float* w, const int32_t* q_self, const uint8_t* visible,
                   const float* thr, int n_thr, int upper, int64_t max_pairs, int32_t* pairs, float* scores, int64_t* count);

class Graph;   // onnx_graph.h
struct GraphSlot;

// geometry the checkpoint's tensor shapes do not determine (transformers Qwen2_5_VLTextConfig): defaults = Qwen2.5-VL-7B-Instruct
struct VlmConfig {
  int n_heads = 28, n_kv_heads = 4, head_dim = 128; float rope_theta = 1e6f, rms_eps = 1e-6f; int mrope[3] = {16, 24, 24};
  int vis_heads = 16, fullatt[8] = {7, 15, 23, 31, 0, 0, 0, 0}, n_fullatt = 4;      // vision tower (Qwen2_5_VLVisionConfig)
  // Qwen3-VL (fe_vlm3_configure): q|k|v without bias, q_norm / k_norm, interleaved M-RoPE, tied lm_head allowed, DeepStack features
  // from after vision blocks deepstack[0 .. n_deepstack) added to the image rows after decoder layers 0 .. n_deepstack - 1
  bool qwen3 = false; int deepstack[8] = {0, 0, 0, 0, 0, 0, 0, 0}, n_deepstack = 0;
  // Qwen2-VL (fe_vlm2_configure): the Qwen2.5-VL decoder with a tied lm_head allowed, and the LayerNorm / QuickGELU tower (model_vlm_ln_vision.hip)
  bool qwen2 = false;
};

struct OpTiming { std::string name; double flops; double bytes; float ms; };

struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  Arena arena;
  std::string err;
  std::mutex mu;
  // per-op profiling (off by default): records events around each conv launch
  bool profile = false;
  std::vector<OpTiming> timings;
  double flops_accum = 0.0;
  double flops_saved = 0.0;   // algorithmic FLOPs NOT executed because a layer ran as Winograd (executed = flops_accum - flops_saved)
  double flops_half = 0.0;    // the part of flops_accum issued on the 2-byte matrix instructions (bf16 / f16 models): a mixed-precision
                              // run is priced per dtype (bench.py roofline: fp32 FLOPs / fp32 peak + 2-byte FLOPs / 2-byte peak)
  int force_variant = 0;   // developer hook: forwarded to ConvParams.variant
  int precision = PREC_F32;   // what the NEXT fe_weights_commit builds (fe_set_precision); each model remembers its own
  bool res32 = false;         // FE_PRECISION_RES32 of the next commit: fp32 residual streams around 2-byte GEMM operands
  bool split3 = false;        // FE_PRECISION_SPLIT3 of the next commit
  // TOPIQ GatedConv activations picked up by the next fe_weights_commit(FE_MODEL_TOPIQ) (fe_topiq_configure)
  int topiq_gate_act = ACT_GELU, topiq_wblk_act = ACT_GELU;
  size_t topiq_f32_below = 0;   // 2-byte TOPIQ: images with fewer pixels run on the model's fp32 weights (fe_topiq_f32_below; 0 = never)

  std::map<std::tuple<int, int, int>, ResizeCoeffsDev> resize_cache;  // (in, out, filter) -> device tables
  // tables of the call on the stack, looked up before resize_cache (nullptr outside such a call): the mixed-size ensemble call keeps the
  // LANCZOS tables of its shapes in call-scoped memory, so a library of distinct sizes leaves nothing behind
  const std::map<std::tuple<int, int, int>, ResizeCoeffsDev>* resize_scoped = nullptr;
  // (in, out, filter, bits of box start, bits of box end) -> device tables of a boxed resize
  std::map<std::tuple<int, int, int, uint32_t, uint32_t>, ResizeCoeffsDev> resize_box_cache;
  std::map<std::tuple<int, int, int>, void*> jpeg_cache;               // (h, w, quality) -> jpeg::Tables on the device
  void* jpegdec_stage = nullptr;      // pinned host block of fe_jpeg_decode's single upload; grows, never shrinks
  size_t jpegdec_stage_cap = 0;
  int32_t jpeg_entropy_stats[4] = {0, 0, 0, 0};      // of the last jpeg_decode_batch: fe_jpeg_entropy_stats
  WeightStore staging[8];
  std::unique_ptr<struct TopiqModel> topiq;
  std::unique_ptr<struct U2NetPModel> u2netp;
  std::unique_ptr<struct SampModel> samp;
  std::unique_ptr<struct ClipModel> clip;
  std::unique_ptr<struct AestheticModel> aesthetic;
  std::unique_ptr<struct ClipTextModel> clip_text;
  std::unique_ptr<struct VlmModel> vlm;
  VlmConfig vlm_cfg;          // read by the next fe_weights_commit(FE_MODEL_VLM) (fe_vlm_configure)
  int vlm_kv_format = 0;      // FE_VLM_KV_* of the next prefill's cache (fe_vlm_set_kv_format)
  int vlm_weight_format = 0;  // FE_VLM_WEIGHTS_* of the next fe_weights_commit(FE_MODEL_VLM) (fe_vlm_set_weight_format)
  std::unique_ptr<GraphSlot> graphs[8];   // ONNX graphs (face detector / landmarks / recognition, ...)
  ~Ctx();
};

// pre-norm transformer layers of pyiqa's CFANet (DETR-style) [DEP-KNOWLEDGE]
struct EncLayerW { MHAW attn; ConvW lin1, lin2; LayerNormW n1, n2; };
struct DecLayerW { MHAW cross; ConvW lin1, lin2; LayerNormW n1, n2, n3; };
struct GatedConvW {
  ConvW split_x1, w0, w2, w4;   // w0 = weight_blk[0] composed with the x2 half of splitconv
  // 64-channel level of a 2-byte model: the whole gate + its 16 x 16 average pool as ONE launch (kernels_gate.hip); null otherwise
  void* fused = nullptr;
  float* fused_bias = nullptr;
  void* w2_frag = nullptr;      // 2-byte models: w2 (3x3, 64 -> 64) in the halo-tiled kernel's fragment order (kernels_c64.hip)
};
void build_gate64_fragments(DeviceWeights& dw, GatedConvW& g, const float* W0, const float* B0, const float* W2, const float* B2, const float* W4, float b4,
                            const float* Wx, const float* Bx);
template <class E>
void launch_topiq_gate64(const TensorT<E>& x, const TensorT<E>& out, const void* frag, const float* bias, int wblk_act, int gate_act, hipStream_t s);

struct TopiqModel {
  DeviceWeights dw;
  ResNet backbone;
  bool has_head = false;
  int gate_act = ACT_GELU;   // activation of the gated branch x1 (pyiqa GatedConv.act)
  int wblk_act = ACT_GELU;   // activation after weight_blk[0] and weight_blk[2]
  GatedConvW gate[5];
  ConvW dim_reduce[5];
  EncLayerW sa[5];
  DecLayerW cross[4];
  EncLayerW pool;
  LayerNormW s_ln0, s_ln3;
  ConvW s_l1, s_l4, s_l6;
  std::vector<float> h_emb, w_emb;           // host copies [128][32] each
  std::map<std::pair<int, int>, float*> pos; // (th,tw) -> device [th*tw][256]
};
// ---- U2-Net-P + SAMP-Net (reference models/samp_net.py) ---------------------------------------------
struct RSUW {
  ConvW in;
  std::vector<ConvW> enc;  // rebnconv1..L
  std::vector<ConvW> dec;  // rebnconv(L-1)d .. rebnconv1d
  int depth = 0;
  bool dilated = false;    // RSU4F
};
struct U2NetPModel {
  DeviceWeights dw;
  RSUW stage[11];          // stage1..6, stage5d..1d
  ConvW side[6], outconv;
};
struct SampModel {
  DeviceWeights dw;
  ResNet backbone;         // ResNet-18 trunk
  ConvW pattern_weight, pattern[8], att_feat, att_pred, com0, com3, com5;
};
void build_u2netp(U2NetPModel& m, const WeightStore& ws);
void build_sampnet(SampModel& m, const WeightStore& ws);
// T = activation type (float | bf16); x_nhwc4 is always the fp32 pixel tensor, the score outputs are always fp32
template <class T>
void u2netp_forward(Ctx& c, const U2NetPModel& m, const Tensor& x_nhwc4, const TensorT<T>& sal);
// TS = element type of the saliency map (U2-Net-P may be committed under another precision than SAMP-Net)
template <class T, class TS>
void sampnet_forward(Ctx& c, const SampModel& m, const Tensor& x_nhwc4, const TensorT<TS>& sal, float* pw, float* attrs,
                     float* dist);

// ---- CLIP ViT image tower + aesthetic MLP -------------------------------------------------------------
struct ClipBlockW {
  LayerNormW ln1, ln2; MHAW attn; ConvW fc, proj;
  // split-operand forms (ClipModel::split3): fused q|k|v and c_fc as [Wh | Wh | Wl] (K' = 3K, against activation rows [xh | xl] read
  // with a wrap), out_proj as [Wh | Wl] (K' = 2K against the plain fp16 attention output read twice), c_proj as [Wh | Wh | Wl]
  ConvW qkv3, out2, fc3, proj3;
};
struct ClipModel {
  DeviceWeights dw;   // dw.prec = the precision this model was committed under
  ConvW patch, proj;
  float* pos = nullptr; float* cls = nullptr;
  LayerNormW ln_pre, ln_post;
  std::vector<ClipBlockW> blocks;
  int width = 0, heads = 0, tokens = 0, patch_size = 0, out_dim = 0;
  // FE_PRECISION_F16 | FE_PRECISION_SPLIT3: every weight and every GEMM operand that LayerNorm or GELU produces is carried as an fp16
  // pair hi + lo (hi = fp16(x), lo = fp16(x - hi): ~22 significant bits) and the products xh.Wh + xl.Wh + xh.Wl are accumulated in
  // fp32 by ONE launch over the concatenated operands - three times the matrix work of plain fp16, fp32-class results
  bool split3 = false;
  float* zero_bias = nullptr;   // [width] zeros: the V bias rides in the fused projection's shift
};
struct AestheticModel { DeviceWeights dw; ConvW l0, l2; };
// CLIP text tower (open_clip TextTransformer: causal, pooled at the EOT token) — SURVEY §8(f)-3
struct ClipTextModel {
  DeviceWeights dw;
  float* tok_emb = nullptr;   // [vocab][width]
  float* pos = nullptr;       // [ctx][width]
  std::vector<ClipBlockW> blocks;
  LayerNormW ln_final;
  ConvW proj;
  int vocab = 0, width = 0, ctx = 0, heads = 0, out_dim = 0;
};
void build_clip_text(ClipTextModel& m, const WeightStore& ws);
// tokens: device int32 [B][ctx]; eot: device int32 [B] (argmax position per row); feat: device [B][out_dim]
void clip_text_forward(Ctx& c, const ClipTextModel& m, const int* tokens, const int* eot, int B, float* feat);
void build_clip(ClipModel& m, const WeightStore& ws);
void build_aesthetic(AestheticModel& m, const WeightStore& ws);
// T: type of the GEMM operands of the tower (float | bf16 | f16); RT: type of the token (residual) stream and of every LayerNorm
// input - T, or float under FE_PRECISION_RES32; input pixels and output features are fp32 either way
template <class T, class RT = T>
void clip_forward(Ctx& c, const ClipModel& m, const Tensor& x_nhwc4, float* feat);
void clip_forward_split3(Ctx& c, const ClipModel& m, const Tensor& x_nhwc4, float* feat);      // split-operand fp16 tower (ClipModel::split3)
void aesthetic_forward(Ctx& c, const AestheticModel& m, const float* feat, int B, float* raw);
void l2_normalize(Ctx& c, const float* x, float* y, int rows, int d);

// ---- VLM tagger text decoder (transformers Qwen2_5_VLForConditionalGeneration; reference models/vlm_tagger.py) - model_vlm.hip ----------
struct VlmLayerW { ConvW qkv, o, gate, up, down; bf16* ln1 = nullptr; bf16* ln2 = nullptr; bf16* qn = nullptr; bf16* kn = nullptr; };
struct VlmVisionBlockW { ConvW qkv, proj, gate, up, down; bf16* n1 = nullptr; bf16* n2 = nullptr; };
struct VlmVisionW {      // model.visual.* (model_vlm_vision.hip)
  bool present = false;
  ConvW patch, m0, m2;
  std::vector<VlmVisionBlockW> blocks;
  bf16* ln_q = nullptr; float* inv_freq = nullptr;
  int hidden = 0, heads = 0, inter = 0, out_hidden = 0, patch_dim = 0;
  std::vector<int> fullatt;
};
// the LayerNorm towers (model_vlm_ln_vision.hip): Qwen2-VL (head_dim 80, QuickGELU) and Qwen3-VL (head_dim 64, tanh GELU, learned position
// table, DeepStack mergers) - LayerNorm blocks with biases, attention over each whole image, fc1 / act / fc2
struct VlmLnMergerW { float* ln_g = nullptr; float* ln_b = nullptr; ConvW fc1, fc2; };      // LayerNorm, fc1, erf GELU, fc2
struct VlmLnBlockW { ConvW qkv, proj, fc1, fc2; float* n1g = nullptr; float* n1b = nullptr; float* n2g = nullptr; float* n2b = nullptr; };
struct VlmLnVisionW {
  bool present = false;
  ConvW patch;
  float* pos_table = nullptr;      // Qwen3 only: [n_pos][hidden], the bf16 table widened to fp32
  std::vector<VlmLnBlockW> blocks;
  VlmLnMergerW merger;             // per-row LayerNorm form
  std::vector<VlmLnMergerW> ds_mergers;      // Qwen3 only (DeepStack: LayerNorm over the 4 hidden-wide view), after the blocks ds_blocks
  std::vector<int> ds_blocks;
  float* inv_freq = nullptr;
  int head_dim = 0, act = ACT_NONE;      // 80 / ACT_QUICKGELU or 64 / ACT_GELU
  int hidden = 0, heads = 0, inter = 0, out_hidden = 0, patch_dim = 0, patch_side = 0, n_pos = 0;
};
struct VlmModel {
  DeviceWeights dw;
  VlmConfig cfg;
  bf16* embed = nullptr; bf16* norm = nullptr; float* inv_freq = nullptr;
  ConvW lm_head;
  std::vector<VlmLayerW> layers;
  int vocab = 0, hidden = 0, inter = 0;
  // storage of the decoder's Linear weights (FE_VLM_WEIGHTS_*), and of the matrices a decode step streams (layer projections + lm_head):
  // their stored bytes, the bytes of their row scales, the quantised rows (fe_vlm_weight_info)
  int weight_format = 0;
  int64_t weight_bytes = 0, scale_bytes = 0, quant_rows = 0;
  VlmVisionW vis;
  bf16* img_embeds = nullptr; int img_rows = 0, img_cap = 0;      // merged image embeddings of the last fe_vlm_encode_images (device)
  // contiguous KV cache: per layer [n_seq][n_kv_heads][max_seq][128] keys (rotated) and values
  // kv_format (FE_VLM_KV_*, fe_vlm_set_kv_format; model_vlm.hip "KV-cache formats"): under FE_VLM_KV_E4M3 kcache / vcache hold the code arrays
  // ([n_seq][n_kv_heads][max_seq][128] uint8) and kscale / vscale the row scales ([n_seq][n_kv_heads][max_seq] fp32)
  std::vector<bf16*> kcache, vcache;
  std::vector<float*> kscale, vscale;
  int kv_format = 0;
  int64_t cache_bytes = 0;      // allocated for K / V rows and scales, all layers
  int cache_B = 0, max_seq = 0, cur_len = 0;
  // left padding of every sequence (device int [cache_B]): set by each prefill (zeros unless fe_vlm_prefill_images_padded), read by the
  // attention kernels of the prefill and of every later decode step (a captured decode graph holds the pointer)
  int* pad = nullptr;
  // log-probabilities of the tokens chosen by the last selection (device float [cache_B], NaN before the first): written by every prefill and
  // decode step, and by each step of a scored fe_vlm_generate_scored (fe_vlm_last_logprobs reads it)
  float* last_lp = nullptr;
  // patch rows of the last fe_vlm_preprocess_rgb (device bf16 [pre_rows][patch_dim]), the input of fe_vlm_encode_preprocessed
  bf16* pre_pv = nullptr; int pre_rows = 0, pre_cap = 0;
  // Qwen2-VL / Qwen3-VL: the LayerNorm tower. Qwen3-VL: the DeepStack features of the last fe_vlm3_encode_images (device bf16
  // [n_ds][ds_cap][hidden], rows as img_embeds), and the row -> image-row slot map of the prefill in flight (device int [rows], -1 for text
  // rows; null outside a prefill)
  VlmLnVisionW vis_ln;
  bf16* ds_feats = nullptr; int ds_n = 0, ds_cap = 0;
  const int* ds_slot = nullptr;
  void reserve_cache(int B, int max_seq, int kv_format = 0);      // a change of shape or format releases the cache first
  void release_cache();
  int64_t kv_token_bytes(int format) const;      // bytes one token of one sequence takes over all layers
  ~VlmModel() { release_cache(); if (img_embeds) (void)hipFree(img_embeds); if (pre_pv) (void)hipFree(pre_pv); if (ds_feats) (void)hipFree(ds_feats); }
};
void build_vlm(VlmModel& m, const WeightStore& ws, const VlmConfig& cfg, int weight_format = 0);
void build_vlm_vision(VlmModel& m, const WeightStore& ws);
void build_vlm_ln_vision(VlmModel& m, const WeightStore& ws);      // the family: m.cfg.qwen3, else Qwen2-VL
// pieces shared by the three towers (model_vlm_vision.hip), hd = head_dim 64 or 80
//   2-D rotary embedding on the q / k thirds of fused qkv rows [rows][3 * heads * hd] -> q_out / k_out [rows][heads * hd]
void vlm_vis_rope(Ctx& c, int hd, const bf16* qkv, const int* pos, const float* inv_freq, bf16* q_out, bf16* k_out, int rows, int heads,
                  int max_blocks = 0);      // (max_blocks: see vlm_grid)
//   non-causal attention inside the segments cu [n_seg + 1] (longest: max_seg rows), v = the V third of the fused qkv rows
void vlm_vis_attention(Ctx& c, int hd, const bf16* q, const bf16* k, const bf16* qkv, bf16* o, const int* cu, int n_seg, int max_seg, int heads);
//   the hd / 4 frequencies of VisionRotaryEmbedding(hd / 2)
float* vlm_vis_inv_freq(DeviceWeights& dw, int hd);
//   x = bf16(gelu_erf(x)) on n elements (a multiple of 4)
void vlm_gelu_erf(Ctx& c, bf16* x, size_t n);
// LayerNorm tower: pv fp32 patch rows or (pv == nullptr) pv_bf16; pos [N][2] (row, column per patch, 2x2-block-major order); interp_idx [N][4] /
// interp_w [N][4] (bilinear taps into the position table; nullptr: no table, Qwen2-VL); cu [n_seg + 1] (one segment per image). out
// [N/4][out_hidden], rows in the order of the patches' merge blocks; ds [n_ds][ds_cap][out_hidden] (nullptr: no DeepStack features)
void vlm_ln_vision_forward(Ctx& c, VlmModel& m, const float* pv, const bf16* pv_bf16, int N, const int* pos, const int* interp_idx, const float* interp_w,
                           const int* cu, int n_seg, int max_seg, bf16* out, bf16* ds);
// pv: fp32 patch rows, or (pv == nullptr) pv_bf16: the rows already in bf16 (fe_vlm_preprocess_rgb)
void vlm_vision_forward(Ctx& c, VlmModel& m, const float* pv, int N, const int* pos, const int* widx, const int* cu_win, int n_win, int max_win,
                        const int* cu_full, int n_full, int max_full, bf16* out, const bf16* pv_bf16 = nullptr);
// Qwen2-VL image processor after its resample (kernels_vlm_pre.hip): resized uint8 RGB [oh][ow][3] (oh, ow multiples of 28) -> patch rows
// [oh/14 * ow/14][3*2*14*14] in the processor's (gh/2, gw/2, 2, 2, C, T, 14, 14) order, each value lut[c][u]; bf16 always, fp32 when
// out_f32 is not null
void vlm_patchify(Ctx& c, const uint8_t* img, int oh, int ow, const float* lut, bf16* out_bf16, float* out_f32);
// the same for 16-pixel patches (Qwen3-VL): oh, ow multiples of 32, rows [oh/16 * ow/16][3*2*16*16]
void vlm_patchify16(Ctx& c, const uint8_t* img, int oh, int ow, const float* lut, bf16* out_bf16, float* out_f32);
// row kernels and helpers shared by the decoder and the vision towers (model_vlm.hip)
inline int grid_n(size_t n, int per = 256) { size_t g = (n + per - 1) / per; return (int)(g > 65535 * 4 ? 65535 * 4 : (g ? g : 1)); }      // grid-stride launches
bf16* upload_bf16(DeviceWeights& dw, const std::vector<float>& v);
// max_blocks of the row passes below (the fe_op_vlm_* test hooks; vlm_forward and the towers pass 0 = grid_n's own cap): at most that many
// 256-thread workgroups for the same work, so the later trips of the grid-stride loops run at small shapes. grid x block stays a multiple
// of 64 (a wave stays on one row, or one (row, head)).
int vlm_grid(size_t n_threads, int max_blocks);
// y = RMSNorm(x) w, rows of d values at strides ldx / ldy (d, ldx, ldy multiples of 4)
void vlm_rmsnorm(Ctx& c, const bf16* x, int ldx, const bf16* w, bf16* y, int ldy, int rows, int d, float eps, int max_blocks = 0);
void vlm_add(Ctx& c, bf16* x, const bf16* y, size_t n, int max_blocks = 0);
void vlm_silu_mul(Ctx& c, const bf16* g, const bf16* u, bf16* h, size_t n, int max_blocks = 0);      // h may be g
// x = bf16(x + y) (+ the DeepStack rows ds[slot[row]] where ds is given and slot[row] >= 0), n = RMSNorm(x) w   (w == nullptr: the sum only)
void vlm_add_rmsnorm(Ctx& c, bf16* x, const bf16* y, const bf16* w, bf16* n, int rows, int d, float eps, const int* slot = nullptr, const bf16* ds = nullptr,
                     int max_blocks = 0);
// n = RMSNorm(x) w for up to 64 rows, one 1024-thread workgroup per row (the finishing pass of the fused steps with no split sums to take:
// x is rewritten with its own bits)
void vlm_few_rows_rmsnorm(Ctx& c, bf16* x, const bf16* w, bf16* n, int rows, int d, float eps);
// The rotary embedding of the q and k heads of fused rows qkv [B * L][(nh + 2 nkv) * 128] + the KV-cache append at positions start .. start + L - 1
// (start_dev != nullptr: the start is read from device memory instead, the form a captured decode graph replays). qwen3: q / k RMSNorm with
// qn / kn [128] and eps, then the interleaved M-RoPE with sections (.., s1, s2); else the chunked one with sections (s0, s1, ..).
// pos: device [3][B * L]; inv_freq: device [64]; q_out [B * L][nh * 128]; kv: the cache and its format (struct VlmKv below).
struct VlmKv;
struct VlmRope {
  bool qwen3 = false;
  const bf16* qn = nullptr; const bf16* kn = nullptr; float eps = 0.f;
  int s0 = 0, s1 = 0, s2 = 0;
  int B = 0, L = 0, nh = 0, nkv = 0;
  int start = 0; const int* start_dev = nullptr;
  int max_blocks = 0;
};
void vlm_rope_cache(Ctx& c, const VlmRope& r, const VlmKv& kv, const bf16* qkv, const int* pos, const float* inv_freq, bf16* q_out);
void vlm_put_rows(Ctx& c, bf16* x, const bf16* rows, const int* index, int n, int d);
void vlm_embed(Ctx& c, const VlmModel& m, const int* tok_dev, int rows, bf16* x);
void vlm_forward(Ctx& c, VlmModel& m, bf16* x, const int* pos, int B, int L, int* next_dev, float* logits_dev, const int* len_dev = nullptr,
                 float* lp_dev = nullptr);
// One layer's KV cache in its format (E4M3: k / v are the code arrays, ks / vs the row scales; else ks = vs = nullptr)
struct VlmKv { int format = 0; bf16* k = nullptr; bf16* v = nullptr; float* ks = nullptr; float* vs = nullptr; int max_seq = 0; };
// bf16 rows ksrc / vsrc [n][L][128] (n = sequences x KV heads) -> positions 0 .. L - 1 of the cache, in its format
void vlm_kv_fill(Ctx& c, const VlmKv& kv, const bf16* ksrc, const bf16* vsrc, int n, int L);
// decode attention of one query row per head over the cache (+ the merge of the key chunks): q / out [B][nh * 128]; Lk keys by value or
// (len_dev != nullptr) *len_dev + 1 of them, the grid then covering max_seq; pad: device [B]. po / pm / pl: arena scratch for nsplit chunks
// ([B * nh * nsplit * 128], [B * nh * nsplit] twice), nsplit = ceil((len_dev ? max_seq : Lk) / 128).
void vlm_decode_attention(Ctx& c, const VlmKv& kv, const bf16* q, int B, int nh, int nkv, int Lk, const int* len_dev, const int* pad, float* po, float* pm,
                          float* pl, int nsplit, bf16* out);
// prefill attention, causal and grouped-query, head_dim 128: q / out [B * Lq][nh * 128], query i of a sequence at position qpos0 + i over keys
// pad[b] .. qpos0 + i of the bf16 cache rows kc / vc [B][nkv][max_seq][128] (Lk = qpos0 + Lq of them are valid); pad: device [B], rows below
// pad[b] come out as zeros
void vlm_prefill_attention(Ctx& c, const bf16* q, const bf16* kc, const bf16* vc, int max_seq, int B, int nh, int nkv, int Lq, int Lk, int qpos0, const int* pad,
                           bf16* out);
// ---- the decode projections launched alone (fe_op_vlm_linear): the decoder's own choice among its kernels, or a forced one
enum VlmLinearForce : int { VLM_LIN_AUTO = 0, VLM_LIN_FORCE_GEMV = 1, VLM_LIN_FORCE_GEMM32 = 2 };
enum VlmLinearFamily : int { VLM_LIN_GEMV = 1, VLM_LIN_GEMM32 = 2, VLM_LIN_WRAPPER = 3 };
// what ran: the family, the GEMV's row template MR, the GEMM's K splits, and whether its single split was written straight to the output
struct VlmLinearInfo { int family = 0, mr = 0, splits = 0, direct = 0; };
// a decoder Linear [N][K] (+ bias) in a weight format (FE_VLM_WEIGHTS_*), as build_vlm packs it; `name`: the tensor in an error message
ConvW vlm_pack_linear(DeviceWeights& dw, int weight_format, const HostTensor& W, const HostTensor* bias, const std::string& name);
// y = x W^T (+ b) in bf16 for any row count (a forced kernel runs under its own checks, whatever the row count)
void vlm_linear(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, bf16* y, int ldy, int force = VLM_LIN_AUTO, VlmLinearInfo* info = nullptr);
// the fp32 logits of the lm_head: lg [M][ldy]
void vlm_logits(Ctx& c, const ConvW& w, const bf16* x, int ldx, int M, float* lg, int ldy, int force = VLM_LIN_AUTO, VlmLinearInfo* info = nullptr);
// the fused steps of a 4 .. 32-row layer; each leaves its split sums in arena scratch (the CALLER rewinds) and returns the split count
//   x = bf16(x + bf16(a W^T)) (+ the DeepStack rows ds[slot[row]] where slot is given), n = RMSNorm(x) ln   (ln == nullptr: the sum only)
int vlm_proj_add_rmsnorm(Ctx& c, const ConvW& w, const bf16* a, int lda, int rows, bf16* x, const bf16* ln, bf16* n, float eps, const int* slot,
                         const bf16* ds);
//   h = bf16(silu(bf16(n Wg^T))) * bf16(n Wu^T), both products from one launch
int vlm_gate_up_silu_mul(Ctx& c, const ConvW& gate, const ConvW& up, const bf16* n, int ldn, int rows, bf16* h);
// fe_vlm_generate_until: the stop rule of a decode loop. fin_dev [B]: -1 while a sequence runs, else the EOS id it emitted (set by the
// caller for sequences whose first token already is one); live_dev [1]: the count of running sequences after the last step, read by the
// host after every `poll` steps. steps_run: out, the steps executed.
struct VlmUntil { int n_eos = 0; int eos[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int poll = 1; int* fin_dev = nullptr; int* live_dev = nullptr; int steps_run = 0; };
void vlm_decode_steps(Ctx& c, VlmModel& m, int* tok_dev, int* pos_dev, int B, int n_steps, int* out_dev, float* out_lp = nullptr, VlmUntil* until = nullptr);
// greedy ids (+ log-probabilities when lp_dev != nullptr) of fp32 logit rows, rounded to bf16 in place (model_vlm.hip)
void vlm_select(Ctx& c, float* lg, int B, int vocab, int* next_dev, float* lp_dev);

void build_topiq_head(TopiqModel& m, const WeightStore& ws);
// feats: the 5 pyramid levels for nb images; scores_dev: device [nb]
// The pooled gate of one pyramid level, fp32: adaptive_avgpool(act(split_x1(f)) * gate) as [n][th][tw][Cout] from the arena. With
// `rowpool`, and where the windows tile the map in widths of 2, 4, 8 or 16, the conv pools rows in its epilogue and a finishing pass adds
// the window's rows (no full-size tensor; *fused = 1); otherwise the conv writes full size and launch_adaptive_avgpool reads it back.
Tensor topiq_gate_pool(Ctx& c, const ConvW& split_x1, const Tensor& f, const ConvOpts& og, int th, int tw, bool rowpool, int* fused = nullptr);
template <class T>
void topiq_head_forward(Ctx& c, TopiqModel& m, const std::vector<TensorT<T>>& feats, float* scores_dev);
// fp32 view of an activation vector: the pointer itself for fp32, an arena copy for bf16
inline const float* to_f32(Ctx&, const float* p, size_t) { return p; }
const float* to_f32(Ctx& c, const bf16* p, size_t n);
const float* to_f32(Ctx& c, const f16* p, size_t n);

}  // namespace fe
