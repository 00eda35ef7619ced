/*
 * facet_engine.h — C ABI of libfacet_engine.so, the MI355X (gfx950) image-scoring engine.
 *
 * The reference (rlorenzo/facet) has no FFI for this path: its model layer is duck-typed Python objects
 * that end in torch nn.Module.__call__ / onnxruntime sessions. Each entry point below
 * names the reference call it stands behind; the facet_amd Python package is the ctypes binding that re-exposes the
 * reference's Python signatures on top of it.
 *
 * Conventions
 *   - every function returns FE_OK (0) or a negative fe_status; fe_last_error(ctx) gives the message.
 *   - no C++ exceptions cross this boundary; no torch / numpy types appear in it.
 *   - the caller owns every input / output buffer for the duration of the call; the engine owns
 *     weights and workspace behind the opaque fe_ctx.
 *   - pointers are HOST pointers unless the parameter is named d_* or `on_device` is non-zero.
 *   - images are uint8 HWC, RGB unless a `bgr` flag says otherwise; float tensors are fp32, NCHW,
 *     contiguous (the layouts the reference hands to its models).
 *   - one thread at a time per ctx for fe_*_score / fe_*_encode / fe_op_* (the reference calls its
 *     models from one "GPU thread", processing/batch_processor.py:123); lifecycle calls are mutex-guarded.
 */
#ifndef FACET_ENGINE_H
#define FACET_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fe_ctx fe_ctx;

enum fe_status {
  FE_OK = 0,
  FE_ERR_INVALID = -1,   /* bad argument / shape */
  FE_ERR_RUNTIME = -2,   /* HIP failure or internal check */
  FE_ERR_NOT_LOADED = -3, /* model weights not committed */
  FE_ERR_CAPACITY = -4   /* the batch does not fit (device memory, arena, KV cache): returned by fe_vlm_preprocess_rgb,
                            fe_vlm_encode_preprocessed, fe_vlm3_encode_images and fe_vlm_prefill_images_padded - retry with fewer images - and by
                            fe_jpeg_encode / fe_thumbnail_jpeg / fe_jpeg_thumbnail / fe_face_thumbnails when an output row is too small for its image */
};

/* Model slots (reference names: models/model_manager.py:393-437 'topiq','clip','samp_net',...). */
enum fe_model {
  FE_MODEL_TOPIQ = 0,     /* pyiqa topiq_nr: ResNet-50 + CFANet head   (models/pyiqa_scorer.py:33-39,212) */
  FE_MODEL_CLIP = 1,      /* open_clip ViT-L/14 image tower             (processing/scorer.py:508,662)     */
  FE_MODEL_SAMP = 2,      /* SAMPNet (ResNet-18 + pattern pooling)      (models/samp_net.py:665-791)       */
  FE_MODEL_U2NETP = 3,    /* U2-Net-P saliency                          (models/samp_net.py:258-342)       */
  FE_MODEL_AESTHETIC = 4, /* Linear(768,256)-ReLU-Linear(256,1)         (processing/scorer.py:579-583)     */
  FE_MODEL_VLM = 5        /* Qwen2.5-VL text decoder (VLM tagger)       (models/vlm_tagger.py:163-184)     */
};

enum fe_act { FE_ACT_NONE = 0, FE_ACT_RELU = 1, FE_ACT_GELU = 2, FE_ACT_SIGMOID = 3, FE_ACT_SOFTPLUS = 5 /* torch.nn.Softplus(beta=1, threshold=20) */ };

/* ---- lifecycle ------------------------------------------------------------------------------- */
/* Creates a context on HIP device `device` with a workspace arena of `arena_bytes`
 * (0 = a quarter of the free HBM, at most 64 GiB). Fails (no CPU fallback) when no gfx950 device is present. */
int fe_create(int device, size_t arena_bytes, fe_ctx** out);
void fe_destroy(fe_ctx* ctx);
const char* fe_last_error(fe_ctx* ctx); /* ctx may be NULL: returns the last fe_create error */
const char* fe_version(void);
int fe_sync(fe_ctx* ctx);
/* images processed per engine pass inside the batched entry points (activation footprint knob) */
int fe_set_microbatch(fe_ctx* ctx, int n);

/* Precision of the models committed AFTER this call (each model keeps the one it was committed under; FE_MODEL_AESTHETIC, the CLIP
 * text tower and the ONNX face graphs always run in fp32).
 *   FE_PRECISION_F32   default: the arithmetic of the reference's CPU path.
 *   FE_PRECISION_F16   what the reference itself runs on a GPU for CLIP (`self.model.half()`, processing/scorer.py:513-516): fp16
 *                      activations and weights in HBM on the matrix cores (v_mfma_f32_32x32x16_f16), fp32 accumulation, fp32
 *                      LayerNorm / softmax statistics, fp32 score heads and outputs; stores saturate at +-65504.
 *   FE_PRECISION_BF16  BASELINE.json configs[3]: the same with bf16 storage (v_mfma_f32_32x32x16_bf16; 8 significant bits against
 *                      fp16's 11, fp32's exponent range).
 *   | FE_PRECISION_RES32  (or-ed onto a 2-byte precision) the residual / skip streams of the network (the ViT token stream, the ResNet
 *                      skip path) and the inputs of every LayerNorm stay fp32; only the GEMM operands are 2 bytes.
 *   | FE_PRECISION_SPLIT3 (or-ed onto FE_PRECISION_F16; the CLIP image tower; implies RES32) split-operand fp16: every weight and every
 *                      GEMM operand LayerNorm / GELU produce is an fp16 pair hi + lo (~22 significant bits) and one launch over the
 *                      concatenated operands accumulates xh.Wh + xl.Wh + xh.Wl in fp32 - three times the matrix work of plain
 *                      fp16 (still a fraction of fp32's), results that hold the fp32 path's 1e-3 gate on the final scores.
 * CLIP's 14x14 patch embedding and the non-7x7 three-channel first layers stay on the fp32 kernels in every precision. */
enum fe_precision { FE_PRECISION_F32 = 0, FE_PRECISION_BF16 = 1, FE_PRECISION_F16 = 2, FE_PRECISION_RES32 = 16, FE_PRECISION_SPLIT3 = 32 };
int fe_set_precision(fe_ctx* ctx, int precision);
int fe_model_precision(fe_ctx* ctx, int model); /* enum fe_precision value of a loaded model, with its RES32 bit; -1 when it is not loaded */

/* ---- VLM tagger (BASELINE configs[4]), slice 1: the text decoder --------------------------------------------
 * Reference: models/vlm_tagger.py loads transformers' Qwen2_5_VLForConditionalGeneration in bfloat16 (:155-184) and calls
 * generate(**inputs, max_new_tokens=..., do_sample=False) (:250-259, :355-360). FE_MODEL_VLM takes that class's state dict (tensor
 * names model.language_model.* and lm_head.weight; model.visual.* is ignored in this slice) and computes in bf16, with the
 * rounding points of the bf16 torch modules; the decoder's Linear weights are stored as bf16 too unless fe_vlm_set_weight_format
 * asked for e4m3 rows (below), which changes the weights' values and nothing else. Token ids in, token ids out: tokenizer, chat template and tag parsing stay on the host
 * (facet_amd/vlm_tagger.py). fe_vlm_configure gives the geometry the tensor shapes do not determine (defaults = Qwen2.5-VL-7B:
 * 28 heads, 4 KV heads, head_dim 128, rope_theta 1e6, rms eps 1e-6, mrope_section 16/24/24) and is read by the NEXT
 * fe_weights_commit(FE_MODEL_VLM).
 * fe_vlm_prefill: n_seq prompts of `len` tokens each (tokens [n_seq][len], position_ids [3][n_seq][len] = the temporal / height /
 * width rotary positions transformers' get_rope_index yields; all three equal for text tokens) fill a fresh KV cache of max_seq
 * positions per sequence (<= 8192) and return the greedy next token of every sequence (argmax of the bf16 logits, first index on
 * ties, as torch.argmax) and, when `logits` is not NULL, those logits [n_seq][vocab]. fe_vlm_decode_step appends one token per
 * sequence (tokens [n_seq], position_ids [3][n_seq]). dims: vocab, hidden, layers, heads, kv_heads, intermediate, max_seq, cur_len. */
int fe_vlm_configure(fe_ctx* ctx, int n_heads, int n_kv_heads, int head_dim, float rope_theta, float rms_eps, const int* mrope_section);
/* Storage of the decoder's Linear weights (all three families), read by the NEXT fe_weights_commit(FE_MODEL_VLM); any other value is an
 * error. FE_VLM_WEIGHTS_E4M3: q|k|v, o, gate, up, down of every layer and lm_head are kept as OCP e4m3 codes with one power-of-two scale
 * per output row (row n: the smallest e with max|w[n]| * 2^-e <= 448, e >= -117; code = w * 2^-e rounded to nearest even, from the
 * bf16-rounded weight) and no bf16 copy of them is uploaded: a decode step streams half the bytes. Every dequantised value is exactly a
 * bf16 value, so the model is the bf16 model on those weights: activations, attention, the KV cache, norms, biases, the embedding table
 * (a tied checkpoint keeps its bf16 table for the lookup beside the e4m3 head) and the vision tower are untouched. Up to 32 rows the
 * projections read the codes directly; above that (prefill, more than 32 sequences) each matrix is widened to a bf16 scratch in the arena
 * first - one extra pass, so decode beyond 32 sequences is slower than with bf16 weights. A NaN or Inf weight fails the commit.
 * fe_vlm_weight_info: info4 = the loaded model's format, the stored bytes of the matrices a decode step streams (layer projections +
 * lm_head), the bytes of their row scales, the number of quantised rows. */
enum fe_vlm_weights { FE_VLM_WEIGHTS_BF16 = 0, FE_VLM_WEIGHTS_E4M3 = 1 };
int fe_vlm_set_weight_format(fe_ctx* ctx, int format);
int fe_vlm_weight_info(fe_ctx* ctx, int64_t* info4);
/* Storage of the decoders' KV cache (all three families), per context, read by the NEXT prefill; an unknown code is an error that leaves the
 * state unchanged. A change of format releases the cache: a decode call before a new prefill then fails ("call fe_vlm_prefill first").
 * One cache row is the 128 values of one (sequence, KV head, position), K and V separately.
 *   FE_VLM_KV_BF16 (default): bf16 rows.
 *   FE_VLM_KV_E4M3: 128 OCP e4m3 codes and one fp32 scale 2^e per row, by the row rule of the e4m3 weights above (the smallest e with
 *     max|row| * 2^-e <= 448, e >= -117; codes rounded to nearest even; nothing saturates): 2 * (128 + 4) bytes per token, KV head and
 *     layer instead of 512. The decode attention (fe_vlm_decode_step, fe_vlm_generate*) reads the codes directly, q and the probabilities
 *     stay bf16 and the sums fp32; the scales multiply scores and probabilities exactly. A prefill attends to its own unquantised K / V
 *     (its logits and first tokens are those of FE_VLM_KV_BF16, bit for bit) and leaves dequantize(quantize(row)) of every row in the
 *     cache. Every dequantised value is exactly a bf16 value: the engine is the bf16 engine on those cache rows. A row holding a NaN or
 *     Inf becomes NaN codes and propagates. Not built: fp8 matrix-core attention, a quantised q, a quantised prefill attention.
 *   FE_VLM_KV_BF16_E4M3: a bf16 cache whose rows are replaced by dequantize(quantize(row)) - the arithmetic of FE_VLM_KV_E4M3 at the storage
 *     of FE_VLM_KV_BF16, for tests and accuracy studies (what the format costs, apart from what the e4m3 kernels do).
 * fe_vlm_kv_info: info4 = the format of the next prefill, the bytes one token of one sequence takes over all layers in that format, the
 * bytes allocated for the live cache (0 before a prefill), its max_seq. Needs a loaded model.
 * fe_vlm_kv_rows: positions pos0 .. pos0 + n - 1 of (layer, seq, kv_head) of the live cache, dequantised, as float k / v [n][128]. */
enum fe_vlm_kv { FE_VLM_KV_BF16 = 0, FE_VLM_KV_E4M3 = 1, FE_VLM_KV_BF16_E4M3 = 2 };
int fe_vlm_set_kv_format(fe_ctx* ctx, int format);
int fe_vlm_kv_info(fe_ctx* ctx, int64_t* info4);
int fe_vlm_kv_rows(fe_ctx* ctx, int layer, int seq, int kv_head, int pos0, int n, float* k, float* v);
/* Vision tower (slice 2; built when the FE_MODEL_VLM checkpoint carries model.visual.*): geometry the tensor shapes do not determine
 * (defaults = Qwen2.5-VL-7B: 16 heads of 80, full attention in blocks 7 / 15 / 23 / 31, every other block inside 112-pixel windows), read
 * by the NEXT fe_weights_commit(FE_MODEL_VLM).
 * fe_vlm_encode_images = `model.visual(pixel_values, grid_thw).pooler_output` (what generate() runs on the processor's output,
 * models/vlm_tagger.py:245-259): pixel_values [n_patches][1176] (the processor's flattened 3 x 2 x 14 x 14 patches, fp32), and the
 * index arrays transformers.vision_utils derives from image_grid_thw (facet_amd/vlm_tagger.py restates them in numpy): patch_pos_hw
 * [n_patches][2] = (row, column) of every patch IN WINDOW ORDER, window_index [n_patches / 4] = raster index of the 2x2 merge block at
 * each window-order slot, cu_window_seqlens [n_windows + 1] and cu_seqlens [n_images + 1] = segment bounds (in patches, window order)
 * of the windowed and the full-attention blocks. The merged embeddings [n_patches / 4][hidden] (raster order) stay on the device for
 * the next fe_vlm_prefill_images and are also copied to `embeds` when it is not NULL (bf16 values widened to float).
 * fe_vlm_prefill_images = fe_vlm_prefill whose rows image_rows[i] (flat index sequence * len + position, one per <|image_pad|> token, in
 * order) take the i-th embedding instead of the token's (`inputs_embeds.masked_scatter(image_mask, image_embeds)`); position_ids are
 * get_rope_index's (temporal / height / width ids of the image tokens). */
int fe_vlm_vision_configure(fe_ctx* ctx, int n_heads, const int* fullatt_block_indexes, int n_fullatt);
int fe_vlm_encode_images(fe_ctx* ctx, const float* pixel_values, int n_patches, const int32_t* patch_pos_hw, const int32_t* window_index,
                         const int32_t* cu_window_seqlens, int n_windows, const int32_t* cu_seqlens, int n_images, float* embeds);
int fe_vlm_prefill_images(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int len, int max_seq, const int32_t* image_rows,
                          int n_image_rows, int32_t* next_tokens, float* logits);
int fe_vlm_dims(fe_ctx* ctx, int* dims8);
int fe_vlm_prefill(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int len, int max_seq, int32_t* next_tokens,
                   float* logits);
int fe_vlm_decode_step(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int32_t* next_tokens, float* logits);
/* n_steps greedy decode steps without a host round trip (the loop generate() runs, models/vlm_tagger.py:255-259): the tokens to feed
 * first (the prefill's choice, [n_seq]) and their positions ([3][n_seq]) go up once, token ids / positions / cache length then live in
 * device memory and one captured HIP graph of a decode step is replayed; out_tokens [n_steps][n_seq] = the token each step chose.
 * End-of-sequence handling is the caller's (cut the rows at the first EOS id). */
int fe_vlm_generate(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int n_steps, int32_t* out_tokens);
/* Scores of the greedy tokens (what `generate(..., output_scores=True)` + log_softmax at the chosen ids gives, models/vlm_tagger.py:497-626):
 * the selection pass that picks a token also takes its log-probability, -log sum_i exp(l_i - max_j l_j) over the bf16-rounded logits.
 * fe_vlm_generate_scored = fe_vlm_generate plus out_logprobs [n_steps][n_seq] (not NULL), each step's log-probs in the same device loop.
 * fe_vlm_last_logprobs: out [n_seq] = the log-probs of the tokens chosen by the most recent prefill (any of the three forms), decode step
 * or generate step (NaN before the first). */
int fe_vlm_generate_scored(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int n_steps, int32_t* out_tokens,
                           float* out_logprobs);
int fe_vlm_last_logprobs(fe_ctx* ctx, float* out);
/* Photos in (the image half of `processor(text=texts, images=images, padding=True)`, models/vlm_tagger.py:245-259 / :346-360):
 * fe_vlm_preprocess_rgb = Qwen2-VL's image processor (PIL backend) after its size choice: rgb holds n_images uint8 RGB images [h][w][3] back
 * to back; sizes [n_images][4] = h, w and the target oh, ow of each (transformers' smart_resize, computed by the caller: multiples of 28).
 * Each image is resampled with PIL's bicubic filter (bit-exact), rescaled by 1/255, normalised by mean / std [3] and patchified into the
 * processor's rows [oh/14 * ow/14][1176] ((gh/2, gw/2, 2, 2, C, T = 2, 14, 14) order, the frame duplicated), images concatenated. The rows
 * stay on the device in bf16 (what the patch embedding converts pixel_values to) for the next fe_vlm_encode_preprocessed; when
 * pixel_values is not NULL they are also copied out as the processor's fp32 values.
 * fe_vlm_encode_preprocessed = fe_vlm_encode_images on those rows (same index arrays, no pixel upload).
 * fe_vlm_prefill_images_padded = fe_vlm_prefill_images of a LEFT-padded batch: sequence b's first pad[b] positions (< len) are padding
 * (attention_mask 0): no position attends to them, in the prefill or in any later fe_vlm_decode_step / fe_vlm_generate, and their own
 * rows compute zeros. The other prefill entry points reset the padding to none. */
int fe_vlm_preprocess_rgb(fe_ctx* ctx, const uint8_t* rgb, int n_images, const int32_t* sizes, const float* mean, const float* stdv, float* pixel_values);
int fe_vlm_encode_preprocessed(fe_ctx* ctx, const int32_t* patch_pos_hw, const int32_t* window_index, const int32_t* cu_window_seqlens, int n_windows,
                               const int32_t* cu_seqlens, int n_images, float* embeds);
int fe_vlm_prefill_images_padded(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int len, int max_seq, const int32_t* pad,
                                 const int32_t* image_rows, int n_image_rows, int32_t* next_tokens, float* logits);

/* Qwen3-VL (transformers Qwen3VLForConditionalGeneration, the 8gb / 16gb profiles' qwen3-vl-2b): fe_vlm3_configure makes the NEXT
 * fe_weights_commit(FE_MODEL_VLM) build that family: q / k / v without bias, q_norm / k_norm (RMSNorm over each head's 128 dims before the
 * rotary embedding), interleaved M-RoPE over mrope_section (24 / 20 / 20 at 2B), lm_head tied to embed_tokens when the checkpoint has no
 * lm_head.weight; vision tower of vis_heads heads of 64 with LayerNorm blocks, a learned position table and DeepStack mergers after the
 * blocks deepstack_indexes[0 .. n_deepstack) (5 / 11 / 17 at 2B). A later fe_vlm_configure selects Qwen2.5-VL again.
 * fe_vlm3_encode_images = `model.visual(pixel_values, grid_thw)` of that class: pixel_values [n_patches][1536] (3 x 2 x 16 x 16 patches,
 * fp32) or NULL = the bf16 rows of the last fe_vlm_preprocess_rgb (which patchifies 16-pixel patches, sides multiples of 32, for this
 * family); patch_pos_hw [n_patches][2] = (row, column) of every patch in the processor's 2x2-block-major order; interp_idx / interp_w
 * [n_patches][4] = the bilinear taps (int32 rows of the position table, fp32 weights) of
 * get_vision_interpolation_indices_and_weights(align_corners=True); cu_seqlens [n_seg + 1] = one segment per image. The merged
 * embeddings [n_patches / 4][hidden] and the n_deepstack feature blocks of the same shape stay on the device for the next
 * fe_vlm_prefill_images(_padded), which puts the embeddings into the image rows and adds feature block i to them after decoder layer i
 * (decode steps never do); they are also copied to `embeds` / `deepstack` [n_deepstack][n_patches / 4][hidden] when those are not NULL.
 * Returns FE_ERR_CAPACITY when the batch does not fit.
 * fe_vlm_vision_dims (either family): dims4 = patch side (14 / 16), patch row width (1176 / 1536), DeepStack levels (0 for Qwen2.5-VL),
 * side of the square position table (0 for Qwen2.5-VL) of the committed tower - what sizes the pixel_values / deepstack outputs above. */
int fe_vlm_vision_dims(fe_ctx* ctx, int* dims4);
int fe_vlm3_configure(fe_ctx* ctx, int n_heads, int n_kv_heads, int head_dim, float rope_theta, float rms_eps, const int* mrope_section, int vis_heads,
                      const int* deepstack_indexes, int n_deepstack);
int fe_vlm3_encode_images(fe_ctx* ctx, const float* pixel_values, int n_patches, const int32_t* patch_pos_hw, const int32_t* interp_idx, const float* interp_w,
                          const int32_t* cu_seqlens, int n_seg, float* embeds, float* deepstack);

/* Qwen2-VL (transformers Qwen2VLForConditionalGeneration, the 24gb profile's composition model qwen2-vl-2b, models/vlm_composition.py):
 * fe_vlm2_configure makes the NEXT fe_weights_commit(FE_MODEL_VLM) build that family: the Qwen2.5-VL decoder (q / k / v with bias,
 * sectioned M-RoPE over mrope_section, 16 / 24 / 24) with lm_head tied to embed_tokens when the checkpoint has no lm_head.weight or
 * carries one equal to embed_tokens (2B ties it); vision tower of vis_heads heads of 80 with LayerNorm blocks, fc1 / QuickGELU / fc2 and
 * attention over each whole image in every block. Defaults of the Python wrapper = Qwen2-VL-2B-Instruct (12 heads over 2 KV heads of 128,
 * theta 1e6). A later fe_vlm_configure / fe_vlm3_configure selects its family again.
 * fe_vlm2_encode_images = `model.visual(pixel_values, grid_thw)` of that class: pixel_values [n_patches][1176] fp32 or NULL = the bf16
 * rows of the last fe_vlm_preprocess_rgb (14-pixel patches, sides multiples of 28, as for Qwen2.5-VL); patch_pos_hw [n_patches][2] =
 * (row, column) of every patch in the processor's 2x2-block-major order; cu_seqlens [n_seg + 1] = one segment per image. The merged
 * embeddings [n_patches / 4][hidden] stay on the device for the next fe_vlm_prefill_images(_padded) and are copied to `embeds` when it
 * is not NULL. Returns FE_ERR_CAPACITY when the batch does not fit. fe_vlm_vision_dims answers 14, 1176, 0, 0 for this family. */
int fe_vlm2_configure(fe_ctx* ctx, int n_heads, int n_kv_heads, int head_dim, float rope_theta, float rms_eps, const int* mrope_section, int vis_heads);
int fe_vlm2_encode_images(fe_ctx* ctx, const float* pixel_values, int n_patches, const int32_t* patch_pos_hw, const int32_t* cu_seqlens, int n_seg, float* embeds);
/* Greedy decode that stops (what `generate` does when every row has emitted EOS; all three families): the device loop of fe_vlm_generate /
 * fe_vlm_generate_scored (out_logprobs NULL / not NULL) for at most max_steps steps. The selection pass marks a sequence finished when it
 * picks one of eos_ids (n_eos <= 8; a first token in `tokens` that already is one counts); a finished sequence keeps being fed that id. The
 * count of unfinished sequences lives in device memory; the host reads it after every `poll` (>= 1) steps and stops launching at zero.
 * steps_run = the steps executed. Rows [0, steps_run) of out_tokens [max_steps][n_seq] are what fe_vlm_generate writes for the same
 * inputs with every sequence's tail after its first EOS holding that EOS id; rows [steps_run, max_steps) hold each sequence's EOS id.
 * out_logprobs is NaN after a sequence's first EOS. The captured decode-step graph is the one fe_vlm_generate replays: the stop is a host
 * decision between replays. */
int fe_vlm_generate_until(fe_ctx* ctx, const int32_t* tokens, const int32_t* position_ids, int n_seq, int max_steps, const int32_t* eos_ids, int n_eos, int poll,
                          int32_t* out_tokens, float* out_logprobs, int* steps_run);

/* ---- device buffers (so callers can keep batches resident in HBM without torch) ------------- */
int fe_dev_alloc(fe_ctx* ctx, size_t bytes, void** d_out);
int fe_dev_free(fe_ctx* ctx, void* d_ptr);
int fe_memcpy_h2d(fe_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int fe_memcpy_d2h(fe_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ---- timing / profiling on the engine's own HIP stream --------------------------------------- */
int fe_timer_start(fe_ctx* ctx);
int fe_timer_stop(fe_ctx* ctx, float* ms_out);
/* per-launch timing of every contraction kernel (serialises; for roofline accounting only) */
int fe_profile_enable(fe_ctx* ctx, int on);
int fe_profile_count(fe_ctx* ctx);
int fe_profile_get(fe_ctx* ctx, int i, char* name, int name_cap, double* flops, double* bytes, float* ms);
/* algorithmic FLOPs issued since the last fe_flops_reset (2*MAC of every contraction launched) */
int fe_flops_reset(fe_ctx* ctx);
int fe_flops_get(fe_ctx* ctx, double* flops);
/* Same counter minus the multiply-adds saved where a layer ran as Winograd F(2x2,3x3) (16 instead of 36 per 2x2 outputs):
 * the FLOPs the matrix cores actually executed. fe_flops_get stays the algorithmic (direct-convolution) count. */
int fe_flops_get_executed(fe_ctx* ctx, double* flops);
/* the part of fe_flops_get issued on the 2-byte (bf16 / fp16) matrix instructions: lets a mixed-precision run be priced per dtype */
int fe_flops_get_half(fe_ctx* ctx, double* flops);

/* ---- weights: replaces state_dict loading inside pyiqa.create_metric / open_clip.create_model /
 *      SAMPNet.load_state_dict (models/pyiqa_scorer.py:108, model_manager.py:140, samp_net.py:895).
 *      Tensors are passed by their checkpoint key names in PyTorch layout. -------------------- */
int fe_weights_begin(fe_ctx* ctx, int model);
int fe_weights_set(fe_ctx* ctx, int model, const char* name, const float* data, const int64_t* shape, int ndim);
int fe_weights_commit(fe_ctx* ctx, int model); /* validates, folds BN, packs for MFMA, uploads */
int fe_model_unload(fe_ctx* ctx, int model);   /* reference: ModelManager.unload_model (model_manager.py:237) */
int fe_model_loaded(fe_ctx* ctx, int model);   /* 1 / 0 */

/* ---- single ops (parity tests and building blocks; host NCHW in/out) -------------------------- */
/* y = act(conv2d(x, w) * scale + shift (+ res)), torch.nn.functional.conv2d semantics.
 * scale/shift/res may be NULL. res_after_act: add the residual after the activation. */
int fe_op_conv2d(fe_ctx* ctx, const float* x, int n, int c, int h, int w, const float* weight, int cout, int kh,
                 int kw, const float* scale, const float* shift, const float* res, int res_after_act, int stride,
                 int pad, int dil, int act, float* y);
/* test hook of the fused TOPIQ gate of the 64-channel pyramid level (kernels_gate.hip; 2-byte precisions only): x [n][64][h][w] (h, w
   multiples of 16), w0 / wx [64][64], w2 [64][64][3][3], w4 [1][64][3][3] ->
   y [n][64][h/16][w/16] = mean_16x16( act_g(wx x + bx) * sigmoid(w4 * act_w(w2 * act_w(w0 x + b0) + b2) + b4) ) */
int fe_op_topiq_gate64(fe_ctx* ctx, const float* x, int n, int h, int w, const float* w0, const float* b0, const float* w2,
                       const float* b2, const float* w4, float b4, const float* wx, const float* bx, int wblk_act,
                       int gate_act, float* y);
/* test hook of the pooled gate of the fp32 TOPIQ head (topiq_gate_pool): x [n][h][w][ldx] (NHWC rows of ldx >= cin floats, the first cin used),
   weight [cout][cin], bias [cout] or NULL, gate [n][h][w] ->
   y [n][th][tw][cout] = adaptive_avgpool( act(weight x + bias) * gate ). fused != 0: routed like the head (the gated 1x1 conv's row-pooling
   epilogue + finishing pass where the windows tile the map in widths 2 / 4 / 8 / 16, else the two plain launches); fused == 0: always the
   plain conv + adaptive pool. *routed (may be NULL) = 1 when the row-pooling route ran. fp32 contexts only. */
int fe_op_gate_rowpool(fe_ctx* ctx, const float* x, int n, int h, int w, int cin, int ldx, const float* weight, const float* bias, int cout,
                       const float* gate, int act, int th, int tw, int fused, float* y, int* routed);
/* test hook of the in-register Winograd F(2x2,3x3) kernel (kernels_wino64.hip; fp32 contexts only), launched alone, whatever route
   fe_op_conv2d would choose: x [n][c][h][w] with c <= 64, weight [cout][c][3][3] with cout <= 64 (c and cout multiples of 4), stride 1,
   padding 1; y = act(conv * scale + shift [+ res]) [+ res when res_after_act] as [n][cout][h][w]. scale / shift / res may be NULL;
   act = FE_ACT_NONE, FE_ACT_RELU or FE_ACT_GELU. */
int fe_op_wino64(fe_ctx* ctx, const float* x, int n, int c, int h, int w, const float* weight, int cout, const float* scale, const float* shift,
                 const float* res, int res_after_act, int act, float* y);
/* test hook of the halo-tiled 3x3 convolution 64 -> 64 (stride 1, padding 1; kernels_c64.hip; 2-byte precisions only): x [n][64][h][w],
   w2 [64][64][3][3], y = act2(conv(x, w2) * scale2 + shift2) [n][64][h][w]; with w3 [256][64] (then res [n][256][h][w] too, act2 = ReLU):
   y = relu((w3 . relu(conv * scale2 + shift2)) * scale3 + shift3 + res) [n][256][h][w] - the tail of a ResNet-50 layer1 bottleneck.
   scale / shift pointers may be null (1 / 0). */
int fe_op_conv3x3_c64(fe_ctx* ctx, const float* x, int n, int h, int w, const float* w2, const float* scale2,
                      const float* shift2, int act2, const float* w3, const float* scale3, const float* shift3,
                      const float* res, float* y);
int fe_op_maxpool2d(fe_ctx* ctx, const float* x, int n, int c, int h, int w, int k, int stride, int pad,
                    int ceil_mode, float* y);
int fe_op_bilinear(fe_ctx* ctx, const float* x, int n, int c, int h, int w, int ho, int wo, float* y);
int fe_op_adaptive_avgpool(fe_ctx* ctx, const float* x, int n, int c, int h, int w, int ho, int wo, float* y);
int fe_op_layernorm(fe_ctx* ctx, const float* x, int rows, int d, const float* g, const float* b, float eps, float* y);
/* Test hooks of the pooling, resampling, row and small-GEMM kernels (kernels_misc.hip), launched alone through the launch functions the
 * models call, on explicit element types (FE_ELEM_*) whatever the context's precision is: fp32 host data is rounded to the element type on
 * the device, results come back as fp32. Upload, launch and download only.
 *
 * fe_op_plane, route 0 maxpool (k, stride, pad, ceil_mode; ho / wo must be torch's output size), 1 bilinear (align_corners = False),
 * 2 adaptive_avgpool: x [n][c][h][w] is placed at channels c0_in .. c0_in + c - 1 of an NHWC device tensor of ctot_in channels whose other
 * channels hold `poison`; the kernel writes the view c0_out .. c0_out + c - 1 of a tensor of ctot_out channels prefilled with `fill`.
 * y [n][ctot_out][ho][wo]: the WHOLE output tensor.
 *
 * fe_op_rowpass, rows of d values, route:
 *   0  layernorm         y [rows][ldy] = LayerNorm(x [rows][ldx], eps) * g [d] + b [d]; (elem_in, elem_out) one of (f32, f32), (bf16, bf16),
 *                        (f16, f16), (f32, bf16), (f32, f16)
 *   1  layernorm_split   f32 -> f16, d in {256, 512, 768, 1024}, ldy >= 2 d: columns 0 .. d - 1 the f16 rounding hi of the result, d .. 2 d - 1
 *                        the rounding lo of (result - hi)
 *   2  softmax_rows      f32, in place on a copy of x [rows][ldx] (ldy == ldx): columns >= d are left alone
 *   3  softmax_rows_pad  the same, columns d .. ldx - 1 zeroed
 *   4  add_rows_bcast    in place on a copy of x [rows][ldx] (elem_in == elem_out, ldy == ldx): row r += g [L][d] row r % L
 *   5  split_hi_lo       f32 [rows][d] -> f16 [rows][2 d] (ldx == d, ldy == 2 d), hi | lo as route 1
 *   6  convert           [rows][d] dense (ldx == ldy == d); (f32, bf16), (bf16, f32), (f32, f16), (f16, f32)
 * x is the whole [rows][ldx] array; the output buffer [rows][ldy] is prefilled with `fill` (routes 0, 1, 5, 6) or is the copy of x, and is
 * returned whole in y. off_x / off_y (0 .. 3 elements) are added to the device base of x / y and off_gb (0 .. 3 floats) to that of g and b,
 * which decides the vector or scalar form of a launch. Any other pair of element types is an error.
 *
 * fe_op_gemm_skinny: y [M][ldy] (prefilled with `fill`) = act(x [M][ldx] . w [N][ldw]^T * scale [N] + shift [N]) over K columns, M <= 32,
 * scale / shift nullable; (ti, tw, to) one of (f32, f32, f32), (bf16, bf16, bf16), (bf16, bf16, f32), (f16, f16, f16), (f16, f16, f32),
 * (f32, bf16, f32), (f32, f16, f32). fe_op_gemm_skinny_res: the same with residual rows res [M][ldr] (nullable, rounded to the output
 * type) added after scale / shift and before the activation, and M <= 4096 (one launch over chunks of 32 rows); res == NULL and M <= 32
 * is fe_op_gemm_skinny. */
#define FE_ELEM_F32 0
#define FE_ELEM_BF16 1
#define FE_ELEM_F16 2
int fe_op_plane(fe_ctx* ctx, int route, int elem, const float* x, int n, int c, int h, int w, int ctot_in, int c0_in, int ctot_out, int c0_out,
                int k, int stride, int pad, int ceil_mode, int ho, int wo, float poison, float fill, float* y);
int fe_op_rowpass(fe_ctx* ctx, int route, int elem_in, int elem_out, const float* x, int rows, int d, int ldx, int ldy, int off_x, int off_y,
                  const float* g, const float* b, int off_gb, int L, float eps, float fill, float* y);
int fe_op_gemm_skinny(fe_ctx* ctx, int ti, int tw, int to, const float* x, int M, int K, int ldx, const float* w, int N, int ldw,
                      const float* scale, const float* shift, int act, int ldy, float fill, float* y);
int fe_op_gemm_skinny_res(fe_ctx* ctx, int ti, int tw, int to, const float* x, int M, int K, int ldx, const float* w, int N, int ldw,
                          const float* scale, const float* shift, const float* res, int ldr, int act, int ldy, float fill, float* y);
/* test hook of the fused head_dim-64 attention kernels, launched alone (kernels_attn.hip: fp32, bf16 / f16 and split-f16 policies):
   q [B][Lq][H*64], k / v [B][Lk][H*64], bv [H*64] -> o [B][Lq][H*64] = softmax(q k^T) v + bv per (batch, head), the semantics of
   torch.nn.functional.scaled_dot_product_attention with scale = 1 (q is passed as the kernel receives it: the caller has applied any
   scaling); causal: key j is visible to query i only if j <= i. form 0: the kernel of the context's precision, operands rounded to it on
   upload. form 1: the split-f16 kernel on hi | lo pairs of the fp32 operands (f16 precision only, no causal mask; hi + lo + bv returned). */
int fe_op_attention(fe_ctx* ctx, const float* q, const float* k, const float* v, const float* bv, int B, int H, int Lq, int Lk,
                    int causal, int form, float* o);
/* test hook of the attention wiring around those kernels (torch.nn.MultiheadAttention, batch_first): x_q [B][Lq][d], x_kv [B][Lk][d],
   in_proj_weight [3d][d], in_proj_bias [3d], out_proj_weight [d][d], out_proj_bias [d], res [B][Lq][d] (NULL: none) ->
   y [B][Lq][d] = res + out_proj(attention(q, k, v)) in the context's precision. head_dim = d / heads; 64 runs the fused kernel, any other
   value the unfused route, which exists for fp32 without a causal mask (anything else is an error). */
int fe_op_mha(fe_ctx* ctx, const float* x_q, const float* x_kv, int B, int Lq, int Lk, int d, int heads, const float* in_proj_weight,
              const float* in_proj_bias, const float* out_proj_weight, const float* out_proj_bias, const float* res, int causal,
              float* y);
/* test hook of the VLM decoder's greedy selection: logits [rows][vocab] (rows <= 65535) are rounded to bf16 as in the decoder; ids [rows] =
   argmax (first index on ties), logprobs [rows] (NULL: not computed) = the log-probability of that id. */
int fe_op_vlm_select(fe_ctx* ctx, const float* logits, int rows, int vocab, int32_t* ids, float* logprobs);
/* Test hook of the VLM decode attention, launched alone (no model): q [B][nh][128], k / v [B][nkv][Lk][128] are rounded to bf16, a cache of
 * Lk rows is built in kv_format (FE_VLM_KV_*) by the engine's own fill pass, and one decode-attention + merge launch pair runs over it with
 * the left padding pad [B] (keys below pad[b] are masked; pad[b] < Lk). len_from_device: Lk reaches the kernel through a device word and
 * the grid covers a larger max_seq, as a replayed decode graph has it. out [B][nh][128]; k_image / v_image [B][nkv][Lk][128] (nullable):
 * the dequantised cache rows. nh / nkv in 1 .. 8. */
int fe_op_vlm_decode_attention(fe_ctx* ctx, const float* q, const float* k, const float* v, int B, int nh, int nkv, int Lk, const int32_t* pad, int kv_format,
                               int len_from_device, float* out, float* k_image, float* v_image);
/* Test hook of the VLM decode projections, launched alone (no model): x [M][ldx] (ldx >= K, a multiple of 8), w [N][K] and w2 (nullable,
 * route 3) are rounded to bf16; the weights are packed in weight_format (FE_VLM_WEIGHTS_*) by the functions that build a model and freed
 * before the call returns. bias [N] is nullable. route:
 *   0  the decoder's Linear: y [M][N] = bf16(x W^T + bias)
 *   1  the logits form of the lm_head: y [M][N] = x W^T + bias in fp32 (a single K split without bias is written straight to y)
 *   2  o / down projection fused with what follows it: y [M][N] = bf16(xres + bf16(x W^T)) (+ ds [n_ds][N] rows where slot [M] >= 0, both
 *      nullable), y2 [M][N] = RMSNorm(y, eps) * g (g [N]); N % 4 == 0, no bias
 *   3  gate | up in one launch fused with the SwiGLU product: y [M][N] = bf16(silu(bf16(x W^T))) * bf16(x W2^T); N % 4 == 0, no bias
 * kernel: 0 what the decoder picks for this shape, 1 the streaming GEMV (M <= 4), 2 the weight-streaming GEMM (M <= 32, K % 128 == 0);
 * routes 2 and 3 are the GEMM's. A forced kernel runs under its own checks: a shape it does not take is FE_ERR_RUNTIME.
 * info [4] (out): the family that ran (1 GEMV, 2 GEMM, 3 the shared layer wrapper, for e4m3 on its bf16 scratch), the GEMV's row
 * template (1, 2 or 4), the GEMM's K splits, 1 if the single split was written straight to y. */
int fe_op_vlm_linear(fe_ctx* ctx, const float* x, int M, int ldx, const float* w, const float* bias, int N, int K, int weight_format, const float* w2,
                     const float* xres, const float* g, float eps, const int32_t* slot, const float* ds, int n_ds, int route, int kernel, float* y,
                     float* y2, int32_t* info);
/* Test hooks of the VLM decoders' row passes, launched alone (no model) through the functions vlm_forward launches them with. fp32 inputs are
 * rounded to bf16 on the device; fp32 outputs hold bf16 values. max_blocks (all three): 0 = the launch of production, else at most that
 * many 256-thread workgroups, so the later trips of the grid-stride loops run at small shapes.
 *
 * fe_op_vlm_rope_cache: rotary embedding of the q and k heads + the KV-cache append. qkv [B * L][(nh + 2 nkv) * 128], pos [3][B * L],
 * inv_freq [64]. family 0: Qwen2.5-VL, chunked sections (sa, sb, 64 - sa - sb) over (temporal, height, width); family 1: Qwen3-VL, q / k
 * RMSNorm with qn / kn [128] and eps, then the interleaved form where frequency j takes the height position if j % 3 == 1 and j < 3 sa, the
 * width position if j % 3 == 2 and j < 3 sb. The caches [B][nkv][max_seq][128] (and, FE_VLM_KV_E4M3, both scale arrays [B][nkv][max_seq])
 * are filled with the byte `fill` first; rows start .. start + L - 1 are then written (start_from_device: the kernel reads start from a
 * device word, as a replayed decode graph has it). Out: q_out [B * L][nh * 128]; k_raw / v_raw the WHOLE caches as stored - bf16 bit
 * patterns (2 bytes per value) or e4m3 codes (1 byte); k_scale / v_scale the whole scale arrays (FE_VLM_KV_E4M3 only, else ignored).
 *
 * fe_op_vlm_rows, rows of d values (d % 4 == 0), route:
 *   0  rmsnorm           out_n [rows][ldy] = RMSNorm(x [rows][ldx], eps) * w [d]; columns d .. ldy - 1 keep the value 768
 *   1  add               out_x [rows][d] = bf16(x + y)
 *   2  add_rmsnorm       out_x = bf16(x + y), out_n = RMSNorm(out_x, eps) * w
 *   3  add_rmsnorm, w == NULL (the last layer's form): out_x only
 *   4  add_rmsnorm with the DeepStack sum: rows with slot [rows] >= 0 take out_x = bf16(bf16(x + y) + ds [n_ds][d] row slot) first
 *   5  few_rows_rmsnorm  the one-workgroup-per-row form of rows <= 64: out_x = x, out_n = RMSNorm(x, eps) * w
 *   6  silu_mul          out_x = bf16(bf16(silu(x)) * y); alias != 0: written over the gate's own buffer, as vlm_forward calls it
 * ldx = ldy = d except for route 0. Unused inputs and outputs may be NULL.
 *
 * fe_op_vlm_vis_rope: the 2-D rotary embedding of the vision towers. qkv [rows][3 * heads * hd], hd 64 or 80, pos [rows][2] (row, column),
 * inv_freq [hd / 4] -> q_out, k_out [rows][heads * hd]. */
int fe_op_vlm_rope_cache(fe_ctx* ctx, const float* qkv, const int32_t* pos, const float* inv_freq, int family, const float* qn, const float* kn, float eps,
                         int sa, int sb, int B, int L, int nh, int nkv, int start, int start_from_device, int max_seq, int kv_format, int max_blocks, int fill,
                         float* q_out, uint8_t* k_raw, uint8_t* v_raw, float* k_scale, float* v_scale);
int fe_op_vlm_rows(fe_ctx* ctx, int route, const float* x, const float* y, const float* w, const int32_t* slot, const float* ds, int n_ds, int rows, int d,
                   int ldx, int ldy, float eps, int alias, int max_blocks, float* out_x, float* out_n);
int fe_op_vlm_vis_rope(fe_ctx* ctx, const float* qkv, const int32_t* pos, const float* inv_freq, int hd, int rows, int heads, int max_blocks, float* q_out,
                       float* k_out);
/* Test hooks of the Qwen-VL attention tile under its two kernels, launched alone (no model) through the one function that launches each.
 * fp32 inputs are rounded to bf16 on the device; fp32 outputs hold bf16 values; every output is filled with 768 before the launch.
 *
 * fe_op_vlm_vis_attention: the vision towers' non-causal attention inside packed segments. q, k, v [N][heads * hd], N = cu [n_seg], segment s
 * = rows cu [s] .. cu [s + 1] - 1 (cu [0] == 0, every segment at least one row, max_seg = the longest, N <= 65536), hd 64 or 80,
 * 1 .. 64 heads. The kernel reads v as the last third of fused rows [N][3 * heads * hd]; the hook fills the other two thirds with 1.0e4.
 * o [N][heads * hd].
 *
 * fe_op_vlm_prefill_attention: the decoders' causal grouped-query prefill attention, head_dim 128. q [B * Lq][nh * 128]; k, v
 * [B][nkv][Lk][128] with Lk = qpos0 + Lq; query i of a sequence sits at position qpos0 + i and sees keys pad [b] .. qpos0 + i; rows below
 * pad [b] come out as zeros. The caches [B][nkv][max_seq][128] are built by the engine's own fill pass; their rows Lk .. max_seq - 1 hold
 * bf16 NaNs. nh % nkv == 0, Lk <= max_seq <= 8192, 0 <= pad [b] < Lk, B * nh <= 65535. o [B * Lq][nh * 128].
 *
 * An argument outside these ranges is FE_ERR_RUNTIME before any launch. */
int fe_op_vlm_vis_attention(fe_ctx* ctx, const float* q, const float* k, const float* v, const int32_t* cu, int n_seg, int max_seg, int hd, int heads, float* o);
int fe_op_vlm_prefill_attention(fe_ctx* ctx, const float* q, const float* k, const float* v, int B, int nh, int nkv, int Lq, int qpos0, int max_seq,
                                const int32_t* pad, float* o);

/* developer hook: force a tile variant of the contraction kernel for every later launch (0 = automatic choice) */
int fe_set_conv_variant(fe_ctx* ctx, int variant);
/* developer hook: average ms of one conv shape on random device-resident data with a forced tile variant (0 = auto) */
int fe_bench_conv(fe_ctx* ctx, int n, int h, int w, int cin, int cout, int k, int stride, int pad, int with_res, int act,
                  int variant, int iters, float* ms_out);

/* ---- TOPIQ (reference: PyIQAScorer.score_image -> self.model(t), models/pyiqa_scorer.py:197-231) */
/* Activations inside pyiqa's GatedConv, read by the NEXT fe_weights_commit(FE_MODEL_TOPIQ): gate_act = the activation of the gated
 * branch x1, weight_blk_act = the one after weight_blk[0] and weight_blk[2] (each FE_ACT_RELU / FE_ACT_GELU / FE_ACT_SOFTPLUS).
 * Default GELU / GELU. Activations carry no parameters, so a checkpoint cannot tell which a pyiqa release used (pyiqa is not
 * vendored in the reference, models/pyiqa_scorer.py:33-39,108-111): the choice is a load-time option [DEP-KNOWLEDGE]. */
int fe_topiq_configure(fe_ctx* ctx, int gate_act, int weight_blk_act);
/* A TOPIQ model committed under a 2-byte precision scores images of fewer than `pixels` pixels on its fp32 weights (0, the default:
 * never). Small images give the head a few dozen tokens per level, too few to average the 2-byte rounding noise below the 1e-3 gate;
 * the PARITY precision policy (facet_amd/precision.py) sets 65536. */
int fe_topiq_f32_below(fe_ctx* ctx, long long pixels);
/* dims = {channels, height, width} of pyramid level `level` for h x w inputs (after the > 1024 LANCZOS cap of
 * models/pyiqa_scorer.py:131-153): the size of one image's block in fe_topiq_features' output. No context needed. */
int fe_topiq_feature_shape(int h, int w, int level, int dims[3]);
/* images: n x h x w x 3 uint8 RGB (all the same size, h and w multiples of 32).
 * level 0..4 = ResNet-50 pyramid feature (stem-relu, layer1..4) returned NCHW to host `out`. */
int fe_topiq_features(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, int level, float* out);
/* raw MOS per image (before the reference's clamp[0,1]*10, pyiqa_scorer.py:166-195) */
int fe_topiq_score(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* scores);

/* ---- U2-Net-P + SAMP-Net (reference models/samp_net.py) ------------------------------------------- */
/* x: fp32 NCHW [n,3,h,w], already Resize(224)+ToTensor+ImageNet-normalised as SAMPNetScorer.preprocess yields
 * (samp_net.py:904-928). fe_u2netp_saliency = SaliencyDetector.detect (:407-422): sal_out [n,h,w] in (0,1). */
int fe_u2netp_saliency(fe_ctx* ctx, const float* x, int n, int h, int w, float* sal_out);
/* = the model part of SAMPNetScorer.score_batch (:1005-1010): saliency = U2NETP(x)[0]; SAMPNet(x, saliency).
 * x is [n,3,224,224]. Outputs: pattern_weights [n,8] (logits), attributes [n,6], score_dist [n,5];
 * sal_out may be NULL. Post-processing (softmax/argmax/expectation, :957-989) stays on the host. */
int fe_samp_forward(fe_ctx* ctx, const float* x, int n, float* pattern_weights, float* attributes, float* score_dist,
                    float* sal_out);

/* ---- CLIP ViT-L/14 image tower + aesthetic MLP (reference processing/scorer.py:640-673) ------------- */
/* x: fp32 NCHW [n,3,224,224] as open_clip's eval transform yields. Any of the three outputs may be NULL:
 *   features      [n,768] = model.encode_image(x)                          (scorer.py:662)
 *   emb_norm      [n,768] = F.normalize(features, dim=-1)                  (:663; stored as 3072-byte blobs, :670)
 *   aesthetic_raw [n]     = aesthetic_head(features) (Linear-ReLU-Linear)  (:664; the (x+1)*5 clamp [0,10] stays on host, :669)
 */
int fe_clip_encode_image(fe_ctx* ctx, const float* x, int n, int on_device, float* features, float* emb_norm,
                         float* aesthetic_raw);

/* aesthetic_head on vectors already at hand: feats [n,768] -> aesthetic_raw [n]. The reference recomputes scores from STORED
 * embeddings this way (Facet.score_from_embedding, processing/scorer.py:619-629: the 3072-byte blob, i.e. the L2-normalised
 * embedding, goes through the same MLP); the (x+1)*5 clamp stays on the host. */
int fe_aesthetic_score(fe_ctx* ctx, const float* feats, int n, float* aesthetic_raw);

/* ---- preprocessing: PIL-exact uint8 resampling (bit-for-bit PIL.Image.resize, RGB 8-bit) ---------------- */
enum fe_filter { FE_LANCZOS = 1, FE_BILINEAR = 2, FE_BICUBIC = 3 }; /* PIL.Image.Resampling values */
/* src [n,h,w,3] uint8 -> dst [n,oh,ow,3] uint8; replaces PIL `image.resize((ow,oh), filter)`
 * (models/pyiqa_scorer.py:153 LANCZOS; torchvision Resize inside models/samp_net.py:823-830; open_clip transform). */
int fe_resize_u8(fe_ctx* ctx, const uint8_t* src, int n, int h, int w, int oh, int ow, int filter, int on_device,
                 uint8_t* dst);

/* The same with a fractional source box: PIL `image.resize((ow,oh), filter, box)`, box = (x0, y0, x1, y1) in source pixels as C
 * floats (what PIL's own C entry takes); NULL = the whole image. Output sample xx is centred at x0 + (xx + 0.5)(x1 - x0)/ow and its
 * support is clamped to the image, not to the box. */
int fe_resize_u8_box(fe_ctx* ctx, const uint8_t* src, int n, int h, int w, int oh, int ow, int filter, const float* box, int on_device,
                     uint8_t* dst);
/* PIL `image.reduce((fx, fy), box)`: integer box (x0, y0, x1, y1), NULL = the whole image; dst [n, ceil((y1-y0)/fy), ceil((x1-x0)/fx), 3].
 * Rounded means of fx*fy samples; the last column / row / corner average what remains (libImaging/Reduce.c, bit-exact). */
int fe_reduce_u8(fe_ctx* ctx, const uint8_t* src, int n, int h, int w, int fx, int fy, const int32_t* box, int on_device, uint8_t* dst);

/* ---- thumbnails: baseline JPEG encoder (byte-exact with Pillow + libjpeg defaults) ----------------------- */
/* Bytes that no encode of an h x w image can exceed (every block at its longest code, every byte stuffed, header, EOI). */
size_t fe_jpeg_bound(int h, int w);
/* img [n,h,w,3] uint8 (bgr = 1: the bytes are B,G,R) -> what PIL `image.save(buf, "JPEG", quality=quality)` writes for each image:
 * JFIF 1.01, YCbCr 4:2:0, integer slow DCT, standard Huffman tables (utils/image_transforms.py:49). out [n][cap] and lengths [n] are
 * host buffers; image i occupies out[i*cap .. i*cap + lengths[i]). When an image needs more than cap bytes the call returns
 * FE_ERR_CAPACITY with a message, lengths[i] is minus the bytes needed (or INT32_MIN) and its row is left alone; nothing is ever stored
 * past a row. cap = fe_jpeg_bound(h, w) always fits. */
int fe_jpeg_encode(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device, int quality, uint8_t* out, size_t cap,
                   int32_t* lengths);
/* generate_photo_thumbnail (utils/image_transforms.py:32-50; processing/scorer.py:1611-1617, :1680-1686) of a batch:
 * `thumb.thumbnail((size, size), LANCZOS); thumb.save(buf, "JPEG", quality=quality)` as reduce -> boxed LANCZOS resize -> encode on the
 * device. (ow, oh), (fx, fy), reduce_box (x0, y0, x1, y1; may be NULL when fx = fy = 1), resize_box (in pixels of the reduced image) and
 * tall (the reduced image is more than 100 times taller than wide: PIL resizes rows first) are facet_amd.thumbnail.thumbnail_plan's values
 * for (w, h, size). out / cap / lengths as fe_jpeg_encode, with cap against fe_jpeg_bound(oh, ow). */
int fe_thumbnail_jpeg(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device, int oh, int ow, int fx, int fy,
                      const int32_t* reduce_box, const float* resize_box, int tall, int quality, uint8_t* out, size_t cap, int32_t* lengths);

/* Face thumbnails (reference analyzers/face.py:43-82, as facet_amd.face.FaceAnalyzer._crop_face_thumbnail states it with Pillow): for
 * each of m faces the rectangle crops[f] = (x0, y0, x1, y1; exclusive ends, inside the image, not empty) of image img_index[f] of the
 * BGR batch is taken as an image of its own, resized to out_sizes[f] = (ow, oh) with PIL's BOX filter (libImaging/Resample.c: horizontal
 * pass into uint8, then vertical; the filter support is clamped to the crop, not to the photo; up- and downscale) and saved as the RGB
 * JPEG of fe_jpeg_encode. Byte-exact with `Image.fromarray(crop[:, :, ::-1]).resize((ow, oh), Image.BOX).save(buf, "JPEG",
 * quality=quality)`. facet_amd.face.face_thumbnail_plan gives rectangle and size for a face box. All faces of a call share three or four
 * launches; the encoder is one workgroup per face. Faces whose output has at most FE_FACE_THUMB_FUSED_SIDE x FE_FACE_THUMB_FUSED_SIDE
 * pixels (384 blocks) keep coefficients, code lengths and the bit buffer in LDS; larger outputs (up to FE_FACE_THUMB_MAX_SIDE a side) run
 * the same workgroup-per-face kernel over arena scratch and give the same bytes. out [m][cap] / lengths [m] are host buffers with
 * fe_jpeg_encode's contract: FE_ERR_CAPACITY and minus the bytes needed when a row is too small, nothing stored past a row, and
 * cap = fe_jpeg_bound(max oh, max ow) always fits. m == 0 returns FE_OK; a bad index, rectangle, size or quality returns FE_ERR_INVALID
 * with a message and launches nothing. A host batch (on_device = 0) is uploaded whole and has to fit the arena. */
#define FE_FACE_THUMB_FUSED_SIDE 128
#define FE_FACE_THUMB_MAX_SIDE 8192
int fe_face_thumbnails(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int m, const int32_t* img_index,
                       const int32_t* crops, const int32_t* out_sizes, int quality, uint8_t* out, size_t cap, int32_t* lengths);

/* ---- JPEG decode: file bytes -> uint8 batch, Pillow's pixels -------------------------------------------- */
/* Status of a file. 0: decoded (or decodable). Positive: a kind of file left to the caller's own decoder, nothing was attempted.
 * Negative: a corrupt stream. */
#define FE_JPEG_OK 0
#define FE_JPEG_PROGRESSIVE 1        /* SOF2; as a flag of the _ex entry points: decode such files too */
#define FE_JPEG_ARITHMETIC 2         /* arithmetic coding */
#define FE_JPEG_PRECISION 3          /* 12-bit samples */
#define FE_JPEG_COMPONENTS 4         /* 4 components (CMYK / YCCK) or 2 */
#define FE_JPEG_ADOBE_RGB 5          /* 3 components stored as RGB (Adobe transform 0) */
#define FE_JPEG_SAMPLING 6           /* sampling other than luma 1x1 / 2x1 / 2x2 with chroma 1x1 (4:4:0, 4:1:1, ...) */
#define FE_JPEG_MULTISCAN 7          /* baseline file with more than one scan */
#define FE_JPEG_OTHER 8              /* lossless / hierarchical frame, DNL, an EXIF / XMP block only Pillow should judge; with
                                      * FE_JPEG_PROGRESSIVE: a progression that is out of order, incomplete or longer than 32 scans, DQT between scans */
#define FE_JPEG_BAD_MARKER (-1)      /* not a JPEG file, a marker segment that makes no sense, a table that is missing */
#define FE_JPEG_BAD_HUFFMAN (-2)     /* a table that is no prefix code, a code that is in no table, a run past the block */
#define FE_JPEG_PREMATURE_END (-3)   /* the file or a segment ends before its data does */
#define FE_JPEG_BAD_RESTART (-4)     /* a restart marker out of sequence, or where none belongs */
#define FE_JPEG_BAD_DIMENSIONS (-5)  /* the file's size is not the h, w of the call */
#define FE_JPEG_BAD_COEFFICIENT (-6) /* samples so far out of range that libjpeg's C and SIMD transforms stop agreeing */
typedef struct { int32_t width, height, components, hsamp, vsamp, restart_interval, orientation, status; } fe_jpeg_info;
/* Reads the markers of one file on the host; needs no context. width / height as stored (before any EXIF transpose), hsamp / vsamp the
 * luma sampling factors, orientation the EXIF tag 0x0112 (1 when absent), status as above with 0 = fe_jpeg_decode takes this file. */
int fe_jpeg_probe(const uint8_t* data, size_t len, fe_jpeg_info* info);
/* n files -> dst [n,h,w,3] uint8 (device memory with dst_on_device, else host), the pixels of Pillow's
 * `ImageOps.exif_transpose(Image.open(f)).convert('RGB')` (utils/image_loading.py:100-106; apply_orientation = 0: without the transpose),
 * as B,G,R with bgr. Baseline Huffman files, YCbCr 4:4:4 / 4:2:2 / 4:2:0 or grayscale, one scan, with or without restart markers; the
 * files of a call may differ in quality, tables, subsampling, restart interval and orientation, and agree on the output size h x w
 * (after the transpose). status [n] (host): see above; the slot of an image with a non-zero status is left untouched. Returns FE_OK when
 * every image got a status. Temporaries come from the context's workspace, in as many chunks as it takes. */
int fe_jpeg_decode(fe_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, int h, int w, int bgr, int apply_orientation,
                   int dst_on_device, uint8_t* dst, int32_t* status);
/* The same with flags. 0: exactly fe_jpeg_probe / fe_jpeg_decode. FE_JPEG_PROGRESSIVE: a progressive Huffman file (SOF2) gets status 0
 * instead of 1 when libjpeg decodes it without inter-block smoothing, which is when its scans obey jdphuff.c's parameter rules, follow the
 * normal progression (a coefficient's first scan has Ah = 0, every later one Ah = the Al before it) and are complete (every coefficient of
 * every component down to Al = 0), in at most 32 scans and with no DQT behind the first SOS; any other progressive file gets
 * FE_JPEG_OTHER or a negative status. progressive: the frame is SOF2 (set only with the flag); scans: the scans read, 0 for a baseline
 * file. The entropy stage runs once per scan over that scan's restart intervals and with that scan's tables, in file order; the
 * transform and colour stages, and therefore the pixels, are those of a baseline file. Progressive and baseline files of one output
 * size may share a call. */
typedef struct { int32_t width, height, components, hsamp, vsamp, restart_interval, orientation, status, progressive, scans; } fe_jpeg_info_ex;
int fe_jpeg_probe_ex(const uint8_t* data, size_t len, int flags, fe_jpeg_info_ex* info);
int fe_jpeg_decode_ex(fe_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, int h, int w, int bgr, int apply_orientation,
                      int dst_on_device, int flags, uint8_t* dst, int32_t* status);
/* A second flag bit of fe_jpeg_decode_ex, fe_jpeg_decode_scaled and fe_jpeg_thumbnail, alone or with FE_JPEG_PROGRESSIVE; fe_jpeg_probe_ex
 * accepts and ignores it. Without it the entropy stage gives a lane to every restart interval, so a file without restart markers is
 * decoded by one lane. With it, every baseline entropy-coded segment (the whole scan, or one restart interval) of at least two
 * subsequences of 128 bytes is decoded by one lane per subsequence: self-synchronising Huffman decoding (Weissenberger & Schmidt, ICPP
 * 2018), in which every lane first decodes from a guessed state, takes over its left neighbour's exit state round by round until no
 * state changes, and then decodes once more for real. Shorter segments and the scans of progressive files keep the lane per segment.
 * Pixels, bytes and statuses never depend on the flag: an image in which the parallel decode met an error is decoded again by the serial
 * kernel inside the same call. */
#define FE_JPEG_FLAG_PARALLEL 0x100
/* The entropy stage of the context's last fe_jpeg_decode* / fe_jpeg_thumbnail call: out[0] segments decoded in parallel, out[1] their
 * subsequences, out[2] the most rounds any segment took, out[3] images decoded again by the serial kernel. All zero without
 * FE_JPEG_FLAG_PARALLEL. The numbers came back with that call's statuses: this waits for nothing. */
int fe_jpeg_entropy_stats(fe_ctx* ctx, int32_t out[4]);
/* The decode at 1/scale that Pillow's `JpegImageFile.draft()` switches on (libjpeg's scale_num / scale_denom), which `Image.thumbnail`
 * calls first on an image that comes from a JPEG file. scale: 1, 2, 4 or 8, anything else returns FE_ERR_INVALID and launches nothing;
 * scale 1 is fe_jpeg_decode_ex bit for bit. h, w: the scaled size, ceil(H / scale) x ceil(W / scale) (fe_jpeg_scaled_size), exchanged
 * after the EXIF transpose as in fe_jpeg_decode. The pixels are those of `im.draft(None, ...); im.convert('RGB')` once draft() has chosen
 * this scale: luma blocks go through libjpeg's 4x4 / 2x2 / 1x1 inverse transforms (jidctred.c), and a subsampled chroma component is
 * scaled up by a transform up to twice that size instead of by the upsampler (jdmaster.c), so this is not the full decode followed by a
 * reduce. Entropy stage, parser, flags and status codes are fe_jpeg_decode_ex's; progressive files under the flag take the same stages. */
int fe_jpeg_scaled_size(int h, int w, int scale, int32_t* scaled_h, int32_t* scaled_w);
int fe_jpeg_decode_scaled(fe_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, int h, int w, int scale, int bgr,
                          int apply_orientation, int dst_on_device, int flags, uint8_t* dst, int32_t* status);
/* Stored JPEG bytes -> smaller JPEG bytes (reference db/maintenance.py:182-272 export_viewer_db, api/routers/thumbnails.py:54-64
 * _resize_thumbnail): `Image.open(f)`, `img.thumbnail((size, size), LANCZOS)`, `img.save(buf, "JPEG", quality=quality)` for n files of
 * one source size, as fe_jpeg_decode_scaled (no EXIF transpose: Image.open + thumbnail does none) -> reduce -> boxed LANCZOS resize ->
 * encode on one resident buffer. scale and the plan (oh .. tall, fe_thumbnail_jpeg's arguments) are
 * facet_amd.thumbnail.thumbnail_plan_jpeg's for (W, H, size); h, w the scaled size the plan is stated on. flags: fe_jpeg_decode_ex's.
 * status [n]: the decode's; a file with a non-zero status gets lengths[i] = 0 and its row is left alone. out / cap / lengths otherwise as
 * fe_thumbnail_jpeg, FE_ERR_CAPACITY included. */
int fe_jpeg_thumbnail(fe_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, int h, int w, int scale, int flags, int oh, int ow,
                      int fx, int fy, const int32_t* reduce_box, const float* resize_box, int tall, int quality, uint8_t* out, size_t cap,
                      int32_t* lengths, int32_t* status);

/* ---- image-level entry points (uint8 HWC images in, per-image results out) ------------------------------ */
/* CLIP from raw RGB images: open_clip eval transform on the GPU (PIL-bicubic shorter side -> 224, center crop 224,
 * /255, CLIP mean/std) + fe_clip_encode_image. Replaces batch_processor.py:95 `scorer.preprocess(pil)` +
 * scorer.py:640-673. */
int fe_clip_encode_images(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* features,
                          float* emb_norm, float* aesthetic_raw);
/* SAMPNetScorer.score_batch from raw images (samp_net.py:904-928,991-1010): optional BGR->RGB, PIL-bilinear
 * Resize((224,224)), ToTensor, ImageNet Normalize, U2NETP saliency, SAMPNet. Outputs as fe_samp_forward. */
int fe_samp_score_images(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device,
                         float* pattern_weights, float* attributes, float* score_dist);
/* CLIP text tower (built when the FE_MODEL_CLIP checkpoint carries token_embedding.weight): tokens int32 [n][77] ->
 * un-normalised text features [n][768]. Replaces `clip_model.encode_text(tokens)` (models/tagger.py:69-75); pooling is
 * at argmax(token id) = the EOT token, as open_clip does. */
int fe_clip_encode_text(fe_ctx* ctx, const int32_t* tokens, int n, int ctx_len, float* features);

/* Batched tag scoring: sims[n][T] = emb[n][d] . text[T][d]^T. Replaces the per-image matmul + loop of
 * CLIPTagger.get_tags_from_embedding (models/tagger.py:100-106); selection (max over synonyms, threshold, top-k) stays on host. */
int fe_tag_similarities(fe_ctx* ctx, const float* emb, int n, const float* text, int T, int d, float* sims);

/* Tag selection on the device: the whole of CLIPTagger.get_tags_from_embedding (models/tagger.py:100-114) for n stored embeddings in
 * one call - similarities, per-tag max over the synonyms, threshold, sort and top-k - for the library-wide passes of the reference
 * (photos.py:578-625 --recompute-tags, tag_existing.py:16-63 after every scan, is_artwork). Only the chosen ids and scores come back.
 *
 * fe_tag_vocab_set keeps ONE vocabulary per context: text [T][d] (host, L2-normalised rows; d a multiple of 4 in 4 .. 8192) is packed
 * once for the GEMM; tag_of_prompt [T] (host) gives each prompt its tag id in 0 .. G-1. Every id must be used and the ids must first
 * appear in ascending order (tag id = position of the tag in the reference's dict, which breaks ties); the prompts of a tag need not
 * be contiguous. Limits: 1 <= G <= T <= 4096. A second call replaces the vocabulary; T = 0 clears it. A broken limit or id rule
 * returns FE_ERR_INVALID with a message that names it, and the vocabulary in place stays.
 *
 * fe_tag_select: emb is n rows of d floats (d from the vocabulary), ld >= d floats apart, on the host (on_device = 0) or the device
 * (records read in place: fe_ensemble_score's record at column 21 with ld = 789; rows that are not packed on a 16-byte boundary are
 * gathered into a packed chunk buffer first). Per row, exactly as the reference:
 *   score of a tag  = its prompts' similarities folded in prompt order: the first, replaced only by a later one that is > it
 *                     (a NaN in first place stays, a later NaN is skipped);
 *   kept            iff (double)score >= threshold (the reference compares float(sim) with a Python float; NaN never passes);
 *   order           descending score, ties by ascending tag id; the first max_tags.
 * Outputs (host): ids [n][max_tags] padded with -1, scores [n][max_tags] padded with 0, counts [n] = the entries written.
 * 1 <= max_tags <= G. Rows go through in chunks sized from the arena (at most 131072 rows; fe_set_tag_chunk(rows) sets a smaller
 * size, 0 restores the default): per chunk one upload or gather, the GEMM on the cached text rows, one selection launch, one copy of
 * the outputs. The similarities never leave the device. The GEMM picks its kernel by the rows of a chunk, so the last bits of a
 * similarity may depend on the chunk size (as they depend on the batch in fe_tag_similarities); exact inputs give equal results.
 * Without a vocabulary: FE_ERR_NOT_LOADED. n = 0 returns FE_OK.
 *
 * fe_tag_select_sims: the selection alone on a given sims matrix of n rows of T floats, ld >= T apart, host or device (read in place
 * at any ld and alignment); same outputs, same vocabulary (its grouping is what is used). */
int fe_tag_vocab_set(fe_ctx* ctx, const float* text, int T, int d, const int32_t* tag_of_prompt, int G);
int fe_set_tag_chunk(fe_ctx* ctx, int rows);
int fe_tag_select(fe_ctx* ctx, const float* emb, int n, int ld, int on_device, double threshold, int max_tags, int32_t* ids, float* scores,
                  int32_t* counts);
int fe_tag_select_sims(fe_ctx* ctx, const float* sims, int n, int ld, int on_device, double threshold, int max_tags, int32_t* ids,
                       float* scores, int32_t* counts);

/* The whole ensemble on one resident batch — what processing/batch_processor.py:169-360 sequences per image.
 * records [n][FE_RECORD_FLOATS]: [0] topiq raw MOS, [1] aesthetic raw, [2..9] SAMP pattern logits, [10..15] SAMP
 * attributes, [16..20] SAMP score distribution, [21..788] L2-normalised CLIP embedding. Fields of models that are
 * not loaded stay 0; *models_run (nullable) = bitmask 1 topiq | 2 clip | 4 samp. This is also the fixed-size
 * per-image record that ranks all-gather in multi-GPU runs. */
#define FE_RECORD_FLOATS 789
int fe_ensemble_score(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* records,
                      int* models_run);

/* Which of the loaded models fe_ensemble_score runs: bitmask 1 topiq | 2 clip (+ aesthetic head) | 4 samp; default 7. The reference's
 * multi-pass mode runs one model group per pass over the same images (processing/multi_pass.py:481-644). */
int fe_ensemble_select(fe_ctx* ctx, int models);
/* fe_ensemble_score with the records left in device memory: d_records [n][ld_records] floats, ld_records >= FE_RECORD_FLOATS (further
 * columns are not touched). Returns once the engine stream has drained: the buffer can go straight into the multi-GPU all-gather
 * (RCCL reads it in place; there is no device -> host -> device hop in the step). */
int fe_ensemble_score_dev(fe_ctx* ctx, const uint8_t* rgb, int n, int h, int w, int on_device, float* d_records, int ld_records,
                          int* models_run);

/* fe_ensemble_score for a chunk of photos as a library holds them: every image has its own size. images[i] points to image i as
 * [h][w][3] RGB with (h, w) = hw[i] (hw is [n][2]); all pointers are host pointers (on_device = 0) or all device pointers, at any
 * alignment and anywhere relative to each other. records [n][FE_RECORD_FLOATS] (host) come back in input order; fields, models_run and
 * fe_ensemble_select as for fe_ensemble_score. Every image needs h >= 32 and w >= 32: a bad size or a null pointer returns
 * FE_ERR_INVALID, the message names the index of the image, nothing is launched.
 * Schedule: with TOPIQ selected the images are grouped by shape (order of first appearance, input order within a group) and cut into
 * micro-batches of at most fe_set_microbatch images of one shape; TOPIQ runs per micro-batch as in fe_ensemble_score (LANCZOS cap per
 * shape), in place when the images of a device micro-batch lie back to back, from a gathered copy otherwise. Without TOPIQ the
 * micro-batches are plain slices of the list. Either way the 224 x 224 CLIP and SAMP crops of a micro-batch come from one launch per
 * resampling pass over per-image descriptors, whatever the sizes, and gather across micro-batches - so across shapes - into the towers'
 * usual chunks. All coefficient tables of the call live in one call-scoped pool: no device allocation per image size, nothing cached. */
int fe_ensemble_score_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, float* records,
                            int* models_run);
/* The preprocessing kernels of fe_ensemble_score_mixed alone. mode FE_MIXED_CLIP: PIL BICUBIC, shorter side to 224, centre crop (open_clip's
 * eval transform); FE_MIXED_SAMP: PIL BILINEAR to 224 x 224 (torchvision Resize((224, 224))). crops [n][224][224][3] uint8 on the host,
 * byte for byte what Pillow gives. images / hw / on_device as above; any h, w >= 1. */
#define FE_MIXED_CLIP 0
#define FE_MIXED_SAMP 1
int fe_preprocess224_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int mode, uint8_t* crops);

/* ---- ONNX-subset graph runtime --------------------------------------------------------------------------------
 * Replaces the onnxruntime InferenceSessions that insightface.app.FaceAnalysis(name='buffalo_l') opens for the reference
 * (analyzers/face.py:30-38: det_10g.onnx, 2d106det.onnx, w600k_r50.onnx; invoked through face_app.get at :99). The
 * engine parses the .onnx bytes itself (no protobuf/onnx dependency) and executes the nodes on its own HIP kernels.
 * Supported operators: Conv (dense and depthwise), Gemm, MatMul (constant B), BatchNormalization, Relu, PRelu, LeakyRelu,
 * Sigmoid, Add/Sub/Mul/Div, MaxPool, AveragePool, GlobalAveragePool, Resize/Upsample (nearest asymmetric-floor, linear
 * half_pixel / pytorch_half_pixel; by sizes, or by scales that give whole pixels: in * scale must be an integer; rejected with
 * a "graph: Resize" error: other scales, pytorch_half_pixel with an output length of 1, every other mode), Concat (channels), Flatten, Reshape, Transpose, Squeeze, Unsqueeze, Softmax, Identity, Dropout, Constant and
 * the constant shape arithmetic exporters emit (Shape, Gather, Cast, Slice, Concat, Floor, Ceil). Anything else fails with
 * an error (fe_last_error) naming the operator. One float image input [N,C,H,W]. */
#define FE_GRAPH_SLOTS 8
/* Parses an .onnx buffer on the host only (no context, no GPU): counts and the declared input dims, or an error text.
 * Lets callers validate a model file before a device is involved. Returns FE_OK or FE_ERR_RUNTIME. */
int fe_onnx_probe(const void* onnx_bytes, size_t len, int* n_nodes, int* n_initializers, int* n_outputs, int64_t in_dims[4],
                  char* err, int err_cap);
enum fe_graph_slot { FE_GRAPH_FACE_DET = 0, FE_GRAPH_FACE_LMK = 1, FE_GRAPH_FACE_REC = 2 };
int fe_graph_load(fe_ctx* ctx, int slot, const void* onnx_bytes, size_t len);
int fe_graph_unload(fe_ctx* ctx, int slot);
int fe_graph_loaded(fe_ctx* ctx, int slot);
/* in_dims: the declared input shape (-1 = dynamic). flags: bit0 / bit1 = a node named Sub* / Mul* (or _minus* / _mul*)
 * is among the first 8 nodes, the probe insightface uses to choose input mean/std [DEP-KNOWLEDGE]. */
int fe_graph_info(fe_ctx* ctx, int slot, int* n_nodes, int* n_outputs, int64_t in_dims[4], int* flags);
/* x: fp32 NCHW (host, or device when on_device). Outputs stay inside the engine until the next run on this slot. */
int fe_graph_run(fe_ctx* ctx, int slot, const float* x, int n, int c, int h, int w, int on_device);
int fe_graph_output_info(fe_ctx* ctx, int slot, int i, char* name, int name_cap, int64_t dims[6], int* rank);
int fe_graph_output_copy(fe_ctx* ctx, int slot, int i, float* dst, size_t cap_floats);

/* ---- face path: what insightface's FaceAnalysis.get does around its three sessions (analyzers/face.py:99) -------------
 * [DEP-KNOWLEDGE: insightface model_zoo scrfd.py / landmark.py / arcface_onnx.py, utils/face_align.py; OpenCV resize/warpAffine]
 *
 * fe_face_detect = SCRFD.detect for a batch of equally sized BGR uint8 images: aspect-preserving cv2.resize (INTER_LINEAR)
 * into the top-left of a zero det_h x det_w canvas, blobFromImage((x-127.5)/128, swapRB), the graph in FE_GRAPH_FACE_DET,
 * then per stride: score >= thresh, distance2bbox / distance2kps from anchor centres, / det_scale. Candidates come back
 * unordered as 16 floats each: score, x1,y1,x2,y2, five (x,y) keypoints, stride level. counts[i] is the number found for
 * image i (only the first max_cand are stored). Sorting and NMS (tiny, data dependent) stay with the caller.
 * det_scale_out (nullable) receives new_height / h. */
int fe_face_detect(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int det_h, int det_w, float thresh,
                   int max_cand, float* cand, int* counts, float* det_scale_out);
/* Warps m square crops with cv2.warpAffine(img[img_index[f]], M[f] (2x3 forward matrix, row-major doubles), (size,size),
 * borderValue=0), applies blobFromImages((x-mean)*scale, swapRB) and runs graph `slot` on all crops in one batch; out
 * [m][out_dim] receives its first output. This is face_align.norm_crop + ArcFaceONNX.get_feat (size 112) and
 * face_align.transform + Landmark.get's forward (size 192). crops_out (nullable) receives the uint8 crops [m][size][size][3];
 * out may be null when only the crops are wanted. */
int fe_face_crops_run(fe_ctx* ctx, int slot, const uint8_t* bgr, int n, int h, int w, int on_device, int m, const int* img_index,
                      const double* M, int size, float mean, float scale, int swap_rb, float* out, int out_dim, uint8_t* crops_out);
/* FaceAnalysis.get(img) for a whole batch in ONE call (reference: face_app.get at analyzers/face.py:99, once per image):
 * fe_face_detect's pipeline, then on the host side of the engine score-sort + NMS(nms_thresh) per image, then for the best
 * max_faces faces of every image: Landmark.get (192-crop, graph FE_GRAPH_FACE_LMK, back-projection) and ArcFaceONNX.get
 * (5-point similarity crop 112, graph FE_GRAPH_FACE_REC), both batched over all faces of a micro-batch. Input normalisation
 * per graph follows insightface's Sub/Mul probe. faces [n][max_faces][FE_FACE_FLOATS]: bbox x1,y1,x2,y2, det_score,
 * kps[5][2], landmark_2d_106[106][2], embedding[512] (zeros for absent models / unused slots); counts[i] = faces that
 * survived NMS for image i (may exceed max_faces). models_run (nullable): 1 det | 2 landmarks | 4 recognition.
 * The fixed-size slots are what ranks all-gather in multi-GPU runs. */
#define FE_FACE_FLOATS 739
int fe_face_analyze(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int det_h, int det_w, float det_thresh,
                    float nms_thresh, int max_faces, float* faces, int* counts, int* models_run);
/* cv2.resize(img, (ow, oh)) with INTER_LINEAR on uint8 HWC 3-channel images, the fixed-point path OpenCV takes. */
int fe_cv_resize_linear_u8(fe_ctx* ctx, const uint8_t* src, int n, int h, int w, int oh, int ow, uint8_t* dst);

/* ---- per-image technical statistics ----------------------------------------------------------------
 * The scans reference analyzers/image_cache.py:28-33 (cv2.cvtColor BGR2GRAY / BGR2HSV, cv2.Laplacian(CV_64F).var()) and
 * analyzers/technical.py:39-342 (calcHist 256 / 180x256, saturation mean, percentiles, Immerkaer cv2.filter2D) run per image
 * on the CPU, as two HBM-bound GPU passes over a BGR uint8 batch. stats [n][FE_STATS_DOUBLES] (all exact integers except
 * [260]): [0..255] gray histogram counts; [256] sum and [257] sum of squares of the 4-neighbour Laplacian (reflect-101 border);
 * [258] sum |Immerkaer 3x3 response|; [259] sum of HSV saturation; [260] sum c*log2(c) over the 180x256 hue-saturation
 * histogram (entropy = log2(N) - [260]/N); [261..263] reserved. gray_out [n][h][w] / hsv_out [n][h][w][3] (nullable) return
 * the converted images themselves. facet_amd/image_stats.py turns the record into the reference's seven metric dicts. */
#define FE_STATS_DOUBLES 264
int fe_image_stats(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, double* stats, uint8_t* gray_out,
                   uint8_t* hsv_out);
/* The records of fe_image_stats for a list of images that each have their own size, in a fixed number of launches per chunk of the list:
 * every image's pixels are cut into segments that are spread over the device, so one large photo uses as many workgroups as its size
 * warrants. images [n] pointers to uint8 [h][w][3] images, hw [n][2] = h, w, on_device: as for fe_ensemble_score_mixed; device images may
 * sit at any byte alignment. Any h, w >= 1 with h * w < 2^31. order: the three bytes of a pixel are B,G,R (FE_ORDER_BGR, what
 * fe_image_stats takes) or R,G,B (FE_ORDER_RGB): an RGB batch needs no BGR copy. stats [n][FE_STATS_DOUBLES] (host) in input order, every
 * double equal to fe_image_stats's for that image, [260] included. Host images are staged chunk by chunk through the arena, device images
 * are read in place. There are no gray / HSV plane outputs: fe_image_stats is the call for those.
 * A null pointer, a bad size or a bad order returns FE_ERR_INVALID, the message names the index of the image, nothing is launched. An
 * image whose own scratch (its pixels when they are staged, h * w gray bytes, 184 320 bytes of histogram, its descriptors) exceeds the
 * arena returns FE_ERR_CAPACITY, the message names its index, nothing is launched. */
#define FE_ORDER_BGR 0
#define FE_ORDER_RGB 1
int fe_image_stats_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, double* stats);
/* Pixels per segment of fe_image_stats_mixed's first pass: 0 = the default, otherwise a multiple of 4096 that is at least 4096 (anything
 * else returns FE_ERR_INVALID and changes nothing). The records do not depend on it. */
int fe_set_stats_segment(fe_ctx* ctx, int pixels);

/* Laplacian statistics of m rectangular ROIs: what analyzers/face.py:160-176 (eye regions) and :272-279
 * (face crop) compute with cv2.cvtColor(roi, BGR2GRAY) + cv2.Laplacian(gray, CV_64F).var() + np.mean(gray) per face on the CPU.
 * rois [m][4] = x1,y1,x2,y2 (exclusive, already clipped to the image like the reference's slices); borders reflect (101) at
 * the ROI edge. out [m][4]: sum of Laplacian, sum of squares, sum of gray, pixel count (exact integers). Empty ROIs give 0s. */
int fe_roi_laplacian(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int m, const int* img_index, const int* rois,
                     double* out);

/* ---- the face calls for a list of images that each have their own size ---------------------------------------------------------------
 * images [n] pointers to uint8 [h][w][3] images, hw [n][2] = h, w, on_device, order: as for fe_image_stats_mixed (h, w within 1 .. 65535,
 * h * w below 2^31). Device images are read in place at any byte alignment, in the byte order `order` names: an RGB batch needs no BGR
 * copy. A null list, a null image pointer, n <= 0, a bad size, an image whose aspect ratio leaves an empty detector input, a bad order or
 * a bad det_h / det_w returns FE_ERR_INVALID; the message names the index of the image where one is at fault; the whole list is checked
 * before anything is launched. Host images go through the arena, each on a 256-byte boundary; one that cannot fit returns
 * FE_ERR_CAPACITY and the message names it. The cv2.resize weight tables of a call live in the arena for the length of the call: none
 * of these calls adds to the tables the per-shape calls keep per size (fe_face_cache_entries counts those).
 *
 * fe_face_analyze_mixed = fe_face_analyze over the list: micro-batches of 2 * fe_set_microbatch images whatever their shapes (host input:
 * fewer when their staged bytes pass a quarter of the arena). Per micro-batch one launch writes the detector's fp32 input from the source
 * images (resize into the corner of the zero canvas + blobFromImage), the detector runs on all of it, one copy brings counts and
 * candidates to the host for sort + NMS, and the landmark and recognition graphs run over ALL faces of the micro-batch, their crops warped
 * straight into the graphs' fp32 input. faces [n][max_faces][FE_FACE_FLOATS], counts [n], models_run: as for fe_face_analyze, in input
 * order; the same network outputs give the same records as fe_face_analyze of each image alone (a graph's summation order may depend on
 * the batch it runs in, so records agree to rounding, not to the bit).
 * fe_face_crops_run_mixed = fe_face_crops_run over the list (swap_rb as there: what it means for B,G,R pixels; R,G,B pixels reach the
 * graph in the same channel order). crops_out receives the bytes in the source's order. Host images are staged all at once.
 * fe_face_det_input_mixed: out [n][det_h][det_w][4] fp32 (host) = the detector input of every image. For the parity tests.
 * fe_roi_laplacian_mixed / fe_face_thumbnails_mixed = fe_roi_laplacian / fe_face_thumbnails with img_index into the list; every double
 * and every byte equals the per-shape call's. Host images are staged all at once. */
int fe_face_analyze_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int det_h, int det_w,
                          float det_thresh, float nms_thresh, int max_faces, float* faces, int* counts, int* models_run);
int fe_face_crops_run_mixed(fe_ctx* ctx, int slot, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int m,
                            const int* img_index, const double* M, int size, float mean, float scale, int swap_rb, float* out, int out_dim,
                            uint8_t* crops_out);
int fe_face_det_input_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int det_h, int det_w,
                            float* out);
int fe_roi_laplacian_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int m, const int* img_index,
                           const int* rois, double* out);
int fe_face_thumbnails_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int m,
                             const int32_t* img_index, const int32_t* crops, const int32_t* out_sizes, int quality, uint8_t* out, size_t cap,
                             int32_t* lengths);
/* entries: the number of cv2.resize weight tables the context keeps per (source length, target length): fe_face_detect, fe_face_analyze
 * and fe_cv_resize_linear_u8 add two with every new size, the mixed calls never do. */
int fe_face_cache_entries(fe_ctx* ctx, int32_t* entries);

/* The reference holds every image twice, as PIL RGB and as cv2 BGR (processing/batch_processor.py:200-215). With a resident batch
 * the second copy is made on the device: dst_device [pixels][3] = src [pixels][3] with the first and third byte of every pixel
 * exchanged. src: host (on_device = 0) or device memory; not in place. */
int fe_swap_rb_u8(fe_ctx* ctx, const uint8_t* src, int on_device, size_t pixels, uint8_t* dst_device);

/* Leading lines (last item): the reference's CompositionAnalyzer.detect_leading_lines (analyzers/composition.py:191-261)
 * runs cv2.GaussianBlur(gray, (5,5), 0), cv2.Canny(blurred, 50, 150) and cv2.HoughLinesP(edges, 1, pi/180, 80, minLineLength =
 * int(min(h,w)*0.15), maxLineGap = 20) per image on the CPU. Here the pixel scans (gray, 5x5 fixed-point blur, Sobel, L1 magnitude,
 * non-maximum suppression + thresholds) run on the GPU over the BGR batch; hysteresis and the progressive probabilistic Hough
 * transform (rho 1 px, theta 1 degree; a sequential, pseudo-random-order vote-and-erase loop) run on the host, one image per
 * thread. lines [n][max_lines][4] = x1,y1,x2,y2 in the order found, counts [n] = segments found per image (may exceed max_lines:
 * only the first max_lines are stored - call again with more room); both nullable together. edges_out [n][h][w] (nullable, host)
 * receives the Canny edge image (0 / 255). facet_amd/composition.py scores the segments as the reference does. */
int fe_leading_lines(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int canny_low, int canny_high, int threshold,
                     int min_line_length, int max_line_gap, int max_lines, int* lines, int* counts, uint8_t* edges_out);

/* External contours of binary images, as cv2.findContours(img, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) followed by cv2.contourArea /
 * cv2.moments / cv2.boundingRect of every contour would give them [DEP-KNOWLEDGE: OpenCV contours.cpp, moments.cpp; parity with
 * cv2 unpinned]. binary [n][h][w] uint8 on the host (on_device = 0) or the device, nonzero = foreground; the image is treated as
 * surrounded by background. Components are 8-connected. A component is external when it does not lie inside a hole of another
 * component, i.e. when the 4-connected background region left of its first pixel (raster order) reaches the image frame.
 * One record of FE_CONTOUR_FIELDS long longs per external contour: [0] start_index = y * w + x of the component's first pixel,
 * [1] a00, [2] a10, [3] a01 = the Green sums over the closed outer-border polygon through the pixel centres (consecutive border
 * points p, q, d = p.x q.y - q.x p.y: a00 += d, a10 += d (p.x + q.x), a01 += d (p.y + q.y)), so contourArea = |a00| / 2,
 * m00 = a00 / 2, m10 = a10 / 6, m01 = a01 / 6, the three moments negated when a00 < 0; [4..7] x_min, y_min, x_max, y_max
 * (inclusive; boundingRect = x_min, y_min, x_max - x_min + 1, y_max - y_min + 1). All fields are exact integers; CHAIN_APPROX_SIMPLE
 * only drops collinear points, which changes none of them.
 * A contour is reported when |a00| >= min_twice_area. records [n][max_contours][FE_CONTOUR_FIELDS], per image in descending
 * start_index order: findContours returns the contour it found last first [DEP-KNOWLEDGE]. counts [n] = contours reported per image
 * (may exceed max_contours: only the first max_contours are stored - call again with more room). A border walk that does not close
 * within 8 * (pixels of the component) + 8 steps makes the call fail (fe_last_error); it cannot for a well-formed labelling. */
#define FE_CONTOUR_FIELDS 8
int fe_external_contours(fe_ctx* ctx, const uint8_t* binary, int n, int h, int w, int on_device, long long min_twice_area, int max_contours,
                         long long* records, int* counts);

/* Subject region for photos without a face box: strategy 1 of the reference's CompositionAnalyzer.detect_subject_region
 * (analyzers/composition.py:16-75), which runs cv2.cvtColor(BGR2GRAY), np.median, cv2.Canny(gray, int(max(0, 0.5 median)),
 * int(min(255, 1.5 median))) and cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) per image on the CPU. Here every stage runs on
 * the device: gray and its histogram (the fe_image_stats pass), the median as twice its value m2 (an even pixel count takes the mean of
 * the two middle values) with lower = m2 / 4 and upper = min(255, 3 m2 / 4), the Canny front end of fe_leading_lines on the
 * un-blurred gray (3x3 Sobel, BORDER_REPLICATE, L1 magnitude, thresholds low < m, high < m) [DEP-KNOWLEDGE], hysteresis as a
 * connected-component labelling of the candidate map (a component stays when it owns a pixel above the upper threshold), and the
 * contours of fe_external_contours over the resulting edge image with min_twice_area = the smallest integer a with
 * a * 5000 >= h * w - a superset of the reference's `contourArea > h * w * 0.0001`, which the caller applies in floating point
 * (facet_amd/composition.py: subject_box). records / counts as in fe_external_contours; thresholds [n][2] (nullable) receives lower,
 * upper; edges_out [n][h][w] (nullable, host) the Canny edge image (0 / 255). Strategy 2 of the reference (cv2.saliency) is not built:
 * the module is absent from the opencv-python wheel the reference installs, so its fallback returns None there too. */
int fe_subject_region(fe_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int on_device, int max_contours, long long* records, int* counts,
                      int* thresholds, uint8_t* edges_out);

/* fe_leading_lines and fe_subject_region for a list of images that each have their own size: per arena chunk of the list every GPU stage
 * is ONE launch over the tiles of all its images (a workgroup finds its image by bisecting a table of cumulative tile counts; nothing is
 * described per tile), and the results of the chunk come down in one or two copies. images / hw / on_device / order: as for
 * fe_image_stats_mixed - host or device pointers to packed [h][w][3] uint8 at any byte alignment, hw [n][2] = h, w, order FE_ORDER_BGR or
 * FE_ORDER_RGB (the gray conversions read R, G, B in place: no swapped copy). Any h, w >= 1 with h * w below 2^30, the per-shape calls'
 * own bound. Results are in input order, and for every image every output equals what the per-shape call returns for that image alone:
 * each edge byte, threshold, segment and contour record, in the same order, and each count. edges_out (nullable, host) is ONE flat
 * buffer: image i starts at the sum of h * w of the images before it.
 * fe_leading_lines_mixed: min_line_length [n] is per image (the reference uses int(min(h, w) * 0.15)); lines [n][max_lines][4] and
 * counts [n] as in fe_leading_lines, nullable together. Hysteresis and the Hough transform run on up to 16 host threads that take the
 * chunk's images largest first from a shared cursor.
 * fe_subject_region_mixed: records [n][max_contours][FE_CONTOUR_FIELDS], counts [n] (exact also beyond max_contours) and thresholds
 * [n][2] (nullable) as in fe_subject_region.
 * A null list, n <= 0, a null image, a side below 1, h * w >= 2^30, a bad order or bad thresholds return FE_ERR_INVALID, the message names
 * the index of the image, nothing is launched. An image whose own scratch (8 bytes per pixel for the lines, about 55 for the subject
 * region, 3 more when the pixels are staged from the host) exceeds the arena returns FE_ERR_CAPACITY; the message names the image, its
 * size, the bytes needed and the bytes held, nothing is launched. */
int fe_leading_lines_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int canny_low,
                           int canny_high, int threshold, const int32_t* min_line_length, int max_line_gap, int max_lines, int* lines, int* counts,
                           uint8_t* edges_out);
int fe_subject_region_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, int max_contours,
                            long long* records, int* counts, int* thresholds, uint8_t* edges_out);
/* Milliseconds the host stage (hysteresis and Hough, over all chunks) of the context's last fe_leading_lines or fe_leading_lines_mixed
 * call took: the part of such a call that is host threads rather than kernels. For measurements (tools/perf_mixed.py --composition). */
int fe_lines_host_ms(fe_ctx* ctx, double* ms);

/* Perceptual hash: `imagehash.phash(pil_img)` with its defaults (hash_size 8, highfreq_factor 4), which the reference stores as
 * str(...) in the `phash` column for every image (processing/batch_processor.py:216, multi_pass.py:449, scorer.py:972):
 * image.convert('L') ((R*19595 + G*38470 + B*7471 + 0x8000) >> 16), .resize((32, 32), LANCZOS) (PIL's two-pass 22-bit fixed-point
 * resampler, horizontal pass first - vertical pass first for an image more than 100 times taller than wide, as Image.resize has it -
 * each pass clipped to uint8, a pass skipped when its axis is already 32),
 * scipy.fftpack.dct over axis 0 then axis 1 (unnormalised DCT-II, fp64), the top-left 8x8 block compared with its numpy.median.
 * img [n][h][w][3] uint8 on the host (on_device = 0) or the device, read once; bgr = 1: the bytes of a pixel are B,G,R.
 * hashes [n]: bit 63 = coefficient [0][0], row-major downwards, so the reference's string is the value as 16 lowercase hex
 * digits. small_out [n][32][32] uint8 (nullable): the resized gray image; dct_out [n][64] doubles (nullable): the 8x8 block,
 * row-major. A coefficient closer to the median than the rounding of the DCT (differences of up to 9e-11 from scipy were
 * observed; the tests allow 1e-6) may fall on either side. */
int fe_phash(fe_ctx* ctx, const uint8_t* img, int n, int h, int w, int bgr, int on_device, uint64_t* hashes, uint8_t* small_out,
             double* dct_out);
/* fe_phash for a list of images that each have their own size, in two launches per arena chunk of the list whatever the sizes: a wave
 * per image row over the rows of all images, then one workgroup per image. images / hw / on_device / order: as for fe_image_stats_mixed;
 * device images may sit at any byte alignment. Any h, w >= 1 within fe_phash's limits (w <= 32768, h <= 65536). hashes [n], small_out
 * [n][32][32] (nullable), dct_out [n][64] (nullable): in input order, every bit and every double equal to fe_phash's for that image
 * alone. The coefficient tables of the call - one per distinct side length, shared by the images that have it - live in one pool that is
 * uploaded once and dropped with the call: nothing is cached per size, unlike fe_phash. Host images are staged chunk by chunk through
 * the arena, device images are read in place.
 * A null pointer, a bad size or a bad order returns FE_ERR_INVALID, the message names the index of the image, nothing is launched. An
 * image whose own scratch (its pixels when they are staged, 32 bytes per row, its descriptor and outputs, next to the pool) exceeds the
 * arena returns FE_ERR_CAPACITY, the message names its index, nothing is launched. */
int fe_phash_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order, uint64_t* hashes,
                   uint8_t* small_out, double* dct_out);

/* fe_thumbnail_jpeg for a list of images that each have their own size and their own plan: reduce, the two LANCZOS passes and the five
 * encoder passes run once per arena chunk of the list, each over all images of the chunk. plans [n]: what
 * facet_amd.thumbnail.thumbnail_plan(w_i, h_i, size) gives - oh, ow: the thumbnail's size; fx, fy: the factors of Image.reduce (1, 1:
 * none) over the integer box reduce_box (x0, y0, x1, y1; read only when a factor exceeds 1); resize_box (x0, y0, x1, y1): the box of the
 * LANCZOS resize in pixels of the (reduced) image; tall: Image.resize's vertical-pass-first case. A plan with oh = h, ow = w, factors 1
 * and the whole-image box means the image is encoded as it is. images / hw / on_device / order: as for fe_image_stats_mixed (h * w below
 * 2^31); device images may sit at any byte alignment. out [n][cap], lengths [n], quality and FE_ERR_CAPACITY: fe_thumbnail_jpeg's
 * contract, with fe_jpeg_bound(max oh, max ow) as the bound that always fits; nothing is stored past a row. Every row holds the bytes
 * fe_thumbnail_jpeg writes for that image alone. The resize tables - one per distinct (input size, box, output size) - live in one pool
 * that is uploaded once and dropped with the call: nothing is cached per size, unlike fe_thumbnail_jpeg.
 * A null pointer, a bad size, a bad order, a bad quality or a plan that does not fit its image returns FE_ERR_INVALID, the message names
 * the index of the image, nothing is launched. */
typedef struct fe_thumb_plan {
  int32_t oh, ow, fx, fy;
  int32_t reduce_box[4];
  float resize_box[4];
  int32_t tall;
} fe_thumb_plan;
int fe_thumbnail_jpeg_mixed(fe_ctx* ctx, const uint8_t* const* images, const int32_t* hw, int n, int on_device, int order,
                            const fe_thumb_plan* plans, int quality, uint8_t* out, size_t cap, int32_t* lengths);

/* Number of per-size resampling tables the context holds (fe_resize_u8, fe_resize_u8_box, fe_phash and fe_thumbnail_jpeg add one or two
 * per new size and never free them; the mixed-size entry points add none). A counter for tests and leak hunts. */
int fe_resize_cache_entries(fe_ctx* ctx, int32_t* entries);

/* Near-duplicate search over stored hashes (reference utils/duplicate.py:89-119, an O(n^2) numpy loop): every pair i < j with
 * popcount(hashes[i] ^ hashes[j]) <= max_distance. hashes [n] on the host (on_device = 0) or the device. count receives the
 * exact number of such pairs; pairs [max_pairs][2] (host; nullable when max_pairs = 0) receives them in ascending (i, j) order
 * when count <= max_pairs. When count > max_pairs only count is defined - call again with more room. n < 2 gives count = 0. */
int fe_hamming_pairs(fe_ctx* ctx, const uint64_t* hashes, int n, int on_device, int max_distance, int64_t max_pairs, int32_t* pairs,
                     int64_t* count);

/* Burst detection over stored hashes (reference processing/scorer.py:1880-1986, `process_bursts`: a Python loop that compares each
 * photo with every member of the open burst and parses both date strings per comparison). Rows are in the reference's order
 * (`ORDER BY date_taken`). link [n] (host) receives, per row i, the largest j < i with similar(i, j), or -1:
 *   both rows have FE_BURST_HAS_DATE, d = |times[i] - times[j]|, dist = popcount(hashes[i] ^ hashes[j]), or 999 unless both rows
 *   have FE_BURST_HAS_HASH, and
 *     d <= window_s and dist <= thr, or
 *     d <= rapid_s and dist <= 2 thr and the rows share a person (either list empty, or the lists intersect).
 * The open burst of the reference is the run [s, i-1], so row i joins it exactly when link[i] >= s; that recurrence and the choice
 * of the lead are the caller's (facet_amd/bursts.py). hashes [n] on the host (on_device = 0) or the device (fe_phash's output in
 * place); times [n] seconds (any epoch, |t| <= 2^61; ignored without FE_BURST_HAS_DATE) and flags [n] on the host. person_off
 * [n + 1] / person_ids [n_person_ids] (host): CSR lists of int32 ids, ascending and distinct within a row; both null = no row has a
 * person. thr, window_s and rapid_s are the reference's settings already floored to integers; any value is accepted (a negative
 * one lets no pair pass its rule). The lower end of each row's search is exact for any row order (prefix maximum of the times, made on
 * the host). n < 2 launches nothing (link[0] = -1). Null pointers, flags outside the two bits, times out of range, offsets that are
 * not monotone within 0 .. n_person_ids and lists that are not ascending return FE_ERR_INVALID with a message and launch nothing. */
#define FE_BURST_HAS_HASH 1
#define FE_BURST_HAS_DATE 2
int fe_burst_links(fe_ctx* ctx, const uint64_t* hashes, int on_device, const int64_t* times, const uint8_t* flags, int n,
                   const int32_t* person_off, const int32_t* person_ids, int n_person_ids, int thr, int64_t window_s, int64_t rapid_s,
                   int32_t* link);

/* Face clustering (reference faces/clusterer.py): `FaceClusterer.cluster_faces` L2-normalises the stored ArcFace embeddings
 * (:157-158) and runs HDBSCAN on them (:188-197 with the `hdbscan` package's approximate boruvka_balltree, or cuML on an NVIDIA GPU
 * :167-181). The three calls below are the O(n^2 d) parts as exact sweeps on the fp32 matrix cores; the n x n matrix is never
 * stored. The tree condensing and the person bookkeeping are host code (facet_amd/face_cluster.py).
 * Common: x [n][d] fp32 rows on the host (on_device = 0) or the device; 2 <= n <= 262144, d a multiple of 32 in 32 .. 1024;
 * normalise = 1: rows become x / (|x| + 1e-10) in fp32 first (clusterer.py:158), 0: rows are used as they are (unit length
 * expected). Anything else returns FE_ERR_INVALID. Squared distances are swept as |a|^2 + |b|^2 - 2 a.b (>= 0) in fp32; every
 * distance that is RETURNED is recomputed from direct differences in fp64, so only the choice of a neighbour or an edge rests on the
 * swept value (error below 2 d 2^-24 for unit rows).
 *
 * fe_knn_core_distances: core [n] = distance to the k-th nearest row, the row itself being the first (1 <= k <= min(32, n)), as
 * `hdbscan` and sklearn.cluster.HDBSCAN define min_samples; core_idx [n] (nullable) = that neighbour. */
int fe_knn_core_distances(fe_ctx* ctx, const float* x, int n, int d, int on_device, int normalise, int k, double* core,
                          int32_t* core_idx);

/* fe_mreach_mst: minimum spanning tree of the mutual-reachability graph mr(i, j) = max(core_i, core_j, |x_i - x_j|) by Boruvka
 * rounds: every row's lightest edge to another component comes from one sweep, edges are ordered by (fp32 bits of the swept mr^2,
 * min(i, j), max(i, j)) - one value from both ends, so no round closes a cycle. edge_u / edge_v / edge_w [n - 1] (host): the edges
 * (u < v) in the order they were accepted, edge_w = max(core_u, core_v, exact distance). core [n] (nullable): as above. rounds
 * (nullable): sweeps used, at most ceil(log2 n) + 1 - more is an error. The same input gives the same bytes on every run. */
int fe_mreach_mst(fe_ctx* ctx, const float* x, int n, int d, int on_device, int normalise, int k, int32_t* edge_u, int32_t* edge_v,
                  double* edge_w, double* core, int32_t* rounds);

/* fe_cosine_best_match: for every query row the candidate row of largest cosine similarity (the centroid loops of
 * clusterer.py:399-405 and :508-518). q [nq][d], c [nc][d] on the host, 1 <= nq, nc <= 262144; both are normalised inside.
 * best_sim [nq] fp32, best_idx [nq]: the first candidate among equals. Thresholds stay with the caller. */
int fe_cosine_best_match(fe_ctx* ctx, const float* q, int nq, const float* c, int nc, int d, float* best_sim, int32_t* best_idx);

/* Similar photos and person-merge suggestions: two more sweeps of the clustering tile core, rows = queries Q [nq][d], columns =
 * candidates C [n][d] (1 <= nq, n <= 262144; d a multiple of 32 in 32 .. 1024), the nq x n matrix never stored.
 *   "similar photos" (reference api/routers/gallery.py:410-539) scores one photo against every other one:
 *       s = wc (cos + 1) / 2 [the query has an embedding]
 *         + wp |Pq n Pc| / max(|Pq|, |Pc|)              [both person sets non-empty]
 *         + wd D(|floor((tq - tc) / 86400)|)            [both dates present]   D(0) = 1, D(<= 7) = 0.5, D(<= 30) = 0.2, else
 *                                                                             max(0, 1 - days / 365); the signed difference is
 *                                                                             floored first, as Python's abs(timedelta.days)
 *                                                                             does: one second later is a day, one second
 *                                                                             earlier is none
 *         + ws max(0, 1 - |aq - ac| / 10)               [both aggregates present and non-zero]
 *     with weights = {wc, wp, wd, ws} (the reference's defaults are 0.4, 0.3, 0.2, 0.1), every operation one fp32 rounding;
 *     cos is the dot product of the normalised rows. score_kind = FE_SIM_FUSED.
 *   person merge suggestions (reference faces/merge_analyzer.py:29-187) need the plain cosine: score_kind = FE_SIM_COSINE, the
 *     metadata and the weights are not read.
 * A candidate is dropped when it is the query itself (q_self [nq], host, candidate index or -1; nullable), when visible [n] (host,
 * uint8, nullable) is 0 for it, or - fused score only - when s <= 0 (the reference's `if total_similarity > 0`); a NaN score is dropped.
 *
 * fe_sim_rows describes one side. emb and the metadata arrays all live on the host (on_device = 0) or all on the device, so a
 * library can be uploaded once and stay resident between calls; normalise = 1: rows become x / (|x| + 1e-10) in fp32 first, as in
 * the clustering calls, 0: they are used as they are (unit length expected; resident rows are then read in place). Metadata
 * pointers may be null (= absent for every row). person_off [n + 1] / person_ids: CSR lists of dense int32 person ids, ascending
 * and unique within a row, of any length. The same pointer, n and flags on both sides prepare the rows once (Q == C).
 * With nq <= 8 the sweep is a single read of C by one wave per candidate row (no matrix tile); its dot products are summed in
 * another order than the tile path's, so a query scored alone and in a batch of more than 8 may differ in the last bits.
 * Bad shapes, k, kinds or null pointers return FE_ERR_INVALID with a message and launch nothing; the context stays usable. */
#define FE_SIM_FUSED 0
#define FE_SIM_COSINE 1
#define FE_SIM_K_MAX 32
#define FE_SIM_NO_DATE INT64_MIN
typedef struct fe_sim_rows {
  const float* emb;          /* [n][d] */
  int32_t n;
  int32_t on_device;         /* where emb and the five arrays below live */
  int32_t normalise;
  int32_t n_person_ids;      /* length of person_ids */
  const uint8_t* has_emb;    /* [n], 0: the row has no embedding (its emb row is not used as a query term); read on the query side only -
                                a candidate without one is masked out through `visible`, as the reference's SQL does */
  const int64_t* date;       /* [n] seconds, FE_SIM_NO_DATE = absent */
  const float* aggregate;    /* [n], 0 or NaN = absent */
  const int32_t* person_off; /* [n + 1] */
  const int32_t* person_ids;
} fe_sim_rows;

/* fe_similar_topk: per query the k best candidates (1 <= k <= FE_SIM_K_MAX) under the order (score descending, candidate index
 * ascending). idx [nq][k] (-1 padded), score [nq][k] fp32 (0 padded), host. The same input gives the same bytes on every run. */
int fe_similar_topk(fe_ctx* ctx, const fe_sim_rows* q, const fe_sim_rows* c, int d, int score_kind, const float* weights,
                    const int32_t* q_self, const uint8_t* visible, int k, int32_t* idx, float* score);

/* fe_similar_pairs: every (query, candidate) with score >= thr; thr (host) holds one value (n_thr = 1) or one per query (n_thr =
 * nq). upper = 1 (Q == C): only candidate index > query index. The fe_hamming_pairs protocol: count receives the exact number;
 * pairs [max_pairs][2] = (query, candidate) and scores [max_pairs] (host; nullable when max_pairs = 0) receive them in ascending
 * (query, candidate) order when count <= max_pairs, otherwise only count is defined - call again with more room. */
int fe_similar_pairs(fe_ctx* ctx, const fe_sim_rows* q, const fe_sim_rows* c, int d, int score_kind, const float* weights,
                     const int32_t* q_self, const uint8_t* visible, const float* thr, int n_thr, int upper, int64_t max_pairs,
                     int32_t* pairs, float* scores, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* FACET_ENGINE_H */
