"""Checkpoint key/shape specs of the hot-path models and seeded synthetic checkpoints.

No weight files exist offline, so benches and parity tests use synthetic checkpoints:
every tensor is drawn from numpy's PCG64 keyed by (seed, crc32(name)) with fan-in scaled magnitudes, under
the *real* checkpoint key names (timm resnet50 / pyiqa CFANet / open_clip VisionTransformer / the
reference's in-tree SAMPNet + U2NETP, models/samp_net.py). A real checkpoint loads through the same
Engine.load_weights(name -> tensor) path.
"""
import zlib

import numpy as np

# ---------------------------------------------------------------------------------------------------
# spec builders: list of (name, shape, kind)
# ---------------------------------------------------------------------------------------------------

def _conv(spec, name, cout, cin, kh, kw=None, bias=False):
    spec.append((name + ".weight", (cout, cin, kh, kw if kw is not None else kh), "conv"))
    if bias:
        spec.append((name + ".bias", (cout,), "bias"))


def _bn(spec, name, c, last=False, kind=None):
    spec.append((name + ".weight", (c,), kind or ("bn_w_last" if last else "bn_w")))
    spec.append((name + ".bias", (c,), "bn_b"))
    spec.append((name + ".running_mean", (c,), "bn_mean"))
    spec.append((name + ".running_var", (c,), "bn_var"))


def _linear(spec, name, out, inp, bias=True):
    spec.append((name + ".weight", (out, inp), "linear"))
    if bias:
        spec.append((name + ".bias", (out,), "bias"))


def _ln(spec, name, d):
    spec.append((name + ".weight", (d,), "ln_w"))
    spec.append((name + ".bias", (d,), "ln_b"))


def resnet_spec(prefix, bottleneck, blocks, seq_names=False):
    """timm/torchvision ResNet keys (conv1,bn1,layerL.B.convK,...); seq_names=True gives the
    nn.Sequential(*children[:-2]) numbering used by reference models/samp_net.py:652-662."""
    spec = []
    n = (lambda plain, seq: prefix + (str(seq) if seq_names else plain))
    _conv(spec, n("conv1", 0), 64, 3, 7)
    _bn(spec, n("bn1", 1), 64)
    inpl = 64
    exp = 4 if bottleneck else 1
    for li, nb in enumerate(blocks):
        planes = 64 * 2 ** li
        lp = prefix + (str(4 + li) if seq_names else f"layer{li + 1}")
        for bi in range(nb):
            bp = f"{lp}.{bi}"
            stride = 2 if (bi == 0 and li > 0) else 1
            if bottleneck:
                _conv(spec, bp + ".conv1", planes, inpl, 1); _bn(spec, bp + ".bn1", planes)
                _conv(spec, bp + ".conv2", planes, planes, 3); _bn(spec, bp + ".bn2", planes)
                _conv(spec, bp + ".conv3", planes * 4, planes, 1); _bn(spec, bp + ".bn3", planes * 4, last=True)
            else:
                _conv(spec, bp + ".conv1", planes, inpl, 3); _bn(spec, bp + ".bn1", planes)
                _conv(spec, bp + ".conv2", planes, planes, 3); _bn(spec, bp + ".bn2", planes, last=True)
            if stride != 1 or inpl != planes * exp:
                _conv(spec, bp + ".downsample.0", planes * exp, inpl, 1)
                _bn(spec, bp + ".downsample.1", planes * exp)
            inpl = planes * exp
    return spec


def _mha(spec, name, d):
    spec.append((name + ".in_proj_weight", (3 * d, d), "linear"))
    spec.append((name + ".in_proj_bias", (3 * d,), "bias"))
    _linear(spec, name + ".out_proj", d, d)


def _enc_layer(spec, name, d, ff):
    _mha(spec, name + ".self_attn", d)
    _linear(spec, name + ".linear1", ff, d)
    _linear(spec, name + ".linear2", d, ff)
    _ln(spec, name + ".norm1", d)
    _ln(spec, name + ".norm2", d)


def _dec_layer(spec, name, d, ff):
    # (pyiqa's decoder layer also owns an unused `self_attn`; its forward is cross-attention only)
    _mha(spec, name + ".multihead_attn", d)
    _linear(spec, name + ".linear1", ff, d)
    _linear(spec, name + ".linear2", d, ff)
    _ln(spec, name + ".norm1", d)
    _ln(spec, name + ".norm2", d)
    _ln(spec, name + ".norm3", d)


TOPIQ_DIMS = [64, 256, 512, 1024, 2048]
TOPIQ_INTER = 256
TOPIQ_FF = 1024


def topiq_spec():
    """pyiqa CFANet (topiq_nr: resnet50, use_ref=False, inter_dim=256, 4 heads, 1 attn layer). [DEP-KNOWLEDGE]"""
    spec = resnet_spec("semantic_model.", True, [3, 4, 6, 3])
    d, ff = TOPIQ_INTER, TOPIQ_FF
    for i, dim in enumerate(TOPIQ_DIMS):
        g = f"weight_pool.{i}"
        _conv(spec, g + ".splitconv", dim * 2, dim, 1, bias=True)
        _conv(spec, g + ".weight_blk.0", 64, dim, 1, bias=True)
        _conv(spec, g + ".weight_blk.2", 64, 64, 3, bias=True)
        _conv(spec, g + ".weight_blk.4", 1, 64, 3, bias=True)
        _conv(spec, f"dim_reduce.{i}.0", d, dim, 1, bias=True)
        _enc_layer(spec, f"sa_attn_blks.{i}.layers.0", d, ff)
    for i in range(len(TOPIQ_DIMS) - 1):
        _dec_layer(spec, f"attn_blks.{i}.layers.0", d, ff)
    _enc_layer(spec, "attn_pool", d, ff)
    _ln(spec, "score_linear.0", d)
    _linear(spec, "score_linear.1", d, d)
    _ln(spec, "score_linear.3", d)
    _linear(spec, "score_linear.4", d, d)
    _linear(spec, "score_linear.6", 1, d)
    spec.append(("h_emb", (1, d // 2, 32, 1), "emb"))
    spec.append(("w_emb", (1, d // 2, 1, 32), "emb"))
    return spec


def clip_vit_spec(width=1024, layers=24, patch=14, grid=16, out_dim=768):
    """open_clip VisionTransformer (ViT-L/14) keys under `visual.` [DEP-KNOWLEDGE]."""
    spec = []
    p = "visual."
    spec.append((p + "conv1.weight", (width, 3, patch, patch), "conv"))
    spec.append((p + "class_embedding", (width,), "emb"))
    spec.append((p + "positional_embedding", (grid * grid + 1, width), "emb"))
    _ln(spec, p + "ln_pre", width)
    for i in range(layers):
        b = f"{p}transformer.resblocks.{i}"
        _ln(spec, b + ".ln_1", width)
        spec.append((b + ".attn.in_proj_weight", (3 * width, width), "linear"))
        spec.append((b + ".attn.in_proj_bias", (3 * width,), "bias"))
        _linear(spec, b + ".attn.out_proj", width, width)
        _ln(spec, b + ".ln_2", width)
        _linear(spec, b + ".mlp.c_fc", width * 4, width)
        _linear(spec, b + ".mlp.c_proj", width, width * 4)
    _ln(spec, p + "ln_post", width)
    spec.append((p + "proj", (width, out_dim), "proj"))
    return spec


def clip_text_spec(width=768, layers=12, ctx=77, vocab=49408, out_dim=768):
    """open_clip CLIP text tower keys (top level of the CLIP checkpoint, next to `visual.*`) [DEP-KNOWLEDGE]."""
    spec = [("token_embedding.weight", (vocab, width), "emb"), ("positional_embedding", (ctx, width), "emb")]
    for i in range(layers):
        b = f"transformer.resblocks.{i}"
        _ln(spec, b + ".ln_1", width)
        spec.append((b + ".attn.in_proj_weight", (3 * width, width), "linear"))
        spec.append((b + ".attn.in_proj_bias", (3 * width,), "bias"))
        _linear(spec, b + ".attn.out_proj", width, width)
        _ln(spec, b + ".ln_2", width)
        _linear(spec, b + ".mlp.c_fc", width * 4, width)
        _linear(spec, b + ".mlp.c_proj", width, width * 4)
    _ln(spec, "ln_final", width)
    spec.append(("text_projection", (width, out_dim), "proj"))
    return spec


def aesthetic_spec():
    """Linear(768,256)-ReLU-Linear(256,1), reference processing/scorer.py:579-583."""
    spec = []
    _linear(spec, "0", 256, 768)
    _linear(spec, "2", 1, 256)
    return spec


_RSU = {  # name -> (depth, dilated)
    "stage1": (7, False), "stage2": (6, False), "stage3": (5, False), "stage4": (4, False),
    "stage5": (4, True), "stage6": (4, True),
    "stage5d": (4, True), "stage4d": (4, False), "stage3d": (5, False), "stage2d": (6, False), "stage1d": (7, False),
}
_RSU_IN = {"stage1": 3, "stage2": 64, "stage3": 64, "stage4": 64, "stage5": 64, "stage6": 64,
           "stage5d": 128, "stage4d": 128, "stage3d": 128, "stage2d": 128, "stage1d": 128}


def rsu_convs(depth, in_ch, mid=16, out=64):
    """(name, cin, cout) of the REBNCONV units of one RSU block (reference models/samp_net.py:62-255)."""
    convs = [("rebnconvin", in_ch, out), ("rebnconv1", out, mid)]
    for k in range(2, depth + 1):
        convs.append((f"rebnconv{k}", mid, mid))
    for k in range(depth - 1, 1, -1):
        convs.append((f"rebnconv{k}d", mid * 2, mid))
    convs.append(("rebnconv1d", mid * 2, out))
    return convs


def u2netp_spec(prefix=""):
    spec = []
    for st, (depth, _dil) in _RSU.items():
        for name, cin, cout in rsu_convs(depth, _RSU_IN[st]):
            _conv(spec, f"{prefix}{st}.{name}.conv_s1", cout, cin, 3, bias=True)
            _bn(spec, f"{prefix}{st}.{name}.bn_s1", cout, kind="bn_w_half")
    for k in range(1, 7):
        spec.append((f"{prefix}side{k}.weight", (1, 64, 3, 3), "conv_small"))
        spec.append((f"{prefix}side{k}.bias", (1,), "bias"))
    _conv(spec, f"{prefix}outconv", 1, 6, 1, bias=True)
    return spec


SAMP_PATTERN_SHAPES = [(1296, 2, 1), (1296, 1, 2), (1373, 2, 1), (1373, 2, 1), (1296, 2, 1), (1296, 2, 2),
                       (1324, 2, 2), (836, 3, 3)]


def sampnet_spec():
    """Reference models/samp_net.py:665-758 (all Linear/Conv bias-free)."""
    spec = resnet_spec("backbone.", False, [2, 2, 2, 2], seq_names=True)
    _linear(spec, "pattern_weight_layer.3", 8, 512, bias=False)
    for i, (c, kh, kw) in enumerate(SAMP_PATTERN_SHAPES):
        spec.append((f"pattern_module.conv_list.{i}.0.weight", (1024, c, kh, kw), "conv"))
    _linear(spec, "att_feature_layer.0", 512, 1024, bias=False)
    _linear(spec, "att_pred_layer.0", 6, 512, bias=False)
    _linear(spec, "com_feature_layer.0", 512, 1024, bias=False)
    _linear(spec, "alpha_predict_layer.0", 2, 1024, bias=False)
    _linear(spec, "com_pred_layer.0", 1024, 1024, bias=False)
    _linear(spec, "com_pred_layer.3", 512, 1024, bias=False)
    _linear(spec, "com_pred_layer.5", 5, 512, bias=False)
    return spec


def qwen2_5_vl_text_spec(hidden=3584, layers=28, heads=28, kv_heads=4, inter=18944, vocab=152064):
    """Text decoder of transformers' Qwen2_5_VLForConditionalGeneration (the class models/vlm_tagger.py:163-184 instantiates), its
    state-dict key names (transformers 5.x: model.language_model.*, lm_head.weight). Defaults = Qwen2.5-VL-7B-Instruct's geometry
    (head_dim 128, q/k/v with bias, untied lm_head)."""
    hd = hidden // heads
    spec = [("model.language_model.embed_tokens.weight", (vocab, hidden), "emb1")]
    for i in range(layers):
        p = f"model.language_model.layers.{i}"
        _linear(spec, p + ".self_attn.q_proj", heads * hd, hidden)
        _linear(spec, p + ".self_attn.k_proj", kv_heads * hd, hidden)
        _linear(spec, p + ".self_attn.v_proj", kv_heads * hd, hidden)
        _linear(spec, p + ".self_attn.o_proj", hidden, heads * hd, bias=False)
        _linear(spec, p + ".mlp.gate_proj", inter, hidden, bias=False)
        _linear(spec, p + ".mlp.up_proj", inter, hidden, bias=False)
        _linear(spec, p + ".mlp.down_proj", hidden, inter, bias=False)
        spec.append((p + ".input_layernorm.weight", (hidden,), "ln_w"))
        spec.append((p + ".post_attention_layernorm.weight", (hidden,), "ln_w"))
    spec.append(("model.language_model.norm.weight", (hidden,), "ln_w"))
    spec.append(("lm_head.weight", (vocab, hidden), "linear"))
    return spec


def qwen2_5_vl_vision_spec(hidden=1280, depth=32, inter=3420, out_hidden=3584, patch=14, temporal=2):
    """Vision tower of Qwen2_5_VLForConditionalGeneration (`model.visual.*`): Conv3d patch embedding (no bias), `depth` blocks of
    RMSNorm - fused qkv (+bias) - proj (+bias) - RMSNorm - SwiGLU MLP (+biases), the patch merger (RMSNorm, Linear(4 hidden, 4 hidden),
    GELU, Linear(4 hidden, out_hidden)). Defaults = Qwen2.5-VL-7B-Instruct (16 heads of 80)."""
    v = "model.visual."
    spec = [(v + "patch_embed.proj.weight", (hidden, 3, temporal, patch, patch), "linear_nd")]
    for i in range(depth):
        b = f"{v}blocks.{i}"
        spec.append((b + ".norm1.weight", (hidden,), "ln_w"))
        spec.append((b + ".norm2.weight", (hidden,), "ln_w"))
        _linear(spec, b + ".attn.qkv", 3 * hidden, hidden)
        _linear(spec, b + ".attn.proj", hidden, hidden)
        _linear(spec, b + ".mlp.gate_proj", inter, hidden)
        _linear(spec, b + ".mlp.up_proj", inter, hidden)
        _linear(spec, b + ".mlp.down_proj", hidden, inter)
    spec.append((v + "merger.ln_q.weight", (hidden,), "ln_w"))
    _linear(spec, v + "merger.mlp.0", 4 * hidden, 4 * hidden)
    _linear(spec, v + "merger.mlp.2", out_hidden, 4 * hidden)
    return spec


def qwen3_vl_text_spec(hidden=2048, layers=28, heads=16, kv_heads=8, inter=6144, vocab=151936, tied=True):
    """Text decoder of transformers' Qwen3VLForConditionalGeneration (model.language_model.*): q / k / v WITHOUT bias, q_norm / k_norm
    over each head's 128 dims, SwiGLU MLP; lm_head tied to embed_tokens (no lm_head.weight) unless tied=False. Defaults = Qwen3-VL-2B."""
    hd = 128
    # (a tied table is also the read-out: 1 / sqrt(hidden) scale keeps its logits O(1); an untied one is unit scale as Qwen2.5-VL's)
    spec = [("model.language_model.embed_tokens.weight", (vocab, hidden), "linear" if tied else "emb1")]
    for i in range(layers):
        p = f"model.language_model.layers.{i}"
        _linear(spec, p + ".self_attn.q_proj", heads * hd, hidden, bias=False)
        _linear(spec, p + ".self_attn.k_proj", kv_heads * hd, hidden, bias=False)
        _linear(spec, p + ".self_attn.v_proj", kv_heads * hd, hidden, bias=False)
        _linear(spec, p + ".self_attn.o_proj", hidden, heads * hd, bias=False)
        spec.append((p + ".self_attn.q_norm.weight", (hd,), "ln_w"))
        spec.append((p + ".self_attn.k_norm.weight", (hd,), "ln_w"))
        _linear(spec, p + ".mlp.gate_proj", inter, hidden, bias=False)
        _linear(spec, p + ".mlp.up_proj", inter, hidden, bias=False)
        _linear(spec, p + ".mlp.down_proj", hidden, inter, bias=False)
        spec.append((p + ".input_layernorm.weight", (hidden,), "ln_w"))
        spec.append((p + ".post_attention_layernorm.weight", (hidden,), "ln_w"))
    spec.append(("model.language_model.norm.weight", (hidden,), "ln_w"))
    if not tied:
        spec.append(("lm_head.weight", (vocab, hidden), "linear"))
    return spec


def qwen3_vl_vision_spec(hidden=1024, depth=24, inter=4096, out_hidden=2048, patch=16, temporal=2, n_pos=2304, n_deepstack=3):
    """Vision tower of Qwen3VLForConditionalGeneration (`model.visual.*`): Conv3d patch embedding with bias, learned position table, `depth`
    blocks of LayerNorm (+bias) - fused qkv (+bias) - proj (+bias) - LayerNorm - fc1 / fc2 (+biases, tanh GELU), the final merger
    (LayerNorm over hidden) and n_deepstack DeepStack mergers (LayerNorm over 4 hidden). Defaults = Qwen3-VL-2B (16 heads of 64)."""
    v = "model.visual."
    spec = [(v + "patch_embed.proj.weight", (hidden, 3, temporal, patch, patch), "linear_nd"), (v + "patch_embed.proj.bias", (hidden,), "bias"),
            (v + "pos_embed.weight", (n_pos, hidden), "emb1")]
    for i in range(depth):
        b = f"{v}blocks.{i}"
        for n in ("norm1", "norm2"):
            spec.append((f"{b}.{n}.weight", (hidden,), "ln_w"))
            spec.append((f"{b}.{n}.bias", (hidden,), "ln_b"))
        _linear(spec, b + ".attn.qkv", 3 * hidden, hidden)
        _linear(spec, b + ".attn.proj", hidden, hidden)
        _linear(spec, b + ".mlp.linear_fc1", inter, hidden)
        _linear(spec, b + ".mlp.linear_fc2", hidden, inter)
    for name, width in [("merger", hidden)] + [(f"deepstack_merger_list.{k}", 4 * hidden) for k in range(n_deepstack)]:
        spec.append((f"{v}{name}.norm.weight", (width,), "ln_w"))
        spec.append((f"{v}{name}.norm.bias", (width,), "ln_b"))
        _linear(spec, f"{v}{name}.linear_fc1", 4 * hidden, 4 * hidden)
        _linear(spec, f"{v}{name}.linear_fc2", out_hidden, 4 * hidden)
    return spec


def qwen2_vl_text_spec(hidden=1536, layers=28, heads=12, kv_heads=2, inter=8960, vocab=151936, tied=True):
    """Text decoder of transformers' Qwen2VLForConditionalGeneration (the composition model of the 24gb profile): the Qwen2.5-VL layer
    (head_dim 128, q / k / v with bias, SwiGLU MLP); lm_head tied to embed_tokens (no lm_head.weight) unless tied=False. Defaults =
    Qwen2-VL-2B-Instruct (12 heads over 2 KV heads: GQA group 6)."""
    spec = qwen2_5_vl_text_spec(hidden, layers, heads, kv_heads, inter, vocab)
    if tied:      # (a tied table is also the read-out: the 1 / sqrt(hidden) scale keeps its logits O(1), as qwen3_vl_text_spec does)
        spec = [(n, s, "linear" if n.endswith("embed_tokens.weight") else k) for n, s, k in spec if n != "lm_head.weight"]
    return spec


def qwen2_vl_vision_spec(hidden=1280, depth=32, inter=5120, out_hidden=1536, patch=14, temporal=2):
    """Vision tower of Qwen2VLForConditionalGeneration (`model.visual.*`): Conv3d patch embedding (no bias), `depth` blocks of LayerNorm
    (+bias) - fused qkv (+bias) - proj (+bias) - LayerNorm - fc1 / QuickGELU / fc2 (+biases), the patch merger (LayerNorm ln_q,
    Linear(4 hidden, 4 hidden), GELU, Linear(4 hidden, out_hidden)). Defaults = Qwen2-VL-2B-Instruct (16 heads of 80)."""
    v = "model.visual."
    spec = [(v + "patch_embed.proj.weight", (hidden, 3, temporal, patch, patch), "linear_nd")]
    for i in range(depth):
        b = f"{v}blocks.{i}"
        for n in ("norm1", "norm2"):
            spec.append((f"{b}.{n}.weight", (hidden,), "ln_w"))
            spec.append((f"{b}.{n}.bias", (hidden,), "ln_b"))
        _linear(spec, b + ".attn.qkv", 3 * hidden, hidden)
        _linear(spec, b + ".attn.proj", hidden, hidden)
        _linear(spec, b + ".mlp.fc1", inter, hidden)
        _linear(spec, b + ".mlp.fc2", hidden, inter)
    spec.append((v + "merger.ln_q.weight", (hidden,), "ln_w"))
    spec.append((v + "merger.ln_q.bias", (hidden,), "ln_b"))
    _linear(spec, v + "merger.mlp.0", 4 * hidden, 4 * hidden)
    _linear(spec, v + "merger.mlp.2", out_hidden, 4 * hidden)
    return spec


# the reduced Qwen3-VL of the parity tests (tests/golden/make_vlm3_golden.py): head_dim 128 with 2:1 grouped KV heads in the decoder,
# head_dim 64 in the tower, an 8 x 8 position table, DeepStack after three non-contiguous blocks including the last
VLM3_TINY = dict(hidden=256, layers=4, heads=4, kv_heads=2, inter=512, vocab=2048)
VLM3_VISION_TINY = dict(hidden=128, depth=4, inter=256, out_hidden=256, n_pos=64, n_deepstack=3)
VLM3_TINY_DEEPSTACK = (0, 2, 3)

# reduced vision tower of the parity tests: Qwen2.5-VL's head_dim 80, window attention with one full-attention block
VLM_VISION_TINY = dict(hidden=160, depth=3, inter=320, out_hidden=512)

# the reduced-depth configuration of the VLM parity tests (tests/golden/make_vlm_golden.py): Qwen2.5-VL's head_dim 128 and 2:1 grouped
# KV heads at a size the CPU oracle generates from in seconds
VLM_TINY = dict(hidden=512, layers=4, heads=4, kv_heads=2, inter=1408, vocab=2048)

# the reduced Qwen2-VL of the parity tests (tests/golden/make_vlm2_golden.py): the 2B checkpoint's GQA group of 6 (6 heads over 1 KV head of
# 128) in the decoder, head_dim 80 and mlp_ratio 4 in the tower
VLM2_TINY = dict(hidden=768, layers=4, heads=6, kv_heads=1, inter=1408, vocab=2048)
VLM2_VISION_TINY = dict(hidden=160, depth=4, inter=640, out_hidden=768)

SPECS = {
    "qwen2_5_vl_text": qwen2_5_vl_text_spec,
    "qwen2_5_vl_text_tiny": lambda: qwen2_5_vl_text_spec(**VLM_TINY),
    "qwen2_5_vl_tiny": lambda: qwen2_5_vl_text_spec(**VLM_TINY) + qwen2_5_vl_vision_spec(**VLM_VISION_TINY),
    "qwen3_vl_text": qwen3_vl_text_spec,
    "qwen3_vl_2b": lambda: qwen3_vl_text_spec() + qwen3_vl_vision_spec(),
    "qwen3_vl_tiny": lambda: qwen3_vl_text_spec(**VLM3_TINY) + qwen3_vl_vision_spec(**VLM3_VISION_TINY),
    "qwen3_vl_tiny_untied": lambda: qwen3_vl_text_spec(**VLM3_TINY, tied=False) + qwen3_vl_vision_spec(**VLM3_VISION_TINY),
    "qwen2_vl_text": qwen2_vl_text_spec,
    "qwen2_vl_2b": lambda: qwen2_vl_text_spec() + qwen2_vl_vision_spec(),
    "qwen2_vl_tiny": lambda: qwen2_vl_text_spec(**VLM2_TINY) + qwen2_vl_vision_spec(**VLM2_VISION_TINY),
    "qwen2_vl_tiny_untied": lambda: qwen2_vl_text_spec(**VLM2_TINY, tied=False) + qwen2_vl_vision_spec(**VLM2_VISION_TINY),
    "topiq": topiq_spec,
    "resnet50": lambda: resnet_spec("semantic_model.", True, [3, 4, 6, 3]),
    "clip": clip_vit_spec,
    "clip_text": clip_text_spec,
    "clip_full": lambda: clip_vit_spec() + clip_text_spec(),
    "aesthetic": aesthetic_spec,
    "u2netp": u2netp_spec,
    "samp_net": sampnet_spec,
}


# ---------------------------------------------------------------------------------------------------
# seeded synthetic tensors
# ---------------------------------------------------------------------------------------------------

def _draw(rng, shape, kind):
    shape = tuple(int(s) for s in shape)
    if kind == "conv":
        fan_in = shape[1] * shape[2] * shape[3]
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_in))
    if kind == "conv_small":  # U2-Net-P side heads: keeps the fused saliency logit out of sigmoid saturation
        fan_in = shape[1] * shape[2] * shape[3]
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(0.7 * np.sqrt(2.0 / fan_in))
    if kind == "bn_w_half":
        return rng.uniform(0.6, 0.9, shape).astype(np.float32)
    if kind == "linear":
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(1.0 / np.sqrt(shape[1]))
    if kind == "linear_nd":      # a linear map stored with an N-d kernel (Conv3d patch embedding): fan-in = everything but the first axis
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(1.0 / np.sqrt(np.prod(shape[1:])))
    if kind == "proj":
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(1.0 / np.sqrt(shape[0]))
    if kind == "bias":
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(0.05)
    if kind == "bn_w":
        return rng.uniform(0.8, 1.2, shape).astype(np.float32)
    if kind == "bn_w_last":  # keeps residual sums tame over 16 blocks
        return rng.uniform(0.2, 0.4, shape).astype(np.float32)
    if kind == "bn_b":
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(0.1)
    if kind == "bn_mean":
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(0.1)
    if kind == "bn_var":
        return rng.uniform(0.8, 1.2, shape).astype(np.float32)
    if kind == "ln_w":
        return rng.uniform(0.8, 1.2, shape).astype(np.float32)
    if kind == "ln_b":
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(0.1)
    if kind == "emb":
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02)
    if kind == "emb1":      # token embeddings of a pre-norm decoder (RMSNorm rescales them; unit scale keeps bf16 away from its subnormals)
        return rng.standard_normal(shape, dtype=np.float32)
    raise ValueError(kind)


def synthetic_state_dict(model, seed=0, spec=None):
    """name -> float32 ndarray for `model` in SPECS (or an explicit spec list)."""
    spec = spec if spec is not None else SPECS[model]()
    out = {}
    for name, shape, kind in spec:
        rng = np.random.default_rng([int(seed), zlib.crc32(name.encode())])
        out[name] = _draw(rng, shape, kind)
    return out


def synthetic_images(seed, n, h, w):
    """uint8 HWC RGB, default_rng(seed).integers(0,256)."""
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------
# e4m3 weight rows of the VLM decoders (Engine.vlm_weight_format("fp8")): facet_amd/csrc/fp8_core.h restated in numpy
# ---------------------------------------------------------------------------------------------------

def _round_bf16(w):
    """float32 -> the nearest-even bfloat16 value, as float32 (what the engine stores for a Linear weight)."""
    u = np.ascontiguousarray(w, np.float32).view(np.uint32)          # (finite inputs: the sum below stays inside 32 bits)
    return ((u + np.uint32(0x7FFF) + ((u >> 16) & 1)) & np.uint32(0xFFFF0000)).view(np.float32)


def _e4m3_values():
    c = np.arange(256)
    E, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    v = np.where(E == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (E.astype(np.float64) - 10))
    v[(E == 15) & ((c & 7) == 7)] = np.nan
    return np.where(c & 0x80, -v, v).astype(np.float32)


def quantize_e4m3_rows(w):
    """w [N, K] float -> (codes uint8 [N, K], exponents int8 [N]): what a commit under vlm_weight_format("fp8") stores for a Linear
    weight. w is rounded to bf16 first, as the engine does; row n then gets the smallest exponent e_n with max|w[n]| * 2^-e_n <= 448
    (frexp; 0 for a zero row; clamped to >= -117) and codes w[n] * 2^-e_n rounded to nearest-even OCP e4m3. NaN / Inf raise."""
    w = np.asarray(w, np.float32)
    if w.ndim != 2:
        raise ValueError("quantize_e4m3_rows takes a [rows, K] matrix")
    if not np.isfinite(w).all() or not np.isfinite(w := _round_bf16(w)).all():
        raise ValueError("quantize_e4m3_rows: NaN or Inf in the weight")
    a = np.abs(w).max(1) if w.shape[1] else np.zeros(w.shape[0], np.float32)
    f, x = np.frexp(a)                                  # a = f * 2^x, f in [0.5, 1); 448 = 0.875 * 2^9
    e = np.where(a > 0, np.where(f <= 0.875, x - 9, x - 8), 0)
    e = np.maximum(e, -117).astype(np.int32)
    s = np.ldexp(w, -e[:, None])                        # float32, exact; |s| <= 448 by the choice of e
    u = s.view(np.uint32)
    sign = ((u >> 24) & 0x80).astype(np.uint8)
    u = u & 0x7FFFFFFF
    # nearest even at 3 mantissa bits on the fp32 bit pattern (e4m3's exponent field is fp32's minus 120); below 2^-6 the grid has step
    # 2^-9, which is the ulp of 2^14 + |s| in fp32 (the addition rounds to nearest even)
    normal = (((u + 0x7FFFF + ((u >> 20) & 1)) >> 20) - (120 << 3)).astype(np.uint8)
    sub = ((u.view(np.float32) + np.float32(16384.0)).view(np.uint32) - 0x46800000).astype(np.uint8)
    codes = np.where(u < 0x3C800000, sub, normal) | sign
    return codes, e.astype(np.int8)


def dequantize_e4m3_rows(codes, exponents):
    """(codes uint8 [N, K], exponents int8 [N]) -> float32 [N, K]: decode(code) * 2^e, every value exactly a bf16 value."""
    codes = np.asarray(codes, np.uint8)
    e = np.asarray(exponents).astype(np.int32)
    return np.ldexp(_e4m3_values()[codes], e[:, None])          # float32: exact, the result is a bf16 value


def checkpoint_or_synthetic(kind, weights_path, synthetic, seed, loader):
    """The state dict the drop-in wrappers load. A real checkpoint path wins. Without one the reference would download the weights
    (pyiqa / open_clip / the aesthetic head, models/pyiqa_scorer.py:108, model_manager.py:140, processing/scorer.py:560-577) and fail
    loudly when it cannot; there is no network here, so the wrappers raise FileNotFoundError instead of scoring with made-up
    weights - unless the caller opts in with synthetic=True or FACET_AMD_SYNTHETIC=1 (tests, bench.py, tools/)."""
    import os
    if weights_path:
        return loader(weights_path)
    if synthetic or os.environ.get("FACET_AMD_SYNTHETIC") == "1":
        return synthetic_state_dict(kind, seed)
    raise FileNotFoundError(
        f"no {kind} checkpoint path given. Pass weights_path=... (a local .safetensors / .pth file); the seeded synthetic checkpoint "
        "is only used when asked for explicitly (synthetic=True or FACET_AMD_SYNTHETIC=1) because its scores are meaningless.")
