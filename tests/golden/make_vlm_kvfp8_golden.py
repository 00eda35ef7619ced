"""Golden vectors for the e4m3 KV cache of the VLM decoders (Engine.vlm_kv_format("fp8")) from an independent implementation:
transformers' own `Qwen2_5_VLForConditionalGeneration`, built and seeded as make_vlm_golden.py does (the planted read-out), running greedy
`generate` on the CPU in bfloat16 over a cache whose layers keep every appended K / V row as
dequantize_e4m3_rows(quantize_e4m3_rows(row)) - the format's numpy statement in facet_amd/weights.py. As transformers' QuantizedCache does
on its first update, a layer returns the UNQUANTISED states for the prompt's own attention and the stored ones afterwards, so the
prefill is the plain model's and every decode step attends to quantised rows (its own token's included).

Stores prompts (B = 2, L = 24), the 40 generated token ids, the first and last steps' logits, every step's top logit and the top-2
margins. Asserts that the smallest margin exceeds 1.0 and that the logits differ from the plain-cache run somewhere (the golden shows the
format at work), and prints both. Run in the build container:  python tests/golden/make_vlm_kvfp8_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from facet_amd.weights import VLM_TINY, dequantize_e4m3_rows, quantize_e4m3_rows  # noqa: E402
from make_vlm_golden import MROPE, RMS_EPS, ROPE_THETA, build  # noqa: E402

from transformers.cache_utils import Cache, DynamicCache, DynamicLayer  # noqa: E402

OUT = os.path.join(HERE, "vlm_kvfp8_golden.npz")


def image(x):
    """bf16 tensor [..., 128] -> the quantise-dequantise image of every row, as bf16 (every image value is exactly a bf16 value)"""
    rows = x.float().numpy().reshape(-1, x.shape[-1])
    img = dequantize_e4m3_rows(*quantize_e4m3_rows(rows))
    out = torch.from_numpy(img.reshape(x.shape)).to(x.dtype)
    assert np.array_equal(out.float().numpy(), img.reshape(x.shape))
    return out


class E4m3Layer(DynamicLayer):
    def update(self, key_states, value_states, *args, **kwargs):
        first = not self.is_initialized
        if first:
            self.lazy_initialization(key_states, value_states)
        self.keys = torch.cat([self.keys, image(key_states)], dim=-2)
        self.values = torch.cat([self.values, image(value_states)], dim=-2)
        return (key_states, value_states) if first else (self.keys, self.values)


class E4m3Cache(DynamicCache):
    def __init__(self):
        Cache.__init__(self, layer_class_to_replicate=E4m3Layer)


def run(m, prompts, new_tokens, cache=None):
    ids = torch.from_numpy(prompts)
    with torch.no_grad():
        out = m.generate(input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=new_tokens, do_sample=False, output_logits=True,
                         return_dict_in_generate=True, pad_token_id=0, eos_token_id=None, past_key_values=cache)
    toks = out.sequences[:, prompts.shape[1]:].numpy().astype(np.int32)
    logits = torch.stack(out.logits, 1).float().numpy()        # [B][new][vocab], the bf16 logits widened
    top2 = np.sort(logits, -1)[..., -2:]
    return toks, logits, (top2[..., 1] - top2[..., 0])


def main():
    B, L, NEW, seed = 2, 24, 40, 16
    prompts = np.random.default_rng(2000 + seed).integers(0, VLM_TINY["vocab"], (B, L)).astype(np.int64)
    m = build(seed)
    cache = E4m3Cache()
    toks, logits, margin = run(m, prompts, NEW, cache)
    assert all(isinstance(layer, E4m3Layer) and layer.keys.shape[-2] == L + NEW - 1 for layer in cache.layers), "the model did not go through the e4m3 layers"
    toks_p, logits_p, margin_p = run(m, prompts, NEW)
    diff = np.abs(logits - logits_p)
    print(f"seed {seed}: e4m3 cache: min top-2 margin {margin.min():.3f}, logit scale {np.abs(logits).max():.2f}, {len(np.unique(toks))} distinct tokens")
    print(f"against the plain cache: ids equal on {int((toks == toks_p).sum())} of {toks.size}, |logit diff| max {diff.max():.4f} mean {diff.mean():.5f}; "
          f"step 0 (the prefill) max {diff[:, 0].max():.4f}; plain min margin {margin_p.min():.3f}")
    assert margin.min() > 1.0
    assert diff[:, 0].max() == 0.0, "the prefill must be the plain model's"
    assert diff[:, 1:].max() > 0.0, "the format left no trace in the logits"
    np.savez_compressed(OUT, seed_w=seed, prompts=prompts.astype(np.int32), tokens=toks, margin=margin.astype(np.float32),
                        logits_step0=logits[:, 0].astype(np.float32), logits_last=logits[:, -1].astype(np.float32),
                        top_logit=logits.max(-1).astype(np.float32), plain_tokens=toks_p, plain_diff_max=np.float32(diff.max()),
                        mrope_section=np.asarray(MROPE, np.int32), rope_theta=np.float32(ROPE_THETA), rms_eps=np.float32(RMS_EPS),
                        **{k: np.int32(v) for k, v in VLM_TINY.items()})
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
