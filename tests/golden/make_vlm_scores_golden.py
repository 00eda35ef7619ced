"""Golden vectors for the VLM tagger's confidence scores (tag_image_with_scores, models/vlm_tagger.py:497-626) from the reference's own
classes: transformers' Qwen2_5_VLForConditionalGeneration (reduced config with the vision tower, make_vlm_vision_golden.py) and
Qwen3VLForConditionalGeneration (make_vlm3_golden.py), each with the planted read-out (lm_head = a permutation of the embeddings / 16: wide
margins, so greedy ids are comparable) and unplanted.

Per family, one photo through Qwen2VLImageProcessorPil (the tagger's defaults for Qwen2.5-VL; 16-pixel patches, mean / std 0.5 and small
min / max pixels for Qwen3-VL) with the tagger's chat text and the stand-in tokenizer of standins/vlm_tokenizer.py:
  - planted, `generate(output_scores=True, return_dict_in_generate=True)` with an end-of-sequence id: the id the run emits at step
    EOS_STEP, declared as EOS in the generation config (and as a special token of the shim), so the run stops there, before
    max_new_tokens. Stored: the generated ids (through the EOS), every step's scores (the fp32 copies of the bf16 logits) and log_softmax
    at the chosen ids;
  - the dict the reference's own VLMTagger.tag_image_with_scores(PIL image) returns for that photo, its `.model` the planted model and
    its `.processor` a shim over the image processor and the stand-in tokenizer;
  - unplanted (Qwen3-VL: tied), no EOS: greedy ids and per-step logits (the GPU test teacher-forces those ids).
Reproducible across x86 hosts: torch's portable CPU kernels (ATEN_CPU_CAPABILITY=default, oneDNN off), one thread.
    python tests/golden/make_vlm_scores_golden.py
"""
import os
import sys

os.environ["ATEN_CPU_CAPABILITY"] = "default"
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.backends.mkldnn.enabled = False
torch.set_num_threads(1)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
import make_vlm3_golden as V3  # noqa: E402
import make_vlm_vision_golden as V2  # noqa: E402
from facet_amd.weights import synthetic_state_dict  # noqa: E402
from facet_amd.vlm_tagger import VLMTagger as Mirror, chat_text, expand_image_pads  # noqa: E402
from standins import vlm_tokenizer as T  # noqa: E402

OUT = os.path.join(HERE, "vlm_scores_golden.npz")
SEED, NEW, EOS_STEP = 16, 16, 9


def processor(family):
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil
    if family == "qwen3":
        return Qwen2VLImageProcessorPil(patch_size=16, merge_size=2, temporal_patch_size=2, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5],
                                        size={"shortest_edge": V3.PHOTO_MIN_PIXELS, "longest_edge": V3.PHOTO_MAX_PIXELS})
    return Qwen2VLImageProcessorPil()


class Shim:
    """The processor calls the reference's tag_image_with_scores makes, over the image processor and the stand-in tokenizer; `eos` is a
    special token here (decodes to "" with skip_special_tokens=True)."""

    def __init__(self, family, eos):
        self.family, self.eos, self.ip = family, eos, processor(family)

    def _inputs(self, text, image):
        r = self.ip(images=[image], return_tensors="np")
        grid = np.asarray(r["image_grid_thw"], np.int64)
        ids = np.asarray([T.encode(expand_image_pads(text, grid))], np.int64)
        return {"input_ids": torch.from_numpy(ids), "attention_mask": torch.ones_like(torch.from_numpy(ids)),
                "pixel_values": torch.from_numpy(np.asarray(r["pixel_values"], np.float32)), "image_grid_thw": torch.from_numpy(grid),
                "mm_token_type_ids": torch.from_numpy((ids == T.TOKENS["image_token_id"]).astype(np.int32))}

    def apply_chat_template(self, messages, tokenize=False, add_generation_prompt=True, return_dict=False, return_tensors=None):
        image, prompt = messages[0]["content"][0]["image"], messages[0]["content"][1]["text"]
        text = chat_text(prompt, self.family)
        return self._inputs(text, image) if tokenize else text

    def __call__(self, text, images, return_tensors="pt", padding=True):
        return self._inputs(text[0], images[0])

    def decode(self, ids, skip_special_tokens=True):
        ids = [int(t) for t in ids]
        if skip_special_tokens:
            return T.decode([t for t in ids if t != self.eos])
        lit = {v: k for k, v in T.SPECIAL.items()}
        lit[self.eos] = "<|eos|>"
        return "".join(lit[t] if t in lit else T.decode([t]) for t in ids)


def build(family, plant):
    if family == "qwen3":
        return V3.build(SEED, plant=plant)
    m = V2.build(SEED)
    if not plant:
        sd = synthetic_state_dict("qwen2_5_vl_tiny", SEED)
        m.load_state_dict({k: torch.from_numpy(v).to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    return m


def generate(m, inputs, eos):
    m.generation_config.eos_token_id = eos
    m.generation_config.pad_token_id = eos if eos is not None else T.TOKENS["pad_token_id"]
    with torch.no_grad():
        out = m.generate(**inputs, max_new_tokens=NEW, do_sample=False, output_scores=True, output_logits=True, return_dict_in_generate=True)
    L = inputs["input_ids"].shape[1]
    ids = out.sequences[0, L:].numpy().astype(np.int32)
    scores = torch.stack(out.scores, 1)[0].float()
    lp = np.array([torch.log_softmax(scores[s], dim=-1)[int(t)].item() for s, t in enumerate(ids)], np.float32)
    return ids, scores.numpy().astype(np.float32), lp


def main():
    from PIL import Image
    rng = np.random.default_rng(33)
    photos = {"qwen2_5": rng.integers(0, 256, (70, 90, 3), dtype=np.uint8), "qwen3": rng.integers(0, 256, (90, 120, 3), dtype=np.uint8)}
    out = {}
    for family, path in (("qwen2_5", "Qwen/Qwen2.5-VL-7B-Instruct"), ("qwen3", "Qwen/Qwen3-VL-2B-Instruct")):
        pil = Image.fromarray(photos[family], "RGB")
        m = build(family, True)
        probe = Shim(family, -1)
        inputs = probe._inputs(probe.apply_chat_template([{"content": [{"image": pil}, {"text": Mirror._fallback_prompt()}]}]), pil)
        free, _, _ = generate(m, inputs, None)
        eos = int(free[EOS_STEP])
        assert eos not in free[:EOS_STEP] and eos not in T.SPECIAL.values(), free
        ids, scores, lp = generate(m, inputs, eos)
        assert len(ids) == EOS_STEP + 1 and ids[-1] == eos and np.array_equal(ids, free[:EOS_STEP + 1])
        top2 = np.sort(scores, -1)[:, -2:]
        print(family, "eos", eos, "ids", ids.tolist(), "lp", lp.round(4).tolist(), "margin min", float((top2[:, 1] - top2[:, 0]).min()))
        # the reference's own method on the PIL photo
        from models.vlm_tagger import VLMTagger
        cfg = {"model_path": path, "max_new_tokens": NEW}
        if family == "qwen3":
            cfg.update(min_pixels=V3.PHOTO_MIN_PIXELS, max_pixels=V3.PHOTO_MAX_PIXELS)
        ref = VLMTagger(cfg)
        ref.model, ref.processor = m, Shim(family, eos)
        res = ref.tag_image_with_scores(pil)
        print(family, "reference tag_image_with_scores", res)
        assert res, "no tags: the comparison needs some"
        mu = build(family, False)
        uids, ulogits, ulp = generate(mu, inputs, None)
        top2 = np.sort(ulogits, -1)[:, -2:]
        print(family, "unplanted ids", uids.tolist(), "|max|", float(np.abs(ulogits).max()), "margin min", float((top2[:, 1] - top2[:, 0]).min()))
        out.update({f"{family}_photo": photos[family], f"{family}_eos": np.int32(eos), f"{family}_input_ids": inputs["input_ids"].numpy().astype(np.int32),
                    f"{family}_ids": ids, f"{family}_scores": scores, f"{family}_logprobs": lp,
                    f"{family}_tags": np.array(list(res.keys())), f"{family}_confidences": np.array(list(res.values()), np.float64),
                    f"{family}_unplanted_ids": uids, f"{family}_unplanted_logits": ulogits, f"{family}_unplanted_logprobs": ulp})
    out.update(seed_w=np.int32(SEED), max_new_tokens=np.int32(NEW), photo_min_pixels=np.int32(V3.PHOTO_MIN_PIXELS), photo_max_pixels=np.int32(V3.PHOTO_MAX_PIXELS))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
