"""Generates tests/golden/vlm_scores_host_golden.json by RUNNING THE REFERENCE'S OWN VLMTagger.tag_image_with_scores and
get_tags_with_scores (models/vlm_tagger.py:497-626) in the build container. Its `.model` is a scripted stub whose `generate` returns fixed
`sequences` / `scores` (what HF returns at batch 1: the generated ids stop at, and include, the first EOS); its `.processor` is a shim over
the stand-in tokenizer of standins/vlm_tokenizer.py, extended by a few multi-character tokens (real BPE tokens such as "sky,sun" carry a
comma inside a word). Per case the file stores the generated ids, the log-probs the reference takes from the scores (fp32 log_softmax at the
chosen ids), the text of every token, and what the reference returned for max_tags 5 / 2 and thresholds 0 / 0.3 / 1.

    python tests/golden/make_vlm_scores_host_golden.py
"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference")
from models.vlm_tagger import VLMTagger  # noqa: E402
from standins import vlm_tokenizer as T  # noqa: E402

VOCAB = 2048
EOS = T.TOKENS["eos_token_ids"][0]
MULTI = {1995: "sky,sun", 1996: "cat dog", 1997: ", ", 1998: "tree,"}      # multi-character tokens of the shim
LITERAL = {v: k for k, v in T.SPECIAL.items()}


def token_text(tid, skip_special):
    if tid in LITERAL:
        return "" if skip_special else LITERAL[tid]
    return MULTI.get(tid, T.decode([tid]))


def ids_for(text):
    """Stand-in ids spelling `text` (lowercase letters and commas; '#' = the EOS id, '{n}' = multi-character token n)."""
    out, i, k = [], 0, 0
    while i < len(text):
        ch = text[i]
        if ch == "#":
            out.append(EOS)
        elif ch == "{":
            j = text.index("}", i)
            out.append(int(text[i + 1:j]))
            i = j
        elif ch == ",":
            out.append(7 * (3 + k % 200))
            k += 1
        else:
            t = next(t for t in range(26 + ord(ch) - 97, 1990, 26) if t % 7 and t >= 10)
            out.append(t + 26 * (k % 5) * 7)       # (several ids per letter; all decode to the same character)
            k += 1
        i += 1
    for t in out:
        assert token_text(t, True) == (MULTI.get(t) or ("" if t in LITERAL else T.decode([t])))
    return out


class Shim:
    """The processor calls tag_image_with_scores makes (qwen2_5 family)."""

    def apply_chat_template(self, messages, tokenize=False, add_generation_prompt=True):
        return "<|im_start|>user\n<|vision_start|><|image_pad|><|vision_end|>tags<|im_end|>\n<|im_start|>assistant\n"

    def __call__(self, text, images, return_tensors="pt", padding=True):
        return {"input_ids": torch.tensor([T.encode(text[0])], dtype=torch.long)}

    def decode(self, ids, skip_special_tokens=True):
        return "".join(token_text(int(t), skip_special_tokens) for t in ids)


class Stub:
    """`generate` returns the scripted ids and per-step fp32 scores (bf16-representable logits, as HF's scores are the fp32 copies of
    the bf16 logits); `spike` steps have every other logit at -1e4 (log-prob exactly 0)."""
    device = "cpu"

    def __init__(self, gen, seed, spikes=()):
        self.gen = gen
        rng = np.random.default_rng(seed)
        sc = rng.normal(0, 3, (max(len(gen), 1), VOCAB)).astype(np.float32)
        for s, t in enumerate(gen):
            sc[s, t] += float(rng.uniform(2, 12))                 # the chosen id stands out by a varying margin
            if s in spikes:
                sc[s, :] = -1e4
                sc[s, t] = 5.0
        self.scores = torch.from_numpy(sc).to(torch.bfloat16).float()

    def generate(self, input_ids, max_new_tokens, do_sample, output_scores, return_dict_in_generate, **kw):
        assert not do_sample and output_scores and return_dict_in_generate
        g = torch.tensor([self.gen], dtype=torch.long).reshape(1, -1)
        return SimpleNamespace(sequences=torch.cat([input_ids, g], 1), scores=tuple(self.scores[s][None] for s in range(len(self.gen))))


class Cfg:
    def get_categories(self):
        return [{"name": "subject", "tags": {"cat": [], "dog": [], "bird": [], "sky": []}}]

    def get_tag_vocabulary(self):
        return {"cat": [], "dog": [], "bird": [], "sky": []}

    config = {"standalone_tags": {}}


CASES = [  # name, text, max_new_tokens, with vocabulary, spike steps
    ("eos_inside", "cat,dog,bird#", 20, False, ()),
    ("no_eos", "sky,tree,grass,wat", 18, False, ()),
    ("leading_comma", ",cat,dog#", 20, False, ()),
    ("adjacent_commas", "cat,,dog,bird#", 20, False, ()),
    ("single_char_and_duplicates", "a,cat,cat,b,dog,x,owl#", 30, False, ()),
    ("more_tags_than_segments", "cat{1995}{1998}owl#", 20, False, ()),
    ("multi_token_words", "{1996}{1997}bird,{1995}#", 20, False, ()),
    ("clamped_at_one", "cat,dog#", 20, False, (0, 1, 2)),
    ("empty_output", "#", 20, False, ()),
    ("only_commas", ",,,#", 20, False, ()),
    ("vocabulary_merges", "cta,dgo,cat,bird,skyy#", 30, True, ()),
    ("many_tags", "ab,cd,ef,gh,ij,kl,mn#", 30, False, ()),
]


def main():
    out = {"eos_token_ids": list(T.TOKENS["eos_token_ids"]), "cases": []}
    for i, (name, text, new, vocab, spikes) in enumerate(CASES):
        gen = ids_for(text)
        assert len(gen) <= new
        stub = Stub(gen, 100 + i, spikes)
        lps = [torch.log_softmax(stub.scores[s], dim=-1)[t].item() for s, t in enumerate(gen)]
        res = {}
        for mt in (5, 2):
            t = VLMTagger({"model_path": "Qwen/Qwen2.5-VL-7B-Instruct", "max_new_tokens": new}, Cfg() if vocab else None)
            t.model, t.processor = stub, Shim()
            res[f"max_tags_{mt}"] = t.tag_image_with_scores(None, max_tags=mt)
        thr = {}
        for th in (0.0, 0.3, 1.0):
            t = VLMTagger({"model_path": "Qwen/Qwen2.5-VL-7B-Instruct", "max_new_tokens": new}, Cfg() if vocab else None)
            t.model, t.processor = stub, Shim()
            thr[repr(th)] = t.get_tags_with_scores(None, threshold=th)
        case = {"name": name, "max_new_tokens": new, "vocabulary": vocab, "ids": gen, "logprobs": lps,
                "token_text": {str(t): token_text(t, True) for t in sorted(set(gen))}, "text": Shim().decode(gen),
                "result": {k: [[tag, c] for tag, c in v.items()] for k, v in res.items()},
                "threshold": {k: [[tag, c] for tag, c in v.items()] for k, v in thr.items()}}
        print(name, repr(case["text"]), res["max_tags_5"], {k: len(v) for k, v in thr.items()})
        out["cases"].append(case)
    path = os.path.join(HERE, "vlm_scores_host_golden.json")
    json.dump(out, open(path, "w"), indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
