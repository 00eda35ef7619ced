"""A stand-in for the Qwen2.5-VL tokenizer in tests and tools (the real one ships inside the checkpoint, not available offline).

Character-level and deterministic, over the reduced vocabulary of the tiny test model (2048 ids): the special tokens of the chat text map
to fixed ids, every other character to 10 + code point mod 1900. `decode` maps ids back to lowercase letters and commas, so generated ids
turn into comma-separated "tags" the tagger's parser can take.
"""
import re

SPECIAL = {"<|image_pad|>": 2000, "<|video_pad|>": 2001, "<|vision_start|>": 2002, "<|vision_end|>": 2003, "<|im_start|>": 2004,
           "<|im_end|>": 2005, "<|endoftext|>": 2006}
TOKENS = dict(image_token_id=2000, vision_start_token_id=2002, vision_end_token_id=2003, pad_token_id=2006, eos_token_ids=(2005, 2006))
_SPLIT = re.compile("(" + "|".join(re.escape(k) for k in SPECIAL) + ")")


def encode(text):
    ids = []
    for piece in _SPLIT.split(text):
        if piece in SPECIAL:
            ids.append(SPECIAL[piece])
        else:
            ids.extend(10 + ord(ch) % 1900 for ch in piece)
    return ids


def decode(ids):
    """skip_special_tokens=True: ids of the special tokens vanish."""
    out = []
    for t in ids:
        t = int(t)
        if t in SPECIAL.values():
            continue
        out.append("," if t % 7 == 0 else chr(97 + t % 26))
    return "".join(out)
