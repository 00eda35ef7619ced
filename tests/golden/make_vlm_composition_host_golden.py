"""Generates tests/golden/vlm_composition_host_golden.json by RUNNING THE REFERENCE'S OWN VLMCompositionAnalyzer
(models/vlm_composition.py) in the build container with a stub model_dict: its COMPOSITION_PROMPT, and what its _parse_response returns
for a list of response strings (well-formed; score 0 / 11 / 7.5; lower-case labels; missing score; missing explanation; multi-line
explanation; every element word; empty). Only the strings and the recorded results are stored.

    python tests/golden/make_vlm_composition_host_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from models.vlm_composition import VLMCompositionAnalyzer  # noqa: E402

RESPONSES = [
    "SCORE: 8\nEXPLANATION: The subject sits on a rule of thirds intersection and the leading lines draw the eye.",
    "SCORE: 0\nEXPLANATION: Nothing works here.",
    "SCORE: 11\nEXPLANATION: Beyond the scale.",
    "SCORE: 7.5\nEXPLANATION: Good balance and symmetry.",
    "score: 6\nexplanation: lower-case labels with strong framing.",
    "Score:3\nExplanation:no space after the colon",
    "EXPLANATION: There is no score line, only depth and layering.",
    "SCORE: 4",
    "SCORE: 9\nEXPLANATION: First line of the explanation.\nSecond line mentions negative space.\nThird line.",
    "SCORE: 5\nEXPLANATION:   padded with spaces   \n",
    "The photo is framed by a window. SCORE: 7 EXPLANATION: everything on one line",
    "SCORE: 6.25\nEXPLANATION: Thirds only.",
    "SCORE: 2\nEXPLANATION: A leading line crosses the frame.",
    "SCORE: 2\nEXPLANATION: Symmetrical facade.",
    "SCORE: 2\nEXPLANATION: Well balanced.",
    "SCORE: 2\nEXPLANATION: Layers of hills.",
    "SCORE: 2\nEXPLANATION: Natural frame of branches.",
    "SCORE: 2\nEXPLANATION: Generous NEGATIVE SPACE around the bird.",
    "SCORE: ten\nEXPLANATION: the score is a word",
    "I would rate this 8 out of 10.",
    "SCORE: 10.0\nEXPLANATION: Rule of thirds, leading lines, symmetry, balance, depth, framing and negative space all at once.",
    "   \n",
    "",
]


def main():
    a = VLMCompositionAnalyzer({"model": None, "processor": None})
    out = {"prompt": VLMCompositionAnalyzer.COMPOSITION_PROMPT, "max_tokens": a.max_tokens,
           "cases": [{"response": r, "result": a._parse_response(r)} for r in RESPONSES]}
    for c in out["cases"]:
        print(repr(c["response"][:50]), c["result"]["composition_score"], sorted(c["result"]["elements"]))
    path = os.path.join(HERE, "vlm_composition_host_golden.json")
    json.dump(out, open(path, "w"), indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
