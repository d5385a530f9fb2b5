"""Generate tests/golden/prompt_syntax.npz FROM THE REAL REFERENCE: what `FrozenOpenCLIPEmbedder.tokenize_line`
(scripts/modelscope/clip_hardcode.py:146-239) returns for the prompts and settings of tests/prompt_inputs.py on the toy tokenizer —
per prompt and (enable_emphasis, comma_padding_backtrack): the chunks' token ids [chunks, 77], their multipliers [chunks, 77] and
the token count.  Data only; the prompts are stored beside them.

    python tests/golden/make_golden_prompt.py
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prompt_inputs as PI  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prompt_syntax.npz")


def main():
    emb, ch = PI.reference_embedder()
    rec = {"prompts": np.array(PI.PROMPTS)}
    for idx, prompt in enumerate(PI.PROMPTS):
        for emphasis, backtrack in PI.SETTINGS:
            chunks, count = PI.reference_chunks(emb, ch, prompt, emphasis, backtrack)
            k = PI.key(idx, emphasis, backtrack)
            rec[k + "_tokens"] = np.array([t for t, _ in chunks], dtype=np.int32)
            rec[k + "_mult"] = np.array([m for _, m in chunks], dtype=np.float64)
            rec[k + "_count"] = np.array(count, dtype=np.int64)
            assert rec[k + "_tokens"].shape == rec[k + "_mult"].shape == (len(chunks), 77)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {len(PI.PROMPTS)} prompts x {len(PI.SETTINGS)} settings, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
