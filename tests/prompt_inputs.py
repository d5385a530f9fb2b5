"""TEST INFRASTRUCTURE — what the prompt-syntax tests share: the deterministic toy tokenizer, the recorded prompts and settings, the
golden's key scheme, and (where the reference checkout is present) the reference's own `tokenize_line` driven on the same tokenizer."""
import re
import types
import zlib

COMMA_ID, START_ID, END_ID = 450, 498, 499          # outside the toy word ids 1 .. 400; inside the tiny tower's vocabulary of 500


class ToyTokenizer:
    """Words and punctuation marks -> crc32 % 400 + 1, a comma -> COMMA_ID.  No BPE: one id per word."""
    encoder = {",</w>": COMMA_ID, "<start_of_text>": START_ID, "<end_of_text>": END_ID}

    def encode(self, text):
        return [COMMA_ID if w == "," else zlib.crc32(w.encode()) % 400 + 1 for w in re.findall(r"\w+|[^\w\s]", text)]


def _words(n, first=0):
    return " ".join(f"w{i}" for i in range(first, first + n))


TABLE_LAST = "a (((house:1.3)) [on] a (hill:0.5), sun, (((sky)))."
EMBEDDER_PROMPT = "a (cat:1.4) on [grass], BREAK (night)"
PROMPTS = [
    "",
    _words(75),                                              # exactly one full chunk
    _words(76),                                              # one token over
    _words(70) + " , " + _words(12, 70),                     # 83 tokens, the comma 5 tokens before the chunk fills: inside a window of 20
    _words(40) + " , " + _words(42, 40),                     # the comma 35 tokens back: outside the window
    "a castle BREAK on a (hill:1.2)",
    "BREAK first word",
    r"((nested) [deep [er]]) \(escaped\) \[too\] \\ (open",
    TABLE_LAST,
    EMBEDDER_PROMPT,
    "(" + _words(60) + ":1.3) , [" + _words(30, 60) + "]",    # weights carried across a back-tracked chunk boundary
]
SETTINGS = [(e, b) for e in (False, True) for b in (0, 20)]


def key(idx, emphasis, backtrack):
    return f"p{idx}_e{int(emphasis)}_b{backtrack}"


def reference_embedder():
    """The reference's FrozenOpenCLIPEmbedder without its constructor (which needs open_clip), on the toy tokenizer, with this
    package's `parse_prompt_attention` in the stubbed `modules.prompt_parser`.  -> (embedder, its module: set module.opts.* per case)."""
    import sys

    from oracle import ref_bootstrap as rb
    from sd_webui_text2video_amd import text_encoder as TE
    rb.bootstrap_pipeline()
    ch = sys.modules["modelscope.clip_hardcode"]
    ch.tokenizer = ToyTokenizer()
    ch.prompt_parser.parse_prompt_attention = TE.parse_prompt_attention
    emb = ch.FrozenOpenCLIPEmbedder.__new__(ch.FrozenOpenCLIPEmbedder)
    emb.id_start, emb.id_end, emb.comma_token, emb.chunk_length = START_ID, END_ID, COMMA_ID, 75
    emb.hijack = types.SimpleNamespace(embedding_db=types.SimpleNamespace(find_embedding_at_position=lambda tokens, position: (None, None)))
    return emb, ch


def reference_chunks(emb, ch, prompt, emphasis, backtrack):
    ch.opts.enable_emphasis, ch.opts.comma_padding_backtrack = emphasis, backtrack
    chunks, count = emb.tokenize_line(prompt)
    return [(list(c.tokens), list(c.multipliers)) for c in chunks], count


# ---- designed inputs of the GPU tests (and of the CPU proofs of what they expose) -----------------------------------------------------
EMPHASIS_GATE = 4 * 2.0 ** -24           # per element, relative: three fp32 roundings (z * m, the ratio, the product) and a margin
EMPHASIS_SHAPES = [(1, 77, 128), (3, 77, 128), (2, 77, 1024)]
UNET_GATE = 6e-3                         # a tiny forward against the oracle (test_unet_frame_count_edge_cases)


def emphasis_inputs(B, Lseq, W, seed=0):
    """z fp32 [B, L, W] (fp16-representable, so that the fp16 and fp32 forms carry the same values) whose rows have different means,
    and multipliers fp32 [B, L]: webui weights, one 0, one negative; the LAST chunk of a batch of several is an "empty chunk" (all
    ones).  Conditioning sum |z m| / |sum z m| stays far below 100: every row mean is positive and of the size of the spread."""
    import torch
    g = torch.Generator().manual_seed(1000 + seed + B * 7 + W)
    means = 0.5 + 1.5 * torch.rand(B, Lseq, 1, generator=g)
    z = (means + torch.randn(B, Lseq, W, generator=g)).half().float()
    choice = torch.tensor([1.0, 1.0, 1.0, 1.1, 1 / 1.1, 1.4, 0.55, 1.573])
    m = choice[torch.randint(0, len(choice), (B, Lseq), generator=g)]
    m[0, 5], m[0, 9] = 0.0, -0.5
    if B > 1:
        m[B - 1] = 1.0
    return z, m.float().contiguous()


def emphasis_ref64(z, m, variant="reference"):
    """The float64 formula on the same inputs.  variant: "reference" (clip_hardcode.py:413-420: the mean of the whole batch),
    "per_row" (each chunk's own mean restored), "inverted" (new mean / original mean)."""
    z, m = z.double(), m.double()
    zm = z * m[..., None]
    if variant == "per_row":
        return zm * (z.sum(dim=(1, 2), keepdim=True) / zm.sum(dim=(1, 2), keepdim=True))
    ratio = z.sum() / zm.sum()
    return zm * (1 / ratio if variant == "inverted" else ratio)


def max_rel(a, ref):
    """max over the elements of |a - ref| / |ref| (elements with ref == 0 must match exactly: they count as inf otherwise)."""
    import torch
    a, ref = a.double(), ref.double()
    d = (a - ref).abs()
    rel = torch.where(ref != 0, d / ref.abs().clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    return float(rel.max())


CTX_SCALE = 1.0        # unit-variance context: WHICH keys a role attends to already moves its eps 25x the gate (test_prompt_syntax_cpu)


def ragged_inputs(cfg, V, F, H, W, Lc, Lu, seed=0):
    """x [V, 4, F, H, W], t (one timestep), c [V, Lc, ctx], uc [V, Lu, ctx] — fp32, the contexts fp16-representable."""
    import torch
    g = torch.Generator().manual_seed(77 + seed)
    x = torch.randn(V, cfg["in_dim"], F, H, W, generator=g)
    c = (CTX_SCALE * torch.randn(V, Lc, cfg["context_dim"], generator=g)).half().float()
    uc = (CTX_SCALE * torch.randn(V, Lu, cfg["context_dim"], generator=g)).half().float()
    return x, torch.tensor([601]), c, uc
