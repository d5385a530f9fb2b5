"""TEST INFRASTRUCTURE — what the tests of a batch of different prompts share (ragged text contexts: one key count and one K / V location
per sample, T2V_OP_ATTENTION's per-sample table): the length lists, the designed inputs of the attention op and of the tiny UNet, and
the float64 formula.  tests/test_prompt_batch_cpu.py proves what the inputs expose."""
import torch

# (cond lengths | uncond lengths) of 1 .. 3 videos, guided: 2 .. 6 outer samples.  Multiples of the 77-token chunk, counts that are no
# multiple of the 32-key MFMA tile on either side of it, a single key, and a pair.
LENGTH_LISTS = [((154, 77, 231), (77, 77, 154)), ((77, 154), (154, 77)), ((33, 32, 31), (1, 40, 24)), ((24,), (40,))]
HEADS, NQ, FRAMES, HEAD_DIM, GUARD = 2, 64, 2, 64, 3
INTERP_GATE = 2e-3           # kernel against the interpreter's reading of the record (the existing two-role test's gate)
EXPOSED = 25 * INTERP_GATE   # what a table read wrongly must move a sample's float64 result by, at least
BOUNDARY_GAIN = 3.0          # K of a sample's first and last row: those keys dominate the softmax of a good share of the queries
SAMPLE_SHIFT = 4.0           # V of sample s: + SAMPLE_SHIFT * (s + 1) standard deviations, alternating sign


def flat(lens):
    """(cond lengths, uncond lengths) -> the lengths in batch order [cond (V) | uncond (V)] and every sample's first packed row."""
    ls = list(lens[0]) + list(lens[1])
    return ls, [sum(ls[:b]) for b in range(len(ls))]


def attention_inputs(lens):
    """-> q fp16 [B * FRAMES * NQ, HEADS * HEAD_DIM] and the packed K | V rows fp16 [GUARD + sum + GUARD, 2 * HEADS * HEAD_DIM]: NaN guard
    rows in front of the first sample's rows and behind the last sample's; the samples' rows directly one after another.  A sample's V
    rows carry its own offset of several standard deviations, and its first and last keys are the strong ones: one key too many reads a
    neighbour's strong key with the neighbour's values, one too few drops an own strong key, whose values no other key of the sample has."""
    ls, starts = flat(lens)
    inner = HEADS * HEAD_DIM
    g = torch.Generator().manual_seed(sum((k + 1) * n for k, n in enumerate(ls)))
    q = torch.randn(len(ls) * FRAMES * NQ, inner, generator=g).half()
    kv = torch.empty(GUARD + sum(ls) + GUARD, 2 * inner)
    kv[:GUARD] = float("nan")
    kv[-GUARD:] = float("nan")
    for s, (n, r) in enumerate(zip(ls, starts)):
        rows = kv[GUARD + r: GUARD + r + n]
        rows[:, :inner] = 1.5 * torch.randn(n, inner, generator=g)
        rows[0, :inner] *= BOUNDARY_GAIN
        rows[-1, :inner] *= BOUNDARY_GAIN
        rows[:, inner:] = torch.randn(n, inner, generator=g) + SAMPLE_SHIFT * (s + 1) * (-1) ** s
        rows[0, inner:] *= -2.0                       # what the strong keys carry is far from the sample's other values (and from a neighbour's)
        if n > 1:
            rows[-1, inner:] *= -2.0
    return q, kv.half()


def attention_ref64(q, kv, table):
    """softmax(q k^T / sqrt(D)) v in float64 for a table [(key count, first row relative to the row behind the guard), ...], one entry
    per outer sample: -> [B * FRAMES * NQ, HEADS * HEAD_DIM].  K / V do not depend on the frame (a text context)."""
    inner = HEADS * HEAD_DIM
    out = torch.empty(q.shape, dtype=torch.float64)
    for s, (n, first) in enumerate(table):
        rows = kv[GUARD + first: GUARD + first + n].double()
        k, v = rows[:, :inner].view(n, HEADS, HEAD_DIM), rows[:, inner:].view(n, HEADS, HEAD_DIM)
        qs = q[s * FRAMES * NQ:(s + 1) * FRAMES * NQ].double().view(-1, HEADS, HEAD_DIM)
        p = torch.softmax(torch.einsum("qhd,khd->hqk", qs, k) * HEAD_DIM ** -0.5, dim=-1)
        out[s * FRAMES * NQ:(s + 1) * FRAMES * NQ] = torch.einsum("hqk,khd->qhd", p, v).reshape(-1, inner)
    return out


# ---- the tiny UNet ------------------------------------------------------------------------------------------------------------------
UNET_CASES = [((2, 8, 8), LENGTH_LISTS[0]), ((3, 16, 16), LENGTH_LISTS[2])]       # V = 3: (geometry, lengths)


def unet_inputs(cfg, geom, lens, seed=0):
    """x [V, 4, F, H, W], t (one timestep), conds / unconds: lists of V contexts [1, L_v, ctx] — fp32, fp16-representable; every
    context has its own mean (one standard deviation per channel, random signs), so a neighbour's row is not one of its own."""
    V = len(lens[0])
    g = torch.Generator().manual_seed(4177 + seed + sum(lens[0]) + 3 * sum(lens[1]))
    x = torch.randn(V, cfg["in_dim"], *geom, generator=g)

    def ctx(n):
        mean = torch.randint(0, 2, (1, 1, cfg["context_dim"]), generator=g).float() * 2 - 1
        return (mean + torch.randn(1, n, cfg["context_dim"], generator=g)).half().float()

    return x, torch.tensor([601]), [ctx(n) for n in lens[0]], [ctx(n) for n in lens[1]]
