"""TEST INFRASTRUCTURE — adversarial inputs for the three attention paths whose softmax lives inside a kernel that does something else as
well: T2V_EPI_TATTN (gemm2.hip tile 10: QKV projection + temporal self-attention), T2V_EPI_XATTN (t2v_epilogue_xattn: to_q projection +
text cross-attention; gemm2 tiles 8, 11, 5 and gemm.hip tile 0) and the second role of T2V_OP_ATTENTION (i[19..21], p[4..5]).  No test
functions here: tests/test_fused_attention_inputs_cpu.py proves on the CPU what the inputs do (and runs every program through the
interpreter), tests/test_gpu_fused_attention_adversarial.py runs the same programs on the GPU.  Both import CASES / build(), so they cannot
drift apart.  Nothing here touches a GPU or imports tests/interp.py; every expected value is `adversarial.softmax_attention_ref` (float64,
explicit formula) on the q, k, v written out below.

Placing logits through a GEMM.  The projections use SELECTION WEIGHTS: every weight row holds one power of two (1/2, 1 or 2 by head) at a
chosen input column and zeros elsewhere, so the fp32-accumulated projection of the fp16 operand is exact and q, k, v are chosen fp16
values.  TATTN: K = 192 heads, head h's q | k | v are columns 192 h .. 192 h + 191 of A, the weight is packed by packing.qkv_head_major.
XATTN: K = N and the selected column is a permutation of the output column.  Two dense TATTN cases (randn / sqrt(K), K = 320, 5 heads) run
the tile-10 main loop on a real reduction; there q, k, v = fp16 of the float64 product.

The inputs.  adversarial.late_max_qkv's construction (0.35 randn background, queries + 4 u, one key 9.5 log2 units up per query parity)
with the direction pair (u0, u1) taken PER SEGMENT from the 64 orthonormal rows of a Hadamard basis (entries +- 1/8: exact in fp16):
neighbouring pixels, strips, samples and heads look along different directions, the peaked key varies with the segment, and v carries a
power-of-two scale 1/8 .. 8 from a cycle of 7 that differs between neighbours (TATTN: per (sample, pixel, head); XATTN, where the strips of
a sample share its keys: per (sample, head, key), and the strips peak on different keys).  Every query also has a runner-up key 3 log2
units below its peak (TATTN: the other parity's peak; XATTN: the last key, so the last key carries visible mass for every strip): a
wrong scale or a miscounted key moves mass between keys whose v differ.  The query noise is orthogonal to the directions its segment is
planted along, so a planted logit is seen at its height.  A logit 40 log2 units up stands where the kernel must not
see it: TATTN — in the NEXT pixel's keys of the tile (the masked key slots F .. 31 of a pixel are the next pixel's rows of the LDS image)
along THIS pixel's directions, on the successor's frame 0 for even pixels and on a deeper frame for odd ones (the successor looks along
its own directions and its query noise is orthogonal to these: it sees that key at its background height); XATTN and the two-role
`masked` cases — on the key row that follows a sample's last key in memory (the next sample's / the second role's key 0, which its owner
sees legitimately, and spare rows behind the last sample).  The two-role cases use adversarial.late_max_qkv / masked_spike as they are
(one seed = one direction pair for both roles), with the keys of a sample rotated so that a window taken with the other role's key count
or stride holds a neighbouring sample's peak: 154 keys — the peaks in the third tile; one-tile second roles — the even-query peak of the
samples after the first on key 0.

Segments.  Errors are one rel-L2 per segment, asserted on the worst one: TATTN (sample, pixel, head) = F x 64 values; XATTN (32-row strip,
head) = one wave item of the epilogue; two roles (outer sample, inner, head).

Fencing.  Every tensor an op reads or writes is a window of a larger NaN allocation: PAD_ROWS rows in front and behind, lda = K + 8,
ldc = cols + 8; the XATTN K is a column window (offset 64) of a wider buffer whose other columns hold another site's finite values.  XATTN
V^T (its leading dimension i[26] is the ABI's): columns i[25] .. i[26] - 1 hold +- 32768, the 64 rows of "another site" in front of and
behind every sample's rows are NaN — so NaN follows the last sample's last row directly.  Outputs start as NaN; `verify` wants every output
finite and every fence element still NaN."""
from __future__ import annotations

import torch

import adversarial as A
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd.program import Buf, Program, Ref

TOL = A.TOL_HI            # 2e-3 on the worst segment: the suite's figure for these kernels' fp16 output against an explicit reference
EMU_BOUND = 5e-4          # the float64 emulation of the kernels' arithmetic against the formula, every segment (a quarter of TOL)
NAN = float("nan")
F16 = torch.float16
PAD_ROWS, PAD_COLS = 3, 8
NOISE, RISE, LAST_RISE = 0.35, 9.5, 6.5
VT_FENCE = 32768.0
K_COL0 = 64               # the XATTN K window starts at this column of the wider buffer
VT_SITE_ROWS = 64         # rows of "another site" in front of and behind every sample's V^T rows
XA_BM = {8: 192, 11: 128, 5: 128, 0: 128}
XA_BN = {8: 320, 11: 320, 5: 128, 0: 128}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def hadamard64():
    """64 orthonormal rows with entries +- 1/8."""
    h = torch.ones(1, 1, dtype=torch.float64)
    for _ in range(6):
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h / 8.0


H64 = hadamard64()


def seg_scale(*idx):
    """Power-of-two scale 1/8 .. 8 from a cycle of 7 (as elementwise_inputs.seg_scale): neighbours along any index differ."""
    e = sum((k + 1) * i for k, i in enumerate(idx))
    return torch.exp2(((torch.as_tensor(e) % 7) - 3).double())


def _unit(scale):
    """Length along a query direction that raises a logit by one log2 unit."""
    return 1.0 / (scale * A.LOG2E * A.AMP)


def _exact16(t):
    """fp16-representable and safe to halve or double: magnitudes below 2^-10 are flushed to zero."""
    t = t.half().double()
    t[t.abs() < 2.0 ** -10] = 0.0
    assert float(t.abs().max()) < 2.0 ** 14
    return t


def head_weight(h):
    return 2.0 ** ((h % 3) - 1)


def seg_errors(got, ref):
    """[nseg, L] x 2 -> one rel-L2 per segment; a non-finite value makes its segment's error infinite."""
    got, ref = got.double(), ref.double()
    n = ref.norm(dim=1)
    assert bool((n > 0).all()), "a segment with a zero reference"
    e = (got - ref).norm(dim=1) / n
    return torch.where(torch.isfinite(got).all(dim=1), e, torch.full_like(e, float("inf")))


class Built:
    """A case's program, weights, initial arena contents, fences and expectations."""

    def __init__(self, case):
        self.case = case
        self.P = Program()
        self.w = {}
        self.sets = []          # (allocation, its initial image: float64, NaN = fence or an output still to be written)
        self.path = ""
        self.x = {}             # the raw inputs and memory images (tests/test_fused_attention_inputs_cpu.py emulates the kernels on them)
        self.ref = None         # [nseg, L] float64
        self.out_big = None     # the allocation that holds the output, and its window (first row, end row, columns)
        self.out_win = None
        self.exact_rows = None  # bool [rows, heads]: one visible key >= 30 log2 units above the rest
        self.exact_val = None   # [rows, cols] the value such a row must have, bit for bit
        self.interp = "Interp"

    def alloc_filled(self, image, dtype="f16"):
        """An allocation holding `image` (2-D float64, NaN = fence)."""
        big = self.P.alloc(image.shape[0], image.shape[1], dtype)
        fin = image[torch.isfinite(image)]
        assert torch.equal(fin.half().double(), fin), "inputs must be representable in fp16"
        self.sets.append((big, image))
        return big

    def fenced(self, rows, cols, pad_cols=PAD_COLS):
        """-> (the all-NaN image of a fenced allocation, (first row, end row, columns) of its window)."""
        image = torch.full((rows + 2 * PAD_ROWS, cols + pad_cols), NAN, dtype=torch.float64)
        return image, (PAD_ROWS, PAD_ROWS + rows, cols)

    def window(self, big, r0, r1, c0, c1):
        return big.row_slice(r0, r1).col_slice(c0, c1)

    def init(self, it):
        for big, image in self.sets:
            it.mat(big.ref, big.rows, big.ld, big.ld, F16, {}).copy_(image.half())

    def to_seg(self, out2d):
        raise NotImplementedError


def _rd(it, big):
    return it.mat(big.ref, big.rows, big.ld, big.ld, F16, {}).clone()


def verify(it, b):
    """Fences, finiteness, per-segment errors and the bit-exact rows of a finished run -> dict(worst, mean, exact)."""
    tag = b.case["id"]
    outputs = (b.out_big, getattr(b, "single_big", None))
    for big, image in b.sets:
        got = _rd(it, big)
        keep = ~torch.isnan(image)
        if any(big is o for o in outputs):
            r0, r1, c1 = b.out_win
            keep[r0:r1, :c1] = True
            assert torch.isfinite(got[r0:r1, :c1]).all(), f"{tag}: non-finite values in the output"
        else:
            assert torch.equal(got[keep].double(), image[keep]), f"{tag}: an input was overwritten"
        assert torch.isnan(got[~keep]).all(), f"{tag}: {int((~torch.isnan(got[~keep])).sum())} fence elements written"
    r0, r1, c1 = b.out_win
    out = _rd(it, b.out_big)[r0:r1, :c1]
    e = seg_errors(b.to_seg(out), b.ref)
    k = int(torch.argmax(e))
    figs = dict(worst=float(e.max()), seg=k, mean=float(e.mean()), exact=0, whole=A.rel_l2(b.to_seg(out), b.ref))
    if b.exact_rows is not None and bool(b.exact_rows.any()):
        heads = b.exact_rows.shape[1]
        g = out.reshape(out.shape[0], heads, -1)[b.exact_rows]
        want = b.exact_val.half().reshape(out.shape[0], heads, -1)[b.exact_rows]
        figs["exact"] = int(b.exact_rows.sum())
        assert torch.equal(g, want), f"{tag}: a row with one key >= 30 log2 units above the rest is not that key's v bit for bit"
    assert figs["worst"] < TOL, (tag, "worst segment %.3e (segment %d), mean %.3e" % (figs["worst"], k, figs["mean"]))
    return figs


def figures_line(b, figs):
    return (f"ADV {b.case['id']}: {b.path}; worst segment {figs['worst']:.2e} (segment {figs['seg']} of {b.ref.shape[0]}), mean {figs['mean']:.2e}, "
            f"whole tensor {figs['whole']:.2e}, bit-exact rows {figs['exact']}")


def _dominant(lg2, v):
    """lg2 [items, nq, nk] (log2 units, -inf masked), v [items, nk, D] -> (rows [items, nq] where one key stands >= 30 above the rest, its v)."""
    top = lg2.topk(min(2, lg2.shape[-1]), dim=-1)
    if lg2.shape[-1] == 1:
        rows = torch.ones(lg2.shape[:2], dtype=torch.bool)
    else:
        rows = (top.values[..., 0] - top.values[..., 1]) >= 30.0
    val = torch.gather(v, 1, top.indices[..., 0:1].expand(-1, -1, v.shape[-1]))
    return rows, val


# ---- T2V_EPI_TATTN ----------------------------------------------------------------------------------------------------------------------------
def tattn_pair(s, pix, h):
    return (pix + 5 * s + 11 * h) % 32


def tattn_peaks(s, pix, h, F):
    s0 = (3 * pix + s + h) % F
    s1 = (s0 + 1 + pix % max(F - 1, 1)) % F
    return s0, (s1 if s1 != s0 else (s0 + 1) % F)


def tattn_spike_frame(pix, F, HW, tpix):
    """Frame j of pixel pix + 1 whose key carries pixel pix's masked spike (slot F + j of pixel pix), or -1: no successor in the tile / no
    masked slot.  Even pixels: the first masked slot; odd pixels: a deeper one where there is one."""
    if (pix + 1) % tpix == 0 or pix + 1 >= HW or F >= 32:
        return -1
    deep = min(F - 1, 31 - F)
    return 0 if pix % 2 == 0 else min(1 + (pix // 2) % 3, deep)


def tattn_qkv(c):
    """q, k, v [S, F, HW, heads, 64] float64 (fp16 values) of a placed case."""
    S, F, HW, heads = c["S"], c["F"], c["HW"], c["heads"]
    tpix = min(12, 192 // F)
    scale = 64 ** -0.5
    u = _unit(scale)
    g = _gen(c["seed"])
    q = NOISE * torch.randn(S, F, HW, heads, 64, generator=g, dtype=torch.float64)
    k = NOISE * torch.randn(S, F, HW, heads, 64, generator=g, dtype=torch.float64)
    v = torch.randn(S, F, HW, heads, 64, generator=g, dtype=torch.float64)
    par = torch.arange(F) % 2
    for s in range(S):
        for pix in range(HW):
            for h in range(heads):
                d = H64[2 * tattn_pair(s, pix, h): 2 * tattn_pair(s, pix, h) + 2]
                # the noise is orthogonal to the pixel's own pair (a logit planted along it is seen at its height) and to the previous pixel's
                # (whose masked spike this pixel's keys carry: this pixel sees that key at its background height)
                dd = torch.cat([d, H64[2 * tattn_pair(s, pix - 1, h): 2 * tattn_pair(s, pix - 1, h) + 2]])
                q[s, :, pix, h] -= (q[s, :, pix, h] @ dd.t()) @ dd
                q[s, :, pix, h] += A.AMP * d[par]
                s0, s1 = tattn_peaks(s, pix, h, F)
                k[s, s0, pix, h] += RISE * u * d[0] + LAST_RISE * u * d[1]      # every query: a peak and a runner-up 3 log2 units below it
                k[s, s1, pix, h] += RISE * u * d[1] + LAST_RISE * u * d[0]
                v[s, :, pix, h] *= seg_scale(s, pix, h)
                j = tattn_spike_frame(pix, F, HW, tpix)
                if j >= 0:
                    k[s, j, pix + 1, h] += A.MASKED_RISE * u * (d[0] + d[1])
    return _exact16(q), _exact16(k), _exact16(v)


class _Tattn(Built):
    def to_seg(self, out2d):
        S, F, HW, heads = (self.case[n] for n in ("S", "F", "HW", "heads"))
        return out2d.double().reshape(S, F, HW, heads, 64).permute(0, 2, 3, 1, 4).reshape(S * HW * heads, F * 64)


def _build_tattn(c):
    b = _Tattn(c)
    S, F, HW, heads = c["S"], c["F"], c["HW"], c["heads"]
    T, C, tpix, scale = S * F * HW, heads * 64, min(12, 192 // F), 64 ** -0.5
    if c["dense"]:
        K = 320
        g = _gen(c["seed"])
        a2d = (1.5 * torch.randn(T, K, generator=g, dtype=torch.float64)).half().double()
        wq, wk, wv = ((torch.randn(C, K, generator=g, dtype=torch.float64) / K ** 0.5) for _ in range(3))
        wv = wv * seg_scale(torch.arange(heads)).repeat_interleave(64)[:, None]
        wq, wk, wv = wq.half().double(), wk.half().double(), wv.half().double()
        q, k, v = ((a2d @ w.t()).half().double().view(S, F, HW, heads, 64) for w in (wq, wk, wv))
        b.x.update(a2d=a2d, wq=wq, wk=wk, wv=wv)
    else:
        K = 192 * heads
        q, k, v = tattn_qkv(c)
        hw_ = torch.tensor([head_weight(h) for h in range(heads)], dtype=torch.float64)
        a2d = (torch.stack([q, k, v], dim=4) / hw_[None, None, None, :, None, None]).reshape(T, K)
        eye = torch.eye(C, dtype=torch.float64) * hw_.repeat_interleave(64)[:, None]
        wq, wk, wv = (torch.zeros(C, K, dtype=torch.float64) for _ in range(3))
        for part, w in enumerate((wq, wk, wv)):
            w.view(C, heads, 3, 64)[:, :, part, :] = eye.view(C, heads, 64)
    b.w["wh"] = pk.qkv_head_major(wq, wk, wv).half()
    assert torch.equal(b.w["wh"].double(), pk.qkv_head_major(wq, wk, wv))
    a_img, (r0, r1, _) = b.fenced(T, K)
    a_img[r0:r1, :K] = a2d
    o_img, b.out_win = b.fenced(T, C)
    abig, b.out_big = b.alloc_filled(a_img), b.alloc_filled(o_img)
    a, out = b.window(abig, r0, r1, 0, K), b.window(b.out_big, r0, r1, 0, C)
    op = b.P.qkv_temporal_attention("tattn", a, Ref("weight", 0, "wh"), out, samples=S, frames=F, hw=HW, heads=heads, k=K, scale=scale)
    tiles_ps = -(-HW // tpix)
    assert op.i[22] == 10 and op.i[16] == L.EPI_TATTN and op.i[10] == tpix == c["tpix"] and op.i[8] == F and op.i[9] == HW
    assert op.i[0] == S * tiles_ps * 192 and op.i[1] == 192 * heads and op.i[2] == K and op.i[3] == K + PAD_COLS and op.i[5] == C + PAD_COLS
    b.path = f"tattn tile 10, tpix {tpix}, {tiles_ps} tiles per sample, {tpix * F} of 192 rows live, K {K}"
    items = lambda t: t.permute(0, 2, 3, 1, 4).reshape(S * HW * heads, F, 64)
    qi, ki, vi = items(q), items(k), items(v)
    b.x.update(q=q, k=k, v=v, scale=scale, tpix=tpix, K=K)
    ref = A.softmax_attention_ref(qi, ki, vi, scale)
    b.ref = ref.reshape(S * HW * heads, F * 64)
    rows, val = _dominant(A.logits(qi, ki, scale) * A.LOG2E, vi)
    back = lambda t, last: t.reshape(S, HW, heads, F, *last).permute(0, 3, 1, 2, *range(4, 4 + len(last)))
    b.exact_rows = back(rows, ()).reshape(T, heads)
    b.exact_val = back(val, (64,)).reshape(T, C)
    return b


# ---- T2V_EPI_XATTN ----------------------------------------------------------------------------------------------------------------------------
def xattn_pair(st, b, h):
    return (st % 3) + 3 * ((b + 2 * h) % 5)


def xattn_peaks(st, b, h, Lc):
    s0 = (11 * (st % 3) + 7 * b + 3 * h + 1) % Lc
    s1 = (s0 + 1 + (st % 3 + h) % 5) % Lc
    return s0, s1


def xattn_dirs(b, h):
    """The six directions the strips of (sample, head) look along, [6, 64]."""
    return torch.cat([H64[2 * xattn_pair(st, b, h): 2 * xattn_pair(st, b, h) + 2] for st in range(3)])


def xattn_qkv(c):
    """q [B, rows, heads, 64], k, v [B, Lc, heads, 64], spare [heads, 64] (the key of the spare rows behind the last sample)."""
    B, rows, Lc, heads, wrap = c["B"], c["rows"], c["Lc"], c["N"] // 64, c["wrap"]
    scale = 64 ** -0.5
    u = _unit(scale)
    g = _gen(c["seed"])
    q = NOISE * torch.randn(B, rows, heads, 64, generator=g, dtype=torch.float64)
    k = NOISE * torch.randn(B, Lc, heads, 64, generator=g, dtype=torch.float64)
    v = torch.randn(B, Lc, heads, 64, generator=g, dtype=torch.float64)
    spare = NOISE * torch.randn(heads, 64, generator=g, dtype=torch.float64)
    par = torch.arange(32) % 2
    bq = lambda bb: 0 if wrap else bb                      # a_wrap: the operand rows of sample 0 serve every sample
    for bb in range(B):
        for h in range(heads):
            d6 = xattn_dirs(bq(bb), h)
            # the noise is orthogonal to the six directions of (sample, head) and of the previous sample, whose masked spike key 0 carries
            dd = d6 if (wrap or bb == 0) else torch.cat([d6, xattn_dirs(bb - 1, h)])
            q[bb, :, h] -= (q[bb, :, h] @ dd.t()) @ dd
            for st in range(rows // 32):
                d = H64[2 * xattn_pair(st, bq(bb), h): 2 * xattn_pair(st, bq(bb), h) + 2]
                q[bb, st * 32:(st + 1) * 32, h] += A.AMP * d[par]
            for st in range(min(3, rows // 32)):
                d = H64[2 * xattn_pair(st, bq(bb), h): 2 * xattn_pair(st, bq(bb), h) + 2]
                s0, s1 = xattn_peaks(st, bb, h, Lc)
                k[bb, s0, h] += RISE * u * d[0]
                k[bb, s1, h] += RISE * u * d[1]
            if Lc > 1:
                k[bb, Lc - 1, h] += LAST_RISE * u * xattn_dirs(bq(bb), h).sum(0)        # the last key carries visible mass for every strip
            v[bb, :, h] *= seg_scale(bb, 2 * h, 3 * torch.arange(Lc))[:, None]
            big = A.MASKED_RISE * u * xattn_dirs(bq(bb), h).sum(0)                      # behind sample bb's last key
            if bb + 1 < B:
                k[bb + 1, 0, h] += big
            else:
                spare[h] += big
    if wrap:
        q[1:] = q[0]
    return _exact16(q), _exact16(k), _exact16(v), _exact16(spare)


class _Xattn(Built):
    def to_seg(self, out2d):
        M, heads = out2d.shape[0], self.case["N"] // 64
        return out2d.double().reshape(M // 32, 32, heads, 64).permute(0, 2, 1, 3).reshape(M // 32 * heads, 32 * 64)


def _build_xattn(c):
    b = _Xattn(c)
    tile, N, K, B, rows, Lc, wrap = (c[n] for n in ("tile", "N", "K", "B", "rows", "Lc", "wrap"))
    heads, M, lcp, scale = N // 64, B * rows, -(-Lc // 32) * 32, 64 ** -0.5
    assert K == N and rows % 32 == 0
    q, k, v, spare = xattn_qkv(c)
    # A and the selection weight: output column n reads input column perm[n], times the head's power of two
    perm = (7 * torch.arange(N) + 3) % K
    assert len(set(perm.tolist())) == N
    hw_ = torch.tensor([head_weight(h) for h in range(heads)], dtype=torch.float64).repeat_interleave(64)
    a_rows = rows if wrap else M
    a2d = torch.zeros(a_rows, K, dtype=torch.float64)
    a2d[:, perm] = (q.reshape(M, N) / hw_)[:a_rows]
    W = torch.zeros(N, K, dtype=torch.float64)
    W[torch.arange(N), perm] = hw_
    b.w["w"] = W.half()
    a_img, (r0, r1, _) = b.fenced(a_rows, K)
    a_img[r0:r1, :K] = a2d
    # K: rows [fence | B Lc keys | spare rows with the spike | fence] x columns [another site (64) | this site's N | 8]
    n_spare = 96 - Lc
    wide = K_COL0 + N + PAD_COLS
    k_img = torch.full((PAD_ROWS + B * Lc + n_spare + PAD_ROWS, wide), NAN, dtype=torch.float64)
    live = slice(PAD_ROWS, PAD_ROWS + B * Lc + n_spare)
    k_img[live, :K_COL0] = (4.0 * torch.randn(B * Lc + n_spare, K_COL0, generator=_gen(c["seed"] + 1), dtype=torch.float64)).half().double()
    k_img[PAD_ROWS:PAD_ROWS + B * Lc, K_COL0:K_COL0 + N] = k.reshape(B * Lc, N)
    k_img[PAD_ROWS + B * Lc:PAD_ROWS + B * Lc + n_spare, K_COL0:K_COL0 + N] = spare.reshape(1, N)
    # V^T: per sample [64 rows of another site: NaN | N rows: v^T in columns < Lc, +- 32768 up to lcp | 64 rows of another site: NaN]
    per = N + 2 * VT_SITE_ROWS
    vt_img = torch.full((B * per, lcp), NAN, dtype=torch.float64)
    for bb in range(B):
        blk = vt_img[bb * per + VT_SITE_ROWS: bb * per + VT_SITE_ROWS + N]
        blk[:, :Lc] = v[bb].reshape(Lc, N).t()
        blk[:, Lc:] = VT_FENCE * (1.0 - 2.0 * ((torch.arange(N)[:, None] + torch.arange(Lc, lcp)[None, :]) % 2).double())
    o_img, b.out_win = b.fenced(M, N)
    abig, kbig, vbig = b.alloc_filled(a_img), b.alloc_filled(k_img), b.alloc_filled(vt_img)
    b.out_big = b.alloc_filled(o_img)
    a = b.window(abig, r0, r1, 0, K)
    out = b.window(b.out_big, PAD_ROWS, PAD_ROWS + M, 0, N)
    kbuf = b.window(kbig, PAD_ROWS, PAD_ROWS + B * Lc, K_COL0, K_COL0 + N)
    vt_site = Buf(vbig.row_slice(VT_SITE_ROWS, vbig.rows).ref, vbig.rows, lcp, lcp, "f16", owns=False)
    b.P.force_tile = tile
    op = b.P.to_q_cross_attention("xattn", a, Ref("weight", 0, "w"), out, k=K, heads=heads, kbuf=kbuf, vt=vt_site, n_keys=Lc, rows_per_sample=rows,
                                  samples=B, scale=scale, a_wrap=rows if wrap else 0)
    assert op is not None and op.meta["tile"] == tile and op.i[22] == tile and op.i[16] == L.EPI_XATTN
    assert (op.i[0], op.i[1], op.i[2], op.i[13], op.i[15]) == (M, N, K, rows if wrap else 0, rows)
    assert (op.i[24], op.i[25], op.i[26], op.i[27], op.i[28]) == (wide, Lc, lcp, Lc * wide, per * lcp)
    b.path = f"xattn tile {tile} ({XA_BM[tile]}x{XA_BN[tile]}), {Lc} keys in {lcp} columns, {-(-M // XA_BM[tile])} x {-(-N // XA_BN[tile])} tiles"
    b.x.update(q=q, k=k, v=v, scale=scale, k_img=k_img, vt_img=vt_img, k_row0=PAD_ROWS, vt_row0=VT_SITE_ROWS, vt_per=per, lcp=lcp, wide=wide)
    items = lambda t: t.permute(0, 2, 1, 3).reshape(B * heads, t.shape[1], 64)
    qi, ki, vi = items(q), items(k), items(v)
    ref = A.softmax_attention_ref(qi, ki, vi, scale)                                   # [B heads, rows, 64]
    rows2d = lambda t: t.reshape(B, heads, rows, -1).permute(0, 2, 1, 3)
    b.ref = b.to_seg(rows2d(ref).reshape(M, N))
    dom, val = _dominant(A.logits(qi, ki, scale) * A.LOG2E, vi)
    b.exact_rows = rows2d(dom).reshape(M, heads)
    b.exact_val = rows2d(val).reshape(M, N)
    return b


# ---- the second role of T2V_OP_ATTENTION -----------------------------------------------------------------------------------------------------
def attn_variant(nq, nk, nk2):
    """launch_attn's rule (csrc/attention.hip), written out: (waves, key tile)."""
    if nq <= 32:
        return (1, 32) if max(nk, nk2) <= 32 else (1, 64)
    return (4, 64)


def two_role_qkv(c):
    """Per role: q [V heads, F nq, D], k, v [V heads, nk, D] (items in (sample, head) order; the F frames of a sample share its keys), the key
    of the spare rows, and the key tile the launch uses."""
    D, nq, F, heads, V = c["D"], c["nq"], c["F"], c["heads"], c["V"]
    scale = D ** -0.5
    tile = attn_variant(nq, *c["lens"])[1]
    items = V * heads
    roles = []
    for r, nk in enumerate(c["lens"]):
        kw = dict(placement="second", shift=r)
        if c["variant"] == "masked":
            # the second role's first sample owns the key row that follows the first role's last key: it carries the spike
            spiked = list(range(heads)) if r == 1 else []
            q, k, v, spare, keys = A.masked_spike(items, F * nq, nk, D, tile, scale, c["seed"], "after", spiked, **kw)
        else:
            q, k, v = A.late_max_qkv(items, F * nq, nk, D, tile, scale, c["seed"], **kw)
            spare = None
        if r == 1:
            q = q.roll(2, dims=1)            # (same seed = same directions u0, u1 in both roles; the rows of role 2 are not those of role 1)
        if r == 1 and nk <= tile and c["variant"] != "masked":
            # one tile: the samples after the first carry their even-query peak on key 0, the row that follows the previous sample's last key
            for it in range(heads, items):
                s0 = A.spike_keys(it, nk, tile, "second", r)[0]
                k[it], v[it] = k[it].roll(-s0, dims=0), v[it].roll(-s0, dims=0)
        if nk > 2 * tile and c["variant"] != "masked":
            # three tiles: the peaks move from the second tile to the third, outside the first 77 keys (a window at the other role's stride
            # then holds the neighbouring sample's peaks and not this sample's)
            k, v = k.roll(tile, dims=1), v.roll(tile, dims=1)
        roles.append(dict(q=q, k=k, v=v, spare=spare, nk=nk))
    return roles, scale, tile


class _TwoRole(Built):
    def to_seg(self, out2d):
        c = self.case
        B, F, nq, heads, D = 2 * c["V"], c["F"], c["nq"], c["heads"], c["D"]
        return out2d.double().reshape(B, F, nq, heads, D).permute(0, 1, 3, 2, 4).reshape(B * F * heads, nq * D)


def _build_two_role(c):
    b = _TwoRole(c)
    b.interp = "PromptInterp"
    D, nq, F, heads, V = c["D"], c["nq"], c["F"], c["heads"], c["V"]
    (L1, L2), B, inner = c["lens"], 2 * V, heads * D
    roles, scale, tile = two_role_qkv(c)
    masked = c["variant"] == "masked"
    n_spare = 4 if masked else 0
    ldq, ldkv = inner + PAD_COLS, 2 * inner + PAD_COLS
    # q / out rows: (outer sample, frame, query); outer samples [0, V) are role 1, [V, 2 V) role 2
    rows_of = lambda t: t.reshape(V, heads, F, nq, D).permute(0, 2, 3, 1, 4).reshape(V * F * nq, inner)
    q_img, (r0, r1, _) = b.fenced(B * F * nq, inner)
    q_img[r0:r1, :inner] = torch.cat([rows_of(roles[0]["q"]), rows_of(roles[1]["q"])])
    kv_img = torch.full((PAD_ROWS + V * (L1 + L2) + n_spare + PAD_ROWS, ldkv), NAN, dtype=torch.float64)
    keys_of = lambda t, nk: t.reshape(V, heads, nk, D).permute(0, 2, 1, 3).reshape(V * nk, inner)
    at = PAD_ROWS
    for r in roles:
        kv_img[at:at + V * r["nk"], :inner] = keys_of(r["k"], r["nk"])
        kv_img[at:at + V * r["nk"], inner:2 * inner] = keys_of(r["v"], r["nk"])
        at += V * r["nk"]
    if masked:
        kv_img[at:at + n_spare, :inner] = roles[1]["spare"].repeat(heads)[None, :]
        kv_img[at:at + n_spare, inner:2 * inner] = 1.0
    qbig, kvbig = b.alloc_filled(q_img), b.alloc_filled(kv_img)
    outs = []
    for _ in range(2):
        o_img, b.out_win = b.fenced(B * F * nq, inner)
        outs.append(b.alloc_filled(o_img))
    b.out_big, b.single_big = outs
    qw = b.window(qbig, r0, r1, 0, inner)
    o_pair, o_single = (b.window(o, r0, r1, 0, inner) for o in outs)
    k1 = b.window(kvbig, PAD_ROWS, PAD_ROWS + V * L1, 0, inner)
    v1 = b.window(kvbig, PAD_ROWS, PAD_ROWS + V * L1, inner, 2 * inner)
    k2 = b.window(kvbig, PAD_ROWS + V * L1, PAD_ROWS + V * (L1 + L2), 0, inner)
    v2 = b.window(kvbig, PAD_ROWS + V * L1, PAD_ROWS + V * (L1 + L2), inner, 2 * inner)
    common = dict(nq=nq, heads=heads, b_inner=F, q_strides=(ldq, F * nq * ldq, nq * ldq), o_strides=(ldq, F * nq * ldq, nq * ldq), scale=scale,
                  head_dim=D)
    op = b.P.attention("pair", qw.ref, k1.ref, v1.ref, o_pair.ref, nk=L1, b_outer=B, kv_strides=(ldkv, L1 * ldkv, 0),
                       alt=(V, L2, k2.ref, v2.ref, L2 * ldkv), **common)
    half = V * F * nq
    b.P.attention("role1", qw.ref, k1.ref, v1.ref, o_single.ref, nk=L1, b_outer=V, kv_strides=(ldkv, L1 * ldkv, 0), **common)
    b.P.attention("role2", qw.row_slice(half, 2 * half).ref, k2.ref, v2.ref, o_single.row_slice(half, 2 * half).ref, nk=L2, b_outer=V,
                  kv_strides=(ldkv, L2 * ldkv, 0), **common)
    assert op.kind == L.OP_ATTENTION and op.i[19:22] == [V, L2, L2 * ldkv] and op.i[0:5] == [nq, L1, heads, B, F] and op.i[14] == D
    assert op.p[4] == k2.ref and op.p[5] == v2.ref and all(o.i[19:22] == [0, 0, 0] and o.p[4].space == "null" for o in b.P.ops[1:])
    waves, kt = attn_variant(nq, L1, L2)
    assert kt == tile
    b.path = f"attn_kernel<{waves}, {D}, {kt}> two roles ({L1}, {L2}) keys, {V} samples each"
    b.x.update(roles=roles, scale=scale, tile=tile, kv_img=kv_img, kv_row0=PAD_ROWS, variant=(waves, kt))
    refs, doms, vals = [], [], []
    for r in roles:
        ref = A.softmax_attention_ref(r["q"], r["k"], r["v"], scale)
        dom, val = _dominant(A.logits(r["q"], r["k"], scale) * A.LOG2E, r["v"])
        refs.append(rows_of(ref)), doms.append(dom.reshape(V, heads, F, nq).permute(0, 2, 3, 1).reshape(V * F * nq, heads)), vals.append(rows_of(val))
    b.ref = b.to_seg(torch.cat(refs))
    b.exact_rows, b.exact_val = torch.cat(doms), torch.cat(vals)
    return b


def verify_pair_equals_singles(it, b):
    """The pair launch and the two single-role launches of the same kernel give the same bits."""
    r0, r1, c1 = b.out_win
    pair, single = _rd(it, b.out_big)[r0:r1, :c1], _rd(it, b.single_big)[r0:r1, :c1]
    half = pair.shape[0] // 2
    assert torch.isfinite(single).all()
    assert torch.equal(pair[:half], single[:half]), (b.case["id"], "first role")
    assert torch.equal(pair[half:], single[half:]), (b.case["id"], "second role")


# ---- the case list --------------------------------------------------------------------------------------------------------------------------
def _case(family, id, **kw):
    c = dict(family=family, id=id, seed=3000 + 13 * len(CASES))
    c.update(kw)
    return c


CASES = []
for _S, _F, _HW, _h, _dense in [(2, 5, 29, 2, False), (1, 16, 25, 2, False), (2, 24, 17, 1, False), (1, 31, 13, 2, False), (1, 32, 13, 2, False),
                                (1, 17, 23, 1, False), (1, 2, 14, 3, False), (2, 12, 16, 5, True), (1, 24, 8, 5, True)]:
    CASES.append(_case("tattn", f"tattn-s{_S}-f{_F}-hw{_HW}-h{_h}" + ("-dense" if _dense else ""), S=_S, F=_F, HW=_HW, heads=_h, dense=_dense,
                       tpix=min(12, 192 // _F)))
for _t, _N, _B, _rows, _Lc, _wrap in [(8, 320, 2, 160, 77, False), (8, 320, 1, 224, 96, False), (11, 320, 2, 96, 77, True), (11, 320, 2, 160, 33, False),
                                      (5, 256, 2, 96, 65, False), (5, 128, 2, 64, 1, False), (0, 256, 2, 160, 64, False), (0, 128, 2, 96, 32, False),
                                      (0, 128, 2, 96, 7, False), (5, 128, 2, 96, 7, False)]:
    CASES.append(_case("xattn", f"xattn-t{_t}-n{_N}-b{_B}-r{_rows}-k{_Lc}" + ("-wrap" if _wrap else ""), tile=_t, N=_N, K=_N, B=_B, rows=_rows, Lc=_Lc,
                       wrap=_wrap))
for _D, _nq, _lens, _V, _var in [(64, 256, (154, 77), 1, "late"), (64, 256, (77, 154), 2, "late"), (64, 256, (154, 77), 2, "masked"),
                                 (64, 256, (77, 154), 1, "masked"), (64, 20, (24, 40), 1, "late"), (64, 20, (40, 24), 2, "late"),
                                 (64, 20, (24, 20), 2, "late"), (64, 64, (33, 32), 1, "late"), (40, 256, (77, 40), 2, "late")]:
    CASES.append(_case("two_role", f"roles-d{_D}-nq{_nq}-k{_lens[0]}+{_lens[1]}-v{_V}-{_var}", D=_D, nq=_nq, lens=_lens, V=_V, variant=_var, F=2, heads=2))
# `lowered`: the combinations the lowerings emit that no case above has (tests/record_paths.py; tests/test_record_paths_cpu.py demands them):
# the fused cross-attention on tile 0 with whole row tiles, and the two-role attention with ragged query blocks on the 4-wave and 1-wave kernels
CASES.append(_case("xattn", "lowered-xattn-t0-n128-b2-r64-k7", tile=0, N=128, K=128, B=2, rows=64, Lc=7, wrap=False))
for _nq in (64, 20):
    CASES.append(_case("two_role", f"lowered-roles-d64-nq{_nq}-k154+77-v1-late", D=64, nq=_nq, lens=(154, 77), V=1, variant="late", F=2, heads=2))
assert len({c["id"] for c in CASES}) == len(CASES)

_BUILDERS = dict(tattn=_build_tattn, xattn=_build_xattn, two_role=_build_two_role)


def build(case):
    return _BUILDERS[case["family"]](case)
