"""TEST INFRASTRUCTURE — inputs, float64 reference and programs for the fused C = 320 GEGLU feed-forward pair (csrc/gemm2.hip ff_fused_kernel,
recognised by csrc/executor.hip ff_pair).  No test functions here: tests/test_ff_fused_inputs_cpu.py proves on the CPU what the inputs
do, tests/test_gpu_ff_fused.py runs the programs on the GPU.  Both import CASES / build() / reference(), so they cannot drift apart.

The pair: hidden[M, 1280] = fp16((X W1v^T + b1v) * gelu(X W1g^T + b1g)) (N = 2560 packed value | gate rows, K = 320), then
out[M, 320] = hidden W2^T + b2 (+ fp32 residual, rows wrapped) stored as fp16 (+ the low-order image).  The fused kernel walks the hidden
dimension in 20 chunks of 64 channels; the inputs make every chunk seam weigh differently:
  X         r[m] z, r a power of two in [1/4, 4] that differs between neighbouring rows and across every multiple of 32;
  W1        value rows of chunk j scaled by v[j] (period 3), gate rows by g[j] (period 2), W2 columns of chunk j by c[j] (changes every
            6 chunks) — powers of two, no two chunks with the same triple, no chunk so small that its loss could hide — on top of a
            per-channel-quad scale: a dropped, repeated or misordered chunk and a swapped value / gate half land orders of magnitude
            outside the bound (proved on the CPU);
  biases    b1 = randn scaled like its row's weights, b2 = c[n] randn; residual = r[m] c[n] randn (fp32), optionally of M / 2 rows.
Magnitudes keep the hidden tensor far inside fp16 (|value| < 100, |gate| < 50).  All operands are rounded to their stored dtype before
the reference sees them; the reference rounds the hidden tensor to fp16, as both GPU forms do.

Bounds (the figures of tests/gemm_inputs.py, per ROW SEGMENT = one row x the 32 columns of an accumulator block):
  fp16 output (plain, and the hi image of hi + lo)   TOL_F16 = 1e-3;
  hi + lo                                             the fp32-class rule max(2e-5, 4 e_torch), e_torch = the same segment's error of torch's
                                                      fp32 CPU evaluation of the same pair — used by the CPU mutation check only: the
                                                      un-rounded hidden tensor moves every product by < 2^-11, the size of the fp16 output's
                                                      own rounding, so no fp16-output bound can see it; on the GPU that mutation is caught
                                                      by the bit-identity with the two-launch form.
Fencing as in tests/gemm_inputs.py: every tensor is a window of a larger NaN allocation, outputs start as NaN."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import gemm_inputs as G
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd.program import NULL, Buf, Ref

C, HID, CHUNK = 320, 1280, 64
NCHUNK = HID // CHUNK
TOL_F16, TOL_F32 = G.TOL_F16, G.TOL_F32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def row_scale(M):
    m = torch.arange(M)
    return torch.exp2(((3 * m + m // 32) % 5 - 2).double())


def chunk_scales():
    j = torch.arange(NCHUNK)
    v = torch.exp2((j % 3 - 1).double())                              # value rows of chunk j: 1/2, 1, 2
    g = torch.exp2((j % 2 - 1).double())                              # gate rows: 1/2, 1
    c = torch.tensor([1.0, 2.0, 0.5, 4.0], dtype=torch.float64)[j // 6]   # W2 columns: (v, g) repeats every 6 chunks, c changes there
    return v, g, c


def make_inputs(M, seed, bias1, bias2, res, res_wrap):
    """-> dict of float64 tensors, each representable in its stored dtype: X [M, 320], W1v / W1g [1280, 320] (unpacked), b1v / b1g, W2
    [320, 1280], b2, res [res_wrap or M, 320]."""
    g = _gen(seed)
    v, gs, c = chunk_scales()
    hq = torch.exp2(((torch.arange(HID) // 4) % 2).double())[:, None]            # neighbouring channel quads differ
    X = (row_scale(M)[:, None] * torch.randn(M, C, generator=g, dtype=torch.float64)).half().double()
    W1v = (torch.randn(HID, C, generator=g, dtype=torch.float64) * v.repeat_interleave(CHUNK)[:, None] * hq / math.sqrt(C) * 0.5).half().double()
    W1g = (torch.randn(HID, C, generator=g, dtype=torch.float64) * gs.repeat_interleave(CHUNK)[:, None] / math.sqrt(C)).half().double()
    cn = G.col_scale(C)
    W2 = (torch.randn(C, HID, generator=g, dtype=torch.float64) * c.repeat_interleave(CHUNK)[None, :] * cn[:, None] / math.sqrt(HID)).half().double()
    d = dict(X=X, W1v=W1v, W1g=W1g, W2=W2, b1v=None, b1g=None, b2=None, res=None, res_wrap=res_wrap)
    if bias1:
        d["b1v"] = (torch.randn(HID, generator=g) * v.repeat_interleave(CHUNK).float()).double()
        d["b1g"] = (torch.randn(HID, generator=g) * gs.repeat_interleave(CHUNK).float()).double()
    if bias2:
        d["b2"] = (cn.float() * torch.randn(C, generator=g)).double()
    if res:
        rr = res_wrap or M
        d["res"] = (row_scale(M)[:rr, None].float() * cn.float() * torch.randn(rr, C, generator=g)).double()
    return d


def reference(d, dtype=torch.float64, mutation=None):
    """The pair in `dtype` (float64: the reference; float32: torch's own fp32 result, e_torch).  mutation (CPU check): ("drop", j) chunk j
    of the hidden tensor never reaches the projection, ("repeat", j) chunk j's hidden values are used again for chunk j + 1,
    ("swap", j) value and gate of chunk j change places, ("unrounded",) the hidden tensor is not rounded to fp16."""
    t = lambda x: None if x is None else x.to(dtype)
    X, W1v, W1g, W2 = t(d["X"]), t(d["W1v"]), t(d["W1g"]), t(d["W2"])
    val, gate = X @ W1v.t(), X @ W1g.t()
    if d["b1v"] is not None:
        val, gate = val + t(d["b1v"])[None, :], gate + t(d["b1g"])[None, :]
    if mutation is not None and mutation[0] == "swap":
        s = slice(mutation[1] * CHUNK, (mutation[1] + 1) * CHUNK)
        val, gate = val.clone(), gate.clone()
        val[:, s], gate[:, s] = gate[:, s].clone(), val[:, s].clone()
    hid = val * F.gelu(gate)
    if not (mutation is not None and mutation[0] == "unrounded"):
        hid = hid.half().to(dtype)
    if mutation is not None and mutation[0] == "drop":
        hid = hid.clone()
        hid[:, mutation[1] * CHUNK:(mutation[1] + 1) * CHUNK] = 0
    if mutation is not None and mutation[0] == "repeat":
        j = mutation[1]
        hid = hid.clone()
        hid[:, (j + 1) * CHUNK:(j + 2) * CHUNK] = hid[:, j * CHUNK:(j + 1) * CHUNK]
    out = hid @ W2.t()
    if d["b2"] is not None:
        out = out + t(d["b2"])[None, :]
    if d["res"] is not None:
        R, rw, M = t(d["res"]), d["res_wrap"], X.shape[0]
        out = out + (torch.cat([R[:rw], R[:M - rw]]) if rw else R[:M])
    return hid, out


def hi_lo(out):
    """The stored images of an fp32-class result: hi = fp16(v), lo = fp16(v - hi) (v in fp32, as the epilogue has it)."""
    v = out.float()
    hi = v.half()
    return hi, (v - hi.float()).half()


def packed_w1(d):
    """The packed GEGLU weight [2560, 320] (+ bias [2560]): row 16 u + 8 g + j = source row g * 1280 + 8 u + j (value rows first)."""
    rows = G.geglu_rows(HID)
    W = torch.cat([d["W1v"], d["W1g"]])[rows]
    b = None if d["b1v"] is None else torch.cat([d["b1v"], d["b1g"]])[rows]
    return W, b


# ---- the case list ------------------------------------------------------------------------------------------------------------------------
# M: one tile, a ragged second tile, three tiles; each bias present and absent; residual present, absent, wrapped at M / 2; hi + lo and plain
CASES = [
    dict(id="M192-b1-b2-res-hilo", M=192, bias1=True, bias2=True, res=True, wrap=False, out_lo=True),
    dict(id="M192-b1-b2-nores-hilo", M=192, bias1=True, bias2=True, res=False, wrap=False, out_lo=True),
    dict(id="M200-nob1-b2-nores-f16", M=200, bias1=False, bias2=True, res=False, wrap=False, out_lo=False),
    dict(id="M200-b1-b2-wrap-f16", M=200, bias1=True, bias2=True, res=True, wrap=True, out_lo=False),
    dict(id="M576-b1-nob2-wrap-hilo", M=576, bias1=True, bias2=False, res=True, wrap=True, out_lo=True),
    dict(id="M576-nob1-nob2-res-f16", M=576, bias1=False, bias2=False, res=True, wrap=False, out_lo=False),
]
for _k, _c in enumerate(CASES):
    _c["seed"] = 4100 + _k
assert len({c["id"] for c in CASES}) == len(CASES)

_INPUTS = {}


def inputs_of(c):
    """Inputs and float64 reference of a case, computed once per process and never modified."""
    if c["id"] not in _INPUTS:
        d = make_inputs(c["M"], c["seed"], c["bias1"], c["bias2"], c["res"], c["M"] // 2 if c["wrap"] else 0)
        hid, ref = reference(d)
        _INPUTS[c["id"]] = (d, hid, ref)
    return _INPUTS[c["id"]]


class BuiltPair(G.Built):
    """Program of a case: the GEGLU GEMM (tile 2, the waiver of the row cut-off set: i[31] = 1), a MEMSET of a scratch buffer, the
    projection (tile 8), and a COPY2D that reads the hidden tensor.  `ops(kind)` picks the records a plan is made of."""

    def ops(self, kind):
        ge, ms, pr, cp = self.P.ops[self.k_geglu], self.P.ops[self.k_memset], self.P.ops[self.k_proj], self.P.ops[self.k_copy]
        return {"adjacent": [ge, pr], "separated": [ge, ms, pr], "third-reader": [ge, pr, cp]}[kind]


def build(c, *, waive_cutoff=True, split_k=False, out_over_x=False):
    """out_over_x: the projection's [M, 640] hi + lo output is the buffer X lives in, with rows twice as long (what the lowerings do with
    the dead operand of the GEGLU GEMM): safe as two launches, not as one — the recognition must leave such a pair alone."""
    d, _, _ = inputs_of(c)
    M = c["M"]
    b = BuiltPair(c)
    P = b.P
    if out_over_x:
        assert c["out_lo"]
        shared = P.alloc(M, 2 * C, "f16")                    # (no fence: X and the output are two views of it)
        x = b.put(Buf(shared.ref, M, C, C, "f16", shared.alloc_off), d["X"])
    else:
        x = b.put(b.fenced(M, C, "f16"), d["X"])
    W1p, b1p = packed_w1(d)
    b.w["ff.w1"], b.w["ff.w2"] = W1p.half(), d["W2"].half()
    b1 = b.put(b.fenced(1, 2 * HID, "f32"), b1p[None, :]).ref if b1p is not None else NULL
    b2 = b.put(b.fenced(1, C, "f32"), d["b2"][None, :]).ref if d["b2"] is not None else NULL
    res = b.put(b.fenced(d["res"].shape[0], C, "f32"), d["res"]) if d["res"] is not None else None
    b.hidden = b.fenced(M, HID, "f16")
    full = shared if out_over_x else b.fenced(M, 2 * C if c["out_lo"] else C, "f16")
    b.out, b.lo = full.col_slice(0, C), (full.col_slice(C, 2 * C) if c["out_lo"] else None)
    b.full = full
    scratch, copy_dst = P.alloc(8, 64, "f32"), P.alloc(M, HID, "f16")
    P.force_tile = 2
    ge = P.gemm("ff.geglu", x, Ref("weight", 0, "ff.w1"), 2 * HID, C, b.hidden, bias=b1, epi=L.EPI_GEGLU, allow_splitk=False)
    if waive_cutoff:
        ge.i[31] = 1
    P.memset("scratch", scratch)
    P.force_tile = 8
    residual = res
    if res is not None and c["wrap"]:
        residual = Buf(res.ref, res.rows, res.cols, res.ld, "f32", res.alloc_off)
    pr = P.gemm("ff.net.2", b.hidden, Ref("weight", 0, "ff.w2"), C, HID, Buf(b.out.ref, M, C, b.out.ld, "f16", b.out.alloc_off), bias=b2,
                residual=residual, res_wrap=M // 2 if c["wrap"] else 0, out_lo=c["out_lo"], allow_splitk=split_k)
    P.force_tile = None
    P.copy2d("reader", b.hidden, copy_dst)
    b.k_geglu, b.k_memset, b.k_proj, b.k_copy = 0, 1, len(P.ops) - 2, len(P.ops) - 1
    I, J = ge.i, pr.i
    assert (I[0], I[1], I[2], I[16], I[19], I[22], I[5]) == (M, 2 * HID, C, L.EPI_GEGLU, 1, 2, HID + G.PAD_COLS)
    assert (J[0], J[1], J[2], J[16], J[22], J[3], J[8]) == (M, C, HID, L.EPI_NONE, 8, I[5], 0) and pr.p[0] == ge.p[5]
    assert (J[19] > 1) == split_k and (J[11] == 1) == c["out_lo"] and J[12] == (M // 2 if c["wrap"] else 0)
    return b


def check_fences(it, b, hidden_written):
    """Every window finite, every fence element still NaN; the hidden window: finite when the pair ran as two launches, untouched (all
    NaN) when it ran fused."""
    for big, r0, r1, c1 in b.fences:
        full = it.mat(big.ref, big.rows, big.ld, big.ld, G.TD[big.dtype], {}).clone()
        is_hidden = big.ref.off == b.hidden.alloc_off
        if is_hidden and not hidden_written:
            assert torch.isnan(full).all(), f"{b.case['id']}: the fused launch wrote {int((~torch.isnan(full)).sum())} elements of the hidden buffer"
            continue
        assert torch.isfinite(full[r0:r1, :c1]).all(), f"{b.case['id']}: non-finite values inside a window"
        full[r0:r1, :c1] = G.NAN
        assert torch.isnan(full).all(), f"{b.case['id']}: {int((~torch.isnan(full)).sum())} fence elements written"
