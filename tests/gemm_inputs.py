"""TEST INFRASTRUCTURE — adversarial inputs for every GEMM path (csrc/gemm.hip, csrc/gemm2.hip, the shared tails of t2v_kernels.h), float64
references, and the case list with the programs that run them.  No test functions here: tests/test_gemm_inputs_cpu.py proves on the CPU
what the inputs do (and runs every program through the interpreter), tests/test_gpu_gemm_adversarial.py runs the same programs on the GPU.
Both import CASES / build(), so they cannot drift apart.  Nothing here touches a GPU, imports tests/interp.py or uses packing.py: whoever
executes a program hands its arena view (`it`, anything with Interp's `mat`) to `Built.init` / `verify`; every expected value comes from
`gather_acc` + `epilogue` in float64 (A @ W.T, F.conv2d, F.conv3d on the UNPACKED weights), and the packed weight images the kernels read
are written out below from the ABI (k = (64-channel chunk, tap, channel); GEGLU rows value | gate interleaved by eights).

Why these inputs.  The other GEMM tests fill A, W, bias and residual with i.i.d. randn and assert one rel-L2 over the tensor: every row and
every column then weighs the same, and a row that leaks into its neighbour, a lost K tail in one row, a column quad that went through fp16
or a bias read with the wrong index disappear in the average.  Here
  scaled   A[m, :] = r[m] z, W[n, :] = c[n] w / sqrt(K): r a power of two in [2^-4, 2^4] that differs between neighbouring rows and across
           every multiple of 32, c a power of two in [1/4, 4], constant on a column quad and different between neighbouring quads;
           residual = r[m] c[n] randn, bias = c[n] randn, row bias = c[n] randn (the bias terms are NOT row-scaled: in small rows the bias
           dominates and its indexing is exposed, in large rows the product);
  marked   scaled, and in the operand the columns either side of every multiple of 64 and the last 8 columns weigh 4 x, the border pixels
           of every image (convolution gathers) / the first and last frame of every clip (temporal gather) 4 x: the padding seam, the k-tile
           seams and the K tail weigh most;
  offset   A = 8 sigma + sigma z per row against a zero-mean W (plain gather): a small difference of large terms.
All operands are rounded to their stored dtype before the reference sees them.  All errors are one rel-L2 per ROW SEGMENT — row m with the
32 output columns of one accumulator block, the last one possibly shorter (`seg_err`); EPI_STATS: per (32-row strip, 32 columns).  Asserts
are on the worst segment and no segment is left out (the builder asserts that every segment's reference norm is > 0):
  fp32 outputs, strips, hi + lo   max(2e-5, 4 e_torch): 2e-5 is the suite's figure for fp32 results, e_torch the SAME segment's error of
                                  torch's fp32 CPU result (torch.matmul / F.conv2d / F.conv3d + the same epilogue) against float64;
                                  hi + lo also strictly closer than hi alone in every segment;
  fp16 outputs                    1e-3 (the suite's figure; 2^-11 = 4.9e-4 per element from the format + the fp32 error);
  GEGLU                           max(1e-3, 4 x the error of torch's fp32 value * gelu(gate) rounded to fp16, same segment);
  two-pass a_lo / weight_lo       the fp32 rule against the float64 product of the UNSPLIT fp32 operand; the one-pass fp16 form of the same
                                  case must be worse in its worst segment.

Fencing.  Every tensor a GEMM reads or writes is a window of a larger NaN allocation: PAD_ROWS rows in front and behind and 8 columns to the
right (ld = cols + 8; the strips buffer and the C8 stem's operand have a leading dimension fixed by the ABI and are fenced by rows only).
Outputs start as NaN; `verify` wants every window finite and every fence element still NaN.  fmaxf drops NaN, so the ReLU cases say less
about finiteness and run a second time with act = 0."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd._lib import GEMM2_TILES, tile0_bn          # the tile table: gemm2.hip's general-purpose ids, tile 0's width by N
from sd_webui_text2video_amd.program import NULL, Buf, Program, Ref

TOL_F32 = 2e-5          # fp32 results, strips, hi + lo: the suite's figure
TOL_F16 = 1e-3          # fp16 outputs: the suite's figure
NAN = float("nan")
TD = {"f16": torch.float16, "f32": torch.float32}
PAD_ROWS, PAD_COLS = 3, 8
BM = {t: L.GEMM_TILES[t].bm for t in (0,) + GEMM2_TILES}
BN = {t: L.GEMM_TILES[t].bn for t in GEMM2_TILES}          # tile 0: 64 or 128 by N (tile0_bn)
VARIANTS = ("scaled", "marked", "offset")


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
def row_scale(M):
    m = torch.arange(M)
    return torch.exp2(((5 * m + m // 32) % 9 - 4).double())


def col_scale(N):
    n = torch.arange(N)
    return torch.exp2(((3 * (n // 4) + n // 32) % 5 - 2).double())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def operand_rows(variant, rows, cols, seed, *, image=None, clip=None):
    """The stored operand X [rows, cols] (float64, representable in fp16).  image = (B, H, W): rows are pixels, the border pixels of every
    image are marked; clip = (B, frames, HW): the first and last stored frame of every clip are marked."""
    assert variant in VARIANTS
    z = torch.randn(rows, cols, generator=_gen(seed), dtype=torch.float64)
    X = row_scale(rows)[:, None] * (8.0 + z if variant == "offset" else z)
    if variant == "marked":
        k = torch.arange(cols)
        mark = torch.ones(cols, dtype=torch.float64)
        mark[((k % 64 == 0) & (k > 0)) | ((k % 64 == 63) & (k < cols - 1))] = 4.0
        mark[-8:] = 4.0
        X = X * mark
        if image is not None:
            B, H, W = image
            y, x = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
            border = ((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).reshape(-1).repeat(B)
            X[border] *= 4.0
        if clip is not None:
            B, Fr, HW = clip
            f = torch.arange(Fr).repeat_interleave(HW).repeat(B)
            X[(f == 0) | (f == Fr - 1)] *= 4.0
    return X.half().double()


def weight_like(variant, shape, seed):
    """W [N, ...] (float64, representable in fp16): c[n] w / sqrt(K), K = the reduction length; `offset`: zero mean along the reduction."""
    N, K = shape[0], math.prod(shape[1:])
    w = torch.randn(*shape, generator=_gen(seed + 1), dtype=torch.float64)
    if variant == "offset":
        w = w - w.reshape(N, -1).mean(dim=1).reshape(N, *([1] * (len(shape) - 1)))
    return (w * (col_scale(N) / math.sqrt(K)).reshape(N, *([1] * (len(shape) - 1)))).half().double()


def split_f32(X64):
    """An fp32 operand and its two fp16 images as the product makes them: -> (unsplit fp32 values in float64, hi = fp16(x), lo = fp16(x - hi));
    hi + lo misses x by the rounding of lo, 2^-22 of x."""
    xf = X64.float().double()
    hi = xf.half()
    return xf, hi, (xf - hi.double()).half()


# ---- the packed weight images the kernels read (the ABI, written out) ---------------------------------------------------------------------
def pack_conv3x3(w4):
    """[Co, Ci, 3, 3] -> [Co, 9 Ci], k = (ci // 64) * 576 + (3 ky + kx) * 64 + ci % 64."""
    co, ci = w4.shape[:2]
    assert ci % 64 == 0
    return w4.permute(0, 2, 3, 1).reshape(co, 9, ci // 64, 64).permute(0, 2, 1, 3).reshape(co, 9 * ci)


def pack_conv3x3_c8(w4):
    """The stem: [Co, 8, 3, 3] -> [Co, 72], k = (3 ky + kx) * 8 + ci."""
    assert w4.shape[1] == 8
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], 72)


def pack_tconv3(w5):
    """[Co, Ci, 3, 1, 1] -> [Co, 3 Ci], k = (ci // 64) * 192 + kt * 64 + ci % 64."""
    co, ci = w5.shape[:2]
    assert ci % 64 == 0
    return w5[:, :, :, 0, 0].permute(0, 2, 1).reshape(co, 3, ci // 64, 64).permute(0, 2, 1, 3).reshape(co, 3 * ci)


def geglu_rows(n_half):
    """Packed row 16 u + 8 g + j holds source row g * n_half + 8 u + j (value rows first, gate rows second in the unpermuted Linear)."""
    u, g, j = torch.arange(n_half // 8)[:, None, None], torch.arange(2)[None, :, None], torch.arange(8)[None, None, :]
    return (g * n_half + 8 * u + j).reshape(-1)


# ---- the float64 reference (and, with dtype = float32, torch's own fp32 result: e_torch) --------------------------------------------------
def gather_acc(kind, X, W, geo, dtype=torch.float64):
    """The product before the epilogue, [M, N] in `dtype`.  kind plain: X[:M] @ W.T (a_wrap: row m >= a_wrap is row m - a_wrap);
    conv / c8: F.conv2d on the [Co, Ci, 3, 3] weight (stride, `up` = nearest x 2 first, pad_after_only = padding (0, 1, 0, 1));
    tconv: F.conv3d, kernel (3, 1, 1), zero padding of one frame — or none when the stored clip carries its halo frames."""
    X, W = X.to(dtype), W.to(dtype)
    if kind == "plain":
        M, aw = geo["M"], geo.get("a_wrap", 0)
        A = torch.cat([X[:aw], X[:M - aw]]) if aw else X[:M]
        return A @ W.t()
    if kind in ("conv", "c8"):
        B, H, Wd = geo["image"]
        x = X.view(B, H, Wd, -1).permute(0, 3, 1, 2)
        if geo.get("up"):
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        x = F.pad(x, (0, 1, 0, 1) if geo.get("pad_after_only") else (1, 1, 1, 1))
        y = F.conv2d(x, W, stride=geo.get("stride", 1))
        return y.permute(0, 2, 3, 1).reshape(-1, W.shape[0])
    assert kind == "tconv"
    B, Fr, HW = geo["clip"]                           # Fr: STORED frames (with the halo frames in the halo layout)
    x = X.view(B, Fr, HW, -1).permute(0, 3, 1, 2)[..., None]
    y = F.conv3d(x, W, padding=(0 if geo.get("halo") else 1, 0, 0))
    return y.permute(0, 2, 3, 1, 4).reshape(-1, W.shape[0])


def conv_out_hw(geo):
    B, H, W = geo["image"]
    if geo.get("up"):
        H, W = 2 * H, 2 * W
    pad = 1 if geo.get("pad_after_only") else 2
    s = geo.get("stride", 1)
    return (H + pad - 3) // s + 1, (W + pad - 3) // s + 1


def out_rows(kind, geo):
    if kind == "plain":
        return geo["M"]
    if kind == "tconv":
        B, Fr, HW = geo["clip"]
        return B * (Fr - 2 if geo.get("halo") else Fr) * HW
    ho, wo = conv_out_hw(geo)
    return geo["image"][0] * ho * wo


def epilogue(acc, e):
    """bias (along N, or along M) -> row bias per rows_per_batch -> SiLU / ReLU -> residual (row m >= res_wrap reads row m - res_wrap) ->
    GEGLU from the unpermuted definition value * gelu(gate), in acc's dtype."""
    dt, v, M = acc.dtype, acc, acc.shape[0]
    if e.get("bias") is not None:
        v = v + (e["bias"].to(dt)[:, None] if e.get("bias_m") else e["bias"].to(dt)[None, :])
    if e.get("rowbias") is not None:
        v = v + e["rowbias"].to(dt)[torch.arange(M) // e["rpb"]]
    if e.get("act") == L.ACT_SILU:
        v = v * torch.sigmoid(v)
    elif e.get("act") == L.ACT_RELU:
        v = torch.relu(v)
    if e.get("res") is not None:
        R, rw = e["res"].to(dt), e.get("res_wrap", 0)
        v = v + (torch.cat([R[:rw], R[:M - rw]]) if rw else R[:M])
    if e.get("geglu"):
        h = v.shape[1] // 2
        v = v[:, :h] * F.gelu(v[:, h:])
    return v


def strip_sums(stored, dtype=torch.float64):
    """[ceil(M / 32), 2, N]: column sums / sums of squares of the stored values per 32-row strip; a ragged last strip counts its real rows."""
    M, N = stored.shape
    ns = -(-M // 32)
    pad = torch.zeros(ns * 32, N, dtype=dtype)
    pad[:M] = stored.to(dtype)
    s = pad.view(ns, 32, N)
    return torch.stack([s.sum(dim=1), (s * s).sum(dim=1)], dim=1)


def seg_norms(x):
    """[rows, cols] -> [rows, ceil(cols / 32)]: the L2 norm of every run of 32 columns (the last one may be shorter)."""
    return torch.stack([p.norm(dim=1) for p in x.double().split(32, dim=1)], dim=1)


def seg_err(got, ref):
    """One rel-L2 per row segment."""
    return seg_norms(got.double() - ref.double()) / seg_norms(ref).clamp_min(1e-300)


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


# ---- programs -----------------------------------------------------------------------------------------------------------------------------
class Built:
    """A case's program, weights, initial arena contents, fences and expectations."""

    def __init__(self, case):
        self.case = case
        self.P = Program()
        self.w = {}
        self.fences = []        # (allocation, r0, r1, c1): rows r0 .. r1 - 1 x columns 0 .. c1 - 1 are the window, the rest stays NaN
        self.sets = []          # (window, tensor) written before the run
        self.outs = []          # the expectations: see _Run.emit
        self.paths = []         # what the op records were asserted to say, one entry per op
        self.features = set()   # what the case covers (tests/test_gemm_inputs_cpu.py asserts the union over CASES)

    def fenced(self, rows, cols, dtype, pad_cols=PAD_COLS):
        big = self.P.alloc(rows + 2 * PAD_ROWS, cols + pad_cols, dtype)
        self.fences.append((big, PAD_ROWS, PAD_ROWS + rows, cols))
        return big.row_slice(PAD_ROWS, PAD_ROWS + rows).col_slice(0, cols)

    def put(self, win, t):
        assert (win.rows, win.cols) == tuple(t.shape), (win.rows, win.cols, t.shape)
        assert torch.equal(t.to(TD[win.dtype]).double(), t.double()), "inputs must be representable in their stored dtype"
        self.sets.append((win, t))
        return win

    def init(self, it):
        for big, _, _, _ in self.fences:
            it.mat(big.ref, big.rows, big.ld, big.ld, TD[big.dtype], {}).fill_(NAN)
        for win, t in self.sets:
            it.mat(win.ref, win.rows, win.cols, win.ld, TD[win.dtype], {}).copy_(t.to(TD[win.dtype]))


def _rd(it, win):
    return it.mat(win.ref, win.rows, win.cols, win.ld, TD[win.dtype], {}).clone()


def bound_of(o):
    """The per-segment bound of an expectation (a tensor shaped like its segment errors)."""
    if o["rule"] == "f16":
        return torch.full_like(o["e_torch"], TOL_F16)
    return torch.maximum(torch.full_like(o["e_torch"], TOL_F16 if o["rule"] == "geglu" else TOL_F32), 4.0 * o["e_torch"])


def check(tag, o, got, lo=None):
    """The asserts of one expectation on `got` (and its low-order image)."""
    assert got.shape == o["ref"].shape, (tag, o["name"], got.shape, o["ref"].shape)
    e, bound = seg_err(got, o["ref"]), bound_of(o)
    if lo is not None:
        assert float(e.max()) <= TOL_F16, (tag, o["name"], "hi", float(e.max()))
        e2 = seg_err(got.double() + lo.double(), o["ref"])
        assert bool((e2 < e).all()), (tag, o["name"], "hi + lo is no closer than hi", float((e2 / e.clamp_min(1e-300)).max()))
        e = e2
    k = int(torch.argmax(e / bound))
    fig = (float(e.flatten()[k]), float(o["e_torch"].flatten()[k]), float(bound.flatten()[k]), float(e.max()))
    assert bool((e <= bound).all()), (tag, o["name"], "worst segment %.3e, e_torch %.3e, bound %.3e" % fig, divmod(k, e.shape[1]))
    return fig          # (error, e_torch, bound) of the segment nearest its bound, and the largest segment error


def verify(it, b):
    """Fences and per-segment errors of a finished run -> {"f32": ..., "f16": ...}: per class of bound (fp32 results, strips and hi + lo /
    fp16 and GEGLU outputs) the segment nearest to — or furthest beyond — its bound over the case's outputs, as dict(worst, e_torch, bound,
    name), or None."""
    tag = b.case["id"]
    for big, r0, r1, c1 in b.fences:
        full = it.mat(big.ref, big.rows, big.ld, big.ld, TD[big.dtype], {}).clone()
        assert torch.isfinite(full[r0:r1, :c1]).all(), f"{tag}: non-finite values inside a window"
        full[r0:r1, :c1] = NAN
        assert torch.isnan(full).all(), f"{tag}: {int((~torch.isnan(full)).sum())} fence elements written"
    figs, worst = {"f32": None, "f16": None}, {}

    def note(cls, name, fig):
        if figs[cls] is None or fig[0] / fig[2] > figs[cls]["worst"] / figs[cls]["bound"]:
            figs[cls] = dict(worst=fig[0], e_torch=fig[1], bound=fig[2], name=name)

    for o in b.outs:
        got = _rd(it, o["win"])
        fig = check(tag, o, got, None if o["lo"] is None else _rd(it, o["lo"]))
        worst[o["name"]] = fig[3]
        note("f32" if o["rule"] == "f32" else "f16", o["name"], fig)
        if o["strips"] is not None:
            # the strips are sums of the STORED values: the reference is taken from what the launch stored (itself checked just above)
            ns, N = -(-got.shape[0] // 32), got.shape[1]
            st = _rd(it, o["strips"]).view(ns, 2, N)
            so = dict(name=o["name"] + ".strips", rule="f32")
            for j, what in enumerate(("sums", "sums of squares")):
                so["ref"] = strip_sums(got)[:, j]
                so["e_torch"] = seg_err(strip_sums(got, torch.float32)[:, j], so["ref"])
                assert bool((seg_norms(so["ref"]) > 0).all()), (tag, what)
                note("f32", so["name"], check(tag + " strip " + what, so, st[:, j]))
    for o in b.outs:
        if o["beats"] is not None:
            assert worst[o["name"]] < worst[o["beats"]], (tag, "the two-pass form is no closer than the one-pass form", worst[o["name"]], worst[o["beats"]])
    return figs


def figures_line(b, figs):
    f = lambda g: "-" if g is None else f"{g['worst']:.2e} ({g['name']}, e_torch {g['e_torch']:.2e}, bound {g['bound']:.2e})"
    return f"GEMMADV {b.case['id']}: ops [{' | '.join(b.paths)}] worst fp32-class segment {f(figs['f32'])}; worst fp16-class segment {f(figs['f16'])}"


_GATHER = dict(plain=L.GATHER_PLAIN, conv=L.GATHER_CONV3X3, c8=L.GATHER_CONV3X3_C8, tconv=L.GATHER_TCONV3)


class _Run:
    """One GEMM op of a case on a shared operand: the constructor allocates every fenced buffer, `emit` appends the op, asserts the path
    from its record and registers the expectation.  (Every buffer of a case is allocated before its first op: an op's scratch is freed when
    it is emitted, and a fenced buffer allocated later would land on it.)"""

    def __init__(self, b, name, kind, a, X, W, geo, *, seed, tile, out_dt="f32", bias=None, rpb=0, act=0, res=False, res_wrap=0, geglu=False,
                 stats=False, out_lo=False, split=1, tickets=False, w_arena=False, a_lo=None, X_full=None, W_full=None, w_lo=False, beats=None,
                 target_cus=None):
        self.b, self.name, self.kind, self.a, self.X, self.W, self.geo, self.tile, self.out_dt = b, name, kind, a, X, W, geo, tile, out_dt
        self.bias, self.rpb, self.act, self.res, self.res_wrap, self.geglu, self.out_lo = bias, rpb, act, res, res_wrap, geglu, out_lo
        self.split, self.tickets, self.a_lo, self.X_full, self.W_full, self.w_lo, self.beats = split, tickets, a_lo, X_full, W_full, w_lo, beats
        self.target_cus, self.uneven = target_cus, False
        N = W.shape[0]
        M = out_rows(kind, geo)
        self.M, self.N, self.K = M, N, math.prod(W.shape[1:])
        n_out = N // 2 if geglu else N
        g, c = _gen(seed + 7), col_scale(N)
        e = dict(act=act, geglu=geglu)
        Wp = {"plain": lambda w: w, "conv": pack_conv3x3, "c8": pack_conv3x3_c8, "tconv": pack_tconv3}[kind](W)
        rows_perm = geglu_rows(N // 2) if geglu else torch.arange(N)
        self.wref = self._weight(name + ".w", Wp[rows_perm], w_arena)
        self.wlo_ref = None
        if w_lo:
            _, whi, wlo = split_f32(W_full)
            self.wref, self.wlo_ref = self._weight(name + ".w", whi.double(), False), self._weight(name + ".w_lo", wlo.double(), False)
        self.bias_ref = None
        if bias is not None:
            e["bias"] = (torch.randn(M, generator=g) if bias == "m" else c.float() * torch.randn(N, generator=g)).double()
            e["bias_m"] = bias == "m"
            bw = b.put(b.fenced(1, M if bias == "m" else N, "f32"), (e["bias"] if bias == "m" else e["bias"][rows_perm])[None, :])
            self.bias_ref = bw.ref
        self.rb = None
        if rpb:
            assert M % rpb == 0
            e["rowbias"], e["rpb"] = (c.float() * torch.randn(M // rpb, N, generator=g)).double(), rpb
            self.rb = b.put(b.fenced(M // rpb, N, "f32"), e["rowbias"])
        self.res_buf = None
        if res:
            rr = res_wrap or M
            e["res"], e["res_wrap"] = (row_scale(M)[:rr, None].float() * c.float() * torch.randn(rr, n_out, generator=g)).double(), res_wrap
            self.res_buf = b.put(b.fenced(rr, n_out, "f32"), e["res"])
        self.e = e
        self.st = b.fenced(-(-M // 32), 2 * N, "f32", pad_cols=0) if stats else None        # (ld = 2 N is the ABI's)
        full = b.fenced(M, 2 * n_out if out_lo else n_out, out_dt)
        self.out, self.lo = full.col_slice(0, n_out), (full.col_slice(n_out, 2 * n_out) if out_lo else None)

    def _weight(self, name, Wp, in_arena):
        if in_arena:
            return self.b.put(self.b.fenced(Wp.shape[0], Wp.shape[1], "f16"), Wp).ref, Wp.shape[1] + PAD_COLS
        self.b.w[name] = Wp.half()
        return Ref("weight", 0, name), None

    def emit(self):
        b, P, geo, kind, M, N, K, e = self.b, self.b.P, self.geo, self.kind, self.M, self.N, self.K, self.e
        P.force_tile, P.splitk_tickets = self.tile, self.tickets
        P.target_cus = self.target_cus or 256
        conv = None
        if kind in ("conv", "c8"):
            B, H, Wd = geo["image"]
            ho, wo = conv_out_hw(geo)
            conv = dict(Hin=H, Win=Wd, Cin=self.X.shape[1], stride=geo.get("stride", 1), up=int(bool(geo.get("up"))), Hout=ho, Wout=wo,
                        pad_after_only=bool(geo.get("pad_after_only")))
        elif kind == "tconv":
            B, Fr, HW = geo["clip"]
            conv = dict(F=Fr - 2 if geo.get("halo") else Fr, HW=HW, Cin=self.X.shape[1])
        (wref, ldw) = self.wref
        P.weight_lo = (lambda w: self.wlo_ref[0] if w == wref else None) if self.w_lo else None
        residual, plain_i30 = self.res_buf, False
        if self.res_wrap and kind == "plain" and self.split > 1:
            # Program.gemm turns split-K off beside i[12]; the record's own residual wrap of every gather (i[30]) is honoured by both folds:
            # hand the lowering a view that claims M rows of the `res_wrap`-row window and set the word on the emitted record
            residual, plain_i30 = Buf(self.res_buf.ref, M, self.res_buf.cols, self.res_buf.ld, "f32", self.res_buf.alloc_off), True
        out = Buf(self.out.ref, M, self.out.cols, self.out.ld, self.out.dtype, self.out.alloc_off)
        n0 = len(P.ops)
        op = P.gemm(self.name, self.a, wref, N, K, out, bias=self.bias_ref or NULL, ldw=ldw, gather=_GATHER[kind], conv=conv, rowbias=self.rb,
                    rows_per_batch=self.rpb, residual=residual, epi=L.EPI_GEGLU if self.geglu else L.EPI_NONE, act=self.act,
                    bias_along_m=self.bias == "m", m=M, allow_splitk=self.split > 1, halo=bool(geo.get("halo")), a_lo=self.a_lo,
                    out_lo=self.out_lo, stats=self.st, a_wrap=geo.get("a_wrap", 0), res_wrap=0 if plain_i30 else self.res_wrap)
        P.weight_lo = None
        if plain_i30:
            op.i[30] = self.res_wrap
        # ---- the path this run names, from the op records ----
        I = op.i
        assert (I[0], I[1], I[2], I[7], I[22], I[19]) == (M, N, K, _GATHER[kind], self.tile, self.split), (self.name, I[:8], I[22], I[19], self.split)
        assert self.tile == 0 or K % 64 == 0, "the executor would fall back to gemm.hip silently"
        assert I[16] == (L.EPI_GEGLU if self.geglu else L.EPI_STATS if self.st is not None else L.EPI_NONE) and op.meta["stats"] == int(self.st is not None)
        assert (op.p[7].space != "null") == (self.st is not None or (self.tickets and self.split > 1 and not self.geglu))
        assert (op.p[6].space != "null") == (self.split > 1) and I[18] == self.act and I[20] == int(self.bias == "m") and I[15] == self.rpb
        assert I[17] == (L.F32 if self.out_dt == "f32" else L.F16)
        if kind == "plain":
            assert (I[11] == 1) == self.out_lo and I[13] == geo.get("a_wrap", 0) and (I[12], I[30]) == ((0, self.res_wrap) if plain_i30 else (self.res_wrap, 0))
        else:
            assert I[30] == self.res_wrap and I[23] == int(bool(geo.get("halo") or geo.get("pad_after_only")))
        assert len(P.ops) - n0 == (2 if (self.a_lo is not None or self.w_lo) else 1)
        if self.split > 1:
            kt, per = -(-K // 64), -(-(-(-K // 64)) // self.split)
            assert -(-kt // per) == self.split, "the launcher would drop an empty split"
            self.uneven = kt % per != 0
        bn = tile0_bn(N) if self.tile == 0 else BN[self.tile]
        feats = {f"tile{self.tile}" + (f"/{bn}" if self.tile == 0 else ""), "gather:" + kind + ("/halo" if geo.get("halo") else ""), "out:" + self.out_dt}
        feats |= {f for f, on in (("bias_n", self.bias == "n"), ("bias_m", self.bias == "m"), ("rowbias", self.rpb), ("silu", self.act == 1),
                                  ("relu", self.act == 2), ("residual", self.res), ("geglu", self.geglu), ("stats:" + self.out_dt, self.st is not None),
                                  ("out_lo", self.out_lo), ("a_lo", self.a_lo is not None), ("weight_lo", self.w_lo), ("ldw", ldw),
                                  ("a_wrap", geo.get("a_wrap")), ("res_wrap:i12", self.res_wrap and kind == "plain" and not plain_i30),
                                  ("res_wrap:i30:" + kind, self.res_wrap and (kind != "plain" or plain_i30)),
                                  ("stride2", geo.get("stride") == 2), ("up", geo.get("up")), ("pad_after_only", geo.get("pad_after_only"))) if on}
        if self.split > 1:
            fold = "tickets" if op.p[7].space != "null" else "reduce"
            feats |= {"splitk:" + fold, f"splitk:{fold}:tile{self.tile}"} | ({"splitk:uneven"} if self.uneven else set())
            feats |= {f"splitk:{fold}:{f}" for f in feats if f in ("bias_n", "bias_m", "rowbias", "silu", "geglu", "out_lo") or f.startswith("res_wrap")}
        b.features |= feats
        b.paths.append(f"{self.name} tile {self.tile}" + (f"/{bn}" if self.tile == 0 else "") + f" {kind} {M}x{N}x{K}" +
                       (f" split {self.split} {'tickets' if op.p[7].space != 'null' else 'reduce'}" if self.split > 1 else ""))
        # ---- the expectation ----
        Xr, Wr = (self.X if self.X_full is None else self.X_full), (self.W if self.W_full is None else self.W_full)
        acc = gather_acc(kind, Xr, Wr, geo)
        ref = epilogue(acc, e)
        t32 = epilogue(gather_acc(kind, Xr, Wr, geo, torch.float32), e)
        rule = "geglu" if self.geglu else "f32" if (self.out_dt == "f32" or self.out_lo) else "f16"
        e_torch = seg_err(t32.half() if rule == "geglu" else t32, ref)
        assert bool((seg_norms(ref) > 0).all()), (self.name, "a segment with a zero reference")
        b.outs.append(dict(name=self.name, win=self.out, lo=self.lo, ref=ref, rule=rule, e_torch=e_torch, strips=self.st, beats=self.beats,
                           run=self, acc=acc))
        return op


def _case(family, id, **kw):
    c = dict(family=family, id=id, variant="scaled", seed=1000 + len(CASES))
    c.update(kw)
    return c


def _plain_operand(b, variant, rows, K, seed):
    X = operand_rows(variant, rows, K, seed)
    return b.put(b.fenced(rows, K, "f16"), X), X


# -- every instantiation, plain gather: one whole tile + a 32-row block + a 5-row block + dead blocks; one whole column tile + a block + a quad ---
def _build_inst(c):
    b = Built(c)
    tile, K, v = c["tile"], c["K"], c["variant"]
    N = c["N"] if tile == 0 else BN[tile] + 36
    a, X = _plain_operand(b, v, 333, K, c["seed"])
    W = weight_like(v, (N, K), c["seed"])
    kw = dict(seed=c["seed"], tile=tile)
    runs = [_Run(b, "f32res", "plain", a, X, W, dict(M=BM[tile] + 37), res=True, w_arena=True, **kw),
            _Run(b, "f16rowbias", "plain", a, X, W, dict(M=333), out_dt="f16", bias="n", rpb=37, act=L.ACT_SILU, **kw)]
    for r in runs:
        r.emit()
    return b


# -- gemm.hip only: the K tail (K % 64 != 0, K < 64) and a single column quad ---------------------------------------------------------------
def _build_tail(c):
    b = Built(c)
    a, X = _plain_operand(b, c["variant"], 165, c["K"], c["seed"])
    W = weight_like(c["variant"], (c["N"], c["K"]), c["seed"])
    kw = dict(seed=c["seed"], tile=0)
    runs = [_Run(b, "f32res", "plain", a, X, W, dict(M=165), res=True, bias="n", w_arena=True, **kw),
            _Run(b, "f16", "plain", a, X, W, dict(M=165), out_dt="f16", bias="n", **kw)]
    for r in runs:
        r.emit()
    assert b.P.ops[0].i[22] == 0
    return b


# -- split-K with an uneven last split, both folds -----------------------------------------------------------------------------------------
def _build_splitk(c):
    b = Built(c)
    tile, K, split, v = c["tile"], c["K"], c["split"], c["variant"]
    M, N = 185, (164 if tile == 0 else BN[tile] + 36)
    a, X = _plain_operand(b, v, M, K, c["seed"])
    W, Wg = weight_like(v, (N, K), c["seed"]), weight_like(v, (288, K), c["seed"] + 50)
    kw = dict(seed=c["seed"], tile=tile, split=split, tickets=c["tickets"])
    runs = [_Run(b, "f32-biasn-rowbias-silu-reswrap", "plain", a, X, W, dict(M=M), bias="n", rpb=37, act=L.ACT_SILU, res=True, res_wrap=100, **kw),
            _Run(b, "hilo-biasm", "plain", a, X, W, dict(M=M), out_dt="f16", bias="m", out_lo=True, **kw),
            _Run(b, "geglu", "plain", a, X, Wg, dict(M=M), out_dt="f16", bias="n", geglu=True, **kw)]
    ops = [r.emit() for r in runs]
    assert all(r.uneven for r in runs), "the last split must be shorter"
    assert ops[2].p[7].space == "null", "GEGLU folds in the reduction kernel"
    return b


# -- bias along M, ReLU, a_wrap and res_wrap of the plain gather (i[12]); the wrap sits inside a 32-row block -------------------------------
def _build_feat(c):
    """N = BN + 60 (one whole column tile, a block and 7 quads): ReLU leaves zeros, and a one-quad segment (N = BN + 36) would be all zero
    in one row out of 16 — no reference norm to divide by.  For the same reason ReLU runs with the bias along N only: in a small-scale row
    a negative bias along M zeroes the whole row."""
    b = Built(c)
    tile, v, M, wrap, K = c["tile"], c["variant"], 293, 150, 384
    N = 188 if tile == 0 else BN[tile] + 60
    a, X = _plain_operand(b, v, wrap, K, c["seed"])
    a2, X2 = _plain_operand(b, v, M, K, c["seed"] + 3)
    W = weight_like(v, (N, K), c["seed"])
    kw = dict(seed=c["seed"], tile=tile)
    runs = [_Run(b, "wraps-biasm", "plain", a, X, W, dict(M=M, a_wrap=wrap), bias="m", res=True, res_wrap=wrap, **kw),
            _Run(b, "biasm-f16", "plain", a2, X2, W, dict(M=M), out_dt="f16", bias="m", **kw),
            _Run(b, "relu", "plain", a2, X2, W, dict(M=M), out_dt="f16", bias="n", act=L.ACT_RELU, **kw),
            _Run(b, "relu-off", "plain", a2, X2, W, dict(M=M), out_dt="f16", bias="n", **kw),
            _Run(b, "relu-f32", "plain", a2, X2, W, dict(M=M), bias="n", act=L.ACT_RELU, **kw),
            _Run(b, "relu-f32-off", "plain", a2, X2, W, dict(M=M), bias="n", **kw)]
    for r in runs:
        r.emit()
    return b


# -- 3x3 convolution: images of 5 x 7 (a swapped H / W shows), B = 3, Cout = 132 ------------------------------------------------------------
def _conv_operand(b, v, image, cin, seed, c8=False):
    B, H, Wd = image
    X = operand_rows(v, B * H * Wd, cin, seed, image=image)
    return b.put(b.fenced(B * H * Wd, cin, "f16", pad_cols=0 if c8 else PAD_COLS), X), X          # (the stem's lda == 8 is the ABI's)


def _build_conv(c):
    b = Built(c)
    tile, cin, v, image = c["tile"], c["cin"], c["variant"], (3, 5, 7)
    a, X = _conv_operand(b, v, image, cin, c["seed"])
    W = weight_like(v, (132, cin, 3, 3), c["seed"])
    kw = dict(seed=c["seed"], tile=tile)
    runs = [_Run(b, "s1", "conv", a, X, W, dict(image=image), bias="n", res=True, **kw),
            _Run(b, "s2", "conv", a, X, W, dict(image=image, stride=2), out_dt="f16", bias="n", **kw),
            _Run(b, "up", "conv", a, X, W, dict(image=image, up=1), bias="n", **kw),
            _Run(b, "pad-after", "conv", a, X, W, dict(image=image, stride=2, pad_after_only=1), out_dt="f16", bias="n", act=L.ACT_SILU, **kw)]
    for r in runs:
        r.emit()
    assert [r.M for r in runs] == [105, 36, 420, 18]
    return b


def _build_c8(c):
    b = Built(c)
    image = (3, 5, 7)
    a, X = _conv_operand(b, c["variant"], image, 8, c["seed"], c8=True)
    W = weight_like(c["variant"], (132, 8, 3, 3), c["seed"])
    kw = dict(seed=c["seed"], tile=0)
    for r in [_Run(b, "stem", "c8", a, X, W, dict(image=image), bias="n", **kw), _Run(b, "stem-f16", "c8", a, X, W, dict(image=image), out_dt="f16", bias="n", **kw)]:
        r.emit()
    return b


# -- temporal convolution: B = 2, F = 5, HW = 6, zero-padded and halo layouts ---------------------------------------------------------------
def _build_tconv(c):
    b = Built(c)
    tile, v, cin = c["tile"], c["variant"], 128
    X = operand_rows(v, 2 * 5 * 6, cin, c["seed"], clip=(2, 5, 6))
    Xh = operand_rows(v, 2 * 7 * 6, cin, c["seed"] + 3, clip=(2, 7, 6))
    a, ah = b.put(b.fenced(60, cin, "f16"), X), b.put(b.fenced(84, cin, "f16"), Xh)
    W = weight_like(v, (132, cin, 3, 1, 1), c["seed"])
    kw = dict(seed=c["seed"], tile=tile)
    runs = [_Run(b, "padded", "tconv", a, X, W, dict(clip=(2, 5, 6)), bias="n", res=True, **kw),
            _Run(b, "halo", "tconv", ah, Xh, W, dict(clip=(2, 7, 6), halo=1), out_dt="f16", bias="n", **kw)]
    for r in runs:
        r.emit()
    assert [r.M for r in runs] == [60, 60]
    return b


# -- the residual wrap of the convolution gathers (i[30]), with and without split-K ---------------------------------------------------------
def _build_reswrap(c):
    b = Built(c)
    tile, v, kind, split = c["tile"], c["variant"], c["kind"], c["split"]
    kw = dict(seed=c["seed"], tile=tile, target_cus=c.get("cus"))
    if kind == "conv":
        image, cin = (3, 5, 7), c["cin"]
        a, X = _conv_operand(b, v, image, cin, c["seed"])
        W = weight_like(v, (132, cin, 3, 3), c["seed"])
        geo, wrap = dict(image=image), 70
    else:
        cin = c["cin"]
        X = operand_rows(v, 60, cin, c["seed"], clip=(2, 5, 6))
        a = b.put(b.fenced(60, cin, "f16"), X)
        W = weight_like(v, (132, cin, 3, 1, 1), c["seed"])
        geo, wrap = dict(clip=(2, 5, 6)), 30
    runs = [_Run(b, "nosplit", kind, a, X, W, geo, bias="n", res=True, res_wrap=wrap, **kw)]
    if split > 1:
        runs += [_Run(b, "reduce", kind, a, X, W, geo, bias="n", res=True, res_wrap=wrap, split=split, **kw),
                 _Run(b, "tickets", kind, a, X, W, geo, out_dt="f16", bias="n", res=True, res_wrap=wrap, split=split, tickets=True, **kw)]
    for r in runs:
        r.emit()
    return b


# -- EPI_STATS with a ragged last strip; out_lo without split-K -----------------------------------------------------------------------------
def _build_stats(c):
    b = Built(c)
    tile, v, K = c["tile"], c["variant"], 384
    M, N = BM[tile] + 37, (164 if tile == 0 else BN[tile] + 36)
    a, X = _plain_operand(b, v, M, K, c["seed"])
    W = weight_like(v, (N, K), c["seed"])
    kw = dict(seed=c["seed"], tile=tile)
    runs = [_Run(b, "stats-f32", "plain", a, X, W, dict(M=M), bias="n", res=True, stats=True, **kw),
            _Run(b, "stats-f16", "plain", a, X, W, dict(M=M), out_dt="f16", bias="n", stats=True, **kw)]
    if c.get("out_lo"):
        runs.append(_Run(b, "hilo", "plain", a, X, W, dict(M=M), out_dt="f16", bias="n", res=True, out_lo=True, **kw))
    for r in runs:
        r.emit()
    return b


# -- the two-pass forms: the operand that is split is fp32 = hi + lo exactly ----------------------------------------------------------------
def _build_twopass(c):
    b = Built(c)
    v, M, N, K = c["variant"], 165, 164, 384
    g = _gen(c["seed"])
    W = weight_like(v, (N, K), c["seed"])
    kw = dict(seed=c["seed"], tile=0)
    if c["which"] == "a_lo":
        Xf, hi, lo = split_f32(row_scale(M)[:, None] * torch.randn(M, K, generator=g, dtype=torch.float64))
        a, al = b.put(b.fenced(M, K, "f16"), hi.double()), b.put(b.fenced(M, K, "f16"), lo.double())
        runs = [_Run(b, "one-pass", "plain", a, hi.double(), W, dict(M=M), bias="n", res=True, X_full=Xf, **kw),
                _Run(b, "two-pass", "plain", a, hi.double(), W, dict(M=M), bias="n", res=True, a_lo=al, X_full=Xf, beats="one-pass", **kw)]
    else:
        Wf, whi, _ = split_f32(col_scale(N)[:, None] * torch.randn(N, K, generator=g, dtype=torch.float64) / math.sqrt(K))
        a, X = _plain_operand(b, v, M, K, c["seed"])
        runs = [_Run(b, "one-pass", "plain", a, X, whi.double(), dict(M=M), bias="n", res=True, W_full=Wf, **kw),
                _Run(b, "two-pass", "plain", a, X, whi.double(), dict(M=M), bias="n", res=True, w_lo=True, W_full=Wf, beats="one-pass", **kw)]
    runs[0].emit()
    op = runs[1].emit()
    first = b.P.ops[-2]
    assert first.name.endswith("." + c["which"].replace("weight_lo", "w_lo")) and op.p[4].space == "arena" and first.p[5] == op.p[4], "the second pass adds the first"
    b.outs[0]["rule"] = "f16"            # the one-pass form is only here to be beaten (bound_of: a flat 1e-3; it is off by the operand's rounding)
    return b


# -- `offset`: the honesty check of the fp32 accumulate, once without split-K and once with -------------------------------------------------
def _build_offset(c):
    b = Built(c)
    tile = c["tile"]
    M, N = BM[tile] + 37, (164 if tile == 0 else BN[tile] + 36)
    a1, X1 = _plain_operand(b, "offset", M, 384, c["seed"])
    a2, X2 = _plain_operand(b, "offset", M, 1600, c["seed"] + 3)
    kw = dict(seed=c["seed"], tile=tile)
    runs = [_Run(b, "nosplit", "plain", a1, X1, weight_like("offset", (N, 384), c["seed"]), dict(M=M), **kw),
            _Run(b, "split", "plain", a2, X2, weight_like("offset", (N, 1600), c["seed"] + 3), dict(M=M), split=3, **kw)]
    for r in runs:
        r.emit()
    return b


# -- `lowered`: one case per code path that a lowered program takes and no case above has (tests/record_paths.py is the key, ---------------
# -- tests/test_record_paths_cpu.py the check that demands them; profiles/lowered_paths.txt names a deployed op for each) ------------------
def _lowered_geo(s, bm):
    """(kind, geo, cin, rows per bias batch, residual wrap) of a spec: two row tiles of the tile and — m_ragged — a remainder (8 x 8 images
    where the row count must be whole tiles, 6 x 10 where it must not; clips of 5 frames, 7 stored in the halo layout)."""
    kind, ragged, split = s["gather"], s["m_ragged"], s["fold"] != "-"
    if kind == "plain":
        M = 2 * bm + (36 if ragged else 0)
        return dict(M=M), (200 if s["k_tail"] else 1024 if split else 128), M // 2 if ragged else bm // 2, M // 2 + 13
    if kind in ("conv", "c8"):
        H, W = (6, 10) if ragged else (8, 8)
        geo = dict(image=(1, H, W), stride=s["stride"], up=s["up"], pad_after_only=s["i23"])
        ho, wo = conv_out_hw(geo)
        B = -(-2 * bm // (ho * wo)) + (1 if ragged else 0)
        while (B * ho * wo % bm != 0) != bool(ragged):
            B += 1
        geo["image"] = (B, H, W)
        return geo, (8 if kind == "c8" else 128 if split else 64), ho * wo, -(-B // 2) * ho * wo
    HW = bm // 4 + 3 if ragged else bm // 2
    Fr = 7 if s["i23"] else 5
    return dict(clip=(2, Fr, HW), halo=s["i23"]), (384 if split else 128), 5 * HW, 5 * HW


def _lowered_n(s):
    """Two column tiles, or one and 48 columns (a multiple of 16: the GEGLU interleave; three quads past a 32-column block: ReLU leaves no
    all-zero segment); tile 0: the width class the spec names."""
    if s["tile"] == 0:
        return {(128, 0): 256, (128, 1): 240, (64, 0): 192, (64, 1): 176}[(s["w"], s["n_ragged"])]
    return 2 * BN[s["tile"]] if not s["n_ragged"] else BN[s["tile"]] + 48


def _build_lowered(c):
    """K: two 64-chunks (128; 9 / 3 taps x one or two chunks for the convolutions) without split-K.  With it the lowering's own policy
    (Program.choose_tile) wants 16 k-tiles before it splits, so K is 1024 / 1152 and the case plans for just enough compute units that the
    policy takes two splits of 8 / 9 k-tiles — the smallest split-K problem the lowering can emit."""
    b, s = Built(c), c
    tile, v = s["tile"], c["variant"]
    bm = BM[tile]
    geo, cin, rpb, wrap = _lowered_geo(s, bm)
    kind, N, split = s["gather"], _lowered_n(s), (2 if s["fold"] != "-" else 1)
    if kind == "plain":
        a, X = _plain_operand(b, v, geo["M"], cin, c["seed"])
        W = weight_like(v, (N, cin), c["seed"])
    elif kind in ("conv", "c8"):
        a, X = _conv_operand(b, v, geo["image"], cin, c["seed"], c8=kind == "c8")
        W = weight_like(v, (N, cin, 3, 3), c["seed"])
    else:
        B, Fr, HW = geo["clip"]
        X = operand_rows(v, B * Fr * HW, cin, c["seed"], clip=geo["clip"])
        a = b.put(b.fenced(B * Fr * HW, cin, "f16"), X)
        W = weight_like(v, (N, cin, 3, 1, 1), c["seed"])
    M = out_rows(kind, geo)
    cus = None
    if split > 1:
        tiles = -(-M // bm) * -(-N // (tile0_bn(N) if tile == 0 else BN[tile]))
        cus = 2 * tiles + (1 if tile == 0 else 0)
    r = _Run(b, "op", kind, a, X, W, geo, seed=c["seed"], tile=tile, out_dt="f32" if s["out"] else "f16", bias=s["bias"], rpb=rpb if s["rowbias"] else 0,
             act=s["act"], res=bool(s["res"]), res_wrap=wrap if s["res_wrap"] != "-" else 0, geglu=s["epi"] == L.EPI_GEGLU, stats=s["epi"] == L.EPI_STATS,
             out_lo=bool(s["out_lo"]), split=split, tickets=s["fold"] == "tickets", target_cus=cus)
    op = r.emit()
    assert (M % bm != 0) == bool(s["m_ragged"]) and M > bm and (op.i[30] > 0) == (s["res_wrap"] == "i30") and (kind != "plain" or (op.i[12] > 0) == (s["res_wrap"] == "i12"))
    return b


def _lowered_case(spec):
    """spec: the fields of a GEMM path key, in the order of _LOWERED_FIELDS."""
    s = dict(zip(_LOWERED_FIELDS, spec))
    s["gather"] = {L.GATHER_PLAIN: "plain", L.GATHER_CONV3X3: "conv", L.GATHER_TCONV3: "tconv", L.GATHER_CONV3X3_C8: "c8"}[s["gather"]]
    s["bias"] = {0: None, 1: "n", 2: "m"}[s["bias"]]
    cid = "lowered-t%d%s-%s%s%s%s-%s%s%s-e%d-%s-a%d-b%s%s%s%s%s" % (
        s["tile"], f"w{s['w']}" if s["tile"] == 0 else "", s["gather"], "-s2" if s["stride"] == 2 else "", "-up" if s["up"] else "", "-i23" if s["i23"] else "",
        s["fold"].replace("-", "nosplit"), "-ktail" if s["k_tail"] else "", ("-mr" if s["m_ragged"] else "") + ("-nr" if s["n_ragged"] else ""), s["epi"],
        "f32" if s["out"] else "f16", s["act"], s["bias"] or "0", "-rowbias" if s["rowbias"] else "", "-res" if s["res"] else "",
        "-wrap_" + s["res_wrap"] if s["res_wrap"] != "-" else "", "-hilo" if s["out_lo"] else "")
    # (GEGLU multiplies two results: with the marked columns' extra weight a product of two 3-sigma values in a 2^4 row and a 2^2 column passes
    #  the fp16 range at K = 128, so those cases run `scaled`)
    return _case("lowered", cid, variant="scaled" if s["epi"] == L.EPI_GEGLU else "marked", **s)


_BUILDERS = dict(inst=_build_inst, tail=_build_tail, splitk=_build_splitk, feat=_build_feat, conv=_build_conv, c8=_build_c8, tconv=_build_tconv,
                 reswrap=_build_reswrap, stats=_build_stats, twopass=_build_twopass, offset=_build_offset, lowered=_build_lowered)


def build(case):
    return _BUILDERS[case["family"]](case)


# ---- the case list --------------------------------------------------------------------------------------------------------------------------
CASES = []
for _v in ("scaled", "marked"):
    for _K in (384, 64):          # 6 k-tiles: the 4-deep ring wraps; 1: fewer k-tiles than stages
        CASES.append(_case("inst", f"inst-t0w64-N164-K{_K}-{_v}", tile=0, N=164, K=_K, variant=_v))
        CASES.append(_case("inst", f"inst-t0w128-N228-K{_K}-{_v}", tile=0, N=228, K=_K, variant=_v))
        CASES += [_case("inst", f"inst-t{_t}-K{_K}-{_v}", tile=_t, K=_K, variant=_v) for _t in GEMM2_TILES]
    CASES += [_case("tail", f"tail-N{_N}-K{_K}-{_v}", N=_N, K=_K, variant=_v) for _N, _K in ((164, 200), (164, 8), (4, 384))]
# K = 1600: 25 k-tiles as 9 + 9 + 7; K = 1088: 17 as 9 + 8
for _t in (0, 5, 9):
    for _K, _s in ((1600, 3), (1088, 2)):
        for _tk in (False, True):
            CASES.append(_case("splitk", f"splitk-t{_t}-K{_K}-{'tickets' if _tk else 'reduce'}", tile=_t, K=_K, split=_s, tickets=_tk,
                               variant="marked" if _tk else "scaled"))
CASES += [_case("feat", f"feat-t{_t}-{_v}", tile=_t, variant=_v) for _t, _v in ((0, "scaled"), (1, "marked"), (8, "scaled"), (3, "marked"), (12, "scaled"))]
CASES += [_case("conv", f"conv-t{_t}-Cin{_c}", tile=_t, cin=_c, variant="marked") for _t in (0,) + GEMM2_TILES for _c in (64, 128)]
CASES.append(_case("c8", "c8-stem", variant="marked"))
CASES += [_case("tconv", f"tconv-t{_t}", tile=_t, variant="marked") for _t in (0,) + GEMM2_TILES]
# tile 0 splits 18 / 27 k-tiles evenly (kt // 8 splits of 9); a forced gemm2 tile on 2 x its tile count of CUs takes 2 splits: 27 as 14 + 13
CASES += [_case("reswrap", "reswrap-conv-t0", kind="conv", tile=0, cin=64, split=1), _case("reswrap", "reswrap-tconv-t0", kind="tconv", tile=0, cin=128, split=1),
          _case("reswrap", "reswrap-conv-t0-split3", kind="conv", tile=0, cin=192, split=3, variant="marked"),
          _case("reswrap", "reswrap-conv-t5-split2", kind="conv", tile=5, cin=192, split=2, cus=4, variant="marked"),
          _case("reswrap", "reswrap-tconv-t0-split3", kind="tconv", tile=0, cin=576, split=3, variant="marked"),
          _case("reswrap", "reswrap-tconv-t3-split2", kind="tconv", tile=3, cin=576, split=2, cus=2, variant="marked")]
CASES += [_case("stats", f"stats-t{_t}-{_v}", tile=_t, variant=_v, out_lo=_t in (0, 11)) for _t, _v in ((0, "marked"), (8, "scaled"), (11, "marked"), (3, "scaled"))]
CASES += [_case("twopass", "twopass-a_lo", which="a_lo"), _case("twopass", "twopass-weight_lo", which="weight_lo")]
CASES += [_case("offset", f"offset-t{_t}", tile=_t, variant="offset") for _t in (0, 1, 12)]
# the `lowered` family: (tile, tile 0's width, gather, stride, up, i[23], fold, K % 64 != 0, M ragged, N ragged, epilogue, out dtype, activation,
# bias 0 / 1 along N / 2 along M, row bias, residual, residual wrap, hi + lo) — a split-K GEMM with a reduction launch is two entries: its
# slab launch (fold "slab": the epilogue fields say how the slabs are folded, any will do) and the reduction's epilogue on tile 5
_LOWERED_FIELDS = ("tile", "w", "gather", "stride", "up", "i23", "fold", "k_tail", "m_ragged", "n_ragged", "epi", "out", "act", "bias", "rowbias", "res",
                   "res_wrap", "out_lo")
_LOWERED = [
    (0, 128, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (0, 128, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 1, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (0, 128, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (0, 128, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 128, 1, 1, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (0, 128, 1, 1, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (0, 128, 1, 1, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (0, 128, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 1, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 1, 1, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 1, 1, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 2, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 2, 0, 1, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 2, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 128, 2, 0, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 128, 2, 0, 0, 1, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 2, 0, 0, 1, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 3, 1, 0, 0, '-', 1, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 1, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 2, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 1, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, 'i12', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 2, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 1, 0, 1, 0, 0, 0, 1, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 1, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 1, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 1, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 1, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 1, 0, 0, 0, 2, 1, 0, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, 'slab', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 2, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 2, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 2, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 2, 0, 1, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 1, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (0, 64, 2, 0, 0, 1, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 2, 0, 0, 1, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (0, 64, 3, 1, 0, 0, '-', 1, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 3, 1, 0, 0, '-', 1, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (1, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 0, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 1, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 1, 0, 0, 'slab', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 1, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 1, 1, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 2, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (11, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (11, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (11, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (11, 0, 0, 0, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (11, 0, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 1, 1, 1, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 2, 0, 0, 1, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 1, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 2, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 1, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, 'i12', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 0, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (12, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 1, 1, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (12, 0, 0, 0, 0, 0, '-', 0, 1, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (12, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (12, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (12, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (12, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (12, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 1, 0, '-', 0),
    (12, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (12, 0, 1, 2, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (12, 0, 1, 2, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (12, 0, 1, 2, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (12, 0, 1, 2, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, 'i30', 0),
    (12, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (12, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (12, 0, 2, 0, 0, 1, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (12, 0, 2, 0, 0, 1, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (2, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 0, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (2, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (2, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (2, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (2, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (2, 0, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 1, 1, 1, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 1, 1, 1, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 1, 1, 1, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 1, 2, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 1, 2, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (2, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (2, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (2, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 0, 0, 'slab', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 0, 0, 'slab', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 1, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 1, 0, 'slab', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 1, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 2, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 2, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 0, 1, 3, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, 'slab', 0, 1, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, 'slab', 0, 1, 1, 0, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, 'slab', 0, 1, 1, 0, 0, 0, 1, 0, 1, '-', 0),
    (5, 0, 0, 0, 0, 0, 'slab', 0, 1, 1, 0, 0, 0, 1, 0, 1, '-', 1),
    (5, 0, 0, 0, 0, 0, 'slab', 0, 1, 1, 0, 0, 0, 1, 1, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, 'slab', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, 'slab', 0, 1, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, 'slab', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 1, 1, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 1, 1, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 1, 1, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 0, 'slab', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 1, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 1, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 1, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 1, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 1, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (8, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 1, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (8, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 1, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 1, 1, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 1, 1, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 2, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 2, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 1, 0, 1, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 1, 1, 0, 0, 0, 1, 1, 0, '-', 0),
    (9, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
]
# the keys of the requestable lattice (tests/geometry_lattice.py) that the matrix lacks: other frame counts and latents put the same
# epilogues on other tiles and gathers and make rows and columns ragged (profiles/geometry_paths.txt names a witness program for each)
_LOWERED += [
    (0, 128, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 2, 0, 0, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (0, 128, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 128, 1, 2, 0, 1, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 2, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 1, 2, 0, 1, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 128, 2, 0, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 2, 0, 0, 1, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (0, 128, 2, 0, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 128, 3, 1, 0, 0, '-', 1, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (0, 64, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (0, 64, 0, 0, 0, 0, '-', 1, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 1, 1, 0, 0, '-', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (0, 64, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 2, 0, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (0, 64, 2, 0, 0, 1, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (1, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (1, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (1, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (1, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (1, 0, 1, 1, 0, 0, 'slab', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 1, 1, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 1, 1, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 2, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 2, 0, 1, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (1, 0, 1, 2, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (11, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (11, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (11, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (11, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (11, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (11, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (11, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (11, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (11, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (11, 0, 1, 1, 1, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 1, 2, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 1, 2, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 1, 2, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (11, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (11, 0, 2, 0, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (11, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (11, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (11, 0, 2, 0, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (12, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (2, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (2, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (2, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (2, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (2, 0, 1, 1, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 1, 1, 1, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (2, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (2, 0, 2, 0, 0, 1, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 2, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 2, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 0, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 0, 0, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (3, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (3, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (3, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (3, 0, 1, 1, 1, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 1, 1, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 2, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 1, 2, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 2, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 2, 0, 0, 0, '-', 0, 0, 1, 3, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 0, '-', 0, 1, 1, 3, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 0, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 1, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (3, 0, 2, 0, 0, 1, '-', 0, 1, 1, 3, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 1, 0, 1, '-', 1),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 0, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 1),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 0, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 1, 0, 1, '-', 1),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 1, 0, 0, 0, 0, '-', 0),
    (5, 0, 0, 0, 0, 0, '-', 0, 1, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 0, 1, 3, 0, 0, 1, 1, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (5, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 1, 1, 1, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 0, '-', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 1, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 1, 2, 0, 1, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 2, 0, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (5, 0, 2, 0, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (5, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 0, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 1, '-', 0),
    (8, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (8, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 1, 0, '-', 0),
    (8, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (8, 0, 1, 1, 0, 0, '-', 0, 0, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 1, 0, '-', 0),
    (8, 0, 1, 1, 0, 0, '-', 0, 1, 0, 3, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 1, 1, 1, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 1, 1, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 2, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 1, 2, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (8, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (8, 0, 2, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 2, 0, 0, 0, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (8, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (8, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 2, 0, 0, 0, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (8, 0, 2, 0, 0, 1, '-', 0, 0, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (8, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (8, 0, 2, 0, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (8, 0, 2, 0, 0, 1, '-', 0, 1, 0, 3, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 0, 1, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 1, 0, 1, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 0, 0, 0, '-', 0),
    (9, 0, 0, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 0, 0, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 0, 1, 0, 0, 0, 1, 1, 0, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 0, 1, 3, 0, 0, 1, 1, 0, '-', 0),
    (9, 0, 1, 1, 0, 0, '-', 0, 0, 1, 3, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 1, 1, 0, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 0, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 1, 0, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 1, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 1, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 1, 0, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 1, 1, 0, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 2, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 2, 0, 0, '-', 0, 1, 1, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 2, 0, 1, '-', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 2, 0, 1, '-', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 2, 0, 1, 'slab', 0, 0, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 1, 2, 0, 1, 'slab', 0, 1, 0, 0, 1, 0, 1, 0, 0, '-', 0),
    (9, 0, 2, 0, 0, 0, '-', 0, 0, 1, 0, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 2, 0, 0, 0, '-', 0, 0, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 2, 0, 0, 0, '-', 0, 1, 0, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 2, 0, 0, 0, '-', 0, 1, 1, 0, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 2, 0, 0, 1, '-', 0, 0, 1, 0, 1, 0, 1, 0, 1, '-', 0),
    (9, 0, 2, 0, 0, 1, '-', 0, 0, 1, 3, 0, 0, 1, 0, 0, '-', 0),
    (9, 0, 2, 0, 0, 1, '-', 0, 1, 1, 0, 1, 0, 1, 0, 1, '-', 0),
]
CASES += [_lowered_case(_s) for _s in _LOWERED]
assert len({c["id"] for c in CASES}) == len(CASES)
