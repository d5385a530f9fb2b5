"""TEST INFRASTRUCTURE — adversarial inputs for every normalisation path (csrc/norm.hip, the norm epilogues of t2v_kernels.h), a float64
reference, and the case list with the programs that run them.  No test functions here: tests/test_norm_inputs_cpu.py proves on the CPU
what the inputs do (and runs every program through the interpreter), tests/test_gpu_norm_adversarial.py runs the same programs on the
GPU.  Both import CASES / build(), so they cannot drift apart.  Nothing here touches a GPU or imports tests/interp.py: whoever executes a
program hands its arena view (`it`, anything with Interp's `mat`) to `Built.init` / `verify`, and every expected value is `groupnorm_ref`.

Why these inputs.  The other norm tests fill x with scale * randn + const: every (instance, group) block then has the same mean and
variance and every row weighs the same, so statistics taken from the neighbouring block, a row lost at a chunk tail or an inv_n that is
off by a row disappear in one rel-L2 over the tensor.  Here
  distinct  x = mu[i, g] + sigma[i, g] z: sigma a power of two in [1/8, 8] that differs between neighbouring instances and groups, mu
            distinct in [-8, 8] with |mu| <= 8 sigma and alternating sign; z is standardised per block, so mu and sigma ARE the block's
            statistics (LayerNorm: per row);
  marked    distinct, and in every instance the first and the last row each carry a quarter of the block's sum of squares, the rows either
            side of every multiple of 32 (strip, tile, chunk seams) are scaled by 4;
  offset    mean / std = 32 (fp32 inputs) or 8 (fp16 inputs) in every block, sigma as above.
Inputs are rounded to the input dtype before the reference sees them.  All errors are one rel-L2 per block (`block_rel_l2`); asserts are on
the maximum over blocks.

Fencing.  Every tensor a norm reads or writes is a window of a larger allocation: rows in front and behind and 8 columns to the right
(ld = C + 8) are NaN, outputs are NaN-filled, and `verify` wants every window finite and every fence element still NaN."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd.program import NULL, Program, Ref, TShardSpec

TOL_F16 = 1e-3          # fp16 output against an explicit reference: the suite's figure for norms
TOL_HILO = 2e-5         # hi + lo / fp32 results: the suite's figure
TOL_ROUNDED = 4e-4      # the float64 reference rounded to fp16
EPS = 1e-5
GROUPS = 32
NAN = float("nan")
TD = {"f16": torch.float16, "f32": torch.float32}
PAD_ROWS, PAD_COLS = 3, 8


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------
def _silu(y):
    return y * torch.sigmoid(y)


def group_sums(x, n_inst, groups):
    """s1, s2 [n_inst, groups] (float64 sums / sums of squares) and n = rows * cpg."""
    C = x.shape[1]
    xv = x.double().view(n_inst, -1, groups, C // groups)
    return xv.sum(dim=(1, 3)), (xv * xv).sum(dim=(1, 3)), xv.shape[1] * xv.shape[3]


def mean_var_of(s1, s2, n):
    mean = s1 / n
    return mean, (s2 / n - mean * mean).clamp_min(0.0)


def groupnorm_ref(x, gamma, beta, n_inst, groups, eps, silu, mean_var=None):
    """GroupNorm (+ SiLU) of x [n_inst * rows, C] (channels last) in float64, written out: per (instance, group) the mean and the biased
    variance over rows x C / groups, (x - mean) / sqrt(var + eps) * gamma + beta.  mean_var = (mean, var) [n_inst, groups] replaces the
    statistics (the mutations of tests/test_norm_inputs_cpu.py)."""
    M, C = x.shape
    xv = x.double().view(n_inst, M // n_inst, groups, C // groups)
    if mean_var is None:
        mean = xv.mean(dim=(1, 3))
        var = ((xv - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    else:
        mean, var = mean_var
    y = (xv - mean[:, None, :, None]) / torch.sqrt(var[:, None, :, None] + eps)
    y = y.reshape(M, C) * gamma.double() + beta.double()
    return _silu(y) if silu else y


def layernorm_ref(x, gamma, beta, eps, mean_var=None):
    """LayerNorm of the rows of x [M, C] in float64: a GroupNorm of M one-row instances with one group."""
    return groupnorm_ref(x, gamma, beta, x.shape[0], 1, eps, False, mean_var)


def blocks(y, n_inst, groups):
    """[n_inst * rows, C] -> [n_inst, groups, rows * cpg]: one statistics block per (instance, group)."""
    M, C = y.shape
    return y.reshape(n_inst, M // n_inst, groups, C // groups).permute(0, 2, 1, 3).reshape(n_inst, groups, -1)


def block_rel_l2(got, ref):
    """One rel-L2 per block: got, ref [..., n] -> [...]."""
    got, ref = got.double(), ref.double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)


def block_err(got, ref, n_inst, groups):
    return block_rel_l2(blocks(got, n_inst, groups), blocks(ref, n_inst, groups))


def torch_block_err(x, gamma, beta, n_inst, groups, eps, silu, ref):
    """e_torch: the per-block error of torch.nn.functional.group_norm in fp32 on the CPU (the class the project is judged against)."""
    M, C = x.shape
    y = F.group_norm(x.float().view(n_inst, M // n_inst, C).permute(0, 2, 1).contiguous(), groups, gamma.float(), beta.float(), eps)
    y = y.permute(0, 2, 1).reshape(M, C)
    return block_err(F.silu(y) if silu else y, ref, n_inst, groups)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
def block_params(variant, n_inst, groups, dtype, seed):
    """mu, sigma [n_inst, groups] (float64)."""
    i, g = torch.arange(n_inst)[:, None], torch.arange(groups)[None, :]
    sigma = torch.exp2((((g + 3 * i + seed) % 7) - 3).double())              # neighbours along i and along g differ
    if variant == "offset":
        return (32.0 if dtype == "f32" else 8.0) * sigma, sigma
    nb = n_inst * groups
    gen = torch.Generator().manual_seed(seed)
    frac = torch.linspace(0.25, 1.0, nb, dtype=torch.float64)[torch.randperm(nb, generator=gen)].view(n_inst, groups)
    sign = (1 - 2 * ((i + g) % 2)).double()
    return sign * frac * 8.0 * sigma.clamp(max=1.0), sigma


def row_scales(variant, rows):
    s = torch.ones(rows, dtype=torch.float64)
    if variant == "marked" and rows >= 3:
        for k in range(32, rows, 32):
            s[k - 1] = s[k] = 4.0
        s[0] = s[-1] = math.sqrt(float((s[1:-1] ** 2).sum()) / 2.0)          # a quarter of the sum of squares each
    return s


def gn_input(variant, n_inst, rows, C, groups, dtype, seed):
    """x [n_inst * rows, C] in float64, representable in `dtype`."""
    assert variant in ("distinct", "marked", "offset")
    mu, sigma = block_params(variant, n_inst, groups, dtype, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    cpg = C // groups
    z = torch.randn(n_inst, rows, groups, cpg, generator=gen, dtype=torch.float64) * row_scales(variant, rows)[None, :, None, None]
    if variant == "marked" and rows >= 3 and cpg >= 2:
        # exactly: the first and the last row sum to zero within a group and carry n / 4 of the block's sum of squares each, the rows between
        # them n / 2 around a zero mean — block mean 0, variance 1
        n = rows * cpg
        for r in (0, rows - 1):
            e = z[:, r] - z[:, r].mean(dim=-1, keepdim=True)
            z[:, r] = e * torch.sqrt(n / 4.0 / (e * e).sum(dim=-1, keepdim=True))
        mid = z[:, 1:-1] - z[:, 1:-1].mean(dim=(1, 3), keepdim=True)
        z[:, 1:-1] = mid * torch.sqrt(n / 2.0 / (mid * mid).sum(dim=(1, 3), keepdim=True))
    elif rows * cpg >= 2:
        z = (z - z.mean(dim=(1, 3), keepdim=True)) / z.std(dim=(1, 3), unbiased=False, keepdim=True)
    x = mu[:, None, :, None] + sigma[:, None, :, None] * z
    return x.reshape(n_inst * rows, C).to(TD[dtype]).double()


def ln_input(variant, M, C, seed):
    """Rows for a LayerNorm (fp32 input): mu / sigma per row."""
    return gn_input(variant, M, 1, C, 1, "f32", seed)


def affine(C, seed):
    g = torch.Generator().manual_seed(seed + 2)
    return 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


# ---- mirrors of the launchers' chunking (csrc/norm.hip coop_chunking, program.Program.groupnorm) -----------------------------------------
GNC_THREADS = 512
COOP_KRS = (4, 8, 12, 16, 20)
SPLITK_KRS = (1, 2, 4, 8, 12, 16, 20)


def coop_chunking(rows, n_inst, cv, ncu, max_chunk, kr_list):
    """-> (kr, rc, nchunk): the first kr whose grid of n_inst * nchunk workgroups is at most one per CU, nchunk <= max_chunk; (0, 0, 0)."""
    for kr in kr_list:
        rc = (GNC_THREADS // cv) * kr
        nchunk = -(-rows // rc)
        if n_inst * nchunk <= ncu and nchunk <= max_chunk:
            return kr, rc, nchunk
    return 0, 0, 0


def stats_blocks(rows, n_inst, target_cus=256):
    """nblk of Program.groupnorm: the rows per statistics workgroup double from 4 until the grid is within 4 workgroups per CU."""
    rpb = 4
    while n_inst * -(-rows // rpb) > 4 * target_cus:
        rpb *= 2
    return -(-rows // rpb)


def rows_for_kr(target, n_inst, C, ncu, kr_list, standalone):
    """The smallest row count at which the launcher picks `target` rows per thread (every smaller kr overflows the device), plus 5."""
    cv = C // 8
    pick = lambda r: coop_chunking(r, n_inst, cv, ncu, stats_blocks(r, n_inst) if standalone else 1 << 30, kr_list)[0]
    rows = 1
    while pick(rows) != target:
        rows += 1
        assert rows < 1 << 16, (target, n_inst, C, ncu)
    assert pick(rows + 5) == target
    return rows + 5


# ---- programs -----------------------------------------------------------------------------------------------------------------------------
class Built:
    """A case's program, weights, initial arena contents, fences and expectations."""

    def __init__(self, case):
        self.case = case
        self.P = Program()
        self.w = {}
        self.fences = []        # (allocation, r0, r1, c1): rows r0 .. r1 - 1 x columns 0 .. c1 - 1 are the window, the rest stays NaN
        self.sets = []          # (window, tensor) written before the run
        self.outs = []          # dict(name, hi, lo, ref, n_inst, groups, tol): norm outputs
        self.exact = []         # (name, window, expected tensor): bit-equal
        self.probs = []         # dict(X, gamma, beta, n_inst, groups, silu, tol, parts): the norm problems, for the CPU proofs
        self.path = ""          # what the op records were asserted to say
        self.kr = None

    def fenced(self, rows, cols, dtype, window=None):
        assert cols % 8 == 0
        big = self.P.alloc(rows + 2 * PAD_ROWS, cols + PAD_COLS, dtype)
        r0, r1 = (0, rows) if window is None else window
        self.fences.append((big, PAD_ROWS + r0, PAD_ROWS + r1, cols))
        return big.row_slice(PAD_ROWS, PAD_ROWS + rows).col_slice(0, cols)

    def put(self, win, t):
        assert (win.rows, win.cols) == tuple(t.shape), (win.rows, win.cols, t.shape)
        self.sets.append((win, t))

    def weight(self, name, t):
        self.w[name] = t
        return Ref("weight", 0, name)

    def init(self, it):
        for big, _, _, _ in self.fences:
            it.mat(big.ref, big.rows, big.ld, big.ld, TD[big.dtype], {}).fill_(NAN)
        for win, t in self.sets:
            it.mat(win.ref, win.rows, win.cols, win.ld, TD[win.dtype], {}).copy_(t.to(TD[win.dtype]))

    def hilo_tol(self, lo, X, gamma, beta, n_inst, groups, silu, full):
        """Per-block bound of hi + lo (None without a low-order output) and, on `offset` rows, the worst e_torch behind it."""
        if not lo:
            return None, None
        tol = torch.full((n_inst, groups), TOL_HILO, dtype=torch.float64)
        if self.case["variant"] != "offset":
            return tol, None
        et = torch_block_err(X, gamma, beta, n_inst, groups, EPS, silu, full)      # another fp32 summation order (up to 20 rows per lane): 4 x
        return torch.maximum(tol, 4.0 * et), float(et.max())

    def expect(self, name, hi, lo, X, gamma, beta, n_inst, groups, silu, parts=None):
        """Register a norm output (window `hi`, low-order window `lo` or None) of input X."""
        full = groupnorm_ref(X, gamma, beta, n_inst, groups, EPS, silu)
        tol, et = self.hilo_tol(lo is not None, X, gamma, beta, n_inst, groups, silu, full)
        self.outs.append(dict(name=name, hi=hi, lo=lo, ref=full, n_inst=n_inst, groups=groups, tol=tol, e_torch=et))
        self.probs.append(dict(name=name, X=X, gamma=gamma, beta=beta, n_inst=n_inst, groups=groups, silu=silu,
                               tol=TOL_F16 if lo is None else TOL_HILO, parts=parts))


def _rd(it, win):
    return it.mat(win.ref, win.rows, win.cols, win.ld, TD[win.dtype], {}).clone()


def verify(it, b):
    """Fences, bit-equal side outputs and per-block errors of a finished run; -> dict(hi, hilo, e_torch): maxima over blocks and outputs."""
    tag = b.case["id"]
    for big, r0, r1, c1 in b.fences:
        full = it.mat(big.ref, big.rows, big.ld, big.ld, TD[big.dtype], {}).clone()
        assert torch.isfinite(full[r0:r1, :c1]).all(), f"{tag}: non-finite values inside a window"
        full[r0:r1, :c1] = NAN
        assert torch.isnan(full).all(), f"{tag}: {int((~torch.isnan(full)).sum())} fence elements written"
    for name, win, want in b.exact:
        assert torch.equal(_rd(it, win), want.to(TD[win.dtype])), f"{tag}: {name} is not bit-equal"
    figs = dict(hi=0.0, hilo=None, e_torch=None)
    for o in b.outs:
        hi = _rd(it, o["hi"]).double()
        assert hi.shape == o["ref"].shape, (tag, o["name"], hi.shape, o["ref"].shape)
        e = block_err(hi, o["ref"], o["n_inst"], o["groups"])
        figs["hi"] = max(figs["hi"], float(e.max()))
        assert float(e.max()) < TOL_F16, (tag, o["name"], "hi", float(e.max()))
        if o["lo"] is not None:
            e2 = block_err(hi + _rd(it, o["lo"]).double(), o["ref"], o["n_inst"], o["groups"])
            figs["hilo"] = max(figs["hilo"] or 0.0, float(e2.max()))
            if o["e_torch"] is not None:
                figs["e_torch"] = max(figs["e_torch"] or 0.0, o["e_torch"])
            assert bool((e2 < o["tol"]).all()), (tag, o["name"], "hi+lo", float(e2.max()), float(o["tol"].max()))
            assert float(e2.max()) < float(e.max()), (tag, o["name"], "hi + lo is no closer than hi", float(e2.max()), float(e.max()))
    return figs


def figures_line(b, figs):
    f = lambda v: "-" if v is None else f"{v:.2e}"
    return f"NORMADV {b.case['id']}: path [{b.path}] KR {b.kr if b.kr else '-'} hi {f(figs['hi'])} hi+lo {f(figs['hilo'])} e_torch {f(figs['e_torch'])}"


# -- stand-alone OP_GROUPNORM ---------------------------------------------------------------------------------------------------------------
def _gn_case(form, n_inst, rows, C, dt, variant, **kw):
    c = dict(family="gn", id=f"gn-{form}-{n_inst}x{rows}x{C}-{dt}-{variant}", form=form, n_inst=n_inst, rows=rows, C=C, dt=dt, variant=variant,
             barrier=False, kr=None, seed=100 + n_inst + rows + C)
    c.update(kw)
    return c


def _build_gn(c, ncu):
    b = Built(c)
    P, form, n_inst, C, dt = b.P, c["form"], c["n_inst"], c["C"], c["dt"]
    rows = c["rows"] if c["kr"] is None else rows_for_kr(c["kr"], n_inst, C, ncu, COOP_KRS, True)
    P.gn_coop = form == "cooperative"
    P.gn_fused_slice_bytes = 1 << 30 if form == "single_launch" else 0
    P.gn_fused_total_bytes = 1 << 30
    M = n_inst * rows
    X = gn_input(c["variant"], n_inst, rows, C, GROUPS, dt, c["seed"])
    gamma, beta = affine(C, c["seed"])
    g, be = b.weight("g", gamma), b.weight("be", beta)
    x = b.fenced(M, C, dt)
    b.put(x, X)
    # every buffer before the first op: an op's scratch is freed when it is emitted, a later allocation would land on it
    combos = [(True, "lo")] if c["kr"] is not None else [(True, "lo"), (False, "lo"), (True, "cast"), (False, "cast")]
    bufs = []
    for silu, second in combos:
        if second == "lo":
            bufs.append((b.fenced(M, 2 * C, "f16"), None))
        else:
            bufs.append((b.fenced(M, C, "f16"), b.fenced(M, 2 * C, "f16")))
    for (silu, second), (out, cast) in zip(combos, bufs):
        name = f"{'silu' if silu else 'plain'}-{second}"
        if second == "lo":
            op = P.groupnorm(name, x, g, be, out.col_slice(0, C), n_inst=n_inst, eps=EPS, silu=silu, lo=True)
            b.expect(name, out.col_slice(0, C), out.col_slice(C, 2 * C), X, gamma, beta, n_inst, GROUPS, silu)
            assert op.i[16] == 1 and op.p[8].space == "null"
        else:
            op = P.groupnorm(name, x, g, be, out, n_inst=n_inst, eps=EPS, silu=silu, cast=cast, cast_lo=True)
            b.expect(name, out, None, X, gamma, beta, n_inst, GROUPS, silu)
            hi = X.half()
            b.exact.append((name + " cast", cast.col_slice(0, C), hi))
            b.exact.append((name + " cast lo", cast.col_slice(C, 2 * C), (X.float() - hi.float()).half()))
            assert op.i[16] == 0 and op.p[8].space == "arena" and op.i[20] == C
        assert op.kind == L.OP_GROUPNORM and op.i[8] == 0 and op.i[12] == (form == "single_launch") and op.i[15] == (form == "cooperative")
        if form == "cooperative":
            assert op.p[7].space == "arena" and op.i[18] > 0            # tagged records in the program's exchange region
            if c["barrier"]:
                op.p[7], op.i[18] = NULL, 0                              # grid-barrier mode: partials in the op's own scratch
        if c["kr"] is not None:
            nblk = -(-rows // op.i[11])
            kr, rc, nchunk = coop_chunking(rows, n_inst, C // 8, ncu, nblk, COOP_KRS)
            assert kr == c["kr"] and rows % rc != 0, (kr, rows, rc)
            b.kr = kr
    assert len(P.ops) == len(combos)
    b.path = f"OP_GROUPNORM i[8]=0 i[12]={int(form == 'single_launch')} i[15]={int(form == 'cooperative')}" + \
             (" barrier" if c["barrier"] else " records" if form == "cooperative" else "") + f" rows={rows}"
    return b


# -- the GEMM in front of a fused / strip-fed norm: an identity weight, so that its result IS the designed tensor ----------------------------
def _identity_gemm(b, name, kind, X, out_dt, *, geo=None, k_extra=0, res=True, **kw):
    """out [M, C] = X exactly: A = fp16(X), W = identity (on the centre tap of a convolution; `k_extra` more operand columns meet zero
    weights), and — fp32 results — a residual that carries X - fp16(X).  Returns (op, y window)."""
    P = b.P
    M, C = X.shape
    hi = X.half()
    eye = torch.eye(C)
    if kind == "conv":
        w4 = torch.zeros(C, C, 3, 3)
        w4[:, :, 1, 1] = eye
        W, K, gather, conv = pk.conv3x3(w4).half(), 9 * C, L.GATHER_CONV3X3, dict(Hin=geo[1], Win=geo[2], Cin=C, stride=1, up=0, Hout=geo[1], Wout=geo[2])
    elif kind == "tconv":
        w5 = torch.zeros(C, C, 3, 1, 1)
        w5[:, :, 1, 0, 0] = eye
        W, K, gather, conv = pk.tconv3(w5).half(), 3 * C, L.GATHER_TCONV3, dict(F=geo[0], HW=geo[1] * geo[2], Cin=C)
    else:
        W, K, gather, conv = torch.cat([eye, torch.zeros(C, k_extra)], dim=1).half(), C + k_extra, L.GATHER_PLAIN, None
    a = P.alloc(M, C + k_extra, "f16")
    A = hi if not k_extra else torch.cat([hi, torch.randn(M, k_extra, generator=torch.Generator().manual_seed(7)).half()], dim=1)
    b.put(a, A)
    r = None
    if out_dt == "f32" and res:
        r = P.alloc(M, C, "f32")
        b.put(r, X.float() - hi.float())
    y = b.fenced(M, C, out_dt, window=(0, 0) if kw.pop("dead", False) else None)
    op = P.gemm(name, a, b.weight(name + ".w", W), C, K, y, gather=gather, conv=conv, residual=r, **kw)
    return op, y


def _case(family, id, variant, **kw):
    c = dict(family=family, id=f"{id}-{variant}", variant=variant)
    c.update(kw)
    return c


# -- strips, phase 3 ---------------------------------------------------------------------------------------------------------------------
def _build_strips(c, ncu):
    b = Built(c)
    n_inst, rows, C = c["n_inst"], c["rows"], c["C"]
    M = n_inst * rows
    X = gn_input(c["variant"], n_inst, rows, C, GROUPS, c.get("dt", "f32"), c["seed"])
    gamma, beta = affine(C, c["seed"])
    # The strips are fp32 sums of x and x^2 over 32 rows (the ABI of T2V_EPI_STATS), so the single-pass variance they give carries at least
    # 2^-24 (1 + (mean / std)^2) = 6e-5 at mean / std = 32, 3e-5 in the output, whatever the fold does: beyond the hi + lo figure by the
    # number format alone.  The `offset` rows therefore run without a low-order output and are held to the fp16 figure.
    lo, dt = c.get("lo", c["variant"] != "offset"), c.get("dt", "f32")
    st = b.P.alloc(M // 32, 2 * C, "f32")
    out = b.fenced(M, 2 * C if lo else C, "f16")
    gop, y = _identity_gemm(b, "l", "plain", X, dt, stats=st, allow_splitk=False)
    assert gop.i[16] == L.EPI_STATS and gop.meta["stats"] == 1 and gop.meta["split"] == 1
    b.exact.append(("stored x", y, X.float() if dt == "f32" else X.half()))
    op = b.P.groupnorm("gn", y, b.weight("g", gamma), b.weight("be", beta), out.col_slice(0, C), n_inst=n_inst, eps=EPS, silu=True, lo=lo, stats=st)
    wide = rows // 32 * (C // GROUPS) > 1024
    assert op.i[8] == 3 and op.p[6].space == "arena" and op.i[17] == C and wide == c["wide"] and len(b.P.ops) == 2
    b.expect("gn", out.col_slice(0, C), out.col_slice(C, 2 * C) if lo else None, X, gamma, beta, n_inst, GROUPS, True)
    b.path = f"OP_GROUPNORM i[8]=3 behind EPI_STATS, {'workgroup' if wide else 'wave'} fold"
    return b


# -- sharded phases 1 / 2 ----------------------------------------------------------------------------------------------------------------
def _build_shard(c, ncu):
    b = Built(c)
    P, C, fr, size, total, dt = b.P, c["C"], c["frame_rows"], c["size"], c["frames"], c["dt"]
    P.target_cus = c.get("target_cus", 1)          # 1: several statistics workgroups per part
    specs = [TShardSpec.make(total, size, q) for q in range(size)]
    prow = [s.frames * fr for s in specs]
    assert len(set(prow)) > 1, "the slices must be uneven"
    Xp = [gn_input(c["variant"], 1, prow[q], C, GROUPS, dt, c["seed"] + 10 * q) for q in range(size)]      # own mu / sigma per part
    X = torch.cat(Xp)
    if c["variant"] == "marked":
        # the clip's first and last row against the CLIP's statistics (the parts' own marks weigh little once the parts' means differ)
        xv = X.view(sum(prow), GROUPS, C // GROUPS).clone()
        m = xv.mean(dim=(0, 2), keepdim=True)
        d = xv - m
        others = (d[1:-1] ** 2).sum(dim=(0, 2))
        for r in (0, -1):
            xv[r] = m[0] + d[r] * torch.sqrt(others / 2.0 / (d[r] ** 2).sum(-1))[:, None]
        X = xv.reshape(sum(prow), C).to(TD[dt]).double()
        Xp = list(X.split(prow))
    gamma, beta = affine(C, c["seed"])
    g, be = b.weight("g", gamma), b.weight("be", beta)
    halo, strips, lo, silu = c["halo"], c["strips"], c.get("lo", not c["halo"]), c.get("silu", True)
    xs, outs, sts, raws = [], [], [], []
    off = 0
    for q in range(size):
        before, after = (fr if q > 0 else 0, fr if q + 1 < size else 0) if halo else (0, 0)
        if strips:
            sts.append(P.alloc(prow[q] // 32, 2 * C, "f32"))
            outs.append(b.fenced(prow[q], 2 * C if lo else C, "f16"))
            gop, y = _identity_gemm(b, f"l{q}", "plain", Xp[q], dt, stats=sts[q], allow_splitk=False)
            assert gop.i[16] == L.EPI_STATS
            xs.append(y)
        elif halo:
            raw = b.fenced(prow[q] + 2 * fr, C, dt, window=(fr - before, fr + prow[q] + after))
            raws.append(raw)
            b.put(raw.row_slice(fr - before, fr + prow[q] + after), X[off - before: off + prow[q] + after])
            xs.append(raw.row_slice(fr, fr + prow[q]))
            outs.append(b.fenced(prow[q] + 2 * fr, C, "f16", window=(fr - before, fr + prow[q] + after)))
        else:
            xs.append(b.fenced(prow[q], C, dt))
            b.put(xs[q], Xp[q])
            outs.append(b.fenced(prow[q], 2 * C if lo else C, "f16"))
        off += prow[q]
    for q in range(size):
        o = outs[q].row_slice(fr, fr + prow[q]) if halo else outs[q].col_slice(0, C)
        P.groupnorm(f"p{q}", xs[q], g, be, o, n_inst=1, eps=EPS, silu=silu, shard=specs[q], lo=lo, stats=sts[q] if strips else None,
                    halo_raw=raws[q] if halo else None)
    gn = [op for op in P.ops if op.kind == L.OP_GROUPNORM]          # p0.stats, p0.apply, p1.stats, ...
    assert len(gn) == 2 * size
    scratch = gn[2 * max(range(size), key=lambda q: prow[q])].p[4]      # one scratch for all parts: the longest part's
    for op in gn:
        op.p[4] = scratch
    st_ops, ap_ops = gn[0::2], gn[1::2]
    off = 0
    for q in range(size):
        before, after = (fr if q > 0 else 0, fr if q + 1 < size else 0) if halo else (0, 0)
        assert st_ops[q].i[8] == 1 and ap_ops[q].i[8] == 2 and st_ops[q].i[9] == size and st_ops[q].i[10] == q and ap_ops[q].i[14] == sum(prow)
        assert (st_ops[q].p[6].space == "arena") == strips and (ap_ops[q].i[21], ap_ops[q].i[22]) == (before, after)
        sl = slice(off - before, off + prow[q] + after)
        hi = outs[q].row_slice(fr - before, fr + prow[q] + after) if halo else outs[q].col_slice(0, C)
        full = groupnorm_ref(X, gamma, beta, 1, GROUPS, EPS, silu)
        tol, et = b.hilo_tol(lo, X, gamma, beta, 1, GROUPS, silu, full)
        b.outs.append(dict(name=f"p{q}", hi=hi, lo=outs[q].col_slice(C, 2 * C) if lo else None, ref=full[sl], n_inst=1, groups=GROUPS, tol=tol, e_torch=et))
        off += prow[q]
    b.probs.append(dict(name="clip", X=X, gamma=gamma, beta=beta, n_inst=1, groups=GROUPS, silu=silu, tol=TOL_HILO if lo else TOL_F16, parts=prow))
    gemms = [op for op in P.ops if op.kind == L.OP_GEMM]
    P.ops = gemms + st_ops + ap_ops                                   # the collectives are the test's: one scratch, every part's slot filled
    b.path = f"OP_GROUPNORM i[8]=1 x{size} then i[8]=2 x{size}" + (" strips (p[6])" if strips else "") + (" halo i[21]/i[22]" if halo else "")
    return b


# -- T2V_EPI_GN ----------------------------------------------------------------------------------------------------------------------------
_EPI_BM = {8: 192, 11: 128, 3: 128, 5: 128, 0: 128}


def _build_epi(c, ncu):
    b = Built(c)
    P, kind, tile, C, dead, lo = b.P, c["kind"], c["tile"], c["C"], c["dead"], c["lo"]
    B, Fr, H, W = c["geo"]
    M = B * Fr * H * W
    n_inst = B * Fr if c["per_frame"] else B
    rows = M // n_inst
    P.force_tile = tile
    X = gn_input(c["variant"], n_inst, rows, C, GROUPS, "f16" if dead else "f32", c["seed"])
    gamma, beta = affine(C, c["seed"])
    full = b.fenced(M, 2 * C if lo else C, "f16")
    op, y = _identity_gemm(b, "g", kind, X, "f16" if dead else "f32", geo=(Fr, H, W), allow_splitk=False, dead=dead)
    assert op.meta["tile"] == tile and op.meta["split"] == 1
    out = full.col_slice(0, C)
    fused = P.groupnorm("gn", y, b.weight("g", gamma), b.weight("be", beta), out, n_inst=n_inst, eps=EPS, silu=True, lo=lo,
                        gb=b.weight("gb", torch.cat([gamma, beta])), x_dead=dead)
    assert fused is op and op.i[16] == L.EPI_GN and len(P.ops) == 1, "the norm did not become the GEMM's epilogue"
    assert (op.i[24], op.i[27], op.i[28], op.i[29], op.i[22]) == (rows, int(lo), GROUPS, int(dead), tile)
    bm = _EPI_BM[tile]
    assert c["seam"] == ("half" if 2 * rows == bm else "whole" if rows % bm == 0 else "straddle")
    if not dead:
        b.exact.append(("stored x", y, X.float()))
    b.expect("gn", out, full.col_slice(C, 2 * C) if lo else None, X, gamma, beta, n_inst, GROUPS, True)
    b.path = f"EPI_GN tile {tile} {kind} rows={rows} ({c['seam']}) dead={int(dead)} lo={int(lo)}"
    return b


# -- splitk_gn_kernel ------------------------------------------------------------------------------------------------------------------------
def _build_splitk(c, ncu):
    b = Built(c)
    P, C, n_inst, dead, lo = b.P, c["C"], c["n_inst"], c["dead"], c["lo"]
    # KR = 1 is the list's first entry: any short instance runs it (101 rows); otherwise the smallest count + 5, and one row more where
    # that is a whole number of chunks (the last chunk must be ragged)
    rows = 101 if c["kr"] == SPLITK_KRS[0] else rows_for_kr(c["kr"], n_inst, C, ncu, SPLITK_KRS, False)
    if rows % coop_chunking(rows, n_inst, C // 8, ncu, 1 << 30, SPLITK_KRS)[1] == 0:
        rows += 1
    M = n_inst * rows
    P.force_tile = 5
    X = gn_input(c["variant"], n_inst, rows, C, GROUPS, "f16" if dead else "f32", c["seed"])
    gamma, beta = affine(C, c["seed"])
    full = b.fenced(M, 2 * C if lo else C, "f16")
    op, y = _identity_gemm(b, "g", "plain", X, "f16" if dead else "f32", k_extra=2048 - C, dead=dead)
    assert op.meta["split"] > 1, op.meta
    out = full.col_slice(0, C)
    fused = P.groupnorm("gn", y, b.weight("g", gamma), b.weight("be", beta), out, n_inst=n_inst, eps=EPS, silu=True, lo=lo,
                        gb=b.weight("gb", torch.cat([gamma, beta])), x_dead=dead)
    assert fused is op and op.i[16] == L.EPI_GN and op.meta["split"] > 1 and len(P.ops) == 1
    kr, rc, nchunk = coop_chunking(rows, n_inst, C // 8, ncu, 1 << 30, SPLITK_KRS)
    assert kr == c["kr"] and rows % rc != 0
    b.kr = kr
    if not dead:
        b.exact.append(("stored x", y, X.float()))
    b.expect("gn", out, full.col_slice(C, 2 * C) if lo else None, X, gamma, beta, n_inst, GROUPS, True)
    b.path = f"EPI_GN split={op.meta['split']} rows={rows} dead={int(dead)} lo={int(lo)}"
    return b


# -- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
def _build_ln(c, ncu):
    b = Built(c)
    M, C = c["M"], c["C"]
    X = ln_input(c["variant"], M, C, c["seed"])
    gamma, beta = affine(C, c["seed"])
    x, out = b.fenced(M, C, "f32"), b.fenced(M, C, "f16")
    b.put(x, X)
    op = b.P.layernorm("ln", x, b.weight("g", gamma), b.weight("be", beta), out, EPS)
    op.i[4] = c["cap"]
    assert op.kind == L.OP_LAYERNORM and (op.i[0], op.i[1]) == (M, C) and (c["cap"] == 0 or -(-M // 4) > c["cap"])
    b.expect("ln", out, None, X, gamma, beta, M, 1, False)
    b.path = f"OP_LAYERNORM C={C} i[4]={c['cap']}" + (" grid-stride" if c["cap"] else "")
    return b


def _build_lnfused(c, ncu):
    b = Built(c)
    M, N, tile = c["M"], c["N"], c["tile"]
    b.P.force_tile = tile
    X = ln_input(c["variant"], M, N, c["seed"])
    gamma, beta = affine(N, c["seed"])
    ln_out = b.fenced(M, N, "f16")
    op, y = _identity_gemm(b, "g", "plain", X, "f32", allow_splitk=False,
                           ln=(b.weight("gb", torch.cat([gamma, beta])), b.weight("g", gamma), b.weight("be", beta), ln_out, EPS))
    assert op.i[22] == tile and op.i[8] == c["mode"] and len(b.P.ops) == 1, "the LayerNorm did not become the GEMM's epilogue"
    b.exact.append(("stored x", y, X.float()))
    b.expect("ln", ln_out, None, X, gamma, beta, M, 1, False)
    b.path = f"GEMM tile {tile} i[8]={c['mode']} ({'across column tiles' if c['mode'] == 2 else 'whole rows'}) N={N}"
    return b


# -- `lowered`: one case per code path that a lowered program takes and no case above has (tests/record_paths.py is the key, ---------------
# -- tests/test_record_paths_cpu.py the check; profiles/lowered_paths.txt names a deployed op for each) ------------------------------------
def _build_lowered_gn(c, ncu):
    """Stand-alone OP_GROUPNORM, phase 0, ONE record: launch form x input dtype x SiLU x low-order image x cast output (x its low-order
    image) x rows per thread of the cooperative kernel x tagged records / grid barrier x the column loop (C = 2560: more than 256 column
    vectors).  C = 640 otherwise (the single-launch kernel needs C / groups % 4 == 0).  The cooperative cases cannot be smaller: the launcher
    picks KR as the first count whose grid fits the device, so KR > 4 needs a tensor that overflows the device at every smaller count
    (256 workgroups x 512 threads x KR rows x 8 channels).  `coop-fallback`: the record asks for the cooperative kernel and no KR fits —
    two statistics blocks per instance (the lowering planning for one compute unit) against 485 rows = three chunks at KR = 20."""
    b = Built(c)
    P, form, dt, silu, lo, cast, barrier = b.P, c["form"], c["dt"], c["silu"], c["lo"], c["cast"], c["barrier"]
    C = 2560 if c["cols_loop"] else 640
    n_inst = 64 if (form == "cooperative" and not c["cols_loop"]) else 2
    rows = 101
    if form == "cooperative":
        rows = rows_for_kr(c["kr"], n_inst, C, ncu, COOP_KRS, True)
    elif form == "coop-fallback":
        P.target_cus, rows = 1, 485
    elif form == "coop-fallback-one-block":
        # more instances than compute units: no KR gives a grid of one workgroup per CU (norm.hip coop_chunking), and an instance of 4 rows is
        # ONE statistics block of the smallest size (Program.groupnorm: 4 rows), so gn_stats_kernel finalises in place (norm.hip:893 g1) —
        # the per-frame norms of a 250-frame clip at the coarsest level
        n_inst, rows = ncu + 1, 4
    P.gn_coop = form in ("cooperative", "coop-fallback", "coop-fallback-one-block")
    P.gn_fused_slice_bytes = 1 << 30 if form == "single_launch" else 0
    P.gn_fused_total_bytes = 1 << 30
    M = n_inst * rows
    X = gn_input(c["variant"], n_inst, rows, C, GROUPS, dt, c["seed"])
    gamma, beta = affine(C, c["seed"])
    x = b.fenced(M, C, dt)
    b.put(x, X)
    out = b.fenced(M, 2 * C if lo else C, "f16")
    cbuf = b.fenced(M, 2 * C if cast == 2 else C, "f16") if cast else None
    op = P.groupnorm("gn", x, b.weight("g", gamma), b.weight("be", beta), out.col_slice(0, C), n_inst=n_inst, eps=EPS, silu=silu, lo=lo, cast=cbuf,
                     cast_lo=cast == 2)
    assert len(P.ops) == 1 and op.kind == L.OP_GROUPNORM and op.i[8] == 0 and op.i[12] == (form == "single_launch") and op.i[15] == int(P.gn_coop)
    assert op.i[16] == int(lo) and (op.p[8].space == "arena") == bool(cast) and (op.i[20] != 0) == (cast == 2)
    nblk = -(-rows // op.i[11])
    kr = coop_chunking(rows, n_inst, C // 8, ncu, nblk, COOP_KRS)[0] if P.gn_coop else 0
    assert kr == (c["kr"] if form == "cooperative" else 0), (kr, rows, nblk)
    assert form != "coop-fallback-one-block" or nblk == 1, (rows, nblk)
    if form == "cooperative":
        assert op.p[7].space == "arena" and op.i[18] > 0
        if barrier:
            op.p[7], op.i[18] = NULL, 0
        b.kr = kr
    b.expect("gn", out.col_slice(0, C), out.col_slice(C, 2 * C) if lo else None, X, gamma, beta, n_inst, GROUPS, silu)
    if cast:
        hi = X.half()
        b.exact.append(("cast", cbuf.col_slice(0, C), hi))
        if cast == 2:
            b.exact.append(("cast lo", cbuf.col_slice(C, 2 * C), (X.float() - hi.float()).half()))
    b.path = f"OP_GROUPNORM i[8]=0 {form} rows={rows} C={C} {dt} silu={int(silu)} lo={int(lo)} cast={cast}" + (" barrier" if barrier else "")
    return b


def _chain_gemm(b, name, kind, X, out_dt, *, seed, geo=None, stride=1, halo=False, bias=True, rpb=0, res=True, res_wrap=0, k_extra=0, dead=False, **kw):
    """_identity_gemm with the epilogue terms the deployed GEMMs carry.  The product is fp16(X) exactly (identity weights: on the centre
    tap of a convolution — stride 2 reads the even pixels of an image four times the size, the halo layout the interior frames — and zero
    weights against every other operand value, which is randn); the epilogue then adds a bias, a row bias per `rpb` rows and a residual in
    fp32, in the kernels' order (t2v_kernels.h t2v_epilogue_rows, norm.hip splitk_gn_kernel).  Each addition is one IEEE fp32 operation, so
    the value the norm sees is reproduced bit for bit on the CPU: X' = ((fp16(X) + bias) + rowbias) + residual, residual = X - (...) in
    fp32 where there is one (X' = X up to one rounding), else the operand is fp16(X - the bias terms) and X' = X up to that rounding.
    Returns (op, y window, X' in float64): the reference of the norm is taken from X', the stored tensor must equal it bit for bit."""
    P = b.P
    M, C = X.shape
    g = torch.Generator().manual_seed(seed + 5)
    eye = torch.eye(C)
    rnd = lambda *shape: torch.randn(*shape, generator=g).half()
    bv = 0.5 * torch.randn(C, generator=g) if bias else None
    rbv = 0.5 * torch.randn(M // rpb, C, generator=g) if rpb else None
    # without a residual to close the gap the operand is fp16(X - bias terms): X' = X up to that rounding, and the designed rows keep their weight
    pre = X.float()
    if not res:
        pre = pre - (bv if bias else 0.0) - (rbv[torch.arange(M) // rpb] if rpb else 0.0)
    hi = pre.half()
    if kind == "conv":
        Fr, H, W = geo
        n_img = M // (H * W)
        w4 = torch.zeros(C, C, 3, 3)
        w4[:, :, 1, 1] = eye
        Wt, K, gather = pk.conv3x3(w4).half(), 9 * C, L.GATHER_CONV3X3
        A = rnd(n_img, stride * H, stride * W, C)
        A[:, ::stride, ::stride] = hi.view(n_img, H, W, C)
        A = A.reshape(-1, C)
        conv = dict(Hin=stride * H, Win=stride * W, Cin=C, stride=stride, up=0, Hout=H, Wout=W)
    elif kind == "tconv":
        Fr, H, W = geo
        HW, clips = H * W, M // (Fr * H * W)
        w5 = torch.zeros(C, C, 3, 1, 1)
        w5[:, :, 1, 0, 0] = eye
        Wt, K, gather, conv = pk.tconv3(w5).half(), 3 * C, L.GATHER_TCONV3, dict(F=Fr, HW=HW, Cin=C)
        A = hi
        if halo:
            A = rnd(clips, Fr + 2, HW, C)
            A[:, 1:-1] = hi.view(clips, Fr, HW, C)
            A = A.reshape(-1, C)
    else:
        Wt, K, gather, conv = torch.cat([eye, torch.zeros(C, k_extra)], dim=1).half(), C + k_extra, L.GATHER_PLAIN, None
        A = hi if not k_extra else torch.cat([hi, rnd(M, k_extra)], dim=1)
    a = P.alloc(A.shape[0], A.shape[1], "f16")
    b.put(a, A)
    v = hi.float()
    bias_ref, rb, r = NULL, None, None
    if bias:
        bias_ref, v = b.weight(name + ".bias", bv), v + bv
    if rpb:
        assert M % rpb == 0
        rb = P.alloc(M // rpb, C, "f32")
        b.put(rb, rbv)
        v = v + rbv[torch.arange(M) // rpb]
    if res:
        rr = res_wrap or M
        rv = (X.float() - v)[:rr]
        r = P.alloc(rr, C, "f32")
        b.put(r, rv)
        v = v + (torch.cat([rv, rv[:M - rr]]) if res_wrap else rv)
    y = b.fenced(M, C, out_dt, window=(0, 0) if dead else None)
    op = P.gemm(name, a, b.weight(name + ".w", Wt), C, K, y, bias=bias_ref, gather=gather, conv=conv, rowbias=rb, rows_per_batch=rpb, residual=r,
                halo=halo, m=M, res_wrap=res_wrap, **kw)
    assert (op.p[2].space != "null") == bool(bias) and (op.p[3].space != "null" or "ln" in kw) == bool(rpb or "ln" in kw) and (op.p[4].space != "null") == bool(res)
    return op, y, v.double()


# row geometry of a fused-norm case: (frames, H, W) of one instance against the tile's rows `bm`: half a tile, a whole tile, 1.5 tiles
# (straddle) or — M ragged — 1.25 tiles (a tile and 32 rows where a quarter tile is no multiple of 32, the unit the lowering asks of an
# instance: program.py `rows % 32`); images of 8 / 12 / 16 columns
def _epi_rows(seam, ragged, bm):
    return {"half": bm // 2, "whole": bm, "straddle": bm + ((bm // 4 if bm % 128 == 0 else 32) if ragged else bm // 2)}[seam]


def _build_lowered_epi(c, ncu):
    """T2V_EPI_GN without split-K on the combinations deployed: tile x gather (stride 2, halo frames) x output dtype x bias / row bias /
    residual x SiLU x low-order image x dead result x how the instances meet the row tiles x ragged M / N.  C: two column tiles of the tile,
    or 320 against 128- / 256-wide tiles (ragged).  `chunked`: more tiles than the device holds at once (the lowering's bound: one
    workgroup of a gemm2 tile per compute unit) — ONE column tile and 256 row tiles + 2: it cannot be smaller."""
    b = Built(c)
    P, kind, tile, seam, ragged, dead, lo, silu = b.P, c["kind"], c["tile"], c["seam"], c["m_ragged"], c["x_dead"], c["lo"], c["silu"]
    bm, bn = L.GEMM_TILES[tile].bm, L.GEMM_TILES[tile].bn
    C = 320 if c["n_ragged"] else (bn if c["chunked"] and bn % GROUPS == 0 and bn >= 256 else 2 * bn)
    rows = _epi_rows(seam, ragged, bm)
    n_inst = (5 if ragged else 4) if seam == "half" else 2
    if kind == "tconv":          # instances are frames of 5-frame clips
        n_inst = 5 if (seam == "whole" or ragged) else 10
    if c["chunked"]:
        n_inst = 256 * L.GEMM_TILES[tile].per_cu * bm // rows + 2
        if kind == "tconv":
            n_inst = -(-n_inst // 5) * 5
    while (n_inst * rows % bm != 0) != bool(ragged):              # the next instance (clip) count at which M is whole tiles, or is not
        n_inst += 5 if kind == "tconv" else 1
    M = n_inst * rows
    assert (M % bm != 0) == bool(ragged), (M, bm)
    geo = (5 if kind == "tconv" else 1, rows // 16 if rows % 16 == 0 else rows // 8, 16 if rows % 16 == 0 else 8)
    assert geo[1] * geo[2] == rows
    P.force_tile = tile
    X = gn_input(c["variant"], n_inst, rows, C, GROUPS, "f32", c["seed"])
    gamma, beta = affine(C, c["seed"])
    full = b.fenced(M, 2 * C if lo else C, "f16")
    op, y, X1 = _chain_gemm(b, "g", kind, X, c["out"], seed=c["seed"], geo=geo, stride=c["stride"], halo=c["halo"], rpb=rows if c["rowbias"] else 0,
                            res=c["res"], dead=dead, allow_splitk=False)
    out = full.col_slice(0, C)
    fused = P.groupnorm("gn", y, b.weight("g", gamma), b.weight("be", beta), out, n_inst=n_inst, eps=EPS, silu=silu, lo=lo,
                        gb=b.weight("gb", torch.cat([gamma, beta])), x_dead=dead)
    assert fused is op and op.i[16] == L.EPI_GN and len(P.ops) == 1 and op.i[19] == 1, "the norm did not become the GEMM's epilogue"
    assert (op.i[24], op.i[27], op.i[28], op.i[29], op.i[22]) == (rows, int(lo), GROUPS, int(dead), tile)
    if not dead:
        b.exact.append(("stored x", y, X1.float() if c["out"] == "f32" else X1.half()))
    b.expect("gn", out, full.col_slice(C, 2 * C) if lo else None, X1, gamma, beta, n_inst, GROUPS, silu)
    b.path = f"EPI_GN tile {tile} {kind} M={M} C={C} rows={rows} ({seam}) dead={int(dead)} lo={int(lo)}" + (" chunked" if c["chunked"] else "")
    return b


def _build_lowered_splitk(c, ncu):
    """splitk_gn_kernel (the reduction launch of a split-K GEMM with T2V_EPI_GN) on the epilogue combinations deployed, at the rows-per-thread
    counts deployed: the launcher picks KR as the first count whose grid fits the device, so the row count is the smallest that overflows
    it at every smaller count (rows_for_kr) — it cannot be smaller."""
    b = Built(c)
    P, C, dead, lo, silu, n_inst = b.P, 640, c["x_dead"], c["lo"], c["silu"], 64
    rows = 20 if c["kr"] == 1 else rows_for_kr(c["kr"], n_inst, C, ncu, SPLITK_KRS, False)
    if rows % coop_chunking(rows, n_inst, C // 8, ncu, 1 << 30, SPLITK_KRS)[1] == 0:
        rows += 1
    rows += rows % 2
    M = n_inst * rows
    P.force_tile = 5
    P.target_cus = max(256, 4 * -(-M // 128) * (C // 128))          # the lowering splits K only where the tiles leave compute units idle
    X = gn_input(c["variant"], n_inst, rows, C, GROUPS, "f32", c["seed"])
    gamma, beta = affine(C, c["seed"])
    full = b.fenced(M, 2 * C if lo else C, "f16")
    op, y, X1 = _chain_gemm(b, "g", "plain", X, c["out"], seed=c["seed"], rpb=rows // 2 if c["rowbias"] else 0, res=c["res"], k_extra=2048 - C, dead=dead)
    out = full.col_slice(0, C)
    fused = P.groupnorm("gn", y, b.weight("g", gamma), b.weight("be", beta), out, n_inst=n_inst, eps=EPS, silu=silu, lo=lo,
                        gb=b.weight("gb", torch.cat([gamma, beta])), x_dead=dead)
    assert fused is op and op.i[16] == L.EPI_GN and op.meta["split"] > 1 and len(P.ops) == 1
    kr, rc, nchunk = coop_chunking(rows, n_inst, C // 8, ncu, 1 << 30, SPLITK_KRS)
    assert kr == c["kr"], (kr, rows)
    b.kr = kr
    if not dead:
        b.exact.append(("stored x", y, X1.float() if c["out"] == "f32" else X1.half()))
    b.expect("gn", out, full.col_slice(C, 2 * C) if lo else None, X1, gamma, beta, n_inst, GROUPS, silu)
    b.path = f"EPI_GN split={op.meta['split']} rows={rows} x {n_inst} dead={int(dead)} lo={int(lo)}"
    return b


def _build_lowered_ln(c, ncu):
    """The fused LayerNorm outputs (i[8] = 1: whole rows in the tile; 2: across column tiles) with the bias and the residual the deployed
    Linears carry: two row tiles (+ 36 rows), N of two column tiles (320 against 256-wide tiles where N is ragged).  `chunked`: more tiles
    than the lowering's co-residency bound holds, so that the launch is cut into row chunks — it cannot be smaller."""
    b = Built(c)
    tile, mode = c["tile"], c["mode"]
    geo = L.GEMM_TILES[tile]
    N = geo.bn if mode == 1 else (320 if c["n_ragged"] else 2 * geo.bn)
    tiles_m = 2
    if c["chunked"]:
        cap = min(geo.per_cu * 256, L.GN_PART_BYTES // (geo.bm * 16))
        tiles_m = cap // -(-N // geo.bn) + 1
    M = tiles_m * geo.bm + (36 if c["m_ragged"] else 0)
    b.P.force_tile = tile
    X = ln_input(c["variant"], M, N, c["seed"])
    gamma, beta = affine(N, c["seed"])
    ln_out = b.fenced(M, N, "f16")
    wrap = M // 2 + 13 if c["wrap"] else 0
    op, y, X1 = _chain_gemm(b, "g", "plain", X, "f32", seed=c["seed"], res=c["res"], res_wrap=wrap, allow_splitk=False,
                            ln=(b.weight("gb", torch.cat([gamma, beta])), b.weight("g", gamma), b.weight("be", beta), ln_out, EPS))
    assert op.i[22] == tile and op.i[8] == mode and len(b.P.ops) == 1 and (op.i[12] > 0) == bool(wrap), "the LayerNorm did not become the GEMM's epilogue"
    b.exact.append(("stored x", y, X1.float()))
    b.expect("ln", ln_out, None, X1, gamma, beta, M, 1, False)
    b.path = f"GEMM tile {tile} i[8]={mode} {M}x{N}" + (" chunked" if c["chunked"] else "") + (" res_wrap" if wrap else "")
    return b


_BUILDERS = dict(gn=_build_gn, strips=_build_strips, shard=_build_shard, epi=_build_epi, splitk=_build_splitk, ln=_build_ln, lnfused=_build_lnfused, lowered_gn=_build_lowered_gn, lowered_epi=_build_lowered_epi, lowered_splitk=_build_lowered_splitk,
                 lowered_ln=_build_lowered_ln)


def build(case, ncu=None):
    """The program of a case.  ncu: the device's CU count (the chunking of the cooperative kernels depends on it); None: the lowering's own
    figure (256 without a device)."""
    return _BUILDERS[case["family"]](case, Program.device_cus() if ncu is None else ncu)


# ---- the case list --------------------------------------------------------------------------------------------------------------------------
VARIANTS = ("distinct", "marked", "offset")
CASES = []
# stand-alone GroupNorm: C = 2560 takes the column loop of gn_stats_kernel (cv > 256) and R = 1 in the cooperative tile; rows = 1: one row
# per instance.  The single-launch kernel needs C / groups % 4 == 0: it has no C = 320 form (the launcher refuses the record).
for _form in ("three_launch", "cooperative", "single_launch"):
    for _n, _r, _C, _dt in ((3, 101, 320, "f32"), (2, 37, 2560, "f16"), (5, 1, 128, "f32")):
        if _form == "single_launch" and (_C // GROUPS) % 4:
            continue
        # (5, 1, 128) has blocks of 4 values: their squares, rounded to fp32, leave the single-pass variance up to 2^-24 (1 + 32^2) = 6e-5 off
        # at mean / std = 32 — 3e-5 in the output whatever the summation order, beyond the hi + lo figure by the number format alone (torch's
        # fp32 group_norm does not form x^2 - mean^2, so e_torch does not pay it): no `offset` rows on that shape
        CASES += [_gn_case(_form, _n, _r, _C, _dt, v) for v in VARIANTS if not (v == "offset" and _r * (_C // GROUPS) < 32)]
CASES.append(_gn_case("cooperative", 3, 101, 320, "f32", "marked", barrier=True, id="gn-cooperative-barrier-3x101x320-f32-marked"))
# gn_coop_kernel at every rows-per-thread count: the row count depends on the device (rows_for_kr), ~2054 at KR = 20 on 256 CUs
CASES += [_gn_case("cooperative", 2, 0, 2560, "f32", "marked", kr=kr, id=f"gn-coop-KR{kr}-2x2560-marked") for kr in COOP_KRS]
for _v in VARIANTS:
    CASES.append(_case("strips", "strips-wave-3x96x320", _v, n_inst=3, rows=96, C=320, wide=False, seed=301))
    CASES.append(_case("strips", "strips-wg-2x832x1280", _v, n_inst=2, rows=832, C=1280, wide=True, seed=302))
    CASES.append(_case("shard", "shard-2parts-48+24", _v, C=320, frame_rows=24, frames=3, size=2, dt="f32", halo=False, strips=False, seed=311))
    CASES.append(_case("shard", "shard-3parts-40+40+20", _v, C=320, frame_rows=20, frames=5, size=3, dt="f16", halo=False, strips=False, seed=312))
    CASES.append(_case("shard", "shard-3parts-strips-64+64+32", _v, C=320, frame_rows=32, frames=5, size=3, dt="f32", halo=False, strips=True, seed=313))
    CASES.append(_case("shard", "shard-2parts-halo-48+24", _v, C=320, frame_rows=24, frames=3, size=2, dt="f32", halo=True, strips=False, seed=314))
# T2V_EPI_GN: 256-row frames (B, F, H, W = 2, 3, 16, 16): per frame they straddle the 192-row tiles and are two 128-row tiles, per clip
# (768 rows) a whole number of either; 64- / 96-row frames are half a tile
# The epilogue folds 32-row column sums of x and x^2 in fp32 (as the strips): `offset` rows go to the cases without a low-order output, for
# the reason given in _build_strips
_EPI_KTC = [("conv", 8, 320), ("tconv", 8, 320), ("plain", 8, 320), ("tconv", 11, 320), ("plain", 11, 320), ("tconv", 0, 640), ("conv", 0, 640),
            ("plain", 0, 640), ("tconv", 5, 640), ("plain", 5, 1280), ("conv", 3, 640), ("plain", 3, 640)]
_EPI_MODES = [(True, True, False), (False, False, True), (False, True, False), (True, False, False)]      # per_frame, dead, lo
_n = 0
for _kind, _tile, _C in _EPI_KTC:
    for _pf, _dead, _lo in _EPI_MODES:
        _seam = "whole" if (not _pf or _EPI_BM[_tile] == 128) else "straddle"
        CASES.append(_case("epi", f"epi-{_kind}-t{_tile}-C{_C}-{'frame' if _pf else 'clip'}-{_seam}{'-dead' if _dead else ''}{'-lo' if _lo else ''}",
                           VARIANTS[_n % (2 if _lo else 3)], kind=_kind, tile=_tile, C=_C, per_frame=_pf, dead=_dead, lo=_lo, geo=(2, 3, 16, 16), seam=_seam,
                           seed=400 + _n))
        _n += 1
for _kind, _tile, _C, _geo in (("plain", 0, 640, (2, 3, 8, 8)), ("conv", 3, 640, (2, 3, 8, 8)), ("tconv", 5, 640, (2, 3, 8, 8)),
                               ("plain", 11, 320, (2, 3, 8, 8)), ("conv", 8, 320, (2, 3, 8, 12)), ("tconv", 8, 320, (2, 3, 8, 12))):
    _dead, _lo = _n % 2 == 0, _n % 2 == 1
    CASES.append(_case("epi", f"epi-{_kind}-t{_tile}-C{_C}-frame-half{'-dead' if _dead else '-lo'}", VARIANTS[_n % (2 if _lo else 3)], kind=_kind, tile=_tile, C=_C,
                       per_frame=True, dead=_dead, lo=_lo, geo=_geo, seam="half", seed=400 + _n))
    _n += 1
# splitk_gn_kernel: two rows-per-thread counts per width
for _C, _kr, _dead, _v in ((640, 1, True, "marked"), (640, 2, False, "distinct"), (1280, 1, False, "offset"), (1280, 2, True, "marked"),
                           (640, 2, False, "offset"), (1280, 2, False, "marked")):
    CASES.append(_case("splitk", f"splitk-C{_C}-KR{_kr}{'-dead' if _dead else '-lo'}", _v, C=_C, n_inst=2, kr=_kr, dead=_dead, lo=not _dead, seed=500 + _C + _kr))
# LayerNorm: one width per instantiation (rows kernel <2>, <3>, wide kernel <5>, <8>), ragged against the 4 rows of a workgroup
for _v in ("distinct", "offset"):
    for _C in (320, 768, 1280, 2048):
        for _M in (77, 513):
            CASES.append(_case("ln", f"ln-{_M}x{_C}", _v, M=_M, C=_C, cap=0, seed=600 + _C + _M))
    CASES.append(_case("ln", "ln-77x320-cap2", _v, M=77, C=320, cap=2, seed=601))
    for _tile in (8, 11, 2):
        CASES.append(_case("lnfused", f"lnfused-t{_tile}-397x320", _v, M=397, N=320, tile=_tile, mode=1, seed=610 + _tile))
    for _tile, _N in ((0, 640), (3, 768), (5, 1280), (9, 512), (12, 1280)):
        CASES.append(_case("lnfused", f"lnx-t{_tile}-397x{_N}", _v, M=397, N=_N, tile=_tile, mode=2, seed=620 + _tile))
# `lowered` LayerNorm paths: row counts that are whole workgroups of 4 rows (the cases above are ragged), with and without the grid-stride walk
for _C, _cap in ((320, 0), (768, 0), (1280, 0), (320, 2), (768, 2)):
    CASES.append(_case("ln", f"lowered-ln-76x{_C}" + (f"-cap{_cap}" if _cap else ""), "distinct", M=76, C=_C, cap=_cap, seed=640 + _C + _cap))
# the `lowered` family, stand-alone GroupNorm records: (launch form, input dtype, SiLU, low-order image, cast output 0 / 1 / 2 = with its low-order
# image, rows per thread of the cooperative kernel, grid barrier instead of tagged records, column loop)
_LOWERED_GN = [
    ('coop-fallback', 'f16', 1, 0, 0, 0, 0, 0),
    ('coop-fallback', 'f32', 0, 0, 0, 0, 0, 0),
    ('coop-fallback', 'f32', 0, 1, 0, 0, 0, 0),
    ('coop-fallback', 'f32', 1, 0, 0, 0, 0, 0),
    ('coop-fallback', 'f32', 1, 0, 2, 0, 0, 0),
    ('coop-fallback', 'f32', 1, 0, 2, 0, 0, 1),
    ('cooperative', 'f16', 1, 0, 0, 4, 0, 0),
    ('cooperative', 'f16', 1, 0, 0, 4, 1, 0),
    ('cooperative', 'f16', 1, 0, 0, 8, 0, 0),
    ('cooperative', 'f16', 1, 0, 0, 12, 0, 0),
    ('cooperative', 'f16', 1, 0, 0, 16, 0, 0),
    ('cooperative', 'f32', 0, 0, 0, 4, 0, 0),
    ('cooperative', 'f32', 0, 0, 0, 8, 0, 0),
    ('cooperative', 'f32', 0, 0, 0, 16, 0, 0),
    ('cooperative', 'f32', 0, 1, 0, 8, 0, 0),
    ('cooperative', 'f32', 0, 1, 0, 16, 0, 0),
    ('cooperative', 'f32', 1, 0, 0, 4, 0, 0),
    ('cooperative', 'f32', 1, 0, 0, 4, 0, 1),
    ('cooperative', 'f32', 1, 0, 0, 4, 1, 0),
    ('cooperative', 'f32', 1, 0, 0, 8, 0, 0),
    ('cooperative', 'f32', 1, 0, 0, 8, 0, 1),
    ('cooperative', 'f32', 1, 0, 0, 12, 0, 0),
    ('cooperative', 'f32', 1, 0, 0, 16, 0, 0),
    ('cooperative', 'f32', 1, 0, 0, 20, 0, 0),
    ('cooperative', 'f32', 1, 0, 0, 20, 0, 1),
    ('cooperative', 'f32', 1, 0, 1, 4, 0, 0),
    ('cooperative', 'f32', 1, 0, 2, 12, 0, 0),
    ('cooperative', 'f32', 1, 0, 2, 16, 0, 0),
    ('single_launch', 'f16', 1, 0, 0, 0, 0, 0),
    ('single_launch', 'f32', 0, 0, 0, 0, 0, 0),
    ('single_launch', 'f32', 1, 0, 0, 0, 0, 0),
    ('single_launch', 'f32', 1, 0, 0, 0, 0, 1),
    ('single_launch', 'f32', 1, 0, 1, 0, 0, 0),
    ('single_launch', 'f32', 1, 0, 2, 0, 0, 1),
    ('three_launch', 'f16', 1, 0, 0, 0, 0, 0),
    ('three_launch', 'f32', 1, 0, 0, 0, 0, 0),
]
def _lowered_gn_cases(specs):
    for _form, _dt, _gsilu, _lo, _cast, _kr, _bar, _cl in specs:
        CASES.append(_case("lowered_gn", f"lowered-gn-{_form}-{_dt}{'-silu' if _gsilu else ''}{'-lo' if _lo else ''}{('', '-cast', '-cast+lo')[_cast]}"
                           f"{'-KR' + str(_kr) if _kr else ''}{'-barrier' if _bar else ''}{'-C2560' if _cl else ''}", "marked", form=_form, dt=_dt, silu=bool(_gsilu),
                           lo=bool(_lo), cast=_cast, kr=_kr, barrier=bool(_bar), cols_loop=_cl, seed=700 + len(CASES)))


_lowered_gn_cases(_LOWERED_GN)
# ... sharded phases 1 / 2 and the strip-fed phase 3: halo rows on both sides (three parts), fp16 inputs, no SiLU, no low-order image, parts of
# one statistics block (4 + 2 rows), the column loop (C = 2560), strips folded by a workgroup (C = 1280: 26 strips x 40 channels > 1024; 4160
# rows: one row more or less in n shows only against the hi + lo figure, so those two keep the low-order image).  (`x_dead` in the
# fused families below: the result is not stored, as `dead` above, but the tensor is the fp32 chain, not an fp16 one)
for _id, _kw in (("3parts-halo-f32", dict(C=320, frame_rows=20, frames=5, size=3, dt="f32", halo=True, strips=False)),
                 ("3parts-halo-f16", dict(C=320, frame_rows=20, frames=5, size=3, dt="f16", halo=True, strips=False)),
                 ("2parts-f32-nolo", dict(C=320, frame_rows=24, frames=3, size=2, dt="f32", halo=False, strips=False, lo=False)),
                 ("2parts-f32-nosilu-lo", dict(C=320, frame_rows=24, frames=3, size=2, dt="f32", halo=False, strips=False, lo=True, silu=False)),
                 ("2parts-f32-nosilu-nolo", dict(C=320, frame_rows=24, frames=3, size=2, dt="f32", halo=False, strips=False, lo=False, silu=False)),
                 ("2parts-4+2rows-f32-nosilu", dict(C=320, frame_rows=2, frames=3, size=2, dt="f32", halo=False, strips=False, lo=False, silu=False, target_cus=256)),
                 ("2parts-4+2rows-f32", dict(C=320, frame_rows=2, frames=3, size=2, dt="f32", halo=False, strips=False, lo=False, target_cus=256)),
                 ("2parts-4+2rows-f16", dict(C=320, frame_rows=2, frames=3, size=2, dt="f16", halo=False, strips=False, lo=False, target_cus=256)),
                 ("2parts-f16-nolo", dict(C=320, frame_rows=24, frames=3, size=2, dt="f16", halo=False, strips=False, lo=False)),
                 ("2parts-C2560-f32", dict(C=2560, frame_rows=24, frames=3, size=2, dt="f32", halo=False, strips=False, lo=False)),
                 ("3parts-strips-wg-f32", dict(C=1280, frame_rows=832, frames=5, size=3, dt="f32", halo=False, strips=True, lo=True)),
                 ("3parts-strips-wg-f16", dict(C=1280, frame_rows=832, frames=5, size=3, dt="f16", halo=False, strips=True, lo=True)),
                 ("3parts-strips-f16", dict(C=320, frame_rows=32, frames=5, size=3, dt="f16", halo=False, strips=True, lo=True))):
    CASES.append(_case("shard", "lowered-shard-" + _id, "distinct" if _kw["frame_rows"] < 3 else "marked", seed=800 + len(CASES), **_kw))
CASES.append(_case("strips", "lowered-strips-wave-3x96x320-f16", "marked", n_inst=3, rows=96, C=320, wide=False, dt="f16", lo=False, seed=303))
# ... T2V_EPI_GN without split-K: (tile, gather, stride, halo frames, M ragged, N ragged, out dtype, row bias, residual, SiLU, low-order image,
# dead result, how instances meet the row tiles, more tiles than the device holds)
_LOWERED_EPI = [
    (0, 'conv', 1, 0, 0, 0, 'f16', 1, 0, 1, 0, 1, 'half', 0),
    (0, 'conv', 1, 0, 0, 0, 'f32', 1, 0, 1, 0, 1, 'half', 0),
    (0, 'conv', 1, 0, 1, 0, 'f16', 1, 0, 1, 0, 1, 'half', 0),
    (0, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 0, 0, 0, 'straddle', 0),
    (0, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 0, 0, 0, 'whole', 0),
    (0, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 0, 1, 0, 'straddle', 0),
    (0, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'half', 0),
    (0, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'whole', 0),
    (0, 'plain', 1, 0, 1, 0, 'f32', 0, 1, 0, 0, 0, 'straddle', 0),
    (0, 'plain', 1, 0, 1, 0, 'f32', 0, 1, 1, 0, 0, 'half', 0),
    (0, 'tconv', 1, 0, 0, 0, 'f16', 0, 0, 1, 0, 1, 'straddle', 0),
    (0, 'tconv', 1, 0, 0, 0, 'f16', 0, 0, 1, 0, 1, 'whole', 0),
    (0, 'tconv', 1, 0, 0, 0, 'f32', 0, 0, 1, 0, 1, 'straddle', 0),
    (0, 'tconv', 1, 0, 0, 0, 'f32', 0, 1, 0, 0, 0, 'half', 0),
    (0, 'tconv', 1, 0, 0, 0, 'f32', 0, 1, 0, 0, 0, 'whole', 0),
    (0, 'tconv', 1, 0, 0, 0, 'f32', 0, 1, 0, 1, 0, 'half', 0),
    (0, 'tconv', 1, 0, 1, 0, 'f16', 0, 0, 1, 0, 1, 'straddle', 0),
    (0, 'tconv', 1, 0, 1, 0, 'f32', 0, 1, 0, 0, 0, 'half', 0),
    (0, 'tconv', 1, 1, 0, 0, 'f32', 0, 1, 0, 0, 0, 'half', 0),
    (0, 'tconv', 1, 1, 1, 0, 'f32', 0, 1, 0, 0, 0, 'half', 0),
    (11, 'conv', 1, 0, 0, 0, 'f16', 1, 0, 1, 0, 1, 'whole', 0),
    (11, 'conv', 1, 0, 0, 0, 'f32', 0, 1, 0, 1, 0, 'whole', 0),
    (11, 'conv', 2, 0, 0, 0, 'f32', 0, 0, 1, 0, 0, 'whole', 0),
    (11, 'conv', 2, 0, 0, 0, 'f32', 0, 0, 1, 0, 0, 'whole', 1),
    (11, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 0, 0, 0, 'whole', 0),
    (11, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 0, 1, 0, 'whole', 0),
    (11, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'whole', 0),
    (11, 'tconv', 1, 0, 0, 0, 'f16', 0, 0, 1, 0, 1, 'whole', 0),
    (11, 'tconv', 1, 0, 0, 0, 'f32', 0, 1, 0, 1, 0, 'whole', 0),
    (11, 'tconv', 1, 1, 0, 0, 'f32', 0, 1, 0, 1, 0, 'whole', 0),
    (3, 'conv', 1, 0, 0, 0, 'f16', 1, 0, 1, 0, 1, 'whole', 0),
    (3, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'whole', 0),
    (3, 'plain', 1, 0, 0, 1, 'f32', 0, 1, 1, 0, 0, 'whole', 0),
    (3, 'tconv', 1, 1, 0, 1, 'f32', 0, 1, 0, 0, 0, 'whole', 0),
    (5, 'conv', 1, 0, 0, 0, 'f16', 1, 0, 1, 0, 1, 'half', 0),
    (5, 'conv', 1, 0, 0, 0, 'f16', 1, 0, 1, 0, 1, 'whole', 0),
    (5, 'conv', 1, 0, 0, 0, 'f16', 1, 0, 1, 0, 1, 'whole', 1),
    (5, 'conv', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'whole', 0),
    (5, 'conv', 1, 0, 0, 1, 'f16', 1, 0, 1, 0, 1, 'straddle', 0),
    (5, 'conv', 1, 0, 0, 1, 'f16', 1, 0, 1, 0, 1, 'whole', 0),
    (5, 'conv', 1, 0, 0, 1, 'f32', 0, 1, 0, 0, 0, 'straddle', 0),
    (5, 'conv', 1, 0, 0, 1, 'f32', 0, 1, 0, 1, 0, 'straddle', 0),
    (5, 'conv', 1, 0, 0, 1, 'f32', 0, 1, 0, 1, 0, 'whole', 0),
    (5, 'conv', 1, 0, 0, 1, 'f32', 1, 0, 1, 0, 1, 'straddle', 0),
    (5, 'conv', 1, 0, 1, 0, 'f16', 1, 0, 1, 0, 1, 'half', 0),
    (5, 'conv', 1, 0, 1, 1, 'f16', 1, 0, 1, 0, 1, 'straddle', 0),
    (5, 'conv', 1, 0, 1, 1, 'f32', 0, 1, 0, 0, 0, 'straddle', 0),
    (5, 'conv', 1, 0, 1, 1, 'f32', 0, 1, 0, 1, 0, 'straddle', 0),
    (5, 'conv', 2, 0, 0, 0, 'f32', 0, 0, 1, 0, 0, 'whole', 0),
    (5, 'conv', 2, 0, 0, 1, 'f32', 0, 0, 1, 0, 0, 'whole', 0),
    (5, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 0, 0, 0, 'whole', 0),
    (5, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'half', 0),
    (5, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'whole', 0),
    (5, 'plain', 1, 0, 0, 1, 'f32', 0, 1, 1, 0, 0, 'straddle', 0),
    (5, 'plain', 1, 0, 0, 1, 'f32', 0, 1, 1, 0, 0, 'whole', 0),
    (5, 'plain', 1, 0, 1, 1, 'f32', 0, 1, 1, 0, 0, 'straddle', 0),
    (5, 'tconv', 1, 0, 0, 0, 'f16', 0, 0, 1, 0, 1, 'whole', 0),
    (5, 'tconv', 1, 0, 0, 0, 'f32', 0, 1, 0, 0, 0, 'half', 0),
    (5, 'tconv', 1, 0, 0, 0, 'f32', 0, 1, 0, 0, 0, 'whole', 0),
    (5, 'tconv', 1, 1, 0, 0, 'f32', 0, 1, 0, 0, 0, 'half', 0),
    (5, 'tconv', 1, 1, 0, 0, 'f32', 0, 1, 0, 0, 0, 'whole', 0),
    (5, 'tconv', 1, 1, 0, 0, 'f32', 0, 1, 0, 0, 0, 'whole', 1),
    (5, 'tconv', 1, 1, 1, 0, 'f32', 0, 1, 0, 0, 0, 'half', 0),
    (8, 'conv', 1, 0, 0, 0, 'f16', 1, 0, 1, 0, 1, 'straddle', 0),
    (8, 'conv', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'whole', 0),
    (8, 'conv', 2, 0, 0, 0, 'f32', 0, 0, 1, 0, 0, 'whole', 1),
    (8, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 0, 1, 0, 'whole', 0),
    (8, 'plain', 1, 0, 0, 0, 'f32', 0, 1, 1, 0, 0, 'straddle', 0),
    (8, 'tconv', 1, 0, 0, 0, 'f16', 0, 0, 1, 0, 1, 'whole', 0),
    (8, 'tconv', 1, 0, 0, 0, 'f32', 0, 1, 0, 1, 0, 'straddle', 0),
]
# ... of the requestable lattice (tests/geometry_lattice.py; profiles/geometry_paths.txt names a witness program for each): other frame counts
# and latents put the same fused norms on the other tiles and make rows and columns ragged.  gn_seam is t2v_kernels.h:912-922's class (an
# instance of half a tile, whole tiles, or a tile that straddles two instances); gn_chunked is gemm.hip:361 / gemm2.hip:519
# t2v_launch_coresident's (more tiles than the device holds at once: the launch is cut into row chunks)
_LOWERED_EPI += [
    (0,'plain',1,0,0,0,'f32',0,1,0,0,0,'straddle',1), (0,'plain',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (0,'plain',1,0,0,0,'f32',0,1,1,0,0,'half',1),
    (0,'plain',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (0,'plain',1,0,0,0,'f32',0,1,1,0,0,'straddle',1), (0,'plain',1,0,0,0,'f32',0,1,1,0,0,'whole',1),
    (0,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',0), (0,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',1), (0,'tconv',1,0,0,0,'f16',0,0,1,0,1,'straddle',1),
    (0,'tconv',1,0,0,0,'f16',0,0,1,0,1,'whole',1), (0,'tconv',1,0,0,0,'f32',0,1,0,0,0,'half',1), (0,'tconv',1,0,0,0,'f32',0,1,0,0,0,'straddle',0),
    (0,'tconv',1,0,0,0,'f32',0,1,0,0,0,'straddle',1), (0,'tconv',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (0,'tconv',1,0,0,0,'f32',0,1,1,0,0,'half',1),
    (0,'tconv',1,0,0,0,'f32',0,1,1,0,0,'straddle',1), (0,'tconv',1,0,0,0,'f32',0,1,1,0,0,'whole',1), (0,'tconv',1,0,1,0,'f32',0,1,0,0,0,'straddle',0),
    (0,'tconv',1,0,1,0,'f32',0,1,0,0,0,'straddle',1), (0,'tconv',1,1,0,0,'f32',0,1,0,0,0,'whole',1),
    (11,'conv',1,0,0,0,'f16',1,0,1,0,1,'half',0), (11,'conv',1,0,0,0,'f16',1,0,1,0,1,'half',1), (11,'conv',1,0,0,0,'f16',1,0,1,0,1,'straddle',0),
    (11,'conv',1,0,0,0,'f16',1,0,1,0,1,'straddle',1), (11,'conv',1,0,0,0,'f16',1,0,1,0,1,'whole',1), (11,'conv',1,0,0,0,'f32',0,1,0,0,0,'whole',1),
    (11,'conv',1,0,0,0,'f32',0,1,0,1,0,'straddle',0), (11,'conv',1,0,0,0,'f32',0,1,0,1,0,'straddle',1), (11,'conv',1,0,0,0,'f32',0,1,0,1,0,'whole',1),
    (11,'conv',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (11,'conv',1,0,0,0,'f32',0,1,1,0,0,'straddle',1), (11,'conv',1,0,0,0,'f32',0,1,1,0,0,'whole',0),
    (11,'conv',1,0,0,0,'f32',0,1,1,0,0,'whole',1), (11,'conv',1,0,1,0,'f16',1,0,1,0,1,'straddle',0), (11,'conv',1,0,1,0,'f16',1,0,1,0,1,'straddle',1),
    (11,'conv',1,0,1,0,'f32',0,1,0,1,0,'straddle',0), (11,'conv',1,0,1,0,'f32',0,1,1,0,0,'straddle',0), (11,'conv',2,0,0,0,'f32',0,0,1,0,0,'half',0),
    (11,'conv',2,0,0,0,'f32',0,0,1,0,0,'half',1), (11,'conv',2,0,0,0,'f32',0,0,1,0,0,'straddle',0), (11,'conv',2,0,0,0,'f32',0,0,1,0,0,'straddle',1),
    (11,'conv',2,0,1,0,'f32',0,0,1,0,0,'straddle',0), (11,'conv',2,0,1,0,'f32',0,0,1,0,0,'straddle',1), (11,'plain',1,0,0,0,'f32',0,1,0,0,0,'straddle',0),
    (11,'plain',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (11,'plain',1,0,0,0,'f32',0,1,0,1,0,'straddle',0), (11,'plain',1,0,0,0,'f32',0,1,0,1,0,'straddle',1),
    (11,'plain',1,0,0,0,'f32',0,1,0,1,0,'whole',1), (11,'plain',1,0,0,0,'f32',0,1,1,0,0,'half',0), (11,'plain',1,0,0,0,'f32',0,1,1,0,0,'half',1),
    (11,'plain',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (11,'plain',1,0,0,0,'f32',0,1,1,0,0,'straddle',1), (11,'plain',1,0,0,0,'f32',0,1,1,0,0,'whole',1),
    (11,'plain',1,0,1,0,'f32',0,1,0,0,0,'straddle',0), (11,'plain',1,0,1,0,'f32',0,1,0,1,0,'straddle',0), (11,'plain',1,0,1,0,'f32',0,1,1,0,0,'half',0),
    (11,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',0), (11,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',1), (11,'tconv',1,0,0,0,'f16',0,0,1,0,1,'straddle',0),
    (11,'tconv',1,0,0,0,'f16',0,0,1,0,1,'straddle',1), (11,'tconv',1,0,0,0,'f16',0,0,1,0,1,'whole',1), (11,'tconv',1,0,0,0,'f32',0,1,0,0,0,'straddle',1),
    (11,'tconv',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (11,'tconv',1,0,0,0,'f32',0,1,0,1,0,'half',0), (11,'tconv',1,0,0,0,'f32',0,1,0,1,0,'half',1),
    (11,'tconv',1,0,0,0,'f32',0,1,0,1,0,'straddle',0), (11,'tconv',1,0,0,0,'f32',0,1,0,1,0,'straddle',1), (11,'tconv',1,0,0,0,'f32',0,1,0,1,0,'whole',1),
    (11,'tconv',1,0,1,0,'f16',0,0,1,0,1,'straddle',0), (11,'tconv',1,0,1,0,'f32',0,1,0,1,0,'straddle',0), (11,'tconv',1,0,1,0,'f32',0,1,0,1,0,'straddle',1),
    (11,'tconv',1,1,0,0,'f32',0,1,0,1,0,'straddle',0), (11,'tconv',1,1,0,0,'f32',0,1,0,1,0,'whole',1),
    (3,'conv',1,0,0,0,'f16',1,0,1,0,1,'half',0), (3,'conv',1,0,0,0,'f16',1,0,1,0,1,'half',1), (3,'conv',1,0,0,0,'f16',1,0,1,0,1,'straddle',0),
    (3,'conv',1,0,0,0,'f16',1,0,1,0,1,'straddle',1), (3,'conv',1,0,0,0,'f16',1,0,1,0,1,'whole',1), (3,'conv',1,0,0,0,'f32',0,1,0,0,0,'straddle',0),
    (3,'conv',1,0,0,0,'f32',0,1,0,0,0,'whole',0), (3,'conv',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (3,'conv',1,0,0,0,'f32',0,1,1,0,0,'whole',0),
    (3,'conv',1,0,1,0,'f16',1,0,1,0,1,'half',0), (3,'conv',1,0,1,0,'f16',1,0,1,0,1,'half',1), (3,'conv',1,0,1,0,'f16',1,0,1,0,1,'straddle',0),
    (3,'conv',1,0,1,0,'f16',1,0,1,0,1,'straddle',1), (3,'conv',1,0,1,0,'f32',0,1,0,0,0,'straddle',0), (3,'conv',1,0,1,0,'f32',0,1,1,0,0,'straddle',0),
    (3,'conv',2,0,0,0,'f32',0,0,1,0,0,'half',0), (3,'conv',2,0,0,0,'f32',0,0,1,0,0,'straddle',0), (3,'conv',2,0,0,0,'f32',0,0,1,0,0,'whole',0),
    (3,'conv',2,0,1,0,'f32',0,0,1,0,0,'straddle',0), (3,'plain',1,0,0,0,'f32',0,1,0,0,0,'straddle',0), (3,'plain',1,0,0,0,'f32',0,1,0,0,0,'whole',0),
    (3,'plain',1,0,0,0,'f32',0,1,1,0,0,'half',0), (3,'plain',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (3,'plain',1,0,0,1,'f32',0,1,0,0,0,'straddle',0),
    (3,'plain',1,0,0,1,'f32',0,1,0,0,0,'straddle',1), (3,'plain',1,0,0,1,'f32',0,1,0,0,0,'whole',0), (3,'plain',1,0,0,1,'f32',0,1,0,0,0,'whole',1),
    (3,'plain',1,0,0,1,'f32',0,1,1,0,0,'half',0), (3,'plain',1,0,0,1,'f32',0,1,1,0,0,'straddle',0), (3,'plain',1,0,0,1,'f32',0,1,1,0,0,'straddle',1),
    (3,'plain',1,0,0,1,'f32',0,1,1,0,0,'whole',1), (3,'plain',1,0,1,0,'f32',0,1,0,0,0,'straddle',0), (3,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',0),
    (3,'plain',1,0,1,1,'f32',0,1,0,0,0,'straddle',0), (3,'plain',1,0,1,1,'f32',0,1,1,0,0,'straddle',0), (3,'plain',1,0,1,1,'f32',0,1,1,0,0,'straddle',1),
    (3,'tconv',1,0,0,0,'f16',0,0,1,0,1,'straddle',0), (3,'tconv',1,0,0,0,'f16',0,0,1,0,1,'whole',0), (3,'tconv',1,0,0,0,'f32',0,1,0,0,0,'half',0),
    (3,'tconv',1,0,0,0,'f32',0,1,0,0,0,'straddle',0), (3,'tconv',1,0,0,0,'f32',0,1,0,0,0,'whole',0), (3,'tconv',1,0,0,0,'f32',0,1,1,0,0,'half',0),
    (3,'tconv',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (3,'tconv',1,0,0,0,'f32',0,1,1,0,0,'whole',0), (3,'tconv',1,0,0,1,'f16',0,0,1,0,1,'straddle',0),
    (3,'tconv',1,0,0,1,'f16',0,0,1,0,1,'straddle',1), (3,'tconv',1,0,0,1,'f16',0,0,1,0,1,'whole',0), (3,'tconv',1,0,0,1,'f16',0,0,1,0,1,'whole',1),
    (3,'tconv',1,0,0,1,'f32',0,1,0,0,0,'half',0), (3,'tconv',1,0,0,1,'f32',0,1,0,0,0,'straddle',0), (3,'tconv',1,0,0,1,'f32',0,1,0,0,0,'straddle',1),
    (3,'tconv',1,0,0,1,'f32',0,1,0,0,0,'whole',0), (3,'tconv',1,0,0,1,'f32',0,1,0,0,0,'whole',1), (3,'tconv',1,0,1,0,'f16',0,0,1,0,1,'straddle',0),
    (3,'tconv',1,0,1,0,'f32',0,1,0,0,0,'straddle',0), (3,'tconv',1,0,1,0,'f32',0,1,1,0,0,'straddle',0), (3,'tconv',1,0,1,1,'f16',0,0,1,0,1,'straddle',0),
    (3,'tconv',1,0,1,1,'f32',0,1,0,0,0,'straddle',0), (3,'tconv',1,0,1,1,'f32',0,1,0,0,0,'straddle',1), (3,'tconv',1,1,0,0,'f32',0,1,0,0,0,'half',0),
    (3,'tconv',1,1,1,0,'f32',0,1,0,0,0,'half',0),
    (5,'conv',1,0,0,0,'f16',1,0,1,0,1,'half',1), (5,'conv',1,0,0,0,'f16',1,0,1,0,1,'straddle',0), (5,'conv',1,0,0,0,'f16',1,0,1,0,1,'straddle',1),
    (5,'conv',1,0,0,0,'f32',0,1,0,0,0,'straddle',0), (5,'conv',1,0,0,0,'f32',0,1,0,0,0,'straddle',1), (5,'conv',1,0,0,0,'f32',0,1,0,0,0,'whole',0),
    (5,'conv',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (5,'conv',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (5,'conv',1,0,0,0,'f32',0,1,1,0,0,'straddle',1),
    (5,'conv',1,0,0,0,'f32',0,1,1,0,0,'whole',1), (5,'conv',1,0,0,1,'f16',1,0,1,0,1,'half',0), (5,'conv',1,0,0,1,'f32',0,1,0,1,0,'half',0),
    (5,'conv',1,0,0,1,'f32',0,1,1,0,0,'half',0), (5,'conv',1,0,0,1,'f32',0,1,1,0,0,'straddle',0), (5,'conv',1,0,0,1,'f32',0,1,1,0,0,'whole',0),
    (5,'conv',1,0,1,0,'f16',1,0,1,0,1,'half',1), (5,'conv',1,0,1,0,'f16',1,0,1,0,1,'straddle',0), (5,'conv',1,0,1,0,'f16',1,0,1,0,1,'straddle',1),
    (5,'conv',1,0,1,0,'f32',0,1,0,0,0,'straddle',0), (5,'conv',1,0,1,0,'f32',0,1,1,0,0,'straddle',0), (5,'conv',1,0,1,1,'f16',1,0,1,0,1,'half',0),
    (5,'conv',1,0,1,1,'f32',0,1,0,1,0,'half',0), (5,'conv',1,0,1,1,'f32',0,1,1,0,0,'half',0), (5,'conv',1,0,1,1,'f32',0,1,1,0,0,'straddle',0),
    (5,'conv',2,0,0,0,'f32',0,0,1,0,0,'half',0), (5,'conv',2,0,0,0,'f32',0,0,1,0,0,'half',1), (5,'conv',2,0,0,0,'f32',0,0,1,0,0,'straddle',0),
    (5,'conv',2,0,0,0,'f32',0,0,1,0,0,'straddle',1), (5,'conv',2,0,0,0,'f32',0,0,1,0,0,'whole',1), (5,'conv',2,0,0,1,'f32',0,0,1,0,0,'half',0),
    (5,'conv',2,0,0,1,'f32',0,0,1,0,0,'straddle',0), (5,'conv',2,0,1,0,'f32',0,0,1,0,0,'half',0), (5,'conv',2,0,1,0,'f32',0,0,1,0,0,'half',1),
    (5,'conv',2,0,1,0,'f32',0,0,1,0,0,'straddle',0), (5,'conv',2,0,1,0,'f32',0,0,1,0,0,'straddle',1), (5,'conv',2,0,1,1,'f32',0,0,1,0,0,'half',0),
    (5,'conv',2,0,1,1,'f32',0,0,1,0,0,'straddle',0), (5,'plain',1,0,0,0,'f32',0,1,0,0,0,'half',0), (5,'plain',1,0,0,0,'f32',0,1,0,0,0,'straddle',0),
    (5,'plain',1,0,0,0,'f32',0,1,0,0,0,'straddle',1), (5,'plain',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (5,'plain',1,0,0,0,'f32',0,1,1,0,0,'half',1),
    (5,'plain',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (5,'plain',1,0,0,0,'f32',0,1,1,0,0,'straddle',1), (5,'plain',1,0,0,0,'f32',0,1,1,0,0,'whole',1),
    (5,'plain',1,0,0,1,'f32',0,1,0,1,0,'half',0), (5,'plain',1,0,0,1,'f32',0,1,0,1,0,'straddle',0), (5,'plain',1,0,0,1,'f32',0,1,0,1,0,'whole',0),
    (5,'plain',1,0,0,1,'f32',0,1,1,0,0,'half',0), (5,'plain',1,0,1,0,'f32',0,1,0,0,0,'half',0), (5,'plain',1,0,1,0,'f32',0,1,0,0,0,'straddle',0),
    (5,'plain',1,0,1,0,'f32',0,1,1,0,0,'half',0), (5,'plain',1,0,1,0,'f32',0,1,1,0,0,'half',1), (5,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',0),
    (5,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',1), (5,'plain',1,0,1,1,'f32',0,1,0,1,0,'half',0), (5,'plain',1,0,1,1,'f32',0,1,0,1,0,'straddle',0),
    (5,'plain',1,0,1,1,'f32',0,1,1,0,0,'half',0), (5,'tconv',1,0,0,0,'f16',0,0,1,0,1,'straddle',0), (5,'tconv',1,0,0,0,'f16',0,0,1,0,1,'straddle',1),
    (5,'tconv',1,0,0,0,'f16',0,0,1,0,1,'whole',1), (5,'tconv',1,0,0,0,'f32',0,1,0,0,0,'half',1), (5,'tconv',1,0,0,0,'f32',0,1,0,0,0,'straddle',0),
    (5,'tconv',1,0,0,0,'f32',0,1,0,0,0,'straddle',1), (5,'tconv',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (5,'tconv',1,0,0,0,'f32',0,1,1,0,0,'half',0),
    (5,'tconv',1,0,0,0,'f32',0,1,1,0,0,'straddle',0), (5,'tconv',1,0,0,0,'f32',0,1,1,0,0,'whole',0), (5,'tconv',1,0,0,1,'f16',0,0,1,0,1,'half',0),
    (5,'tconv',1,0,0,1,'f16',0,0,1,0,1,'straddle',0), (5,'tconv',1,0,0,1,'f16',0,0,1,0,1,'whole',0), (5,'tconv',1,0,0,1,'f32',0,1,0,1,0,'half',0),
    (5,'tconv',1,0,0,1,'f32',0,1,0,1,0,'straddle',0), (5,'tconv',1,0,0,1,'f32',0,1,0,1,0,'whole',0), (5,'tconv',1,0,1,0,'f16',0,0,1,0,1,'straddle',0),
    (5,'tconv',1,0,1,0,'f32',0,1,0,0,0,'half',0), (5,'tconv',1,0,1,0,'f32',0,1,0,0,0,'half',1), (5,'tconv',1,0,1,0,'f32',0,1,0,0,0,'straddle',0),
    (5,'tconv',1,0,1,0,'f32',0,1,0,0,0,'straddle',1), (5,'tconv',1,0,1,0,'f32',0,1,1,0,0,'half',0), (5,'tconv',1,0,1,0,'f32',0,1,1,0,0,'straddle',0),
    (5,'tconv',1,0,1,1,'f16',0,0,1,0,1,'half',0), (5,'tconv',1,0,1,1,'f16',0,0,1,0,1,'straddle',0), (5,'tconv',1,0,1,1,'f32',0,1,0,1,0,'half',0),
    (5,'tconv',1,0,1,1,'f32',0,1,0,1,0,'straddle',0), (5,'tconv',1,1,0,1,'f32',0,1,0,1,0,'whole',0),
    (8,'conv',1,0,0,0,'f16',1,0,1,0,1,'half',0), (8,'conv',1,0,0,0,'f16',1,0,1,0,1,'half',1), (8,'conv',1,0,0,0,'f16',1,0,1,0,1,'straddle',1),
    (8,'conv',1,0,0,0,'f16',1,0,1,0,1,'whole',0), (8,'conv',1,0,0,0,'f16',1,0,1,0,1,'whole',1), (8,'conv',1,0,0,0,'f32',0,1,0,0,0,'straddle',0),
    (8,'conv',1,0,0,0,'f32',0,1,0,0,0,'straddle',1), (8,'conv',1,0,0,0,'f32',0,1,0,0,0,'whole',0), (8,'conv',1,0,0,0,'f32',0,1,0,0,0,'whole',1),
    (8,'conv',1,0,0,0,'f32',0,1,0,1,0,'whole',0), (8,'conv',1,0,0,0,'f32',0,1,0,1,0,'whole',1), (8,'conv',1,0,0,0,'f32',0,1,1,0,0,'straddle',0),
    (8,'conv',1,0,0,0,'f32',0,1,1,0,0,'straddle',1), (8,'conv',1,0,0,0,'f32',0,1,1,0,0,'whole',1), (8,'conv',1,0,1,0,'f16',1,0,1,0,1,'straddle',0),
    (8,'conv',1,0,1,0,'f16',1,0,1,0,1,'straddle',1), (8,'conv',1,0,1,0,'f32',0,1,0,0,0,'straddle',0), (8,'conv',1,0,1,0,'f32',0,1,0,0,0,'straddle',1),
    (8,'conv',1,0,1,0,'f32',0,1,0,1,0,'straddle',0), (8,'conv',1,0,1,0,'f32',0,1,1,0,0,'straddle',0), (8,'conv',1,0,1,0,'f32',0,1,1,0,0,'straddle',1),
    (8,'conv',2,0,0,0,'f32',0,0,1,0,0,'half',0), (8,'conv',2,0,0,0,'f32',0,0,1,0,0,'half',1), (8,'conv',2,0,0,0,'f32',0,0,1,0,0,'straddle',0),
    (8,'conv',2,0,0,0,'f32',0,0,1,0,0,'straddle',1), (8,'conv',2,0,0,0,'f32',0,0,1,0,0,'whole',0), (8,'conv',2,0,1,0,'f32',0,0,1,0,0,'straddle',0),
    (8,'conv',2,0,1,0,'f32',0,0,1,0,0,'straddle',1), (8,'plain',1,0,0,0,'f32',0,1,0,0,0,'straddle',1), (8,'plain',1,0,0,0,'f32',0,1,0,0,0,'whole',0),
    (8,'plain',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (8,'plain',1,0,0,0,'f32',0,1,0,1,0,'whole',1), (8,'plain',1,0,0,0,'f32',0,1,1,0,0,'half',0),
    (8,'plain',1,0,0,0,'f32',0,1,1,0,0,'half',1), (8,'plain',1,0,0,0,'f32',0,1,1,0,0,'straddle',1), (8,'plain',1,0,0,0,'f32',0,1,1,0,0,'whole',0),
    (8,'plain',1,0,0,0,'f32',0,1,1,0,0,'whole',1), (8,'plain',1,0,1,0,'f32',0,1,0,0,0,'straddle',1), (8,'plain',1,0,1,0,'f32',0,1,0,1,0,'straddle',0),
    (8,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',0), (8,'plain',1,0,1,0,'f32',0,1,1,0,0,'straddle',1), (8,'tconv',1,0,0,0,'f16',0,0,1,0,1,'straddle',1),
    (8,'tconv',1,0,0,0,'f16',0,0,1,0,1,'whole',1), (8,'tconv',1,0,0,0,'f32',0,1,0,0,0,'half',0), (8,'tconv',1,0,0,0,'f32',0,1,0,0,0,'half',1),
    (8,'tconv',1,0,0,0,'f32',0,1,0,0,0,'straddle',0), (8,'tconv',1,0,0,0,'f32',0,1,0,0,0,'straddle',1), (8,'tconv',1,0,0,0,'f32',0,1,0,0,0,'whole',0),
    (8,'tconv',1,0,0,0,'f32',0,1,0,0,0,'whole',1), (8,'tconv',1,0,0,0,'f32',0,1,0,1,0,'straddle',1), (8,'tconv',1,0,0,0,'f32',0,1,0,1,0,'whole',0),
    (8,'tconv',1,0,0,0,'f32',0,1,0,1,0,'whole',1), (8,'tconv',1,0,1,0,'f16',0,0,1,0,1,'straddle',0), (8,'tconv',1,0,1,0,'f16',0,0,1,0,1,'straddle',1),
    (8,'tconv',1,0,1,0,'f32',0,1,0,0,0,'straddle',1), (8,'tconv',1,0,1,0,'f32',0,1,0,1,0,'straddle',0), (8,'tconv',1,0,1,0,'f32',0,1,0,1,0,'straddle',1),
    (8,'tconv',1,1,0,0,'f32',0,1,0,1,0,'whole',0), (8,'tconv',1,1,0,0,'f32',0,1,0,1,0,'whole',1),
]
for _n, _e in enumerate(_LOWERED_EPI):
    CASES.append(_case("lowered_epi", "lowered-epi-t%d-%s%s%s%s%s-%s%s%s%s%s%s-%s%s" % (
        _e[0], _e[1], "-s2" if _e[2] == 2 else "", "-halo" if _e[3] else "", "-mr" if _e[4] else "", "-nr" if _e[5] else "", _e[6], "-rowbias" if _e[7] else "",
        "-res" if _e[8] else "", "-silu" if _e[9] else "", "-lo" if _e[10] else "", "-dead" if _e[11] else "", _e[12], "-chunked" if _e[13] else ""),
        ("marked", "distinct")[_n % 2], tile=_e[0], kind=_e[1], stride=_e[2], halo=bool(_e[3]), m_ragged=_e[4], n_ragged=_e[5], out=_e[6], rowbias=_e[7],
        res=bool(_e[8]), silu=bool(_e[9]), lo=bool(_e[10]), x_dead=bool(_e[11]), seam=_e[12], chunked=_e[13], seed=900 + _n))
# ... the reduction launch of a split-K GEMM with T2V_EPI_GN: (rows per thread, out dtype, row bias, residual, SiLU, low-order image, dead result)
_LOWERED_SPLITK = [
    (1, 'f16', 0, 0, 1, 0, 1),
    (1, 'f16', 1, 0, 1, 0, 1),
    (1, 'f32', 0, 0, 1, 0, 0),
    (1, 'f32', 0, 1, 0, 0, 0),
    (1, 'f32', 0, 1, 0, 1, 0),
    (1, 'f32', 0, 1, 1, 0, 0),
    (1, 'f32', 1, 0, 1, 0, 1),
    (12, 'f16', 1, 0, 1, 0, 1),
    (12, 'f32', 0, 0, 1, 0, 0),
    (12, 'f32', 0, 1, 1, 0, 0),
    (2, 'f16', 0, 0, 1, 0, 1),
    (2, 'f16', 1, 0, 1, 0, 1),
    (2, 'f32', 0, 0, 1, 0, 0),
    (2, 'f32', 0, 1, 0, 0, 0),
    (2, 'f32', 0, 1, 1, 0, 0),
    (4, 'f16', 1, 0, 1, 0, 1),
    (4, 'f32', 0, 0, 1, 0, 0),
    (4, 'f32', 0, 1, 0, 0, 0),
    (4, 'f32', 0, 1, 1, 0, 0),
    (8, 'f16', 1, 0, 1, 0, 1),
    (8, 'f32', 0, 0, 1, 0, 0),
    (8, 'f32', 0, 1, 0, 0, 0),
    (8, 'f32', 0, 1, 1, 0, 0),
]
# ... of the requestable lattice (tests/geometry_lattice.py): KR is the first count of norm.hip:788 t2v_launch_splitk_reduce_gn's list
# (1, 2, 4, 8, 12, 16, 20) whose grid is at most one workgroup per CU — other instance sizes take 16 and 20 and meet the other epilogues
_LOWERED_SPLITK += [
    (12, 'f32', 0, 1, 0, 0, 0),
    (16, 'f16', 1, 0, 1, 0, 1),
    (16, 'f32', 0, 0, 1, 0, 0),
    (20, 'f16', 1, 0, 1, 0, 1),
    (20, 'f32', 0, 0, 1, 0, 0),
    (4, 'f16', 0, 0, 1, 0, 1),
    (4, 'f32', 0, 1, 0, 1, 0),
    (8, 'f32', 0, 1, 0, 1, 0),
]
for _n, _e in enumerate(_LOWERED_SPLITK):
    CASES.append(_case("lowered_splitk", "lowered-splitk-KR%d-%s%s%s%s%s%s" % (_e[0], _e[1], "-rowbias" if _e[2] else "", "-res" if _e[3] else "",
                                                                               "-silu" if _e[4] else "", "-lo" if _e[5] else "", "-dead" if _e[6] else ""),
                       ("marked", "distinct")[_n % 2], kr=_e[0], out=_e[1], rowbias=_e[2], res=bool(_e[3]), silu=bool(_e[4]), lo=bool(_e[5]), x_dead=bool(_e[6]),
                       seed=1100 + _n))
# ... the fused LayerNorm outputs (`offset` rows only where a residual closes the gap to the designed tensor: an fp16 operand of mean / std = 32
# rows has lost the designed spread): (tile, i[8], M ragged, N ragged, residual, residual wrap i[12], more tiles than the co-residency bound)
_LOWERED_LN = [
    (0, 2, 0, 0, 0, 0, 0),
    (0, 2, 0, 0, 1, 0, 0),
    (0, 2, 1, 0, 0, 0, 0),
    (0, 2, 1, 0, 1, 0, 0),
    (11, 1, 0, 0, 0, 0, 0),
    (11, 1, 0, 0, 1, 0, 0),
    (12, 2, 0, 0, 0, 0, 0),
    (12, 2, 0, 0, 0, 0, 1),
    (12, 2, 0, 0, 1, 0, 0),
    (12, 2, 0, 0, 1, 0, 1),
    (12, 2, 0, 0, 1, 1, 0),
    (12, 2, 1, 0, 0, 0, 0),
    (12, 2, 1, 0, 1, 0, 0),
    (2, 1, 0, 0, 0, 0, 0),
    (2, 1, 0, 0, 1, 0, 0),
    (3, 2, 0, 0, 0, 0, 0),
    (3, 2, 0, 0, 1, 0, 0),
    (3, 2, 0, 1, 0, 0, 0),
    (3, 2, 0, 1, 1, 0, 0),
    (3, 2, 1, 0, 0, 0, 0),
    (3, 2, 1, 0, 1, 0, 0),
    (5, 2, 0, 0, 0, 0, 0),
    (5, 2, 0, 0, 0, 0, 1),
    (5, 2, 0, 0, 1, 0, 0),
    (5, 2, 0, 0, 1, 0, 1),
    (5, 2, 1, 0, 0, 0, 0),
    (5, 2, 1, 0, 0, 0, 1),
    (5, 2, 1, 0, 1, 0, 0),
    (5, 2, 1, 0, 1, 0, 1),
    (8, 1, 0, 0, 0, 0, 0),
    (8, 1, 0, 0, 1, 0, 0),
    (8, 1, 1, 0, 0, 0, 0),
    (8, 1, 1, 0, 1, 0, 0),
    (9, 2, 0, 0, 0, 0, 1),
    (9, 2, 0, 0, 1, 0, 1),
    (9, 2, 1, 0, 0, 0, 0),
    (9, 2, 1, 0, 0, 0, 1),
    (9, 2, 1, 0, 1, 0, 0),
    (9, 2, 1, 0, 1, 0, 1),
    (9, 2, 1, 1, 0, 0, 1),
    (9, 2, 1, 1, 1, 0, 1),
]
# ... of the requestable lattice: the same fused LayerNorms on the tiles other row counts select, ragged in M and N, and cut into row chunks
# (lnx_chunked: more tiles than program.py's co-residency bound, per_cu x CUs or the record region)
_LOWERED_LN += [
    (0, 2, 0, 0, 0, 0, 1),
    (0, 2, 0, 0, 1, 0, 1),
    (0, 2, 1, 0, 0, 0, 1),
    (0, 2, 1, 0, 1, 0, 1),
    (11, 1, 1, 0, 0, 0, 0),
    (11, 1, 1, 0, 1, 0, 0),
    (12, 2, 1, 0, 0, 0, 1),
    (12, 2, 1, 0, 1, 0, 1),
    (2, 1, 1, 0, 0, 0, 0),
    (2, 1, 1, 0, 1, 0, 0),
    (3, 2, 0, 1, 0, 0, 1),
    (3, 2, 0, 1, 1, 0, 1),
    (3, 2, 1, 1, 0, 0, 0),
    (3, 2, 1, 1, 0, 0, 1),
    (3, 2, 1, 1, 1, 0, 0),
    (3, 2, 1, 1, 1, 0, 1),
    (5, 2, 0, 1, 0, 0, 0),
    (5, 2, 1, 1, 0, 0, 0),
    (9, 2, 0, 0, 0, 0, 0),
    (9, 2, 0, 0, 1, 0, 0),
    (9, 2, 0, 1, 0, 0, 1),
    (9, 2, 0, 1, 1, 0, 1),
]
for _n, _e in enumerate(_LOWERED_LN):
    CASES.append(_case("lowered_ln", "lowered-ln%d-t%d%s%s%s%s%s" % (_e[1], _e[0], "-mr" if _e[2] else "", "-nr" if _e[3] else "", "-res" if _e[4] else "",
                                                                      "-wrap" if _e[5] else "", "-chunked" if _e[6] else ""),
                       ("distinct", "offset")[_n % 2 if _e[4] else 0], tile=_e[0], mode=_e[1], m_ragged=_e[2], n_ragged=_e[3], res=bool(_e[4]), wrap=_e[5], chunked=_e[6], seed=1200 + _n))
# ... of the requestable lattice, stand-alone GroupNorm records (the fields of _LOWERED_GN; last in the list: the seeds above count the cases
# before them).  KR: norm.hip:629 coop_chunking takes the first of (4, 8, 12, 16, 20) whose grid is at most one workgroup per CU, so every
# latent size has its own; `cols_loop` (C = 2560: more than 256 column vectors, norm.hip:895 R = 1) meets each of them at the 8 x 8-level
# of a large latent.  `coop-fallback-one-block`: no KR fits and an instance is one statistics block (norm.hip:893 g1)
_lowered_gn_cases([
    ('coop-fallback', 'f32', 1, 0, 0, 0, 0, 1),
    ('coop-fallback-one-block', 'f16', 1, 0, 0, 0, 0, 0),
    ('coop-fallback-one-block', 'f32', 0, 0, 0, 0, 0, 0),
    ('coop-fallback-one-block', 'f32', 0, 1, 0, 0, 0, 0),
    ('coop-fallback-one-block', 'f32', 1, 0, 0, 0, 0, 0),
    ('coop-fallback-one-block', 'f32', 1, 0, 2, 0, 0, 0),
    ('coop-fallback-one-block', 'f32', 1, 0, 2, 0, 0, 1),
    ('cooperative', 'f16', 1, 0, 0, 20, 0, 0),
    ('cooperative', 'f32', 0, 0, 0, 12, 0, 0),
    ('cooperative', 'f32', 0, 0, 0, 20, 0, 0),
    ('cooperative', 'f32', 0, 1, 0, 12, 0, 0),
    ('cooperative', 'f32', 0, 1, 0, 20, 0, 0),
    ('cooperative', 'f32', 1, 0, 0, 12, 0, 1),
    ('cooperative', 'f32', 1, 0, 0, 16, 0, 1),
    ('cooperative', 'f32', 1, 0, 2, 12, 0, 1),
    ('cooperative', 'f32', 1, 0, 2, 16, 0, 1),
    ('cooperative', 'f32', 1, 0, 2, 20, 0, 0),
    ('cooperative', 'f32', 1, 0, 2, 20, 0, 1),
    ('cooperative', 'f32', 1, 0, 2, 4, 0, 1),
    ('cooperative', 'f32', 1, 0, 2, 8, 0, 0),
    ('cooperative', 'f32', 1, 0, 2, 8, 0, 1),
])
# the strip-fed norm with the workgroup fold (norm.hip:933: more than 1024 strip sums per instance) on an fp16 stream without a low-order image
CASES.append(_case("strips", "lowered-strips-wg-2x832x1280-f16", "marked", n_inst=2, rows=832, C=1280, wide=True, dt="f16", lo=False, seed=304))
assert len({c["id"] for c in CASES}) == len(CASES)
