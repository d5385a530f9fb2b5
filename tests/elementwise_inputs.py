"""TEST INFRASTRUCTURE — adversarial inputs for every layout, pointwise and sampler-update kernel of csrc/elementwise.hip and for
softmax_rows_kernel (csrc/attention.hip), float64 references written out from the formulas in the kernels' comments, and the case list with
the programs (or, for the sampler bindings, the single op) that run them.  No test functions here: tests/test_elementwise_inputs_cpu.py
proves on the CPU what the inputs do (and runs every case through the interpreter), tests/test_gpu_elementwise_adversarial.py runs the same
cases on the GPU.  Both import CASES / build(), so they cannot drift apart.  Nothing here touches a GPU or imports tests/interp.py: whoever
executes a case hands its arena view (`it`, anything with Interp's `mat`) to `Built.init` / `verify`.

Segments.  Every error is taken per segment and asserted on the maximum over segments: a (sample, channel, frame) line of HW pixels for the
layout conversions, a row for copy2d and softmax, a (sample, channel) row of `inner` values for ddim_step, a run of 256 consecutive elements
for lincomb, a (sample, cos | sin half) for time_embed, a frame for depth_tokens, an output token for avgpool2 (to_uint8 is bit-exact over
the whole video: one segment).

Distinct inputs.  Every segment has its own power-of-two scale from a cycle of 7 (1/8 .. 8; the exponent is (i0 + 2 i1 + 3 i2) % 7 - 3 of the
segment's indices, so segments that are neighbours along ANY index differ by a factor >= 2) and its elements carry random signs and
magnitudes in [0.75, 1.25) x scale: a value fetched from a neighbouring segment is never a rounding error.  Inputs are rounded to the input
dtype before the reference sees them; shapes are non-powers-of-two with F != HW != C.  copy2d, softmax, to_uint8 and depth_tokens have inputs
of their own (see their builders).

Fencing.  Every arena tensor an op reads or writes is a window of a larger allocation: NaN rows in front and behind, NaN columns to the
right where the op's record has a leading dimension (dense tensors: NaN elements in front and behind); uint8 outputs are fenced with the byte
0xA5.  Outputs start as NaN; `verify` wants every checked output finite (except where a case expects NaN) and every fence element untouched.
The sampler bindings (samplers._ddim_update, _ddim_update_blend, _lincomb) get views into larger NaN-filled tensors in the same way.

Wrap cases.  grid_for() caps every grid at 8192 workgroups of 256 threads; `*-wrap` cases have 2 097 152 work units plus a ragged
remainder, so the second pass of the grid-stride loop runs; the inputs only that pass reads are 16 x larger and all negative.

Out of scope: embed_rows, reshard_rows and resample — their tests already demand bit equality with an explicit expectation at strided and
ragged shapes."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd.program import NULL, Op, Program, Ref

NAN = float("nan")
TD = {"f16": torch.float16, "f32": torch.float32, "u8": torch.uint8}
DT = {"f16": L.F16, "f32": L.F32}
PAD_ROWS, PAD_FLAT, U8_FENCE = 3, 64, 0xA5
GRID_UNITS = 8192 * 256
TOL_TIME, TOL_SOFTMAX, TOL_F32ACT, TOL_DDIM32, TOL_DDIM16 = 2e-3, 1e-3, 1e-5, 1e-6, 1e-3      # the suite's figures for these ops


# ---- small numerics -----------------------------------------------------------------------------------------------------------------------
def ulp16(v):
    """One fp16 ulp at |v| (2^-24 for denormals), float64."""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -14))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), (e - 1).clamp_min(-14) - 10)


def seg_scale(*idx):
    """Power-of-two scale 1/8 .. 8 of the segment with indices idx (broadcast tensors): neighbours along any index differ."""
    e = sum((k + 1) * i for k, i in enumerate(idx))
    return torch.exp2(((e % 7) - 3).double())


def body(shape, gen):
    """Random signs x magnitudes in [0.75, 1.25), float64."""
    sign = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=gen).double()
    return sign * (0.75 + 0.5 * torch.rand(shape, generator=gen, dtype=torch.float64))


def rnd(x, dt):
    return x.to(TD[dt]).double()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


# ---- criteria: got -> one ratio per segment (error / bound; > 1 fails) -----------------------------------------------------------------
class Crit:
    def __init__(self, label, fn, unit=None):
        self.label, self.fn, self.unit = label, fn, unit          # unit: the bound of a ratio that is a plain figure (rel-L2 tolerances)


def c_exact(want, seg):
    """Bit equality with `want` (NaN matches NaN): ratio inf for a segment with a differing element, else 0."""
    def fn(got):
        assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
        same = _bits(got) == _bits(want)
        if got.is_floating_point():
            same = same | (torch.isnan(got) & torch.isnan(want))
        bad = seg((~same).double()).amax(dim=-1)
        return torch.where(bad > 0, torch.full_like(bad, float("inf")), bad)
    return Crit("bits", fn)


def _err(got, ref):
    e = (got.double() - ref).abs()
    return torch.where(torch.isfinite(got.double()), e, torch.full_like(e, float("inf")))


def c_rel_l2(ref, seg, tol, label="relL2"):
    """Per-segment rel-L2 against ref (float64) over tol; tol a number or one per segment."""
    def fn(got):
        e = seg(_err(got, ref)).norm(dim=-1) / seg(ref).norm(dim=-1).clamp_min(1e-30)
        return torch.nan_to_num(e, nan=float("inf")) / tol
    return Crit(label, fn, tol if isinstance(tol, float) else None)


def c_elem(ref, bound, seg, label):
    """Per element |got - ref| <= bound (float64 tensors): the segment's worst ratio."""
    def fn(got):
        return torch.nan_to_num(seg(_err(got, ref) / bound).amax(dim=-1), nan=float("inf"))
    return Crit(label, fn)


def rows_seg(t):
    return t.reshape(t.shape[0], -1)


def one_seg(t):
    return t.reshape(1, -1)


def runs_seg(t):
    """Runs of 256 consecutive elements (the last one padded with zeros)."""
    f = t.reshape(-1)
    pad = (-f.numel()) % 256
    return torch.cat([f, f.new_zeros(pad)]).view(-1, 256)


# ---- a built case ---------------------------------------------------------------------------------------------------------------------------
class Built:
    """A case's program (or sampler op), weights, initial contents, fences and checks."""

    def __init__(self, case):
        self.case = case
        self.P = Program()
        self.w = {}
        self.fences = []        # dict(big, r0, r1, c0, c1): the window inside an arena allocation; the rest keeps its fill
        self.sets = []          # (window, tensor) written before the run
        self.ext = {}           # name -> dict(big, off, n, shape): fenced flat tensors of the sampler bindings (slot numbers in .slots)
        self.slots = {}
        self.ops = None         # sampler cases: the op records the interpreter runs (mirrors of what the bindings fill in)
        self.call = None        # sampler cases: call(samplers module, {name: view}) performs the launches
        self.checks = []        # dict(name, get, crits, exact): get(rd) -> the tensor the criteria judge
        self.mutations = lambda: []      # -> [(what, {check name: mutated output}, {check name: affected-segment mask or None})]
        self.notes = {}         # extra figures for the ELTADV line (e32 ...)
        self.path = ""
        self.adapter = False    # needs the interpreter's adapter records (DEPTH_TOKENS, AVGPOOL2)

    # arena tensors
    def fenced(self, rows, cols, dtype, pad_cols=4):
        big = self.P.alloc(rows + 2 * PAD_ROWS, cols + pad_cols, dtype)
        self.fences.append(dict(big=big, r0=PAD_ROWS, r1=PAD_ROWS + rows, c0=0, c1=cols))
        return big.row_slice(PAD_ROWS, PAD_ROWS + rows).col_slice(0, cols)

    def flat(self, n, dtype):
        """A dense tensor of n elements with PAD_FLAT fence elements either side, as a [1, n] window."""
        big = self.P.alloc(1, n + 2 * PAD_FLAT, dtype)
        self.fences.append(dict(big=big, r0=0, r1=1, c0=PAD_FLAT, c1=PAD_FLAT + n))
        return big.col_slice(PAD_FLAT, PAD_FLAT + n)

    def put(self, win, t):
        assert win.rows * win.cols == t.numel(), (win.rows, win.cols, t.shape)
        self.sets.append((win, t.reshape(win.rows, win.cols)))

    def weight(self, name, t):
        self.w[name] = t
        return Ref("weight", 0, name)

    # fenced tensors of the sampler bindings
    def xflat(self, name, slot, dtype, n, value=None):
        big = torch.full((n + 2 * PAD_FLAT,), NAN, dtype=TD[dtype])
        if value is not None:
            big[PAD_FLAT: PAD_FLAT + n] = value.reshape(-1).to(TD[dtype])
        self.ext[name] = dict(big=big, off=PAD_FLAT, n=n)
        self.slots[name] = slot
        return Ref("ext", slot)

    def xview(self, name, big=None):
        e = self.ext[name]
        return (e["big"] if big is None else big)[e["off"]: e["off"] + e["n"]]

    def ext_views(self):
        return {self.slots[k]: self.xview(k) for k in self.ext}

    def init(self, it):
        for f in self.fences:
            big = f["big"]
            it.mat(big.ref, big.rows, big.ld, big.ld, TD[big.dtype], {}).fill_(U8_FENCE if big.dtype == "u8" else NAN)
        for win, t in self.sets:
            it.mat(win.ref, win.rows, win.cols, win.ld, TD[win.dtype], {}).copy_(t.to(TD[win.dtype]))

    def check(self, name, get, crits, exact=False, ref=None, dt=None):
        """ref / dt: the float64 reference and the output format of a bounded check (the CPU file rounds the one to the other)."""
        self.checks.append(dict(name=name, get=get, crits=crits, exact=exact, ref=ref, dt=dt))

    def ratios(self, chk, got):
        return torch.stack([c.fn(got) for c in chk["crits"]]).amax(dim=0)


def win_of(win):
    return lambda rd: rd(win)


def verify(it, b):
    """Fences and every check of a finished run; -> {figure name: measured maximum}."""
    tag = b.case["id"]
    for f in b.fences:
        big = f["big"]
        full = it.mat(big.ref, big.rows, big.ld, big.ld, TD[big.dtype], {}).clone()
        keep = torch.ones_like(full, dtype=torch.bool)
        keep[f["r0"]:f["r1"], f["c0"]:f["c1"]] = False
        ok = (full == U8_FENCE) if big.dtype == "u8" else torch.isnan(full)
        assert bool(ok[keep].all()), f"{tag}: {int((~ok[keep]).sum())} fence elements written"
    for name, e in b.ext.items():
        outside = torch.cat([e["big"][: e["off"]], e["big"][e["off"] + e["n"]:]])
        assert bool(torch.isnan(outside).all()), f"{tag}: fence of {name} written"

    def rd(win):
        if isinstance(win, str):
            return b.xview(win).clone()
        return it.mat(win.ref, win.rows, win.cols, win.ld, TD[win.dtype], {}).clone()
    figs = {}
    for chk in b.checks:
        got = chk["get"](rd)
        for c in chk["crits"]:
            r = float(c.fn(got).max())
            key = f"{chk['name']}.{c.label}"
            figs[key] = r * c.unit if c.unit else r
            assert r <= 1.0, (tag, key, figs[key], "bound", c.unit if c.unit else "1 (ratio)")
    figs.update(b.notes)
    return figs


def figures_line(b, figs):
    f = lambda v: f"{v:.2e}" if isinstance(v, float) else str(v)
    return f"ELTADV {b.case['id']}: path [{b.path}] " + " ".join(f"{k} {f(v)}" for k, v in figs.items())


def second_pass(n_units, per_unit=1):
    """Mask over n_units * per_unit consecutive elements: those only the second pass of the grid-stride loop touches."""
    m = torch.zeros(n_units, dtype=torch.bool)
    m[GRID_UNITS:] = True
    return m.repeat_interleave(per_unit) if per_unit > 1 else m


def mark_wrap(x, mask):
    x = x.clone()
    x[mask] = -16.0 * x[mask].abs()
    return x


# ---- NCTHW_TO_CL ----------------------------------------------------------------------------------------------------------------------------
def layout_input(B, C, F, HW, seed):
    b, c, f = torch.arange(B).view(B, 1, 1, 1), torch.arange(C).view(1, C, 1, 1), torch.arange(F).view(1, 1, F, 1)
    return seg_scale(c, f, b) * body((B, C, F, HW), _gen(seed))


def ncthw_ref(X, B, C, F, HW, ld, scale, lo_mode, mut=None):
    """X [Bsrc, C, F, HW] (float64, representable) -> hi [B F HW, ld], lo (or None): v = fp32(x * scale) (the double product of two fp32 numbers
    is exact, so this is the kernel's fp32 product), hi = fp16(v), lo = fp16(v - hi); padding channels +0; sample b reads b % Bsrc."""
    Bsrc = X.shape[0]
    src = torch.arange(B) % Bsrc
    if mut == "clamp":
        src = torch.arange(B).clamp(max=Bsrc - 1)
    elif mut == "block":
        src = torch.arange(B) // (B // Bsrc)
    x = X[src]
    if mut == "swap":       # pixel index and frame index exchanged in the source address
        x = X[src].reshape(B, C, F * HW)[:, :, (torch.arange(HW).view(1, HW) * F + torch.arange(F).view(F, 1)).reshape(-1)].view(B, C, F, HW)
    s = 1.0 if mut == "noscale" else float(np.float32(scale))
    v32 = (x * s).float()
    hi = v32.half()
    lo = (v32 - hi.float()).half()
    if mut == "lozero":
        lo = torch.zeros_like(lo)
    elif mut == "looff":
        lo = lo.roll(-1, 1)
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(B * F * HW, C)
    out = torch.zeros(B * F * HW, ld, dtype=torch.float16)
    out[:, :C] = cl(hi)
    lo_out = None
    if lo_mode == "pad":
        out[:, C:2 * C] = cl(lo)
    elif lo_mode == "buf":
        lo_out = torch.zeros(B * F * HW, ld, dtype=torch.float16)
        lo_out[:, :C] = cl(lo)
    return out, lo_out, v32.double(), src


def _build_ncthw(c):
    b = Built(c)
    B, Bsrc, C, F, HW, ld, dt, scale, lo_mode = (c[k] for k in ("B", "Bsrc", "C", "F", "HW", "ld", "dt", "scale", "lo"))
    nsrc = Bsrc if Bsrc else B
    X = layout_input(nsrc, C, F, HW, c["seed"])
    if c.get("wrap"):
        X = mark_wrap(X, second_pass(B * F * HW).view(1, 1, F, HW).expand(nsrc, C, F, HW))
    X = rnd(X, dt)
    src = b.flat(X.numel(), dt)
    b.put(src, X)
    out = b.fenced(B * F * HW, ld, "f16", pad_cols=0)
    lo = b.fenced(B * F * HW, ld, "f16", pad_cols=0) if lo_mode == "buf" else None
    op = b.P.ncthw_to_cl("in", src.ref, dt, out, B=B, C=C, F=F, HW=HW, scale=scale, src_batch=Bsrc, lo=lo, lo_in_pad=lo_mode == "pad")
    assert op.kind == L.OP_NCTHW_TO_CL and op.i[5] == DT[dt] and op.i[6] == Bsrc and op.i[7] == (lo_mode == "pad") and op.i[4] == ld
    assert (op.p[2].space == "arena") == (lo_mode == "buf")
    seg = lambda t: t.reshape(B, F, HW, ld).permute(0, 3, 1, 2).reshape(B * ld * F, HW)
    want, want_lo, v, _ = ncthw_ref(X, B, C, F, HW, ld, scale, lo_mode)
    b.check("out", win_of(out), [c_exact(want, seg)], exact=True)
    if lo is not None:
        b.check("lo", win_of(lo), [c_exact(want_lo, seg)], exact=True)
    if lo_mode != "none":
        vcl = torch.zeros(B * F * HW, ld, dtype=torch.float64)
        vcl[:, :C] = v.permute(0, 2, 3, 1).reshape(-1, C)
        live = torch.zeros(ld, dtype=torch.bool)
        live[:C] = True
        bound = (vcl.abs() * 2.0 ** -21).clamp_min(2.0 ** -24)

        def hilo(rd):
            o = rd(out).double()
            l = rd(lo).double() if lo is not None else torch.cat([o[:, C:2 * C], o.new_zeros(o.shape[0], ld - C)], dim=1)
            return torch.where(live, o + l, torch.zeros_like(o))
        b.check("hi+lo", hilo, [c_elem(vcl, bound, seg, "x2^-21|v|")])

    def mutations():
        chan = torch.zeros(B, ld, F, dtype=torch.bool)

        def aff(samples, chans):
            m = chan.clone()
            m[samples.view(-1, 1, 1) & chans.view(1, -1, 1).expand(B, ld, F)] = True
            return m.reshape(-1)
        every, data = torch.ones(B, dtype=torch.bool), torch.arange(ld) < C
        lo_ch = (torch.arange(ld) >= C) & (torch.arange(ld) < 2 * C) if lo_mode == "pad" else data
        lo_name = "lo" if lo_mode == "buf" else "out"
        muts = []
        true_src = torch.arange(B) % nsrc
        for what, key in (("sample b read from min(b, Bsrc - 1)", "clamp"), ("sample b read from b // (B / Bsrc)", "block")):
            if Bsrc:
                o, l, _, s = ncthw_ref(X, B, C, F, HW, ld, scale, lo_mode, key)
                if bool((s != true_src).any()):
                    muts.append((what, {"out": o}, {"out": aff(s != true_src, data)}))
        if F > 1:
            o, l, _, _ = ncthw_ref(X, B, C, F, HW, ld, scale, lo_mode, "swap")
            muts.append(("f and pix swapped", {"out": o}, {"out": aff(every, data)}))
        if float(np.float32(scale)) != 1.0:
            o, l, _, _ = ncthw_ref(X, B, C, F, HW, ld, scale, lo_mode, "noscale")
            muts.append(("scale dropped", {"out": o}, {"out": aff(every, data)}))
        if lo_mode != "none":
            for what, key in (("lo all zero", "lozero"), ("lo one channel off", "looff")):
                o, l, _, _ = ncthw_ref(X, B, C, F, HW, ld, scale, lo_mode, key)
                muts.append((what, {lo_name: l if lo_mode == "buf" else o}, {lo_name: aff(every, lo_ch)}))
        return muts
    b.mutations = mutations
    b.path = f"OP_NCTHW_TO_CL in={dt} i[6]={Bsrc} i[7]={int(lo_mode == 'pad')} lo={lo_mode} ld={ld}" + (" grid-stride" if c.get("wrap") else "")
    return b


# ---- CL_TO_NCTHW ----------------------------------------------------------------------------------------------------------------------------
def _build_cl(c):
    b = Built(c)
    B, C, F, HW, ld, dt = (c[k] for k in ("B", "C", "F", "HW", "ld", "dt"))
    X = layout_input(B, C, F, HW, c["seed"])
    if c.get("wrap"):
        X = mark_wrap(X, second_pass(B * C * F * HW).view(B, C, F, HW))
    X = rnd(X, "f32")
    tok = X.permute(0, 2, 3, 1).reshape(B * F * HW, C)
    x = b.fenced(B * F * HW, C, "f32", pad_cols=ld - C)          # the padding channels c >= C are NaN: they must not reach the output
    b.put(x, tok)
    dst = b.flat(B * C * F * HW, dt)
    op = b.P.cl_to_ncthw("out", x, dst.ref, dt, B=B, C=C, F=F, HW=HW)
    assert op.kind == L.OP_CL_TO_NCTHW and op.i[4] == ld and op.i[5] == DT[dt]
    seg = lambda t: t.reshape(B * C * F, HW)
    b.check("out", win_of(dst), [c_exact(X.to(TD[dt]).reshape(1, -1), seg)], exact=True)

    def mutations():
        muts = []
        if ld != C:
            padded = torch.full((B * F * HW, ld), NAN, dtype=torch.float64)
            padded[:, :C] = tok
            wrong = padded.reshape(-1)[: B * F * HW * C].view(B, F, HW, C).permute(0, 3, 1, 2)
            muts.append(("ld taken as C", {"out": wrong.to(TD[dt]).reshape(1, -1)}, {"out": None}))
        # f and c exchanged when the output index is taken apart: element ((b C + c) F + f) is read as ((b F + f') C + c')
        r = torch.arange(B * C * F)
        cc, ff, bb = r % C, (r // C) % F, r // (C * F)
        if F > 1:
            wrong = tok.view(B, F, HW, C)[bb, ff, :, cc]
            muts.append(("f and c swapped", {"out": wrong.to(TD[dt]).reshape(1, -1)}, {"out": (cc != (r // F) % C) | (ff != r % F)}))
        return muts
    b.mutations = mutations
    b.path = f"OP_CL_TO_NCTHW out={dt} ld={ld}" + (" grid-stride" if c.get("wrap") else "")
    return b


# ---- TIME_EMBED -----------------------------------------------------------------------------------------------------------------------------
T_VALUES = (999.0, 981.0, 500.0, 1.0, 0.0)


def time_ref(t, fr, mut=None):
    """[B, dim] float64: cos | sin of the fp32 product t * f (exact in double, then rounded to fp32)."""
    if mut == "tnext":
        t = t.roll(-1)
    if mut == "foff":
        fr = fr.roll(-1)
    a = (t.double()[:, None] * fr.double()[None, :]).float().double()
    return torch.cat([torch.sin(a), torch.cos(a)] if mut == "swap" else [torch.cos(a), torch.sin(a)], dim=1)


def _build_time(c):
    b = Built(c)
    B, dim = c["B"], c["dim"]
    half = dim // 2
    t = torch.tensor([T_VALUES[(k + c["first"]) % 5] for k in range(B)])
    fr = torch.pow(10000, -torch.arange(half).to(torch.float32).div(half))          # the model's frequencies (unet.time_freqs)
    tw = b.flat(B, "f32")
    b.put(tw, t)
    out = b.fenced(B, dim, "f16", pad_cols=0)             # the record has no leading dimension: rows of `dim`
    op = b.P.time_embed("te", tw.ref, b.weight("fr", fr), out)
    assert op.kind == L.OP_TIME_EMBED and (op.i[0], op.i[1]) == (B, dim)
    ref = time_ref(t, fr)
    seg = lambda x: x.reshape(B * 2, half)
    ref16 = ref.half().double()
    b.check("out", win_of(out), [c_rel_l2(ref16, seg, TOL_TIME), c_elem(ref16, torch.full_like(ref, 2.0 ** -10), seg, "x2^-10")],
            ref=ref, dt="f16")
    zero = t == 0
    if bool(zero.any()):
        want = torch.cat([torch.ones(half), torch.zeros(half)]).half().expand(int(zero.sum()), dim)
        b.check("t=0 row", lambda rd: rd(out)[zero], [c_exact(want.contiguous(), one_seg)], exact=True)

    def mutations():
        nz = (~zero).repeat_interleave(2)
        muts = [("cos / sin swapped", {"out": time_ref(t, fr, "swap").half()}, {"out": None}),
                ("frequency index off by one", {"out": time_ref(t, fr, "foff").half()}, {"out": nz})]      # t = 0: cos 0 | sin 0 at any frequency
        if B > 1:
            muts.append(("t of the next sample", {"out": time_ref(t, fr, "tnext").half()}, {"out": None}))
        return muts
    b.mutations = mutations
    b.path = f"OP_TIME_EMBED B={B} dim={dim} units={B * half}"
    return b


# ---- COPY2D ---------------------------------------------------------------------------------------------------------------------------------
COPY_MAGS = [2.0 ** k for k in range(-10, 7)] + [80.0]


def act_ref(x, act):
    """float64: 0 identity, 1 SiLU, 2 GELU (erf), 3 quick GELU x sigmoid(1.702 x)."""
    if act == 1:
        return x / (1.0 + torch.exp(-x))
    if act == 2:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == 3:
        return x / (1.0 + torch.exp(-1.702 * x))
    return x


def copy_input(rows, cols, dt, seed):
    """Row r: magnitude COPY_MAGS[r % 18] x [0.5, 1], sign alternating by row; |x| <= 80."""
    r = torch.arange(rows)
    mag = torch.tensor(COPY_MAGS, dtype=torch.float64)[r % len(COPY_MAGS)]
    sign = (1.0 - 2.0 * (r % 2)).double()
    return rnd((sign * mag)[:, None] * (0.5 + 0.5 * torch.rand(rows, cols, generator=_gen(seed), dtype=torch.float64)), dt)


def _build_copy(c):
    b = Built(c)
    rows, cols, sdt, ddt, act, lo, form = (c[k] for k in ("rows", "cols", "sdt", "ddt", "act", "lo", "form"))
    X = copy_input(rows, cols, sdt, c["seed"])
    if c.get("wrap"):
        X = rnd(mark_wrap(X, second_pass(rows * cols // 4, 4).view(rows, cols)), sdt)
    lds, ldd = cols + 12, cols + 4
    sentinel = None
    if form == "inplace":
        src = dst = b.fenced(rows, cols, sdt, pad_cols=4)
        lds = ldd
    elif form == "concat":      # the skip-connection concat: columns 320 .. 451 of a 640-column buffer whose other columns must survive
        src = b.fenced(rows, cols, sdt, pad_cols=12)
        wide = b.fenced(rows, 640, ddt, pad_cols=4)
        sentinel = torch.full((rows, 640), 7.0, dtype=torch.float64) * seg_scale(torch.arange(rows))[:, None]
        b.put(wide, sentinel)
        dst, ldd = wide.col_slice(320, 320 + cols), 644
    else:
        src, dst = b.fenced(rows, cols, sdt, pad_cols=12), b.fenced(rows, cols, ddt, pad_cols=4)
    b.put(src, X)
    lo_w = b.fenced(rows, cols, "f16", pad_cols=4) if lo else None
    op = b.P.copy2d("cp", src, dst, act=act, lo=lo_w)
    assert op.kind == L.OP_COPY2D and (op.i[2], op.i[3], op.i[4], op.i[5], op.i[6]) == (lds, ldd, DT[sdt], DT[ddt], act)
    assert (op.p[2].space == "arena") == lo
    ref = act_ref(X, act)
    v32 = X.float()

    def crits_for(ref, act):
        if act == 0:
            return [c_exact(ref.to(TD[ddt]), rows_seg)], True
        if act == 2:     # Abramowitz-Stegun 7.1.26 by design: |erf error| <= 1.5e-7 (+ 2^-21 for the fast reciprocal and exponential)
            bound = 0.5 * X.abs() * (1.5e-7 + 2.0 ** -21)
            bound = bound + (torch.maximum(2.0 ** -11 * (ref.abs() + bound), torch.full_like(ref, 2.0 ** -25)) if ddt == "f16" else 2.0 ** -24 * (ref.abs() + bound))
            return [c_elem(ref, bound, rows_seg, "xAS7.1.26")], False
        if ddt == "f16":
            r16 = ref.half().double()
            return [c_elem(r16, ulp16(r16), rows_seg, "ulp16")], False
        return [c_rel_l2(ref, rows_seg, TOL_F32ACT)], False
    crits, exact = crits_for(ref, act)
    b.check("out", win_of(dst), crits, exact=exact, ref=None if exact else ref, dt=ddt)
    if lo:
        b.check("lo", win_of(lo_w), [c_exact((v32 - v32.half().float()).half(), rows_seg)], exact=True)
    if sentinel is not None:
        keep = torch.ones(640, dtype=torch.bool)
        keep[320:320 + cols] = False
        b.check("rest of the concat buffer", lambda rd: rd(wide)[:, keep], [c_exact(sentinel.to(TD[ddt])[:, keep].contiguous(), rows_seg)], exact=True)

    def mutations():
        muts = []
        other = 1 if act == 0 else 0
        # every activation here tends to the identity for large positive x: the rows that can tell are the negative ones and |x| <= 4
        r = torch.arange(rows)
        tells = (r % 2 == 1) | (torch.tensor(COPY_MAGS)[r % len(COPY_MAGS)] <= 4.0)
        if c.get("wrap"):
            tells = (X < 0).any(dim=1)
        muts.append((f"the activation of act {other}", {"out": act_ref(X, other).to(TD[ddt])}, {"out": tells}))
        if form != "inplace":      # destination rows addressed with the source's leading dimension
            width = 640 if form == "concat" else cols
            c0 = 320 if form == "concat" else 0
            mem = torch.full((rows * max(lds, ldd) + width + 16,), NAN, dtype=torch.float64)
            if sentinel is not None:
                mem[: rows * ldd].view(rows, ldd)[:, :640] = sentinel
            for r in range(rows):
                mem[r * lds + c0: r * lds + c0 + cols] = ref[r]
            wrong = mem[: rows * ldd].view(rows, ldd)[:, c0:c0 + cols]
            aff = torch.ones(rows, dtype=torch.bool)
            aff[0] = False
            muts.append(("lds used for ldd", {"out": wrong.to(TD[ddt])}, {"out": aff}))
        if lo:
            muts.append(("lo missing", {"lo": torch.zeros(rows, cols, dtype=torch.float16)}, {"lo": None}))
        return muts
    b.mutations = mutations
    b.path = f"OP_COPY2D {sdt}->{ddt} i[6]={act} lo={int(lo)} {form}" + (" grid-stride" if c.get("wrap") else "")
    return b


# ---- SOFTMAX --------------------------------------------------------------------------------------------------------------------------------
SOFTMAX_SCALE = 0.5


def softmax_input(rows, cols, seed):
    """x [rows, cols] fp32.  Row r: the logits x * 0.5 lie in [-spread_r, 0] with spread_r = 30 ln 2 / 2^(r % 3) (30, 15, 7.5 log2 units:
    neighbouring rows differ by 2 x); the maximum 0 sits at column 0, at the last column or — rows wider than 768 — at a column of the
    ragged tail c >= 768, by row, and every other logit is at least spread / 50 below it; the last row has all logits equal.
    In the row whose maximum is in the ragged tail the first 768 columns sit another 130 log2 units lower: softmax does not depend on
    which constant is subtracted, so a maximum taken over those columns only shows when exp(l - max) overflows fp32 (beyond 2^128) — a
    spread of 30 log2 units cannot expose it.  That row's output is the softmax of its tail."""
    g = _gen(seed)
    x = torch.empty(rows, cols, dtype=torch.float64)
    where = []
    for r in range(rows):
        spread = 30.0 * math.log(2.0) / 2 ** (r % 3)
        x[r] = -spread * (0.02 + 0.98 * torch.rand(cols, generator=g, dtype=torch.float64)) / SOFTMAX_SCALE
        pos = (0, cols - 1, 768 + (r * 37) % (cols - 769) if cols > 770 else cols // 2)[r % 3]
        if pos >= 768:
            x[r, :768] -= 130.0 * math.log(2.0) / SOFTMAX_SCALE
        x[r, pos] = 0.0
        where.append(pos)
    x[rows - 1] = -3.0 * rows
    where[rows - 1] = -1
    return rnd(x, "f32"), where


def softmax_ref(x, mut=None):
    """float64; the mutations in fp32, where the overflow of a wrong maximum happens."""
    l = x * SOFTMAX_SCALE if mut is None else (x * SOFTMAX_SCALE).float()
    mx = (l[:, :768] if mut == "max768" else l).amax(dim=1, keepdim=True)
    e = torch.exp(l - mx)
    return e / (e[:, :768] if mut == "sum768" else e).sum(dim=1, keepdim=True)


def _build_softmax(c):
    b = Built(c)
    rows, cols, ld_in, ld_out = c["rows"], c["cols"], c["ld_in"], c["ld_out"]
    X, where = softmax_input(rows, cols, c["seed"])
    x, out = b.fenced(rows, cols, "f32", pad_cols=ld_in - cols), b.fenced(rows, cols, "f16", pad_cols=ld_out - cols)
    b.put(x, X)
    op = b.P.softmax("sm", x, out, SOFTMAX_SCALE)
    assert op.kind == L.OP_SOFTMAX and list(op.i[0:4]) == [rows, cols, ld_in, ld_out]
    b.check("out", win_of(out), [c_rel_l2(softmax_ref(X), rows_seg, TOL_SOFTMAX)], ref=softmax_ref(X), dt="f16")

    def mutations():
        if cols <= 768:
            return []
        tail = torch.tensor([w >= 768 for w in where])
        wide = torch.ones(rows, dtype=torch.bool)
        # the maximum over the first 768 columns only OVERFLOWS: exp(l - max) is inf in fp32 at the true maximum (2^130 and more), the sum is
        # inf and the row comes out as NaN / 0
        return [("maximum over the first 768 columns only", {"out": softmax_ref(X, "max768").half()}, {"out": tail}),
                ("sum over the first 768 columns only", {"out": softmax_ref(X, "sum768").half()}, {"out": wide})]
    b.mutations = mutations
    b.path = f"OP_SOFTMAX {rows}x{cols} ld {ld_in}/{ld_out}"
    return b


# ---- DDIM_STEP (through samplers._ddim_update / _ddim_update_blend) ------------------------------------------------------------------------
def ddim_coefs(mode, which, eta, gscale):
    """The six coefficients (and, mode 1, the q_sample pair of the blend) of one step of a 50-step run on the SD linear schedule, computed as
    the samplers do: float64 tables cast to fp32 per lookup, then fp32 arithmetic (samplers.py DDIM loop; videocrafter.py DDIMSampler).
    which: 0 the first step, 1 one in the middle, 2 the last (a_prev = alphas_cumprod[0]).  With 1000 timesteps and 50 steps the first
    timestep is 981 and the last is 1."""
    f32 = torch.float32
    betas = tp.beta_schedule_linear_sd()
    ac = torch.cumprod(1 - betas, dim=0)
    stride = 1000 // 50
    if mode == 0:
        steps = (1 + torch.arange(0, 1000, stride)).clamp(0, 999).flip(0)
        t = int(steps[(0, 24, 49)[which]])
        a_t, a_prev = ac[t].to(f32), ac[max(t - stride, 0)].to(f32)
        sigma = eta * torch.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))
        coef = [float(torch.sqrt(1.0 / ac)[t].to(f32)), float(torch.sqrt(1.0 / ac - 1)[t].to(f32)), float(torch.sqrt(a_prev)),
                float(torch.sqrt(1 - a_prev - sigma ** 2)), float(sigma) if t != 0 else 0.0, gscale]
        return t, coef, None
    ac32 = ac.to(f32)                                     # the LVDM model keeps fp32 cumprods
    ts = np.asarray(list(range(0, 1000, stride))) + 1
    alphas, alphas_prev = ac32[ts], torch.cat([ac32[0:1], ac32[ts[:-1]]])
    a64, p64 = alphas.double(), alphas_prev.double()
    sigmas = eta * torch.sqrt((1 - p64) / (1 - a64) * (1 - a64 / p64))
    index = (49, 25, 0)[which]
    a_t, a_prev, sigma_t, s1m = alphas[index].to(f32), alphas_prev[index].to(f32), sigmas[index].to(f32), torch.sqrt(1.0 - alphas)[index].to(f32)
    coef = [float(s1m), float(a_t.sqrt()), float(a_prev.sqrt()), float((1.0 - a_prev - sigma_t ** 2).sqrt()), float(sigma_t), gscale]
    tq = int(ts[index]) - 1
    return int(ts[index]), coef, (float(torch.sqrt(ac32)[tq]), float(torch.sqrt(1.0 - ac32)[tq]))


def ddim_formula(x, y, u, noise, coef, gm, mode, blend=None, dt=torch.float64):
    """The update written out (x, y, u, noise [C, inner]; gm [C, 1] guided channels; coefficients are fp32 numbers):
    o = u + g (y - u) on guided channels, else y;  mode 0: x0 = a x - b o, eps = (a x - x0) / b, x' = c x0 + d eps;
    mode 1: x0 = (x - a o) / b, x' = c x0 + d o;  x' += sigma noise;  blend: x' = (q0 known + q1 qnoise) m + (1 - m) x'.
    dt = float32 is the plain torch restatement in the reference's operation order (the e32 yardstick)."""
    f = [torch.tensor(float(np.float32(v)), dtype=dt) for v in coef]
    x, y = x.to(dt), y.to(dt)
    o = y
    if u is not None:
        u = u.to(dt)
        o = torch.where(gm, u + f[5] * (y - u), y)
    if mode == 0:
        x0 = f[0] * x - f[1] * o
        eps = (f[0] * x - x0) / f[1]
        xn = f[2] * x0 + f[3] * eps
    else:
        x0 = (x - f[0] * o) / f[1]
        xn = f[2] * x0 + f[3] * o
    if noise is not None and float(coef[4]) != 0.0:
        xn = xn + f[4] * noise.to(dt)
    if blend is not None:
        known, m, qn, qc = blend
        k = torch.tensor(float(np.float32(qc[0])), dtype=dt) * known.to(dt)
        if qn is not None and float(qc[1]) != 0.0:
            k = k + torch.tensor(float(np.float32(qc[1])), dtype=dt) * qn.to(dt)
        xn = k * m.to(dt) + (1.0 - m.to(dt)) * xn
    return xn


def _build_ddim(c):
    b = Built(c)
    S, Cs, inner, guided, edt, xdt, mode, eta, which, gscale, blend = (c[k] for k in ("S", "Cs", "inner", "guided", "edt", "xdt", "mode", "eta", "which", "gscale", "blend"))
    C = S * Cs
    g = _gen(c["seed"])
    t, coef, qcoef = ddim_coefs(mode, which, eta, gscale)
    s_i, c_i = torch.arange(C).view(C, 1) // Cs, torch.arange(C).view(C, 1) % Cs
    scale = seg_scale(c_i, s_i)
    X, Y, U = scale * body((C, inner), g), scale * body((C, inner), g), scale * body((C, inner), g)      # |y - u| ~ |y|
    N = torch.randn(C, inner, generator=g, dtype=torch.float64)
    if c.get("wrap"):
        m = second_pass(C * inner).view(C, inner)
        X, Y, U = mark_wrap(X, m), mark_wrap(Y, m), mark_wrap(U, m)
    X, Y, U, N = rnd(X, xdt), rnd(Y, edt), rnd(U, edt), rnd(N, "f32")
    sigma_on = float(coef[4]) != 0.0
    gm = c_i < guided
    n = C * inner
    b.xflat("x", L.EXT_XT, xdt, n, X)
    b.xflat("eps", L.EXT_EPS, edt, 2 * n if guided else n, torch.cat([Y, U]) if guided else Y)      # unguided: the conditional half, then fence
    b.xflat("noise", L.EXT_NOISE, "f32", n, N if sigma_on else None)                                  # sigma = 0: NaN, must not be read
    b.xflat("out", L.EXT_XT_OUT, xdt, n)
    bl = None
    if blend:
        K = rnd(scale * body((C, inner), g), "f32")
        M = torch.tensor([0.0, 1.0, 0.25, 1.0])[torch.arange(C) % 4].double().view(C, 1).expand(C, inner).contiguous()
        Q = rnd(torch.randn(C, inner, generator=g, dtype=torch.float64), "f32") if blend == "qnoise" else None
        qc = qcoef if Q is not None else (qcoef[0], 0.0)
        b.xflat("known", 9, "f32", n, K)
        b.xflat("mask", 10, "f32", n, M)
        if Q is not None:
            b.xflat("qnoise", 11, "f32", n, Q)
        bl = (K, M, Q, qc)
    differential = 0 < guided < Cs
    if differential:
        b.xflat("out0", 12, xdt, n)

    def record(gd, out_slot):
        op = Op(L.OP_DDIM_STEP, "ddim")
        op.i[0:8] = [C, inner, gd, DT[edt], DT[xdt], mode, Cs, int(bool(blend))]
        op.f[0:6] = coef
        op.p[0:4] = [Ref("ext", L.EXT_XT), Ref("ext", L.EXT_EPS), Ref("ext", L.EXT_NOISE) if sigma_on else NULL, Ref("ext", out_slot)]
        if blend:
            op.f[6], op.f[7] = bl[3]
            op.p[4:7] = [Ref("ext", 9), Ref("ext", 10), Ref("ext", 11) if bl[2] is not None else NULL]
        return op
    b.ops = [record(guided, L.EXT_XT_OUT)] + ([record(0, 12)] if differential else [])
    shape = (S, Cs, inner)

    def call(Smod, v):
        sh = lambda k: v[k].view(shape)
        if blend:
            Smod._ddim_update_blend(sh("out"), sh("x"), v["eps"], sh("noise"), coef, guided, sh("known"), sh("mask"), sh("qnoise") if bl[2] is not None else None, bl[3])
        else:
            Smod._ddim_update(sh("out"), sh("x"), v["eps"], sh("noise"), coef, guided, mode)
        if differential:
            Smod._ddim_update(sh("out0"), sh("x"), v["eps"], sh("noise"), coef, 0, mode)
    b.call = call
    Nz = N if sigma_on else None
    Uz = U if guided else None
    ref = ddim_formula(X, Y, Uz, Nz, coef, gm, mode, bl)
    if xdt == "f32":
        r32 = ddim_formula(X.float(), Y.float(), None if Uz is None else Uz.float(), None if Nz is None else Nz.float(), coef, gm, mode,
                           None if bl is None else tuple(None if v is None else (v.float() if torch.is_tensor(v) else v) for v in bl), dt=torch.float32)
        e32 = rows_seg(r32.double() - ref).norm(dim=-1) / rows_seg(ref).norm(dim=-1)
        tol = torch.maximum(torch.full_like(e32, TOL_DDIM32), 4.0 * e32)
        b.notes["e32"] = float(e32.max())
        b.notes["bound"] = float(tol.max())
        # two criteria on the same figure: the bound (one per segment) and, with a bound of 1, the plain rel-L2 for the record
        crits = [c_rel_l2(ref, rows_seg, tol, "relL2/max(1e-6,4e32)"), c_rel_l2(ref, rows_seg, 1.0)]
    else:
        r16 = ref.half().double()
        crits = [c_rel_l2(ref, rows_seg, TOL_DDIM16), c_elem(r16, ulp16(r16), rows_seg, "ulp16")]
    b.check("out", lambda rd: rd("out").view(C, inner), crits, ref=ref, dt=xdt)
    if differential:
        ung = ~gm.view(-1)
        b.check("unguided channels of both launches", lambda rd: (_bits(rd("out").view(C, inner)[ung]) - _bits(rd("out0").view(C, inner)[ung])).to(torch.int32),
                [c_exact(torch.zeros(int(ung.sum()), inner, dtype=torch.int32), rows_seg)], exact=True)

    def mutations():
        every = torch.ones(C, dtype=torch.bool)
        gch, flat = gm.view(-1), torch.cat([Y.reshape(-1), U.reshape(-1)])
        cast = lambda r: {"out": r.to(TD[xdt])}
        open_ = every if not bl else (bl[1][:, 0] != 1.0)      # mask = 1: the channel is the known region whatever the step computed
        muts = [("the other mode's formula", cast(ddim_formula(X, Y, Uz, Nz, coef, gm, 1 - mode, bl)), {"out": open_})]
        if guided and gscale != 1.0:
            if guided < Cs:
                muts.append(("guidance on all channels", cast(ddim_formula(X, Y, Uz, Nz, coef, torch.ones_like(gm), mode, bl)), {"out": ~gch}))
            if S > 1 and guided < Cs:
                wrong = torch.arange(C).view(C, 1) < guided
                muts.append(("guidance on c < guided without % cps", cast(ddim_formula(X, Y, Uz, Nz, coef, wrong, mode, bl)), {"out": gch & ~wrong.view(-1)}))
        if guided:
            if S > 1 and gscale != 1.0:      # (g = 1: o = u + (y - u) = y whatever u is)
                u2 = flat[Cs * inner: Cs * inner + n].view(C, inner)
                muts.append(("the unconditional half taken at cps * inner", cast(ddim_formula(X, Y, u2, Nz, coef, gm, mode, bl)), {"out": gch}))
            muts.append(("cond / uncond swapped", cast(ddim_formula(X, U, Y, Nz, coef, gm, mode, bl)), {"out": gch}))
        if sigma_on:
            muts.append(("noise dropped", cast(ddim_formula(X, Y, Uz, None, coef, gm, mode, bl)), {"out": open_}))
        if S > 1:
            muts.append(("x of the next sample", cast(ddim_formula(X.roll(-Cs, 0), Y, Uz, Nz, coef, gm, mode, bl)), {"out": open_}))
        if bl:
            muts.append(("mask inverted", cast(ddim_formula(X, Y, Uz, Nz, coef, gm, mode, (bl[0], 1.0 - bl[1], bl[2], bl[3]))), {"out": every}))
            if bl[2] is not None:
                muts.append(("qnoise dropped", cast(ddim_formula(X, Y, Uz, Nz, coef, gm, mode, (bl[0], bl[1], None, bl[3]))), {"out": bl[1][:, 0] != 0.0}))
        return [(what, got, {k: m if what == "mask inverted" else m & open_ for k, m in aff.items()}) for what, got, aff in muts]
    b.mutations = mutations
    b.path = (f"OP_DDIM_STEP eps={edt} x={xdt} mode={mode} i[2]={guided} i[6]={Cs} i[7]={int(bool(blend))} S={S} t={t} sigma={'on' if sigma_on else 'off'}"
              + (f" q={blend}" if blend else "") + (" grid-stride" if c.get("wrap") else ""))
    return b


# ---- LINCOMB (through samplers._lincomb) ---------------------------------------------------------------------------------------------------
def _build_lincomb(c):
    b = Built(c)
    n, dts, odt = c["n"], c["terms"], c["out"]
    g = _gen(c["seed"])
    K = len(dts)
    run = seg_scale(torch.arange(n) // 256)
    coefs = [(-1.0) ** k * 2.0 ** (k - 2) for k in range(K)]          # +-2^k against term magnitudes 2^-k: every term weighs the same
    terms = [run * body((n,), g) * 2.0 ** -(k - 2) for k in range(K)]
    if c.get("cancel"):                                               # UniPC-like: the first two terms nearly opposite
        coefs[1] = -coefs[0] * 0.5
        terms[1] = terms[0] * 2.0 * (1.0 + 2.0 ** -9 * torch.rand(n, generator=g, dtype=torch.float64))
    if c.get("wrap"):
        terms = [mark_wrap(t, second_pass(n)) for t in terms]
    terms = [rnd(t, dt) for t, dt in zip(terms, dts)]
    for k in range(K):
        b.xflat(f"t{k}", 1 + k, dts[k], n, terms[k])
    b.xflat("out", 7, odt, n)
    op = Op(L.OP_LINCOMB, "lincomb")
    op.i[0:3] = [n, K, DT[odt]]
    for k in range(K):
        op.i[3 + k], op.f[k], op.p[k] = DT[dts[k]], coefs[k], Ref("ext", 1 + k)
    op.p[6] = Ref("ext", 7)
    b.ops = [op]
    b.call = lambda Smod, v: Smod._lincomb(v["out"], [(coefs[k], v[f"t{k}"]) for k in range(K)])

    def formula(cs, ts):
        return sum(cv * t for cv, t in zip(cs, ts))
    ref = formula(coefs, terms)
    mass = sum(abs(cv) * t.abs() for cv, t in zip(coefs, terms))
    bound = (K + 1) * 2.0 ** -24 * mass                               # sequential fp32 accumulation
    if odt == "f16":
        bound = bound + torch.maximum(2.0 ** -11 * (ref.abs() + bound), torch.full_like(ref, 2.0 ** -25))      # + the output rounding
    b.check("out", win_of("out"), [c_elem(ref, bound, runs_seg, "x(K+1)2^-24 sum|ct|")], ref=ref, dt=odt)

    def mutations():
        muts = []
        for k in range(K):
            if K > 1:
                muts.append((f"term {k} dropped", {"out": formula(coefs[:k] + coefs[k + 1:], terms[:k] + terms[k + 1:]).to(TD[odt])}, {"out": None}))
        if K > 1:
            muts.append(("coefficient k applied to term k + 1", {"out": formula(coefs, terms[1:] + terms[:1]).to(TD[odt])}, {"out": None}))
        return muts
    b.mutations = mutations
    b.path = f"OP_LINCOMB n={n} terms={'+'.join(dts)} out={odt}" + (" cancel" if c.get("cancel") else "") + (" grid-stride" if c.get("wrap") else "")
    return b


# ---- TO_UINT8 -------------------------------------------------------------------------------------------------------------------------------
def boundary_table(dt):
    """For every k in 0 .. 255 the `dt` value nearest the truncation boundary 2 k / 255 - 1 and its neighbours at +-1 and +-2 ulp, then -1.5, -1
    and 1 with their two neighbours, 3.0, +-0 and a denormal: finite values only.  float64 values representable in dt."""
    npdt = np.float32 if dt == "f32" else np.float16
    vals = []
    for k in range(256):
        v = npdt(2.0 * k / 255.0 - 1.0)
        lo1, hi1 = np.nextafter(v, npdt(-4)), np.nextafter(v, npdt(4))
        vals += [np.nextafter(lo1, npdt(-4)), lo1, v, hi1, np.nextafter(hi1, npdt(4))]
    for v in (npdt(-1.0), npdt(1.0)):
        vals += [np.nextafter(v, npdt(-4)), v, np.nextafter(v, npdt(4))]
    vals += [npdt(-1.5), npdt(3.0), npdt(0.0), npdt(-0.0), npdt(1e-40) if dt == "f32" else npdt(6e-8)]
    return torch.from_numpy(np.asarray(vals, dtype=npdt)).double()


def u8_video(dt, shape, seed):
    """[NI, C, F, H, W]: the boundary table(s) scattered over the video (fp32 inputs carry the fp32 AND the fp16 table: the HALF kernels round
    them to fp16 first), the rest uniform in (-1.2, 1.2)."""
    n = int(np.prod(shape))
    g = _gen(seed)
    tab = boundary_table(dt) if dt == "f16" else torch.cat([boundary_table("f32"), boundary_table("f16")])
    v = rnd(2.4 * torch.rand(n, generator=g, dtype=torch.float64) - 1.2, dt)
    k = min(n, tab.numel())
    v[torch.randperm(n, generator=g)[:k]] = tab[:k]
    return v.view(shape), k == tab.numel()


def u8_formula(video, half, bgr, mut=None):
    """tensor2vid written out (t2v_pipeline.py:447-460): v * 0.5 + 0.5 (two roundings), clamp to [0, 1], * 255, truncated; `half`: every
    intermediate rounded to fp16.  video [NI, C, F, H, W] fp32 / fp16 -> uint8 [F, H, NI * W, C]."""
    v = video.half() if half else video.float()
    if mut == "fp32once":
        s = ((v.float() * 0.5 + 0.5).clamp(0, 1) * 255).half().float()
    elif mut == "clamp_after":
        s = ((v * 0.5 + 0.5) * 255).clamp(0, 255).float()
    else:
        s = ((v * 0.5 + 0.5).clamp(0, 1) * 255).float()
    s = torch.round(s) if mut == "nearest" else torch.floor(s)
    u8 = s.to(torch.uint8).permute(2, 3, 0, 4, 1)
    NI, C, Fr, H, W = video.shape
    u8 = u8.reshape(Fr, H, NI * W, C)
    return (u8.flip(-1) if (bgr and mut != "nobgr") else u8).contiguous()


def _build_u8(c):
    b = Built(c)
    NI, C, Fr, H, W = shape = c["shape"]
    dt, half, bgr, ld = c["dt"], c["half"], c["bgr"], c["ld"]
    V, whole = u8_video(dt, shape, c["seed"])
    assert whole or c.get("wrap")
    if ld:       # channels-last decoder tokens [(i f y x), ld]; the padding channels are NaN
        src = b.fenced(NI * Fr * H * W, C, dt, pad_cols=ld - C)
        b.put(src, V.permute(0, 2, 3, 4, 1).reshape(-1, C))
        strides = (Fr * H * W * ld, 1, H * W * ld, W * ld, ld)
    else:
        src = b.flat(V.numel(), dt)
        b.put(src, V)
        strides = (C * Fr * H * W, Fr * H * W, H * W, W, 1)
    dst = b.flat(V.numel(), "u8")
    op = b.P.to_uint8("u8", src.ref, dt, dst.ref, NI=NI, C=C, F=Fr, H=H, W=W, strides=strides, half=half, bgr=bgr)
    assert op.kind == L.OP_TO_UINT8 and (op.i[5], op.i[6], op.i[7]) == (DT[dt], int(half), int(bgr)) and op.i[14] == (ld or 1)
    vid = V.to(TD[dt])
    oracle = torch.from_numpy(np.stack(tp.tensor2vid_uint8(vid.half() if half else vid.float())))      # pinned to the reference's own function
    want = (oracle.flip(-1) if bgr else oracle).contiguous()
    b.check("bytes", win_of(dst), [c_exact(want.reshape(1, -1), one_seg)], exact=True)
    b.u8 = dict(video=vid, want=want, oracle=oracle)

    def mutations():
        muts = [("round to nearest instead of truncating", {"bytes": u8_formula(vid, half, bgr, "nearest").reshape(1, -1)}, {"bytes": None})]
        if half:
            muts.append(("the HALF chain computed in fp32 and rounded once", {"bytes": u8_formula(vid, half, bgr, "fp32once").reshape(1, -1)}, {"bytes": None}))
        if bgr:
            muts.append(("bgr ignored", {"bytes": u8_formula(vid, half, bgr, "nobgr").reshape(1, -1)}, {"bytes": None}))
        return muts
    b.mutations = mutations
    b.path = f"OP_TO_UINT8 in={dt} i[6]={int(half)} i[7]={int(bgr)} {'tokens ld=' + str(ld) if ld else 'NCFHW'}" + (" grid-stride" if c.get("wrap") else "")
    return b


# ---- DEPTH_TOKENS ---------------------------------------------------------------------------------------------------------------------------
def depth_frame(kind, hw, dt, g):
    """One frame [hw] (float64, representable in dt) and where its extremes are.  kind = (range lo, range hi, min position, max position) |
    "const" | "nan": the interior lies strictly inside the range."""
    if kind == "const":
        return torch.full((hw,), -2.5, dtype=torch.float64)
    nan = kind == "nan"
    lo, hi, pmin, pmax = (0.0, 10.0, hw - 1, hw // 2) if nan else kind
    pmin, pmax = pmin % hw, pmax % hw
    d = rnd(lo + (hi - lo) * (0.1 + 0.8 * torch.rand(hw, generator=g, dtype=torch.float64)), dt)
    d[pmin], d[pmax] = lo, hi
    if nan:
        d[hw // 3] = NAN
    return d


def depth_ref(D, H, W, norm, mut=None):
    """D [n, H W] -> (tokens in numpy fp32 arithmetic, every operation rounded on its own, cast to fp16; the same in float64)."""
    n, hw = D.shape
    d32 = D.numpy().astype(np.float32)
    with np.errstate(invalid="ignore"):
        if mut == "nanmin":
            mn, mx = np.nanmin(d32, axis=1, keepdims=True), np.nanmax(d32, axis=1, keepdims=True)      # fminf / fmaxf drop the NaN
        else:
            mn, mx = np.min(d32[:, :256] if mut == "min256" else d32, axis=1, keepdims=True), np.max(d32, axis=1, keepdims=True)
        if mut == "next":
            mn, mx = np.roll(mn, -1, 0), np.roll(mx, -1, 0)
        if norm:
            den = (mx - mn) + np.float32(1e-7)
            v32 = (np.float32(2.0) * (d32 - mn)) / den - np.float32(1.0)
            D64 = D.numpy()
            v64 = 2.0 * (D64 - mn.astype(np.float64)) / (mx.astype(np.float64) - mn.astype(np.float64) + 1e-7) - 1.0
        else:
            v32, v64 = d32, D.numpy()

    def unshuffle(v):      # channel = (y % 8) * 8 + x % 8 of token (y // 8, x // 8)
        t = torch.from_numpy(np.ascontiguousarray(v)).view(n, H // 8, 8, W // 8, 8)
        t = t.permute(0, 1, 3, 4, 2) if mut == "chan" else t.permute(0, 1, 3, 2, 4)
        return t.reshape(n * (H // 8) * (W // 8), 64)
    return unshuffle(v32).half(), unshuffle(v64).double()


def _build_depth(c):
    b = Built(c)
    b.adapter = True
    n, H, W, dt, norm, ld, kinds = (c[k] for k in ("n", "H", "W", "dt", "norm", "ld", "frames"))
    hw = H * W
    g = _gen(c["seed"])
    D = torch.stack([depth_frame(k, hw, dt, g) for k in kinds])
    src = b.flat(n * hw, dt)
    b.put(src, D)
    out = b.fenced(n * hw // 64, 64, "f16", pad_cols=ld - 64)
    op = b.P.depth_tokens("dt", src.ref, dt, out, n=n, H=H, W=W, normalise=bool(norm))
    assert op.kind == L.OP_DEPTH_TOKENS and (op.i[3], op.i[4], op.i[5]) == (DT[dt], norm, ld)
    want, ref64 = depth_ref(D, H, W, norm)
    seg = lambda t: t.reshape(n, -1)
    b.check("tokens", win_of(out), [c_exact(want, seg)], exact=True)
    finite = torch.isfinite(ref64)
    b.check("tokens vs float64", lambda rd: torch.where(finite, rd(out).double(), torch.zeros_like(ref64)),
            [c_elem(torch.where(finite, ref64, torch.zeros_like(ref64)), ulp16(torch.where(finite, ref64, torch.zeros_like(ref64))), seg, "ulp16")])
    const = torch.tensor([k == "const" for k in kinds])
    nanf = torch.tensor([k == "nan" for k in kinds])
    if norm:
        assert bool((seg(want)[const] == -1).all()) and bool(torch.isnan(seg(want)[nanf]).all()) and bool(torch.isfinite(seg(want)[~nanf]).all())
    b.depth = dict(D=D, const=const, nan=nanf)

    def mutations():
        every = torch.ones(n, dtype=torch.bool)
        muts = [("channel as (x % 8) * 8 + y % 8", {"tokens": depth_ref(D, H, W, norm, "chan")[0]}, {"tokens": ~(const | nanf) if norm else every})]
        if norm:
            muts.append(("extremes of the next frame", {"tokens": depth_ref(D, H, W, norm, "next")[0]}, {"tokens": every}))
            late = torch.tensor([k not in ("const", "nan") and k[2] % hw >= 256 for k in kinds])
            if bool(late.any()):
                muts.append(("the minimum over the first 256 pixels only", {"tokens": depth_ref(D, H, W, norm, "min256")[0]}, {"tokens": late}))
            if bool(nanf.any()):
                muts.append(("NaN dropped (fminf / fmaxf semantics)", {"tokens": depth_ref(D, H, W, norm, "nanmin")[0]}, {"tokens": nanf}))
        return muts
    b.mutations = mutations
    b.path = f"OP_DEPTH_TOKENS in={dt} i[4]={norm} ld={ld} {n}x{H}x{W}"
    return b


# ---- AVGPOOL2 -------------------------------------------------------------------------------------------------------------------------------
def pool_ref(X, n, H, W, C, mut=None):
    """X [n H W, C] float64 -> (mean of the 2 x 2 taps [n Ho Wo, C], sum of their magnitudes): nn.AvgPool2d(2, 2), an odd last row / column
    is ignored."""
    Ho, Wo = H // 2, W // 2
    flat = torch.cat([X, torch.full((W + 2, C), NAN, dtype=torch.float64)])
    if mut == "odd":
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
    f, y, x = torch.arange(n).view(n, 1, 1), torch.arange(Ho).view(1, Ho, 1), torch.arange(Wo).view(1, 1, Wo)
    s0 = ((f * H + 2 * y) * W + 2 * x).reshape(-1).clamp(max=flat.shape[0] - W - 2)
    down = W // 2 if mut == "stride" else W
    a, bb, d, e = flat[s0], flat[s0 + 1], flat[s0 + down], flat[s0 + down + 1]
    if mut == "three":
        e = torch.zeros_like(e)
    return ((a + bb) + (d + e)) * 0.25, (a.abs() + bb.abs() + d.abs() + e.abs())


def _build_pool(c):
    b = Built(c)
    b.adapter = True
    n, H, W, C, ld_in, outs = (c[k] for k in ("n", "H", "W", "C", "ld_in", "outs"))
    Ho, Wo = H // 2, W // 2
    f, y, x = torch.arange(n).view(n, 1, 1, 1), torch.arange(H).view(1, H, 1, 1), torch.arange(W).view(1, 1, W, 1)
    X = (seg_scale(x // 2, y // 2, f) * body((n, H, W, C), _gen(c["seed"]))).reshape(n * H * W, C)      # one scale per output token
    if c.get("wrap"):
        late = second_pass(n * Ho * Wo * (C // 4), 4).view(n, Ho, Wo, C)
        X = mark_wrap(X.view(n, H, W, C), late.repeat_interleave(2, 1).repeat_interleave(2, 2)).reshape(n * H * W, C)
    X = rnd(X, "f32")
    xin = b.fenced(n * H * W, C, "f32", pad_cols=ld_in - C)
    b.put(xin, X)
    pad = 0 if c.get("wrap") else 4
    o32 = b.fenced(n * Ho * Wo, C, "f32", pad_cols=pad) if "f32" in outs else None
    o16 = b.fenced(n * Ho * Wo, C, "f16", pad_cols=pad) if "f16" in outs else None
    op = b.P.avgpool2("pool", xin, n=n, H=H, W=W, out32=o32, out16=o16)
    assert op.kind == L.OP_AVGPOOL2 and op.i[4] == ld_in and (op.p[1].space == "arena") == (o32 is not None) and (op.p[2].space == "arena") == (o16 is not None)
    ref, mass = pool_ref(X, n, H, W, C)
    if o32 is not None:
        b.check("out32", win_of(o32), [c_elem(ref, (1.5 * 2.0 ** -23 * mass / 4).clamp_min(1e-45), rows_seg, "x1.5*2^-23 mean|tap|")], ref=ref, dt="f32")
    if o16 is not None:
        r16 = ref.half().double()
        b.check("out16", win_of(o16), [c_elem(r16, ulp16(r16), rows_seg, "ulp16")], ref=ref, dt="f16")

    def mutations():
        muts = []
        for what, key in (("stride taken as W / 2", "stride"), ("three of four taps", "three"), ("odd last row / column included", "odd")):
            if key == "odd" and H % 2 == 0 and W % 2 == 0:
                continue
            r, _ = pool_ref(X, n, H, W, C, key)
            aff = None
            if key == "odd":        # the token index moves once the output is (W + 1) / 2 wide: every token behind the first output row
                r = r[: n * Ho * Wo]
                aff = torch.arange(n * Ho * Wo) >= Wo if W % 2 else torch.arange(n * Ho * Wo) >= Ho * Wo
            got = {}
            if o32 is not None:
                got["out32"] = r.float()
            if o16 is not None:
                got["out16"] = r.half()
            muts.append((what, got, {k: aff for k in got}))
        return muts
    b.mutations = mutations
    b.path = f"OP_AVGPOOL2 {n}x{H}x{W}x{C} ld_in={ld_in} out={'+'.join(outs)}" + (" grid-stride" if c.get("wrap") else "")
    return b


_BUILDERS = dict(ncthw=_build_ncthw, cl=_build_cl, time=_build_time, copy=_build_copy, softmax=_build_softmax, ddim=_build_ddim,
                 lincomb=_build_lincomb, u8=_build_u8, depth=_build_depth, pool=_build_pool)


def build(case):
    """The program (Built.P) or the sampler op (Built.ops / Built.call) of a case, with init / checks / mutations."""
    return _BUILDERS[case["family"]](case)


# ---- the case list --------------------------------------------------------------------------------------------------------------------------
CASES = []


def _add(family, id, **kw):
    CASES.append(dict(family=family, id=id, seed=1000 + 7 * len(CASES), **kw))


for _B, _Bs, _C, _F, _HW, _ld, _dt, _sc, _lo in ((4, 2, 4, 3, 35, 8, "f32", 1 / 0.18215, "none"), (2, 0, 4, 5, 37, 8, "f32", 0.5, "pad"),
                                                 (3, 0, 3, 2, 33, 8, "f32", 1.0, "buf"), (2, 1, 4, 3, 35, 4, "f16", 1.0, "none")):
    _add("ncthw", f"ncthw-B{_B}src{_Bs}-C{_C}F{_F}HW{_HW}-ld{_ld}-{_dt}-lo_{_lo}", B=_B, Bsrc=_Bs, C=_C, F=_F, HW=_HW, ld=_ld, dt=_dt, scale=_sc, lo=_lo)
_add("ncthw", "ncthw-wrap", B=1, Bsrc=0, C=4, F=1, HW=2097409, ld=4, dt="f32", scale=0.5, lo="none", wrap=True)
for _B, _C, _F, _HW, _ld, _dt in ((2, 4, 3, 35, 8, "f32"), (1, 3, 2, 33, 4, "f16"), (2, 4, 5, 37, 4, "f16")):
    _add("cl", f"cl-B{_B}C{_C}F{_F}HW{_HW}-ld{_ld}-{_dt}", B=_B, C=_C, F=_F, HW=_HW, ld=_ld, dt=_dt)
_add("cl", "cl-wrap", B=1, C=3, F=1, HW=699100, ld=4, dt="f32", wrap=True)
for _B, _dim, _first in ((1, 320, 0), (5, 320, 0), (3, 1280, 2)):
    _add("time", f"time-B{_B}-dim{_dim}", B=_B, dim=_dim, first=_first)
for _s, _d, _a, _lo, _form in (("f32", "f16", 0, True, "plain"), ("f32", "f16", 1, False, "plain"), ("f32", "f32", 0, False, "plain"),
                               ("f16", "f16", 0, False, "concat"), ("f16", "f16", 2, False, "inplace"), ("f16", "f32", 3, False, "plain"),
                               ("f16", "f32", 1, False, "plain")):
    _add("copy", f"copy-{_s}-{_d}-act{_a}{'-lo' if _lo else ''}-{_form}", rows=37, cols=132, sdt=_s, ddt=_d, act=_a, lo=_lo, form=_form)
_add("copy", "copy-wrap", rows=4099, cols=2052, sdt="f32", ddt="f16", act=0, lo=True, form="plain", wrap=True)
for _r, _c, _li, _lo in ((5, 1000, 1008, 1004), (3, 40, 40, 48), (4, 1024, 1024, 1024)):
    _add("softmax", f"softmax-{_r}x{_c}-ld{_li}-{_lo}", rows=_r, cols=_c, ld_in=_li, ld_out=_lo)
_DDIM = [(1, 4, 105, 2, "f32", "f32", 0, 0, None), (1, 4, 105, 4, "f16", "f32", 0, 1, None), (3, 4, 105, 2, "f32", "f32", 0, 0, None),
         (2, 4, 99, 0, "f16", "f16", 0, 0, None), (1, 4, 105, 4, "f32", "f32", 1, 1, None), (2, 4, 99, 4, "f16", "f32", 1, 0, None),
         (2, 4, 99, 0, "f32", "f32", 1, 1, None), (2, 4, 99, 4, "f32", "f32", 1, 1, "qnoise"), (2, 4, 99, 4, "f32", "f32", 1, 1, "null")]
for _S, _Cs, _in, _g, _e, _x, _m, _eta, _bl in _DDIM:
    for _which in range(3):
        for _gs in ((9.0, 1.0) if _g else (1.0,)):
            _add("ddim", f"ddim-S{_S}-in{_in}-g{_g}-{_e}-{_x}-mode{_m}-eta{_eta}{'-blend_' + _bl if _bl else ''}-step{_which}-gs{_gs:g}", S=_S, Cs=_Cs,
                 inner=_in, guided=_g, edt=_e, xdt=_x, mode=_m, eta=float(_eta), which=_which, gscale=_gs, blend=_bl)
_add("ddim", "ddim-wrap", S=1, Cs=4, inner=524353, guided=2, edt="f32", xdt="f32", mode=0, eta=1.0, which=1, gscale=9.0, blend=None, wrap=True)
for _n, _t, _o, _kw in ((1, ("f32",), "f32", {}), (255, ("f16", "f32"), "f16", {}), (257, ("f32", "f16", "f32"), "f32", {}),
                        (756, ("f32", "f16", "f32", "f16", "f32", "f16"), "f32", {}), (756, ("f16", "f16", "f32", "f32"), "f16", {}),
                        (257, ("f32",) * 5, "f16", {}), (756, ("f32", "f32", "f16"), "f32", dict(cancel=True))):
    _add("lincomb", f"lincomb-n{_n}-{len(_t)}terms-{_o}{'-cancel' if _kw else ''}", n=_n, terms=_t, out=_o, **_kw)
_add("lincomb", "lincomb-wrap", n=2097409, terms=("f32", "f16"), out="f32", wrap=True)
for _dt in ("f32", "f16"):
    for _half in (False, True):
        for _ld in (0, 4, 8):
            for _bgr in (False, True):
                _add("u8", f"u8-{_dt}-{'half' if _half else 'full'}-{'cl' + str(_ld) if _ld else 'ncfhw'}{'-bgr' if _bgr else ''}", shape=(2, 3, 2, 7, 31), dt=_dt,
                     half=_half, bgr=_bgr, ld=_ld)
_add("u8", "u8-wrap", shape=(1, 3, 1, 1, 2097452), dt="f32", half=False, bgr=True, ld=0, wrap=True)
# depth frames: (range lo, range hi, position of the minimum, position of the maximum) | "const" | "nan".  Positions 199 / 250 (+ 256 k) are
# in the last wave's share only; with 64 pixels the waves 1 - 3 only ever see src[0]
_add("depth", "depth-3x16x24-f32-norm", n=3, H=16, W=24, dt="f32", norm=1, ld=64, frames=[(0.0, 10.0, -1, 255), (-3.0, -1.0, -1, 256), (1000.0, 1001.0, 199, 250)])
_add("depth", "depth-3x8x8-f16-norm", n=3, H=8, W=8, dt="f16", norm=1, ld=72, frames=[(0.0, 10.0, -1, 37), "const", "nan"])
_add("depth", "depth-4x40x72-f32-norm", n=4, H=40, W=72, dt="f32", norm=1, ld=64, frames=[(1000.0, 1001.0, -1, 255), "const", "nan", (-3.0, -1.0, 2760, 1023)])
_add("depth", "depth-2x16x24-f16-plain", n=2, H=16, W=24, dt="f16", norm=0, ld=72, frames=[(0.0, 10.0, -1, 255), (-3.0, -1.0, -1, 256)])
for _outs in (("f32",), ("f16",), ("f32", "f16")):
    _add("pool", f"pool-2x6x10x68-{'+'.join(_outs)}", n=2, H=6, W=10, C=68, ld_in=72, outs=_outs)
_add("pool", "pool-1x7x11x8-odd", n=1, H=7, W=11, C=8, ld_in=8, outs=("f32", "f16"))
_add("pool", "pool-wrap", n=1, H=2, W=2 * 131075, C=68, ld_in=68, outs=("f32",), wrap=True)
# `lowered`: the combinations the lowerings emit that no case above has (tests/record_paths.py): plain fp32 / fp16 tokens without a low-order
# image, the shared-sample source with one; the fp32 -> fp16 cast without its second output and the fp16 -> fp32 copy without an activation
for _B, _Bs, _ld, _dt, _sc, _lo in ((2, 0, 8, "f32", 1.0, "none"), (2, 0, 4, "f16", 1.0, "none"), (4, 2, 8, "f32", 0.5, "pad")):
    _add("ncthw", f"lowered-ncthw-B{_B}src{_Bs}-ld{_ld}-{_dt}-lo_{_lo}", B=_B, Bsrc=_Bs, C=4, F=3, HW=35, ld=_ld, dt=_dt, scale=_sc, lo=_lo)
for _s, _d in (("f32", "f16"), ("f16", "f32")):
    _add("copy", f"lowered-copy-{_s}-{_d}-act0-plain", rows=37, cols=132, sdt=_s, ddt=_d, act=0, lo=False, form="plain")
assert len({c["id"] for c in CASES}) == len(CASES)
