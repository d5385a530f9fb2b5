"""Weight plumbing: turns the reference-layout state dict (torch [Cout, Cin, k...] tensors)
into the GEMM-ready packed images the HIP kernels read ([N, K] fp16, reduction ordered (64-channel
chunk, tap, channel); fp32 bias / affine vectors).  Pure layout work with torch ops, run once per
weight version (and again after `invalidate()`, e.g. when the LoRA hook of the reference,
scripts/stable_lora/stable_utils/lora_processor.py:215-246, has mutated `.weight` in place).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Tuple

import torch

Recipe = Callable[[Dict[str, torch.Tensor]], torch.Tensor]

RELPOS_LONG_PADL = 72          # T2V_RELPOS_LONG_PADL (include/t2v_hip.h): replicated left-edge columns of relpos_table_long's Ev^T


def _f16(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float16).contiguous()


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def pad_rows(w: torch.Tensor, mult: int = 4) -> torch.Tensor:
    n = w.shape[0]
    if n % mult == 0:
        return w
    pad = mult - n % mult
    return torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], dim=0)


def linear(w: torch.Tensor) -> torch.Tensor:
    """nn.Linear / Conv1d k=1 / Conv2d 1x1 weight -> [N, K]."""
    return w.reshape(w.shape[0], -1)


KCHUNK = 64   # channels per reduction chunk (= the GEMM k-tile)


def conv3x3(w: torch.Tensor, cin_pad: int = 0) -> torch.Tensor:
    """[Co, Ci, 3, 3] -> [Co, 9*Ci'].  Reduction order for Ci % 64 == 0 (every conv of the UNet/VAE
    body): k = (ci // 64) * 9*64 + (ky*3+kx) * 64 + ci % 64 — "64-channel chunk, tap, channel" — so
    that the 9 taps that re-read the same activation cache lines are CONSECUTIVE k-tiles (they hit
    L1/L2 instead of re-streaming the tensor 9x).  The 4(+4 zero)-channel stem uses k = tap*8 + ci."""
    co, ci = w.shape[0], w.shape[1]
    w = w.permute(0, 2, 3, 1)                      # Co, ky, kx, Ci
    if cin_pad and cin_pad > ci:
        w = torch.cat([w, w.new_zeros(co, 3, 3, cin_pad - ci)], dim=3)
        ci = cin_pad
    if ci % KCHUNK == 0:
        w = w.reshape(co, 9, ci // KCHUNK, KCHUNK).permute(0, 2, 1, 3)   # Co, chunk, tap, 64
    return w.reshape(co, -1)


def conv3x3_c8_dup(w: torch.Tensor) -> torch.Tensor:
    """Stem conv [Co, 4, 3, 3] -> [Co, 9 * 8] with the 4 real input channels REPEATED in the 4 padding channels (k = tap * 8 + ci):
    the entry op puts the low-order fp16 images of the latent there, so the one GEMM pass computes (x_hi + x_lo) . W."""
    assert w.shape[1] == 4
    return conv3x3(torch.cat([w, w], dim=1))


def relpos_table16(tab: torch.Tensor, frames: int, transposed: bool) -> torch.Tensor:
    """A relative-position table [2R+1, d] (lvdm RelativePosition.embeddings_table, attention_temporal.py:21-41) as the persistent MFMA
    kernel of clips of <= 16 frames reads it (csrc/attention.hip relpos16_kernel): only rows R-(F-1) .. R+(F-1) are ever addressed by
    a clip of F frames (no clipping when R >= F-1), so slot jl = row jl + R-(F-1), 32 slots, fp16, zero-padded.
    transposed=False: [32, DK] (K-side table, DK = d rounded up to 16);  True: [DV, 32] (V-side table, DV = d rounded up to 32)."""
    n_rows, d = tab.shape
    R = (n_rows - 1) // 2
    assert frames <= 16 and R >= frames - 1
    jbase = R - (frames - 1)
    n = min(32, n_rows - jbase)
    if transposed:
        out = torch.zeros((d + 31) // 32 * 32, 32, dtype=torch.float16, device=tab.device)
        out[:d, :n] = tab[jbase:jbase + n].t().to(torch.float16)
    else:
        out = torch.zeros(32, (d + 15) // 16 * 16, dtype=torch.float16, device=tab.device)
        out[:n, :d] = tab[jbase:jbase + n].to(torch.float16)
    return out.contiguous()


def relpos_long_cols(R: int) -> int:
    """Columns of the transposed V-side table of relpos_table_long (T2V_RELPOS_LONG_COLS in include/t2v_hip.h)."""
    return (2 * R + 158) // 8 * 8


def relpos_table_long(tab: torch.Tensor, transposed: bool) -> torch.Tensor:
    """A relative-position table [2R+1, d] as the MFMA kernel for clips of any length reads it (csrc/attention.hip relpos_long_kernel,
    RELPOS_ATTN i[17] = 3), fp16 and independent of the frame count.
    transposed=False: [2R+1, DK] = the table, zero columns beyond d (DK = d rounded up to 16).
    True: [DV, relpos_long_cols(R)] = the table transposed with replicated edges: column c holds row clamp(c - RELPOS_LONG_PADL, 0, 2R),
    zero rows beyond d (DV = d rounded up to 32), so that any 80-column window the kernel reads is a plain column range."""
    n_rows, d = tab.shape
    R = (n_rows - 1) // 2
    assert n_rows == 2 * R + 1
    if not transposed:
        out = torch.zeros(n_rows, (d + 15) // 16 * 16, dtype=torch.float16, device=tab.device)
        out[:, :d] = tab.to(torch.float16)
        return out.contiguous()
    rows = (torch.arange(relpos_long_cols(R), device=tab.device) - RELPOS_LONG_PADL).clamp(0, 2 * R)
    out = torch.zeros((d + 31) // 32 * 32, rows.numel(), dtype=torch.float16, device=tab.device)
    out[:d] = tab[rows].t().to(torch.float16)
    return out.contiguous()


RESAMPLE_PRECISION_BITS = 22   # Pillow's PRECISION_BITS (Resample.c): 8-bit resampling coefficients are 22-bit fixed point


def _lanczos(x: float) -> float:
    """Pillow's lanczos_filter: sinc(x) * sinc(x / 3) on -3 <= x < 3 (libm's sin through `math`, as the C code calls it)."""
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def resample_ksize(in_size: int, out_size: int) -> int:
    """Row length of resample_table(in_size, out_size): Pillow's ksize = ceil(support) * 2 + 1 with support = 3 * max(in / out, 1)."""
    return int(math.ceil(3.0 * max(in_size / out_size, 1.0))) * 2 + 1


def resample_identity_table(size: int):
    """One-tap table that copies every index (coefficient 2^22: acc = 2^21 + u * 2^22, acc >> 22 = u): the pass that only converts
    uint8 frames already at the target size into the encoder's tokens."""
    import numpy as np
    coef = np.full((size, 1), 1 << RESAMPLE_PRECISION_BITS, dtype=np.int32)
    bounds = np.stack([np.arange(size, dtype=np.int32), np.ones(size, dtype=np.int32)], axis=1)
    return coef, bounds


def resample_table(in_size: int, out_size: int):
    """Coefficient table of ONE pass of Pillow's 8-bit Lanczos resize (`Image.resize(..., Image.LANCZOS)`, Resample.c
    precompute_coeffs + normalize_coeffs_8bpc) from `in_size` to `out_size` pixels, computed in float64 in the same operation order:
    -> (coef int32 [out, ksize], bounds int32 [out, 2] = {first source index, taps}); taps beyond a row's count are zero.
    T2V_OP_RESAMPLE evaluates it: acc = 2^21 + sum_j src[first + j] * coef[j], value = clamp(acc >> 22, 0, 255)."""
    import numpy as np
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample_table: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = resample_ksize(in_size, out_size)
    ss = 1.0 / filterscale
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    one = float(1 << RESAMPLE_PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((j + xmin - center + 0.5) * ss) for j in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for j, v in enumerate(w):
            coef[xx, j] = int(0.5 + v * one) if v >= 0 else int(-0.5 + v * one)
        bounds[xx] = (xmin, xmax)
    return coef, bounds


def resample_lut() -> torch.Tensor:
    """fp32 [256]: 2 * (u / 255) - 1 in float32, with the reference's own operations (process_modelscope.py:129,137: numpy `/ 255`
    on a float32 array, then torch `2 * x - 1`) — the value table of T2V_OP_RESAMPLE's token forms, so that the bits do not depend on
    the device's division."""
    import numpy as np
    return 2 * torch.from_numpy(np.arange(256).astype(np.float32) / 255) - 1


BICUBIC_A = -0.75              # torch's cubic convolution coefficient (aten UpSample.h: cubic_convolution1 / 2)


def bicubic_table(in_size: int, out_size: int, dtype=None):
    """Tap table of ONE axis of torch's bicubic resize, `F.interpolate(mode="bicubic", align_corners=False)` without antialiasing
    (aten upsample_bicubic2d; ddpm3d.py:1443-1468 resizes the frames to the depth estimator's size and the depth maps back), from `in_size`
    to `out_size` pixels, enlarging or reducing: -> (weights float32 [out, 4], indices int32 [out, 4]).  For output index o:
    real = (in / out) * (o + 0.5) - 0.5 (NOT clamped at 0), i0 = floor(real), t = real - i0; the taps are i0 - 1 .. i0 + 2, each clamped
    to [0, in - 1]; the weights c2(t + 1), c1(t), c1(1 - t), c2(2 - t) with c1(x) = ((A + 2) x - (A + 3)) x^2 + 1 and
    c2(x) = ((A x - 5 A) x + 8 A) x - 4 A, A = -0.75.  Coordinates and weights are evaluated in float64 and the weights rounded ONCE to
    float32 (torch evaluates them in float32: its coordinate error alone is 1e-5 .. 1e-4 of output error, more than the 16-tap sum's; the
    float64 table does not depend on how a build contracts that arithmetic).  `dtype=numpy.float64` keeps the unrounded weights (tests).
    T2V_OP_RESAMPLE with i[9] = 1 evaluates out = sum_a wy[a] * (sum_b wx[b] * src[iy[a]][ix[b]]) with one table per axis."""
    import numpy as np
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"bicubic_table: sizes must be positive, got {in_size} -> {out_size}")
    A = BICUBIC_A
    o = np.arange(out_size, dtype=np.float64)
    real = (in_size / out_size) * (o + 0.5) - 0.5
    fl = np.floor(real)
    t = real - fl

    def c1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def c2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A

    w = np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], axis=1)
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, in_size - 1).astype(np.int32)
    return np.ascontiguousarray(w.astype(np.float32 if dtype is None else dtype)), np.ascontiguousarray(idx)


def linear_dup(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> [N, 2K] = [W | W]: consumer of an operand laid out [hi (K) | lo (K)] per row."""
    w = linear(w)
    return torch.cat([w, w], dim=1)


def tconv3(w: torch.Tensor) -> torch.Tensor:
    """[Co, Ci, 3, 1, 1] -> [Co, 3*Ci] with k = (ci // 64) * 3*64 + kt * 64 + ci % 64 (Ci % 64 == 0)."""
    co, ci = w.shape[0], w.shape[1]
    w = w[:, :, :, 0, 0].permute(0, 2, 1)          # Co, kt, Ci
    assert ci % KCHUNK == 0
    return w.reshape(co, 3, ci // KCHUNK, KCHUNK).permute(0, 2, 1, 3).reshape(co, 3 * ci)


def qkv_head_major(wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, head_dim: int = 64) -> torch.Tensor:
    """to_q / to_k / to_v weights [heads * d, K] -> [heads][q (d) | k (d) | v (d)][K]: one head's three projections are 3 * d
    consecutive output columns = one tile of the fused QKV + temporal attention GEMM (T2V_EPI_TATTN)."""
    heads = wq.shape[0] // head_dim
    parts = [w.reshape(heads, head_dim, -1) for w in (wq, wk, wv)]
    return torch.stack(parts, dim=1).reshape(3 * heads * head_dim, -1)


def geglu_perm(n_half: int, device=None) -> torch.Tensor:
    """Row permutation for the fused GEGLU epilogue: packed row 16u + 8g + j  <-  source row
    (g ? n_half : 0) + 8u + j   (value rows first, gate rows second in nn.Linear(dim, 2*inner),
    reference t2v_model.py:817-821)."""
    assert n_half % 8 == 0
    u = torch.arange(n_half // 8, device=device).view(-1, 1, 1)
    g = torch.arange(2, device=device).view(1, -1, 1)
    j = torch.arange(8, device=device).view(1, 1, -1)
    return (g * n_half + 8 * u + j).reshape(-1)


class _ReadLog:
    """Read-only view of a state dict that notes which keys a recipe touches."""

    def __init__(self, sd: Dict[str, torch.Tensor]):
        self.sd, self.read = sd, set()

    def __getitem__(self, k):
        self.read.add(k)
        return self.sd[k]

    def __contains__(self, k):
        self.read.add(k)
        return k in self.sd

    def get(self, k, default=None):
        self.read.add(k)
        return self.sd.get(k, default)


class WeightPacker:
    """Collects (name -> recipe) pairs during lowering and materialises them on a device.
    `materialise` packs everything and learns which state-dict keys each recipe reads; `update` re-packs, in
    place, only the images that depend on changed keys — the LoRA merge of the reference
    (scripts/stable_lora/stable_utils/lora_processor.py:202-246) rewrites some hundred attention / conv weights
    out of ~2600 tensors, and the device addresses bound into the denoise programs stay valid."""

    def __init__(self):
        self.recipes: List[Tuple[str, str, Recipe]] = []   # (name, 'f16'|'f32'|'i32', fn)
        self._names = set()
        self.deps: Dict[str, frozenset] = {}                # packed name -> state-dict keys its recipe read

    def add(self, name: str, dtype: str, fn: Recipe) -> str:
        if name not in self._names:
            self._names.add(name)
            self.recipes.append((name, dtype, fn))
        return name

    def add_lo(self, name: str) -> str:
        """Second-order image of an fp16 weight image: lo = fp16(W - fp16(W)), so that A.W_hi + A.W_lo carries more of
        the fp32 weight through two fp16 MFMA passes (packing is layout-only, hence linear: pack(W) splits like W).
        All zeros for a model that is already `.half()` (the deployed form, t2v_pipeline.py:103-104).
        Precision actually carried: the residual is ~2^-12 |W|; for |W| below 2^-3 it lies in the fp16 SUBNORMAL
        range, whose spacing is 2^-24 absolute — torch's conversion and the gfx950 MFMA keep subnormals, so nothing is flushed,
        but the pair then resolves W to ~2^-25 absolute = 19-21 significant bits for the 1e-2..1e-1 weights of these networks
        (the full 22 only for |W| >= 2^-3).  A 2^11 pre-scale of `lo` with the factor folded into the second pass would restore
        the rest; not done — with fp16 deployment the option only matters for fp32-weight experiments."""
        lo = name + ":lo"
        if lo not in self._names:
            base = next(fn for n, d, fn in self.recipes if n == name)

            def fn(sd, base=base):
                t = base(sd).float()
                return t - t.half().float()
            self.add(lo, "f16", fn)
        return lo

    @staticmethod
    def _cast(t: torch.Tensor, dtype: str, device) -> torch.Tensor:
        if dtype == "i32":          # integer tables (T2V_OP_RESAMPLE coefficients / bounds)
            return t.detach().to(device=device, dtype=torch.int32).contiguous()
        return _f16(t, device) if dtype == "f16" else _f32(t, device)

    def materialise(self, sd: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
        out = {}
        for name, dtype, fn in self.recipes:
            log = _ReadLog(sd)
            out[name] = self._cast(fn(log), dtype, device)
            self.deps[name] = frozenset(log.read)
        return out

    def update(self, packed: Dict[str, torch.Tensor], sd: Dict[str, torch.Tensor], device, changed, deps=None) -> int:
        """Re-pack the images whose recipes read any key in `changed`, writing through the existing device
        tensors.  `deps` = the key sets learnt by the `materialise` that produced `packed` (default: this
        packer's own).  Returns the number of images rewritten, or -1 if an image or its key set is missing, or
        its shape changed (the caller then falls back to `materialise` and re-binds its programs)."""
        changed = set(changed)
        deps = self.deps if deps is None else deps
        todo = [(n, d, f) for n, d, f in self.recipes if n not in deps or (deps[n] & changed)]
        for name, dtype, fn in todo:
            if name not in packed or name not in deps:
                return -1
        fresh = []
        for name, dtype, fn in todo:
            t = self._cast(fn(sd), dtype, device)
            if t.shape != packed[name].shape:
                return -1
            fresh.append((name, t))
        for name, t in fresh:
            packed[name].copy_(t)
        return len(fresh)


# ---- byte-level fingerprints of the parameters (T2V_OP_FINGERPRINT) ------------------------------------------------------------------
# The signature the repack decision rests on, (id, _version, device, dtype, shape), cannot see a write through `.data` (the VideoCrafter
# LoRA loaders of the reference, lvdm/models/modules/lora.py:656-740: `weight.data += ...`, `weight.data = origin.clone()`): neither the
# object nor its version counter moves.  The fingerprint looks at the bytes.  A tensor's storage is read as n little-endian 16-bit words:
#     value = sum_j v_j (2 j + 1) + 2^32 sum_j v_j^2 + (n + 1) FINGERPRINT_LEN   (mod 2^64)          (include/t2v_hip.h)
FINGERPRINT_CHUNK = 65536                       # T2V_FINGERPRINT_CHUNK: bytes of one tensor per workgroup
FINGERPRINT_LEN = 0x9E3779B97F4A7C15            # T2V_FINGERPRINT_LEN
_M64 = (1 << 64) - 1


def _as_words(t: torch.Tensor) -> torch.Tensor:
    """The bytes of a contiguous tensor as int16 words (a view)."""
    flat = t.detach().reshape(-1)
    if (flat.numel() * flat.element_size()) % 2 != 0:
        raise ValueError(f"fingerprint: a byte range of odd length ({flat.numel() * flat.element_size()} bytes)")
    return flat.view(torch.int16) if flat.numel() else flat.new_zeros(0, dtype=torch.int16)


def fingerprint_torch(t: torch.Tensor) -> int:
    """The fingerprint of one tensor's bytes with torch integer ops (int64 arithmetic wraps like the kernel's unsigned adds) — the
    implementation for parameters that live on the CPU beside a CPU pack, and the reference of the kernel's tests."""
    w = _as_words(t.contiguous())
    n = w.numel()
    total = ((n + 1) * FINGERPRINT_LEN) & _M64
    step = 1 << 20                              # pieces keep every partial sum far below 2^63: the fold to 64 bits is done in Python
    for j0 in range(0, n, step):
        v = w[j0:j0 + step].to(torch.int64) & 0xFFFF
        j = torch.arange(j0, j0 + v.numel(), dtype=torch.int64, device=v.device)
        hi = v >> 8                             # v (2 j + 1) < 2^49 per word: split so that 2^20 of them sum below 2^63
        lin = int((hi * (2 * j + 1)).sum()) * 256 + int(((v & 0xFF) * (2 * j + 1)).sum())
        sq = int((v * v).sum())                 # < 2^32 * 2^20
        total = (total + lin + (sq << 32)) & _M64
    return total


class ParamFingerprint:
    """Fingerprints of a list of named tensors, one value each.  Tensors on a GPU: ONE launch of T2V_OP_FINGERPRINT over a device table
    {address, nbytes} per tensor and a chunk table (FINGERPRINT_CHUNK bytes of one tensor per workgroup), both rebuilt only when an
    address or a size changes; tensors on the CPU: `fingerprint_torch`.  `recorded` holds the values of the last pack (the owner
    stores them there)."""

    def __init__(self):
        self._key = None
        self._tables = None
        self.recorded = None            # name -> value at the end of the last full / partial pack (None: nothing recorded)
        self.last_bytes = 0             # bytes the last device launch read

    @staticmethod
    def chunk_table(sizes):
        """[(segment, chunk)] of byte sizes: every chunk of every segment once; an empty segment keeps its chunk 0."""
        out = []
        for s, nb in enumerate(sizes):
            out.extend((s, c) for c in range(max(1, -(-nb // FINGERPRINT_CHUNK))))
        return out

    def compute_ranges(self, ranges, device, stream=None):
        """ranges: [(address, nbytes)] on `device` (even, readable for the duration of the call) -> [int]; one launch, then one copy back."""
        import ctypes
        import numpy as np
        from . import _lib as L
        if not ranges:
            return []
        for a, nb in ranges:
            if (a | nb) & 1 or nb < 0:
                raise L.T2VError(f"fingerprint: byte range ({a:#x}, {nb}) is not 2-byte aligned")
        key = tuple(ranges)
        if key != self._key or self._tables is None or self._tables[0].device != device:
            chunks = self.chunk_table([nb for _, nb in ranges])
            if len(chunks) >= 1 << 31:
                raise L.T2VError("fingerprint: too many chunks for one launch")
            seg = torch.from_numpy(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2).view(np.int64)).to(device)
            chk = torch.from_numpy(np.asarray(chunks, dtype=np.uint32).reshape(-1, 2).view(np.int32)).to(device)
            out = torch.empty(len(ranges), dtype=torch.int64, device=device)
            self._key, self._tables = key, (seg, chk, out)
        seg, chk, out = self._tables
        op = L.T2VOp()
        op.kind = L.OP_FINGERPRINT
        op.i[0], op.i[1] = len(ranges), chk.shape[0]
        op.p[0], op.p[1], op.p[2] = seg.data_ptr(), out.data_ptr(), chk.data_ptr()
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        L.check(L.load().t2v_run_ops(ctypes.byref(op), 1, None, 0, ctypes.c_void_p(stream)))
        self.last_bytes = sum(nb for _, nb in ranges)
        return [int(v) & _M64 for v in out.cpu().tolist()]

    def compute(self, named, device):
        """named: [(name, tensor)]; device: where the pack lives.  -> {name: value}, or None when the tensors are not fingerprinted:
        they live on the CPU while the pack is on a GPU (hashing gigabytes on the host per call is not acceptable), or on several devices."""
        device = torch.device(device)
        named = [(n, t) for n, t in named if t is not None]
        if not named:
            return {}
        devs = {t.device for _, t in named}
        if len(devs) != 1:
            return None
        src = next(iter(devs))
        if src.type == "cpu":
            if device.type != "cpu":
                return None
            return {n: fingerprint_torch(t) for n, t in named}
        if device.type == "cpu" or src != device:
            return None
        keep = [t if t.is_contiguous() else t.detach().contiguous() for _, t in named]     # (a strided parameter: a dense copy, alive until the copy back)
        ranges = [(t.data_ptr() if t.numel() else 0, t.numel() * t.element_size()) for t in keep]
        vals = self.compute_ranges(ranges, src)
        return {n: v for (n, _), v in zip(named, vals)}
