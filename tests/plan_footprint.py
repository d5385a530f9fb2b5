"""TEST INFRASTRUCTURE — what ONE program record touches: `footprint(op)` -> [Access].

An independent statement of the bytes every op kind reads and writes, derived from the field lists of include/t2v_hip.h, the launchers
and kernels under csrc/ and (for the roles of the pointer slots) `output_slots` in csrc/executor.hip — NOT from tests/interp.py and not
from the lowerings' `Buf` objects: tests/plan_hazards.py checks the lowerings against this table, and tests/test_plan_hazards_cpu.py /
tests/test_gpu_plan_confinement.py check the table against the interpreter and the kernels.

An Access names the space ("arena" | "weight" | "ext"), the pointer slot, a mode ("r" read, "w" written, "scratch" written and read
by this launch only) and the bytes as strided rectangles.  Arenas reach several GB, so nothing here or downstream builds a byte map:
a rectangle is (offset, outer counts, outer pitches, row bytes) and two rectangles are compared exactly through their sorted row
intervals (`Rect.intervals`, `overlap`); the bounding intervals are only the fast path that says "certainly apart".

Reads a kernel performs and discards:
  * the residual prefetch of the GEMM epilogue loads rows / columns outside the matrix from the FIRST element of the residual
    (csrc/t2v_kernels.h:418-430, "park on the first element"): inside the declared rectangle, nothing to add;
  * the large-tile GEMM's operand DMA parks rows past M / N and the padding taps of the convolution gathers on the library's own zero
    page (csrc/gemm2.hip:74-80), not on the arena: nothing to add;
  * T2V_EPI_XATTN reads the V^T rows up to the key count rounded up to 32 ("finite beyond i[25]", include/t2v_hip.h:136-140): declared.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

# mirrors of include/t2v_hip.h (tests/test_abi.py holds the package's own mirror to the header; these are checked against the package's
# by tests/test_plan_hazards_cpu.py::test_footprint_constants)
(GEMM, GROUPNORM, LAYERNORM, ATTENTION, SOFTMAX, NCTHW_TO_CL, CL_TO_NCTHW, TIME_EMBED, COPY2D, DDIM_STEP, MEMSET, LINCOMB, RELPOS_ATTN,
 EMBED_ROWS, TO_UINT8, ALLGATHER, HALO_EXCHANGE, RESHARD_ROWS, ALLTOALL, STATS_HALO, RESAMPLE, DEPTH_TOKENS, AVGPOOL2, EMPHASIS,
 FINGERPRINT) = range(1, 26)
PLAIN, CONV3X3, TCONV3, CONV3X3_C8 = 0, 1, 2, 3
EPI_NONE, EPI_GEGLU, EPI_TATTN, EPI_STATS, EPI_GN, EPI_XATTN = range(6)
F16, F32 = 0, 1
SYNC_INTS, SYNC_BARRIER_INTS, GN_PART_BYTES, GN_ROWS_PER_BLOCK = 4096, 512, 2 << 20, 64
RELPOS_LONG_COLS = lambda R: (2 * R + 158) // 8 * 8

# slots that own the synchronisation words and the exchange-record region (include/t2v_hip.h: GEMM p[7] tickets, p[10], p[11];
# GROUPNORM p[5], p[7]) — accesses through them carry sync=True and are judged by rule R5 alone
SYNC_SLOTS = {GEMM: (7, 10, 11), GROUPNORM: (5, 7)}


@dataclass(frozen=True)
class Rect:
    """Bytes off + sum_d idx_d * pitches[d] + [0, row) for 0 <= idx_d < counts[d]."""
    off: int
    counts: Tuple[int, ...]
    pitches: Tuple[int, ...]
    row: int

    @staticmethod
    def make(off, counts, pitches, row) -> "Rect":
        """Normalised: unit dimensions dropped, a dimension whose pitch equals the extent below it folded into it."""
        dims = [(int(c), int(p)) for c, p in zip(counts, pitches) if c != 1]
        assert row > 0 and all(c > 0 and p >= 0 for c, p in dims), (off, counts, pitches, row)
        row = int(row)
        while dims and dims[-1][1] == row:                     # dense innermost dimension -> longer rows
            row *= dims.pop()[0]
        out = []
        for c, p in reversed(dims):                            # fold outer dims that continue the one inside them
            if out and p == out[0][0] * out[0][1]:
                out[0] = (out[0][0] * c, out[0][1])
            else:
                out.insert(0, (c, p))
        return Rect(int(off), tuple(c for c, _ in out), tuple(p for _, p in out), row)

    @staticmethod
    def mat(off, rows, cols, ld, item) -> "Rect":
        return Rect.make(off, (rows,), (ld * item,), cols * item)

    @staticmethod
    def flat(off, nbytes) -> "Rect":
        return Rect(int(off), (), (), int(nbytes))

    @property
    def lo(self) -> int:
        return self.off

    @property
    def hi(self) -> int:
        return self.off + sum((c - 1) * p for c, p in zip(self.counts, self.pitches)) + self.row

    @property
    def nbytes_upper(self) -> int:
        n = self.row
        for c in self.counts:
            n *= c
        return n

    def shifted(self, d: int) -> "Rect":
        return Rect(self.off + d, self.counts, self.pitches, self.row)

    def intervals(self):
        """Sorted, disjoint, merged [start, end) byte intervals: (starts, ends) int64 arrays — exact."""
        starts = np.array([self.off], dtype=np.int64)
        for c, p in zip(self.counts, self.pitches):
            starts = (starts[:, None] + (np.arange(c, dtype=np.int64) * p)[None, :]).reshape(-1)
        return merge_intervals(starts, starts + self.row)


def merge_intervals(starts, ends):
    if len(starts) <= 1:
        return starts.astype(np.int64), ends.astype(np.int64)
    order = np.argsort(starts, kind="stable")
    s, e = starts[order], ends[order]
    emax = np.maximum.accumulate(e)
    new = np.ones(len(s), dtype=bool)
    new[1:] = s[1:] > emax[:-1]
    idx = np.flatnonzero(new)
    return s[idx], np.maximum.reduceat(e, idx)


def union(rects):
    if not rects:
        z = np.zeros(0, dtype=np.int64)
        return z, z
    parts = [r.intervals() for r in rects]
    return merge_intervals(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


def intersect(a, b):
    """Exact intersection of two sorted disjoint interval lists -> (starts, ends)."""
    (as_, ae), (bs, be) = a, b
    z = np.zeros(0, dtype=np.int64)
    if len(as_) == 0 or len(bs) == 0 or as_[0] >= be[-1] or bs[0] >= ae[-1]:
        return z, z
    cuts = np.unique(np.concatenate([as_, ae, bs, be]))
    lo, hi = cuts[:-1], cuts[1:]
    ia, ib = np.searchsorted(as_, lo, "right") - 1, np.searchsorted(bs, lo, "right") - 1
    ina = (ia >= 0) & (lo < ae[np.maximum(ia, 0)])
    inb = (ib >= 0) & (lo < be[np.maximum(ib, 0)])
    keep = ina & inb
    return merge_intervals(lo[keep], hi[keep])


def subtract(a, b):
    """a minus b, both sorted disjoint interval lists."""
    (as_, ae), (bs, be) = a, b
    if len(as_) == 0 or len(bs) == 0:
        return as_, ae
    cuts = np.unique(np.concatenate([as_, ae, bs, be]))
    lo, hi = cuts[:-1], cuts[1:]
    ia, ib = np.searchsorted(as_, lo, "right") - 1, np.searchsorted(bs, lo, "right") - 1
    ina = (ia >= 0) & (lo < ae[np.maximum(ia, 0)])
    inb = (ib >= 0) & (lo < be[np.maximum(ib, 0)])
    keep = ina & ~inb
    return merge_intervals(lo[keep], hi[keep])


def overlap(ra, rb):
    """First overlapping byte range of two rectangle lists (or Accesses), or None.  Bounding intervals first (apart -> None: the fast
    path); everything else is decided exactly on the row intervals."""
    a_rects, b_rects = getattr(ra, "rects", ra), getattr(rb, "rects", rb)
    if not a_rects or not b_rects:
        return None
    if min(r.lo for r in a_rects) >= max(r.hi for r in b_rects) or min(r.lo for r in b_rects) >= max(r.hi for r in a_rects):
        return None
    s, e = intersect(ra.intervals() if isinstance(ra, Access) else union(ra), rb.intervals() if isinstance(rb, Access) else union(rb))
    return (int(s[0]), int(e[0])) if len(s) else None


@dataclass
class Access:
    space: str                 # "arena" | "weight" | "ext"
    slot: int                  # pointer slot of the record
    mode: str                  # "r" | "w" | "scratch"
    rects: List[Rect]          # arena: arena byte offsets; weight: offsets inside the named image; ext: offsets inside the caller's tensor
    name: str = ""             # weight image name / ext slot number
    sync: bool = False         # through a slot that owns synchronisation words / the exchange-record region
    what: str = ""
    dtype: str = ""            # element type of the bytes (the in-place classes of rule R3 need it)
    ld: int = 0                # leading dimension in elements (0 = dense)
    wrap: int = 0              # row wrap in force on this access
    launch: int = 0            # a record that runs as two launches (a split-K GEMM and its reduction): which of them

    def bounds(self):
        return min(r.lo for r in self.rects), max(r.hi for r in self.rects)

    def intervals(self):
        """union(self.rects), computed once."""
        iv = self.__dict__.get("_iv")
        if iv is None:
            iv = self.__dict__["_iv"] = union(self.rects)
        return iv


class _B:
    """Collects the accesses of one record."""

    def __init__(self, op):
        self.op, self.out, self.launch = op, [], 0

    def add(self, slot, mode, rects, what="", sync=False, dtype="", ld=0, wrap=0):
        ref = self.op.p[slot]
        if ref.space == "null":
            return
        rects = [rects] if isinstance(rects, Rect) else list(rects)
        base = ref.off if ref.space in ("arena", "weight") else 0
        rects = [r.shifted(base) for r in rects if r is not None]
        if not rects:
            return
        name = ref.name if ref.space == "weight" else (str(ref.off) if ref.space == "ext" else "")
        self.out.append(Access(ref.space, slot, mode, rects, name, sync, what, dtype, ld, wrap, self.launch))

    def mat(self, slot, mode, rows, cols, ld, item, what="", col0=0, **kw):
        self.add(slot, mode, Rect.mat(col0 * item, rows, cols, ld, item), what, dtype={2: "f16", 4: "f32", 1: "u8", 8: "f64"}[item], ld=ld, **kw)


def _u64(lo, hi):
    return (lo & 0xFFFFFFFF) | (hi << 32)


def _gemm(op, b: _B):
    I = op.i
    M, N, K, lda, ldw, ldc, ldr, g = I[0:8]
    epi, oitem, split = I[16], (4 if I[17] == F32 else 2), max(I[19], 1)
    if epi == EPI_TATTN:       # include/t2v_hip.h:114-118: tile rows are pixels x frames; the tokens are samples * F * HW
        Fr, HW, pix = I[8], I[9], I[10]
        T = M // 192 // -(-HW // pix) * Fr * HW
        b.mat(0, "r", T, K, lda, 2, "A")
        b.mat(1, "r", N, K, ldw, 2, "W head-major q|k|v")
        b.mat(5, "w", T, N // 192 * 64, ldc, 2, "attention output")
        return
    if epi == EPI_XATTN:       # include/t2v_hip.h:136-140
        aw, rps, ldk, Lc, lcp, ks, vs = I[13], I[15], I[24], I[25], I[26], I[27], I[28]
        samples = M // rps
        b.mat(0, "r", aw if aw else M, K, lda, 2, "A", wrap=aw)
        b.mat(1, "r", N, K, ldw, 2, "W")
        b.add(8, "r", Rect.make(0, (samples, Lc), (2 * ks, 2 * ldk), 2 * N), "text K", dtype="f16")
        b.add(9, "r", Rect.make(0, (samples, N), (2 * vs, 2 * lcp), 2 * min(lcp, -(-Lc // 32) * 32)), "text V^T, keys rounded up to 32", dtype="f16")
        b.mat(5, "w", M, N, ldc, 2, "attention output")
        return
    n_out = N // 2 if epi == EPI_GEGLU else N
    ln = g == PLAIN and I[8] in (1, 2)
    # A operand (include/t2v_hip.h:100-108, 180-193)
    if g == PLAIN:
        b.mat(0, "r", I[13] if I[13] else M, K, lda, 2, "A", wrap=I[13])
    elif g in (CONV3X3, CONV3X3_C8):
        nimg = M // (I[13] * I[14])
        b.mat(0, "r", nimg * I[8] * I[9], I[10], lda, 2, "A images [nimg, Hin, Win, Cin]")
    else:
        nb = M // (I[8] * I[9])
        b.mat(0, "r", nb * (I[8] + (2 if I[23] else 0)) * I[9], I[10], lda, 2, "A clips [nb, F (+2 halo), HW, Cin]")
    b.mat(1, "r", N, K, ldw, 2, "W")
    # split-K without tickets: the GEMM launch stores fp32 slabs and a reduction launch folds them and applies the whole epilogue — bias,
    # row bias, residual, the outputs and a fused GroupNorm belong to that second launch (csrc/t2v_kernels.h:423,455: `p.splitk == 1 &&`
    # guards the residual and bias loads of the GEMM's own epilogue; include/t2v_hip.h:199-201)
    two = split > 1 and (ln or op.p[7].space == "null")
    if two:
        b.add(6, "scratch", Rect.flat(0, split * M * N * 4), "split-K slabs", dtype="f32")
        b.launch = 1
        b.add(6, "scratch", Rect.flat(0, split * M * N * 4), "split-K slabs", dtype="f32")
    b.mat(2, "r", 1, M if I[20] else N, 0, 4, "bias")
    if ln:
        b.mat(3, "r", 1, 2 * N, 0, 4, "LayerNorm gamma | beta")
    elif I[15] > 0:
        b.mat(3, "r", M // I[15], N, I[21], 4, "row bias")
    rw = I[30] if I[30] > 0 else (I[12] if g == PLAIN else 0)
    b.mat(4, "r", rw if rw else M, n_out, ldr, 4, "residual", wrap=rw)
    if not (epi == EPI_GN and I[29] == 1):                     # i[29] = 1: `out` is NOT written (include/t2v_hip.h:132)
        b.mat(5, "w", M, n_out, ldc, oitem, "out")
        if g == PLAIN and I[11] == 1:                          # low-order image at column N + n (include/t2v_hip.h:194-195)
            b.mat(5, "w", M, N, ldc, 2, "out_lo", col0=N)
    if split > 1 and not two:
        b.add(6, "scratch", Rect.flat(0, split * M * N * 4), "split-K slabs", dtype="f32")
        b.add(7, "scratch", Rect.flat(0, SYNC_INTS * 4), "split-K tile tickets", sync=True)
    elif epi == EPI_STATS:
        b.add(7, "w", Rect.flat(0, -(-M // 32) * 2 * N * 4), "statistics strips [ceil(M/32)][2][N]", dtype="f32")
    if ln:
        b.mat(7, "w", M, N, I[9], 2, "ln_out")
        if I[8] == 2:
            b.add(10, "scratch", Rect.flat(0, GN_PART_BYTES), "exchange records", sync=True)
            b.add(11, "scratch", Rect.flat(0, SYNC_BARRIER_INTS * 4), "grid-barrier words", sync=True)
    if epi == EPI_GN:                                          # include/t2v_hip.h:124-135
        b.mat(8, "r", 1, 2 * N, 0, 4, "GroupNorm gamma | beta")
        b.mat(9, "w", M, N, I[25], 2, "gn_out")
        if I[27]:
            b.mat(9, "w", M, N, I[25], 2, "gn_lo", col0=N)
        b.add(10, "scratch", Rect.flat(0, GN_PART_BYTES), "exchange records", sync=True)
        b.add(11, "scratch", Rect.flat(0, SYNC_BARRIER_INTS * 4), "grid-barrier words", sync=True)


def _groupnorm(op, b: _B):
    I = op.i
    n_inst, rows, C, ld_in, groups, in_dt, _silu, ld_out, phase, nparts, part, rpb = I[0:12]
    nparts, item = max(nparts, 1), (4 if in_dt == F32 else 2)
    before, after = (I[21], I[22]) if phase == 2 else (0, 0)
    strips = op.p[6].space != "null" and phase in (1, 3)
    total = n_inst * rows + before + after
    if not (phase == 1 and strips):        # phase 1 from the producer's strips makes no pass over the tensor (include/t2v_hip.h:211-212)
        b.add(0, "r", Rect.mat(0, total, C, ld_in, item).shifted(-before * ld_in * item), "x (+ received boundary frames)", dtype="f32" if item == 4 else "f16", ld=ld_in)
    if strips:
        b.add(6, "r", Rect.flat(0, n_inst * (rows // 32) * 2 * I[17] * 4), "producer strips", dtype="f32")
    nblk = -(-rows // (rpb if rpb > 0 else GN_ROWS_PER_BLOCK))
    blk, fin, pb = n_inst * nblk * groups * 16, n_inst * groups * 8, n_inst * groups * 16
    if phase in (0, 3):
        b.add(4, "scratch", Rect.flat(0, blk + fin), "block partials, {mean, rstd}")
    elif phase == 1:
        b.add(4, "w", Rect.flat(part * pb, pb), "this rank's statistics part")
        b.add(4, "scratch", Rect.flat(nparts * pb, blk + fin), "block partials, finals (csrc/norm.hip:932-943: both fold kernels write them)")
    else:
        b.add(4, "r", Rect.flat(0, nparts * pb), "gathered statistics parts")
        b.add(4, "scratch", Rect.flat(nparts * pb + blk, fin), "{mean, rstd}")
    if phase != 1:
        b.mat(1, "r", 1, C, 0, 4, "gamma")
        b.mat(2, "r", 1, C, 0, 4, "beta")
        b.add(3, "w", Rect.mat(0, total, C, ld_out, 2).shifted(-before * ld_out * 2), "out", dtype="f16", ld=ld_out)
        if I[16]:
            b.add(3, "w", Rect.mat(2 * C, total, C, ld_out, 2).shifted(-before * ld_out * 2), "out low-order image", dtype="f16", ld=ld_out)
        b.mat(8, "w", n_inst * rows, C, I[19], 2, "raw cast")
        if I[20] > 0:
            b.mat(8, "w", n_inst * rows, C, I[19], 2, "raw cast low-order image", col0=I[20])
    if I[15]:
        b.add(5, "scratch", Rect.flat(0, SYNC_BARRIER_INTS * 4), "grid-barrier words", sync=True)
        if I[18] > 0:
            b.add(7, "scratch", Rect.flat(0, I[18]), "exchange records", sync=True)


def _attention(op, b: _B):
    I = op.i
    rel = op.kind == RELPOS_ATTN
    nq, nk, heads, bo, bi = I[0:5]
    D = I[14] if I[14] > 0 else 64
    sq, sk, so = I[5:8], I[8:11], I[11:14]
    row = heads * D * 2

    def seq(n, s, outer=bo, outer_stride=None):
        return Rect.make(0, (outer, bi, n), (2 * (s[1] if outer_stride is None else outer_stride), 2 * s[2], 2 * s[0]), row)

    alt = 0 if rel else I[19]
    b.add(0, "r", seq(nq, sq), "q", dtype="f16")
    for slot in (1, 2):
        b.add(slot, "r", seq(nk, sk, outer=alt if alt else bo), "k / v", dtype="f16")
    if alt:                                                    # include/t2v_hip.h:241-245
        for slot in (4, 5):
            b.add(slot, "r", seq(I[20], sk, outer=bo - alt, outer_stride=I[21]), "second role k / v", dtype="f16")
    b.add(3, "w", seq(nq, so), "out", dtype="f16")
    lo_off = I[18] if rel else I[16]
    if lo_off:
        b.add(3, "w", seq(nq, so).shifted(2 * lo_off), "out low-order image", dtype="f16")
    if rel:
        R, sel = I[15], I[17]
        for slot in (4, 5):
            b.mat(slot, "r", 2 * R + 1, D, D, 4, "Ek / Ev")
        if sel == 2:
            b.add(6, "r", Rect.flat(0, 32 * (-(-D // 16) * 16) * 2), "Ek packed")
            b.add(7, "r", Rect.flat(0, (-(-D // 32) * 32) * 32 * 2), "Ev^T packed")
        elif sel == 3:
            b.add(6, "r", Rect.flat(0, (2 * R + 1) * (-(-D // 16) * 16) * 2), "Ek packed (long)")
            b.add(7, "r", Rect.flat(0, (-(-D // 32) * 32) * RELPOS_LONG_COLS(R) * 2), "Ev^T packed (long)")
    elif op.p[6].space != "null":                              # include/t2v_hip.h:238-240: V^T scratch fp16 [bo * bi * heads * 64, i[17]]
        b.add(6, "scratch", Rect.flat(0, bo * bi * heads * 64 * I[17] * 2), "V^T scratch", dtype="f16")


def _reshard(op, b: _B):
    I = op.i
    rows, cols, P, s_src, s_dst, ld_src, ld_dst, dt, ld_res = I[0:9]
    item = 4 if dt == F32 else 2
    nparts = I[9] if I[9] > 1 else 1
    ps_src, ps_dst, ps_res, own, own_is_src = I[10:15] if nparts > 1 else (0, 0, 0, -1, 0)

    def grid(stride, ld, it):
        full, tail = rows // P, rows % P
        out = []
        if full:
            out.append(Rect.make(0, (full, P), (stride * ld * it, ld * it), cols * it))
        if tail:
            out.append(Rect.make(full * stride * ld * it, (tail,), (ld * it,), cols * it))
        return out

    src, dst, res = grid(s_src, ld_src, item), grid(s_dst, ld_dst, item), grid(s_dst, ld_res, 4)
    dts = "f32" if item == 4 else "f16"
    for q in range(nparts):
        if q == own and own_is_src:
            b.add(3, "r", src, "own part (source)", dtype=dts, ld=ld_src)
        else:
            b.add(0, "r", [r.shifted(q * ps_src * item) for r in src], "src", dtype=dts, ld=ld_src)
        if q == own and not own_is_src:
            b.add(3, "w", dst, "own part (destination)", dtype=dts, ld=ld_dst)
        else:
            b.add(1, "w", [r.shifted(q * ps_dst * item) for r in dst], "dst", dtype=dts, ld=ld_dst)
        b.add(2, "r", [r.shifted(q * ps_res * 4) for r in res], "residual", dtype="f32", ld=ld_res)


def footprint(op) -> List[Access]:
    """Every access of one record (a program.Op: symbolic pointers, so arena offsets are arena-relative)."""
    b, I, k = _B(op), op.i, op.kind
    if k == GEMM:
        _gemm(op, b)
    elif k == GROUPNORM:
        _groupnorm(op, b)
    elif k == LAYERNORM:
        M, C, ld_in, ld_out = I[0:4]
        b.mat(0, "r", M, C, ld_in, 4, "x")
        b.mat(1, "r", 1, C, 0, 4, "gamma")
        b.mat(2, "r", 1, C, 0, 4, "beta")
        b.mat(3, "w", M, C, ld_out, 2, "out")
    elif k in (ATTENTION, RELPOS_ATTN):
        _attention(op, b)
    elif k == SOFTMAX:
        b.mat(0, "r", I[0], I[1], I[2], 4, "in")
        b.mat(1, "w", I[0], I[1], I[3], 2, "out")
    elif k == NCTHW_TO_CL:
        B, C, Fr, HW, ld, in_dt = I[0:6]
        Bsrc = I[6] if 0 < I[6] < B else B
        b.add(0, "r", Rect.flat(0, Bsrc * C * Fr * HW * (4 if in_dt == F32 else 2)), "NCTHW source", dtype="f32" if in_dt == F32 else "f16")
        # the whole row of ld channels is written: the values, (i[7]) their low-order images, zeros beyond (csrc/elementwise.hip ncthw_to_cl)
        b.mat(1, "w", B * Fr * HW, ld, ld, 2, "tokens (all ld channels)")
        b.mat(2, "w", B * Fr * HW, ld, ld, 2, "low-order tokens (all ld channels)")
    elif k == CL_TO_NCTHW:
        B, C, Fr, HW, ld, out_dt = I[0:6]
        b.mat(0, "r", B * Fr * HW, C, ld, 4, "tokens")
        b.add(1, "w", Rect.flat(0, B * C * Fr * HW * (4 if out_dt == F32 else 2)), "NCTHW destination", dtype="f32" if out_dt == F32 else "f16")
    elif k == TIME_EMBED:
        b.mat(0, "r", 1, I[0], 0, 4, "t")
        b.mat(1, "r", 1, I[1] // 2, 0, 4, "freqs")
        b.mat(2, "w", I[0], I[1], I[1], 2, "out")
    elif k == COPY2D:
        rows, cols, lds, ldd, sdt, ddt = I[0:6]
        b.mat(0, "r", rows, cols, lds, 4 if sdt == F32 else 2, "src")
        b.mat(1, "w", rows, cols, ldd, 4 if ddt == F32 else 2, "dst")
        b.mat(2, "w", rows, cols, ldd, 2, "low-order image")
    elif k == DDIM_STEP:
        n = I[0] * I[1]
        ei, xi = (4 if I[3] == F32 else 2), (4 if I[4] == F32 else 2)
        de, dx = ("f32" if ei == 4 else "f16"), ("f32" if xi == 4 else "f16")
        b.add(0, "r", Rect.flat(0, n * xi), "x_t", dtype=dx)
        b.add(1, "r", Rect.flat(0, (2 if I[2] > 0 else 1) * n * ei), "eps (pair when guided)", dtype=de)
        b.add(2, "r", Rect.flat(0, n * 4), "eta noise", dtype="f32")
        b.add(3, "w", Rect.flat(0, n * xi), "x_{t-1}", dtype=dx)
        if I[7]:
            for slot in (4, 5, 6):
                b.add(slot, "r", Rect.flat(0, n * 4), "known x0 / mask / q-noise", dtype="f32")
    elif k == MEMSET:
        b.add(0, "w", Rect.flat(0, max(_u64(I[0], I[1]), 1)), "zeroed bytes")
    elif k == LINCOMB:
        for j in range(I[1]):
            b.add(j, "r", Rect.flat(0, I[0] * (4 if I[3 + j] == F32 else 2)), "term", dtype="f32" if I[3 + j] == F32 else "f16")
        b.add(6, "w", Rect.flat(0, I[0] * (4 if I[2] == F32 else 2)), "out", dtype="f32" if I[2] == F32 else "f16")
    elif k == EMBED_ROWS:
        rows, W, Lp, vocab, tdt = I[0:5]
        b.add(0, "r", Rect.flat(0, rows * 4), "ids", dtype="i32")
        b.add(1, "r", Rect.flat(0, vocab * W * (4 if tdt == F32 else 2)), "table", dtype="f32" if tdt == F32 else "f16")
        b.add(2, "r", Rect.flat(0, Lp * W * 4), "positions", dtype="f32")
        b.mat(3, "w", rows, W, W, 4, "out")
    elif k == TO_UINT8:
        NI, C, Fr, H, W, in_dt = I[0:6]
        item = 4 if in_dt == F32 else 2
        si, sc, sf, sy, sx = _u64(I[8], I[9]), I[10], _u64(I[11], I[12]), I[13], I[14]
        b.add(0, "r", Rect.make(0, (NI, C, Fr, H, W), (si * item, sc * item, sf * item, sy * item, sx * item), item), "float video", dtype="f32" if item == 4 else "f16")
        b.add(1, "w", Rect.flat(0, Fr * H * NI * W * C), "uint8 frames", dtype="u8")
    elif k == ALLGATHER:
        nb, n, me = _u64(I[0], I[1]), I[2], I[3]
        b.add(0, "r", Rect.flat(me * nb, nb), "this rank's part")
        b.add(0, "w", [Rect.flat(q * nb, nb) for q in range(n) if q != me], "the other ranks' parts")
    elif k in (HALO_EXCHANGE, STATS_HALO):
        if k == STATS_HALO:
            nb, n, me = _u64(I[0], I[1]), I[2], I[3]
            b.add(0, "r", Rect.flat(me * nb, nb), "this rank's statistics part")
            b.add(0, "w", [Rect.flat(q * nb, nb) for q in range(n) if q != me], "the other ranks' parts")
            slot, fb, Fr, prev, nxt = 1, _u64(I[4], I[5]), I[6], I[7], I[8]
        else:
            slot, fb, Fr, prev, nxt = 0, _u64(I[0], I[1]), I[2], I[3], I[4]
        b.add(slot, "r", [Rect.flat(f * fb, fb) for f, peer in ((1, prev), (Fr, nxt)) if peer >= 0], "boundary frames sent")
        b.add(slot, "w", [Rect.flat(f * fb, fb) for f, peer in ((0, prev), (Fr + 1, nxt)) if peer >= 0], "halo frames received")
    elif k == RESHARD_ROWS:
        _reshard(op, b)
    elif k == ALLTOALL:
        nb, n, me, base, last, direction = _u64(I[0], I[1]), I[2], I[3], I[4], I[5], I[6]
        cnt = lambda q: last if q == n - 1 else base
        peers = [q for q in range(n) if q != me]
        if direction == 0:
            b.add(0, "r", [Rect.flat(q * cnt(me) * nb, cnt(me) * nb) for q in peers], "sent chunks")
            b.add(1, "w", [Rect.flat(q * base * nb, cnt(q) * nb) for q in peers], "received chunks")
        else:
            b.add(0, "r", [Rect.flat(q * base * nb, cnt(q) * nb) for q in peers], "sent chunks")
            b.add(1, "w", [Rect.flat(q * cnt(me) * nb, cnt(me) * nb) for q in peers], "received chunks")
    elif k == RESAMPLE:
        Nn, H, W, _c, out, axis, ksize, form, ld = I[0:9]
        b.add(0, "r", Rect.flat(0, Nn * H * W * 3), "uint8 source", dtype="u8")
        px = Nn * (H * out if axis == 0 else out * W)
        b.add(1, "w", Rect.flat(0, px * (3 if form == 0 else ld * (4 if form == 1 else 2))), "destination (token forms: all ld channels)", dtype=("u8", "f32", "f16")[form])
        b.add(2, "r", Rect.flat(0, out * ksize * 4), "coefficients", dtype="i32")
        b.add(3, "r", Rect.flat(0, out * 8), "bounds", dtype="i32")
        if form:
            b.add(4, "r", Rect.flat(0, 1024), "value table", dtype="f32")
    elif k == DEPTH_TOKENS:
        n, H, W, in_dt, _norm, ld = I[0:6]
        b.add(0, "r", Rect.flat(0, n * H * W * (4 if in_dt == F32 else 2)), "depth frames", dtype="f32" if in_dt == F32 else "f16")
        b.mat(1, "w", n * (H // 8) * (W // 8), 64, ld, 2, "tokens (columns 64 .. ld-1 are not written)")
    elif k == AVGPOOL2:
        n, H, W, C, ld_in, ld32, ld16 = I[0:7]
        Ho, Wo = H // 2, W // 2
        b.add(0, "r", Rect.make(0, (n, 2 * Ho, 2 * Wo), (H * W * ld_in * 4, W * ld_in * 4, ld_in * 4), C * 4), "images (a last odd row / column is dropped)", dtype="f32")
        b.mat(1, "w", n * Ho * Wo, C, ld32, 4, "fp32 mean")
        b.mat(2, "w", n * Ho * Wo, C, ld16, 2, "fp16 mean")
    elif k == EMPHASIS:
        rows, W, ldz, ldo, zdt = I[0:5]
        b.mat(0, "r", rows, W, ldz, 4 if zdt == F32 else 2, "z")
        b.add(1, "r", Rect.flat(0, rows * 4), "multipliers", dtype="f32")
        b.mat(2, "w", rows, W, ldo, 4, "out")
    elif k == FINGERPRINT:     # stand-alone (never part of a plan); the segments themselves are named by the table, not by the record
        b.add(0, "r", Rect.flat(0, I[0] * 16), "segment table")
        b.add(2, "r", Rect.flat(0, I[1] * 8), "chunk table")
        b.add(1, "w", Rect.flat(0, I[0] * 8), "fingerprints")
    else:
        raise KeyError(f"no footprint for op kind {k} ({op.name})")
    return b.out
