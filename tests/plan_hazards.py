"""TEST INFRASTRUCTURE — arena hazards of a lowered program, per op and per byte.

`Recorder` wraps Program.alloc, Program.free and Arena.free while a lowering runs (installed with monkeypatch: nothing in the package
changes) and yields every allocation with the op count at its birth and at its ACTUAL release (deferred frees included).
`check(prog, events)` evaluates the rules below on the footprints of tests/plan_footprint.py for both plans of a program — the full op
list, then the list without the `step_invariant` ops starting from the state the first pass left — and returns a list of Hazard.

R1  written before read: every arena byte an op reads has a last writer earlier in the pass (pass 2: possibly from pass 1).
    One exemption, and only with the row's TShardSpec at hand: the slices of a T-sharded clip are padded to the longest one, so on the
    rank that holds the SHORT LAST slice the tail of its own part of an ALLGATHER — bytes [part * frames / max_frames, part) — is padding
    that travels unwritten.  That tail is left out of R1, the writer's-life half of R2 and R4 for that one read, and only if NO byte of it
    has a writer inside the allocation's life (a part whose tail is real data, such as a statistics part, is judged whole).  Every other
    byte any collective sends is judged like any other read.  Report.padding_exempt counts the reads it applied to; the test pins it per row.
R2  inside one live allocation: every access rectangle lies inside a single allocation that is live at that op (an allocation made
    between op j and op j + 1 counts as live for op j: the peepholes fold into the op emitted last; release = the actual Arena.free),
    and the last writer of every byte read wrote it during that same allocation's life.
    KNOWN LIMIT: if a block is reused by an allocation that contains the old rectangle ENTIRELY and an op of the new life writes the
    bytes before the stale reader runs, the reader finds "an allocation that is live and holds its rectangle" and a writer inside that
    life: the rule cannot tell the two lives apart (the reader's record does not say which allocation it meant).  It is caught only when
    the reader runs before the new life's first writer (R2: writer of another life) or the rectangle straddles the new block.
R3  no overlap inside one launch: a launch's written rectangles overlap none of its read rectangles and none of its other written
    ones, except the closed list INPLACE_CLASSES (record fields only).  A pair the library runs as one launch (R6) is one launch.
R4  step-invariant data: in pass 2 every read has the same last writer as in pass 1; an invariant op reads only ext, weights and
    invariant-written bytes; bytes an invariant op wrote and a non-invariant op reads are never released and never written by a
    non-invariant op.
R5  synchronisation words: `_sync` is the first allocation; `_sync` and `_gn_part` are touched only through the slots that own them
    (plan_footprint.SYNC_SLOTS), inside the region each slot is meant for; no other rectangle overlaps them.
R6  the fused feed-forward pair: the plan-time decision of csrc/executor.hip ff_pair modelled twice — as the library makes it
    (ff_pair_library: bounding ranges per pointer slot; tests/test_plan_hazards_cpu.py holds the model to the built library through
    t2v_plan_num_launches) and exactly, on the rectangles of the footprints (ff_pair_extent).  ff_pair_pointer is the scan on base
    pointers the library used to make.  Where the library would fuse, no later record may read a byte of the hidden
    tensor before some record rewrites it, and the result must not lie over X, W1 or b1 — by extent.  A disagreement is a hazard.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

import plan_footprint as FP
from plan_footprint import Access, Rect, footprint, intersect, merge_intervals, overlap, subtract, union

FF_MIN_M = 49152          # csrc/executor.hip FF_MIN_M_DEFAULT


# ------------------------------------------------------------------------------------------------------------------------------------
# the recorder
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Alloc:
    id: int
    off: int
    size: int
    born: int                       # len(prog.ops) when Program.alloc returned
    died: Optional[int] = None      # len(prog.ops) at the actual Arena.free (None: never released)
    asked: Optional[int] = None     # len(prog.ops) when Program.free was first called on it (a deferred free: asked < died)

    @property
    def end(self):
        return self.off + self.size


class Recorder:
    def __init__(self):
        self._by_arena: Dict[int, tuple] = {}          # id(arena) -> (prog, [Alloc])

    def install(self, monkeypatch):
        from sd_webui_text2video_amd import program as PG
        rec, p_alloc, p_free, a_free = self, PG.Program.alloc, PG.Program.free, PG.Arena.free

        def alloc(self, rows, cols, dtype, ld=None):
            buf = p_alloc(self, rows, cols, dtype, ld)
            _, events = rec._by_arena.setdefault(id(self.arena), (self, []))
            events.append(Alloc(len(events), buf.alloc_off, self.arena.live[buf.alloc_off], len(self.ops)))
            return buf

        def free(self, *bufs):
            entry = rec._by_arena.get(id(self.arena))
            if entry is not None:
                for b in bufs:
                    if b is not None and b.alloc_off >= 0:
                        for a in reversed(entry[1]):
                            if a.off == b.alloc_off and a.died is None:
                                if a.asked is None:
                                    a.asked = len(self.ops)
                                break
            return p_free(self, *bufs)

        def arena_free(self, off):
            entry = rec._by_arena.get(id(self))
            if entry is not None:
                prog, events = entry
                for a in reversed(events):
                    if a.off == off and a.died is None:
                        a.died = len(prog.ops)
                        break
            return a_free(self, off)

        monkeypatch.setattr(PG.Program, "alloc", alloc)
        monkeypatch.setattr(PG.Program, "free", free)
        monkeypatch.setattr(PG.Arena, "free", arena_free)
        return self

    def events(self, prog) -> List[Alloc]:
        return self._by_arena[id(prog.arena)][1]


# ------------------------------------------------------------------------------------------------------------------------------------
# results
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Hazard:
    rule: str
    ops: list                 # [(index, name), ...] — the first is the op the rule fired at
    slots: list
    byte_range: tuple
    detail: str = ""
    plan: str = "full"

    @property
    def op(self):
        return self.ops[0][0]

    def __str__(self):
        return (f"{self.rule} [{self.plan}] " + " / ".join(f"op {i} {n}" for i, n in self.ops) +
                f" slots {self.slots} bytes [{self.byte_range[0]}, {self.byte_range[1]}) {self.detail}")


@dataclass
class Report:
    hazards: List[Hazard] = field(default_factory=list)
    ops: int = 0
    accesses: int = 0
    allocations: int = 0
    inplace: Dict[str, int] = field(default_factory=dict)
    fused_pairs: Dict[str, list] = field(default_factory=dict)
    seconds: float = 0.0
    roles: set = field(default_factory=set)      # (kind, slot, mode, slot is in csrc/executor.hip output_slots)
    padding_exempt: int = 0       # ALLGATHER reads whose padding tail was left out (module docstring, R1)
    carried: object = None        # pass 2: (starts, ends) of the arena bytes whose last writer is a pass-1 (invariant) op


# ------------------------------------------------------------------------------------------------------------------------------------
# R3: the closed list of in-place classes.  Each: (name, predicate(op, written access, other access), the kernel line that shows the
# SAME thread reads the element before it writes it).  Conditions are record fields alone: identical base, pitch and dtype, no wrap.
# ------------------------------------------------------------------------------------------------------------------------------------
def _same_view(op, w: Access, r: Access, sw: int, sr: int) -> bool:
    return (w.slot == sw and r.slot == sr and op.p[sw] == op.p[sr] and w.ld == r.ld and w.dtype == r.dtype and not r.wrap and not w.wrap
            and w.what in ("out", "dst") )


def _gemm_res_is_out(op, w, r):
    # out[m, n] = acc + res[m, n]: the lane that loads res (m, n .. n+3) is the lane that stores out (m, n .. n+3)
    return (op.kind == FP.GEMM and _same_view(op, w, r, 5, 4) and op.i[5] == op.i[6] and op.i[17] == FP.F32 and op.i[16] != FP.EPI_GEGLU
            and op.i[12 if op.i[7] == FP.PLAIN else 30] == 0 and op.i[30] == 0)


def _copy_in_place(op, w, r):
    return (op.kind == FP.COPY2D and w.slot == 1 and r.slot == 0 and op.p[0] == op.p[1] and op.i[2] == op.i[3] and op.i[4] == op.i[5]
            and op.p[2].space == "null")


INPLACE_CLASSES = [
    ("gemm residual == out (fp32, same ld, no wrap)", _gemm_res_is_out,
     "csrc/t2v_kernels.h:423-430 res_load and :456-460 the store: row mt + rrow + 8 i, columns n .. n + 3 of the same lane"),
    ("copy2d src == dst (same ld and dtype, no low-order image)", _copy_in_place,
     "csrc/elementwise.hip:93-122 copy2d_kernel: a thread loads its 4 elements s[0..3] into registers, then stores d[0..3] at the same place"),
]


# ------------------------------------------------------------------------------------------------------------------------------------
# R6: the two models of ff_pair
# ------------------------------------------------------------------------------------------------------------------------------------
_ARENA_BASE, _WEIGHT_BASE, _WEIGHT_STEP = 1 << 44, 1 << 45, 1 << 38


class _Addr:
    """Pointer values as BoundProgram would resolve them, over made-up bases that keep the spaces apart."""

    def __init__(self):
        self.names = {}

    def __call__(self, ref) -> int:
        if ref.space == "null":
            return 0
        if ref.space == "ext":
            return ref.off
        if ref.space == "arena":
            return _ARENA_BASE + ref.off
        return _WEIGHT_BASE + self.names.setdefault(ref.name, len(self.names)) * _WEIGHT_STEP + ref.off


# slots only written, per kind: csrc/executor.hip output_slots (tests/test_plan_hazards_cpu.py parses the source and compares)
OUTPUT_SLOTS = {FP.GEMM: (5, 6, 7, 10, 11), FP.GROUPNORM: (3, 4, 5, 7, 8), FP.LAYERNORM: (3,), FP.ATTENTION: (3, 6), FP.RELPOS_ATTN: (3,),
                FP.SOFTMAX: (1,), FP.NCTHW_TO_CL: (1, 2), FP.CL_TO_NCTHW: (1,), FP.TIME_EMBED: (2,), FP.COPY2D: (1, 2), FP.DDIM_STEP: (3,),
                FP.MEMSET: (0,), FP.LINCOMB: (6,), FP.EMBED_ROWS: (3,), FP.TO_UINT8: (1,), FP.RESAMPLE: (1,), FP.DEPTH_TOKENS: (1,),
                FP.AVGPOOL2: (1, 2), FP.EMPHASIS: (2,), FP.FINGERPRINT: (1,), FP.RESHARD_ROWS: (1,), FP.ALLTOALL: (1,)}


def output_slots(op):
    s = set(OUTPUT_SLOTS.get(op.kind, ()))
    if op.kind == FP.GEMM and op.i[16] == FP.EPI_GN:
        s.add(9)
    return s


def _ff_shape(ops, k, A, min_m) -> bool:
    """The record-shape conditions of ff_pair (csrc/executor.hip ff_pair, stated there on two decoded views), shared by both models."""
    if k + 1 >= len(ops):
        return False
    a, b = ops[k], ops[k + 1]
    if a.kind != FP.GEMM or b.kind != FP.GEMM:
        return False
    ai, bi, M = a.i, b.i, a.i[0]
    if ai[16] != FP.EPI_GEGLU or ai[7] != FP.PLAIN or ai[19] > 1 or ai[1] != 2560 or ai[2] != 320 or ai[17] != FP.F16:
        return False
    if ai[3] < 320 or ai[4] < 320 or ai[5] < 1280 or ai[8] or ai[11] or ai[12] or ai[13] or ai[18] or ai[20] or ai[30]:
        return False
    if A(a.p[0]) == 0 or A(a.p[1]) == 0 or A(a.p[3]) or A(a.p[4]) or A(a.p[5]) < 16:
        return False
    if bi[16] != FP.EPI_NONE or bi[7] != FP.PLAIN or bi[19] > 1 or bi[1] != 320 or bi[2] != 1280 or bi[8]:
        return False
    if bi[0] != M or A(b.p[0]) != A(a.p[5]) or bi[3] != ai[5] or bi[4] < 1280 or bi[13] or bi[20] or A(b.p[1]) == 0 or A(b.p[5]) == 0:
        return False
    if bi[12] and bi[30]:
        return False
    if M < (1 if ai[31] == 1 else min_m):
        return False
    if A(a.p[0]) < 16 or A(a.p[1]) < 16 or (A(a.p[2]) and A(a.p[2]) < 16) or A(b.p[5]) < 16:
        return False
    return True


def ff_pair_pointer(ops, k, A, min_m=FF_MIN_M, fps=None) -> bool:
    """The scan on BASE POINTERS, as csrc/executor.hip ff_pair made it before it looked at extents: kept as the model that shows what a
    pointer comparison misses (the seeded R6 case hands it to analyse as `ff_model`)."""
    if not _ff_shape(ops, k, A, min_m):
        return False
    a, b, M = ops[k], ops[k + 1], ops[k].i[0]
    o0 = A(b.p[5])
    o1 = o0 + ((M - 1) * b.i[5] + 320 * (2 if b.i[11] == 1 else 1)) * (4 if b.i[17] == FP.F32 else 2)
    apart = lambda r0, n: r0 == 0 or o1 <= r0 or o0 >= r0 + n
    if not apart(A(a.p[0]), ((M - 1) * a.i[3] + 320) * 2) or not apart(A(a.p[1]), (2559 * a.i[4] + 320) * 2) or not apart(A(a.p[2]), 2560 * 4):
        return False
    lo = A(a.p[5])
    hi = lo + ((M - 1) * a.i[5] + 1280) * 2
    for j in range(k + 1, len(ops)):
        outs, rewritten = output_slots(ops[j]), False
        for q, ref in enumerate(ops[j].p):
            v = A(ref)
            if v < lo or v >= hi:
                continue
            if j == k + 1 and q == 0:
                continue
            if q not in outs or j == k + 1:
                return False
            rewritten = True
        if rewritten:
            break
    return True


def ff_pair_library(ops, fps, k, A, min_m=FF_MIN_M) -> bool:
    """csrc/executor.hip ff_pair as it is now: the shape conditions, the result apart from X, W1, b1 (on base pointers and bounding
    extents), then the scan of the later records by the BOUNDING range of every pointer slot (slot_range) over the bytes of the hidden
    tensor that no DENSE output range has rewritten yet; a read is also fine when an earlier STRIDED output range holds every byte of it
    (range_inside).  Conservative where the exact model (ff_pair_extent) is exact: other strided accesses count with their bounding range."""
    if not _ff_shape(ops, k, A, min_m):
        return False
    a, b, M = ops[k], ops[k + 1], ops[k].i[0]
    o0 = A(b.p[5])
    o1 = o0 + ((M - 1) * b.i[5] + 320 * (2 if b.i[11] == 1 else 1)) * (4 if b.i[17] == FP.F32 else 2)
    apart = lambda r0, n: r0 == 0 or o1 <= r0 or o0 >= r0 + n
    if not apart(A(a.p[0]), ((M - 1) * a.i[3] + 320) * 2) or not apart(A(a.p[1]), (2559 * a.i[4] + 320) * 2) or not apart(A(a.p[2]), 2560 * 4):
        return False
    if a.p[5].space != "arena":
        return False
    lo = a.p[5].off
    hi = lo + ((M - 1) * a.i[5] + 1280) * 2
    left, strided = [(lo, hi)], []

    def geometry(xs):
        """(b, e, rows, pitch, row bytes) of a slot: rows of equal length at one pitch (rows == 1: one flat run), or rows == 0 when only
        the bound is known — slot_range's SlotRange."""
        s, e = union([r for x in xs for r in x.rects])
        b0, e0 = int(s[0]), int(e[-1])
        if len(s) == 1:
            return b0, e0, 1, 0, e0 - b0
        if all(len(r.counts) <= 1 for x in xs for r in x.rects) and len(set((e - s).tolist())) == 1 and len(set(np.diff(s).tolist())) == 1:
            return b0, e0, len(s), int(s[1] - s[0]), int(e[0] - s[0])
        return b0, e0, 0, 0, 0

    def inside(r, w):
        (rb, re_, rrows, rp, rrow), (wb, we, wrows, wp, wrow) = r, w
        if rrows <= 0 or wrows <= 0 or rb < wb or re_ > we:
            return False
        if wrows == 1:
            return True
        i0, c = divmod(rb - wb, wp)
        if c + rrow > wrow:
            return False
        return i0 < wrows if rrows == 1 else (rp == wp and i0 + rrows <= wrows)

    for j in range(k + 1, len(ops)):
        outs, slots = output_slots(ops[j]), {}
        for x in fps[j]:
            if x.space == "arena":
                slots.setdefault(x.slot, []).append(x)
        ranges = {q: geometry(xs) for q, xs in slots.items()}
        for q, g in sorted(ranges.items()):
            if j == k + 1 and q == 0:
                continue
            if not any(g[0] < s1 and s0 < g[1] for s0, s1 in left):
                continue
            if q in outs and j != k + 1:
                continue
            if not any(inside(g, w) for w in strided):
                return False
        for q, g in sorted(ranges.items()):
            if q not in outs:
                continue
            b0, e0, rows, pitch, rowb = g
            if rows != 1:
                if rows <= 0 or b0 >= hi or lo >= e0:
                    continue
                t = 0                                      # adjacent column slices of the same rows join; slices that fill the pitch are dense
                while t < len(strided):
                    ob, oe, orows, op_, orow = strided[t]
                    after = orows == rows and op_ == pitch and ob + orow == b0
                    before = orows == rows and op_ == pitch and b0 + rowb == ob
                    if not after and not before:
                        t += 1
                        continue
                    if after:
                        b0 = ob
                    rowb += orow
                    e0 = b0 + (rows - 1) * pitch + rowb
                    del strided[t]
                    t = 0
                if rowb < pitch:
                    strided.append((b0, e0, rows, pitch, rowb))
                    continue
            rest = []
            for s0, s1 in left:
                if e0 <= s0 or b0 >= s1:
                    rest.append((s0, s1))
                    continue
                if s0 < b0:
                    rest.append((s0, b0))
                if e0 < s1:
                    rest.append((e0, s1))
            left = rest
        if not left:
            break
    return True


def ff_pair_extent(ops, fps, k, A, min_m=FF_MIN_M):
    """The same decision on extents: (fuses, reason, the byte range the reason is about — the hidden tensor's own where nothing narrower
    applies).  Shape conditions as the library's; the result apart from X, W1, b1 and from the
    hidden tensor, and no later record reading a byte of the hidden tensor that no record has rewritten since, by footprint."""
    if not _ff_shape(ops, k, A, min_m):
        return False, "shape", (0, 0)
    fa, fb = fps[k], fps[k + 1]
    hidden = [x for x in fa if x.slot == 5 and x.mode == "w"]
    result = [x for x in fb if x.mode in ("w", "scratch") and not x.sync]
    if any(x.space != "arena" for x in hidden):
        return False, "hidden tensor outside the arena", (0, 0)
    whole = (min(x.bounds()[0] for x in hidden), max(x.bounds()[1] for x in hidden))
    for w in result:
        for r in [x for x in fa if x.mode == "r"] + hidden:
            if w.space == r.space and w.name == r.name and overlap(w, r) is not None:
                return False, f"result (slot {w.slot}) over slot {r.slot} of the GEGLU record", (overlap(w, r) if w.space == "arena" else whole)
    left = union([r for x in hidden for r in x.rects])
    for j in range(k + 1, len(ops)):
        touching = [x for x in fps[j] if x.space == "arena" and not x.sync and x.bounds()[0] < left[1][-1] and x.bounds()[1] > left[0][0]]
        for x in touching:
            if x.mode != "r" or (j == k + 1 and x.slot == 0):
                continue
            s, e = intersect(x.intervals(), left)
            if len(s):
                return False, f"op {j} {ops[j].name} slot {x.slot} reads hidden bytes [{int(s[0])}, {int(e[0])})", (int(s[0]), int(e[0]))
        for x in touching:
            if x.mode in ("w", "scratch"):
                left = subtract(left, x.intervals())
                if len(left[0]) == 0:
                    break
        if len(left[0]) == 0:
            break
    return True, "", whole


# ------------------------------------------------------------------------------------------------------------------------------------
# the last-writer map: sorted disjoint byte intervals, each tagged (writer op, allocation id)
# ------------------------------------------------------------------------------------------------------------------------------------
class WriterMap:
    """The map cut at `cuts` (the offsets allocations ever started at) into independent pieces: a write splices only the arrays of the
    pieces it touches, whatever the rest of a multi-GB arena has accumulated."""

    def __init__(self, cuts=()):
        self.cuts = np.unique(np.array([0] + [int(c) for c in cuts], dtype=np.int64))
        self.subs = [_SubMap() for _ in self.cuts]

    def _pieces(self, qs, qe):
        i0 = int(np.searchsorted(self.cuts, qs[0], "right")) - 1
        i1 = int(np.searchsorted(self.cuts, qe[-1], "left"))
        for i in range(max(i0, 0), i1):
            if i0 + 1 == i1:
                yield self.subs[i], qs, qe
                return
            lo = self.cuts[i]
            hi = self.cuts[i + 1] if i + 1 < len(self.cuts) else np.int64(1) << 62
            s, e = np.maximum(qs, lo), np.minimum(qe, hi)
            keep = s < e
            if keep.any():
                yield self.subs[i], s[keep], e[keep]

    def lookup(self, qs, qe):
        cov, unc = [], []
        for sub, s, e in self._pieces(qs, qe):
            c, u = sub.lookup(s, e)
            cov.append(c)
            unc.append(u)
        if len(cov) == 1:
            return cov[0], unc[0]
        us, ue = np.concatenate([u[0] for u in unc]), np.concatenate([u[1] for u in unc])
        return tuple(np.concatenate([c[j] for c in cov]) for j in range(4)), merge_intervals(us, ue)

    def write(self, ws, we, writer, alloc):
        for sub, s, e in self._pieces(ws, we):
            sub.write(s, e, writer, alloc)


class _SubMap:
    def __init__(self):
        z = np.zeros(0, dtype=np.int64)
        self.S, self.E, self.W, self.A = z, z, z.copy(), z.copy()

    def _local(self, lo, hi):
        return int(np.searchsorted(self.E, lo, "right")), int(np.searchsorted(self.S, hi, "left"))

    def lookup(self, qs, qe):
        """-> (lo, hi, writer, alloc) of the covered pieces of the query, and (lo, hi) of the uncovered pieces."""
        i0, i1 = self._local(qs[0], qe[-1])
        S, E = self.S[i0:i1], self.E[i0:i1]
        if len(S) == 1 and S[0] <= qs[0] and E[0] >= qe[-1]:                     # one writer's dense piece under the whole (strided) view
            n = len(qs)
            return (qs, qe, np.full(n, self.W[i0], dtype=np.int64), np.full(n, self.A[i0], dtype=np.int64)), (qs[:0], qe[:0])
        if len(S) == len(qs) and (S == qs).all() and (E == qe).all():          # the same strided view as the map's pieces: no cutting
            return (qs, qe, self.W[i0:i1], self.A[i0:i1]), (qs[:0], qe[:0])
        cuts = np.unique(np.concatenate([S, E, qs, qe]))
        lo, hi = cuts[:-1], cuts[1:]
        iq = np.searchsorted(qs, lo, "right") - 1
        inq = (iq >= 0) & (lo < qe[np.maximum(iq, 0)])
        if len(S):
            im = np.searchsorted(S, lo, "right") - 1
            inm = (im >= 0) & (lo < E[np.maximum(im, 0)])
        else:
            im, inm = np.zeros(len(lo), dtype=np.int64), np.zeros(len(lo), dtype=bool)
        cov, unc = inq & inm, inq & ~inm
        idx = im[cov] + i0
        return (lo[cov], hi[cov], self.W[idx], self.A[idx]), merge_intervals(lo[unc], hi[unc])

    def write(self, ws, we, writer, alloc):
        i0, i1 = self._local(ws[0], we[-1])
        S, E, W, A = self.S[i0:i1], self.E[i0:i1], self.W[i0:i1], self.A[i0:i1]
        if len(S) == len(ws) and len(ws) > 1 and (S == ws).all() and (E == we).all() and (ws[1:] > we[:-1]).all():
            self.W[i0:i1], self.A[i0:i1] = writer, alloc        # the same strided view (rows apart): only the tags change
            return
        if len(S):
            cuts = np.unique(np.concatenate([S, E, ws, we]))
            lo, hi = cuts[:-1], cuts[1:]
            im = np.searchsorted(S, lo, "right") - 1
            inm = (im >= 0) & (lo < E[np.maximum(im, 0)])
            iw = np.searchsorted(ws, lo, "right") - 1
            inw = (iw >= 0) & (lo < we[np.maximum(iw, 0)])
            keep = inm & ~inw
            ks, ke, kw, ka = lo[keep], hi[keep], W[im[keep]], A[im[keep]]
        else:
            ks = ke = kw = ka = np.zeros(0, dtype=np.int64)
        ns = np.concatenate([ks, ws])
        ne = np.concatenate([ke, we])
        nw = np.concatenate([kw, np.full(len(ws), writer, dtype=np.int64)])
        na = np.concatenate([ka, np.full(len(ws), alloc, dtype=np.int64)])
        order = np.argsort(ns, kind="stable")
        ns, ne, nw, na = ns[order], ne[order], nw[order], na[order]
        if len(ns) > 1:                                         # coalesce touching pieces with the same tags
            new = np.ones(len(ns), dtype=bool)
            new[1:] = (ns[1:] != ne[:-1]) | (nw[1:] != nw[:-1]) | (na[1:] != na[:-1])
            idx = np.flatnonzero(new)
            last = np.append(idx[1:] - 1, len(ns) - 1)
            ns, ne, nw, na = ns[idx], ne[last], nw[idx], na[idx]
        self.S = np.concatenate([self.S[:i0], ns, self.S[i1:]])
        self.E = np.concatenate([self.E[:i0], ne, self.E[i1:]])
        self.W = np.concatenate([self.W[:i0], nw, self.W[i1:]])
        self.A = np.concatenate([self.A[:i0], na, self.A[i1:]])


def _coalesce_by_writer(lo, hi, w):
    """Maximal runs, in address order, of covered pieces of ONE access that share a writer: (first byte, end of the last piece, writer).
    Gaps of the access itself (the pitch of a strided view) do not end a run, so the runs do not depend on how the map happened to be
    cut — two passes over the same access compare equal exactly when every byte has the same last writer."""
    if len(lo) <= 1:
        return lo, hi, w
    new = np.ones(len(lo), dtype=bool)
    new[1:] = w[1:] != w[:-1]
    idx = np.flatnonzero(new)
    last = np.append(idx[1:] - 1, len(lo) - 1)
    return lo[idx], hi[last], w[idx]


# ------------------------------------------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------------------------------------------
def analyse(prog, events: List[Alloc], ops=None, ff_min_m: int = FF_MIN_M, shard=None, ff_model=None) -> Report:
    t0 = time.perf_counter()
    ops = list(prog.ops if ops is None else ops)
    n = len(ops)
    rep = Report(ops=n, allocations=len(events), inplace={name: 0 for name, _, _ in INPLACE_CLASSES})
    fps = [footprint(op) for op in ops]
    rep.accesses = sum(len(f) for f in fps)
    for op, f in zip(ops, fps):
        outs = output_slots(op)
        rep.roles |= {(op.kind, x.slot, x.mode, x.slot in outs) for x in f}
    seen = set()

    def hazard(rule, plan, k_ops, slots, rng, detail=""):
        key = (rule, tuple(k_ops), tuple(slots), detail)
        if key in seen:
            return
        seen.add(key)
        rep.hazards.append(Hazard(rule, [(k, ops[k].name) for k in k_ops], list(slots), (int(rng[0]), int(rng[1])), detail, plan))

    a_off = np.array([a.off for a in events], dtype=np.int64)
    a_end = np.array([a.end for a in events], dtype=np.int64)
    a_born = np.array([a.born for a in events], dtype=np.int64)
    a_died = np.array([(1 << 60) if a.died is None else a.died for a in events], dtype=np.int64)

    def live_alloc(k, lo, hi):
        """The allocations that hold [lo, hi) and are live at op k, as a tag (a1 + 1) | (a2 + 1) << 32: a1 born before the op was emitted,
        a2 born between op k and op k + 1 (a peephole's output; the block may be the one a1 was released from at the same op count).
        0 = none."""
        m = (a_off <= lo) & (a_end >= hi) & (a_born <= k + 1) & (a_died >= k + 1)
        ids = np.flatnonzero(m)
        early, late = ids[a_born[ids] <= k], ids[a_born[ids] == k + 1]
        return (int(early[-1]) + 1 if len(early) else 0) | ((int(late[-1]) + 1 if len(late) else 0) << 32)

    # ---- R5 (static part): the regions
    sync, part = prog._sync, getattr(prog, "_gn_part", None)
    if not events or events[0].off != sync.alloc_off or events[0].born != 0:
        hazard("R5", "full", [0] if n else [], [], (sync.alloc_off, sync.alloc_off), "_sync is not the first allocation")
    sync_a = next((a for a in events if a.off == sync.alloc_off and a.born == 0), None)
    part_a = next((a for a in events if part is not None and a.off == part.alloc_off and a.born == 0), None)
    regions = {"tickets": (sync.ref.off, sync.ref.off + 4 * FP.SYNC_INTS),
               "barrier": (sync.ref.off + 4 * FP.SYNC_INTS, sync.ref.off + 4 * (FP.SYNC_INTS + FP.SYNC_BARRIER_INTS)),
               "records": (part_a.off, part_a.end) if part_a is not None else (0, 0)}
    owner = {(FP.GEMM, 7): "tickets", (FP.GEMM, 11): "barrier", (FP.GROUPNORM, 5): "barrier", (FP.GEMM, 10): "records", (FP.GROUPNORM, 7): "records"}
    guarded = [(a.off, a.end) for a in (sync_a, part_a) if a is not None]

    inv = [bool(op.meta.get("step_invariant")) for op in ops]
    A = _Addr()
    static_done = set()
    acc_alloc: Dict[tuple, int] = {}

    def static_rules(plan, launch, accs):
        """R2 (containment), R3, R5 of one launch: accs = [(k, access index, Access)]."""
        for k, ai, x in accs:
            if x.space != "arena":
                continue
            lo, hi = x.bounds()
            if x.sync:
                reg = regions.get(owner.get((ops[k].kind, x.slot)))
                if reg is None or not (reg[0] <= lo and hi <= reg[1]):
                    hazard("R5", plan, [k], [x.slot], (lo, hi), f"{x.what}: outside the region its slot owns")
                continue
            for g0, g1 in guarded:
                if lo < g1 and g0 < hi and overlap(x, [Rect.flat(g0, g1 - g0)]) is not None:
                    hazard("R5", plan, [k], [x.slot], (max(lo, g0), min(hi, g1)), f"{x.what} ({x.mode}) overlaps the synchronisation / exchange region")
            aid = live_alloc(k, lo, hi)
            acc_alloc[(k, ai)] = aid
            if aid == 0:
                hazard("R2", plan, [k], [x.slot], (lo, hi), f"{x.what} ({x.mode}): not inside one allocation that is live at this op")
        arena = [(k, ai, x) for k, ai, x in accs if x.space == "arena" and not x.sync]
        for i, (k, ai, w) in enumerate(arena):
            if w.mode == "r":
                continue
            for j, (k2, aj, y) in enumerate(arena):
                if j == i or (y.mode != "r" and j < i) or (k == k2 and w.launch != y.launch):
                    continue
                rng = overlap(w, y)
                if rng is None:
                    continue
                cls = next((name for name, pred, _ in INPLACE_CLASSES if k == k2 and y.mode == "r" and pred(ops[k], w, y)), None)
                if cls is not None:
                    if (k, ai, aj) not in static_done:
                        static_done.add((k, ai, aj))
                        rep.inplace[cls] += 1
                    continue
                hazard("R3", plan, [k] if k == k2 else [k, k2], [w.slot, y.slot], rng,
                       f"{w.what} ({w.mode}) overlaps {y.what} ({y.mode}) inside one launch")

    # ---- both plans
    wm = WriterMap(a.off for a in events)
    pass1_reads: Dict[tuple, tuple] = {}
    shared_lo, shared_hi = [], []
    for plan in ("full", "skip"):
        idx = [k for k in range(n) if plan == "full" or not inv[k]]
        plan_ops = [ops[k] for k in idx]
        plan_fps = [fps[k] for k in idx]
        if plan == "skip" and len(idx) == n:
            break
        fused = {}
        j = 0
        while j < len(idx):
            ptr = (ff_model(plan_ops, j, A, ff_min_m) if ff_model is not None else ff_pair_library(plan_ops, plan_fps, j, A, ff_min_m))
            ext, why, rng6 = ff_pair_extent(plan_ops, plan_fps, j, A, ff_min_m)
            if ptr != ext:
                hazard("R6", plan, [idx[j], idx[j + 1]], [5], rng6,
                       f"{'pointer' if ff_model is not None else 'library'} model {'fuses' if ptr else 'does not fuse'}, extent model {'fuses' if ext else 'does not: ' + why}")
            if ptr:
                fused[j] = True
                j += 2
            else:
                j += 1
        rep.fused_pairs[plan] = [idx[j] for j in fused]
        carried = []
        j = 0
        while j < len(idx):
            ks = [idx[j], idx[j + 1]] if j in fused else [idx[j]]
            accs = []
            for k in ks:
                for ai, x in enumerate(fps[k]):
                    if len(ks) == 2 and ((k == ks[0] and x.slot == 5 and x.mode == "w") or (k == ks[1] and x.slot == 0)):
                        continue        # THE HIDDEN BUFFER IS NOT WRITTEN BY A FUSED PAIR (include/t2v_hip.h:207), nor read
                    accs.append((k, ai, x))
            key = (tuple(ks))
            if key not in static_done:
                static_done.add(key)
                static_rules(plan, ks, accs)
            # R1 / R2 (writer's life) / R4 on the reads, then the writes enter the map
            for k, ai, x in accs:
                if x.space != "arena" or x.sync or x.mode != "r":
                    continue            # (ext and weight reads: always allowed, also for an invariant op)
                qs, qe = x.intervals()
                (lo, hi, w, al), (us, ue) = wm.lookup(qs, qe)
                aid = acc_alloc.get((k, ai), 0)
                mine = [v for v in (aid & 0xFFFFFFFF, aid >> 32) if v]
                w1, w2 = al & 0xFFFFFFFF, al >> 32
                ok = np.zeros(len(al), dtype=bool)
                for v in mine:
                    ok |= (w1 == v) | (w2 == v)
                if shard is not None and ops[k].kind == FP.ALLGATHER and shard.frames < shard.max_frames and aid and len(x.rects) == 1:
                    nb = x.rects[0].row                                  # this rank's part: the padding behind its `frames` real frames
                    if nb % shard.max_frames == 0:
                        p0, p1 = x.rects[0].off + nb // shard.max_frames * shard.frames, x.rects[0].off + nb
                        tail = lo >= p0
                        if not ok[tail].any():                           # nothing of the tail was written in this life: it IS padding
                            keep = ~tail
                            lo, hi, w, al, ok, w1, w2 = lo[keep], hi[keep], w[keep], al[keep], ok[keep], w1[keep], w2[keep]
                            us, ue = subtract((us, ue), (np.array([p0], dtype=np.int64), np.array([p1], dtype=np.int64)))
                            rep.padding_exempt += plan == "full"
                if len(us):
                    hazard("R1", plan, [k], [x.slot], (us[0], ue[0]), f"{x.what}: {int((ue - us).sum())} bytes read that no earlier op of the pass wrote")
                if aid and len(al):
                    bad = np.flatnonzero(~ok)
                    if len(bad):
                        b0 = bad[0]
                        hazard("R2", plan, [k, int(w[b0])], [x.slot], (lo[b0], hi[b0]),
                               f"{x.what}: last writer wrote during the life of allocation {[int(w1[b0]) - 1, int(w2[b0]) - 1]}, the reader's is {[v - 1 for v in mine]}")
                cl, ch, cw = _coalesce_by_writer(lo, hi, w)
                if plan == "full":
                    pass1_reads[(k, ai)] = (cl, ch, cw)
                    if len(cw):
                        winv = np.array(inv, dtype=bool)[cw]
                        if inv[k] and not winv.all():
                            b0 = np.flatnonzero(~winv)[0]
                            hazard("R4", plan, [k, int(cw[b0])], [x.slot], (cl[b0], ch[b0]), f"{x.what}: an invariant op reads bytes a non-invariant op wrote")
                        if not inv[k] and winv.any():
                            exact = np.array(inv, dtype=bool)[w]
                            shared_lo.append(lo[exact])
                            shared_hi.append(hi[exact])
                            a1 = (aid & 0xFFFFFFFF) - 1
                            if a1 >= 0 and events[a1].died is not None and events[a1].died < n:      # (a release behind the last op is bookkeeping only)
                                hazard("R4", plan, [k, int(cw[winv][0])], [x.slot], (cl[winv][0], ch[winv][0]),
                                       f"{x.what}: invariant-written bytes in allocation {a1}, which is released at op count {events[a1].died}")
                else:
                    pl, ph, pw = pass1_reads.get((k, ai), (cl[:0], ch[:0], cw[:0]))
                    if not (len(pl) == len(cl) and (pl == cl).all() and (ph == ch).all() and (pw == cw).all()):
                        d = 0
                        m = min(len(pl), len(cl))
                        neq = np.flatnonzero((pl[:m] != cl[:m]) | (ph[:m] != ch[:m]) | (pw[:m] != cw[:m]))
                        d = int(neq[0]) if len(neq) else m
                        now = int(cw[d]) if d < len(cw) else -1
                        was = int(pw[d]) if d < len(pw) else -1
                        rng = (cl[d], ch[d]) if d < len(cl) else (pl[d], ph[d])
                        hazard("R4", plan, [k] + [q for q in (now, was) if q >= 0], [x.slot], rng,
                               f"{x.what}: last writer in pass 2 is op {now}, in pass 1 it was op {was}")
                    if len(cw):
                        winv = np.array(inv, dtype=bool)[cw]
                        if winv.any():
                            exact = np.array(inv, dtype=bool)[w]
                            carried.append((lo[exact], hi[exact]))
            for k, ai, x in accs:
                if x.space == "arena" and not x.sync and x.mode in ("w", "scratch"):
                    ws, we = x.intervals()
                    wm.write(ws, we, k, acc_alloc.get((k, ai), 0))
            j += len(ks)
        if plan == "skip":
            rep.carried = merge_intervals(np.concatenate([c[0] for c in carried]), np.concatenate([c[1] for c in carried])) if carried else \
                (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    # R4, last clause: invariant-written bytes that a non-invariant op reads are never written by a non-invariant op
    if shared_lo:
        sh = merge_intervals(np.concatenate(shared_lo), np.concatenate(shared_hi))
        for k in range(n):
            if inv[k]:
                continue
            for x in fps[k]:
                if x.space == "arena" and not x.sync and x.mode in ("w", "scratch"):
                    lo, hi = x.bounds()
                    if lo >= sh[1][-1] or hi <= sh[0][0]:
                        continue
                    s, e = intersect(x.intervals(), sh)
                    if len(s):
                        hazard("R4", "skip", [k], [x.slot], (s[0], e[0]), f"{x.what} ({x.mode}): a non-invariant op writes bytes that hold step-invariant data")
    rep.seconds = time.perf_counter() - t0
    return rep


def check(prog, events, ops=None, ff_min_m: int = FF_MIN_M, **kw) -> List[Hazard]:
    return analyse(prog, events, ops=ops, ff_min_m=ff_min_m, **kw).hazards


# ------------------------------------------------------------------------------------------------------------------------------------
# the footprint table against an execution: the confinement protocol of one op (CPU interpreter or GPU, the same code)
# ------------------------------------------------------------------------------------------------------------------------------------
def _views(t, r: Rect):
    """The bytes of a rectangle as tensor views of the arena `t`: one strided view, or (a rectangle that visits a byte twice: pitch 0
    of a repeated row, overlapping rows) one slice per merged interval."""
    import torch
    s, e = r.intervals()
    if int((e - s).sum()) == r.nbytes_upper:
        return [torch.as_strided(t, tuple(r.counts) + (r.row,), tuple(r.pitches) + (1,), r.off)]
    return [t[a:b] for a, b in zip(s.tolist(), e.tolist())]


def guarded_prefix(prog) -> int:
    """End of the synchronisation words and the exchange-record region: they are the program's first allocations (R5), so a prefix."""
    end = prog._sync.alloc_off + prog.arena.ALIGN * -(-(prog._sync.rows * prog._sync.ld * 4) // prog.arena.ALIGN)
    part = getattr(prog, "_gn_part", None)
    if part is not None:
        assert part.alloc_off == end, "the exchange-record region does not follow the synchronisation words"
        end = part.alloc_off + part.rows
    return end


class Confinement:
    """Protocol for op k from the state S_k of a clean chain (arena `A`, which this object advances op by op):
      run A: the op's pure outputs pre-filled 0x00;
      run B: arena `B`, where every byte outside the op's declared read rectangles is 0xFF (its pure outputs included);
      in both, the synchronisation words and the exchange-record region are what the clean chain left.
    Asserted: A and B bit-equal on every written rectangle (an under-declared read shows as NaN in B's output, an over-declared write
    as 0x00 against 0xFF); outside written and scratch rectangles B equals its pre-state (a stray store shows as a changed fence byte).
    `run(k, arena, ext)` executes op k alone on `arena` with the ext tensors `ext`."""

    def __init__(self, prog, arena, run):
        import torch
        self.prog, self.A, self.run = prog, arena, run
        self.B = torch.full_like(arena, 0xFF)
        self.guard = guarded_prefix(prog)
        self.errors: List[str] = []
        self.checked = 0

    def step(self, k, op, ext) -> List[str]:
        import torch
        A, B, errs = self.A, self.B, []
        fp = footprint(op)
        arena = [x for x in fp if x.space == "arena" and not x.sync]
        reads = [x for x in arena if x.mode == "r"]
        writes = [x for x in arena if x.mode == "w"]
        scratch = [x for x in arena if x.mode == "scratch"]
        for x in reads:
            for r in x.rects:
                for vb, va in zip(_views(B, r), _views(A, r)):
                    vb.copy_(va)
        pure = [x for x in reads if all(overlap(x, y) is None for y in writes + scratch)]
        snaps = [(x, r, [v.clone() for v in _views(A, r)]) for x in pure for r in x.rects]
        for x in writes:
            if all(overlap(x, y) is None for y in reads):
                for r in x.rects:
                    for v in _views(A, r):
                        v.zero_()
            else:                                              # in place: only the bytes that are not also read
                s, e = subtract(x.intervals(), union([r for y in reads for r in y.rects]))
                for a, b in zip(s.tolist(), e.tolist()):
                    A[a:b] = 0
        if self.guard:
            B[: self.guard].copy_(A[: self.guard])
        wext = {int(x.name) for x in fp if x.space == "ext" and x.mode != "r"}
        ext_b = {s: (t.clone() if s in wext else t) for s, t in ext.items()}
        self.run(k, A, ext)
        self.run(k, B, ext_b)
        tag = f"op {k} {op.name} (kind {op.kind})"
        for x in writes:
            for r in x.rects:
                n = sum(int((va != vb).sum()) for va, vb in zip(_views(A, r), _views(B, r)) if not torch.equal(va, vb))
                if n:
                    errs.append(f"{tag}: slot {x.slot} {x.what}: {n} bytes differ between the zero-filled and the poisoned run")
        for s in wext:
            if not torch.equal(ext[s].view(torch.uint8) if ext[s].dtype != torch.uint8 else ext[s],
                               ext_b[s].view(torch.uint8) if ext_b[s].dtype != torch.uint8 else ext_b[s]):
                errs.append(f"{tag}: ext slot {s} differs between the zero-filled and the poisoned run")
        for x, r, snap in snaps:
            if not all(torch.equal(v, c) for v, c in zip(_views(B, r), snap)):
                errs.append(f"{tag}: slot {x.slot} {x.what}: read-only bytes changed")
        for x in arena:
            for r in x.rects:
                for v in _views(B, r):
                    v.fill_(0xFF)
        if int(B[self.guard:].min()) != 0xFF:
            bad = torch.nonzero(B[self.guard:] != 0xFF).flatten()
            errs.append(f"{tag}: {len(bad)} bytes changed outside every declared rectangle, first at arena offset {int(bad[0]) + self.guard}")
            B[self.guard:].fill_(0xFF)
        self.checked += 1
        self.errors += errs
        return errs


def ext_tensors(prog, device="cpu", seed=5):
    """One tensor per ext slot the program names, sized and typed from the footprints (random contents; int32 ids small and valid)."""
    import torch
    need: Dict[int, tuple] = {}
    for op in prog.ops:
        for x in footprint(op):
            if x.space == "ext":
                hi = max(r.hi for r in x.rects)
                old = need.get(int(x.name), (0, x.dtype))
                assert x.dtype and (old[0] == 0 or old[1] == x.dtype), (op.name, x.slot, x.dtype, old)
                need[int(x.name)] = (max(old[0], hi), x.dtype)
    g = torch.Generator().manual_seed(seed)
    out = {}
    for slot, (nbytes, dt) in sorted(need.items()):
        if dt == "i32":
            t = torch.randint(1, 200, (nbytes // 4,), generator=g, dtype=torch.int32)
        elif dt == "u8":
            t = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)
        else:
            t = torch.randn(nbytes // (4 if dt == "f32" else 2), generator=g).to(torch.float32 if dt == "f32" else torch.float16)
        out[slot] = t.abs() * 400 + 1 if slot == 2 and dt == "f32" and nbytes <= 64 else t      # (EXT_T: timesteps)
        out[slot] = out[slot].to(device)
    return out
