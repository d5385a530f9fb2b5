"""TEST INFRASTRUCTURE — the corpus of GEMM and ATTENTION records, and of whole plans, whose verdicts tests/golden/record_verdicts.npz pins.
No test functions here: tests/golden/make_golden_record_verdicts.py asks a library built from the PARENT commit for the verdicts and writes
the golden; tests/test_record_verdicts_cpu.py replays the golden against the library of this checkout.  Nothing needs a GPU: t2v_plan_create
validates records and pairs the feed-forward GEMMs on whatever addresses it is given.

A verdict is what a caller sees: the status of t2v_plan_create for the record as a one-record plan and the exact t2v_last_error() text; for a
whole plan, t2v_plan_num_launches (ops minus fused feed-forward pairs: the only CPU-visible witness of the pairing and of the slot extents
it scans).  This file knows the record as a caller does — 32 ints, 8 floats, 12 pointer slots — and nothing of how the library reads it.

The corpus, in this order, deduplicated by (kind, ints, floats, which pointers are set):
  1. every GEMM / ATTENTION record of every program the CPU suite lowers (tools/program_digest.py rows + test_plan_hazards_cpu.extra_rows
     under program_digest.FIXED);
  2. every such record of the adversarial case lists: gemm_inputs, fused_attention_inputs, ff_fused_inputs (every variant of its builder),
     the attention cases of adversarial.py, and the table / plain / two-role records of the prompt_batch_inputs length lists;
  3. single-field mutations of the first record of every record_paths.path_key class of 1. and 2.: every int word set to 0, 1, -1, value + 1,
     value + 4; every pointer slot toggled; f[0], f[1], f[2] set to 0 — thinned to every MUTATION_STRIDE-th mutation per class, staggered
     from class to class so that every word meets every value in some class;
  4. the hand-written records of HAND: refusals that no single-field mutation of an emitted record reaches.
A pointer that is set is the address SLOT_BASE + slot * SLOT_STEP (16-byte aligned, far above T2V_EXT_SLOTS): for these two kinds validation
asks only whether a pointer is there."""
from __future__ import annotations

import collections
import ctypes
import os
import struct

import numpy as np

import record_paths as RP
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import program as PG

KINDS = (L.OP_GEMM, L.OP_ATTENTION)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_verdicts.npz")
SLOT_BASE, SLOT_STEP = 0x100000000000, 1 << 36
MUTATION_STRIDE = 3
ARENA, WEIGHTS = 0x100000000000, 0x700000000000          # the addresses test_plan_hazards_cpu._launches binds plans to

Rec = collections.namedtuple("Rec", "kind ints floats mask")          # ints: 32 int32, floats: 8 float32 (as their bits), mask: bit k = p[k] set


def _i32(v):
    v = int(v) & 0xffffffff
    return v - (1 << 32) if v >= (1 << 31) else v


def _f32bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def rec_of(op) -> Rec:
    """A program.Op as the bytes BoundProgram hands the library (pointers: only whether they are set)."""
    return Rec(op.kind, tuple(_i32(v) for v in op.i), tuple(_f32bits(v) for v in op.f), sum(1 << k for k, r in enumerate(op.p) if r.space != "null"))


def struct_of(rec: Rec):
    r = L.T2VOp()
    r.kind, r.tag = rec.kind, 0
    for k, v in enumerate(rec.ints):
        r.i[k] = v
    for k, v in enumerate(rec.floats):
        r.f[k] = struct.unpack("<f", struct.pack("<I", v))[0]
    for k in range(L.OP_NP):
        r.p[k] = SLOT_BASE + k * SLOT_STEP if (rec.mask >> k) & 1 else 0
    return r


def verdict(lib, rec: Rec):
    """(status of t2v_plan_create, the error text or '') of the record as a one-record plan."""
    arr = (L.T2VOp * 1)(struct_of(rec))
    handle = ctypes.c_void_p()
    rc = lib.t2v_plan_create(arr, 1, ctypes.byref(handle))
    if rc == 0:
        lib.t2v_plan_destroy(handle)
        return 0, ""
    return rc, lib.t2v_last_error().decode()


def launches(lib, prog, ops=None):
    """t2v_plan_num_launches of the plan the library makes of these records on made-up addresses; -1: the plan is refused."""
    names = sorted({p.name for op in prog.ops for p in op.p if p.space == "weight"})
    fake = {n: WEIGHTS + (k << 36) for k, n in enumerate(names)}
    try:
        bound = PG.BoundProgram(prog, ARENA, fake, ops=ops, reset_sync=False)
    except L.T2VError:
        return -1
    return lib.t2v_plan_num_launches(bound.handle)


# ---- 1. / 2. the emitted records and the plans ---------------------------------------------------------------------------------------------
def lowered_programs():
    """(label, program) of every row the CPU suite lowers; the caller provides the FIXED environment (test_plan_hazards_cpu._fixed_environment)."""
    from test_plan_hazards_cpu import ROOT, _lower, extra_rows
    from tools import program_digest as PD
    for source in (PD.rows(ROOT), extra_rows()):
        for r in source:
            yield r.label, _lower(r).prog


def with_and_without_invariants(label, prog):
    """The two plans a program runs as: all of it, and (where it has any) without its step-invariant ops."""
    keep = [op for op in prog.ops if not op.meta.get("step_invariant")]
    return [(label, prog, None)] + ([(label + " | without the step-invariant ops", prog, keep)] if keep and len(keep) != len(prog.ops) else [])


FF_VARIANTS = (dict(), dict(waive_cutoff=False), dict(split_k=True), dict(out_over_x=True))
FF_KINDS = ("adjacent", "separated", "third-reader")


def ff_plans():
    """(label, program, ops) of every plan the builder of tests/ff_fused_inputs.py makes: every case, variant and record selection."""
    import ff_fused_inputs as FF
    for c in FF.CASES:
        for kw in FF_VARIANTS:
            if (kw.get("out_over_x") and not c["out_lo"]) or (kw.get("split_k") and c["wrap"]):
                continue          # (the builder has no such program: X doubles as the hi + lo output; a wrapped residual takes no split-K)
            b = FF.build(c, **kw)
            for kind in FF_KINDS:
                yield f"ff:{c['id']}:{','.join(sorted(kw)) or 'default'}:{kind}", b.P, b.ops(kind)


def prompt_batch_ops():
    """The ATTENTION records of tests/test_gpu_prompt_batch.py for every length list of prompt_batch_inputs: one table over all samples, each
    sample as a plain launch, the uniform and the two-role layouts as a table and as the record they equal."""
    import prompt_batch_inputs as PB
    from sd_webui_text2video_amd.program import Program, Ref
    for lens in PB.LENGTH_LISTS:
        heads, nq, F, D = PB.HEADS, PB.NQ, PB.FRAMES, PB.HEAD_DIM
        inner, ld = heads * D, 2 * heads * D
        ls, starts = PB.flat(lens)
        B, total, per = len(ls), sum(ls), F * nq
        P = Program("attention table")
        q, kv, o = P.alloc(B * per, inner, "f16"), P.alloc(total, ld, "f16"), P.alloc(B * per, inner, "f16")
        k1, v1 = kv.col_slice(0, inner), kv.col_slice(inner, ld)
        common = dict(nq=nq, heads=heads, b_inner=F, q_strides=(inner, per * inner, nq * inner), o_strides=(inner, per * inner, nq * inner), scale=D ** -0.5)
        tab = lambda lens_, starts_: (Ref("weight", 0, "table"), list(lens_), list(starts_))
        P.attention("table", q.ref, k1.ref, v1.ref, o.ref, nk=max(ls), b_outer=B, kv_strides=(ld, 0, 0), table=tab(ls, starts), **common)
        for s, n in enumerate(ls):
            P.attention(f"single.{s}", q.ref, k1.ref, v1.ref, o.ref, nk=n, b_outer=1, kv_strides=(ld, 0, 0), **common)
        L0 = ls[0]
        Vu = min(B, total // L0)
        P.attention("uniform.table", q.ref, k1.ref, v1.ref, o.ref, nk=L0, b_outer=Vu, kv_strides=(ld, 0, 0), table=tab([L0] * Vu, [s * L0 for s in range(Vu)]), **common)
        P.attention("uniform.plain", q.ref, k1.ref, v1.ref, o.ref, nk=L0, b_outer=Vu, kv_strides=(ld, L0 * ld, 0), **common)
        Lu = next((n for n in ls if n != L0), None)
        if Lu is not None and B >= 2:
            Vp = min(B // 2, total // (L0 + Lu))
            P.attention("pair.table", q.ref, k1.ref, v1.ref, o.ref, nk=max(L0, Lu), b_outer=2 * Vp, kv_strides=(ld, 0, 0),
                        table=tab([L0] * Vp + [Lu] * Vp, [s * L0 for s in range(Vp)] + [Vp * L0 + s * Lu for s in range(Vp)]), **common)
            P.attention("pair.roles", q.ref, k1.ref, v1.ref, o.ref, nk=L0, b_outer=2 * Vp, kv_strides=(ld, L0 * ld, 0), alt=(Vp, Lu, k1.ref, v1.ref, Lu * ld), **common)
        yield from P.ops


def adversarial_ops():
    import adversarial as A
    import attention_records as AR
    import fused_attention_inputs as FA
    import gemm_inputs as G
    for mod in (G, FA):
        for c in mod.CASES:
            yield from mod.build(c).P.ops
    for _, prog, _ in ff_plans():
        yield from prog.ops
    for c in A.ATTN_CASES:
        for attn2 in ((True, False) if c["attn2"] else (False,)):
            yield from AR.build_attn(c, attn2).P.ops
    yield from prompt_batch_ops()


# ---- 3. mutations ----------------------------------------------------------------------------------------------------------------------------
def mutations(rec: Rec, phase: int):
    """The single-field edits of a record, every MUTATION_STRIDE-th of them starting at `phase`."""
    out = []
    for k, v in enumerate(rec.ints):
        for w in (0, 1, -1, _i32(v + 1), _i32(v + 4)):
            out.append(rec._replace(ints=rec.ints[:k] + (w,) + rec.ints[k + 1:]))
    for k in range(L.OP_NP):
        out.append(rec._replace(mask=rec.mask ^ (1 << k)))
    for k in range(3):
        out.append(rec._replace(floats=rec.floats[:k] + (0,) + rec.floats[k + 1:]))
    return out[phase % MUTATION_STRIDE::MUTATION_STRIDE]


# ---- 4. hand-written records -----------------------------------------------------------------------------------------------------------------
def _rec(kind, ints, ptrs, floats=()):
    i, f = [0] * L.OP_NI, [0] * L.OP_NF
    for k, v in ints.items():
        i[k] = v
    for k, v in enumerate(floats):
        f[k] = _f32bits(v)
    return Rec(kind, tuple(i), tuple(f), sum(1 << k for k in ptrs))


def hand_written():
    """Refusals that need two words off the emitted path at once; each names the message it is there for."""
    g = lambda ints, ptrs=(0, 1, 5), floats=(): _rec(L.OP_GEMM, {0: 256, 1: 320, 2: 320, 3: 320, 4: 320, 5: 320, 22: 8, **ints}, ptrs, floats)
    a = lambda ints, ptrs=(0, 1, 2, 3): _rec(L.OP_ATTENTION, {0: 64, 1: 64, 2: 2, 3: 2, 4: 1, 5: 128, 6: 8192, 8: 256, 11: 128, 12: 8192, 14: 64, **ints}, ptrs, (0.125,))
    return [
        g({7: 5}),                                                               # unknown gather mode
        g({7: L.GATHER_CONV3X3, 2: 576, 10: 64, 11: 1, 12: 2, 13: 16, 14: 16}),  # upsample must be 0 or 1
        g({7: L.GATHER_CONV3X3_C8, 2: 72, 3: 8, 10: 8, 11: 3, 13: 16, 14: 16, 22: 0}),          # stride must be 1 or 2 (the C8 stem)
        g({7: L.GATHER_CONV3X3_C8, 2: 72, 3: 16, 10: 8, 22: 0}),                # C8 conv needs Cin == lda == 8, K == 72
        g({7: L.GATHER_TCONV3, 2: 192, 8: 3, 9: 100, 10: 64}),                  # M not a multiple of F*HW
        g({16: L.EPI_GN, 19: 2, 24: 256, 25: 320, 28: 64}, (0, 1, 5, 6, 8, 9, 10, 11)),          # fused GroupNorm on a split-K GEMM: groups <= 32
        g({16: L.EPI_GN, 24: 256, 25: 320, 28: 32, 22: 9}, (0, 1, 5, 8, 9, 10, 11)),             # fused GroupNorm: tile must be 8, 11, 3, 5 or 0
        g({16: L.EPI_GN, 24: 256, 25: 320, 28: 32, 22: 0}, (0, 1, 5, 8, 9, 10, 11)),             # ... on the 128x128-class kernel: N % 128 == 0
        g({16: L.EPI_GN, 1: 1024, 5: 1024, 24: 256, 25: 1024, 28: 2, 22: 5}, (0, 1, 5, 8, 9, 10, 11)),      # ... a group no wider than the tile
        g({16: L.EPI_GN, 24: 256, 25: 320, 28: 32, 29: 0}, (0, 1, 8, 9, 10, 11)),                # ... `out` is null but i[29] asks for it
        g({16: L.EPI_GN, 24: 256, 25: 320, 28: 32, 6: 8}, (0, 1, 4, 5, 8, 9, 10, 11)),           # ... ldc / ldr
        g({16: L.EPI_XATTN, 17: L.F16, 15: 64, 24: 320, 25: 7, 26: 32, 12: 4}, (0, 1, 5, 8, 9), (0, 0.125)),      # fused cross-attention: no residual wrap
        g({16: L.EPI_XATTN, 17: L.F16, 15: 64, 24: 320, 25: 7, 26: 32, 5: 316}, (0, 1, 5, 8, 9), (0, 0.125)),     # fused cross-attention: ldc
        g({16: L.EPI_TATTN, 17: L.F16, 22: 10, 0: 192, 1: 192, 5: 60, 8: 16, 9: 12, 10: 12}, (0, 1, 5), (0, 0.125)),      # fused temporal attention: ldc < heads * 64
        g({16: L.EPI_TATTN, 17: L.F16, 22: 10, 0: 192, 1: 192, 5: 64, 8: 2, 9: 12, 10: 12, 15: 0}, (0, 1, 3, 5), (0, 0.125)),      # F = 2 reads as a LayerNorm mode: the row-bias check waves it through, TATTN refuses the pointer
        g({16: L.EPI_TATTN, 17: L.F16, 22: 10, 0: 192, 1: 192, 5: 64, 8: 16, 9: 24, 10: 12}, (0, 1, 5), (0, 0.125)),      # fused temporal attention: M must be samples * ceil(HW / pixels per tile) * 192
        g({30: 128, 16: L.EPI_GEGLU, 17: L.F16}, (0, 1, 4, 5)),                  # residual row wrap i[30]: plain / statistics / GroupNorm epilogues only
        g({8: 2, 17: L.F32, 9: 320, 22: 9, 6: 8}, (0, 1, 3, 4, 5, 7, 10, 11)),   # cross-tile LayerNorm output: ldc / ldr
        g({8: 1, 17: L.F32, 9: 320, 6: 8}, (0, 1, 3, 4, 5, 7)),                  # fused LayerNorm output: ldc / ldr
        a({19: 1, 20: 64, 21: 0, 17: 64}, (0, 1, 2, 3, 4, 5, 6)),                # attention second role: not for ... the V^T scratch path
        a({22: 3, 23: 64, 24: 128}, (0, 1, 2, 3, 7)),                            # attention per-sample table: i[22] rows == batch_outer
        a({22: 2, 23: 64, 24: 128, 15: 1}, (0, 1, 2, 3, 7)),                     # attention per-sample table: not for causal launches
        a({22: 2, 23: 64, 24: 128, 17: 64}, (0, 1, 2, 3, 6, 7)),                 # attention per-sample table: not for the V^T scratch path
        a({22: 2, 23: 64, 24: 128, 20: 5}, (0, 1, 2, 3, 7)),                     # attention per-sample table: not together with the second role
    ]


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------
def corpus():
    """(records, plans): the deduplicated records in corpus order and [(label, program, ops or None)] of every plan.  The caller provides the
    FIXED environment."""
    recs, plans, reps = collections.OrderedDict(), [], collections.OrderedDict()

    def add_ops(ops):
        for op in ops:
            if op.kind in KINDS:
                recs.setdefault(rec_of(op), None)
                reps.setdefault(RP.path_key(op), op)

    for label, prog in lowered_programs():
        plans += with_and_without_invariants(label, prog)
        add_ops(prog.ops)
    plans += list(ff_plans())
    add_ops(adversarial_ops())
    for c, op in enumerate(reps.values()):
        for m in mutations(rec_of(op), c):
            recs.setdefault(m, None)
    for r in hand_written():
        recs.setdefault(r, None)
    return list(recs), plans


def arrays_of(records):
    return dict(kind=np.array([r.kind for r in records], np.int8), ints=np.array([r.ints for r in records], np.int32),
                floats=np.array([r.floats for r in records], np.uint32).view(np.float32), pmask=np.array([r.mask for r in records], np.uint16))


def records_of(z):
    """The records of a loaded golden."""
    fl = np.ascontiguousarray(z["floats"]).view(np.uint32)
    return [Rec(int(k), tuple(int(v) for v in i), tuple(int(v) for v in f), int(m)) for k, i, f, m in zip(z["kind"], z["ints"], fl, z["pmask"])]
