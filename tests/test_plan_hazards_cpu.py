"""CPU: arena hazards of every lowered program, per op and per byte (tests/plan_footprint.py, tests/plan_hazards.py).

(1) the rectangle arithmetic against brute-force byte sets and the footprint table's roles against csrc/executor.hip output_slots;
(2) the matrix: every row of tools/program_digest.py plus the text tower, the adapter program, the ragged-context ModelScope rows and
    the DDIM step programs — rules R1 to R6 on both plans of every row: zero hazards;
(3) proof that the rules bite: hand-built programs / edited records, each flagged under the named rule at the named op, beside an
    unedited twin that is clean;
(4) the footprint table against the interpreter: the confinement protocol (plan_hazards.Confinement) on every tiny row without
    collectives.
Figures (ops, accesses, allocations, in-place overlaps, seconds): profiles/plan_hazards.txt."""
import os
import re
import time

import numpy as np
import pytest
import torch

import adapter_ref as AR
import plan_footprint as FP
import plan_hazards as H
from interp_adapter import AdapterInterp
from interp_prompt import PromptInterp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import program as PG
from sd_webui_text2video_amd.program import Buf, Program, Ref
from test_resample_cpu import ResampleInterp
from tools import program_digest as PD

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


class AllInterp(AdapterInterp, PromptInterp, ResampleInterp):
    """Every record the interpreters know, in one class."""


def _fixed_environment(mp):
    for k in [k for k in os.environ if k.startswith("T2V_") and k not in PD.FIXED]:
        mp.delenv(k)
    for k, v in PD.FIXED.items():
        mp.setenv(k, v)
    mp.setattr(Program, "_DEVICE_CUS", None)          # (cached from T2V_DEVICE_CUS at first use)


def extra_rows():
    """The rows the digest tool lacks."""
    from oracle import configs, synth
    from sd_webui_text2video_amd import text_encoder as TE, unet as U, videocrafter as VC
    from test_text_encoder_cpu import TINY, _seed_params
    model = _seed_params(TE.OpenClipTextModel(**TINY), 4)
    tower = TE.ClipTextTower(model, heads=2, act="gelu", skip_last=1)
    yield PD.row("text tower b=2 l=77", model, lambda: tower._compile(2, 77))
    yield PD.row("text tower b=2 l=77 emphasis", model, lambda: tower._compile(2, 77, emphasis=True))
    for name in AR.OPTION_SETS:
        ad = VC.Adapter(**AR.SMALL, **AR.OPTION_SETS[name])
        yield PD.row(f"adapter small {name} n=5 64x48 normalise", ad, lambda ad=ad: ad._compile(5, 64, 48, "f32", True))
    ad = VC.Adapter(**AR.SMALL, **AR.OPTION_SETS["t2i"])
    yield PD.row("adapter small front_only fp16", ad, lambda: ad._compile(5, 64, 48, "f16", False, front_only=True))
    ms = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(ms, seed=0)
    for lens, V, share in (((154, 77), 1, True), ((154, 77), 1, False), ((24, 40), 1, False), ((24, 40), 2, False)):
        yield PD.row(f"tiny modelscope ragged {lens} V={V} share={int(share)}", ms,
                     lambda lens=lens, V=V: ms._compile(2 * V, 2, 8, 8, lens, "f32", "f32", "f32", x_batch=V), dict(_share_now=share))

    class _Step:
        packer = None

        def __init__(self, masked):
            self.prog = Program("ddim_step")
            op = self.prog.ddim_step("ddim.step", C=4, inner=3 * 64, guided=4, eps_dtype="f32", x_dtype="f32", mode=1 if masked else 0, samples=2)
            if masked:      # the record samplers.masked_ddim_step hands to t2v_run_ops: blend flag, known x0 / mask / q-noise
                op.i[7] = 1
                op.p[4], op.p[5], op.p[6] = Ref("ext", 9), Ref("ext", 10), Ref("ext", 11)

    yield PD.row("ddim_step program", None, lambda: _Step(False), weights=False)
    yield PD.row("masked ddim_step record", None, lambda: _Step(True), weights=False)


def _launches(lib, prog, ops=None):
    """Launches of the plan the built library makes of these records, on made-up addresses (plan creation needs no GPU)."""
    names = sorted({p.name for op in prog.ops for p in op.p if p.space == "weight"})
    fake = {n: 0x700000000000 + (k << 36) for k, n in enumerate(names)}
    bound = PG.BoundProgram(prog, 0x100000000000, fake, ops=ops, reset_sync=False)
    return lib.t2v_plan_num_launches(bound.handle)


def _lower(r):
    if r.net is None:
        return r.thunk()
    with PD.applied(r):
        return r.thunk()


def _confine(comp, r):
    """The interpreter protocol on one lowered program: (errors, ops checked)."""
    prog = comp.prog
    weights = comp.packer.materialise(r.net.state_dict(), "cpu") if comp.packer is not None else {}
    it = AllInterp(prog, weights)
    ext = H.ext_tensors(prog)

    def run(k, arena, e):
        it.arena = arena
        it.run(e, ops=[prog.ops[k]])

    conf = H.Confinement(prog, it.arena, run)
    for k, op in enumerate(prog.ops):
        conf.step(k, op, ext)
    it.arena = conf.A
    return conf.errors, conf.checked


@pytest.fixture(scope="module")
def matrix(built_lib):
    mp = pytest.MonkeyPatch()
    out, t_all = {}, time.perf_counter()
    try:
        _fixed_environment(mp)
        rec = H.Recorder().install(mp)
        for source in (PD.rows(ROOT), extra_rows()):
            for r in source:
                t0 = time.perf_counter()
                comp = _lower(r)
                t1 = time.perf_counter()
                rep = H.analyse(comp.prog, rec.events(comp.prog), shard=r.shard)
                # the library's own decisions: launches of the full plan and of the plan without the step-invariant ops
                keep = [op for op in comp.prog.ops if not op.meta.get("step_invariant")]
                lib_fused = (len(comp.prog.ops) - _launches(built_lib, comp.prog), len(keep) - _launches(built_lib, comp.prog, keep) if keep else 0)
                tiny = r.weights or r.net is None
                collective = any(op.kind in PG.COLLECTIVE_KINDS for op in comp.prog.ops)
                errs, checked, t2 = None, 0, time.perf_counter()
                if tiny and not collective:
                    errs, checked = _confine(comp, r)
                out[r.label] = dict(report=rep, lower_s=t1 - t0, confine=errs, checked=checked, confine_s=time.perf_counter() - t2,
                                    arena=comp.prog.arena.high, lib_fused=lib_fused, shard=r.shard, allgathers=sum(op.kind == L.OP_ALLGATHER for op in comp.prog.ops))
    finally:
        mp.undo()
    out["_seconds"] = time.perf_counter() - t_all
    return out


# ---- 1. the arithmetic and the roles -------------------------------------------------------------------------------------------------
def _bytes(rect):
    s = set()

    def walk(d, off):
        if d == len(rect.counts):
            s.update(range(off, off + rect.row))
            return
        for i in range(rect.counts[d]):
            walk(d + 1, off + i * rect.pitches[d])
    walk(0, rect.off)
    return s


def test_rectangles_are_compared_exactly():
    g = np.random.default_rng(7)
    for _ in range(300):
        def rnd():
            nd = int(g.integers(0, 3))
            return FP.Rect.make(int(g.integers(0, 40)), [int(g.integers(1, 5)) for _ in range(nd)], [int(g.integers(0, 30)) for _ in range(nd)],
                                int(g.integers(1, 12)))
        a, b = rnd(), rnd()
        A, B = _bytes(a), _bytes(b)
        sa, ea = a.intervals()
        assert set(x for s, e in zip(sa, ea) for x in range(s, e)) == A and (sa[1:] > ea[:-1]).all()
        assert (a.lo, a.hi) == (min(A), max(A) + 1)
        si, ei = FP.intersect(a.intervals(), b.intervals())
        assert set(x for s, e in zip(si, ei) for x in range(s, e)) == A & B
        sd, ed = FP.subtract(a.intervals(), b.intervals())
        assert set(x for s, e in zip(sd, ed) for x in range(s, e)) == A - B
        ov = FP.overlap([a], [b])
        assert (ov is None) == (not (A & B)) and (ov is None or ov[0] == min(A & B))
    # interleaved column halves of one buffer: bounding intervals overlap, the bytes do not
    left, right = FP.Rect.mat(0, 1000, 320, 640, 2), FP.Rect.mat(640, 1000, 320, 640, 2)
    assert left.lo < right.hi and right.lo < left.hi and FP.overlap([left], [right]) is None
    assert FP.overlap([left], [FP.Rect.mat(638, 1000, 320, 640, 2)]) == (638, 640)


def test_writer_map_against_a_byte_array():
    g = np.random.default_rng(3)
    wm, ref = H.WriterMap(cuts=(0, 37, 64, 200)), np.full(400, -1)
    for step in range(200):
        r = FP.Rect.make(int(g.integers(0, 300)), [int(g.integers(1, 6))], [int(g.integers(1, 20))], int(g.integers(1, 12)))
        s, e = r.intervals()
        if step % 3:
            wm.write(s, e, step, step + 1)
            for a, b in zip(s, e):
                ref[a:b] = step
        else:
            (lo, hi, w, al), (us, ue) = wm.lookup(s, e)
            got = np.full(400, -2)
            for a, b, ww in zip(lo, hi, w):
                got[a:b] = ww
            for a, b in zip(us, ue):
                got[a:b] = -1
            want = np.full(400, -2)
            for a, b in zip(s, e):
                want[a:b] = ref[a:b]
            assert (got == want).all() and (al == w + 1).all()


def test_footprint_constants():
    for name in ("SYNC_INTS", "SYNC_BARRIER_INTS", "GN_PART_BYTES", "GN_ROWS_PER_BLOCK", "F16", "F32", "EPI_NONE", "EPI_GEGLU", "EPI_TATTN",
                 "EPI_STATS", "EPI_GN", "EPI_XATTN"):
        assert getattr(FP, name) == getattr(L, name), name
    assert (FP.PLAIN, FP.CONV3X3, FP.TCONV3, FP.CONV3X3_C8) == (L.GATHER_PLAIN, L.GATHER_CONV3X3, L.GATHER_TCONV3, L.GATHER_CONV3X3_C8)
    for name in ("GEMM", "GROUPNORM", "LAYERNORM", "ATTENTION", "SOFTMAX", "NCTHW_TO_CL", "CL_TO_NCTHW", "TIME_EMBED", "COPY2D", "DDIM_STEP", "MEMSET",
                 "LINCOMB", "RELPOS_ATTN", "EMBED_ROWS", "TO_UINT8", "ALLGATHER", "HALO_EXCHANGE", "RESHARD_ROWS", "ALLTOALL", "STATS_HALO", "RESAMPLE",
                 "DEPTH_TOKENS", "AVGPOOL2", "EMPHASIS", "FINGERPRINT"):
        assert getattr(FP, name) == getattr(L, "OP_" + name), name
    assert FP.RELPOS_LONG_COLS(31) == (2 * 31 + 158) // 8 * 8


def test_output_slots_mirror_the_executor():
    """plan_hazards.OUTPUT_SLOTS is csrc/executor.hip output_slots, read from the source."""
    src = open(os.path.join(ROOT, "sd-webui-text2video_amd", "csrc", "executor.hip")).read()
    body = src[src.index("unsigned output_slots(const t2v_op& op)"):]
    body = body[:body.index("\n}\n")]
    found = {}
    for kind, slots in re.findall(r"case T2V_OP_(\w+): return bits\(\{([\d, ]+)\}\)", body):
        found[getattr(FP, kind)] = tuple(int(v) for v in slots.split(","))
    assert found == H.OUTPUT_SLOTS
    assert "gemm_writes_gn(gemm_decode(op).form) ? bits({9})" in body          # (the two GroupNorm forms: T2V_EPI_GN with and without split-K)


# accesses whose mode is not what output_slots says of their slot, each with its reason
ROLE_EXCEPTIONS = {
    (FP.GROUPNORM, 4, "r"): "phase 2 reads the gathered statistics parts of the scratch",
    (FP.ALLGATHER, 0, "w"): "in-place collective: output_slots counts its slot as read",
    (FP.HALO_EXCHANGE, 0, "w"): "in-place collective",
    (FP.STATS_HALO, 0, "w"): "in-place collective",
    (FP.STATS_HALO, 1, "w"): "in-place collective",
    (FP.RESHARD_ROWS, 3, "w"): "the own part's destination: output_slots counts a slot in doubt as read",
}


def test_footprint_roles_agree_with_output_slots(matrix):
    seen = set()
    for label, res in matrix.items():
        if not label.startswith("_"):
            seen |= res["report"].roles
    for kind, slot, mode, is_out in sorted(seen):
        written = mode in ("w", "scratch")
        assert written == is_out or (kind, slot, mode) in ROLE_EXCEPTIONS, (kind, slot, mode, is_out)
    kinds = {k for k, _, _, _ in seen}
    assert kinds >= set(range(1, 25)) - {FP.LINCOMB}, sorted(set(range(1, 25)) - kinds)      # every kind a lowering emits was seen


# rows whose rank holds a SHORT last slice (5 frames over 3 ranks: 2, 2, 1; 125 over 4: 32, 32, 32, 29), with the number of ALLGATHER
# records of the program: each sends this rank's K / V part, padded to the longest slice
PADDED_ALLGATHERS = {"tiny modelscope rank 2/3 of 5 f": 51, "tiny lvdm rank 2/3 of 5 f": 38, "modelscope rank 3/4 of 125 f 32x32": 17}


# ---- 2. the matrix -------------------------------------------------------------------------------------------------------------------
def test_every_row_is_free_of_hazards(matrix):
    rows = {k: v for k, v in matrix.items() if not k.startswith("_")}
    assert len(rows) >= 101 + 11
    classes = [name for name, _, _ in H.INPLACE_CLASSES]
    print("\nin-place classes, in column order: " + " | ".join(classes))
    print(f"{'row':<58} {'ops':>5} {'acc':>6} {'allocs':>6} {'in-place':>8} {'fused ff pairs':>14} {'padding':>7} {'lower s':>8} {'analyse s':>9}")
    bad = []
    for label, res in rows.items():
        rep = res["report"]
        print(f"{label:<58} {rep.ops:5d} {rep.accesses:6d} {rep.allocations:6d} {'/'.join(str(rep.inplace[c]) for c in classes):>8} "
              f"{'/'.join(str(len(v)) for v in rep.fused_pairs.values()):>14} {rep.padding_exempt:7d} {res['lower_s']:8.2f} {rep.seconds:9.2f}")
        bad += [f"{label}: {h}" for h in rep.hazards]
        # the model of the plan-time fusion is the built library's decision, in both plans
        assert res["lib_fused"] == (len(rep.fused_pairs["full"]), len(rep.fused_pairs.get("skip", rep.fused_pairs["full"]))), (label, res["lib_fused"])
        # the one exemption (plan_hazards, R1): the padded all-gathers of the rank that holds a short last slice, and nothing else
        assert rep.padding_exempt == PADDED_ALLGATHERS.get(label, 0), (label, rep.padding_exempt)
        if label in PADDED_ALLGATHERS:
            assert rep.padding_exempt == res["allgathers"] and res["shard"].frames < res["shard"].max_frames
    print(f"analysis {sum(r['report'].seconds for r in rows.values()):.1f} s, lowering {sum(r['lower_s'] for r in rows.values()):.1f} s, "
          f"interpreter protocol {sum(r['confine_s'] for r in rows.values()):.1f} s, fixture {matrix['_seconds']:.1f} s")
    assert not bad, "\n".join(bad[:40])
    # the plan-time fusion of the feed-forward pair is part of what was checked: the full-size rows have pairs, in both plans
    assert len(rows["modelscope b=2 x_batch=1 24 f 32x32"]["report"].fused_pairs["full"]) > 0
    assert rows["modelscope b=2 x_batch=1 24 f 32x32"]["report"].fused_pairs["skip"]


def test_interpreter_stays_inside_the_footprints(matrix):
    rows = {k: v for k, v in matrix.items() if not k.startswith("_") and v["confine"] is not None}
    assert len(rows) >= 60 and sum(v["checked"] for v in rows.values()) > 10000
    bad = [f"{label}: {e}" for label, v in rows.items() for e in v["confine"]]
    print("\n" + "\n".join(f"{label:<58} {v['checked']:5d} ops {v['arena'] / 1e6:6.1f} MB {v['confine_s']:6.2f} s" for label, v in rows.items()))
    assert not bad, "\n".join(bad[:40])


# ---- 3. proof that the rules bite ------------------------------------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    _fixed_environment(monkeypatch)
    return H.Recorder().install(monkeypatch)


def _w(name):
    return Ref("weight", 0, name)


def _flagged(hz, rule, op_index):
    return [h for h in hz if h.rule == rule and h.op == op_index]


def test_seeded_free_before_the_last_reader(rec):
    def build(early):
        P = Program()
        x, y, w = P.alloc(64, 64, "f32"), P.alloc(64, 64, "f32"), P.alloc(64, 64, "f32")
        P.memset("fill.x", x)
        P.copy2d("first reader", x, y)
        if early:
            P.free(x)
        z = P.alloc(16, 64, "f32")                 # first fit: the front of x's block when x was released
        P.memset("fill.z", z)
        P.copy2d("last reader", x, w)
        return P, (z.alloc_off == x.alloc_off)
    P, reused = build(True)
    hz = H.check(P, rec.events(P))
    assert reused and _flagged(hz, "R2", 3) and "last reader" in str(_flagged(hz, "R2", 3)[0]), [str(h) for h in hz]
    P, reused = build(False)
    assert not reused and H.check(P, rec.events(P)) == []


def test_seeded_read_of_an_allocation_nobody_wrote(rec):
    def build(written):
        P = Program()
        x, y = P.alloc(64, 64, "f32"), P.alloc(64, 64, "f16")
        if written:
            P.memset("fill.x", x)
        P.copy2d("reader", x, y)
        return P
    P = build(False)
    hz = H.check(P, rec.events(P))
    assert [h.rule for h in hz] == ["R1"] and hz[0].op == 0 and hz[0].byte_range == (P.ops[0].p[0].off, P.ops[0].p[0].off + 64 * 64 * 4)
    P = build(True)
    assert H.check(P, rec.events(P)) == []


def test_seeded_fused_groupnorm_over_the_gemm_operand(rec, monkeypatch):
    M, N, K = 256, 128, 256

    def build():
        P = Program()
        a, x = P.alloc(M, K, "f16"), P.alloc(M, N, "f32")
        P.memset("fill.a", a)
        P.gemm("conv", a, _w("w"), N, K, x, bias=_w("b"))
        P.free(a)
        P.alloc(64, 1, "f32")                      # a small neighbour takes the front of whatever block is free first
        out = P.alloc(M, N, "f16")
        P.groupnorm("norm", x, _w("g"), _w("be"), out, n_inst=1, eps=1e-5, silu=True, gb=_w("gb"), x_dead=True)
        P.finish()
        return P, a, out
    P, a, out = build()
    assert len(P.ops) == 2 and P.ops[1].i[16] == L.EPI_GN and not (a.alloc_off <= out.alloc_off < a.alloc_off + M * K * 2)
    assert H.check(P, rec.events(P)) == []
    monkeypatch.setattr(Program, "_is_operand_of_last_gemm", lambda self, b: False)
    P, a, out = build()
    assert len(P.ops) == 2 and P.ops[1].i[16] == L.EPI_GN and a.alloc_off < out.alloc_off < a.alloc_off + M * K * 2
    hz = H.check(P, rec.events(P))
    hit = _flagged(hz, "R3", 1)
    assert hit and hit[0].slots == [9, 0] and hit[0].ops[0][1] == "conv", [str(h) for h in hz]


def test_seeded_output_on_the_tickets(rec):
    def build(on_sync):
        P = Program()
        x, y = P.alloc(8, 64, "f32"), P.alloc(8, 64, "f32")
        P.memset("fill.x", x)
        P.copy2d("copy", x, Buf(P.sync_ref("tickets"), 8, 64, 64, "f32") if on_sync else y)
        return P
    P = build(True)
    hit = _flagged(H.check(P, rec.events(P)), "R5", 1)
    assert hit and hit[0].slots == [1]
    P = build(False)
    assert H.check(P, rec.events(P)) == []


def test_seeded_invariant_output_released_and_reused(rec):
    def build(reuse):
        P = Program()
        kv, y, w = P.alloc(64, 64, "f16"), P.alloc(64, 64, "f16"), P.alloc(64, 64, "f16")
        P.copy2d("context.kv", Buf(Ref("ext", L.EXT_CTX), 64, 64, 64, "f32"), kv).meta["step_invariant"] = True
        P.copy2d("consumer", kv, y)
        if reuse:
            P.free(kv)
        z = P.alloc(64, 64, "f16")
        P.copy2d("later writer", y, z)
        P.copy2d("tail", z, w)
        return P, z.alloc_off == kv.alloc_off
    P, reused = build(True)
    hz = H.check(P, rec.events(P))
    skip = [h for h in _flagged(hz, "R4", 1) if h.plan == "skip" and "pass 2" in h.detail]
    assert reused and skip and skip[0].ops[1][1] == "later writer" and any("released" in h.detail for h in _flagged(hz, "R4", 1)), [str(h) for h in hz]
    assert any(h.rule == "R4" and h.op == 2 and "non-invariant op writes" in h.detail for h in hz)
    P, reused = build(False)
    assert not reused and H.check(P, rec.events(P)) == []


def test_seeded_residual_in_place_with_and_without_wrap(rec):
    M, N, K = 128, 128, 64
    P = Program()
    a, out = P.alloc(M, K, "f16"), P.alloc(M, N, "f32")
    P.memset("fill.a", a)
    P.memset("fill.out", out)
    op = P.gemm("residual add", a, _w("w"), N, K, out, bias=_w("b"), residual=out, allow_splitk=False)
    P.finish()
    rep = H.analyse(P, rec.events(P))
    assert rep.hazards == [] and rep.inplace["gemm residual == out (fp32, same ld, no wrap)"] == 1 and sum(rep.inplace.values()) == 1
    op.i[30] = M // 2                                   # the same record with the residual's rows wrapped: row m >= R reads row m - R
    hit = _flagged(H.check(P, rec.events(P)), "R3", 2)
    assert hit and hit[0].slots == [5, 4]


def test_seeded_window_into_the_hidden_tensor(rec, built_lib):
    M = 256

    def build(reach):
        P = Program()
        x, pre, hidden, out, sink = P.alloc(M, 320, "f16"), P.alloc(8, 1280, "f16"), P.alloc(M, 1280, "f16"), P.alloc(M, 320, "f32"), P.alloc(16, 1280, "f32")
        assert hidden.ref.off == pre.ref.off + 8 * 1280 * 2
        P.memset("fill.x", x)
        P.memset("fill.pre", pre)
        ff1 = P.gemm("ff.net.0", x, _w("w1"), 2560, 320, hidden, bias=_w("b1"), epi=L.EPI_GEGLU, allow_splitk=False)
        P.gemm("ff.net.2", hidden, _w("w2"), 320, 1280, out, bias=_w("b2"), allow_splitk=False)
        ff1.i[31] = 1                                   # the test hook of csrc/executor.hip ff_pair: the row cut-off is waived
        rows = 16 if reach else 8
        P.copy2d("window", Buf(pre.ref, rows, 1280, 1280, "f16"), Buf(sink.ref, rows, 1280, 1280, "f32"))
        P.finish()
        return P
    P = build(True)
    A = H._Addr()
    fps = [FP.footprint(op) for op in P.ops]
    assert H.ff_pair_pointer(P.ops, 2, A) and not H.ff_pair_extent(P.ops, fps, 2, A)[0] and not H.ff_pair_library(P.ops, fps, 2, A)
    assert _launches(built_lib, P) == len(P.ops)                       # the library itself: two launches for the pair
    assert H.check(P, rec.events(P)) == [] or all(h.rule != "R6" for h in H.check(P, rec.events(P)))
    hit = _flagged(H.check(P, rec.events(P), ff_model=H.ff_pair_pointer), "R6", 2)     # a scan on base pointers would have fused
    assert hit and "pointer model fuses" in hit[0].detail and "window" in hit[0].detail and hit[0].ops[1][1] == "ff.net.2"
    hidden = P.ops[2].p[5].off
    assert hit[0].byte_range == (hidden, hidden + 8 * 1280 * 2)          # the rows of the hidden tensor the window reaches into
    P = build(False)
    rep = H.analyse(P, rec.events(P))
    assert rep.hazards == [] and rep.fused_pairs["full"] == [2] and _launches(built_lib, P) == len(P.ops) - 1


def test_protocol_notices_a_wrong_footprint(rec, monkeypatch):
    """The protocol itself, on the tiny LVDM program with the table edited: a read left out, a write left out, a write two bytes too wide."""
    r = next(r for r in PD.rows(ROOT) if r.label == "tiny lvdm defaults")
    comp = _lower(r)
    table = FP.footprint

    def errors(edit):
        monkeypatch.setattr(H, "footprint", lambda op: edit(table(op)))
        return _confine(comp, r)[0]

    def widen(f):
        for x in f:
            if x.what == "out" and x.slot == 5 and x.space == "arena":
                x.rects = [FP.Rect(q.off, q.counts, q.pitches, q.row + 2) for q in x.rects]
        return f

    assert errors(lambda f: f) == []
    assert any("slot 5 out" in e and "differ" in e for e in errors(lambda f: [x for x in f if x.what != "residual"]))
    assert any("outside every declared rectangle" in e for e in errors(lambda f: [x for x in f if x.what != "gn_out"]))
    assert any("slot 5 out: 2 bytes differ" in e for e in errors(widen))


def test_seeded_all_gather_of_unwritten_bytes(rec):
    """What a collective sends is read like anything else; only the padding tail of a short last slice is left out, and only with the
    row's TShardSpec."""
    from sd_webui_text2video_amd.program import TShardSpec
    short, even = TShardSpec.make(5, 3, 2), TShardSpec.make(6, 3, 2)       # slices 2, 2, 1 (this rank: one frame of two) / 2, 2, 2
    frame = 64 * 64 * 2

    def build(spec, written_frames):
        P = Program()
        kv = P.alloc(3 * 2 * 64, 64, "f16")                                # three parts of two frames
        if written_frames:
            P.memset("kv", Buf(kv.ref.shifted(2 * 2 * frame), written_frames * 64, 64, 64, "f16"))
        P.allgather("kv.allgather", kv, 2 * frame, spec)
        return P, kv.ref.off + 2 * 2 * frame
    P, own = build(short, 1)
    rep = H.analyse(P, rec.events(P), shard=short)
    assert rep.hazards == [] and rep.padding_exempt == 1
    hz = H.check(P, rec.events(P))                                         # without the spec there is no exemption
    assert [h.rule for h in hz] == ["R1"] and hz[0].op == 1 and hz[0].byte_range == (own + frame, own + 2 * frame)
    P, own = build(short, 0)                                               # the real frame itself was never produced
    hz = H.analyse(P, rec.events(P), shard=short).hazards
    assert [h.rule for h in hz] == ["R1"] and hz[0].op == 0 and hz[0].byte_range == (own, own + frame)
    P, own = build(even, 1)                                                # no short slice: the second frame is real data
    rep = H.analyse(P, rec.events(P), shard=even)
    assert [h.rule for h in rep.hazards] == ["R1"] and rep.padding_exempt == 0 and rep.hazards[0].byte_range == (own + frame, own + 2 * frame)
    P, own = build(even, 2)
    assert H.analyse(P, rec.events(P), shard=even).hazards == []
