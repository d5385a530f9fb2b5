"""CPU: the inputs of tests/fused_attention_inputs.py do what tests/test_gpu_fused_attention_adversarial.py needs them to do.

Everything here depends on the inputs, the float64 reference (adversarial.softmax_attention_ref) and a float64 emulation of each kernel's
arithmetic and index arithmetic, written out below from the kernels — never on the product.  The emulation: q, k, v are fp16; the maximum
is taken over the visible key slots; exp2; P is rounded to fp16 before it meets V while the row sum uses the unrounded P; the output is
rounded to fp16; the two-role cases add adversarial.stale_max_schedule.  The XATTN emulation reads K and V^T from the same memory images the
programs are initialised with (fences included), at the addresses the kernel computes.

  * every case's emulation stays within EMU_BOUND = 5e-4 of the reference on EVERY segment (a quarter of the GPU tolerance); the dense TATTN
    cases take their projection from torch's fp32 matmul on the CPU;
  * every mutation — a variant of the emulation or of its index arithmetic — pushes EVERY affected segment past 10 x the GPU tolerance;
    the test names the affected segments and asserts there are some;
  * confined to a single segment, such a mutation passes a whole-tensor rel-L2 at the GPU tolerance;
  * t2v_epilogue_xattn's three key blocks: with all three blocks loaded whatever the key count (the kernel before this suite) the emulation
    meets the NaN rows behind a sample's V^T in the last head whenever the keys fill fewer than 96 columns; bounded by ceil(keys / 32) it
    does not;
  * every case's program runs through the interpreter under the GPU file's checks (fences, finiteness, tolerance, bit-exact rows);
  * the case list covers what it names."""
import math

import pytest
import torch

import adversarial as A
import fused_attention_inputs as FA
from interp import Interp
from interp_prompt import PromptInterp
from sd_webui_text2video_amd import _lib as L

BY = {f: [c for c in FA.CASES if c["family"] == f] for f in ("tattn", "xattn", "two_role")}
FAR = 10 * FA.TOL
_BUILT = {}


def built(c):
    if c["id"] not in _BUILT:
        _BUILT[c["id"]] = FA.build(c)
    return _BUILT[c["id"]]


def _softmax_pv(sc, vis, v, premask=False):
    """sc [.., nq, ns] log2 units, vis [ns] bool, v [.., ns, D] -> fp16(P) V / sum P with the maximum over the visible slots (premask: over all)."""
    masked = sc.masked_fill(~vis, -math.inf)
    m = (sc if premask else masked).max(dim=-1, keepdim=True).values
    p = torch.exp2(masked - m)
    return (p.half().double() @ v) / p.sum(dim=-1, keepdim=True)


# ---- T2V_EPI_TATTN ----------------------------------------------------------------------------------------------------------------------------
TATTN_MUTATIONS = ("premask", "F+1", "pixel+1", "base12", "sample0", "kswap", "frame_major", "scale")


def tattn_emulate(b, mut=None):
    c, x = b.case, b.x
    S, F, HW, heads, tpix = c["S"], c["F"], c["HW"], c["heads"], x["tpix"]
    q, k, v = x["q"], x["k"], x["v"]
    if c["dense"]:
        a32 = x["a2d"].float()
        q, k, v = ((a32 @ x[n].float().t()).half().double().view(S, F, HW, heads, 64) for n in ("wq", "wk", "wv"))
    sl2 = x["scale"] * A.LOG2E * (A.LOG2E if mut == "scale" else 1.0)      # exp() of the base-2 argument
    out = torch.full((S, F, HW, heads, 64), float("nan"), dtype=torch.float64)
    hk = torch.tensor([min(h ^ 1, heads - 1) if mut == "kswap" else h for h in range(heads)])
    r = torch.arange(tpix * F)
    pl_r, f_r = (r % tpix, r // tpix) if mut == "frame_major" else (r // F, r % F)
    vis = torch.arange(32) < F + (1 if mut == "F+1" else 0)
    for s in range(S):
        ss = 0 if mut == "sample0" else s
        for t in range(-(-HW // tpix)):
            # the LDS image of the tile: rows of dead pixels and dead rows are zero (the slots behind row 191 are the V^T bytes: finite, not modelled)
            Q, K, V = (torch.zeros(256, heads, 64, dtype=torch.float64) for _ in range(3))
            pix_r = t * (12 if mut == "base12" else tpix) + pl_r
            ok = pix_r < HW
            Q[r[ok]], K[r[ok]], V[r[ok]] = q[ss, f_r[ok], pix_r[ok]], k[ss, f_r[ok], pix_r[ok]][:, hk], v[ss, f_r[ok], pix_r[ok]]
            for pl in range(tpix):
                pix = t * tpix + pl
                if pix >= HW:
                    continue
                r0 = (pl + (1 if mut == "pixel+1" else 0)) * F
                sc = torch.einsum("fhd,ghd->hfg", Q[r0:r0 + F], K[r0:r0 + 32]) * sl2
                vs = torch.zeros(heads, 32, 64, dtype=torch.float64)             # V^T slots F .. 31 are zeroed
                vs[:, :F] = V[r0:r0 + F].permute(1, 0, 2)
                out[s, :, pix] = _softmax_pv(sc, vis, vs, premask=mut == "premask").permute(1, 0, 2)
    return b.to_seg(out.half().double().reshape(S * F * HW, heads * 64))


def tattn_affected(b, mut):
    c = b.case
    S, F, HW, heads, tpix = c["S"], c["F"], c["HW"], c["heads"], b.x["tpix"]
    s, pix, h = torch.meshgrid(torch.arange(S), torch.arange(HW), torch.arange(heads), indexing="ij")
    spike = torch.tensor([FA.tattn_spike_frame(p, F, HW, tpix) for p in range(HW)])[pix]
    every = torch.ones_like(pix, dtype=torch.bool)
    placed = not c["dense"]
    return {"premask": (spike >= 0) & placed, "F+1": (spike == 0) & placed, "pixel+1": every, "base12": (pix >= tpix) & (tpix != 12), "sample0": s >= 1,
            "kswap": torch.tensor([min(hh ^ 1, heads - 1) != hh for hh in range(heads)])[h], "frame_major": every, "scale": every}[mut].reshape(-1)


# ---- T2V_EPI_XATTN ----------------------------------------------------------------------------------------------------------------------------
XATTN_MUTATIONS = ("unmasked", "unclamped", "tile_sample", "sample0", "swap_in", "swap_across", "vt_stride", "koff", "scale")


def xattn_emulate(b, mut=None, bounded=True):
    c, x = b.case, b.x
    tile, N, B, rows, Lc = c["tile"], c["N"], c["B"], c["rows"], c["Lc"]
    heads, M, lcp = N // 64, B * rows, x["lcp"]
    BM, BN = FA.XA_BM[tile], FA.XA_BN[tile]
    HEADS = BN // 64
    q2d = x["q"].reshape(M, N)
    nan_rows = lambda img, n: torch.cat([img, torch.full((n, img.shape[1]), float("nan"), dtype=torch.float64)])
    kimg, vflat = nan_rows(x["k_img"], 200), nan_rows(x["vt_img"], 8).reshape(-1)
    sl2 = (1.0 if mut == "scale" else x["scale"]) * A.LOG2E
    slots = torch.arange((-(-Lc // 32) if bounded else 3) * 32)
    vis = torch.ones_like(slots, dtype=torch.bool) if mut == "unmasked" else slots < Lc
    koff = 0 if mut == "koff" else FA.K_COL0
    out = torch.empty(M, N, dtype=torch.float64)
    for mt in range(0, M, 32):
        m0 = mt // BM * BM
        smp = {"tile_sample": m0 // rows, "sample0": 0}.get(mut, mt // rows)
        for h in range(heads):
            n0 = h * 64 // BN * BN
            hh = h - n0 // 64
            hk = {"swap_in": n0 // 64 + HEADS - 1 - hh, "swap_across": (h + HEADS) % heads}.get(mut, h)
            krow = x["k_row0"] + smp * Lc + (slots if mut == "unclamped" else slots.clamp(max=Lc - 1))
            kk = kimg[krow, koff + hk * 64: koff + hk * 64 + 64]
            sc = q2d[mt:mt + 32, h * 64:(h + 1) * 64] @ kk.t() * sl2
            row = x["vt_row0"] + smp * (N if mut == "vt_stride" else x["vt_per"]) + hk * 64 + torch.arange(64)
            vt = vflat[row[:, None] * lcp + slots[None, :]]                      # the loads run along the row, into the next rows past lcp
            out[mt:mt + 32, h * 64:(h + 1) * 64] = _softmax_pv(sc, vis, vt.t(), premask=mut == "unclamped")
    return b.to_seg(out.half().double())


def xattn_affected(b, mut):
    c = b.case
    tile, N, B, rows, Lc = c["tile"], c["N"], c["B"], c["rows"], c["Lc"]
    heads, BM, BN = N // 64, FA.XA_BM[tile], FA.XA_BN[tile]
    mt, h = torch.meshgrid(torch.arange(0, B * rows, 32), torch.arange(heads), indexing="ij")
    every = torch.ones_like(h, dtype=torch.bool)
    hh = h % (BN // 64)
    # a strip with a row on which one key stands >= 30 log2 units above the rest returns that key's v whatever the softmax does with the others
    free = ~b.exact_rows.reshape(-1, 32, heads).any(dim=1)
    return {"unmasked": free & (Lc % 32 != 0), "unclamped": free & (Lc % 32 != 0), "tile_sample": (mt // BM * BM) // rows != mt // rows,
            "sample0": mt // rows >= 1, "swap_in": (BN // 64 - 1 - hh) != hh, "swap_across": every & (N > BN), "vt_stride": mt // rows >= 1,
            "koff": every & (Lc > 1), "scale": free & (Lc > 1)}[mut].reshape(-1)


# ---- the second role of T2V_OP_ATTENTION -----------------------------------------------------------------------------------------------------
ROLE_MUTATIONS = ("nk1", "stride1", "bo", "skip_o")


def roles_emulate(b, mut=None, stats=None):
    c, x = b.case, b.x
    D, nq, F, heads, V, (L1, L2) = c["D"], c["nq"], c["F"], c["heads"], c["V"], c["lens"]
    inner = heads * D
    img = torch.cat([x["kv_img"], torch.full((400, x["kv_img"].shape[1]), float("nan"), dtype=torch.float64)])
    outs = []
    for bo in range(2 * V):
        alt = bo >= V
        nk = L1 if (not alt or mut == "nk1") else L2
        stride = L1 if (not alt or mut == "stride1") else L2
        idx = bo if (not alt or mut == "bo") else bo - V
        base = x["kv_row0"] + (V * L1 if alt else 0) + idx * stride
        kk = img[base:base + nk, :inner].reshape(nk, heads, D).permute(1, 0, 2)
        vv = img[base:base + nk, inner:2 * inner].reshape(nk, heads, D).permute(1, 0, 2)
        qq = x["roles"][int(alt)]["q"].reshape(V, heads, F * nq, D)[bo - V if alt else bo]
        lg2 = torch.einsum("htd,hsd->hts", qq, kk) * x["scale"] * A.LOG2E
        s = A.stale_max_schedule(lg2, vv, x["tile"], skip="o" if (alt and mut == "skip_o") else None)
        if stats is not None and alt:
            stats.append(s)
        outs.append(s["out"].reshape(heads, F, nq, D).permute(1, 2, 0, 3).reshape(F * nq, inner))
    return b.to_seg(torch.cat(outs).half().double())


def roles_affected(b, mut):
    c = b.case
    V, F, heads = c["V"], c["F"], c["heads"]
    bo = torch.arange(2 * V).repeat_interleave(F * heads)
    late = -(-c["lens"][1] // b.x["tile"]) >= 2
    first = V + 1 if c["variant"] == "masked" else V          # (the sample whose key 0 carries the 40-unit spike has its maximum in the first tile)
    free = ~b.exact_rows.reshape(2 * V, F, c["nq"], heads).any(dim=2).reshape(-1)       # (as in xattn_affected)
    return {"nk1": (bo >= V) & free, "stride1": bo >= V + 1, "bo": bo >= V, "skip_o": (bo >= first) & late}[mut]


FAMILY = dict(tattn=(tattn_emulate, tattn_affected, TATTN_MUTATIONS), xattn=(xattn_emulate, xattn_affected, XATTN_MUTATIONS),
              two_role=(roles_emulate, roles_affected, ROLE_MUTATIONS))


# ---- the tests --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FA.CASES, ids=lambda c: c["id"])
def test_emulation_stays_within_a_quarter_of_the_gpu_tolerance_on_every_segment(c):
    b = built(c)
    for t in (b.x.get("q"), b.x.get("k"), b.x.get("v")):
        assert t is None or (torch.equal(t, t.half().double()) and torch.isfinite(t).all())
    stats = []
    emu = FAMILY[c["family"]][0](b) if c["family"] != "two_role" else roles_emulate(b, stats=stats)
    e = FA.seg_errors(emu, b.ref)
    print(f"EMU {c['id']}: worst segment {float(e.max()):.2e}, mean {float(e.mean()):.2e} over {len(e)} segments")
    assert float(e.max()) < FA.EMU_BOUND, (c["id"], float(e.max()))
    if c["family"] == "two_role" and -(-c["lens"][1] // b.x["tile"]) >= 2:
        # running maxima advance after the first tile in every role-2 sample (but the one whose key 0 carries the 40-unit spike)
        late = stats[1:] if c["variant"] == "masked" else stats
        assert all(s["pairs_late"] >= 0.10 * s["pairs"] for s in late), [(s["pairs_late"], s["pairs"]) for s in stats]
        assert late or c["V"] == 1


@pytest.mark.parametrize("family,mut", [(f, m) for f in FAMILY for m in FAMILY[f][2]])
def test_every_mutation_lands_far_outside_the_tolerance_on_every_affected_segment(family, mut):
    emulate, affected, _ = FAMILY[family]
    lo, n_aff, where = float("inf"), 0, []
    for c in BY[family]:
        b = built(c)
        aff = affected(b, mut)
        assert aff.shape == (b.ref.shape[0],)
        if not bool(aff.any()):
            continue
        e = FA.seg_errors(emulate(b, mut), b.ref)
        where.append(f"{c['id']} ({int(aff.sum())} of {len(aff)}: {float(e[aff].min()):.2g})")
        n_aff += int(aff.sum())
        lo = min(lo, float(e[aff].min()))
        assert bool((e[aff] > FAR).all()), (c["id"], mut, float(e[aff].min()), int(torch.nonzero(aff)[int(e[aff].argmin())]))
    print(f"MUT {family} {mut}: smallest affected-segment error {lo:.3g} over {n_aff} affected segments — " + "; ".join(where))
    assert n_aff > 0, (family, mut)


def test_a_whole_tensor_rel_l2_misses_a_mutated_segment():
    """A mutation confined to ONE affected segment (the one that weighs least in the tensor: v's scale differs by segment): that segment is
    more than 10 x the tolerance off while one rel-L2 over the tensor stays inside the tolerance."""
    b = built(BY["tattn"][0])
    clean, missed = tattn_emulate(b), []
    for mut in TATTN_MUTATIONS:
        bad, aff = tattn_emulate(b, mut), tattn_affected(b, mut)
        if not bool(aff.any()):
            continue
        k = int((bad - b.ref).norm(dim=1).masked_fill(~aff, float("inf")).argmin())
        mixed = clean.clone()
        mixed[k] = bad[k]
        seg, whole = float(FA.seg_errors(mixed, b.ref)[k]), A.rel_l2(mixed, b.ref)
        print(f"MISS tattn {mut}: segment {k} is {seg:.3g} off, the whole tensor {whole:.2e}")
        assert seg > FAR
        if whole < FA.TOL:
            missed.append(mut)
    assert missed


@pytest.mark.parametrize("c", BY["xattn"], ids=lambda c: c["id"])
def test_xattn_key_blocks_beyond_the_key_count_meet_the_nan_behind_vt(c):
    b = built(c)
    heads = c["N"] // 64
    last_head = (torch.arange(b.ref.shape[0]) % heads) == heads - 1
    assert torch.isfinite(xattn_emulate(b)).all()
    bad = ~torch.isfinite(xattn_emulate(b, bounded=False)).all(dim=1)
    if b.x["lcp"] < 96:
        assert bool(bad[last_head].all()) and not bool(bad[~last_head].any()), c["id"]
    else:
        assert not bool(bad.any())


@pytest.mark.parametrize("c", FA.CASES, ids=lambda c: c["id"])
def test_programs_pass_the_gpu_checks_in_the_interpreter(c):
    b = built(c)
    it = (PromptInterp if b.interp == "PromptInterp" else Interp)(b.P, b.w, poison=False)
    b.init(it)
    it.run({})
    figs = FA.verify(it, b)
    if c["family"] == "two_role":
        FA.verify_pair_equals_singles(it, b)
    print(FA.figures_line(b, figs).replace("ADV", "INTERP"))
    if c["family"] == "xattn" and c["Lc"] == 1:
        assert figs["exact"] == c["B"] * c["rows"] * (c["N"] // 64) and figs["worst"] == 0.0
    if c.get("variant") == "masked" or c.get("wrap"):
        assert figs["exact"] > 0


def test_case_list_covers_what_it_names():
    bs = [built(c) for c in FA.CASES]
    xa = [b for b in bs if b.case["family"] == "xattn"]
    assert {b.P.ops[0].meta["tile"] for b in xa} == {8, 11, 5, 0}
    assert {b.P.ops[0].i[25] for b in xa} == {1, 7, 32, 33, 64, 65, 77, 96}
    assert {(b.P.ops[0].i[22], b.P.ops[0].i[25], b.P.ops[0].i[26]) for b in xa} >= {(0, 7, 32), (5, 7, 32)}
    assert any(b.P.ops[0].i[13] == b.P.ops[0].i[15] == 96 for b in xa)                       # a_wrap
    for b in xa:                                                                            # a sample seam inside a row tile, where named
        op = b.P.ops[0]
        if b.case["id"] in ("xattn-t8-n320-b2-r160-k77", "xattn-t5-n256-b2-r96-k65"):
            assert op.i[15] % FA.XA_BM[op.i[22]] != 0 and bool(xattn_affected(b, "tile_sample").any())
    ta = [b.P.ops[0] for b in bs if b.case["family"] == "tattn"]
    assert all(op.i[16] == L.EPI_TATTN and op.i[22] == 10 for op in ta)
    assert {op.i[10] for op in ta} == {6, 8, 11, 12}
    live = {op.i[10] * op.i[8] for op in ta}
    assert 192 in live and min(live) < 96                                                   # a full and a partly filled tile
    assert any(op.i[9] % op.i[10] for op in ta)                                             # a ragged last tile
    assert {32 - op.i[8] for op in ta} >= {0, 1, 8, 30}                                      # masked slots
    assert sum(1 for op in ta if op.i[2] == 320 and op.i[1] == 5 * 192) == 2                 # the dense cases: five column tiles
    # launch_attn's rule, written out in fused_attention_inputs.attn_variant, on the op records
    variants = set()
    for b in bs:
        if b.case["family"] == "two_role":
            op = b.P.ops[0]
            assert op.i[19] > 0 and op.i[20] > 0
            variants.add(FA.attn_variant(op.i[0], op.i[1], op.i[20]))
    assert variants == {(4, 64), (1, 64), (1, 32)}
    assert {b.case["V"] for b in bs if b.case["family"] == "two_role"} == {1, 2}
    assert {b.case["D"] for b in bs if b.case["family"] == "two_role"} == {40, 64}
