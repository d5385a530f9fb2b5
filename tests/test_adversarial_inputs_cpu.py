"""CPU: the adversarial attention inputs of tests/adversarial.py do what tests/test_gpu_attention_adversarial.py needs them to do.

Every condition here depends on the inputs, the float64 reference and the float64 emulation of the kernels' stale-maximum schedule only —
never on the product.  For EVERY case the GPU file runs (the lists are imported from tests/adversarial.py by both):
  * the emulated schedule matches the float64 softmax to 1e-4 (what is left is the fp16 rounding of P);
  * where the keys span two tiles or more: at least 10 % of the (item, query) pairs advance their running maximum on a tile after the
    first, at least one 32-query block has some but not all of its queries advance, and the schedule WITHOUT the rescale of O is off by
    more than 0.1 — 50 times the loosest tolerance of the GPU file;
  * for the long-clip kernel, where an advance meets a non-zero w_lo / w_hi: the schedule WITHOUT their rescale is off by more than 0.1, and
    over the case list advances meet a non-zero w_lo and a non-zero w_hi.
The single-tile cases (nk <= 32 on attn_kernel<1, D, 32>, clips of <= 32 frames) are exempt from the conditions on advances: their only
rescale multiplies zeros by exp2(-inf).  They check the range of 2^x and the masks."""
import math

import pytest
import torch

import adversarial as A


def _measure(c, rel):
    if rel:
        x = A.relpos_inputs(c)
        full, sched, causal, tile = (x["ek"], x["ev"], c["R"], c["off"]), (x["ev"], c["R"], c["off"]), False, 32
    else:
        x = A.attn_inputs(c)
        full, sched, causal, tile = None, None, c["causal"], c["tile"]
    ref = A.softmax_attention_ref(x["q"], x["k"], x["v"], x["scale"], causal, full)
    lg2 = A.logits(x["q"], x["k"], x["scale"], causal, full) * A.LOG2E
    s = A.stale_max_schedule(lg2, x["v"], tile, rel=sched)
    ntiles = -(-x["k"].shape[1] // tile)
    return x, ref, lg2, s, ntiles, tile, sched


def _check(c, rel):
    x, ref, lg2, s, ntiles, tile, sched = _measure(c, rel)
    for t in (x["q"], x["k"], x["v"]):
        assert torch.equal(t, t.half().double()) and torch.isfinite(t).all()
    assert torch.isfinite(ref).all()
    err = A.rel_l2(s["out"], ref)
    print(f"{c['id']}: schedule vs float64 {err:.2e}, advances on {s['pairs_late']} of {s['pairs']} pairs, mixed blocks {s['mixed']}, "
          f"w_lo hits {s['w_lo_hits']}, w_hi hits {s['w_hi_hits']}")
    assert err < 1e-4, err
    if ntiles < 2:
        assert s["late"] == 0
        return s
    assert s["pairs_late"] >= 0.10 * s["pairs"], (s["pairs_late"], s["pairs"])
    assert s["mixed"] >= 1
    no_o = A.rel_l2(A.stale_max_schedule(lg2, x["v"], tile, rel=sched, skip="o")["out"], ref)
    assert no_o > 0.1, no_o
    if s["w_lo_hits"] + s["w_hi_hits"] > 0:
        no_w = A.rel_l2(A.stale_max_schedule(lg2, x["v"], tile, rel=sched, skip="w")["out"], ref)
        assert no_w > 0.1, no_w
    return s


@pytest.mark.parametrize("c", A.ATTN_CASES, ids=lambda c: c["id"])
def test_attention_cases_reach_the_rescale(c):
    _check(c, False)


@pytest.mark.parametrize("c", A.RELPOS_LONG_CASES + A.RELPOS_SHORT_CASES, ids=lambda c: c["id"])
def test_relpos_cases_reach_the_rescale(c):
    _check(c, True)


def test_long_clip_cases_rescale_both_edge_masses():
    """Over the list: advances on a non-zero w_lo and on a non-zero w_hi; a whole clip with T >= R + 96 has both, a slice at the end of
    the clip only w_lo, every case with an edge tile followed by a later tile at least one."""
    lo = hi = 0
    for c in A.RELPOS_LONG_CASES:
        s = _measure(c, True)[3]
        lo, hi = lo + s["w_lo_hits"], hi + s["w_hi_hits"]
        if c["Tq"] == c["T"] and c["T"] >= c["R"] + 96:
            assert s["w_lo_hits"] > 0 and s["w_hi_hits"] > 0, c["id"]
        if c["off"] + c["Tq"] == c["T"] and c["off"] >= c["R"] + 64:
            assert s["w_lo_hits"] > 0 and s["w_hi_hits"] == 0, c["id"]
    assert lo > 0 and hi > 0


def test_case_lists_cover_what_they_name():
    ids = [c["id"] for c in A.ATTN_CASES + A.RELPOS_LONG_CASES + A.RELPOS_SHORT_CASES]
    assert len(ids) == len(set(ids))
    spatial = {(c["D"], c["nq"]) for c in A.ATTN_CASES if c["id"].startswith("spatial") and c["variant"] == "late"}
    assert spatial == {(D, hw) for D in (40, 64, 80, 160) for hw in (300, 1000)}
    assert {c["nq"] for c in A.ATTN_CASES if c["causal"]} == {77, 129, 200}
    assert {(c["nq"], c["waves"]) for c in A.ATTN_CASES if c["attn2"] and c["variant"] == "late"} == {(1024, 8), (1000, 4), (2304, 0), (320, 8)}
    assert {(c["D"], c["T"], c["R"]) for c in A.RELPOS_LONG_CASES if c["Tq"] == c["T"] and c["variant"] == "late"} == {
        (40, 250, 16), (64, 100, 2), (80, 125, 16), (160, 48, 16), (40, 33, 2), (160, 64, 63), (40, 1024, 16), (160, 40, 16)}
    assert {(c["D"], c["T"], c["Tq"], c["off"], c["R"]) for c in A.RELPOS_LONG_CASES if c["Tq"] != c["T"]} == {
        (64, 250, 84, 166, 2), (40, 64, 20, 0, 16), (80, 100, 34, 33, 16)} | {(D, 40, 5, off, 16) for D in (40, 80, 160) for off in (0, 35)}
    assert {c["T"] for c in A.RELPOS_SHORT_CASES} == {5, 8, 16, 17, 18, 24, 25, 32}
    # T-sharded slices on the VALU kernel: the start, the middle and the end of clips of 5, 8 and 16 frames
    shard = {(c["T"], c["off"], c["off"] + c["Tq"] == c["T"]) for c in A.RELPOS_SHORT_CASES if c["Tq"] < c["T"] and 0 in c["sels"]}
    assert {(T, pos) for T in (5, 8, 16) for pos in ("start", "middle", "end")} | {(24, "start"), (24, "middle")} == {
        (T, "start" if off == 0 else "end" if end else "middle") for T, off, end in shard}
    for c in A.RELPOS_SHORT_CASES:                        # the selectors each case names apply to it
        if 1 in c["sels"]:
            assert c["R"] >= c["T"] - 1 and c["R"] <= 31
        if 2 in c["sels"]:
            assert c["T"] <= 16 and c["R"] >= c["T"] - 1


def test_spikes_arrive_in_every_tile_position():
    """Over the late-maximum cases the planted maximum arrives in the first tile, the last tile and tiles in between, and the two spikes of
    an item sit in different tiles somewhere (even and odd lanes of one block advance at different times)."""
    first = last = middle = split = 0
    for c in A.ATTN_CASES:
        if c["variant"] != "late" or c["placement"] != "cycle":
            continue
        nt = -(-c["nk"] // c["tile"])
        items = c["B"] * c["heads"] * (1 if c["layout"] == "cross" else c["F"])
        for it in range(items):
            s0, s1 = A.spike_keys(it, c["nk"], c["tile"], c["placement"], c["shift"])
            assert 0 <= s0 < c["nk"] and 0 <= s1 < c["nk"] and s0 != s1
            j0, j1 = s0 // c["tile"], s1 // c["tile"]
            first += j0 == 0 and nt > 1
            last += j0 == nt - 1 and nt > 1
            middle += 0 < j0 < nt - 1
            split += j0 != j1
    assert first and last and middle and split


def test_masked_spikes_dominate_where_they_are_visible_only():
    """masked_spike: how far the planted logit stands above every other logit of the row (40 log2 units less the late-maximum spike of up to
    ~12 and the query's own noise along the spike).  A maximum taken before the mask scales the row's visible probabilities by 2^-gap: from
    2^-25 on the fp16 P operand is zero (the median row), and at 2^-16 it is already below fp16's smallest normal 2^-14, so at most 8 of its
    bits survive — an error of 2^-9 = 2e-3, the tolerance (nine rows in ten; the query noise along the spike is 5 log2 units wide)."""
    for c in A.ATTN_CASES:
        if c["variant"] != "masked":
            continue
        x = A.attn_inputs(c)
        lg2 = A.logits(x["q"], x["k"], x["scale"], False, None) * A.LOG2E         # unmasked
        seen = 0
        for it, s in enumerate(x["keys"]):
            if s < 0:
                assert not c["causal"]
                continue
            row = lg2[it]
            others = torch.cat([row[:, :s], row[:, s + 1:]], dim=1).max(dim=1).values
            gap = row[:, s] - others
            assert gap.median() >= 25.0 and (gap >= 16.0).double().mean() >= 0.9, (c["id"], it, float(gap.min()), float(gap.median()))
            seen += 1
        assert seen >= 1
        assert float(x["spare_k"].abs().max()) < 6e4


def test_reference_is_the_explicit_formula():
    """softmax_attention_ref against torch.softmax written the way tests/test_gpu_relpos_long.py writes it (float64), with and without the
    relative-position terms and the causal mask."""
    g = torch.Generator().manual_seed(5)
    items, Tq, T, D, R, off = 3, 7, 19, 8, 4, 6
    q, k, v = (torch.randn(items, n, D, generator=g, dtype=torch.float64) for n in (Tq, T, T))
    ek, ev = A.rel_tables(R, D, 9)
    idx = (torch.arange(T)[None, :] - (torch.arange(Tq)[:, None] + off)).clamp(-R, R) + R
    sim = (torch.einsum("itd,isd->its", q, k) + torch.einsum("itd,tsd->its", q, ek[idx])) * 0.3
    p = sim.softmax(dim=-1)
    want = torch.einsum("its,isd->itd", p, v) + torch.einsum("its,tsd->itd", p, ev[idx])
    assert A.rel_l2(A.softmax_attention_ref(q, k, v, 0.3, rel=(ek, ev, R, off)), want) < 1e-14
    q2 = torch.randn(items, T, D, generator=g, dtype=torch.float64)
    sim = (torch.einsum("itd,isd->its", q2, k) * 0.3).masked_fill(torch.arange(T)[None, :] > torch.arange(T)[:, None], -math.inf)
    want = torch.einsum("its,isd->itd", sim.softmax(dim=-1), v)
    got = A.softmax_attention_ref(q2, k, v, 0.3, causal=True)
    assert A.rel_l2(got, want) < 1e-14
    assert torch.equal(got[:, 0], v[:, 0])


def test_schedule_on_randn_never_rescales():
    """The gap these inputs close: on randn inputs no running maximum advances after the first tile, so both mutants are invisible."""
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(4, 300, 64, generator=g).half().double() for _ in range(3))
    lg2 = A.logits(q, k, 0.125) * A.LOG2E
    s = A.stale_max_schedule(lg2, v, 64)
    assert s["late"] == 0
    assert torch.equal(s["out"], A.stale_max_schedule(lg2, v, 64, skip="o")["out"])
