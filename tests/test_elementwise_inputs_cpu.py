"""CPU: the adversarial elementwise inputs of tests/elementwise_inputs.py do what tests/test_gpu_elementwise_adversarial.py needs them to
do, and every case is right in layout and fencing before it meets a GPU.

For EVERY case the GPU file runs (the list is imported from tests/elementwise_inputs.py by both), on the inputs and the float64 reference
alone:
  * the inputs are finite (except the one NaN pixel a depth case carries) and representable in their dtype;
  * the reference rounded to the output format passes the case's own checks with room to spare — the tolerance is not spent on the format;
  * each mutation of the reference (the list per op is in the builders' `mutations`) pushes EVERY affected segment above 10 x the bound
    the GPU file applies to it; for the bit-exact checks it changes at least one element of every affected segment.  Segments a mutation
    cannot reach (a guided-channel bug on an unguided channel, a frequency slip at t = 0) are named by the builder and left out.
    One mutation one would list for to_uint8 is provably none: clamping tensor2vid after the multiplication by 255 gives the same bytes for every
    input (s <= 1 <=> 255 s <= 255, and both clamps return exactly 0 / 255 outside), so no test can expose it; this file asserts that.
    "The maximum taken over the first 768 columns only" overflows: exp(l - max) reaches 2^30 at the true maximum, beyond fp16.
Then the case runs through the interpreter ALONE (programs through Interp / AdapterInterp, the sampler ops as single records on fenced
tensors) and `elementwise_inputs.verify` applies the GPU file's own checks: outputs finite, every fence element untouched, exact checks
bit-equal, per-segment errors within the GPU bounds.  That also tests the interpreter's restatement of these ops against the independent
reference."""
import pytest
import torch

import elementwise_inputs as E
from interp import Interp
from interp_adapter import AdapterInterp
from sd_webui_text2video_amd.program import Program


def run_in_interpreter(b):
    if b.ops is not None:                       # a sampler binding: its record(s) on views into the fenced tensors
        it = Interp(Program(), {}, poison=False)
        it.run(b.ext_views(), ops=b.ops)
        return it
    it = (AdapterInterp if b.adapter else Interp)(b.P, b.w, poison=False)
    b.init(it)
    it.run({})
    return it


@pytest.mark.parametrize("c", E.CASES, ids=lambda c: c["id"])
def test_inputs_expose_the_mutations_and_the_case_passes_in_the_interpreter(c):
    b = E.build(c)
    assert b.checks
    for win, t in b.sets:
        if win.dtype != "u8":
            assert torch.equal(torch.nan_to_num(t.double(), nan=0.5), torch.nan_to_num(t.to(E.TD[win.dtype]).double(), nan=0.5)), "inputs must be representable"
            assert bool(torch.isfinite(t).all()) or c["family"] == "depth"
    by_name = {chk["name"]: chk for chk in b.checks}
    muts = b.mutations()
    assert muts or c["family"] == "softmax" and c["cols"] <= 768 or c["family"] == "lincomb" and len(c["terms"]) == 1, "no mutation reaches this case"
    for what, outs, affected in muts:
        assert outs
        for name, got in outs.items():
            chk = by_name[name]
            r = b.ratios(chk, got)
            aff = affected[name]
            aff = torch.ones_like(r, dtype=torch.bool) if aff is None else aff.reshape(-1)
            assert aff.shape == r.shape and bool(aff.any()), (c["id"], what, name, aff.shape, r.shape)
            worst = float(r[aff].min())
            print(f"ELTMUT {c['id']}: {what}: {name}: " + ("changes every affected segment" if chk["exact"] and worst > 0 else f"least affected segment {worst:.3g} x bound"))
            assert worst > (0.0 if chk["exact"] else 10.0), (c["id"], what, name, "an affected segment stays within 10 x the bound", worst)
    for chk in b.checks:                        # the reference rounded once to the output format stays within the case's own bounds
        if chk["ref"] is not None:
            r = b.ratios(chk, chk["ref"].to(E.TD[chk["dt"]]))
            assert float(r.max()) <= 1.0, (c["id"], chk["name"], "the rounded reference misses the bound", float(r.max()))
    it = run_in_interpreter(b)
    print(E.figures_line(b, E.verify(it, b)))


def test_the_inputs_are_what_the_docstring_says():
    # neighbouring segments differ by >= 2 x along every index
    i = torch.arange(9)
    s = E.seg_scale(i.view(9, 1, 1), i.view(1, 9, 1), i.view(1, 1, 9))
    for d in range(3):
        ratio = s / s.roll(1, d)
        inner = ratio.narrow(d, 1, 8)
        assert bool(((inner >= 2) | (inner <= 0.5)).all())
    assert set(s.log2().flatten().tolist()) == set(range(-3, 4))
    X = E.layout_input(3, 4, 5, 37, 1)
    mag = X.abs()
    assert bool((mag / E.seg_scale(torch.arange(4).view(1, 4, 1, 1), torch.arange(5).view(1, 1, 5, 1), torch.arange(3).view(3, 1, 1, 1)) >= 0.75).all())
    assert bool((X > 0).any(dim=-1).all()) and bool((X < 0).any(dim=-1).all())                  # every line carries both signs
    # copy2d: magnitudes 2^-10 .. 64 and 80, sign by row, |x| <= 80
    C = E.copy_input(37, 132, "f16", 3)
    assert float(C.abs().max()) <= 80 and bool((C[0::2] > 0).all()) and bool((C[1::2] < 0).all())
    assert float(C[0].abs().max()) <= 2.0 ** -10 and float(C[17].abs().min()) >= 40
    # softmax: the designed maximum, the spread, the constant row
    Xs, where = E.softmax_input(5, 1000, 2)
    for r, pos in enumerate(where):
        if pos >= 0:
            live = Xs[r, 768:] if pos >= 768 else Xs[r]
            assert int(Xs[r].argmax()) == pos and float(live.max() - live.min()) * E.SOFTMAX_SCALE <= 30.0 * 0.6932
            assert pos < 768 or float(Xs[r, :768].max()) * E.SOFTMAX_SCALE < -128 * 0.6932
        else:
            assert Xs[r].unique().numel() == 1
    assert any(w >= 768 for w in where) and 0 in where and 999 in where
    # wrap cases reach the second pass of a grid capped at 8192 workgroups
    units = dict(ncthw=lambda c: c["B"] * c["F"] * c["HW"], cl=lambda c: c["B"] * c["C"] * c["F"] * c["HW"], copy=lambda c: c["rows"] * c["cols"] // 4,
                 ddim=lambda c: c["S"] * c["Cs"] * c["inner"], lincomb=lambda c: c["n"], u8=lambda c: c["shape"][0] * c["shape"][2] * c["shape"][3] * c["shape"][4],
                 pool=lambda c: c["n"] * (c["H"] // 2) * (c["W"] // 2) * (c["C"] // 4))
    wraps = [c for c in E.CASES if c.get("wrap")]
    assert {c["family"] for c in wraps} == set(units)
    for c in wraps:
        n = units[c["family"]](c)
        assert E.GRID_UNITS < n < 2 * E.GRID_UNITS and n % 256 != 0, (c["id"], n)


def test_the_uint8_table_sits_on_every_truncation_boundary():
    """Every byte value occurs in the expected output of every to_uint8 case — so each boundary k - 1 | k has inputs on either side — and
    for the fp32 kernels most boundaries are straddled WITHIN the five neighbours (+-2 ulp) of 2 k / 255 - 1.  The written-out formula
    equals the oracle's function, and clamping after the multiplication by 255 changes no byte."""
    for c in (c for c in E.CASES if c["family"] == "u8" and not c.get("wrap")):
        b = E.build(c)
        want, vid = b.u8["want"], b.u8["video"]
        assert set(want.unique().tolist()) == set(range(256)), c["id"]
        assert torch.equal(E.u8_formula(vid, c["half"], c["bgr"]), want)
        assert torch.equal(E.u8_formula(vid, c["half"], c["bgr"], "clamp_after"), want)
    tab = E.boundary_table("f32")[: 256 * 5].float().view(256, 5)
    byte = torch.floor((tab * 0.5 + 0.5).clamp(0, 1) * 255)
    straddled = int(((byte.amin(dim=1) < byte.amax(dim=1))[1:]).sum())
    print(f"fp32 boundaries straddled within +-2 ulp: {straddled} of 255")
    assert straddled >= 128
    assert bool(torch.isfinite(E.boundary_table("f16")).all()) and bool(torch.isfinite(E.boundary_table("f32")).all())


def test_the_depth_frames_are_what_the_cases_say():
    for c in (c for c in E.CASES if c["family"] == "depth"):
        b = E.build(c)
        D, hw = b.depth["D"], c["H"] * c["W"]
        for k, kind in enumerate(c["frames"]):
            if kind == "const":
                assert D[k].unique().numel() == 1
            elif kind == "nan":
                assert int(torch.isnan(D[k]).sum()) == 1
            else:
                lo, hi, pmin, pmax = kind
                assert int(D[k].argmin()) == pmin % hw and int(D[k].argmax()) == pmax % hw and float(D[k].min()) == lo and float(D[k].max()) == hi
                assert int((D[k] == lo).sum()) == 1 and int((D[k] == hi).sum()) == 1
