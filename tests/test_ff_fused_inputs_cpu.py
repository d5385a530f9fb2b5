"""CPU: what the inputs of tests/test_gpu_ff_fused.py (tests/ff_fused_inputs.py) can and cannot see.

The GPU test asserts (a) bit-identity of the fused launch with the two-launch form and (b) the suite's fp16-output bound, 1e-3 per row
segment, against the float64 reference that rounds the hidden tensor to fp16.  Here every way the fused kernel's chunk walk can go wrong is
applied to the float64 emulation and must land far outside that bound on these very inputs:
  dropped chunk      chunk j of the hidden tensor never reaches the projection (first, a middle one, the last);
  repeated chunk     the projection of chunk j + 1 runs on chunk j's hidden values;
  swapped halves     value and gate of a chunk change places;
each must miss 1e-3 by at least 10 x in its worst segment (they miss it by orders of magnitude).
The fourth mutation, a hidden tensor that is NOT rounded to fp16, moves every product by less than 2^-11 — the size of the fp16 output's own
rounding — and stays inside any fp16-output bound by construction (measured here: it is asserted to stay BELOW 1e-3, so that nobody
mistakes (b) for a check of the rounding point).  It is visible where the output keeps fp32 precision: on the hi + lo cases it must miss
the suite's fp32-class bound max(2e-5, 4 e_torch) by at least 10 x, and it must change stored bits — which is how the GPU test catches it:
assertion (a) compares with the two-launch form, which rounds.
Also: the unmutated float64 reference rounded to the stored images is inside both bounds (the bounds are reachable), every segment has
a non-zero reference norm, the hidden tensor is far inside fp16, the programs name the records the recognition wants, and the case list
covers every tile count, bias, residual and output form the kernel has."""
import pytest
import torch

import ff_fused_inputs as FF
import gemm_inputs as G

MUTATIONS = [("drop", 0), ("drop", 7), ("drop", FF.NCHUNK - 1), ("repeat", 0), ("repeat", 11), ("swap", 0), ("swap", 13), ("swap", FF.NCHUNK - 1)]


def _worst(got, ref):
    return float(G.seg_err(got, ref).max())


@pytest.mark.parametrize("c", FF.CASES, ids=lambda c: c["id"])
def test_reference_is_reachable_and_every_segment_counts(c):
    d, hid, ref = FF.inputs_of(c)
    assert bool((G.seg_norms(ref) > 0).all())
    assert float(hid.abs().max()) < 16384, "the hidden tensor must stay far inside fp16"
    assert float(hid.abs().max()) > 1.0
    hi, lo = FF.hi_lo(ref)
    e = _worst(hi, ref)
    print(f"FFIN {c['id']}: float64 reference stored as fp16: worst segment {e:.3e} (bound {FF.TOL_F16:.0e}); |hidden| max {float(hid.abs().max()):.1f}")
    assert e <= FF.TOL_F16
    e2 = _worst(hi.double() + lo.double(), ref)
    assert e2 <= FF.TOL_F32, e2


@pytest.mark.parametrize("c", FF.CASES, ids=lambda c: c["id"])
def test_chunk_mutations_miss_the_bound_by_orders_of_magnitude(c):
    d, _, ref = FF.inputs_of(c)
    for mut in MUTATIONS:
        _, out = FF.reference(d, mutation=mut)
        hi, _ = FF.hi_lo(out)
        e = _worst(hi, ref)
        print(f"FFIN {c['id']}: {mut}: worst segment {e:.3e} = {e / FF.TOL_F16:.0f} x the bound")
        assert e >= 10 * FF.TOL_F16, (c["id"], mut, e)


@pytest.mark.parametrize("c", FF.CASES, ids=lambda c: c["id"])
def test_unrounded_hidden_tensor_is_seen_by_the_bits_and_the_hi_lo_bound_only(c):
    d, _, ref = FF.inputs_of(c)
    _, out = FF.reference(d, mutation=("unrounded",))
    hi, lo = FF.hi_lo(out)
    rhi, rlo = FF.hi_lo(ref)
    e = _worst(hi, ref)
    changed = float((hi.view(torch.int16) != rhi.view(torch.int16)).float().mean())
    print(f"FFIN {c['id']}: unrounded hidden: fp16 output worst segment {e:.3e} (inside 1e-3 by construction); {100 * changed:.1f} % of the stored hi values differ")
    assert e < FF.TOL_F16, "an fp16-output bound was expected NOT to see the rounding point; if it does, tighten the docstring, not the bound"
    assert changed > 0.05, "the mutation must change stored bits: assertion (a) of the GPU test is what catches it"
    if c["out_lo"]:
        _, t32 = FF.reference(d, dtype=torch.float32)
        e_torch = G.seg_err(t32, ref)
        bound = torch.maximum(torch.full_like(e_torch, FF.TOL_F32), 4.0 * e_torch)
        e2 = G.seg_err(hi.double() + lo.double(), ref)
        ratio = float((e2 / bound).max())
        print(f"FFIN {c['id']}: unrounded hidden: hi + lo worst segment {float(e2.max()):.3e}, {ratio:.1f} x its fp32-class bound")
        assert ratio >= 10.0, (c["id"], ratio)
        assert float((lo.view(torch.int16) != rlo.view(torch.int16)).float().mean()) > 0.5


def test_case_list_covers_what_the_fused_kernel_can_get_wrong():
    Ms = {c["M"] for c in FF.CASES}
    assert Ms == {192, 200, 576}, "one tile, a ragged second tile, three tiles"
    for key in ("bias1", "bias2", "res", "wrap", "out_lo"):
        assert {c[key] for c in FF.CASES} == {True, False}, key
    v, g, cs = FF.chunk_scales()
    # neighbouring chunks never share all three scales, and value / gate of a chunk never weigh the same as its neighbour's
    trip = [(float(v[j]), float(g[j]), float(cs[j])) for j in range(FF.NCHUNK)]
    assert len(set(trip)) == FF.NCHUNK, "every chunk has its own (value, gate, projection) scales"


@pytest.mark.parametrize("c", [FF.CASES[0], FF.CASES[3]], ids=lambda c: c["id"])
def test_programs_name_the_records_the_recognition_wants(c):
    from sd_webui_text2video_amd import _lib as L
    b = FF.build(c)
    ge, pr = b.ops("adjacent")
    assert ge.i[31] == 1 and ge.kind == L.OP_GEMM and pr.kind == L.OP_GEMM and pr.p[0] == ge.p[5]
    assert [o.kind for o in b.ops("separated")] == [L.OP_GEMM, L.OP_MEMSET, L.OP_GEMM]
    assert b.ops("third-reader")[2].p[0] == ge.p[5]
    assert FF.build(c, waive_cutoff=False).ops("adjacent")[0].i[31] == 0
    if not c["wrap"]:
        assert FF.build(c, split_k=True).ops("adjacent")[1].i[19] == 2
