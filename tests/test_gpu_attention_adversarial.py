"""GPU (-m gpu): every streaming-softmax attention kernel of csrc/attention.hip on peaked and late-maximum inputs.

attn_kernel, attn2_kernel and relpos_long_kernel advance their running maximum only when a key tile's maximum exceeds it by more than 2^8
and then multiply O, l (and w_lo / w_hi) by alpha = exp2(m_run - m_tile).  On randn inputs that never happens after the first tile, so the
other attention tests cannot see a wrong rescale.  The inputs here (tests/adversarial.py; tests/test_adversarial_inputs_cpu.py proves on
the CPU what they do) make it happen on 15 - 65 % of the rows, in every tile position, for part of a 32-query block at a time, on non-zero
edge masses, and put a logit 40 log2 units up behind every mask (causal, keys past nk: the next item's first key and spare rows).

`harness.run_both` only executes; the expected values are `adversarial.softmax_attention_ref` (float64, explicit formula), never the
interpreter.  Outputs are NaN-filled first and must come back finite; the rows allocated around Q / K / V / O that no item owns are NaN
(spare K rows behind the last item carry the spike in the masked set) and the ones around O must still be NaN afterwards.
Tolerances are the suite's own for these kernels against an explicit reference on randn inputs: 2e-3 for the fp16 output, 1e-3 for hi + lo,
with hi + lo closer than hi.  Measured values: profiles/attention_adversarial.txt.

Not here: the fused QKV + temporal-attention GEMM record, the fused to_q + text cross-attention record and the second role of
T2V_OP_ATTENTION — tests/test_gpu_fused_attention_adversarial.py (the logits are placed through the GEMMs with selection weights)."""
import pytest
import torch

import adversarial as A
import attention_records as R
from harness import run_both
from sd_webui_text2video_amd import _lib as L

pytestmark = pytest.mark.gpu


def _check(tag, hi, low, ref, pads):
    """hi / low / ref in item order [items, nq, D]; pads: the spare rows around the output."""
    assert torch.isfinite(hi).all(), tag
    assert torch.isnan(pads).all(), f"{tag}: rows around the output written"
    r = A.rel_l2(hi, ref)
    r2 = None
    if low is not None:
        assert torch.isfinite(low).all(), tag
        r2 = A.rel_l2(hi.double() + low.double(), ref)
    print(f"ADV {tag}: hi {r:.2e}" + (f" hi+lo {r2:.2e}" if r2 is not None else ""))
    assert r < A.TOL_HI, (tag, r)
    if r2 is not None:
        assert r2 < r and r2 < A.TOL_HILO, (tag, r, r2)
    return r


# ---- attn_kernel / attn2_kernel --------------------------------------------------------------------------------------------------------
def _run_attn(c, x, attn2):
    b = R.build_attn(c, attn2)
    _, got, _, _ = run_both(b.P, b.w, {}, lambda it: b.init(it, x))
    return b.read(got)


@pytest.mark.parametrize("c", A.ATTN_CASES, ids=lambda c: c["id"])
def test_attention_kernels_on_late_maximum_and_masked_spike_inputs(c):
    x = A.attn_inputs(c)
    ref = A.softmax_attention_ref(x["q"], x["k"], x["v"], x["scale"], c["causal"])
    hi, low, pads = _run_attn(c, x, c["attn2"])
    _check(c["id"], hi, low, ref, pads)
    if c["attn2"]:
        # same scores in the same order: attn_kernel gives the same bits — now with the rescale path live in both
        hi1, low1, pads1 = _run_attn(c, x, False)
        _check(c["id"] + " (attn_kernel)", hi1, low1, ref, pads1)
        assert torch.equal(hi, hi1) and (low is None or torch.equal(low, low1)), "attn2_kernel and attn_kernel must give the same bits"
    if c["variant"] == "masked" and not c["causal"]:
        # an item whose key 0 carries the spike sees it.  Where key 0 stands >= 30 log2 units above the row's other logits (float64; the
        # query's own noise along the spike moves the 40 by +- 10) every other probability is below 2^-25, zero in the fp16 P operand, and
        # l = 1 + nk 2^-30: the output row is v[0], bit for bit
        spiked = [it for it, s in enumerate(x["keys"]) if s == 0]
        assert spiked
        exact = 0
        for it in spiked:
            lg2 = A.logits(x["q"][it:it + 1], x["k"][it:it + 1], x["scale"])[0] * A.LOG2E
            rows = (lg2[:, 0] - lg2[:, 1:].max(dim=1).values) >= 30.0
            exact += int(rows.sum())
            assert torch.equal(hi[it][rows], x["v"][it, 0].float().expand_as(hi[it])[rows]), (c["id"], it)
        assert exact >= 0.25 * len(spiked) * hi.shape[1], (c["id"], exact)
    if c["causal"]:
        assert torch.equal(hi[:, 0], x["v"][:, 0].float())            # row 0 attends to key 0 only


# ---- relative-position temporal attention -----------------------------------------------------------------------------------------------
def _run_relpos(c, x, sel):
    b = R.build_relpos(c, sel, (x["ek"], x["ev"]))
    _, got, _, _ = run_both(b.P, b.w, {}, lambda it: b.init(it, x))
    return b.read(got)


@pytest.mark.parametrize("c", A.RELPOS_LONG_CASES, ids=lambda c: c["id"])
def test_long_clip_relpos_kernel_on_late_maximum_and_masked_spike_inputs(c):
    """relpos_long_kernel: advances of the running maximum on non-zero w_lo / w_hi (whole clips), on w_lo only (a slice at the end of the
    clip), for part of a 32-query block; T = 1024 is T2V_RELPOS_MAX_FRAMES, the documented bound."""
    assert c["T"] <= L.RELPOS_MAX_FRAMES
    x = A.relpos_inputs(c)
    ref = A.softmax_attention_ref(x["q"], x["k"], x["v"], x["scale"], rel=(x["ek"], x["ev"], c["R"], c["off"]))
    hi, low, pads = _run_relpos(c, x, None)
    _check(c["id"], hi, low, ref, pads)


@pytest.mark.parametrize("c", A.RELPOS_SHORT_CASES, ids=lambda c: c["id"])
def test_relpos_kernels_up_to_32_frames_on_peaked_inputs(c):
    """The VALU kernel (0), the round-3 MFMA kernel (1), the persistent MFMA kernel (2) and the forced long-clip kernel (3) on the same
    inputs: each against the formula, and against each other to the same tolerance.  One key tile: the range of 2^x and the masks."""
    x = A.relpos_inputs(c)
    ref = A.softmax_attention_ref(x["q"], x["k"], x["v"], x["scale"], rel=(x["ek"], x["ev"], c["R"], c["off"]))
    outs = {}
    for sel in c["sels"]:
        hi, low, pads = _run_relpos(c, x, sel)
        _check(f"{c['id']} i[17]={sel}", hi, low, ref, pads)
        outs[sel] = hi
    sels = list(outs)
    for n, a in enumerate(sels):
        for bsel in sels[n + 1:]:
            r = A.rel_l2(outs[a], outs[bsel])
            print(f"ADV {c['id']} i[17]={a} vs {bsel}: {r:.2e}")
            assert r < A.TOL_HI, (a, bsel, r)
