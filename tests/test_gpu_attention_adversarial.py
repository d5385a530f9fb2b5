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
from harness import run_both
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd.program import Program, Ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
F16 = torch.float16


def _padded(P, rows, cols, pad):
    """rows x cols fp16 with `pad` rows that no item owns on either side: (whole allocation, the window)."""
    big = P.alloc(rows + 2 * pad, cols, "f16")
    return big, big.row_slice(pad, pad + rows)


def _items_view(it, ref, dims, strides, D):
    """[b_outer, b_inner, heads, n, D] view of the arena at `ref` with (sequence, outer, inner) element strides."""
    bo, bi, heads, n = dims
    return it.view(ref, (bo, bi, heads, n, D), (strides[1], strides[2], D, strides[0], 1), F16, {})


def _nan_fill(it, big):
    it.mat(big.ref, big.rows, big.ld, big.ld, F16, {}).fill_(NAN)


def _spare_keys(it, big, win, k_col0, heads, D, spare_k):
    """The spike of the masked set in the K columns of the spare rows that follow the last item."""
    pad = (big.rows - win.rows) // 2
    tail = big.row_slice(big.rows - pad, big.rows)
    it.mat(tail.ref.shifted(2 * k_col0), pad, heads * D, big.ld, F16, {}).view(pad, heads, D).copy_(spare_k.half())


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
    D, B, F, heads, nq, nk = c["D"], c["B"], c["F"], c["heads"], c["nq"], c["nk"]
    inner, lay, lo = heads * D, c["layout"], c["lo"]
    P = Program()
    if lay == "cross":
        pad = 64
        qbig, qb = _padded(P, B * F * nq, inner, pad)
        kvbig, kv = _padded(P, B * nk, 2 * inner + 8, pad)
        q_ref, k_ref, v_ref, k_col0 = qb.ref, kv.col_slice(8, 8 + inner).ref, kv.col_slice(8 + inner, 8 + 2 * inner).ref, 8
        q_str, kv_str = (inner, F * nq * inner, nq * inner), (kv.ld, nk * kv.ld, 0)
        o_rows, o_unit = B * F * nq, (1, F * nq, nq)
        bigs = [qbig, kvbig]
    else:
        assert nq == nk and (lay == "temporal" or F == 1)
        px = F if lay == "temporal" else 1                 # rows per sequence step
        pad = 64 * px
        kvbig, kv = _padded(P, B * nq * px, 3 * inner, pad)
        ld = kv.ld
        q_ref, k_ref, v_ref, k_col0 = kv.ref, kv.col_slice(inner, 2 * inner).ref, kv.col_slice(2 * inner, 3 * inner).ref, inner
        q_str = kv_str = (px * ld, nq * px * ld, ld if lay == "temporal" else 0)
        o_rows, o_unit = B * nq * px, (px, nq * px, 1 if lay == "temporal" else 0)
        bigs = [kvbig]
    obig, o = _padded(P, o_rows, 2 * inner if lo else inner, pad)
    o_str = tuple(u * o.ld for u in o_unit)
    vt = P.alloc(B * F * heads * 64, -(-nk // 64) * 64, "f16") if attn2 else None
    op = P.attention("a", q_ref, k_ref, v_ref, o.ref, nq=nq, nk=nk, heads=heads, b_outer=B, b_inner=F, q_strides=q_str, kv_strides=kv_str,
                     o_strides=o_str, scale=x["scale"], head_dim=D, causal=c["causal"], lo_off=inner if lo else 0, vt_scratch=vt,
                     waves=c["waves"] if attn2 else 0)
    # the op record names the kernel the case is about
    assert op.kind == L.OP_ATTENTION and op.i[14] == D and op.i[15] == int(c["causal"]) and op.i[16] == (inner if lo else 0)
    if attn2:
        assert op.p[6].space != "null" and op.i[17] == -(-nk // 64) * 64 and op.i[18] == c["waves"]
    else:
        assert op.p[6].space == "null"
    kv_dims = (B, 1, heads, nk) if lay == "cross" else (B, F, heads, nk)

    def init(it):
        for b in bigs + [obig]:
            _nan_fill(it, b)
        if lay == "cross":
            _items_view(it, q_ref, (B, F, heads, nq), q_str, D).copy_(x["q"].view(B, heads, F, nq, D).permute(0, 2, 1, 3, 4).half())
        else:
            _items_view(it, q_ref, (B, F, heads, nq), q_str, D).copy_(x["q"].view(B, F, heads, nq, D).half())
        _items_view(it, k_ref, kv_dims, kv_str, D).copy_(x["k"].view(*kv_dims, D).half())
        _items_view(it, v_ref, kv_dims, kv_str, D).copy_(x["v"].view(*kv_dims, D).half())
        if x["spare_k"] is not None and not c["causal"]:
            _spare_keys(it, kvbig, kv, k_col0, heads, D, x["spare_k"])
    _, got, _, _ = run_both(P, {}, {}, init)

    def out(ref_):
        t = _items_view(got, ref_, (B, F, heads, nq), o_str, D).float()
        return (t.permute(0, 2, 1, 3, 4).reshape(B * heads, F * nq, D) if lay == "cross" else t.reshape(B * F * heads, nq, D)).clone()
    hi = out(o.ref)
    low = out(o.ref.shifted(2 * inner)) if lo else None
    allo = got.mat(obig.ref, obig.rows, obig.ld, obig.ld, F16, {})
    pads = torch.cat([allo[:pad], allo[pad + o_rows:]]).clone()
    return hi, low, pads


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
    D, T, Tq, off, R, lo, hw, b, heads = (c[n] for n in ("D", "T", "Tq", "off", "R", "lo", "hw", "b", "heads"))
    inner = heads * D
    ek, ev = x["ek"].float(), x["ev"].float()
    w = {"ek": ek, "ev": ev, "ekL": pk.relpos_table_long(ek, False), "evL": pk.relpos_table_long(ev, True)}
    extra = dict(rel_k_long=Ref("weight", 0, "ekL"), rel_vT_long=Ref("weight", 0, "evL"))
    if sel == 2:
        w["ek16"], w["ev16"] = pk.relpos_table16(ek, T, False), pk.relpos_table16(ev, T, True)
        extra.update(rel_k16=Ref("weight", 0, "ek16"), rel_vT16=Ref("weight", 0, "ev16"))
    pad = 32 * hw
    P = Program()
    qbig, q = _padded(P, b * Tq * hw, inner, pad)
    kvbig, kv = _padded(P, b * T * hw, 2 * inner, pad)
    obig, o = _padded(P, b * Tq * hw, 2 * inner if lo else inner, pad)
    q_str, kv_str, o_str = (hw * inner, Tq * hw * inner, inner), (hw * kv.ld, T * hw * kv.ld, kv.ld), (hw * o.ld, Tq * hw * o.ld, o.ld)
    op = P.attention("a", q.ref, kv.col_slice(0, inner).ref, kv.col_slice(inner, 2 * inner).ref, o.ref, nq=Tq, nk=T, heads=heads,
                     b_outer=b, b_inner=hw, q_strides=q_str, kv_strides=kv_str, o_strides=o_str, scale=x["scale"], head_dim=D,
                     rel_k=Ref("weight", 0, "ek"), rel_v=Ref("weight", 0, "ev"), max_rel=R, q_offset=off, relpos_mfma=sel,
                     lo_off=inner if lo else 0, **extra)
    want = 3 if T > 32 else sel
    assert op.kind == L.OP_RELPOS_ATTN and op.i[17] == want and op.i[16] == off and op.i[15] == R and op.i[18] == (inner if lo else 0)
    assert (op.p[6].space != "null") == (want in (2, 3))

    def init(it):
        for big in (qbig, kvbig, obig):
            _nan_fill(it, big)
        _items_view(it, q.ref, (b, hw, heads, Tq), q_str, D).copy_(x["q"].view(b, hw, heads, Tq, D).half())
        _items_view(it, kv.ref, (b, hw, heads, T), kv_str, D).copy_(x["k"].view(b, hw, heads, T, D).half())
        _items_view(it, kv.ref.shifted(2 * inner), (b, hw, heads, T), kv_str, D).copy_(x["v"].view(b, hw, heads, T, D).half())
        if x["spare_k"] is not None:
            _spare_keys(it, kvbig, kv, 0, heads, D, x["spare_k"])
    _, got, _, _ = run_both(P, w, {}, init)
    out = lambda r: _items_view(got, r, (b, hw, heads, Tq), o_str, D).float().reshape(b * hw * heads, Tq, D).clone()
    allo = got.mat(obig.ref, obig.rows, obig.ld, obig.ld, F16, {})
    pads = torch.cat([allo[:pad], allo[pad + o.rows:]]).clone()
    return out(o.ref), (out(o.ref.shifted(2 * inner)) if lo else None), pads


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
