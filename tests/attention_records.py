"""TEST INFRASTRUCTURE — the programs of the attention cases of tests/adversarial.py (ATTN_CASES, RELPOS_LONG_CASES, RELPOS_SHORT_CASES):
the record of every case, its padded buffers, how the inputs are laid out in them and how the outputs are read back.  No test functions
here.  tests/test_gpu_attention_adversarial.py runs these programs on the GPU; tests/test_record_paths_cpu.py keys their records on the
CPU — both import `build_attn` / `build_relpos`, so they cannot drift apart.  (tests/adversarial.py itself imports nothing of the
product; this module does.)  Building a program needs no inputs: `init(it, x)` takes them (adversarial.attn_inputs / relpos_inputs)."""
from __future__ import annotations

import torch

from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd.program import Program, Ref

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


class BuiltAttn:
    """P: the program (one record, `op`); w: its weights; init(it, x): fills the arena from the case's inputs; read(got) -> (hi, low, pads):
    the outputs in item order [items, nq, D], the low-order image or None, and the spare rows around the output."""
    P = op = w = init = read = None


def scale_of(c):
    return c["D"] ** -0.5          # adversarial.attn_inputs / relpos_inputs


# ---- attn_kernel / attn2_kernel --------------------------------------------------------------------------------------------------------
def build_attn(c, attn2):
    D, B, F, heads, nq, nk = c["D"], c["B"], c["F"], c["heads"], c["nq"], c["nk"]
    inner, lay, lo = heads * D, c["layout"], c["lo"]
    b = BuiltAttn()
    P = b.P = Program()
    b.w = {}
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
    op = b.op = P.attention("a", q_ref, k_ref, v_ref, o.ref, nq=nq, nk=nk, heads=heads, b_outer=B, b_inner=F, q_strides=q_str, kv_strides=kv_str,
                            o_strides=o_str, scale=scale_of(c), head_dim=D, causal=c["causal"], lo_off=inner if lo else 0, vt_scratch=vt,
                            waves=c["waves"] if attn2 else 0)
    # the op record names the kernel the case is about
    assert op.kind == L.OP_ATTENTION and op.i[14] == D and op.i[15] == int(c["causal"]) and op.i[16] == (inner if lo else 0)
    if attn2:
        assert op.p[6].space != "null" and op.i[17] == -(-nk // 64) * 64 and op.i[18] == c["waves"]
    else:
        assert op.p[6].space == "null"
    kv_dims = (B, 1, heads, nk) if lay == "cross" else (B, F, heads, nk)

    def init(it, x):
        assert x["scale"] == scale_of(c)
        for big in bigs + [obig]:
            _nan_fill(it, big)
        if lay == "cross":
            _items_view(it, q_ref, (B, F, heads, nq), q_str, D).copy_(x["q"].view(B, heads, F, nq, D).permute(0, 2, 1, 3, 4).half())
        else:
            _items_view(it, q_ref, (B, F, heads, nq), q_str, D).copy_(x["q"].view(B, F, heads, nq, D).half())
        _items_view(it, k_ref, kv_dims, kv_str, D).copy_(x["k"].view(*kv_dims, D).half())
        _items_view(it, v_ref, kv_dims, kv_str, D).copy_(x["v"].view(*kv_dims, D).half())
        if x["spare_k"] is not None and not c["causal"]:
            _spare_keys(it, kvbig, kv, k_col0, heads, D, x["spare_k"])

    def read(got):
        def out(ref_):
            t = _items_view(got, ref_, (B, F, heads, nq), o_str, D).float()
            return (t.permute(0, 2, 1, 3, 4).reshape(B * heads, F * nq, D) if lay == "cross" else t.reshape(B * F * heads, nq, D)).clone()
        hi = out(o.ref)
        low = out(o.ref.shifted(2 * inner)) if lo else None
        allo = got.mat(obig.ref, obig.rows, obig.ld, obig.ld, F16, {})
        pads = torch.cat([allo[:pad], allo[pad + o_rows:]]).clone()
        return hi, low, pads
    b.init, b.read = init, read
    return b


# ---- relative-position temporal attention -----------------------------------------------------------------------------------------------
def build_relpos(c, sel, tables=None):
    """sel: the selector asked for (None: the lowering's default).  tables = (ek, ev) float64 [2R+1, D] (adversarial.rel_tables); None: zeros
    of the right shape (the record does not depend on the values)."""
    D, T, Tq, off, R, lo, hw, nb, heads = (c[n] for n in ("D", "T", "Tq", "off", "R", "lo", "hw", "b", "heads"))
    inner = heads * D
    ek, ev = (torch.zeros(2 * R + 1, D), torch.zeros(2 * R + 1, D)) if tables is None else (tables[0].float(), tables[1].float())
    b = BuiltAttn()
    w = b.w = {"ek": ek, "ev": ev, "ekL": pk.relpos_table_long(ek, False), "evL": pk.relpos_table_long(ev, True)}
    extra = dict(rel_k_long=Ref("weight", 0, "ekL"), rel_vT_long=Ref("weight", 0, "evL"))
    if sel == 2:
        w["ek16"], w["ev16"] = pk.relpos_table16(ek, T, False), pk.relpos_table16(ev, T, True)
        extra.update(rel_k16=Ref("weight", 0, "ek16"), rel_vT16=Ref("weight", 0, "ev16"))
    pad = 32 * hw
    P = b.P = Program()
    qbig, q = _padded(P, nb * Tq * hw, inner, pad)
    kvbig, kv = _padded(P, nb * T * hw, 2 * inner, pad)
    obig, o = _padded(P, nb * Tq * hw, 2 * inner if lo else inner, pad)
    q_str, kv_str, o_str = (hw * inner, Tq * hw * inner, inner), (hw * kv.ld, T * hw * kv.ld, kv.ld), (hw * o.ld, Tq * hw * o.ld, o.ld)
    op = b.op = P.attention("a", q.ref, kv.col_slice(0, inner).ref, kv.col_slice(inner, 2 * inner).ref, o.ref, nq=Tq, nk=T, heads=heads,
                            b_outer=nb, b_inner=hw, q_strides=q_str, kv_strides=kv_str, o_strides=o_str, scale=scale_of(c), head_dim=D,
                            rel_k=Ref("weight", 0, "ek"), rel_v=Ref("weight", 0, "ev"), max_rel=R, q_offset=off, relpos_mfma=sel,
                            lo_off=inner if lo else 0, **extra)
    want = 3 if T > 32 else sel
    assert op.kind == L.OP_RELPOS_ATTN and op.i[17] == want and op.i[16] == off and op.i[15] == R and op.i[18] == (inner if lo else 0)
    assert (op.p[6].space != "null") == (want in (2, 3))

    def init(it, x):
        assert x["scale"] == scale_of(c)
        for big in (qbig, kvbig, obig):
            _nan_fill(it, big)
        _items_view(it, q.ref, (nb, hw, heads, Tq), q_str, D).copy_(x["q"].view(nb, hw, heads, Tq, D).half())
        _items_view(it, kv.ref, (nb, hw, heads, T), kv_str, D).copy_(x["k"].view(nb, hw, heads, T, D).half())
        _items_view(it, kv.ref.shifted(2 * inner), (nb, hw, heads, T), kv_str, D).copy_(x["v"].view(nb, hw, heads, T, D).half())
        if x["spare_k"] is not None:
            _spare_keys(it, kvbig, kv, 0, heads, D, x["spare_k"])

    def read(got):
        out = lambda r: _items_view(got, r, (nb, hw, heads, Tq), o_str, D).float().reshape(nb * hw * heads, Tq, D).clone()
        allo = got.mat(obig.ref, obig.rows, obig.ld, obig.ld, F16, {})
        pads = torch.cat([allo[:pad], allo[pad + o.rows:]]).clone()
        return out(o.ref), (out(o.ref.shifted(2 * inner)) if lo else None), pads
    b.init, b.read = init, read
    return b
