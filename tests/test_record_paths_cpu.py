"""CPU: every code path a lowered program takes has an adversarial case (tests/record_paths.py is the key).

Lowered side: the matrix of tests/test_plan_hazards_cpu.py (tools/program_digest.py rows + extra_rows) under program_digest.FIXED; every
record is keyed per launch.  Adversarial side: every case of tests/gemm_inputs.py, norm_inputs.py, ff_fused_inputs.py,
fused_attention_inputs.py, elementwise_inputs.py and the attention case lists of tests/adversarial.py (programs: attention_records.py).
(1) every lowered key has at least one adversarial case — no exemptions; the message names the key, a row and an op;
(2) the key bites: for every field that takes more than one value in the matrix, an edit of a lowered record moves that field of its key;
(3) the assertion bites: without the only case of a lowered key, that key is reported with its row and op.
The report (printed; committed as profiles/lowered_paths.txt) counts keys per kind and names, for every case of the `lowered` families, the
key it closes and a deployed op that has it."""
import collections
import copy
import os

import pytest

import adversarial as A
import attention_records as AR
import elementwise_inputs as E
import ff_fused_inputs as FF
import fused_attention_inputs as FA
import gemm_inputs as G
import norm_inputs as N
import record_paths as RP
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd.program import NULL, Ref
from test_plan_hazards_cpu import ROOT, _fixed_environment, _lower, extra_rows
from tools import program_digest as PD


_ADVERSARIAL = []


def adversarial_side():
    """(adversarial: key -> [case id], the ids of the `lowered` cases); the caller provides the FIXED environment.  Shared with
    tests/test_geometry_paths_cpu.py and tools/geometry_paths.py: built once per process (nobody edits the result)."""
    if _ADVERSARIAL:
        return _ADVERSARIAL[0]
    adv, new = collections.OrderedDict(), set()

    def add(ops, cid, is_new=False):
        for op in ops:
            for k in RP.path_keys(op):
                adv.setdefault(k, []).append(cid)
        if is_new:
            new.add(cid)

    lowered = lambda c: c.get("family") == "lowered" or str(c["id"]).startswith("lowered-")
    for mod, tag in ((G, "gemm"), (N, "norm"), (FF, "ff"), (FA, "fused-attention")):
        for c in mod.CASES:
            add(mod.build(c).P.ops, f"{tag}:{c['id']}", lowered(c))
    for c in E.CASES:
        if not c.get("wrap"):          # (the grid-stride cases are their own size class of one kernel each and cost seconds to build)
            b = E.build(c)
            add(b.ops if b.ops is not None else b.P.ops, f"elementwise:{c['id']}", lowered(c))
    for c in A.ATTN_CASES:
        for attn2 in ((True, False) if c["attn2"] else (False,)):
            add(AR.build_attn(c, attn2).P.ops, f"attention:{c['id']}", lowered(c))
    for c in A.RELPOS_LONG_CASES:
        add(AR.build_relpos(c, None).P.ops, f"relpos:{c['id']}", lowered(c))
    for c in A.RELPOS_SHORT_CASES:
        for sel in c["sels"]:
            add(AR.build_relpos(c, sel).P.ops, f"relpos:{c['id']}/i[17]={sel}", lowered(c))
    _ADVERSARIAL.append((adv, new))
    return adv, new


@pytest.fixture(scope="module")
def sides():
    """(lowered: key -> [(row label, op name)], one sample record per key, adversarial: key -> [case id], the ids of the `lowered` cases)."""
    mp = pytest.MonkeyPatch()
    low, sample = collections.OrderedDict(), {}
    try:
        _fixed_environment(mp)
        for source in (PD.rows(ROOT), extra_rows()):
            for r in source:
                for op in _lower(r).prog.ops:
                    for k in RP.path_keys(op):
                        low.setdefault(k, []).append((r.label, op.name))
                        sample.setdefault(k, op)
        adv, new = adversarial_side()
    finally:
        mp.undo()
    return low, sample, adv, new


def missing_of(low, adv):
    """The failure lines: one per lowered key without a case, with the key, a row label and an op name."""
    return [f"{RP.kind_of(k)} [{RP.show(k)}] has no adversarial case: row '{low[k][0][0]}', op '{low[k][0][1]}' (+ {len(low[k]) - 1} more)"
            for k in low if k not in adv]


def test_every_lowered_path_has_an_adversarial_case(sides):
    low, _, adv, new = sides
    kinds = sorted({RP.kind_of(k) for k in low})
    lines = ["# kind: lowered keys, adversarial keys, lowered keys without a case, lowered keys only the `lowered` cases cover (= missing before them)"]
    for kind in kinds:
        lk = [k for k in low if RP.kind_of(k) == kind]
        ak = [k for k in adv if RP.kind_of(k) == kind]
        only_new = [k for k in lk if k in adv and all(cid in new for cid in adv[k])]
        lines.append(f"{kind}: {len(lk)} lowered, {len(ak)} adversarial, {sum(k not in adv for k in lk)} without a case, {len(only_new)} closed by the `lowered` cases")
    lines.append("# case of a `lowered` family -> the key it closes | a deployed op that has it")
    for k in low:
        if k in adv and all(cid in new for cid in adv[k]):
            lines.append(f"{adv[k][0]} -> {RP.kind_of(k)} [{RP.show(k)}] | {low[k][0][0]}: {low[k][0][1]}")
    print("\n".join("LOWERED-PATHS " + ln for ln in lines))
    if os.environ.get("T2V_WRITE_LOWERED_PATHS"):
        with open(os.environ["T2V_WRITE_LOWERED_PATHS"], "w") as f:
            f.write("\n".join(lines) + "\n")
    miss = missing_of(low, adv)
    assert not miss, f"{len(miss)} lowered code paths without an adversarial case:\n" + "\n".join(miss)


def _toggle_i(k, *values):
    """Editor: word k steps through `values` (default: 0 <-> 1)."""
    values = values or (0, 1)

    def edit(op):
        op.i[k] = values[(values.index(op.i[k]) + 1) % len(values)] if op.i[k] in values else values[0]
    return edit


def _toggle_p(k):
    def edit(op):
        op.p[k] = Ref("arena", 256) if op.p[k].space == "null" else NULL
    return edit


def _scale_i(k, f):
    def edit(op):
        op.i[k] = op.i[k] * f
    return edit


def _bump_i(k, d):
    def edit(op):
        op.i[k] = op.i[k] + d
    return edit


def _both(*edits):
    def edit(op):
        for e in edits:
            e(op)
    return edit


# field of a key -> the edits of a RECORD (the words and pointers the field is read from) that can move it; the test tries each on the
# matrix's records of that kind until one moves the field
_GEMM_EPILOGUE = {"epi": [_toggle_i(16, L.EPI_NONE, L.EPI_STATS, L.EPI_GEGLU)], "out": [_toggle_i(17)], "act": [_toggle_i(18, 0, 1, 2)], "bias": [_toggle_p(2)],
                  "bias_m": [_toggle_i(20)], "rowbias": [_toggle_p(3)], "res": [_toggle_p(4)], "res_wrap": [_toggle_i(30, 0, 5), _toggle_i(12, 0, 5)],
                  "out_lo": [_toggle_i(11)], "gn_silu": [_toggle_i(26)], "gn_lo": [_toggle_i(27)], "i29": [_toggle_i(29)]}
EDITS = {
    "GEMM": dict(_GEMM_EPILOGUE, tile=[_toggle_i(22, 5, 3, 0)], tile0_bn=[_toggle_i(1, 128, 64)], gather=[_toggle_i(7, 0, 1, 2)], stride=[_toggle_i(11, 1, 2)],
                 up=[_toggle_i(12)], i23=[_toggle_i(23)], ln=[_toggle_i(8, 0, 1, 2)], fold=[_toggle_i(19, 1, 4), _toggle_i(19, 4, 1), _toggle_i(19, 2, 1)],
                 k_tail=[_bump_i(2, 8)], m_ragged=[_bump_i(0, 1)], n_ragged=[_bump_i(1, 4)], lnx_chunked=[_scale_i(0, 1000)],
                 gn_seam=[_scale_i(24, 3), _scale_i(24, 2)], gn_chunked=[_scale_i(0, 1000)], xa_ragged=[_bump_i(25, 1)], xa_blocks=[_bump_i(26, 64)]),
    "GEMM.reduce": _GEMM_EPILOGUE,
    "GEMM.reduce+gn": dict(_GEMM_EPILOGUE, kr=[_both(_scale_i(0, 64), _scale_i(24, 64))]),
    "GROUPNORM": {"in": [_toggle_i(5)], "silu": [_toggle_i(6)], "phase": [_toggle_i(8, 0, 1, 2, 3)], "launch": [_toggle_i(12), _toggle_i(8, 0, 1, 2)],
                  "i12": [_toggle_i(12)], "i15": [_toggle_i(15)], "kr": [_scale_i(1, 8), _scale_i(1, 40)], "records": [_toggle_p(7)], "lo": [_toggle_i(16)],
                  "cast": [_toggle_p(8)], "cast_lo": [_toggle_i(20, 0, 8)], "halo": [_toggle_i(21, 0, 4), _toggle_i(22, 0, 4)], "nparts": [_toggle_i(9, 1, 3)],
                  "strips_wide": [_scale_i(1, 256)], "cols_loop": [_toggle_i(2, 320, 2560), _scale_i(2, 8)], "one_block": [_scale_i(1, 4096), _toggle_i(1, 4, 4096)]},
    "LAYERNORM": {"maxv": [_toggle_i(1, 320, 768, 1280, 2048)], "grid_stride": [_toggle_i(4, 0, 2)], "m_ragged": [_bump_i(0, 1)]},
    "ATTENTION": {"head_dim": [_toggle_i(14, 40, 64, 80, 160)], "causal": [_toggle_i(15)], "lo": [_toggle_i(16, 0, 128)], "kernel": [_scale_i(0, 64), _toggle_i(0, 16, 256)],
                  "second_role": [_both(_toggle_i(19), _toggle_i(20, 0, 77))], "nk_tiles": [_scale_i(1, 64), _toggle_i(1, 16, 256)], "nk_ragged": [_bump_i(1, 1)],
                  "nk2_ragged": [_toggle_i(20, 77, 128), _toggle_i(20, 154, 128), _toggle_i(20, 40, 64), _toggle_i(20, 24, 64)], "nq_ragged": [_bump_i(0, 1)]},
    "RELPOS_ATTN": {"kernel": [_toggle_i(17, 0, 3)], "head_dim": [_toggle_i(14, 40, 80, 160)], "offset": [_toggle_i(16, 0, 1)], "nq_lt_nk": [_bump_i(1, 1)],
                    "lo": [_toggle_i(18, 0, 128)], "tb": [_bump_i(1, 8)], "clipped": [_toggle_i(15, 1, 64)], "tiles": [_bump_i(1, 32)]},
    "NCTHW_TO_CL": {"in": [_toggle_i(5)], "bsrc": [_toggle_i(6, 0, 1)], "second": [_toggle_p(2)], "lo": [_toggle_i(7)]},
    "CL_TO_NCTHW": {"out": [_toggle_i(5)]},
    "COPY2D": {"src": [_toggle_i(4)], "dst": [_toggle_i(5)], "act": [_toggle_i(6, 0, 1, 2, 3)], "second": [_toggle_p(2)]},
    "SOFTMAX": {"cols_gt_256": [_scale_i(1, 64), _toggle_i(1, 64, 1024)]},
    "DDIM_STEP": {"eps": [_toggle_i(3)], "x": [_toggle_i(4)], "mode": [_toggle_i(5)], "guided": [_toggle_i(2, 0, 4)], "cps": [_toggle_i(6, 0, 1)],
                  "blend": [_toggle_i(7)], "i8": [_toggle_i(8, 0, 1, 2, 3)], "i9": [_toggle_i(9)]},
    "DEPTH_TOKENS": {"in": [_toggle_i(3)], "norm": [_toggle_i(4)]},
    "AVGPOOL2": {"f32_out": [_toggle_p(1)], "f16_out": [_toggle_p(2)]},
}


def test_every_key_field_bites(sides):
    """For every field of every kind's key that takes more than one value in the matrix: an edit of a lowered RECORD — the words and pointers
    the field is read from, not the key — moves that field.  A field without an edit in EDITS fails the test: a new key field brings its own."""
    low, sample, _, _ = sides
    by_kind = collections.defaultdict(list)
    for k in low:
        by_kind[RP.kind_of(k)].append(k)
    checked = 0
    for kind, keys in by_kind.items():
        for name in sorted({n for k in keys for n, _ in k[1:]}):
            if len({dict(k)[name] for k in keys if name in dict(k)}) < 2:
                continue          # one value in the whole matrix: nothing to tell apart (it is in the key for the day a lowering emits another)
            assert name in EDITS.get(kind, {}), f"no record edit for field '{name}' of {kind}"
            moved = False
            for k in keys:
                for edit in EDITS[kind][name]:
                    op = copy.deepcopy(sample[k])
                    try:
                        edit(op)
                        after = [kk for kk in RP.path_keys(op) if RP.kind_of(kk) == kind]
                    except (KeyError, ZeroDivisionError, AssertionError):
                        continue          # the edited record is not one the key can read (a tile id without a kernel ...)
                    if after and name in dict(after[0]) and name in dict(k) and dict(after[0])[name] != dict(k)[name]:
                        moved = True
                        break
                if moved:
                    break
            assert moved, f"{kind}: no edit of a record moves key field '{name}'"
            checked += 1
    assert checked >= 60, checked


def test_the_assertion_bites(sides):
    """Without the only case that covers some lowered key, that key is reported — with its row and its op."""
    low, _, adv, _ = sides
    sole = [(k, adv[k][0]) for k in low if k in adv and len(set(adv[k])) == 1]
    assert sole, "no lowered key with a single cover"
    for k, cid in (sole[0], sole[len(sole) // 2], sole[-1]):
        pruned = {kk: [c for c in cids if c != cid] for kk, cids in adv.items()}
        pruned = {kk: v for kk, v in pruned.items() if v}
        miss = missing_of(low, pruned)
        want = f"row '{low[k][0][0]}', op '{low[k][0][1]}'"
        assert any(RP.show(k) in m and want in m for m in miss), (cid, RP.show(k))


def test_out_of_scope_kinds_are_named_with_a_reason():
    assert all(isinstance(why, str) and why for why in RP.OUT_OF_SCOPE.values())
    assert set(RP.OUT_OF_SCOPE) | set(RP.KIND_NAMES) == set(range(1, L.OP_KIND_MAX))
