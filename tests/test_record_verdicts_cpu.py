"""CPU: what the library says of GEMM and ATTENTION records is what the commit before the record decodes said
(tests/golden/record_verdicts.npz, written by tests/golden/make_golden_record_verdicts.py against a build of that commit; the corpus:
tests/record_verdicts.py).
(1) every record of the golden, as a one-record plan: the status of t2v_plan_create and the exact t2v_last_error() text;
(2) every plan — each lowered program, whole and without its step-invariant ops, and every plan of tests/ff_fused_inputs.py: the same
    label, op count and t2v_plan_num_launches, i.e. the same feed-forward pairs fused."""
import collections

import numpy as np
import pytest

import record_verdicts as RV
from sd_webui_text2video_amd import _lib as L
from test_plan_hazards_cpu import _fixed_environment


@pytest.fixture(scope="module")
def golden():
    z = np.load(RV.GOLDEN)
    return {k: z[k] for k in z.files}


def test_every_record_gets_the_parents_verdict(built_lib, golden):
    records, messages = RV.records_of(golden), [str(m) for m in golden["messages"]]
    assert len(records) == len(set(records)) >= 40000 and len(str(golden["parent"])) == 40
    wrong = []
    for rec, status, msg in zip(records, golden["status"], golden["msg"]):
        got = RV.verdict(built_lib, rec)
        if got != (int(status), messages[msg]):
            wrong.append(f"kind {rec.kind} i={list(rec.ints)} pointers={rec.mask:#05x}: {got} != {(int(status), messages[msg])}")
    assert not wrong, f"{len(wrong)} of {len(records)} verdicts differ from the parent's:\n" + "\n".join(wrong[:20])
    # both kinds have accepted and refused records, and no message is there without a record
    seen = collections.Counter((r.kind, int(s) == 0) for r, s in zip(records, golden["status"]))
    assert all(seen[(k, ok)] > 0 for k in RV.KINDS for ok in (True, False)), seen
    assert set(golden["msg"].tolist()) == set(range(len(messages)))
    assert set(RV.hand_written()) <= set(records)


def test_every_plan_fuses_the_parents_pairs(built_lib, golden):
    mp = pytest.MonkeyPatch()
    try:
        _fixed_environment(mp)
        plans = [(label, prog, None) for label, prog in RV.lowered_programs()]
        plans = [p for label, prog, _ in plans for p in RV.with_and_without_invariants(label, prog)] + list(RV.ff_plans())
        got = [(label, len(ops if ops is not None else prog.ops), RV.launches(built_lib, prog, ops)) for label, prog, ops in plans]
    finally:
        mp.undo()
    want = list(zip((str(v) for v in golden["plan_labels"]), golden["plan_ops"].tolist(), golden["plan_launches"].tolist()))
    assert [g[0] for g in got] == [w[0] for w in want]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:10]
    assert sum(n - l for _, n, l in want) >= 40 and any(n == l for _, n, l in want) and all(l >= 0 for _, _, l in want)      # fused pairs, and plans without one

