"""Writes tests/golden/record_verdicts.npz: the verdicts of a library built from the PARENT commit on the corpus of tests/record_verdicts.py.
Run once per refactor of the record decoding, against the parent's build — this script builds nothing:

    python tests/golden/make_golden_record_verdicts.py PARENT/libt2v_hip.so --parent <commit hash> [--csrc PARENT/csrc]

--csrc: the parent's csrc directory; every bad("...") literal of its GEMM and ATTENTION validation is then looked for among the messages the
corpus drew, and the ones no record reaches are printed (profiles/record_decode.txt names the check that shadows each).
Stored: per record kind, the 32 ints, the 8 floats, the mask of the pointers that are set, the status of t2v_plan_create and an index into
`messages` (0: accepted); per plan its label, its op count and t2v_plan_num_launches; the parent's commit hash."""
import argparse
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("library")
    ap.add_argument("--parent", required=True)
    ap.add_argument("--csrc")
    ap.add_argument("--out", default=os.path.join(HERE, "record_verdicts.npz"))
    args = ap.parse_args()
    os.environ["T2V_LIB_PATH"] = os.path.abspath(args.library)          # read by sd_webui_text2video_amd._lib at import
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import pytest
    import record_verdicts as RV
    from sd_webui_text2video_amd import _lib as L
    from test_plan_hazards_cpu import _fixed_environment
    assert os.path.samefile(L.LIB_PATH, args.library)
    lib = L.load()
    mp = pytest.MonkeyPatch()
    try:
        _fixed_environment(mp)
        records, plans = RV.corpus()
        verdicts = [RV.verdict(lib, r) for r in records]
        counts = [(label, len(ops if ops is not None else prog.ops), RV.launches(lib, prog, ops)) for label, prog, ops in plans]
    finally:
        mp.undo()
    strip = lambda m: re.sub(r"^op 0 \(kind \d+, tag 0\): ", "", m)
    messages = [""] + sorted({m for _, m in verdicts if m})
    index = {m: k for k, m in enumerate(messages)}
    np.savez_compressed(args.out, **RV.arrays_of(records), status=np.array([s for s, _ in verdicts], np.int32),
                        msg=np.array([index[m] for _, m in verdicts], np.int16), messages=np.array(messages),
                        plan_labels=np.array([c[0] for c in counts]), plan_ops=np.array([c[1] for c in counts], np.int32),
                        plan_launches=np.array([c[2] for c in counts], np.int32), parent=np.array(args.parent))
    ok = sum(s == 0 for s, _ in verdicts)
    print(f"{len(records)} records ({ok} accepted, {len(records) - ok} refused with {len(messages) - 1} distinct messages), {len(counts)} plans "
          f"({sum(n - l for _, n, l in counts if l >= 0)} fused pairs), {os.path.getsize(args.out)} bytes")
    for m in messages[1:]:
        print(f"  {sum(mm == m for _, mm in verdicts):6d}  {strip(m)}")
    if args.csrc:
        src = open(os.path.join(args.csrc, "executor.hip")).read()
        body = src[src.index("case T2V_OP_GEMM: {"):src.index("case T2V_OP_GROUPNORM: {")] + src[src.index("case T2V_OP_ATTENTION: {"):src.index("case T2V_OP_RELPOS_ATTN:")]
        literals = re.findall(r'bad\("((?:[^"\\]|\\.)*)"\)', body)
        seen = {strip(m) for m in messages}
        # (validate_op formats into 160 bytes: the longest literal arrives cut off, so a drawn message may be a prefix of its literal)
        missing = [t for t in literals if not any(m and t.startswith(m) for m in seen)]
        print(f"{len(literals)} bad(...) literals in the two validation cases, {len(missing)} not reached:")
        for t in missing:
            print("  NOT REACHED:", t)


if __name__ == "__main__":
    main()
