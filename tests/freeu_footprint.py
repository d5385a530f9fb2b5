"""TEST INFRASTRUCTURE — the footprint of T2V_OP_FREEU (27) for the arena-hazard analysis of tests/plan_hazards.py, beside the table of
tests/plan_footprint.py (which stays as it is): what the record reads and writes, from its field list in include/t2v_hip.h.

The op works in place: it reads and writes columns [0, C_h / 2) and [C_h, C_total) of the buffer and nothing else — not columns
[C_h / 2, C_h), not a column beyond C_total.  Rule R3 (no overlap of a launch's reads and writes) admits it as one more in-place class:
a workgroup owns its (frame, 64-channel slab) for the whole launch, reads all of it, meets at a barrier and only then stores
(csrc/freeu.hip: pass 1, `__syncthreads`, pass 2), so no thread reads an element another workgroup writes.

`installed()` puts both in force for the analyses run inside it and takes them out again."""
import contextlib

import plan_footprint as FP
import plan_hazards as H

FREEU = 27
INPLACE = "freeu in place (a workgroup owns its frame and channel slab; reads end at a barrier before the stores)"


def footprint(op):
    if op.kind != FREEU:
        return FP.footprint(op)
    rows, c_total, ld, c_h = op.i[0:4]
    b = FP._B(op)
    for col0, cols, what in ((0, c_h // 2, "scaled half of the stream"), (c_h, c_total - c_h, "filtered skip")):
        if cols > 0:
            b.mat(0, "r", rows, cols, ld, 4, what + " (read)", col0=col0)
            b.mat(0, "w", rows, cols, ld, 4, what, col0=col0)
    return b.out


def _in_place(op, w, r):
    return op.kind == FREEU and w.slot == 0 and r.slot == 0 and w.rects == r.rects and w.ld == r.ld and w.dtype == r.dtype == "f32"


@contextlib.contextmanager
def installed():
    held = H.footprint
    H.footprint = footprint
    H.INPLACE_CLASSES.append((INPLACE, _in_place, "csrc/freeu.hip freeu_kernel: pass 1, __syncthreads, pass 2 on the workgroup's own slab"))
    try:
        yield
    finally:
        H.footprint = held
        H.INPLACE_CLASSES.pop()
