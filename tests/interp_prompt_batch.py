"""TEST INFRASTRUCTURE — the CPU interpreter (tests/interp.py, through tests/interp_prompt.py) extended by the per-sample table of a
T2V_OP_ATTENTION record: i[22] rows of the table (== batch_outer), i[23] its largest key count, i[24] the K / V rows it spans,
p[7] int32 [batch_outer][2] = {key count, first row}.  Same contract as its base: the SAME op list, arena offsets and packed weights the
library executes.
"""
import copy

import torch

from interp_prompt import PromptInterp
from sd_webui_text2video_amd.program import NULL


class PromptBatchInterp(PromptInterp):
    def table(self, op, ext):
        """The record's table as a list of (key count, first row), checked against what the record says about it."""
        rows = self.view(op.p[7], (op.i[22], 2), (2, 1), torch.int32, ext).tolist()
        assert op.i[22] == op.i[3] and all(0 < n <= op.i[23] and 0 <= r and r + n <= op.i[24] for n, r in rows), (rows, op.i[22:25])
        assert max(n for n, _ in rows) == op.i[23]
        return rows

    def _op4(self, op, ext, rel=False):
        """ATTENTION with a table = one plain record per outer sample, on that sample's keys."""
        if rel or not op.i[22]:
            return super()._op4(op, ext, rel)
        assert not op.i[15] and op.p[6].space == "null" and not op.i[19] and op.p[4].space == "null" and op.p[5].space == "null"
        for s, (n, first) in enumerate(self.table(op, ext)):
            one = copy.copy(op)
            one.i, one.p = list(op.i), list(op.p)
            one.i[22] = one.i[23] = one.i[24] = 0
            one.p[7] = NULL
            one.i[3], one.i[1] = 1, n
            one.p[0] = op.p[0].shifted(2 * s * op.i[6])
            one.p[3] = op.p[3].shifted(2 * s * op.i[12])
            one.p[1], one.p[2] = op.p[1].shifted(2 * first * op.i[8]), op.p[2].shifted(2 * first * op.i[8])
            super()._op4(one, ext)
