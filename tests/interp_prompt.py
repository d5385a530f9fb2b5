"""TEST INFRASTRUCTURE — the CPU interpreter (tests/interp.py) extended by the records of the prompt-syntax work:
T2V_OP_EMPHASIS (24) and the second role of a T2V_OP_ATTENTION record (i[19] alt_from, i[20] its key count, i[21] its sample stride,
p[4] / p[5] its K / V bases).  Same contract as its base: the SAME op list, arena offsets and packed weights the library executes.
"""
import copy

import torch

from interp import _TD, Interp
from sd_webui_text2video_amd.program import NULL


class PromptInterp(Interp):
    def _op4(self, op, ext, rel=False):
        """ATTENTION with two roles = two plain records: outer samples [0, alt_from) as given, [alt_from, b_outer) on their own keys."""
        alt_from = op.i[19]
        if rel or not alt_from:
            return super()._op4(op, ext, rel)
        assert not op.i[15] and op.p[6].space == "null" and 0 < alt_from < op.i[3]
        first, second = copy.copy(op), copy.copy(op)
        for o in (first, second):
            o.i, o.p = list(op.i), list(op.p)
            o.i[19] = o.i[20] = o.i[21] = 0
            o.p[4] = o.p[5] = NULL
        first.i[3] = alt_from
        second.i[3] = op.i[3] - alt_from
        second.i[1], second.i[9] = op.i[20], op.i[21]
        second.p[0] = op.p[0].shifted(2 * alt_from * op.i[6])
        second.p[3] = op.p[3].shifted(2 * alt_from * op.i[12])
        second.p[1], second.p[2] = op.p[4], op.p[5]
        super()._op4(first, ext)
        super()._op4(second, ext)

    def _op24(self, op, ext):
        """EMPHASIS: out = fp32(fp32(z * m) * fp32(sum z / sum (z * m))), the sums over the whole batch in fp64."""
        rows, W, ldz, ldo, zdt = op.i[0:5]
        z = self.mat(op.p[0], rows, W, ldz, _TD[zdt], ext).float()
        m = self.view(op.p[1], (rows,), (1,), torch.float32, ext)
        zm = z * m[:, None]
        ratio = (z.double().sum() / (z.double() * m.double()[:, None]).sum()).float()
        self.mat(op.p[2], rows, W, ldo, torch.float32, ext).copy_(zm * ratio)
