"""TEST INFRASTRUCTURE — `Interp` with T2V_OP_FREEU (27, include/t2v_hip.h): the record's documented semantics in plain torch — the
float64 closed form of tests/freeu_ref.py, rounded once to fp32, in place on the concat buffer."""
import torch

import freeu_ref as FR
from interp import Interp


class FreeuInterp(Interp):
    def _op27(self, op, ext):
        rows, c_total, ld, c_h, frames, h, w = op.i[0:7]
        assert rows == frames * h * w and c_h % 2 == 0 and 0 < c_h <= c_total <= ld
        X = self.mat(op.p[0], rows, c_total, ld, torch.float32, ext)
        X.copy_(FR.freeu_concat(X, frames, h, w, c_h, c_total, op.f[0], op.f[1]).float())
