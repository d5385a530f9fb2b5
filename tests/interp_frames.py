"""TEST INFRASTRUCTURE — `Interp` with form 1 of T2V_OP_TO_UINT8 (torch_to_np, include/t2v_hip.h): the record's documented semantics in
plain torch.  Form 0 stays the parent class's."""
import torch

from interp import _TD, Interp


class FramesInterp(Interp):
    def _op15(self, op, ext):
        if op.i[15] == 0:
            return super()._op15(op, ext)
        assert op.i[15] == 1 and op.i[7] == 0
        NI, C, Fr, H, W, in_dt, half = op.i[0:7]
        si, sc = (op.i[8] & 0xFFFFFFFF) | (op.i[9] << 32), op.i[10]
        sf, sy, sx = (op.i[11] & 0xFFFFFFFF) | (op.i[12] << 32), op.i[13], op.i[14]
        v = self.view(op.p[0], (NI, C, Fr, H, W), (si, sc, sf, sy, sx), _TD[in_dt], ext)
        v = v.half().float() if half else v.float()
        b = (v + 1.0) * 127.5                                     # two fp32 roundings
        b = torch.where(b > 0, b.clamp(max=255.0), torch.zeros_like(b))      # NaN and everything <= 0 -> 0, +inf -> 255
        u8 = b.to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()          # [NI, F, H, W, C]
        if op.p[1].space == "ext":
            out = ext[op.p[1].off]
            assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == u8.numel()
            out.view(u8.shape).copy_(u8)
        else:
            self.view(op.p[1], (u8.numel(),), (1,), torch.uint8, ext).copy_(u8.reshape(-1))
