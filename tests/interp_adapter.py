"""TEST INFRASTRUCTURE — the CPU interpreter (tests/interp.py) extended by the ABI-11 records of the depth adapter:
T2V_OP_DEPTH_TOKENS (22), T2V_OP_AVGPOOL2 (23), the ReLU activation of a GEMM (i[18] = 2) and the residual row wrap of every gather
mode (i[30]).  Same contract as its base: the SAME op list, arena offsets and packed weights the library executes, with plain torch.
"""
import copy

import torch
import torch.nn.functional as F

from interp import _TD, Interp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd.program import Ref

_TMP_SLOT = L.EXT_SLOTS + 1          # a private ext key for the expanded residual (never a real slot)


class AdapterInterp(Interp):
    def _op1(self, op, ext):
        I = op.i
        relu, wrap = I[18] == L.ACT_RELU, I[30]
        if not relu and not wrap:
            return super()._op1(op, ext)
        op2 = copy.copy(op)
        op2.i, op2.p = list(op.i), list(op.p)
        if wrap:                                 # residual of `wrap` rows, row m >= wrap reads row m - wrap
            M, N, ldr = I[0], I[1], I[6]
            assert M <= 2 * wrap and op.p[4].space != "null" and I[16] in (L.EPI_NONE, L.EPI_STATS, L.EPI_GN)
            R = self.mat(op.p[4], wrap, N, ldr, torch.float32, ext)
            ext = dict(ext)
            ext[_TMP_SLOT] = torch.cat([R, R[: M - wrap]], dim=0).contiguous()
            op2.p[4], op2.i[6], op2.i[30] = Ref("ext", _TMP_SLOT), N, 0
        if relu:                                 # the activation sits between bias and residual; the adapter never combines the two
            assert op.p[4].space == "null" and I[16] == L.EPI_NONE and op.p[3].space == "null"
            op2.i[18] = 0
        super()._op1(op2, ext)
        if relu:
            out = self.mat(op.p[5], I[0], I[1], I[5], _TD[I[17]], ext)
            out.copy_(F.relu(out))               # (rounding and ReLU commute)

    def _op22(self, op, ext):
        """DEPTH_TOKENS: per-frame min-max normalisation (optional) + PixelUnshuffle(8) -> fp16 tokens."""
        n, H, W, in_dt, norm, ld = op.i[0:6]
        d = self.view(op.p[0], (n, 1, H, W), (H * W, H * W, W, 1), _TD[in_dt], ext).float()
        if norm:
            lo, hi = torch.amin(d, dim=[1, 2, 3], keepdim=True), torch.amax(d, dim=[1, 2, 3], keepdim=True)
            d = 2. * (d - lo) / (hi - lo + 1e-7) - 1.
        tok = F.pixel_unshuffle(d, 8).permute(0, 2, 3, 1).reshape(n * (H // 8) * (W // 8), 64)
        self._st(self.mat(op.p[1], tok.shape[0], 64, ld, torch.float16, ext), tok, torch.float16)

    def _op23(self, op, ext):
        """AVGPOOL2: 2 x 2 mean of channels-last fp32 tokens, fp32 and / or fp16 out."""
        n, H, W, C, ld_in, ld32, ld16 = op.i[0:7]
        x = self.view(op.p[0], (n, H, W, C), (H * W * ld_in, W * ld_in, ld_in, 1), torch.float32, ext)
        Ho, Wo = H // 2, W // 2
        x = x[:, :2 * Ho, :2 * Wo]
        v = ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])) * 0.25
        v = v.reshape(n * Ho * Wo, C)
        if op.p[1].space != "null":
            self._st(self.mat(op.p[1], v.shape[0], C, ld32, torch.float32, ext), v, torch.float32)
        if op.p[2].space != "null":
            self._st(self.mat(op.p[2], v.shape[0], C, ld16, torch.float16, ext), v, torch.float16)

    def _op18(self, op, ext):
        """RESHARD_ROWS with an ext-slot source (the feature add: chunk stride 0 = the feature's rows repeat); other forms: the base."""
        if op.p[0].space != "ext":
            return super()._op18(op, ext)
        rows, cols, P, s_src, s_dst, ld_src, ld_dst, dt, ld_res = op.i[0:9]
        assert op.i[9] <= 1 and _TD[dt] == torch.float32
        r = torch.arange(rows)
        rs, rd = (r // P) * s_src + r % P, (r // P) * s_dst + r % P
        v = self.mat(op.p[0], int(rs.max()) + 1, cols, ld_src, torch.float32, ext)[rs].clone()
        if op.p[2].space != "null":
            v = v + self.mat(op.p[2], int(rd.max()) + 1, cols, ld_res, torch.float32, ext)[rd]
        self.mat(op.p[1], int(rd.max()) + 1, cols, ld_dst, torch.float32, ext)[rd] = v
