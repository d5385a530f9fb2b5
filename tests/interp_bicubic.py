"""numpy evaluation of T2V_OP_RESAMPLE's float bicubic mode (i[9] = 1) with exactly the arithmetic include/t2v_hip.h states:

    out[p][y][x] = sum_{a = 0..3} wy[y][a] * ( sum_{b = 0..3} wx[x][b] * fp32(src[p][iy[y][a]][ix[x][b]]) )

both sums in ascending order starting from the first product, every multiply and add rounded on its own.  numpy's elementwise
operators round each result to the array's dtype and never contract a multiply with an add, so float32 arrays give the kernel's
bits.  The tables come from packing.bicubic_table (float64 coordinates and weights, the weights rounded once to float32).  With
dtype=numpy.float64 the same code evaluates the unrounded weights on float64 input: the check of the tables against torch's
float64 interpolation."""
import numpy as np

from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk


def bicubic_eval(x, wy, iy, wx, ix):
    """x [P, H, W]; wy / iy [Ho, 4], wx / ix [Wo, 4] -> [P, Ho, Wo] in the dtype of x (the weights must have the same dtype).  The indices
    are clamped to the image before use, as the kernel clamps them."""
    assert x.ndim == 3 and x.dtype == wy.dtype == wx.dtype and wy.shape[1] == wx.shape[1] == 4
    P, H, W = x.shape
    iy, ix = np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)
    out = None
    with np.errstate(invalid="ignore", over="ignore"):          # 0 * inf, inf - inf: NaN as on the device, no warning wanted
        for a in range(4):
            rows = x[:, iy[:, a], :]                             # [P, Ho, W]
            h = None
            for b in range(4):
                term = wx[None, None, :, b] * rows[:, :, ix[:, b]]
                h = term if h is None else h + term
            term = wy[None, :, None, a] * h
            out = term if out is None else out + term
    return out


def bicubic_interp(x, Ho, Wo, dtype=np.float32):
    """x [P, H, W] (float16 / float32 / float64 numpy array) -> [P, Ho, Wo] of `dtype`: the record's result (dtype float32), or the
    float64 evaluation of the unrounded tables (dtype float64)."""
    x = np.asarray(x)
    P, H, W = x.shape
    wy, iy = pk.bicubic_table(H, Ho, dtype=dtype)
    wx, ix = pk.bicubic_table(W, Wo, dtype=dtype)
    return bicubic_eval(x.astype(dtype), wy, iy, wx, ix)


def bicubic_record(op, src, weights, indices):
    """Evaluate one lowered record (program.Op of Program.bicubic): `src` the source as a numpy array of P * H * W elements of the
    record's input dtype, `weights` / `indices` its packed tables (p[2] / p[3]) as numpy arrays -> float32 [P, Ho, Wo]."""
    I = op.i
    P, H, W, Ho, Wo = I[0], I[1], I[2], I[4], I[10]
    assert op.kind == L.OP_RESAMPLE and I[9] == 1 and (I[3], I[5], I[6], I[7]) == (1, 0, 4, 1) and I[11] in (L.F16, L.F32)
    src = np.asarray(src)
    assert src.dtype == (np.float16 if I[11] == L.F16 else np.float32) and src.size == P * H * W
    weights, indices = np.asarray(weights), np.asarray(indices)
    assert weights.dtype == np.float32 and indices.dtype == np.int32 and weights.shape == indices.shape == (Ho + Wo, 4)
    return bicubic_eval(src.reshape(P, H, W).astype(np.float32), weights[:Ho], indices[:Ho], weights[Ho:], indices[Ho:])
