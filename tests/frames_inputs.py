"""Designed inputs of T2V_OP_TO_UINT8 form 1 (torch_to_np, videocrafter/sample_utils.py:98-107) and the seeded inputs of the per-video
driver golden: shared by the generators (tests/golden/make_golden_frames.py, make_golden_driver.py) and the CPU / GPU tests.  The
expected bytes are NOT computed here: they are in tests/golden/torch_to_np_designed.npz, written by the reference's own function."""
import numpy as np
import torch

# ---- torch_to_np: designed inputs -----------------------------------------------------------------------------------------------------------
BLOCK = (2, 3, 2, 3, 5)          # NI, C, F, H, W of one block of 180 elements; the frames axis is repeated to hold the inputs


def f16_inputs() -> np.ndarray:
    """Every non-NaN fp16 value, +-inf included: 63 490 (the 2 x 1023 NaN patterns are outside the bit-exact contract)."""
    v = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16)
    v = v[~np.isnan(v)]
    assert v.size == 63490
    return v


def f32_inputs() -> np.ndarray:
    """For every k in 0 .. 255 the fp32 value nearest k / 127.5 - 1 (where (x + 1) * 127.5 crosses k) with two neighbours on either side,
    then +-0, denormals, +-1 with their neighbours, +-inf and values far outside [-1, 1]."""
    f = np.float32
    vals = []
    for k in range(256):
        v = f(k / 127.5 - 1.0)
        lo1, hi1 = np.nextafter(v, f(-4)), np.nextafter(v, f(4))
        vals += [np.nextafter(lo1, f(-4)), lo1, v, hi1, np.nextafter(hi1, f(4))]
    for v in (f(-1.0), f(1.0)):
        vals += [np.nextafter(v, f(-4)), v, np.nextafter(v, f(4))]
    vals += [f(0.0), f(-0.0), f(1e-40), f(-1e-40), f(1.4e-45), f(np.inf), f(-np.inf), f(3.0), f(-1.5), f(1e6), f(-1e6), f(3e38), f(-3e38),
             f(65504.0), f(65520.0), f(-65520.0), f(0.999), f(1.0039), f(1.00394)]
    return np.asarray(vals, dtype=np.float32)


def frames_for(n: int) -> int:
    """The number of frames F (a multiple of BLOCK's 2) at which [2, 3, F, 3, 5] holds n elements."""
    per = BLOCK[0] * BLOCK[1] * BLOCK[3] * BLOCK[4]
    f = -(-n // per)
    return f + f % 2


def as_video(flat: torch.Tensor, fill: float = 0.25):
    """flat [n] -> ([2, 3, F, 3, 5] video holding flat in its first n elements (row-major) and `fill` behind them, n)."""
    n = flat.numel()
    shape = (BLOCK[0], BLOCK[1], frames_for(n), BLOCK[3], BLOCK[4])
    v = torch.full((int(np.prod(shape)),), fill, dtype=flat.dtype)
    v[:n] = flat
    return v.view(shape), n


def want_video(bytes_flat: torch.Tensor, fill_byte: int, shape):
    """The fixture's per-element bytes laid out as torch_to_np lays out the video of `as_video`: [NI, F, H, W, C]."""
    n = bytes_flat.numel()
    w = torch.full((int(np.prod(shape)),), fill_byte, dtype=torch.uint8)
    w[:n] = bytes_flat
    return w.view(shape).permute(0, 2, 3, 4, 1).contiguous()


FILL, FILL_BYTE = 0.25, 159          # (0.25 + 1) * 127.5 = 159.375, exact in fp32 and for the fp16 input


# ---- the driver golden: three single-video runs of the reference's DDIMSampler ---------------------------------------------------------------
SEED = 1234                # video v: noise_gen seeded SEED + v
VIDEOS, STEPS, ETA, CFG = 3, 4, 1.0, 7.5
SHAPE = (4, 5, 8, 8)       # the tiny LVDM latent [c, t, h, w]


def driver_inputs():
    """-> (ctx [2, 9, 768]: cond, uncond; x_T [3, 4, 5, 8, 8]: one start latent per video)."""
    g = torch.Generator().manual_seed(77)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(VIDEOS, *SHAPE, generator=g)
    return ctx, x_T
