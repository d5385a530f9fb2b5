"""TEST INFRASTRUCTURE — designed operands for T2V_OP_FREEU and what each of them exposes (tests/test_freeu_inputs_cpu.py proves it on
the float64 restatement of tests/freeu_ref.py; tests/test_gpu_freeu.py runs the kernel on the same operands).

An operand is a channels-last concat buffer X [frames * h * w, ld] fp32 = [stream (c_h) | skip (c_s) | NaN guard columns].  The stream
is N(0, 1); the skip planes follow `name`:
  noise       N(0, 1), every frame its own draw
  cos_y       a(f, c) cos(2 pi y / h)                 h >= 3: bins +1 and -1 carry it, only -1 is scaled -> comes back x (s + 1) / 2
  cos_x       a(f, c) cos(2 pi x / w)                 likewise along the other axis
  cos_minus   a(f, c) cos(2 pi (y / h - x / w))       bins (1, -1) and (-1, 1): neither is scaled -> comes back unchanged (h, w >= 3)
  cos_plus    a(f, c) cos(2 pi (y / h + x / w))       bins (1, 1) and (-1, -1): one of the two is scaled -> x (s + 1) / 2 (h, w >= 3)
with a(f, c) = (1 + f) (1 + c % 3): frames and channels differ, so sums taken over the wrong set show."""
import math

import torch

import freeu_ref as FR

GUARD = 8                                # NaN-filled columns behind C_total (ld = C_total + GUARD)
# (frames, h, w, C_h, C_s): the issue's list, one geometry whose h * w = 77 is more than a workgroup's 16 (or 4) rows per trip and no
# multiple of either, and one whose widths (C_h % 8 != 0, C_s % 4 != 0) take the one-element-per-lane path
GEOMS = [(2, 1, 4, 64, 32), (2, 2, 3, 64, 64), (3, 3, 5, 64, 96), (2, 9, 5, 128, 64), (2, 18, 10, 128, 128), (1, 36, 64, 128, 64),
         (2, 7, 11, 64, 40), (2, 5, 8, 64, 32), (2, 3, 5, 6, 5)]
B, S = 1.3, 0.25                         # the op-level values: far from 1, exactly representable or not does not matter

# mutant of tests/freeu_ref.py -> (operand name, geometry) that exposes it
CATCHES = {
    "hermitian": ("cos_y", (2, 9, 5, 128, 64)),
    "anti_diagonal": ("cos_minus", (2, 9, 5, 128, 64)),
    "swapped": ("cos_y", (2, 9, 5, 128, 64)),
    # (for real planes a mask moved by one bin along an axis is the same filter when the other axis is odd too — the two masks are complex
    #  conjugates — so the centre mutants show where one axis is even: floor((n - 1) / 2) differs from n // 2 on an even axis, ceil(n / 2)
    #  on an odd one, and the other axis must break the symmetry)
    "centre_floor": ("noise", (2, 18, 10, 128, 128)),
    "centre_ceil": ("noise", (2, 5, 8, 64, 32)),
    "length1_twice": ("noise", (2, 1, 4, 64, 32)),
    "all_frames": ("cos_y", (2, 9, 5, 128, 64)),
    "whole_stream": ("noise", (2, 2, 3, 64, 64)),
    "half_skip": ("noise", (2, 2, 3, 64, 64)),
}
NAMES = ("noise", "cos_y", "cos_x", "cos_minus", "cos_plus")


def operand(name: str, geom, seed: int = 0) -> torch.Tensor:
    frames, h, w, c_h, c_s = geom
    g = torch.Generator().manual_seed(1000 * seed + 7 * h + w + c_h)
    X = torch.full((frames * h * w, c_h + c_s + GUARD), float("nan"))
    X[:, :c_h] = torch.randn(frames * h * w, c_h, generator=g)
    if name == "noise":
        X[:, c_h:c_h + c_s] = torch.randn(frames * h * w, c_s, generator=g)
        return X
    y = torch.arange(h, dtype=torch.float64)[:, None] / h
    x = torch.arange(w, dtype=torch.float64)[None, :] / w
    plane = {"cos_y": torch.cos(2 * math.pi * y).expand(h, w), "cos_x": torch.cos(2 * math.pi * x).expand(h, w),
             "cos_minus": torch.cos(2 * math.pi * (y - x)), "cos_plus": torch.cos(2 * math.pi * (y + x))}[name]
    amp = (1 + torch.arange(frames, dtype=torch.float64))[:, None] * (1 + torch.arange(c_s) % 3)[None, :].double()      # [frames, c_s]
    sk = amp[:, None, None, :] * plane[None, :, :, None]                                                                 # [frames, h, w, c_s]
    X[:, c_h:c_h + c_s] = sk.reshape(frames * h * w, c_s).float()
    return X


def expected_factor(name: str, h: int, w: int, s: float):
    """What the filter multiplies the designed skip planes by (float64 arithmetic on the exact pattern), or None where the pattern is
    not a pure pair of bins at this size (an axis shorter than 3)."""
    need = {"cos_y": h >= 3, "cos_x": w >= 3, "cos_minus": h >= 3 and w >= 3, "cos_plus": h >= 3 and w >= 3}.get(name)
    if not need:
        return None
    return 1.0 if name == "cos_minus" else (s + 1.0) / 2.0


def reference(X: torch.Tensor, geom, b: float = B, s: float = S, variant: str = "") -> torch.Tensor:
    frames, h, w, c_h, c_s = geom
    return FR.freeu_concat(X, frames, h, w, c_h, c_h + c_s, b, s, variant)


def fp32_fft(X: torch.Tensor, geom, s: float = S) -> torch.Tensor:
    """The skip columns through the fp32 torch.fft formulation (what FreeU itself computes): [frames * h * w, c_s] fp32."""
    frames, h, w, c_h, c_s = geom
    sk = X[:, c_h:c_h + c_s].reshape(frames, h, w, c_s).permute(0, 3, 1, 2).contiguous()
    return FR.fourier_filter_fft(sk, float(torch.tensor(s, dtype=torch.float32))).permute(0, 2, 3, 1).reshape(frames * h * w, c_s)
