"""TEST INFRASTRUCTURE — FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net") restated in plain torch, for the tests of T2V_OP_FREEU.

Two forms of the Fourier filter with threshold 1 on planes v [..., H, W]:
  * `fourier_filter_fft`: the formulation FreeU itself runs — fftshift(fftn), a mask that is `scale` on the Python slices
    [H//2 - 1 : H//2 + 1, W//2 - 1 : W//2 + 1] and 1 elsewhere, ifftn(ifftshift) and the real part.  In the dtype it is given:
    float64 is the reference of every test, float32 is what FreeU computes and gives the tests their gate;
  * `fourier_filter_closed`: the closed form the kernel evaluates — the masked bins are u in {-1, 0} x v in {-1, 0} as DISTINCT
    indices modulo the axis length, so  out = v + (scale - 1) / (H W) * sum_bins (Re c cos(theta) - Im c sin(theta)).
`freeu_concat` applies FreeU to a channels-last concat buffer as the record describes it; `MUTANTS` are wrong versions of it, each of
which a designed operand of tests/freeu_inputs.py must expose."""
import math

import torch

SHAPES = [(1, 1), (1, 4), (4, 1), (2, 2), (2, 3), (3, 5), (4, 4), (5, 8), (9, 5), (18, 10)]       # (H, W) at which the two forms are compared
MODELSCOPE = {"b1": 1.2, "b2": 1.4, "s1": 0.9, "s2": 0.2}                                         # the authors' values for ModelScope


def fourier_filter_fft(v: torch.Tensor, scale: float) -> torch.Tensor:
    H, W = v.shape[-2:]
    V = torch.fft.fftshift(torch.fft.fftn(v, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(H, W, dtype=v.dtype)
    mask[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = scale
    return torch.fft.ifftn(torch.fft.ifftshift(V * mask, dim=(-2, -1)), dim=(-2, -1)).real


def bins(H: int, W: int, variant: str = ""):
    """The masked frequency bins (u, v).  Variants are the mutants' wrong sets."""
    us = sorted({0, -1 % H})
    vs = sorted({0, -1 % W})
    if variant == "hermitian":                 # +-1 both scaled
        us, vs = sorted({0, -1 % H, 1 % H}), sorted({0, -1 % W, 1 % W})
    out = [(u, v) for u in us for v in vs]
    if variant == "anti_diagonal":             # (-1, +1) and (+1, -1) included
        out += [b for b in [(-1 % H, 1 % W), (1 % H, -1 % W)] if b not in out]
    if variant == "length1_twice":             # an axis of length 1 counted as two bins
        out = [(u, v) for u in ([0, 0] if H == 1 else us) for v in ([0, 0] if W == 1 else vs)]
    return out


def fourier_filter_closed(v: torch.Tensor, scale: float, variant: str = "") -> torch.Tensor:
    """v [..., frames, C, H, W] or any [..., H, W] -> float64.  variant: a mutant ("" = the statement)."""
    H, W = v.shape[-2:]
    y = torch.arange(H, dtype=torch.float64)[:, None]
    x = torch.arange(W, dtype=torch.float64)[None, :]
    dy, dx = (W, H) if variant == "swapped" else (H, W)          # the mutant divides y by W and x by H, and takes its bins from (W, H)
    v64 = v.double()
    delta = torch.zeros_like(v64)
    blist = bins(dy, dx, variant)
    if variant in ("centre_floor", "centre_ceil"):      # the mask's centre taken as (H - 1) // 2, or as ceil(H / 2)
        cy, cx = ((H - 1) // 2, (W - 1) // 2) if variant == "centre_floor" else (-(-H // 2), -(-W // 2))
        rows = [r for r in range(cy - 1, cy + 1) if 0 <= r < H]
        cols = [c for c in range(cx - 1, cx + 1) if 0 <= c < W]
        blist = sorted({((r - H // 2) % H, (c - W // 2) % W) for r in rows for c in cols})
    over = (-4, -2, -1) if variant == "all_frames" and v.ndim >= 4 else (-2, -1)      # the mutant sums over the frames as well
    for u, w_ in blist:
        theta = 2 * math.pi * (u * y / dy + w_ * x / dx)
        re = (v64 * torch.cos(theta)).sum(dim=over, keepdim=True)
        im = -(v64 * torch.sin(theta)).sum(dim=over, keepdim=True)
        delta = delta + re * torch.cos(theta) - im * torch.sin(theta)
    return v64 + (scale - 1.0) / (H * W) * delta


def freeu_concat(X: torch.Tensor, frames: int, h: int, w: int, c_h: int, c_total: int, b: float, s: float, variant: str = "") -> torch.Tensor:
    """X [frames * h * w, ld] channels-last -> float64 copy with FreeU applied as T2V_OP_FREEU states it: columns [0, c_h / 2) times b
    (the product of the float32 values, exact in float64), columns [c_h, c_total) filtered per (frame, channel), the rest as it was.
    variant: a mutant of the statement ("" = the statement)."""
    out = X.double().clone()
    n_scaled = c_h if variant == "whole_stream" else c_h // 2
    out[:, :n_scaled] = X[:, :n_scaled].double() * float(torch.tensor(b, dtype=torch.float32))
    f0, f1 = (c_h, c_h + (c_total - c_h) // 2) if variant == "half_skip" else (c_h, c_total)
    if f1 > f0:
        sk = X[:, f0:f1].double().reshape(frames, h, w, f1 - f0).permute(0, 3, 1, 2)          # [frames, C, h, w]
        filt = fourier_filter_closed(sk, float(torch.tensor(s, dtype=torch.float32)), variant if variant not in ("whole_stream", "half_skip") else "")
        out[:, f0:f1] = filt.permute(0, 2, 3, 1).reshape(frames * h * w, f1 - f0)
    return out


MUTANTS = ("hermitian", "anti_diagonal", "swapped", "centre_floor", "centre_ceil", "length1_twice", "all_frames", "whole_stream", "half_skip")


def stage_gains(c_h: int, dim: int, freeu: dict, exchanged: bool = False):
    """(b, s) of a decoder block whose stream has c_h channels, or None — the channel-keyed rule.  exchanged: the mutant that gives the
    4 dim stage the second stage's values and the other way round."""
    first, second = (freeu["b1"], freeu["s1"]), (freeu["b2"], freeu["s2"])
    if exchanged:
        first, second = second, first
    return {4 * dim: first, 2 * dim: second}.get(c_h)


def apply_to_reference_unet(unet, stream_widths, dim: int, freeu: dict):
    """FreeU on a reference-style UNetSD whose `output_blocks[j][0]` is the ResBlock that reads decoder block j's skip concatenation
    [(b f), C_h + C_s, H, W] with C_h = stream_widths[j]: forward pre-hooks that split that input at the stream width and apply the
    torch.fft formulation in the input's dtype.  -> the hook handles (call .remove() on each)."""
    handles = []
    for j, blk in enumerate(unet.output_blocks):
        gains = stage_gains(stream_widths[j], dim, freeu)
        if gains is None:
            continue

        def hook(module, args, c_h=stream_widths[j], b=gains[0], s=gains[1]):
            x = args[0].clone()
            x[:, :c_h // 2] = x[:, :c_h // 2] * b
            x[:, c_h:] = fourier_filter_fft(x[:, c_h:], s)
            return (x,) + tuple(args[1:])
        handles.append(blk[0].register_forward_pre_hook(hook))
    return handles
