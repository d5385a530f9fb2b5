"""Torch restatement (fp32, sort-based) of T2V_OP_DDIM_STEP mode 2 (include/t2v_hip.h), the thresholded data prediction of UniPC
(uni_pc/uni_pc.py:351-364 behind the guidance combine of :304-307), the cases of its golden file and the designed inputs of its tests.

  x0_of(x, eps_pair, sigma, alpha, g, guided)   e = eu + g (ec - eu) over all channels when guided, x0 = (x - sigma e) / alpha; every
                                                 operation is one fp32 tensor operation, i.e. rounded by itself
  measure(x0, 0.995)                             tests/x0_threshold_ref.py: a sort, torch.quantile's fp32 rank arithmetic, torch.lerp
  threshold(x0, s)                               min(max(x0, -s), s) / s per video — torch.clamp with tensor bounds, NaN propagating
  x0_threshold_cpu(...)                          stand-in for samplers._x0_threshold (same arguments): writes `out` and the table row
"""
import numpy as np
import torch

import x0_threshold_ref as XR
from x0_threshold_ref import ranks

F32 = torch.float32
QUANTILE = 0.995


def measure(x0: torch.Tensor, p: float):
    """The measure pass of mode 0 (x0_threshold_ref.measure: sort, fp32 rank, the two order statistics) with the interpolation pinned
    down: torch.lerp's formula, w < 0.5 ? a + w d : b - (1 - w) d with d = b - a rounded to fp32, the product and the sum in ONE
    rounding — what the kernel's fma and torch's vectorised CPU kernel compute.  torch.lerp itself rounds a lone element twice on some
    hosts (1 ulp), so the value is formed in float64, where the product of two fp32 numbers is exact."""
    tab = XR.measure(x0, p)
    _, _, w = ranks(x0[0].numel(), p)
    a, b = tab[:, 2], tab[:, 3]
    d = (b - a).double()
    q = ((np.float64(w) * d + a.double()) if w < 0.5 else (np.float64(np.float32(w - np.float32(1.0))) * d + b.double())).to(F32)
    q = torch.where(torch.isnan(tab[:, 1]), tab[:, 1], q)
    return torch.stack([q.clamp(min=1.0), q, a, b], dim=1)


def x0_of(x, eps_pair, sigma, alpha, g, guided):
    nb = x.shape[0]
    sg, al, gs = (torch.tensor(float(v), dtype=F32) for v in (sigma, alpha, g))
    e = eps_pair[0:nb].to(F32)
    if guided:
        u = eps_pair[nb:2 * nb].to(F32)
        d = gs * (e - u)
        e = u + d
    se = sg * e
    num = x.to(F32) - se
    return num / al


def threshold(x0, s):
    sv = s.to(F32).view(-1, *((1,) * (x0.ndim - 1)))
    return torch.min(torch.max(x0, -sv), sv) / sv


def predict(x, eps_pair, sigma, alpha, g, guided, quantile=QUANTILE):
    """-> (thresholded x0, table [videos, 4] = {s, q, v_lo, v_hi})."""
    x0 = x0_of(x, eps_pair, sigma, alpha, g, guided)
    table = measure(x0, quantile)
    return threshold(x0, table[:, 0]), table


def x0_threshold_cpu(out, x, eps_pair, sigma, alpha, guide, guided, table):
    r, tab = predict(x, eps_pair, sigma, alpha, guide, guided)
    table.copy_(tab)
    out.copy_(r)
    return out


# ---- designed inputs: x0 values that reach the kernel exactly (eps = 0, sigma = 0.5, alpha = 1: x0 = (x - 0) / 1 = x, -0.0 and inf kept) ---
def design(name: str, n: int, g: torch.Generator) -> torch.Tensor:
    lo, hi, _ = ranks(n, QUANTILE)
    if name == "ties_straddle":        # one run of equal keys covers rank lo AND rank hi: v_lo = v_hi = the tie, not "the next key"
        v = torch.rand(n, generator=g) * 0.5
        v[torch.randperm(n, generator=g)[: n - max(lo - 2, 0)]] = -2.25          # the largest n - lo + 2 keys are the tie
        return v
    if name == "hi_past_ties":         # the run of ties ends exactly at rank lo: v_hi is the smallest key above it (the second scan)
        if hi == lo:                   # (the rank is whole at this n: nothing lies past)
            return design("ties_straddle", n, g)
        srt = torch.cat([torch.full((lo + 1,), 1.5), 3.0 + torch.rand(n - lo - 1, generator=g)])
        return srt[torch.randperm(n, generator=g)] * (1 - 2 * torch.randint(0, 2, (n,), generator=g).float())
    if name == "all_equal":
        return torch.full((n,), -2.5)
    if name == "signed_zeros":         # +-0 only: every key is 0, q = 0, s = 1, out = +-0 / 1
        v = torch.zeros(n)
        v[::2] = -0.0
        return v
    if name == "infs":                 # +-inf among ordinary values, fewer than the tail above rank hi holds: ordinary (largest) keys
        v = torch.randn(n, generator=g) * 3
        v[0], v[n // 2] = float("inf"), float("-inf") if n - 1 - hi >= 2 else 3.0
        return v
    if name == "below_one":            # q < 1: s = 1, the output is x0 itself
        return torch.rand(n, generator=g) * 1.8 - 0.9
    if name == "normal":
        return torch.randn(n, generator=g) * 3
    raise KeyError(name)


DESIGNS = ["ties_straddle", "hi_past_ties", "all_equal", "signed_zeros", "infs", "below_one", "normal"]
SHAPES = [(4, 1, 8, 8), (4, 3, 16, 16), (4, 5, 24, 24)]      # per video: 256 (fewer keys than threads), 3072, 11520 (two 8192-key trips, the second partial)


# ---- the golden runs (tests/golden/make_golden_unipc.py): the reference's UniPC class, one video, tiny UNet, 3 frames @ 128x128 ---------
STEPS, GUIDANCE = 6, 9.0
CASES = {          # name -> (steps, guidance, strength, sampler keywords)
    "bh2": (6, 9.0, None, dict(variant="bh2")),
    "time_quadratic": (6, 9.0, None, dict(skip_type="time_quadratic")),
    "logSNR": (6, 9.0, None, dict(skip_type="logSNR")),
    "order2": (6, 9.0, None, dict(order=2)),
    "order1": (6, 9.0, None, dict(order=1)),
    "order2_bh2_2steps": (2, 9.0, None, dict(order=2, variant="bh2")),
    "no_lower_order_final": (6, 9.0, None, dict(lower_order_final=False)),
    "no_initial_corrector": (6, 9.0, None, dict(initial_corrector=False)),
    "denoise_to_zero": (6, 9.0, None, dict(denoise_to_zero=True)),
    "thresholding": (6, 9.0, None, dict(thresholding=True)),
    "thresholding_bh2_s07_dtz": (6, 9.0, 0.7, dict(thresholding=True, variant="bh2", denoise_to_zero=True)),
    "thresholding_unguided": (6, 1.0, None, dict(thresholding=True)),
}
THRESHOLDED = [k for k, v in CASES.items() if v[3].get("thresholding")]
# the cases whose UNet answers are stored for replay (<case>_eps): the file stays below modelscope_threshold_tiny.npz only with these —
# the thresholded runs, where q and s are compared per evaluation, and the 2-step run
REPLAYED = THRESHOLDED + ["order2_bh2_2steps"]


def evaluations(name):
    steps, _, _, kw = CASES[name]
    return steps + (1 if kw.get("denoise_to_zero") else 0)
