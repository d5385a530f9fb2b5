"""Shared by the DDIM inversion tests (CPU and GPU) and tests/golden/make_golden_inversion.py: the torch restatement of
T2V_OP_DDIM_STEP mode 3 (include/t2v_hip.h), the stand-in for `samplers._ddim_invert`, the inputs of the goldens and the constant-eps
model of the round-trip check.  No GPU and no reference needed to import it."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ddim_inversion_tiny.npz")
SHAPE = (1, 4, 3, 16, 16)
ROUNDTRIPS = ((4, 3), (4, 4), (20, 20))          # (S, n) of roundtrip_ref_rel, in its order
UCG_SCHEDULE = [9.0, 7.0, 5.0, 3.0]
TEMPERATURE = 0.5
NOISE_SEED = 0                                   # torch.manual_seed before the eta run: the per-step draws come from the global generator


def invert_step(x, eps_pair, cx, ce, g, guided, dtype=torch.float32):
    """Mode 3 in `dtype` arithmetic, the reference's statements (ddim/sampler.py:249-254) with the coefficients as fp32 values:
    e = e_u + g (e_c - e_u) over all channels when guided, else e_c;  out = cx x + ce e (both products, then the sum).
    x [S, C, ...]; eps_pair [2 S, C, ...] = [cond (S) | uncond (S)] (the second half is not touched when not guided)."""
    n = x.shape[0]
    f = lambda v: torch.tensor(float(np.float32(v)), dtype=dtype)
    e = eps_pair[:n].to(dtype)
    if guided:
        u = eps_pair[n:2 * n].to(dtype)
        e = u + f(g) * (e - u)
    return f(cx) * x.to(dtype) + f(ce) * e


def invert_cpu(out, x, eps_pair, coef, guided, keep=None):
    """What `samplers._ddim_invert` launches, in fp32 torch on the host."""
    assert x.dtype == torch.float32 and out.dtype == torch.float32
    r = invert_step(x, eps_pair, coef[0], coef[1], coef[2], guided)
    out.copy_(r)
    if keep is not None:
        keep.copy_(r)
    return out


def inputs(context_dim=1024):
    """z0 (seed 11), the start noise and c / uc (generator 5) of make_golden.py:other_samplers, in its order of draws."""
    from oracle import synth
    g = torch.Generator().manual_seed(5)
    torch.randn(2, 4, 3, 16, 16, generator=g); torch.randn(2, 7, context_dim, generator=g); torch.randn(2, 4, 8, 8, generator=g)
    c = torch.randn(1, 7, context_dim, generator=g)
    uc = torch.randn(1, 7, context_dim, generator=g)
    noise, _, _ = synth.synth_inputs(3, 128, 128)
    z0 = torch.randn(SHAPE, generator=torch.Generator().manual_seed(11))
    return z0, noise, c, uc


def const_eps():
    """The fixed eps of the constant-eps round trip."""
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(3))


class ConstEpsModel:
    """A model whose eps depends neither on x nor on t: with it decode(encode(x0, n), n) is the algebraic identity."""
    parameterization = "eps"
    num_timesteps = 1000

    def __init__(self, eps, device="cpu"):
        self.eps = eps.to(device)
        self.device = torch.device(device)
        self.calls = []

    def __call__(self, x, t, c):
        self.calls.append((x.shape[0], [float(v) for v in t.reshape(-1).tolist()]))
        return self.eps.expand(x.shape[0], *self.eps.shape[1:]).clone()


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())
