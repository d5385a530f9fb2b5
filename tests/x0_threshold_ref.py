"""Torch restatement (fp32, sort-based) of the x0 restriction of T2V_OP_DDIM_STEP mode 0 (include/t2v_hip.h: i[8], i[9]) and the designed
inputs of its tests.  Everything here is the arithmetic of the reference's `restrict_range_x0` / `get_eps` (gaussian_sampler.py:110-120,
199-211) and of `torch.quantile` on fp32, written so that each intermediate is visible:

  measure(x0, p)      -> (s, q, v_lo, v_hi) per sample: rank = float32(p) * float32(n - 1) in fp32, the two order statistics from a sort,
                         torch.lerp of the two, s = max(q, 1); a NaN in the sample gives q = s = NaN
  restrict(x0, kind)  -> the three restrictions (none / clamp / threshold by s)
  step(...)           -> one restricted DDIM_Gaussian step in `test_samplers_cpu._ddim_update_cpu`'s operation order
"""
import numpy as np
import torch

F32 = torch.float32


def ranks(n: int, p: float):
    """-> (lo, hi, w): torch.quantile's rank arithmetic on an fp32 input — the product is rounded to fp32."""
    rank = np.float32(p) * np.float32(n - 1)
    lo = np.floor(rank)
    return int(lo), int(np.ceil(rank)), np.float32(rank - lo)


def measure(x0: torch.Tensor, p: float):
    """x0 [samples, ...] fp32 -> table [samples, 4] = {max(q, 1), q, v_lo, v_hi}."""
    flat = x0.reshape(x0.shape[0], -1).to(F32).abs()
    n = flat.shape[1]
    lo, hi, w = ranks(n, p)
    srt, _ = torch.sort(flat, dim=1)                       # NaNs sort last
    v_lo, v_hi = srt[:, lo].clone(), srt[:, hi].clone()
    q = torch.lerp(v_lo, v_hi, torch.tensor(w, dtype=F32))
    q = torch.where(torch.isnan(flat).any(dim=1), torch.full_like(q, float("nan")), q)
    s = q.clamp(min=1.0)                                   # s.clamp_(1.0): a NaN stays a NaN
    return torch.stack([s, q, v_lo, v_hi], dim=1)


def restrict(x0: torch.Tensor, kind: int, bound: float = 1.0, s: torch.Tensor = None):
    """kind 0 none, 1 clamp(x0, -bound, bound), 2 min(s, max(-s, x0)) / s with s [samples] (each sample its own s)."""
    if kind == 0:
        return x0
    if kind == 1:
        return x0.clamp(-np.float32(bound), np.float32(bound))
    sv = s.to(F32).view(-1, *((1,) * (x0.ndim - 1)))
    return torch.min(sv, torch.max(-sv, x0)) / sv


def x0_of(xt, eps_pair, coef, guided):
    """The x0 of a mode-0 step and f0 * x: guidance combine included, every operation rounded by itself."""
    f = [torch.tensor(c, dtype=F32) for c in coef]
    nb = xt.shape[0]
    e = eps_pair[0:nb].float()
    if guided:
        u = eps_pair[nb:2 * nb].float()
        e = torch.cat([u[:, :guided] + f[5] * (e[:, :guided] - u[:, :guided]), e[:, guided:]], dim=1)
    ax = f[0] * xt.float()
    return ax - f[1] * e, ax


def step(xt, eps_pair, noise, coef, guided, *, kind=0, bound=1.0, percentile=None, table=None, grad=None, sqrt_1mat=0.0):
    """One restricted DDIM_Gaussian step -> (x_{t-1}, table or None).  kind 2 with `percentile`: measure, then threshold; with `table`
    given instead, threshold by its column 0."""
    f = [torch.tensor(c, dtype=F32) for c in coef]
    x0, ax = x0_of(xt, eps_pair, coef, guided)
    if kind == 2 and table is None:
        table = measure(x0, percentile)
    x0 = restrict(x0, kind, bound, None if table is None else table[:, 0])
    eps = (ax - x0) / f[1]
    if grad is not None:
        eps = eps - torch.tensor(sqrt_1mat, dtype=F32) * grad.float()
        x0 = ax - f[1] * eps
    r = f[2] * x0 + f[3] * eps
    if noise is not None and float(f[4]) != 0.0:
        r = r + f[4] * noise
    return r, table


def restricted_step_cpu(out, xt, eps_pair, noise, coef, guided, *, percentile=None, table=None, bound=None, grad=None, sqrt_1mat=0.0):
    """Stand-in for samplers._ddim_restricted_step (same arguments): writes `out` and the table row."""
    kind = 2 if percentile is not None else 1 if bound is not None else 0
    r, tab = step(xt, eps_pair, noise, coef, guided, kind=kind, bound=bound if bound is not None else 1.0, percentile=percentile,
                  grad=grad, sqrt_1mat=sqrt_1mat)
    if tab is not None:
        table.copy_(tab)
    out.copy_(r)
    return out


# ---- designed inputs of the measure pass: name -> (builder(n, generator) -> flat fp32 [n], what a wrong kernel would return) -------
def _perm(v, g):
    return v[torch.randperm(v.numel(), generator=g)]


def design(name: str, n: int, g: torch.Generator) -> torch.Tensor:
    if name == "all_equal":            # every bin count is n in one bin: a select that loses the tie count returns 0 or garbage for v_hi
        return torch.full((n,), -2.5)
    if name == "all_zero":             # q = 0, s must be 1 (a kernel that divides by q gives NaN)
        return torch.zeros(n)
    if name == "below_one":            # every |x0| < 1: s is the clamp to 1, q the true quantile
        return torch.rand(n, generator=g) * 1.8 - 0.9
    if name == "ten_values":           # ten distinct values, heavy ties straddling lo / hi: a kernel that takes "the next key" for v_hi is wrong
        vals = torch.tensor([0.25, -0.5, 0.75, 1.0, -1.5, 2.0, 3.0, -4.0, 6.0, 8.0])
        return vals[torch.randint(0, 10, (n,), generator=g)]
    if name == "low_byte":             # keys differ only in the lowest mantissa byte: only the last digit pass separates them
        bits = 0x40490F00 + torch.randint(0, 256, (n,), generator=g, dtype=torch.int32)
        return _perm(bits.view(torch.float32) * (1 - 2 * torch.randint(0, 2, (n,), generator=g).float()), g)
    if name == "high_byte":            # keys differ only in the highest byte: only the first digit pass separates them
        bits = (torch.randint(1, 0x7F, (n,), generator=g, dtype=torch.int32) << 24) + 0x00123456
        return bits.view(torch.float32)
    if name == "denormals":            # denormals and -0.0: a kernel that flushes, or ranks -0.0 by its sign bit, is wrong
        bits = torch.randint(0, 0x00800000, (n,), generator=g, dtype=torch.int32)
        v = bits.view(torch.float32).clone()
        v[::3] = -0.0
        v[1::3] = -v[1::3]
        return v
    if name == "one_inf":              # one +inf: an ordinary (largest) key
        v = torch.randn(n, generator=g) * 3
        v[n // 2] = float("inf")
        return v
    if name == "one_nan":              # one NaN: s = q = NaN
        v = torch.randn(n, generator=g) * 3
        v[n // 3] = float("nan")
        return v
    if name == "normal":
        return torch.randn(n, generator=g) * 3
    raise KeyError(name)


DESIGNS = ["all_equal", "all_zero", "below_one", "ten_values", "low_byte", "high_byte", "denormals", "one_inf", "one_nan", "normal"]
MEASURE_SHAPES = [(4, 9), (3, 67), (4, 630), (6, 21967), (4, 24 * 32 * 32)]      # (C, inner): see tests/test_gpu_x0_threshold.py


# ---- the golden runs (tests/golden/make_golden_threshold.py) ---------------------------------------------------------------------
STEPS, GUIDANCE = 4, 9.0
CASES = {          # name -> sampler keywords
    "percentile": dict(percentile=0.995),
    "clamp03": dict(clamp=0.3),
    "clamp50": dict(clamp=5.0),
    "percentile_cond": dict(percentile=0.995, condition_fn="roll"),
    "plain": dict(),
}


def condition_roll(xt, t):
    return 0.1 * xt.roll(1, -1)


def case_kwargs(name):
    kw = dict(CASES[name])
    if kw.get("condition_fn") == "roll":
        kw["condition_fn"] = condition_roll
    return kw
