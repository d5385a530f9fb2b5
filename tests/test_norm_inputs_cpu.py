"""CPU: the adversarial norm inputs of tests/norm_inputs.py do what tests/test_gpu_norm_adversarial.py needs them to do, and every case's
program is right in layout and fencing before it meets a GPU.

For EVERY case the GPU file runs (the list is imported from tests/norm_inputs.py by both), on the inputs and the float64 reference alone:
  * the reference rounded to fp16 stays under 4e-4 per block — the fp16 tolerance of 1e-3 is not spent on the output format;
  * each mutation of the reference's statistics pushes blocks above 10 x the tightest tolerance the GPU file applies to the case
    (2e-5 where it checks hi + lo, 1e-3 otherwise):
      1. the statistics of block (i, g) taken from (i + 1, g) or from (i, g + 1): EVERY block;
      2. a marked row (the first, the last) left out of the sums, or counted twice (`marked` inputs): EVERY block of every instance;
      3. n off by one row, either way: the worst block — inv_n is one number per launch, all blocks move at once, and the GPU file
         asserts on the maximum over blocks;
      4. the parts of a sharded norm averaged without weighting by their rows: the worst block, for the same reason.
    LayerNorm rows (one row, one group) have no row to lose: 1. along the rows, and a 64-column piece left out of the sums (the unit a
    column tile of the cross-tile form could drop).
Then the case's program runs through the interpreter ALONE (no GPU) and `norm_inputs.verify` applies the GPU file's own checks: windows
finite, every fence element still NaN, stored tensors and casts bit-equal, per-block errors within the GPU tolerances."""
import pytest
import torch

import norm_inputs as N
from interp import Interp


def _above(p, what, mean_var, base, every):
    y = N.groupnorm_ref(p["X"], p["gamma"], p["beta"], p["n_inst"], p["groups"], N.EPS, p["silu"], mean_var)
    e = N.block_err(y, base, p["n_inst"], p["groups"])
    worst = float(e.min() if every else e.max())
    assert worst > 10 * p["tol"], (p["name"], what, worst, 10 * p["tol"])


def _prove(c, p):
    X, n_inst, groups = p["X"], p["n_inst"], p["groups"]
    M, C = X.shape
    rows, cpg = M // n_inst, C // groups
    base = N.groupnorm_ref(X, p["gamma"], p["beta"], n_inst, groups, N.EPS, p["silu"])
    s1, s2, n = N.group_sums(X, n_inst, groups)
    mean, var = N.mean_var_of(s1, s2, n)
    assert N.block_err(N.groupnorm_ref(X, p["gamma"], p["beta"], n_inst, groups, N.EPS, p["silu"], (mean, var)), base, n_inst, groups).max() < 1e-9
    if n_inst > 1:
        _above(p, "statistics of the next instance", (mean.roll(-1, 0), var.roll(-1, 0)), base, True)
    if groups > 1:
        _above(p, "statistics of the next group", (mean.roll(-1, 1), var.roll(-1, 1)), base, True)
    xv = X.view(n_inst, rows, groups, cpg)
    if groups == 1 and rows == 1:                  # LayerNorm rows
        piece = xv[:, 0, :, :64]
        _above(p, "a 64-column piece left out", N.mean_var_of(s1 - piece.sum(-1), s2 - (piece * piece).sum(-1), n), base, True)
        return
    if c["variant"] == "marked":
        for r in sorted({0, rows - 1}):
            r1, r2 = xv[:, r].sum(-1), (xv[:, r] ** 2).sum(-1)
            _above(p, f"row {r} left out", N.mean_var_of(s1 - r1, s2 - r2, n), base, True)
            _above(p, f"row {r} counted twice", N.mean_var_of(s1 + r1, s2 + r2, n), base, True)
    _above(p, "n one row long", N.mean_var_of(s1, s2, n + cpg), base, False)
    if rows > 1:
        _above(p, "n one row short", N.mean_var_of(s1, s2, n - cpg), base, False)
    if p["parts"]:
        m, q, off = 0.0, 0.0, 0
        for pr in p["parts"]:
            a, b2, k = N.group_sums(X[off: off + pr], 1, groups)
            m, q, off = m + a / k / len(p["parts"]), q + b2 / k / len(p["parts"]), off + pr
        _above(p, "parts averaged without their row counts", (m, (q - m * m).clamp_min(0.0)), base, False)


@pytest.mark.parametrize("c", N.CASES, ids=lambda c: c["id"])
def test_inputs_expose_the_mutations_and_the_program_passes_in_the_interpreter(c):
    b = N.build(c)
    assert b.probs and b.outs
    for p in b.probs:
        dt = torch.float16 if c.get("dt") == "f16" or c.get("dead") else torch.float32
        assert torch.isfinite(p["X"]).all() and torch.equal(p["X"], p["X"].to(dt).double()), "inputs must be representable in the input dtype"
        _prove(c, p)
    for o in b.outs:
        e = N.block_err(o["ref"].half().double(), o["ref"], o["n_inst"], o["groups"])
        assert float(e.max()) < N.TOL_ROUNDED, (c["id"], o["name"], float(e.max()))
    it = Interp(b.P, b.w, poison=False)
    b.init(it)
    it.run({})
    print(N.figures_line(b, N.verify(it, b)))


def test_the_inputs_are_what_the_docstring_says():
    mu, sigma = N.block_params("distinct", 3, 32, "f32", 5)
    assert mu.abs().max() <= 8 and mu.unique().numel() == mu.numel() and set(sigma.log2().flatten().tolist()) <= set(range(-3, 4))
    assert (sigma != sigma.roll(1, 0)).all() and (sigma != sigma.roll(1, 1)).all()
    x = N.gn_input("distinct", 3, 101, 320, 32, "f32", 5)
    s1, s2, n = N.group_sums(x, 3, 32)
    m, v = N.mean_var_of(s1, s2, n)
    assert torch.allclose(m, mu, atol=1e-5) and torch.allclose(v.sqrt(), sigma, rtol=1e-5)      # z is standardised: mu, sigma ARE the statistics
    xm = N.blocks(N.gn_input("marked", 3, 101, 320, 32, "f32", 5) - mu.repeat_interleave(10, 1).repeat_interleave(101, 0), 3, 32).view(3, 32, 101, 10)
    share = (xm ** 2).sum(-1) / (xm ** 2).sum((-1, -2))[..., None]
    assert (share[..., 0] > 0.15).all() and (share[..., -1] > 0.15).all() and float(share[..., 1:-1].max()) < 0.15
    for dt, ratio in (("f32", 32.0), ("f16", 8.0)):
        s1, s2, n = N.group_sums(N.gn_input("offset", 2, 37, 2560, 32, dt, 9), 2, 32)
        m, v = N.mean_var_of(s1, s2, n)
        assert torch.allclose(m / v.sqrt(), torch.full_like(m, ratio), rtol=2e-2)
