"""Generate tests/golden/modelscope_threshold_tiny.npz FROM THE REAL REFERENCE (run where the reference is mounted):

    python tests/golden/make_golden_threshold.py

The reference's own `GaussianDiffusion.sample` (gaussian_sampler.py:214-296, through oracle/ref_bootstrap.py) on the tiny UNet with the
inputs of make_golden.py:tiny — batch 1, 4 steps, guidance 9 — once per case of tests/x0_threshold_ref.py:CASES: percentile=0.995,
clamp=0.3, clamp=5.0, percentile=0.995 with a condition_fn, and plain.  `restrict_range_x0` is wrapped at run time (nothing of the
reference is changed or copied): per step the x0 that entered it and, for the percentile runs, the s it computed — the tensor
`torch.quantile` returned to it, read after the method's in-place `clamp_(1.0)`.  A forward hook on the UNet records what the sampler
gave it and what it answered: per step the x_t of the conditional call and the two predictions (conditional, unconditional) — the
tests replay them, so that a loop under test is compared with the reference's loop and not with another UNet's rounding.

Stored: <case>_out (the final latent), <case>_x0 [steps, ...] and <case>_s [steps] (restricted cases), <case>_xt [steps, ...] and
<case>_eps [steps, 2, ...] (the restricted cases; clamp50's are asserted equal to clamp03's and not stored twice)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402
import x0_threshold_ref as XR  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def inputs():
    """The draws of make_golden.py:tiny, in its order."""
    cfg = configs.TINY_UNET
    g = torch.Generator().manual_seed(5)
    torch.randn(2, 4, 3, 16, 16, generator=g); torch.randn(2, 7, cfg["context_dim"], generator=g); torch.randn(2, 4, 8, 8, generator=g)
    c = torch.randn(1, 7, cfg["context_dim"], generator=g)
    uc = torch.randn(1, 7, cfg["context_dim"], generator=g)
    return c, uc


def main():
    cfg = configs.TINY_UNET
    unet, betas = rb.build_reference_unet(cfg)
    synth.load_synth(unet, seed=0)
    ref = rb.bootstrap()
    c, uc = inputs()
    out = {}
    for name in XR.CASES:
        s = ref.samplers.Txt2VideoSampler(unet, torch.device("cpu"), betas=betas, sampler_name="DDIM_Gaussian")
        _, noise, shape = s.get_noise(1, 4, 3, 128, 128, seed=1234)
        smp = s.sampler
        x0s, ss = [], []
        inner = smp.restrict_range_x0

        def wrapped(percentile, x0, clamp=False):
            x0s.append(x0.clone())
            real_q, got = torch.quantile, []
            torch.quantile = lambda *a, **k: (got.append(real_q(*a, **k)), got[-1])[1]
            try:
                r = inner(percentile, x0, clamp=clamp)
            finally:
                torch.quantile = real_q
            if got:
                ss.append(got[0].clone())          # after the method's in-place clamp_(1.0): the s it divided by
            return r
        smp.restrict_range_x0 = wrapped
        seen = []
        hook = unet.register_forward_hook(lambda m, i, o: seen.append((i[0].clone(), i[1].clone(), o.clone())))
        torch.manual_seed(0)
        with torch.no_grad():
            x = smp.sample(x_T=noise.clone(), S=XR.STEPS, shape=shape, conditioning=c, unconditional_conditioning=uc,
                           unconditional_guidance_scale=XR.GUIDANCE, eta=0.0, **XR.case_kwargs(name))
        hook.remove()
        assert len(seen) == 2 * XR.STEPS and all(torch.equal(seen[2 * k][0], seen[2 * k + 1][0]) for k in range(XR.STEPS))
        assert [int(a[1]) for a in seen[::2]] == [751, 501, 251, 1]
        out[f"{name}_out"] = x.numpy()
        out[f"{name}_xt"] = torch.stack([seen[2 * k][0] for k in range(XR.STEPS)]).numpy()
        out[f"{name}_eps"] = torch.stack([torch.cat([seen[2 * k][2], seen[2 * k + 1][2]]) for k in range(XR.STEPS)]).numpy()
        if x0s:
            assert len(x0s) == XR.STEPS
            out[f"{name}_x0"] = torch.stack(x0s).numpy()
        if ss:
            assert len(ss) == XR.STEPS
            out[f"{name}_s"] = torch.cat(ss).numpy()
        print(name, float(x.std()), [float(v) for v in ss])
    # the conditions that make the cases mean something
    for name in ("percentile", "percentile_cond"):
        assert (out[f"{name}_s"] > 1).sum() * 2 >= XR.STEPS, (name, out[f"{name}_s"])
    for name in ("clamp03", "clamp50"):
        for k in range(XR.STEPS):
            frac = float((np.abs(out[f"{name}_x0"][k]) > 1).mean())
            assert frac >= 0.01, (name, k, frac)
    assert np.array_equal(out["clamp03_out"], out["clamp50_out"])
    assert not np.array_equal(out["clamp03_out"], out["plain_out"]) and not np.array_equal(out["percentile_out"], out["plain_out"])
    for k in ("xt", "eps"):
        assert np.array_equal(out[f"clamp03_{k}"], out[f"clamp50_{k}"])
        del out[f"clamp50_{k}"], out[f"plain_{k}"]
    np.savez_compressed(os.path.join(OUT, "modelscope_threshold_tiny.npz"), **out)


if __name__ == "__main__":
    main()
