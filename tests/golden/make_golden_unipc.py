"""Generate tests/golden/unipc_options_tiny.npz FROM THE REAL REFERENCE (run where the reference is mounted):

    python tests/golden/make_golden_unipc.py

The reference's own `UniPC` class (uni_pc/uni_pc.py:314-743, through oracle/ref_bootstrap.py) with the options its wrapper hard-codes
away (uni_pc/sampler.py:77-88) set per case of tests/unipc_ref.py:CASES, on the tiny UNet with the inputs of make_golden.py:tiny —
one video, 3 frames @ 128x128, the noise of seed 1234.  The class is constructed exactly as the wrapper constructs it (NoiseScheduleVP
'discrete' on the fp32 alphas_cumprod, model_wrapper with classifier-free guidance); nothing of the reference is changed or copied.
A forward hook on the UNet records what it answered at every evaluation (conditional, then unconditional; one answer at guidance 1),
and `torch.quantile` is wrapped for the duration of a run: per thresholded evaluation the q it returned.

Stored: c, uc, noise; <case>_out (the final latent); for the cases of unipc_ref.REPLAYED <case>_eps [evaluations, 2 | 1, ...] and
<case>_t [evaluations] (the timestep the UNet was given); for the thresholded cases <case>_q and <case>_s [evaluations]."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402
import unipc_ref as UR  # noqa: E402

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
    import samplers.uni_pc.sampler as ups
    import samplers.uni_pc.uni_pc as up
    ups.UniPCSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)      # (its buffers are pinned to "cuda")
    c, uc = inputs()
    cpu = torch.device("cpu")
    s = ref.samplers.Txt2VideoSampler(unet, cpu, betas=betas, sampler_name="UniPC")
    _, noise, shape = s.get_noise(1, 4, 3, 128, 128, seed=1234)
    out = {"c": c.numpy(), "uc": uc.numpy(), "noise": noise.numpy()}
    for name, (steps, guidance, strength, kw) in UR.CASES.items():
        ref.state.sampling_step = 0
        ns = up.NoiseScheduleVP("discrete", alphas_cumprod=s.sampler.alphas_cumprod)
        model_fn = up.model_wrapper(lambda x, t, cc: unet(x, t, cc), ns, model_type="noise", guidance_type="classifier-free",
                                    condition=c, unconditional_condition=uc, guidance_scale=guidance)
        solver = up.UniPC(model_fn, ns, predict_x0=True, thresholding=kw.get("thresholding", False), variant=kw.get("variant", "bh1"))
        seen, qs = [], []
        hook = unet.register_forward_hook(lambda m, i, o: seen.append((float(i[1].reshape(-1)[0]), o.clone())))
        real_q = torch.quantile
        torch.quantile = lambda *a, **k: (qs.append(real_q(*a, **k).clone()), qs[-1])[1]
        try:
            with torch.no_grad():
                x = solver.sample(noise.clone(), steps=steps, t_start=strength, skip_type=kw.get("skip_type", "time_uniform"),
                                  method="multistep", order=kw.get("order", 3), lower_order_final=kw.get("lower_order_final", True),
                                  initial_corrector=kw.get("initial_corrector", True), denoise_to_zero=kw.get("denoise_to_zero", False))
        finally:
            torch.quantile = real_q
            hook.remove()
        per = 1 if guidance == 1.0 else 2
        evals = UR.evaluations(name)
        assert len(seen) == per * evals, (name, len(seen))
        assert torch.isfinite(x).all()
        out[f"{name}_out"] = x.numpy()
        if name in UR.REPLAYED:
            out[f"{name}_eps"] = torch.stack([torch.cat([seen[per * k + j][1] for j in range(per)]) for k in range(evals)]).numpy()
            out[f"{name}_t"] = np.asarray([seen[per * k][0] for k in range(evals)], dtype=np.float64)
        if kw.get("thresholding"):
            assert len(qs) == evals
            q = torch.cat([v.reshape(-1) for v in qs])
            out[f"{name}_q"] = q.numpy()
            out[f"{name}_s"] = q.clamp(min=1.0).numpy()
            assert (q > 1).any(), (name, q)            # otherwise max(q, 1) hides the quantile
        print(name, float(x.std()), [round(float(v), 4) for v in qs])
    ref_out = out["bh2_out"]
    for name in UR.CASES:                              # every option changes the result
        if name != "bh2":
            assert not np.array_equal(out[f"{name}_out"], ref_out), name
    path = os.path.join(OUT, "unipc_options_tiny.npz")
    np.savez_compressed(path, **out)
    limit = os.path.getsize(os.path.join(OUT, "modelscope_threshold_tiny.npz"))
    assert os.path.getsize(path) < limit, (os.path.getsize(path), limit)
    print(os.path.getsize(path), "bytes; limit", limit)


if __name__ == "__main__":
    main()
