"""Generate tests/golden/modelscope_inpaint_tiny.npz FROM THE REAL REFERENCE (run where the reference is mounted):

    python tests/golden/make_golden_inpaint.py

The reference's legacy loop `GaussianDiffusion.ddim_sample_loop` (modelscope/t2v_model.py:1460-1577, reached through
oracle/ref_bootstrap.py) — the loop whose keyframe blend works — on the tiny UNet, once per case of tests/keyframe_inputs.py:CASES.
Nothing of the reference is changed or copied; two things about it decide how it is called:
  * the class is built with var_type="fixed_small": with its default "learned_range" `p_mean_variance` raises UnboundLocalError
    (t2v_model.py:1368).  "fixed_small" means guidance over all channels;
  * the loop casts the contexts to fp16 (:1538-1539): the model is wrapped as `unet(xt, t, y.float())` and the contexts are
    fp16-representable.
`torch.randn_like` is wrapped at run time and every draw recorded; `ddim_sample` is wrapped to record the x_t that enters every step
(after the initial add_noise, then after every blend).

Stored per case: <case>_out (the final latent), <case>_latents and <case>_mask (the inputs), <case>_noise [S, ...] (row 0 = n0,
row i + 1 = the blend noise after step i: the layout of `inpaint_noise=`; masked cases), <case>_eta [S, ...] (the eta draws, where
eta != 0: they enter nothing otherwise) and <case>_xt [S, ...] (the x_t that entered step i); once for all cases: c, uc (fp16)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402
import keyframe_inputs as KI  # noqa: E402


def main():
    unet, betas = rb.build_reference_unet(configs.TINY_UNET)
    synth.load_synth(unet, seed=0)
    ref = rb.bootstrap()
    model = lambda xt, t, y: unet(xt, t, y.float())
    out = {}
    for name, (S, eta, _) in KI.CASES.items():
        latents, mask, c, uc = KI.case_inputs(name)
        diff = ref.t2v.GaussianDiffusion(betas, var_type="fixed_small")
        draws, xts = [], []
        real_randn_like, real_step = torch.randn_like, diff.ddim_sample
        torch.randn_like = lambda *a, **k: (draws.append(real_randn_like(*a, **k)), draws[-1])[1]
        diff.ddim_sample = lambda xt, *a, **k: (xts.append(xt.clone()), real_step(xt, *a, **k))[1]
        torch.manual_seed(KI.SEED)
        try:
            x = diff.ddim_sample_loop(latents.clone(), model, c=c, uc=uc, guide_scale=KI.GUIDANCE, ddim_timesteps=S, eta=eta,
                                      mask=None if mask is None else mask.clone())
        finally:
            torch.randn_like = real_randn_like
        assert len(xts) == S, (name, len(xts))               # num_timesteps % S == 0: the loop walks S entries
        out[f"{name}_out"] = x.numpy()
        out[f"{name}_xt"] = torch.stack(xts).numpy()
        out[f"{name}_latents"] = latents.numpy()
        for k, v in (("c", c), ("uc", uc)):                 # the same contexts in every case, fp16-representable: stored once, as fp16
            assert torch.equal(v, v.half().float())
            assert k not in out or np.array_equal(out[k], v.half().numpy())
            out[k] = v.half().numpy()
        if mask is None:
            assert len(draws) == S
        else:
            # n0, then per step the eta draw and (all steps but the last) the blend draw
            assert len(draws) == 2 * S, (name, len(draws))
            out[f"{name}_mask"] = mask.numpy()
            out[f"{name}_noise"] = torch.stack([draws[0]] + [draws[2 + 2 * i] for i in range(S - 1)]).numpy()
            if eta != 0.0:
                out[f"{name}_eta"] = torch.stack([draws[1 + 2 * i] for i in range(S)]).numpy()
            assert torch.equal(xts[0], diff.add_noise(latents, draws[0], 1 + (S - 1) * (1000 // S)))
        print(name, "std", float(x.std()), "max", float(x.abs().max()))
    # the conditions that make the cases mean something
    lat = torch.from_numpy(out["frames_eta0_latents"])
    for name in ("frames_eta0", "frames_eta1"):
        x = torch.from_numpy(out[f"{name}_out"])
        held, free = float((x[:, :, 0] - lat[:, :, 0]).abs().max()), float((x[:, :, 4] - lat[:, :, 4]).abs().max())
        print(name, "weight-0 frame against the image latent:", held, " weight-1 frame:", free)
        assert held < 0.5 < free, (name, held, free)
        assert not np.array_equal(out[f"{name}_out"], out["plain_out"])
    assert not np.array_equal(out["frames_eta0_out"], out["frames_eta1_out"])
    m = out["spatial_mask"]
    assert len(np.unique(m[0, 0, 2])) > 8                     # the mask varies inside a frame
    np.savez_compressed(KI.GOLD, **out)
    print("wrote", KI.GOLD, os.path.getsize(KI.GOLD), "bytes")


if __name__ == "__main__":
    main()
