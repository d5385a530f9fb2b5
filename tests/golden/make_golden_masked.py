"""Generate the masked-DDIM golden FROM THE REAL REFERENCE (run where oracle/ref_bootstrap.py finds the reference checkout).

    python tests/golden/make_golden_masked.py          # lvdm_masked_tiny.npz, seconds on a CPU

The reference's own UNetModel (openaimodel3d.py) and DDIMSampler (lvdm/samplers/ddim.py), unmodified, run the mask blend of
ddim.py:188-195 on the tiny LVDM config.  As in make_golden.py:lvdm the sampler is given a stand-in for LatentDiffusion exposing what
it reads from the model: ddpm3d.py itself cannot be imported (it needs pytorch_lightning, which is absent), so the stand-in's
`q_sample` is ddpm3d.py:283-286 restated on the reference's own `extract_into_tensor` (util.py:85-88) and the
DDPM.register_schedule buffers computed with the reference's make_beta_schedule.  The cases and their seeded inputs are those of
tests/masked_ref.py; `torch.manual_seed(GLOBAL_SEED)` precedes every run, because q_sample draws `randn_like(x0)` from the default
generator.  Stored per case: the output, the x0 and mask inputs, the t values q_sample saw, and for (a) the unmasked run's output."""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import masked_ref as MR  # noqa: E402
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    rb.bootstrap()
    om = importlib.import_module("videocrafter.lvdm.models.modules.openaimodel3d")
    vu = importlib.import_module("videocrafter.lvdm.models.modules.util")
    dd = importlib.import_module("videocrafter.lvdm.samplers.ddim")
    dd.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    net = om.UNetModel(**configs.TINY_LVDM_UNET).eval()
    synth.load_synth(net, seed=0)
    betas = vu.make_beta_schedule("linear", 1000, linear_start=configs.LVDM_SCHEDULE["linear_start"],
                                  linear_end=configs.LVDM_SCHEDULE["linear_end"])
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    seen = []

    def q_sample(x_start, t, noise=None):
        seen.append(t.tolist())
        noise = torch.randn_like(x_start) if noise is None else noise
        return (vu.extract_into_tensor(model.sqrt_alphas_cumprod, t, x_start.shape) * x_start +
                vu.extract_into_tensor(model.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    model = types.SimpleNamespace(num_timesteps=1000, betas=f32(betas), alphas_cumprod=f32(ac),
                                  alphas_cumprod_prev=f32(np.append(1.0, ac[:-1])), sqrt_alphas_cumprod=f32(np.sqrt(ac)),
                                  sqrt_one_minus_alphas_cumprod=f32(np.sqrt(1.0 - ac)), device=torch.device("cpu"),
                                  apply_model=lambda xx, tt, c, **kw: net(xx, tt, context=c), q_sample=q_sample)
    ctx = MR.inputs_tiny()[2]
    out = {}
    for name in MR.CASES:
        c = MR.case(name)
        nb = c["batch"]
        for masked in (True, False) if name == "a" else (True,):
            smp = dd.DDIMSampler(model)
            smp.noise_gen.manual_seed(MR.NOISE_GEN_SEED)
            torch.manual_seed(MR.GLOBAL_SEED)
            seen.clear()
            kw = dict(mask=c["mask"], x0=c["x0"]) if masked else {}
            if c["cfg"] != 1.0:
                kw.update(unconditional_guidance_scale=c["cfg"], unconditional_conditioning=ctx[1:2].repeat(nb, 1, 1))
            with torch.no_grad():
                x, _ = smp.sample(S=MR.STEPS, conditioning=ctx[0:1].repeat(nb, 1, 1), batch_size=nb, shape=list(MR.SHAPE), verbose=False,
                                  eta=c["eta"], x_T=c["x_T"], **kw)
            if masked:
                out[f"{name}_out"], out[f"{name}_x0"], out[f"{name}_mask"] = x.numpy(), c["x0"].numpy(), c["mask"].numpy()
                out[f"{name}_t"] = np.asarray(seen, dtype=np.int64)
            else:
                out[f"{name}_unmasked"] = x.numpy()
        print("case", name, out[f"{name}_out"].shape, float(out[f"{name}_out"].std()), out[f"{name}_t"].tolist())
    held = torch.from_numpy(out["a_out"])[:, :, 0:2]
    free = torch.from_numpy(out["a_out"])[:, :, 2:]
    print("(a) held frames vs x0, rel-L2:", float((held - MR.case("a")["x0"][:, :, 0:2]).norm() / MR.case("a")["x0"][:, :, 0:2].norm()))
    print("(a) free frames vs the unmasked run, rel-L2:", float((free - torch.from_numpy(out["a_unmasked"])[:, :, 2:]).norm() / free.norm()))
    np.savez_compressed(os.path.join(OUT, "lvdm_masked_tiny.npz"), **out)


if __name__ == "__main__":
    main()
