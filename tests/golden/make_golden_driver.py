"""Generate the per-video driver golden FROM THE REAL REFERENCE (run where oracle/ref_bootstrap.py finds the reference checkout).

    python tests/golden/make_golden_driver.py          # lvdm_driver_tiny.npz, seconds on a CPU

The reference's own UNetModel (openaimodel3d.py) and DDIMSampler (lvdm/samplers/ddim.py), unmodified, make the three videos that the
loop of process_videocrafter.py:61-79 makes for batch_count = 3: one single-video `sample` per video with `noise_gen` seeded
seed + v (:70), eta = 1.0 (VideoCrafter's default), CFG 7.5, 4 steps, on the tiny LVDM config.  As in make_golden_masked.py the sampler
is given a stand-in for LatentDiffusion exposing what it reads from the model (ddpm3d.py needs pytorch_lightning, which is absent).
The start latents are given (`x_T`): the reference draws them on its device generator, whose stream differs between devices.
Stored: x_T [3, 4, 5, 8, 8], out [3, 4, 5, 8, 8] (video v from x_T[v] and seed + v), seed."""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frames_inputs as FI  # noqa: E402
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
    model = types.SimpleNamespace(num_timesteps=1000, betas=f32(betas), alphas_cumprod=f32(ac),
                                  alphas_cumprod_prev=f32(np.append(1.0, ac[:-1])), sqrt_alphas_cumprod=f32(np.sqrt(ac)),
                                  sqrt_one_minus_alphas_cumprod=f32(np.sqrt(1.0 - ac)), device=torch.device("cpu"),
                                  apply_model=lambda xx, tt, c, **kw: net(xx, tt, context=c))
    ctx, x_T = FI.driver_inputs()
    smp = dd.DDIMSampler(model)               # ONE sampler, reseeded per video, as the reference's loop has it
    outs = []
    for v in range(FI.VIDEOS):
        smp.noise_gen.manual_seed(FI.SEED + v)
        with torch.no_grad():
            x, _ = smp.sample(S=FI.STEPS, conditioning=ctx[0:1], batch_size=1, shape=list(FI.SHAPE), verbose=False, eta=FI.ETA,
                              x_T=x_T[v:v + 1], unconditional_guidance_scale=FI.CFG, unconditional_conditioning=ctx[1:2])
        outs.append(x)
        print("video", v, tuple(x.shape), float(x.std()))
    out = torch.cat(outs)
    print("video 1 vs video 0, rel-L2:", float((out[1] - out[0]).norm() / out[0].norm()))
    np.savez_compressed(os.path.join(OUT, "lvdm_driver_tiny.npz"), x_T=x_T.numpy(), out=out.numpy(), seed=np.int64(FI.SEED))


if __name__ == "__main__":
    main()
