"""Generate the VideoCrafter fixtures of clips longer than 32 frames FROM THE REAL REFERENCE (run in the build container).

    python tests/golden/make_golden_long.py

The reference's VideoCrafter path takes any frame count (its temporal attention clamps relative distances to
+-temporal_length); these fixtures pin the relative-position attention kernel of long clips (RELPOS_ATTN i[17] = 3)
end to end.  As in make_golden.py:lvdm, the reference's own UNetModel (openaimodel3d.py) and DDIMSampler
(lvdm/samplers/ddim.py) are imported read-only through oracle/ref_bootstrap.py on the seeded synthetic weights of
oracle/synth.py; only outputs are stored, inputs are re-derived from the seeds below.
    lvdm_tiny_40f.npz    TINY_LVDM_UNET, 40 frames at 8x8, b = 2: UNet eps, and x0 of a 4-step DDIM run (CFG 7.5, eta 0.3)
    lvdm_48f_16x16.npz   the released LVDM_UNET, 48 frames at 16x16, t = 500, 77 context tokens: UNet eps
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def lvdm_inputs_tiny(frames):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, frames, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(1, 4, frames, 8, 8, generator=g)
    return x, torch.tensor([801, 401]), ctx, x_T


def lvdm_inputs_full(frames, hw):
    g = torch.Generator().manual_seed(1234)
    return torch.randn(1, 4, frames, hw, hw, generator=g), torch.tensor([500]), torch.randn(1, 77, 768, generator=g)


def main():
    rb.bootstrap()
    om = importlib.import_module("videocrafter.lvdm.models.modules.openaimodel3d")
    vu = importlib.import_module("videocrafter.lvdm.models.modules.util")
    dd = importlib.import_module("videocrafter.lvdm.samplers.ddim")
    dd.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    net = om.UNetModel(**configs.TINY_LVDM_UNET).eval()
    synth.load_synth(net, seed=0)
    x, t, ctx, x_T = lvdm_inputs_tiny(40)
    with torch.no_grad():
        eps = net(x, t, context=ctx)
    betas = vu.make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    model = types.SimpleNamespace(num_timesteps=1000, betas=f32(betas), alphas_cumprod=f32(ac),
                                  alphas_cumprod_prev=f32(np.append(1.0, ac[:-1])), device=torch.device("cpu"),
                                  apply_model=lambda xx, tt, c, **kw: net(xx, tt, context=c))
    smp = dd.DDIMSampler(model)
    smp.noise_gen.manual_seed(123)
    with torch.no_grad():
        x0, _ = smp.sample(S=4, conditioning=ctx[0:1], batch_size=1, shape=list(x_T.shape[1:]), verbose=False,
                           unconditional_guidance_scale=7.5, unconditional_conditioning=ctx[1:2], eta=0.3, x_T=x_T)
    np.savez_compressed(os.path.join(OUT, "lvdm_tiny_40f.npz"), unet_eps=eps.numpy(), ddim_x0=x0.numpy())
    print("lvdm tiny 40f done", eps.std().item(), x0.std().item())
    net = om.UNetModel(**configs.LVDM_UNET).eval()
    synth.load_synth(net, seed=0)
    x, t, ctx = lvdm_inputs_full(48, 16)
    with torch.no_grad():
        eps = net(x, t, context=ctx)
    np.savez_compressed(os.path.join(OUT, "lvdm_48f_16x16.npz"), unet_eps=eps.numpy())
    print("lvdm 48f 16x16 done", eps.std().item())


if __name__ == "__main__":
    main()
