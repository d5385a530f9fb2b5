"""Generate the depth-adapter goldens FROM THE REAL REFERENCE (run where oracle/ref_bootstrap.py finds the reference checkout).

    python tests/golden/make_golden_adapter.py            # all four cases (the released-size UNet forward takes minutes on a CPU)
    python tests/golden/make_golden_adapter.py --small    # cases 1-3 only

Outputs of the reference's own Adapter (lvdm/models/modules/adapter.py), UNetModel.forward(features_adapter=) (openaimodel3d.py) and
DDIMSampler (lvdm/samplers/ddim.py), imported read-only through oracle/ref_bootstrap.py, on the seeded weights of oracle/synth.py and
the seeded inputs of tests/adapter_ref.py:
  lvdm_adapter_small.npz   case 1: Adapter(channels=[32, 64, 64]) on 5 raw depth frames of 64 x 48, normalised per frame, for the three
                           option sets the reference can run; the state-dict keys / shapes of those and of the released shape
  lvdm_adapter_tiny.npz    cases 2, 3: TINY_LVDM_UNET forward with one feature (a batch of two, and the [cond | uncond] form on one x),
                           and the 4-step DDIM loop (CFG 7.5, eta 0.3, generator seed 123) with it
  lvdm_adapter_16f.npz     case 4: LVDM_UNET forward, 16 frames @ 32 x 32, with the features of the 77 M-parameter adapter on a
                           seeded depth clip; eps and strided samples of the features (adapter_ref.STRIDES)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adapter_ref as AR  # noqa: E402
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEED_ADAPTER = 11


def modules():
    rb.bootstrap()
    ad = importlib.import_module("videocrafter.lvdm.models.modules.adapter")
    om = importlib.import_module("videocrafter.lvdm.models.modules.openaimodel3d")
    vu = importlib.import_module("videocrafter.lvdm.models.modules.util")
    dd = importlib.import_module("videocrafter.lvdm.samplers.ddim")
    dd.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    return ad, om, vu, dd


def normalise(d):
    """get_batch_depth's normalisation (ddpm3d.py:1463-1464; that module needs pytorch_lightning and cannot be imported): the same two
    lines, frame by frame as its encode_bs = 1 loop runs them."""
    out = []
    for x in torch.split(d, 1, dim=0):
        lo, hi = torch.amin(x, dim=[1, 2, 3], keepdim=True), torch.amax(x, dim=[1, 2, 3], keepdim=True)
        out.append(2. * (x - lo) / (hi - lo + 1e-7) - 1.)
    return torch.cat(out, dim=0)


def small(ad):
    depth = AR.small_depth()
    out = dict(depth=depth.numpy(), depth_norm=normalise(depth).numpy())
    for name, opts in AR.OPTION_SETS.items():
        net = ad.Adapter(**AR.SMALL, **opts).eval()
        synth.load_synth(net, seed=SEED_ADAPTER)
        with torch.no_grad():
            feats = net(normalise(depth))
        for k, f in enumerate(feats):
            out[f"{name}_feat{k}"] = f.numpy()
        sd = net.state_dict()
        out[f"{name}_keys"] = np.array(list(sd.keys()))
        out[f"{name}_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        rel = ad.Adapter(channels=AR.RELEASED["channels"], cin=64, **opts)
        sd = rel.state_dict()
        out[f"{name}_released_keys"] = np.array(list(sd.keys()))
        out[f"{name}_released_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        out[f"{name}_released_params"] = np.array(sum(p.numel() for p in rel.parameters()))
        del rel
    np.savez_compressed(os.path.join(OUT, "lvdm_adapter_small.npz"), **out)
    print("adapter small done", {k: v.shape for k, v in out.items() if "feat" in k})


def tiny(om, vu, dd):
    cfg = configs.TINY_LVDM_UNET
    net = om.UNetModel(**cfg).eval()
    synth.load_synth(net, seed=0)
    g = torch.Generator().manual_seed(7)                       # tests/test_gpu_videocrafter.py::_inputs_tiny
    x = torch.randn(2, 4, 5, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(1, 4, 5, 8, 8, generator=g)
    t = torch.tensor([801, 401])
    feat = AR.tiny_feature()
    with torch.no_grad():
        eps = net(x, t, context=ctx, features_adapter=[feat])
        # the [cond | uncond] batch of a guided step: one x_t, one t, two contexts, ONE feature for both roles
        pair = net(torch.cat([x[0:1]] * 2), torch.tensor([801, 801]), context=ctx, features_adapter=[feat[0:1]])
    betas = vu.make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    model = types.SimpleNamespace(num_timesteps=1000, betas=f32(betas), alphas_cumprod=f32(ac),
                                  alphas_cumprod_prev=f32(np.append(1.0, ac[:-1])), device=torch.device("cpu"),
                                  apply_model=lambda xx, tt, c, **kw: net(xx, tt, context=c, **kw))
    smp = dd.DDIMSampler(model)
    smp.noise_gen.manual_seed(123)
    with torch.no_grad():
        x0, _ = smp.sample(S=4, conditioning=ctx[0:1], batch_size=1, shape=list(x_T.shape[1:]), verbose=False,
                           unconditional_guidance_scale=7.5, unconditional_conditioning=ctx[1:2], eta=0.3, x_T=x_T,
                           features_adapter=[feat[0:1]])
    np.savez_compressed(os.path.join(OUT, "lvdm_adapter_tiny.npz"), feature=feat.numpy(), unet_eps=eps.numpy(), unet_eps_pair=pair.numpy(),
                        ddim_x0=x0.numpy())
    print("adapter tiny done", eps.std().item(), pair.std().item(), x0.std().item())


def released(ad, om):
    adapter = ad.Adapter(**AR.RELEASED).eval()
    synth.load_synth(adapter, seed=SEED_ADAPTER)
    depth = AR.released_depth()
    b, _, t, h, w = depth.shape
    with torch.no_grad():
        feats = adapter(normalise(depth.permute(0, 2, 1, 3, 4).reshape(b * t, 1, h, w)))
    del adapter
    net = om.UNetModel(**configs.LVDM_UNET).eval()
    synth.load_synth(net, seed=0)
    g = torch.Generator().manual_seed(1234)                    # test_released_config_forward_matches_reference_golden
    x = torch.randn(1, 4, 16, 32, 32, generator=g)
    ctx = torch.randn(1, 77, 768, generator=g)
    with torch.no_grad():
        eps = net(x, torch.tensor([500]), context=ctx, features_adapter=[f.reshape(b, t, *f.shape[1:]).permute(0, 2, 1, 3, 4) for f in feats])
    out = dict(unet_eps=eps.numpy())
    for k, f in enumerate(feats):
        out[f"feat{k}"] = AR.subsample(f).contiguous().numpy()
    np.savez_compressed(os.path.join(OUT, "lvdm_adapter_16f.npz"), **out)
    print("adapter 16f done", eps.std().item(), [tuple(f.shape) for f in feats])


if __name__ == "__main__":
    ad, om, vu, dd = modules()
    torch.manual_seed(0)
    if "--released-only" not in sys.argv:
        small(ad)
        tiny(om, vu, dd)
    if "--small" not in sys.argv:
        released(ad, om)
