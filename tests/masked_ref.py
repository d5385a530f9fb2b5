"""Seeded inputs of the masked-DDIM cases (tests/golden/lvdm_masked_tiny.npz): shared by the generator
(tests/golden/make_golden_masked.py) and the CPU / GPU tests, and torch restatements of the blend's documented semantics
(include/t2v_hip.h, DDIM_STEP i[7] = 1)."""
import torch

NOISE_GEN_SEED = 123        # DDIMSampler.noise_gen (eta noise)
GLOBAL_SEED = 11            # torch.manual_seed before every sample call: the stream q_sample's randn_like draws from
STEPS = 4
SHAPE = (4, 5, 8, 8)        # the tiny LVDM latent [c, t, h, w]


def inputs_tiny():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 5, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(1, 4, 5, 8, 8, generator=g)
    return x, torch.tensor([801, 401]), ctx, x_T


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def case(name):
    """-> dict(batch, x_T, x0, mask, cfg, eta): (a) frames 0-1 held, guided, eta 0.3; (b) a soft full-shape mask, unguided, eta 0;
    (c) two videos and a spatial box, guided, eta 0."""
    x_T = inputs_tiny()[3]
    if name == "a":
        mask = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0]).view(1, 1, 5, 1, 1)
        return dict(batch=1, x_T=x_T, x0=_randn(31, 1, *SHAPE), mask=mask, cfg=7.5, eta=0.3)
    if name == "b":
        mask = torch.rand(1, *SHAPE, generator=torch.Generator().manual_seed(33))
        return dict(batch=1, x_T=x_T, x0=_randn(32, 1, *SHAPE), mask=mask, cfg=1.0, eta=0.0)
    if name == "c":
        mask = torch.zeros(1, 1, 1, 8, 8)
        mask[..., 2:6, 1:5] = 1.0
        return dict(batch=2, x_T=torch.cat([x_T, _randn(9, 1, *SHAPE)]), x0=_randn(34, 2, *SHAPE), mask=mask, cfg=7.5, eta=0.0)
    raise KeyError(name)


CASES = ("a", "b", "c")


def conditions(c, device="cpu"):
    """-> the keyword arguments of DDIMSampler.sample for a case (conditioning as the product's dict form)."""
    ctx = inputs_tiny()[2].to(device)
    kw = dict(S=STEPS, conditioning={"c_crossattn": [ctx[0:1].repeat(c["batch"], 1, 1)]}, batch_size=c["batch"], shape=list(SHAPE),
              verbose=False, eta=c["eta"], x_T=c["x_T"].to(device), mask=c["mask"].to(device), x0=c["x0"].to(device))
    if c["cfg"] != 1.0:
        kw.update(unconditional_guidance_scale=c["cfg"], unconditional_conditioning={"c_crossattn": [ctx[1:2].repeat(c["batch"], 1, 1)]})
    return kw


def blend_cpu(xn, known, mask, qnoise, qcoef):
    """known' = f6 * x0 + f7 * qnoise;  out = known' * mask + (1 - mask) * xn, every operation rounded to fp32 on its own."""
    f6, f7 = (torch.tensor(v, dtype=torch.float32) for v in qcoef)
    k = f6 * known.float()
    if qnoise is not None and float(f7) != 0.0:
        k = k + f7 * qnoise.float()
    m = mask.float()
    return k * m + (1.0 - m) * xn
