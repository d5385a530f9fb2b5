"""Generate tests/golden/context_windows.npz FROM THE REAL REFERENCE (run in the build container, CPU, a few seconds).

    python tests/golden/make_golden_context_windows.py

The reference has no context windows, but its samplers take any callable model(x, t, c) -> eps.  Here that callable
wraps the reference's own tiny UNetSD (oracle/ref_bootstrap.py): it evaluates the UNet once per window of the clip and blends the
windows' eps per frame in float64 — the schedule, batch order and weights of `samplers.ContextWindows`, written out again below.  The
callable goes to the reference's OWN samplers (DDIM_Gaussian, DDIM, UniPC), unchanged, so everything around the model evaluation is the
reference's arithmetic.

Geometry: 6 frames at 128 x 128 (latent 16 x 16), windows of 4 frames with overlap 2 (starts 0, 2), pyramid weights, 4 steps, CFG 9,
eta 0; one video per seed (1234 and 1235: the two videos of the batched GPU test).  Only latents are stored."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FRAMES, LENGTH, OVERLAP, STEPS, SCALE, SEEDS = 6, 4, 2, 4, 9.0, (1234, 1235)


def window_starts(frames, length, overlap):
    stride, out, s = length - overlap, [], 0
    while s + length < frames:
        out.append(s)
        s += stride
    if not out or out[-1] != frames - length:
        out.append(frames - length)
    return out


class WindowedModel:
    """model(x, t, c): the wrapped UNet on every window of x [b, 4, F, h, w], blended per frame in float64 with pyramid weights.
    Every other attribute is the UNet's (the samplers read and set schedule buffers on the model they are given)."""

    def __init__(self, unet):
        object.__setattr__(self, "unet", unet)
        object.__setattr__(self, "windows_seen", 0)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "unet"), name)

    def __call__(self, x, t, c):
        frames = x.shape[2]
        if frames <= LENGTH:
            return self.unet(x, t, c)
        acc = torch.zeros(x.shape, dtype=torch.float64)
        wsum = torch.zeros(frames, dtype=torch.float64)
        for s in window_starts(frames, LENGTH, OVERLAP):
            eps = self.unet(x[:, :, s:s + LENGTH].contiguous(), t, c).double()
            for j in range(LENGTH):
                w = float(min(j + 1, LENGTH - j))
                acc[:, :, s + j] += w * eps[:, :, j]
                wsum[s + j] += w
            object.__setattr__(self, "windows_seen", self.windows_seen + 1)
        return (acc / wsum.view(1, 1, -1, 1, 1)).to(x.dtype)


def conditioning():
    """The c / uc of tests/test_samplers_cpu.py::_inputs (the draws before them are the tiny golden's other inputs)."""
    g = torch.Generator().manual_seed(5)
    torch.randn(2, 4, 3, 16, 16, generator=g); torch.randn(2, 7, 1024, generator=g); torch.randn(2, 4, 8, 8, generator=g)
    return torch.randn(1, 7, 1024, generator=g), torch.randn(1, 7, 1024, generator=g)


def main():
    unet, betas = rb.build_reference_unet(configs.TINY_UNET)
    synth.load_synth(unet, seed=0)
    ref = rb.bootstrap()
    import samplers.uni_pc.sampler as ups          # (importable once the reference is bootstrapped)
    ups.UniPCSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)      # its buffers are pinned to "cuda"
    c, uc = conditioning()
    cpu = torch.device("cpu")
    out = {"starts": np.asarray(window_starts(FRAMES, LENGTH, OVERLAP), dtype=np.int32)}
    for seed in SEEDS:
        for name in ("DDIM_Gaussian", "DDIM", "UniPC"):
            model = WindowedModel(unet)
            s = ref.samplers.Txt2VideoSampler(model, cpu, betas=betas, sampler_name=name)
            if name == "DDIM":
                s.sampler.device = cpu                  # (pinned to "cuda" like UniPC's buffers)
            lat, noise, shape = s.get_noise(1, 4, FRAMES, 128, 128, seed=seed)
            ref.state.sampling_step = 0
            with torch.no_grad():
                x0 = s.sample_loop(steps=STEPS, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=lat,
                                   shape=shape, noise=noise, guidance_scale=SCALE, eta=0.0, sampler_name=name)
            assert model.windows_seen > 0 and tuple(x0.shape) == (1, 4, FRAMES, 16, 16)
            out[f"{name}_x0_{seed}"] = x0.numpy().astype(np.float32)
            print(name, seed, "windows evaluated:", model.windows_seen, "std", float(x0.std()))
    np.savez_compressed(os.path.join(OUT, "context_windows.npz"), **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
