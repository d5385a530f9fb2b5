"""Generate tests/golden/freeu_tiny.npz FROM THE REAL REFERENCE (run where the reference is mounted; seconds on a CPU):

    python tests/golden/make_golden_freeu.py

FreeU (Si et al.) on the reference's own tiny UNetSD (through oracle/ref_bootstrap.py, synthetic weights of oracle/synth.py, seed 0):
a forward pre-hook on the first ResBlock of every `output_blocks[j]` splits its input — the reference's torch.cat([x, xs.pop()], dim=1),
t2v_model.py:444 — at the stream width and applies the torch.fft formulation of tests/freeu_ref.py in fp32 (the channel-keyed rule:
4 dim -> b1 / s1, 2 dim -> b2 / s2).  Nothing of the reference is changed or copied.  Stored:
  eps_64     the forward of 2 samples x 3 frames at 64 x 64 px (latent 8 x 8: the levels are 8^2, 4^2, 2^2, 1^2), inputs of make_golden.py:tiny cut to 8 x 8
  eps_odd    the forward of 1 sample x 2 frames on a 40 x 72 latent (levels 40 x 72, 20 x 36, 10 x 18, 5 x 9: odd sizes at the lowest)
  latents    3 steps of the reference's own DDIM_Gaussian sampler around that UNet (guidance 9, eta 0, 1 x 4 x 3 x 16 x 16)
  plain_*    the same three without the hooks (what the FreeU results must differ from)
  freeu      the values used, b1 b2 s1 s2
The FreeU results differ from the plain ones by at least 10 x the forward gate of the tests (4e-3 rel-L2): asserted here."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402
import freeu_ref as FR  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FORWARD_GATE = 4e-3
STEPS = 3


def inputs(cfg):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 3, 16, 16, generator=g)
    y = torch.randn(2, 7, cfg["context_dim"], generator=g)
    g2 = torch.Generator().manual_seed(17)
    x_odd = torch.randn(1, 4, 2, 40, 72, generator=g2)
    c = torch.randn(1, 7, cfg["context_dim"], generator=g2)
    uc = torch.randn(1, 7, cfg["context_dim"], generator=g2)
    return x[:, :, :, :8, :8].contiguous(), y, torch.tensor([801, 401]), x_odd, c, uc


def stream_widths(cfg):
    """Channels of the stream that enters decoder block j (the reference's constructor loop, t2v_model.py:148-318)."""
    dim, mult, nrb = cfg["dim"], list(cfg["dim_mult"]), cfg["num_res_blocks"]
    dec = [dim * u for u in [mult[-1]] + mult[::-1]]
    widths = []
    for i, (cin, cout) in enumerate(zip(dec[:-1], dec[1:])):
        for j in range(nrb + 1):
            widths.append(cin)
            cin = cout
    return widths


def rel(a, b):
    return float((a - b).norm() / b.norm())


def main():
    cfg = configs.TINY_UNET
    unet, betas = rb.build_reference_unet(cfg)
    synth.load_synth(unet, seed=0)
    ref = rb.bootstrap()
    x, y, t, x_odd, c, uc = inputs(cfg)
    widths = stream_widths(cfg)
    assert len(widths) == len(unet.output_blocks)
    values = dict(FR.MODELSCOPE)

    def run():
        with torch.no_grad():
            e64 = unet(x, t, y)
            eodd = unet(x_odd, torch.tensor([601]), c)
            s = ref.samplers.Txt2VideoSampler(unet, torch.device("cpu"), betas=betas, sampler_name="DDIM_Gaussian")
            lat, noise, shape = s.get_noise(1, 4, 3, 128, 128, seed=1234)
            lat = s.sample_loop(steps=STEPS, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=lat,
                                shape=shape, noise=noise, guidance_scale=9.0, eta=0.0, sampler_name="DDIM_Gaussian")
        return e64, eodd, lat

    plain = run()
    for attempt in range(4):
        handles = FR.apply_to_reference_unet(unet, widths, cfg["dim"], values)
        assert len(handles) == sum(w in (4 * cfg["dim"], 2 * cfg["dim"]) for w in widths)
        got = run()
        for h in handles:
            h.remove()
        moved = [rel(a, b) for a, b in zip(got, plain)]
        print("freeu", values, "moves the results by", moved)
        if min(moved[:2]) >= 10 * FORWARD_GATE:
            break
        # the authors' values do not move the synthetic-weight forward far enough: stronger ones (recorded in the file)
        values = {"b1": values["b1"] + 0.3, "b2": values["b2"] + 0.3, "s1": values["s1"] - 0.3, "s2": max(values["s2"] - 0.1, 0.0)}
    assert min(moved[:2]) >= 10 * FORWARD_GATE, moved
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(again, plain)), "the hooks were not removed"
    np.savez_compressed(os.path.join(OUT, "freeu_tiny.npz"), eps_64=got[0].numpy(), eps_odd=got[1].numpy(), latents=got[2].numpy(),
                        plain_64=plain[0].numpy(), plain_odd=plain[1].numpy(), plain_latents=plain[2].numpy(),
                        freeu=np.array([values[k] for k in ("b1", "b2", "s1", "s2")], dtype=np.float64))


if __name__ == "__main__":
    main()
