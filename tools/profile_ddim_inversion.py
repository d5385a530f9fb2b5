"""Time of the DDIM inversion record (T2V_OP_DDIM_STEP mode 3) and of one `DDIMSampler.encode` step beside one `decode` step.  Writes the
timing section of profiles/ddim_inversion.txt (or the file given as the first argument).  Reported only: nothing is gated on it.

Launch: the 24-frame latent 1x4x24x32x32 (and four videos of it), fp32 eps pair, guided — the inversion step with and without its kept
second destination beside the LDM DDIM update (mode 1) that `decode` launches; device events around 300 calls after 30 warm-up calls,
the variants alternated over three rounds (min..max of the rounds), beside a calibration GEMM of the box.
Step: the tiny UNet (oracle/configs.py:TINY_UNET, synthetic weights) on the same latent, scale 9, a 20-step schedule: 20 encode steps
and the 20 decode steps that walk them back, wall time per step between two device synchronisations, three rounds.
Usage: python tools/profile_ddim_inversion.py [out.txt]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from oracle import configs, synth, torch_port as tp  # noqa: E402
from sd_webui_text2video_amd import samplers as S, unet as U  # noqa: E402

DEV = "cuda:0"
LATENTS = [(1, 4, 24, 32, 32), (4, 4, 24, 32, 32)]


def timed(fn, iters=300, warm=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ddim_inversion.txt")
    rows = []

    def say(s):
        print(s, flush=True)
        rows.append(s)

    a = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    b = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    cal = timed(lambda: torch.matmul(a, b), 50, 10)
    say(f"calibration GEMM 4096^3 fp16 (torch.matmul): {cal:.1f} us = {2 * 4096 ** 3 / cal / 1e6:.0f} TFLOP/s")
    for shape in LATENTS:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(shape, generator=g).to(DEV)
        eps = torch.randn((2 * shape[0],) + shape[1:], generator=g).to(DEV)
        out, keep = torch.empty_like(x), torch.empty_like(x)
        coef1 = [0.6, 0.8, 0.9, 0.4, 0.0, 9.0]
        variants = (("mode 3", lambda: S._ddim_invert(out, x, eps, (0.9, 0.4, 9.0), True)),
                    ("mode 3 + kept copy", lambda: S._ddim_invert(out, x, eps, (0.9, 0.4, 9.0), True, keep=keep)),
                    ("mode 1 (decode's update)", lambda: S._ddim_update(out, x, eps, None, coef1, shape[1], mode=1)))
        t = {}
        for _ in range(3):
            for name, fn in variants:
                t.setdefault(name, []).append(timed(fn))
        say(f"latent {shape}, n = {x.numel()}, us per call through the Python binding over three rounds: "
            + "; ".join(f"{k} {min(v):.1f}..{max(v):.1f}" for k, v in t.items()))
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    smp = S.Txt2VideoSampler(net, torch.device(DEV), betas=betas, sampler_name="DDIM")
    smp.progress = False
    g = torch.Generator().manual_seed(2)
    z0 = torch.randn(LATENTS[0], generator=g).to(DEV)
    c, uc = (torch.randn(1, 77, configs.TINY_UNET["context_dim"], generator=g).to(DEV) for _ in range(2))
    s, n = smp.sampler, 20
    s.make_schedule(n)
    kw = dict(unconditional_guidance_scale=9.0, unconditional_conditioning=uc)
    enc_t, dec_t = [], []
    for r in range(4):                                   # round 0 compiles and warms
        torch.cuda.synchronize(); t0 = time.perf_counter()
        enc, _ = s.encode(z0, c, n, model_timesteps="schedule", **kw)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        s.decode(enc, c, n, **kw)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        if r:
            enc_t.append((t1 - t0) / n * 1e3); dec_t.append((t2 - t1) / n * 1e3)
    say(f"tiny UNet, latent {LATENTS[0]}, scale 9, {n} steps, ms per step over three rounds: encode {min(enc_t):.3f}..{max(enc_t):.3f}; "
        f"decode {min(dec_t):.3f}..{max(dec_t):.3f}")
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
