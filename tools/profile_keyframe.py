"""Time of the keyframe record (T2V_OP_DDIM_STEP mode 4) beside the plain mode-0 record, and the end-to-end errors of
tests/test_gpu_keyframe.py.  Writes the measured section of profiles/keyframe_inpaint.txt (or the file given as the first argument).
Reported only: nothing is gated on the timing.

Launch: the deployed latent 1x4x24x32x32, fp32 eps pair, 2 of 4 channels guided, with eta noise; device events around 300 calls after
30 warm-up calls, the two records alternated over five rounds (min..max of the rounds), beside a calibration GEMM of the box.
Bytes per element: the plain record reads x, both eps halves (the guided channels: half of them) and the eta noise and writes out; mode 4
reads the original latent, the mask and the blend noise as well.
Usage: python tools/profile_keyframe.py [out.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import keyframe_inputs as KI  # noqa: E402
from oracle import configs, synth, torch_port as tp  # noqa: E402
from sd_webui_text2video_amd import samplers as S, unet as U  # noqa: E402

DEV = "cuda:0"
LATENT = (1, 4, 24, 32, 32)


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keyframe_inpaint.txt")
    rows = []

    def say(s):
        print(s, flush=True)
        rows.append(s)

    a = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    b = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    cal = timed(lambda: torch.matmul(a, b), 50, 10)
    say(f"calibration GEMM 4096^3 fp16 (torch.matmul): {cal:.1f} us = {2 * 4096 ** 3 / cal / 1e6:.0f} TFLOP/s")
    g = torch.Generator().manual_seed(1)
    x, noise, orig, qn = (torch.randn(LATENT, generator=g).to(DEV) for _ in range(4))
    mask = torch.rand(LATENT, generator=g).to(DEV)
    eps = torch.randn((2,) + LATENT[1:], generator=g).to(DEV)
    out = torch.empty_like(x)
    coef = list(KI.COEF)
    variants = (("mode 0 (plain)", lambda: S._ddim_update(out, x, eps, noise, coef, 2, 0)),
                ("mode 4 (keyframe)", lambda: S._ddim_update_keyframe(out, x, eps, noise, coef, 2, orig, mask, qn, KI.QCOEF, 0.5)))
    t = {}
    for _ in range(5):
        for name, fn in variants:
            t.setdefault(name, []).append(timed(fn))
    plain_b, key_b = 4 * (1 + 1.5 + 1 + 1), 4 * (1 + 1.5 + 1 + 1 + 3)
    say(f"latent {LATENT}, n = {x.numel()}, fp32 eps, 2 of 4 channels guided, eta noise; us per call through the Python binding over five "
        "alternated rounds: " + "; ".join(f"{k} {min(v):.2f}..{max(v):.2f} (median {float(np.median(v)):.2f})" for k, v in t.items()))
    say(f"bytes per element: plain {plain_b:.0f}, keyframe {key_b:.0f}: expected ratio {key_b / plain_b:.2f}; measured ratio of the medians "
        f"{float(np.median(t['mode 4 (keyframe)'])) / float(np.median(t['mode 0 (plain)'])):.2f}")

    # the end-to-end errors the GPU test gates (rel-L2 against the goldens of the reference's legacy loop)
    gold = dict(np.load(KI.GOLD))
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    S.available_samplers[0].register_buffers_to_model(net, betas, torch.device(DEV))
    d = S.GaussianDiffusion(net, betas, var_type="fixed_small")
    r = {}
    for name, (steps, eta, kind) in KI.CASES.items():
        if eta != 0.0:
            continue
        latents, m, c, uc = KI.case_inputs(name)
        kw = {} if kind is None else dict(mask=m.to(DEV), inpaint="legacy", inpaint_noise=torch.from_numpy(gold[f"{name}_noise"]).to(DEV))
        got = d.sample(x_T=latents.to(DEV), S=steps, shape=tuple(latents.shape), conditioning=c.to(DEV), unconditional_conditioning=uc.to(DEV),
                       unconditional_guidance_scale=KI.GUIDANCE, eta=eta, **kw).cpu().double()
        want = torch.from_numpy(gold[f"{name}_out"]).double()
        r[name] = float((got - want).norm() / want.norm())
    say("tiny UNet, rel-L2 against the reference golden: " + " ".join(f"{k} {v:.3e}" for k, v in r.items())
        + f"; gate of the masked cases 1.5 x plain = {1.5 * r['plain']:.3e}")
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
