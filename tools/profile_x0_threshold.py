"""Added time per DDIM_Gaussian step of the x0 restriction records of T2V_OP_DDIM_STEP (i[8]: clamp, measure pass, threshold) on top of the
plain step.  Writes the timing section of profiles/x0_threshold.txt (or the file given as the first argument).

Per latent: the plain step, the clamp step, the measure pass alone, the thresholding step alone, and measure + threshold as the sampler
sends them (two records, one t2v_run_ops call) — device events around 300 calls after 30 warm-up calls, the variants alternated over three
rounds (min..max of the rounds is printed: the spread), beside a calibration GEMM of the box.  The records are built once, so a call is
the library's launch path, not Python.  Latents: 1x4x24x32x32 (the deployed 24 frames @ 256^2), 1x4x125x32x32, 1x4x24x72x128
(1024x576), and four videos of the first in one batch.  Reported only: the parent commit has nothing to compare the new records with.
Usage: python tools/profile_x0_threshold.py [out.txt]"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from sd_webui_text2video_amd import _lib as L, samplers as S  # noqa: E402

DEV = "cuda:0"
LATENTS = [(1, 4, 24, 32, 32), (1, 4, 125, 32, 32), (1, 4, 24, 72, 128), (4, 4, 24, 32, 32)]


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "x0_threshold.txt")
    lib = L.load()
    rows = []

    def say(s):
        print(s, flush=True)
        rows.append(s)

    a = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    b = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    cal = timed(lambda: torch.matmul(a, b), 50, 10)
    say(f"calibration GEMM 4096^3 fp16 (torch.matmul): {cal:.1f} us = {2 * 4096 ** 3 / cal / 1e6:.0f} TFLOP/s")
    coef = [1.7130, 1.3908, 0.9, 0.3, 0.0, 9.0]
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    for shape in LATENTS:
        g = torch.Generator().manual_seed(1)
        xt = torch.randn(shape, generator=g).to(DEV)
        eps = torch.randn((2 * shape[0],) + shape[1:], generator=g).to(DEV)
        out, table = torch.empty_like(xt), torch.zeros(shape[0], 4, device=DEV)
        plan = S.GaussianDiffusion(None, np.linspace(1e-4, 2e-2, 1000))._step_plan(shape[1], int(np.prod(shape[2:])), 2, "f32", "f32", samples=shape[0])
        c6 = (ctypes.c_float * 6)(*coef)
        both = S._ddim_restricted_records(out, xt, eps, None, coef, 2, percentile=0.995, table=table)
        clamp = S._ddim_restricted_records(out, xt, eps, None, coef, 2, bound=1.0)
        m_only, a_only = (L.T2VOp * 1)(both[0]), (L.T2VOp * 1)(both[1])
        run = lambda ops: (lambda: L.check(lib.t2v_run_ops(ops, len(ops), None, 0, stream)))
        variants = (("plain (t2v_ddim_step)", lambda: L.check(lib.t2v_ddim_step(plan.handle, xt.data_ptr(), eps.data_ptr(), None, out.data_ptr(), c6, stream))),
                    ("clamp", run(clamp)), ("measure", run(m_only)), ("threshold", run(a_only)), ("measure + threshold", run(both)))
        t = {}
        for _ in range(3):
            for name, fn in variants:
                t.setdefault(name, []).append(timed(fn))
        n = int(np.prod(shape[1:]))
        say(f"latent {shape}, n = {n} per video, us per call over three rounds: " + "; ".join(f"{k} {min(v):.1f}..{max(v):.1f}" for k, v in t.items()))
        say(f"    s = {[round(v, 4) for v in table[:, 0].tolist()]}; percentile adds {min(t['measure + threshold']) - min(t['plain (t2v_ddim_step)']):.1f} us to the plain "
            f"step, clamp {min(t['clamp']) - min(t['plain (t2v_ddim_step)']):.1f} us; the measure pass reads {n * 10 * 5 / 1e6:.1f} MB in five passes of x and the eps pair "
            f"(2 of 4 channels guided: 10 bytes per element): {n * 10 * 5 / min(t['measure']) / 1e3:.1f} GB/s")
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
