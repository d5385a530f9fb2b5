"""Frames/s of a batch of DIFFERENT prompts in one pass (ragged text contexts) beside the ways the same videos could be made before:
the prompts one after another, and `videos=V` of one prompt.  ModelScope UNet + VAE decoder fp16 with seeded weights, 24 frames @
256x256, 50 DDIM_Gaussian steps, CFG 9 — the benchmark's workload, `infer_conditioned(..., to_host=False)` around a device synchronise.

Per V in {2, 4}: prompts of 77 and 154 tokens alternating, one 77-token negative prompt.
  sequential   V calls of one video each (programs keyed 77 and (154, 77))          — runs on any commit
  videos       one call, videos=V of the 77-token prompt (the existing batching)    — runs on any commit
  batch        one call with the V contexts as lists                                — needs the per-sample table
All programs stay compiled (`max_programs` raised).  One warm-up pass over every variant, then `--rounds` rounds that alternate the
variants; min..max over the rounds is printed (the spread).  `--tree DIR` imports the package (and its built library) from another checkout, so that the same script times the parent
commit's `sequential` and `videos` beside this one's in the same job.  With `batch`: every video of the batch against its own
sequential run, rel-L2 of the final latents.
Usage: python tools/profile_prompt_batch.py [--tree DIR] [--variants sequential,videos,batch] [--rounds 3] [--out out.txt]"""
import argparse
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--variants", default="sequential,videos,batch")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.tree)]
    import bench
    from sd_webui_text2video_amd import _lib as L
    from sd_webui_text2video_amd import configs, pipeline, unet as U, vae as V

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    net = U.UNetSD(**configs.MODELSCOPE_UNET, init_weights=False).half().to(dev).eval()
    bench.random_weights_(net, 0)
    ae = V.AutoencoderKL(configs.VAE_DDCONFIG, 4, init_weights=False).half().to(dev).eval()
    bench.random_weights_(ae, 3)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, autoencoder=ae, device=dev)
    pipe.diffusion.progress = False
    net.max_programs = 8       # the six programs of this script stay compiled (the default keeps four: the timings would include re-lowering)
    g = torch.Generator().manual_seed(1)
    ctx = {77: torch.randn(1, 77, 1024, generator=g).half().to(dev), 154: torch.randn(1, 154, 1024, generator=g).half().to(dev)}
    uncond = torch.randn(1, 77, 1024, generator=g).half().to(dev)
    say(f"tree {os.path.abspath(args.tree)}; {args.frames} frames @ 256x256, {args.steps} DDIM_Gaussian steps, CFG 9, fp16, seeded weights")
    say(f"calibration GEMM 8192^3 fp16 (gemm2 256x256 tile): {bench.calibration_gemm(dev)} TFLOP/s")
    common = dict(steps=args.steps, frames=args.frames, scale=9.0, width=256, height=256, eta=0.0, to_host=False)
    SEED = 1234

    def lens(nv):
        return [77, 154] * (nv // 2)

    def sequential(nv):
        return [pipe.infer_conditioned(ctx[n], uncond, seed=SEED + v, **common)[1] for v, n in enumerate(lens(nv))]

    def videos(nv):
        return pipe.infer_conditioned(ctx[77], uncond, seed=SEED, videos=nv, **common)[1]

    def batch(nv):
        return pipe.infer_conditioned([ctx[n] for n in lens(nv)], [uncond] * nv, seed=SEED, **common)[1]

    fns = {"sequential": sequential, "videos": videos, "batch": batch}
    todo = [(name, nv) for nv in (2, 4) for name in args.variants.split(",")]
    last = {}
    for name, nv in todo:                      # warm-up: programs compiled, arenas bound, code objects loaded
        last[(name, nv)] = fns[name](nv)
    torch.cuda.synchronize(dev)
    L.async_status()
    times = {k: [] for k in todo}
    for _ in range(args.rounds):
        for name, nv in todo:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fns[name](nv)
            torch.cuda.synchronize(dev)
            times[(name, nv)].append(time.perf_counter() - t0)
    L.async_status()
    for nv in (2, 4):
        for name in args.variants.split(","):
            t = times[(name, nv)]
            fps = [nv * args.frames / v for v in t]
            say(f"  V = {nv} {name:<10} {min(t):7.3f} .. {max(t):7.3f} s per {nv} videos   {min(fps):6.2f} .. {max(fps):6.2f} frames/s   ({len(t)} rounds)")
        if "batch" in fns and ("batch", nv) in last and ("sequential", nv) in last:
            rel = [float((last[("batch", nv)][v:v + 1].float() - s.float()).norm() / s.float().norm()) for v, s in enumerate(last[("sequential", nv)])]
            say(f"  V = {nv} batch against each video's own run, final latents rel-L2: " + " ".join(f"{r:.3e}" for r in rel))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
