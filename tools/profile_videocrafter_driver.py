"""The VideoCrafter driver at the configs[4] geometry (16 frames @ 256x256, 50 DDIM steps, CFG 7.5, eta 1.0, fp16 weights, random-init
0.96 B UNetModel + VAE decoder as bench.py --model lvdm builds them).  Writes the timing section of profiles/videocrafter_driver.txt (or
the file given as the first argument).

  1. decode + conversion of one video's latent to uint8 frames ON THE HOST: the float route
     `torch_to_np(decode_first_stage(z, decode_bs, return_cpu=False))` against `decode_first_stage_uint8(z, decode_bs)`, at
     decode_frame_bs 1 (what the reference passes) and None (all frames in one program).  Host clock around calls that end with the
     frames in host memory; 10 calls after 2 warm-up calls, the two routes alternated over three rounds (min..max = the spread).
  2. wall time per video of `process_videocrafter`: the loop route (`one_pass=False`) against one pass, batch_count 1 / 2 / 4, at
     decode_frame_bs 1 and None.  Host clock around whole calls (they end with the frames in host memory), one warm-up call per
     variant (program compilation, arenas), then three alternated rounds.
Beside both: a calibration GEMM of the box.  Usage: python tools/profile_videocrafter_driver.py [out.txt] [steps]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bench  # noqa: E402
from sd_webui_text2video_amd import configs, videocrafter as VC  # noqa: E402

DEV = torch.device("cuda", 0)
FRAMES, SIDE = 16, 256


def build():
    ld = VC.LatentDiffusion(configs.LVDM_UNET, dict(ddconfig=configs.VAE_DDCONFIG, embed_dim=4), image_size=[SIDE // 8, SIDE // 8],
                            video_length=FRAMES, init_weights=False, **configs.LVDM_SCHEDULE)
    ld = ld.half().to(DEV).eval()
    bench.random_weights_(ld.model.diffusion_model, 0)
    bench.random_weights_(ld.first_stage_model, 3)
    g = torch.Generator().manual_seed(1)
    table = {"a prompt": torch.randn(1, 77, 768, generator=g).half().to(DEV), "": torch.randn(1, 77, 768, generator=g).half().to(DEV)}

    class Clip:                      # the text tower is outside the timed path
        def encode(self, prompts):
            return torch.cat([table[p] for p in prompts], 0)
    ld.cond_stage_model = Clip()
    return ld


def wall(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3          # ms per call


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "videocrafter_driver.txt")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    rows = []

    def say(s):
        print(s, flush=True)
        rows.append(s)

    torch.cuda.set_device(0)
    a = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    b = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    torch.matmul(a, b)
    torch.cuda.synchronize()
    cal = wall(lambda: torch.matmul(a, b), 50, 10) * 1e3
    say(f"calibration GEMM 4096^3 fp16 (torch.matmul): {cal:.1f} us = {2 * 4096 ** 3 / cal / 1e6:.0f} TFLOP/s")
    ld = build()
    z = (torch.randn(1, 4, FRAMES, SIDE // 8, SIDE // 8, generator=torch.Generator().manual_seed(2)) * ld.scale_factor).to(DEV)
    say(f"== decode + conversion of one video ({FRAMES} f @ {SIDE}x{SIDE}, fp16 weights) to uint8 frames in host memory, ms per call, min..max of three rounds")
    for bs in (1, None):
        routes = (("float route", lambda: VC.torch_to_np(ld.decode_first_stage(z, decode_bs=bs, return_cpu=False)).numpy()),
                  ("uint8 route", lambda: ld.decode_first_stage_uint8(z, decode_bs=bs).numpy()))
        same = np.array_equal(routes[0][1](), routes[1][1]())
        t = {}
        for _ in range(3):
            for name, fn in routes:
                t.setdefault(name, []).append(wall(fn, 10, 2))
        say(f"decode_frame_bs {bs}: " + "; ".join(f"{k} {min(v):.2f}..{max(v):.2f}" for k, v in t.items()) +
            f"; uint8 / float = {min(t['uint8 route']) / min(t['float route']):.3f}; bytes equal: {same}")
    say(f"== process_videocrafter, {steps} steps, CFG 7.5, eta 1.0: wall ms PER VIDEO, loop route | one pass, min..max of three rounds")
    smp = VC.DDIMSampler(ld)
    for bs in (1, None):
        for count in (1, 2, 4):
            args = dict(model=ld, sampler=smp, prompt="a prompt", n_prompt="", steps=steps, frames=FRAMES, seed=100, cfg_scale=7.5, eta=1.0,
                        batch_count=count, decode_frame_bs=bs)
            variants = [("loop", lambda: VC.process_videocrafter(dict(args, one_pass=False)))]
            if count > 1:
                variants.append(("one pass", lambda: VC.process_videocrafter(dict(args, one_pass=True))))
            t = {}
            for name, fn in variants:
                fn()                                     # warm-up: compiles the programs of this batch size
            for _ in range(3):
                for name, fn in variants:
                    t.setdefault(name, []).append(wall(fn, 1, 0) / count)
            line = f"decode_frame_bs {bs}, batch_count {count}: " + "; ".join(f"{k} {min(v):.1f}..{max(v):.1f}" for k, v in t.items())
            if count > 1:
                line += f"; one pass / loop = {min(t['one pass']) / min(t['loop']):.3f} ({(min(t['loop']) / min(t['one pass']) - 1) * 100:+.1f} % videos/s)"
            say(line)
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
