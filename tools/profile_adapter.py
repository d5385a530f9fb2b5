"""Cost of the VideoCrafter depth adapter on the GPU: the adapter program (16 frames @ 256x256, the 77 M-parameter T2I-Adapter shape)
and the guided UNet step of BASELINE.json configs[4] (16 frames @ 32x32 latent, b = 2 on one x_t) with and without features, timed
back to back in the same process, beside the box's calibration GEMM.  Random weights (timing only).
Usage: python tools/profile_adapter.py        (the output is what profiles/adapter_overhead.txt records)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from sd_webui_text2video_amd import configs  # noqa: E402
from sd_webui_text2video_amd import _lib as L, videocrafter as VC  # noqa: E402
from tools.profile_unet import random_weights_  # noqa: E402


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    dev = torch.device("cuda:0")
    print(L.device_info())
    print(f"calibration GEMM 8192^3 fp16: {bench.calibration_gemm(dev):.1f} TF/s (before)")
    ad = VC.Adapter(channels=[320, 640, 1280, 1280], nums_rb=2, cin=64, ksize=1, sk=True, use_conv=False, init_weights=False).half().to(dev)
    random_weights_(ad)
    depth = torch.rand(16, 1, 256, 256, device=dev) * 10
    feats = ad(depth, normalise=True)
    prog = ad.last_program
    ms = timed(lambda: ad(depth, normalise=True), 20)
    kinds = {}
    for op in prog.ops:
        kinds[op.kind] = kinds.get(op.kind, 0) + 1
    print(f"adapter program, 16 frames @ 256x256 (77 M parameters): {ms:.3f} ms per call (host allocation of the four outputs included), "
          f"{len(prog.ops)} launches {dict(sorted(kinds.items()))}, {prog.total_flops() / 1e9:.1f} GFLOP, arena {prog.arena.high / 2**20:.1f} MiB")
    feats5 = [f.reshape(1, 16, *f.shape[1:]).permute(0, 2, 1, 3, 4) for f in feats]
    net = VC.UNetModel(**configs.LVDM_UNET, init_weights=False).half().to(dev)
    random_weights_(net)
    net.auto_refresh = False
    x = torch.randn(1, 4, 16, 32, 32, device=dev)
    y = torch.randn(2, 77, net.context_dim, device=dev, dtype=torch.float16)
    t = torch.full((2,), 500, device=dev)

    def step(f):
        net.single_timestep = True
        return net(x, t, context=y, features_adapter=f)
    net.refresh_weights(dev)
    for f in (None, feats5):
        step(f)
    torch.cuda.synchronize()
    rows = []
    for rep in range(3):                         # interleaved: without, with, without, with ...
        rows.append((timed(lambda: step(None), 20), timed(lambda: step(feats5), 20)))
    n_ops = {k[-1] if isinstance(k[-1], tuple) and k[-1][0] == "adapter" else None: len(c.prog.ops) for k, c in net._programs.items()}
    for a, b in rows:
        print(f"guided UNet step configs[4] (b = 2 on one x_t, 16 f @ 32x32, fp16): {a:.3f} ms without features, {b:.3f} ms with (+{b - a:.3f} ms)")
    print(f"launches per step: {n_ops}; layout conversions of the features over all steps: {net.adapter_conversions}")
    print(f"calibration GEMM 8192^3 fp16: {bench.calibration_gemm(dev):.1f} TF/s (after)")


if __name__ == "__main__":
    main()
