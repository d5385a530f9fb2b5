"""Cost of context windows (`context_windows=`, samplers.ContextWindows) at the 125-frame 256x256 geometry with windows of 16 frames and
overlap 4 (11 windows per video).  Writes profiles/context_windows.txt (or the file given as the first argument).

Kernels: the window gather (T2V_OP_LINCOMB i[9] = 2) of all 11 windows and the window blend (i[9] = 1) of a guided step, latent
1x4x125x32x32, fp32 and fp16 operands, and the blend behind forwards of 4 windows (three COPY2D records in front of it, one call) —
device events around 300 calls after 30 warm-up calls, the variants alternated over three rounds (min..max of the rounds), beside a
calibration GEMM of the box.  The records are built once, so a call is the library's launch path, not Python.
Run: the full-size UNet with random weights (bench.py's model), 125 frames @ 256x256, guidance 9, DDIM_Gaussian at 10 steps without
the VAE: wall time of `infer_conditioned(decode=False)` for the full-clip forward (no keyword: the code path the parent commit has),
all windows in one forward, and forwards of 4 windows — alternated over three rounds after one warm-up each; frames/s = 125 / time.
Then the GEMM tiles of the programs each layout ran.  Nothing here is gated.
Usage: python tools/profile_context_windows.py [out.txt]"""
import collections
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from sd_webui_text2video_amd import _lib as L, samplers as S  # noqa: E402

DEV = "cuda:0"
FRAMES, LENGTH, OVERLAP, STEPS = 125, 16, 4, 10


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "context_windows.txt")
    lib = L.load()
    rows = []

    def say(s):
        print(s, flush=True)
        rows.append(s)

    a = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    b = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    cal = timed(lambda: torch.matmul(a, b), 50, 10)
    say(f"calibration GEMM 4096^3 fp16 (torch.matmul): {cal:.1f} us = {2 * 4096 ** 3 / cal / 1e6:.0f} TFLOP/s")
    win = S.ContextWindows(LENGTH, OVERLAP)
    starts = win.starts(FRAMES)
    nW = len(starts)
    say(f"{FRAMES} frames, windows of {LENGTH} with overlap {OVERLAP}: {nW} windows per video at {starts} = {nW * LENGTH} frames per step "
        f"({nW * LENGTH / FRAMES:.2f} x the clip)")
    starts_d = torch.tensor(starts, dtype=torch.int32, device=DEV)
    weights_d = torch.tensor([win.weight(j) for j in range(LENGTH)], dtype=torch.float32, device=DEV)

    # the bindings launch through samplers._run_ops: capture the records they build once, then time the library call alone
    captured = []
    real = S._run_ops
    S._run_ops = lambda ops, device: captured.append(ops)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    variants, keep = [], []
    for dt in (torch.float32, torch.float16):
        x = torch.randn(1, 4, FRAMES, 32, 32, device=DEV).to(dt)
        xw = torch.empty(nW, 4, LENGTH, 32, 32, device=DEV, dtype=dt)
        e = torch.randn(2 * nW, 4, LENGTH, 32, 32, device=DEV).to(dt)
        out = torch.empty(2, 4, FRAMES, 32, 32, device=DEV)
        parts = [torch.cat([e[r0:r0 + n], e[nW + r0:nW + r0 + n]]).contiguous() for r0, n in S.ContextWindows(LENGTH, OVERLAP, batch=4).chunks(nW)]
        stage = torch.empty_like(e)
        keep += [x, xw, e, out, parts, stage]
        tag = "fp32" if dt == torch.float32 else "fp16"
        S._window_gather(xw, x, starts_d, 0)
        variants.append((f"gather {tag} ({(x.numel() + xw.numel()) * x.element_size() / 1e6:.1f} MB moved at most)", captured.pop()))
        S._window_blend(out, [e], starts_d, weights_d, 2)
        variants.append((f"blend {tag} eps ({(e.numel() * e.element_size() + out.numel() * 4) / 1e6:.1f} MB)", captured.pop()))
        S._window_blend(out, parts, starts_d, weights_d, 2, stage=stage)
        variants.append((f"blend {tag} eps behind forwards of 4 windows ({len(parts)} COPY2D + blend)", captured.pop()))
    S._run_ops = real

    def run(ops):
        one = isinstance(ops, L.T2VOp)
        arg, n = (ctypes.byref(ops), 1) if one else (ops, len(ops))
        return lambda: L.check(lib.t2v_run_ops(arg, n, None, 0, stream))
    t = {}
    for _ in range(3):
        for name, ops in variants:
            t.setdefault(name, []).append(timed(run(ops)))
    say("us per call over three rounds (device events, 300 calls): ")
    for k, v in t.items():
        say(f"    {k}: {min(v):.1f}..{max(v):.1f}")

    # ---- a 10-step run of the full-size UNet ------------------------------------------------------------------------------------------
    import bench
    from sd_webui_text2video_amd import configs, pipeline, unet as U
    dev = torch.device(DEV)
    net = U.UNetSD(**configs.MODELSCOPE_UNET, init_weights=False).half().to(dev).eval()
    bench.random_weights_(net, 0)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, autoencoder=None, device=dev)
    pipe.diffusion.progress = False
    gen = torch.Generator().manual_seed(1)
    cond = torch.randn(1, 77, 1024, generator=gen).half().to(dev)
    uncond = torch.randn(1, 77, 1024, generator=gen).half().to(dev)

    def run_clip(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.infer_conditioned(cond, uncond, STEPS, FRAMES, 1234, 9.0, 256, 256, 0.0, decode=False, sampler="DDIM_Gaussian", **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    base = dict(length=LENGTH, overlap=OVERLAP)
    cases = (("full-clip forward (no keyword)", {}), ("windows, one forward per step", dict(context_windows=base)),
             ("windows, forwards of 4", dict(context_windows=dict(base, batch=4))))
    for _, kw in cases:
        run_clip(**kw)                                # warm-up: the UNet programs of this layout are built once
    t = {}
    for _ in range(3):
        for name, kw in cases:
            t.setdefault(name, []).append(run_clip(**kw))
    say(f"DDIM_Gaussian, {STEPS} steps, {FRAMES} frames @ 256x256, guidance 9, full-size UNet (random weights), no VAE; s per run over three rounds "
        f"and frames/s of the best:")
    for k, v in t.items():
        say(f"    {k}: {min(v):.3f}..{max(v):.3f} s = {FRAMES / min(v):.2f} frames/s")
    full = min(t["full-clip forward (no keyword)"])
    say(f"    windows cost {min(t['windows, one forward per step']) / full:.2f} x the full-clip run in one forward per step, "
        f"{min(t['windows, forwards of 4']) / full:.2f} x in forwards of 4 ({nW * LENGTH / FRAMES:.2f} x the frames per step, by design)")
    say("GEMM tiles of the UNet programs that ran (batch rows B, frames F: tile id x records) — what the tile policy gives these shapes today:")
    for key, comp in net._programs.items():
        tiles = collections.Counter(op.i[22] for op in comp.prog.ops if op.kind == L.OP_GEMM)
        say(f"    B = {key[0]}, F = {key[1]}: " + ", ".join(f"tile {k} x {n}" for k, n in sorted(tiles.items())))
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
