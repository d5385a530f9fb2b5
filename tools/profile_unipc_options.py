"""Cost of UniPC's thresholded data prediction (T2V_OP_DDIM_STEP mode 2: a measure and an apply record in one t2v_run_ops call) beside
the T2V_OP_LINCOMB it replaces, and of a 10-step UniPC run with and without `thresholding`.  Writes the timing section of
profiles/unipc_options.txt (or the file given as the first argument).

Per latent: the plain data prediction (one 3-term LINCOMB), the measure pass alone, the apply pass alone, and both as the sampler sends
them — device events around 300 calls after 30 warm-up calls, the variants alternated over three rounds (min..max of the rounds is
printed: the spread), beside a calibration GEMM of the box.  The records are built once, so a call is the library's launch path, not
Python.  Latents: 1x4x24x32x32 (24 frames @ 256x256) and 1x4x24x72x128 (1024x576).  Then the full-size UNet with random weights
(bench.py's model), 24 frames @ 256x256, guidance 9: wall time of `sample_loop` with UniPC at 10 steps, default options and
`thresholding=True`, alternated over three rounds after one warm-up each.  Reported only: nothing here has a parent to compare with.
Usage: python tools/profile_unipc_options.py [out.txt]"""
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from sd_webui_text2video_amd import _lib as L, samplers as S  # noqa: E402

DEV = "cuda:0"
LATENTS = [(1, 4, 24, 32, 32), (1, 4, 24, 72, 128)]


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "unipc_options.txt")
    lib = L.load()
    rows = []

    def say(s):
        print(s, flush=True)
        rows.append(s)

    a = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    b = torch.randn(4096, 4096, device=DEV, dtype=torch.float16)
    cal = timed(lambda: torch.matmul(a, b), 50, 10)
    say(f"calibration GEMM 4096^3 fp16 (torch.matmul): {cal:.1f} us = {2 * 4096 ** 3 / cal / 1e6:.0f} TFLOP/s")
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    sigma, alpha, g = 0.7431, 0.6692, 9.0
    for shape in LATENTS:
        gen = torch.Generator().manual_seed(1)
        x = torch.randn(shape, generator=gen).to(DEV)
        eps = torch.randn((2 * shape[0],) + shape[1:], generator=gen).to(DEV)
        out, table = torch.empty_like(x), torch.zeros(shape[0], 4, device=DEV)
        both = S._x0_threshold_records(out, x, eps, sigma, alpha, g, True, table)
        m_only, a_only = (L.T2VOp * 1)(both[0]), (L.T2VOp * 1)(both[1])
        run = lambda ops: (lambda: L.check(lib.t2v_run_ops(ops, len(ops), None, 0, stream)))
        nb = shape[0]
        terms = [(1.0 / alpha, x), (-sigma * g / alpha, eps[0:nb]), (-sigma * (1.0 - g) / alpha, eps[nb:2 * nb])]
        variants = (("plain (3-term LINCOMB)", lambda: S._lincomb(out, terms)), ("measure", run(m_only)), ("apply", run(a_only)),
                    ("measure + apply", run(both)))
        t = {}
        for _ in range(3):
            for name, fn in variants:
                t.setdefault(name, []).append(timed(fn))
        n = 1
        for d in shape[1:]:
            n *= d
        say(f"latent {shape}, n = {n} per video, us per call over three rounds: " + "; ".join(f"{k} {min(v):.1f}..{max(v):.1f}" for k, v in t.items()))
        say(f"    s = {[round(v, 4) for v in table[:, 0].tolist()]}; thresholding adds {min(t['measure + apply']) - min(t['plain (3-term LINCOMB)']):.1f} us to a "
            f"data prediction (the LINCOMB timing includes its Python binding, the records do not); the measure pass reads {n * 12 * 5 / 1e6:.1f} MB in five "
            f"passes of x and the fp32 eps pair (12 bytes per element): {n * 12 * 5 / min(t['measure']) / 1e3:.1f} GB/s")

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

    def run10(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.infer_conditioned(cond, uncond, 10, 24, 1234, 9.0, 256, 256, 0.0, decode=False, sampler="UniPC", **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    cases = (("default", {}), ("thresholding", dict(unipc=dict(thresholding=True))), ("bh2", dict(unipc=dict(variant="bh2"))))
    for _, kw in cases:
        run10(**kw)                                   # warm-up: the UNet program of this geometry is built once
    t = {}
    for _ in range(3):
        for name, kw in cases:
            t.setdefault(name, []).append(run10(**kw))
    say("UniPC, 10 steps, 24 frames @ 256x256, guidance 9, full-size UNet (random weights), ms per run over three rounds: "
        + "; ".join(f"{k} {min(v):.1f}..{max(v):.1f}" for k, v in t.items()))
    say(f"    thresholding adds {min(t['thresholding']) - min(t['default']):.2f} ms to the run ({(min(t['thresholding']) / min(t['default']) - 1) * 100:.2f} %); "
        f"bh2 changes host scalars only ({min(t['bh2']) - min(t['default']):+.2f} ms)")
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
