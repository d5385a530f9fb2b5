"""Cost and accuracy of FreeU (T2V_OP_FREEU, `freeu=`).  Writes profiles/freeu.txt (or the file given as the first argument).

Accuracy: the kernel and the fp32 torch.fft formulation (what FreeU itself computes) against the float64 restatement on the operands of
tests/freeu_inputs.py — maximum absolute error per geometry; the tests gate the kernel at 4 x the fft's error.
Records: the ten FreeU records of the released 24-frame 256 x 256 guided-step program (batch 2: cond | uncond), each on a buffer of its
own — device events around 100 calls after 10 warm-up calls, alternated over three rounds (min..max of the rounds; the buffers are
refilled between rounds).  The records are built once, so a call is the library's launch path, not Python.  Beside each time the bytes
the record must move at the least — the scaled and the filtered columns read once and written once — and with the filtered columns read
twice (the kernel's second pass, when it misses the caches), as GB/s and as a share of the 8.0 TB/s HBM peak.
Step: the guided step (`forward_cfg_pair`, full-size UNet with random weights, bench.py's model) without the keyword — the code the
parent commit runs — and with the authors' values, alternated over three rounds of 10 forwards after a warm-up of each.
Nothing here is gated.
Usage: python tools/profile_freeu.py [out.txt]"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from sd_webui_text2video_amd import _lib as L  # noqa: E402
from sd_webui_text2video_amd import configs, unet as U  # noqa: E402

DEV = "cuda:0"
VALUES = {"b1": 1.2, "b2": 1.4, "s1": 0.9, "s2": 0.2}
HBM_PEAK = 8.0e12


def timed(fn, iters, warm):
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


def record(i, f, ptr):
    op = L.T2VOp()
    op.kind = L.OP_FREEU
    for k, v in enumerate(i):
        op.i[k] = v
    op.f[0], op.f[1] = f
    op.p[0] = ptr
    return op


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "freeu.txt")
    lib = L.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    rows = []

    def say(s):
        print(s, flush=True)
        rows.append(s)

    # ---- accuracy ---------------------------------------------------------------------------------------------------------------------
    import freeu_inputs as FI
    say(f"max abs error against float64 per geometry (frames, h, w, C_h, C_s), N(0, 1) operand, b = {FI.B}, s = {FI.S}: kernel | fp32 torch.fft")
    for geom in FI.GEOMS:
        frames, h, w, c_h, c_s = geom
        X = FI.operand("noise", geom)
        buf = X.to(DEV).contiguous()
        L.check(lib.t2v_run_ops(ctypes.byref(record((frames * h * w, c_h + c_s, X.shape[1], c_h, frames, h, w), (FI.B, FI.S), buf.data_ptr())), 1, None, 0, stream))
        torch.cuda.synchronize()
        ref = FI.reference(X, geom)[:, c_h:c_h + c_s]
        ek = (buf.cpu()[:, c_h:c_h + c_s].double() - ref).abs().max().item()
        ef = (FI.fp32_fft(X, geom).double() - ref).abs().max().item()
        say(f"    {geom}: {ek:.3e} | {ef:.3e}")

    # ---- the records of the released program ------------------------------------------------------------------------------------------
    import bench
    dev = torch.device(DEV)
    net = U.UNetSD(**configs.MODELSCOPE_UNET, init_weights=False).half().to(dev).eval()
    bench.random_weights_(net, 0)
    net._share_now = True
    net.enable_freeu(s1=VALUES["s1"], s2=VALUES["s2"], b1=VALUES["b1"], b2=VALUES["b2"])
    prog = net._compile(2, 24, 32, 32, 77, "f16", "f16", "f16", x_batch=1).prog
    net.disable_freeu()
    net._share_now = False
    recs = [op for op in prog.ops if op.kind == L.OP_FREEU]
    say(f"released UNet, 24 frames @ 256 x 256, guided step (batch 2): {len(recs)} FreeU records among {len(prog.ops)} ops")
    variants = []
    for op in recs:
        n_rows, c_total, ld, c_h, frames, h, w = op.i[0:7]
        buf = torch.empty(n_rows, ld, device=DEV)
        least = n_rows * (c_h // 2 + c_total - c_h) * 4 * 2
        twice = least + n_rows * (c_total - c_h) * 4
        variants.append((op.name, (n_rows, c_total, ld, c_h, frames, h, w), record(op.i[0:7], (op.f[0], op.f[1]), buf.data_ptr()), buf, least, twice))
    t = {}
    for _ in range(3):
        for name, geo, rec, buf, _, _ in variants:
            buf.normal_()
            t.setdefault(name, []).append(timed(lambda: L.check(lib.t2v_run_ops(ctypes.byref(rec), 1, None, 0, stream)), 100, 10))
    say("us per record over three rounds (device events, 100 calls) | MB at the least / with the filtered columns read twice | GB/s of the best "
        "round on either count | share of the 8.0 TB/s HBM peak on either count")
    total = 0.0
    for name, geo, rec, buf, least, twice in variants:
        v = t[name]
        best = min(v) * 1e-6
        total += min(v)
        say(f"    {name} rows {geo[0]} C_h {geo[3]} C_s {geo[1] - geo[3]} {geo[5]}x{geo[6]}: {min(v):.1f}..{max(v):.1f} us | {least / 1e6:.1f} / {twice / 1e6:.1f} MB | "
            f"{least / best / 1e9:.0f} / {twice / best / 1e9:.0f} GB/s | {100 * least / best / HBM_PEAK:.0f} % / {100 * twice / best / HBM_PEAK:.0f} %")
    least_all = sum(v[4] for v in variants)
    bound_us = least_all / 6.29e12 * 1e6
    say(f"    sum of the ten records, best rounds: {total:.1f} us for {least_all / 1e6:.0f} MB at the least = {total / bound_us:.1f} x the {bound_us:.0f} us "
        f"those bytes take at the 6.29 TB/s a copy reaches (the 4 x 4 and 8 x 8 levels hold 16 and 64 rows per workgroup: latency, not bytes)")

    # ---- the guided step ------------------------------------------------------------------------------------------------------------------
    del variants
    torch.cuda.empty_cache()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(1, 4, 24, 32, 32, generator=gen).half().to(dev)
    ctx = torch.randn(2, 77, 1024, generator=gen).half().to(dev)
    tt = torch.tensor([500.0], device=dev)

    def step(freeu):
        def fn():
            if freeu:
                net.enable_freeu(s1=VALUES["s1"], s2=VALUES["s2"], b1=VALUES["b1"], b2=VALUES["b2"])
            try:
                net.forward_cfg_pair(x, tt, ctx, context_token="profile", single_t=True)
            finally:
                net.disable_freeu()
        return fn
    cases = (("without the keyword (the parent's program)", step(False)), ("freeu = the authors' ModelScope values", step(True)))
    with torch.no_grad():
        for _, fn in cases:
            timed(fn, 2, 2)
        t = {}
        for _ in range(3):
            for name, fn in cases:
                t.setdefault(name, []).append(timed(fn, 10, 1) / 1e3)
    say("guided step (forward_cfg_pair, full-size UNet, random weights, fp16, 24 frames @ 256 x 256), ms per forward over three rounds of 10:")
    for k, v in t.items():
        say(f"    {k}: {min(v):.3f}..{max(v):.3f} ms")
    a, b = (min(v) for v in t.values())
    say(f"    FreeU adds {(b - a) * 1e3:.0f} us = {100 * (b - a) / a:.2f} % of the step (the records alone: {total:.0f} us = {100 * total / 1e3 / a:.2f} %); "
        f"the expectation from bytes alone was {100 * bound_us / 1e3 / a:.2f} %, well under 1 %: it {'held' if total / 1e3 / a < 0.01 and (b - a) / a < 0.01 else 'did not hold'}")
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
