"""The float bicubic mode of T2V_OP_RESAMPLE (the resizes around the depth estimator of the VideoCrafter depth adapter): its error table
and its cost.  Writes profiles/bicubic.txt (or the file given as the first argument).

Errors (CPU, no GPU needed): per test shape, torch's own float32 error and the error of the record's arithmetic (tests/interp_bicubic.py,
which the kernel equals bit for bit: tests/test_gpu_bicubic.py), both against torch's float64 interpolation, and their ratio — the
quantities tests/test_bicubic_cpu.py gates (ratio <= 2).

Timings (GPU): the two passes of a 16-frame 256 x 256 clip — 48 planes 256^2 -> 384^2 (`prepare_midas_input`), and 16 planes
384^2 -> 256^2 plus the normalisation (one program: bicubic pass + front end) — each beside torch's `F.interpolate` of the same tensor on
the same GPU (for the second pass: plus torch's min-max normalisation), alternating, device events around batches of calls, medians over
the repetitions after a warm-up.  Reported only: there is no gate, the parent commit has nothing to compare with.
Usage: python tools/profile_bicubic.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from interp_bicubic import bicubic_interp  # noqa: E402
from sd_webui_text2video_amd import _lib as L, videocrafter as VC  # noqa: E402

SHAPES = [((1, 1, 1), (3, 5)), ((2, 2, 3), (7, 5)), ((3, 5, 7), (13, 3)), ((2, 8, 8), (24, 16)), ((2, 24, 16), (8, 8)), ((3, 32, 32), (24, 24)),
          ((1, 24, 24), (32, 32)), ((1, 4, 300), (3, 259)), ((3, 40, 56), (384, 384)), ((2, 384, 384), (40, 56))]


def error_table():
    rows = ["errors against torch's float64 interpolation (x ~ N(0, 1), torch.Generator().manual_seed(0) per shape), CPU:",
            f"{'shape':>28}  {'err_ref (torch fp32)':>20}  {'err_int (record)':>16}  {'ratio':>6}  {'float64 tables':>14}"]
    for src, dst in SHAPES:
        x = torch.randn(*src, generator=torch.Generator().manual_seed(0))
        kw = dict(size=dst, mode="bicubic", align_corners=False)
        exact = F.interpolate(x[None].double(), **kw)[0].numpy()
        err_ref = float(np.abs(F.interpolate(x[None], **kw)[0].numpy() - exact).max())
        err_int = float(np.abs(bicubic_interp(x.numpy(), *dst) - exact).max())
        err64 = float(np.abs(bicubic_interp(x.double().numpy(), *dst, dtype=np.float64) - exact).max())
        rows.append(f"{str(src) + ' -> ' + str(dst):>28}  {err_ref:20.3e}  {err_int:16.3e}  {err_int / max(err_ref, 1e-300):6.2f}  {err64:14.1e}")
    return rows


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def compare(ours, theirs, calls=50, reps=9):
    for fn in (ours, theirs):                     # warm-up: code objects, program compilation and binding, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(reps):                         # alternating
        t_ours.append(event_ms(ours, calls))
        t_theirs.append(event_ms(theirs, calls))
    return statistics.median(t_ours), min(t_ours), max(t_ours), statistics.median(t_theirs), min(t_theirs), max(t_theirs)


def timings():
    if not torch.cuda.is_available():
        return ["timings: not measured (no GPU)"]
    dev = torch.device("cuda:0")
    rows = [f"timings on {L.device_info()[0]} (ms per call, device events around 50 calls, median [min .. max] of 9 alternating repetitions; "
            "a call includes the host side: output allocation, plan run)"]
    g = torch.Generator().manual_seed(1)
    frames = torch.randn(48, 1, 256, 256, generator=g).to(dev)            # 16 frames x 3 channels
    kw = dict(mode="bicubic", align_corners=False)
    r = compare(lambda: VC.bicubic_resize(frames, (384, 384)), lambda: F.interpolate(frames, size=(384, 384), **kw))
    rows.append(f"  48 planes 256^2 -> 384^2:                      T2V_OP_RESAMPLE i[9]=1 {r[0]:.4f} [{r[1]:.4f} .. {r[2]:.4f}]   F.interpolate {r[3]:.4f} [{r[4]:.4f} .. {r[5]:.4f}]")
    diff = float((VC.bicubic_resize(frames, (384, 384)) - F.interpolate(frames, size=(384, 384), **kw)).abs().max())
    rows.append(f"    max |ours - F.interpolate on the GPU| = {diff:.3e}")
    ad = VC.Adapter(channels=[320], nums_rb=1, cin=64, ksize=1, sk=True, use_conv=False, init_weights=False).to(dev)
    depth = (torch.randn(16, 1, 384, 384, generator=g) * 3 + 5).to(dev)

    def torch_back():
        d = F.interpolate(depth, size=(256, 256), **kw)
        mn, mx = torch.amin(d, dim=[1, 2, 3], keepdim=True), torch.amax(d, dim=[1, 2, 3], keepdim=True)
        return 2. * (d - mn) / (mx - mn + 1e-7) - 1.
    r = compare(lambda: ad.normalise_depth(depth, size=(256, 256)), torch_back)
    rows.append(f"  16 planes 384^2 -> 256^2 + normalisation:      one program (2 launches) + the fold back to [n, 1, H, W] {r[0]:.4f} [{r[1]:.4f} .. {r[2]:.4f}]   torch {r[3]:.4f} [{r[4]:.4f} .. {r[5]:.4f}]")
    assert [o.kind for o in ad.last_program.ops] == [L.OP_RESAMPLE, L.OP_DEPTH_TOKENS]
    diff = float((ad.normalise_depth(depth, size=(256, 256)) - torch_back()).abs().max())
    rows.append(f"    max |ours - torch on the GPU| = {diff:.3e} (ours holds the fp16 values the adapter's first convolution reads)")
    return rows


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bicubic.txt")
    rows = ["float bicubic mode of T2V_OP_RESAMPLE (tools/profile_bicubic.py)", ""] + error_table() + [""] + timings()
    text = "\n".join(rows) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
