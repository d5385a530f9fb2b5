"""Cost of a Stable LoRA merge on one GPU (T2V_OP_LORA_MERGE, sd-webui-text2video_amd/stable_lora.py) -> profiles/stable_lora.txt

    python tools/profile_stable_lora.py [--out FILE] [--rank 16] [--tiny]

The full-size ModelScope UNet in fp16 on the device and a rank-16 file over EVERY Linear, Conv2d and Conv3d that `process_lora` matches.
Reported: (0) a calibration line — an in-place torch elementwise op over 1 GiB on this device, the read + write rate of the box at the time
of the run; (1) the host side of `process_lora`: resolution of the keys, upload of the factors, the segment and tile tables; (2) the merge
launch by device events after warm-up, alternating +alpha and -alpha over the same tables, the bytes it must move (one read and one write of
every touched weight; the factors are 1-2 % of that and are not counted) and the share of the 6.29 TB/s the project measures for HBM;
(3) the partial re-pack that follows (`_refresh_weights(also_changed=...)`); (4) the same merge in torch ops on the same device: `_merge_torch`
(the contract: r rank-1 updates per weight) and the reference's own loop (`B @ A`, clone, scaled add per module).  The weights are random:
none of these times depends on the values."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch
from torch import nn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from sd_webui_text2video_amd import _lib as L  # noqa: E402
from sd_webui_text2video_amd import configs, stable_lora as SL, unet as U  # noqa: E402

ACHIEVABLE_GBS = 6290.0
ON = (True, True, True, True, True)            # use_bias, use_time, use_conv, use_emb, use_linear


def make_file(net, rank, seed=0):
    """{key: fp16 CPU tensor}: factors for every Linear / Conv2d / Conv3d of `net` ('proj' Linears with the 3-D factors of a trained file)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, m in net.named_modules():
        if not isinstance(m, (nn.Linear, nn.Conv2d, nn.Conv3d)):
            continue
        w = m.weight
        cols = w[0].numel() * (3 if isinstance(m, nn.Conv3d) else 1)
        A = (torch.randn(rank, cols, generator=g) * 0.02).half()
        B = (torch.randn(w.shape[0], rank, generator=g) * 0.02).half()
        if isinstance(m, nn.Linear) and "proj" in name:
            A, B = A.unsqueeze(-1), B.unsqueeze(-1)
        sd[name + ".lora_A"], sd[name + ".lora_B"] = A, B
    return sd


def wall(fn, dev, reps=3):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def events_ms(fn, dev, reps):
    st = torch.cuda.current_stream(dev)
    ms = []
    for k in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn(k)
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--tiny", action="store_true", help="the tiny test configuration (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {L.device_info()[0]}, {L.device_info()[1]} CUs; tile {L.LORA_TILE} elements per workgroup; HBM figure of the project {ACHIEVABLE_GBS / 1e3:.2f} TB/s")
    # (0) calibration
    buf = torch.zeros(1 << 29, dtype=torch.float16, device=dev)
    for _ in range(3):
        buf.add_(1.0)
    ms = events_ms(lambda k: buf.add_(1.0), dev, 10)
    med = statistics.median(ms)
    say(f"calibration: torch `x.add_(1.0)` over 1 GiB fp16 (read + write 2.147 GB): median {med:.3f} ms = {2 * buf.numel() * 2 / med / 1e6:.0f} GB/s")
    del buf
    torch.cuda.empty_cache()

    if args.tiny:
        from oracle import configs as oc
        cfg, label = oc.TINY_UNET, "tiny UNet (rehearsal)"
    else:
        cfg, label = configs.MODELSCOPE_UNET, "ModelScope UNet"
    net = U.UNetSD(**cfg, init_weights=False).half().to(dev)
    with torch.no_grad():
        for p in net.parameters():
            p.normal_(0, 0.02)
    file = make_file(net, args.rank)
    proc = SL.StableLoraProcessor()

    # (1) host side: resolution, factor upload, tables — process_lora's own steps, timed one by one
    t0 = time.perf_counter()
    plan = proc._resolve(net, [file], True, True, True, True)
    t1 = time.perf_counter()
    todo = plan[0]
    keep, segments = [], []
    for name, m, A, B, N, J, r, form in todo:
        w = m.weight
        A, B = A.to(dev, w.dtype).contiguous(), B.to(dev, w.dtype).contiguous()
        keep.append((A, B))
        segments.append((w.data_ptr(), A.data_ptr(), B.data_ptr(), N, J, r, form, L.F16))
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    seg_d, til_d = SL.merge_device(segments, 0.0, dev)          # alpha 0: W + 0 = W, the tables are what is wanted
    torch.cuda.synchronize(dev)
    t3 = time.perf_counter()
    elements = sum(s[3] * s[4] for s in segments)
    factor_bytes = sum(2 * (A.numel() + B.numel()) for A, B in keep)
    say(f"{label} fp16, rank {args.rank}: {len(segments)} weights ({sum(1 for s in segments if s[6] == L.LORA_TEMPORAL)} temporal), {elements / 1e9:.3f} G elements, "
        f"{til_d.shape[0]} tiles; factors {factor_bytes / 1e6:.1f} MB")
    say(f"host: resolve and shape-check every key {1e3 * (t1 - t0):.1f} ms; cast + upload of {2 * len(keep)} factors {1e3 * (t2 - t1):.1f} ms; "
        f"segment + tile tables, their upload and the FIRST launch of the process (it loads the code object) {1e3 * (t3 - t2):.1f} ms")

    # (2) the launch
    op = L.T2VOp()
    op.kind = L.OP_LORA_MERGE
    op.i[0], op.i[1] = len(segments), til_d.shape[0]
    op.p[0], op.p[1] = seg_d.data_ptr(), til_d.data_ptr()
    lib = L.load()
    st = torch.cuda.current_stream(dev)

    def launch(k):
        op.f[0] = 0.7 if k % 2 == 0 else -0.7
        L.check(lib.t2v_run_ops(ctypes.byref(op), 1, None, 0, ctypes.c_void_p(st.cuda_stream)))

    for k in range(4):
        launch(k)
    ms = events_ms(launch, dev, 20)
    med = statistics.median(ms)
    moved = 2 * 2 * elements
    gbs = moved / med / 1e6
    say(f"merge launch (device events, median of {len(ms)}, +alpha / -alpha alternating): {med:.3f} ms [min {min(ms):.3f}, max {max(ms):.3f}]; "
        f"{moved / 1e9:.3f} GB read + written = {gbs:.0f} GB/s = {100 * gbs / ACHIEVABLE_GBS:.0f} % of {ACHIEVABLE_GBS / 1e3:.2f} TB/s "
        f"(the least time at that rate: {moved / ACHIEVABLE_GBS / 1e6:.3f} ms)")
    del keep, seg_d, til_d

    # (3) process_lora as a user meets it, without and with a live pack
    w = wall(lambda: proc.process_lora(net, [file], *ON, 0.7), dev)
    say(f"process_lora, no pack yet (resolve + upload + tables + launch + synchronise, wall clock): median {statistics.median(w):.1f} ms [min {min(w):.1f}]")
    t0 = time.perf_counter()
    net.refresh_weights(dev)
    torch.cuda.synchronize(dev)
    say(f"first full pack: {1e3 * (time.perf_counter() - t0):.0f} ms ({len(net._packed)} images)")
    touched = [name + ".weight" for name, *_ in todo]
    w = wall(lambda: net._refresh_weights(dev, also_changed=touched), dev)
    say(f"refresh_weights after the merge (every touched weight: {net.last_repack} of {len(net._packed)} images re-packed, fingerprints recorded; wall clock): "
        f"median {statistics.median(w):.1f} ms [min {min(w):.1f}]")
    w = wall(lambda: proc.process_lora(net, [file], *ON, 0.7), dev)
    say(f"process_lora with the live pack (merge + that refresh, wall clock): median {statistics.median(w):.1f} ms [min {min(w):.1f}]")

    # (4) torch ops on the same device
    dev_factors = [(m.weight, A.to(dev, torch.float16).contiguous(), B.to(dev, torch.float16).contiguous(), form) for _, m, A, B, _, _, _, form in todo]

    def merge_torch():
        for wt, A, B, form in dev_factors:
            SL._merge_torch(wt, A, B, 0.7, form)

    @torch.no_grad()
    def reference_loop():
        for wt, A, B, form in dev_factors:
            delta = B @ A
            if form == L.LORA_TEMPORAL:
                delta = torch.mean(delta.view(wt.shape[0], wt.shape[1], 3, 3, 1), dim=-2, keepdim=True)
            new = wt.detach().clone()
            new += delta.view(wt.shape) * 0.7
            wt.copy_(new)

    for tag, fn in (("_merge_torch (r rank-1 updates per weight, fp32 sums)", merge_torch), ("the reference's loop in torch ops (B @ A, clone, scaled add)", reference_loop)):
        fn()
        w = wall(fn, dev)
        say(f"{tag} over the same {len(dev_factors)} weights, factors already on the device (wall clock): median {statistics.median(w):.1f} ms [min {min(w):.1f}]")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
