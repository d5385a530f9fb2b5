"""Cost of the parameter fingerprint (T2V_OP_FINGERPRINT) and of a VideoCrafter LoRA merge on one GPU -> profiles/lora_fingerprint.txt

    python tools/profile_fingerprint.py [--out FILE]

(1) the fingerprint launch by device events, after warm-up, over the parameters of the full-size ModelScope UNet (fp16) and of the
released LVDM UNet (fp32): bytes of the table, time, GB/s against the 6.3 TB/s achievable HBM figure; (2) `verify_weights` as the
samplers call it (host work + launch + copy back), wall clock; (3) `net_load_lora` of a rank-4 LoRA over every attention Linear of
the released LVDM UNet: wall time to the end of the next `refresh_weights`.  The weights are whatever the allocator holds: none of
these times depends on the values."""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from sd_webui_text2video_amd import _lib as L  # noqa: E402
from sd_webui_text2video_amd import configs, unet as U, videocrafter as VC  # noqa: E402

ACHIEVABLE_GBS = 6300.0


def launch_ms(fp, dev, reps=20):
    seg, chk, out = fp._tables
    op = L.T2VOp()
    op.kind = L.OP_FINGERPRINT
    op.i[0], op.i[1] = seg.shape[0], chk.shape[0]
    op.p[0], op.p[1], op.p[2] = seg.data_ptr(), out.data_ptr(), chk.data_ptr()
    st = torch.cuda.current_stream(dev)
    lib = L.load()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        L.check(lib.t2v_run_ops(ctypes.byref(op), 1, None, 0, ctypes.c_void_p(st.cuda_stream)))
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def wall(fn, dev, reps=5):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {L.device_info()[0]}, {L.device_info()[1]} CUs; chunk {L.FINGERPRINT_CHUNK} bytes per workgroup; achievable HBM {ACHIEVABLE_GBS / 1e3:.1f} TB/s")
    lvdm = None
    for label, make in (("ModelScope UNet fp16", lambda: U.UNetSD(**configs.MODELSCOPE_UNET, init_weights=False).half()),
                        ("released LVDM UNet fp32", lambda: VC.LatentDiffusion(configs.LVDM_UNET, None, image_size=[32, 32], video_length=16,
                                                                               init_weights=False, **configs.LVDM_SCHEDULE))):
        model = make().to(dev)
        net = model if isinstance(model, U.UNetSD) else model.model.diffusion_model
        named = net._named_params()
        fp = net._fingerprint
        for _ in range(3):
            vals = fp.compute(named, dev)
        ms = launch_ms(fp, dev)
        med = statistics.median(ms)
        gbs = fp.last_bytes / med / 1e6
        say(f"{label}: {len(named)} tensors, {fp._tables[1].shape[0]} chunks, {fp.last_bytes / 1e9:.3f} GB: launch (memset + kernel, device events, "
            f"median of {len(ms)}) {med:.3f} ms [min {min(ms):.3f}, max {max(ms):.3f}] = {gbs:.0f} GB/s = {100 * gbs / ACHIEVABLE_GBS:.0f} % of achievable")
        assert len(set(vals.values())) > 1
        w = wall(lambda: fp.compute(named, dev), dev)
        say(f"    fingerprint of all tensors as verify_weights runs it (table key, launch, copy back; wall clock): median {statistics.median(w):.2f} ms [min {min(w):.2f}]")
        if not isinstance(model, U.UNetSD):
            lvdm = (model, net)
        else:
            del model, net, named, fp
            torch.cuda.empty_cache()

    ld, net = lvdm
    with torch.no_grad():
        for p in net.parameters():
            p.normal_(0, 0.02)
    t0 = time.perf_counter()
    net.refresh_weights(dev)
    torch.cuda.synchronize(dev)
    say(f"released LVDM UNet: first full pack {1e3 * (time.perf_counter() - t0):.0f} ms ({len(net._packed)} images, fingerprints recorded)")
    w = wall(lambda: net.verify_weights(dev), dev)
    say(f"    verify_weights with nothing changed (wall clock): median {statistics.median(w):.2f} ms [min {min(w):.2f}]")
    w = wall(lambda: net.refresh_weights(dev), dev)
    say(f"    refresh_weights with nothing changed (the signature check alone, wall clock): median {statistics.median(w):.2f} ms")
    g = torch.Generator().manual_seed(0)
    sd = {}
    for name, mod in net.named_modules():
        if mod.__class__ is torch.nn.Linear and (".attn" in name):
            sd[f"model.diffusion_model.{name}.lora_down.weight"] = torch.randn(4, mod.weight.shape[1], generator=g) * 0.05
            sd[f"model.diffusion_model.{name}.lora_up.weight"] = torch.randn(mod.weight.shape[0], 4, generator=g) * 0.05
    path = os.path.join(tempfile.mkdtemp(), "lora.ckpt")
    torch.save(sd, path)
    for tag, remove in (("merge", False), ("un-merge", True), ("merge again", False)):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        VC.net_load_lora(ld, path, alpha=0.7, remove=remove)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        net.refresh_weights(dev)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        say(f"net_load_lora over {len(sd) // 2} attention Linears ({tag}): load + merge {1e3 * (t1 - t0):.1f} ms, refresh_weights {1e3 * (t2 - t1):.1f} ms "
            f"({net.last_repack} of {len(net._packed)} images), together {1e3 * (t2 - t0):.1f} ms   (ModelScope-style merge: 7.4 ms, profiles/r06_aux_stages.txt)")
    # the reference's own way: a write through .data, found by the fingerprint
    w0 = next(p for n, p in net.named_parameters() if n.endswith("attn2.to_k.weight"))
    w0.data += 0.01
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    changed = net.verify_weights(dev)
    torch.cuda.synchronize(dev)
    say(f"verify_weights after `to_k.weight.data += 0.01`: {1e3 * (time.perf_counter() - t0):.1f} ms, changed {changed}, {net.last_repack} images re-packed")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
