#!/usr/bin/env python
"""bench.py — denoised frames/sec (UNet sampling loop + VAE decode), BASELINE.json's metric.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is ONE whole video through the hot path behind the reference's entry points:
`TextToVideoSynthesis.infer_conditioned` = Txt2VideoSampler.sample_loop (50 DDIM_Gaussian steps,
classifier-free guidance 9, eta 0; cond+uncond batched => 50 b=2 UNet forwards + 50 fused
update kernels) + batched VAE decode of all frames + uint8 conversion, all on device
(inputs — noise, conditioning, weights — are resident in HBM before the timed region).
Workload: BASELINE.json configs[1] — ModelScope t2v fp16, 24 frames @256x256 (the clip BASELINE.json's metric names).
N = 1: one video on the GPU (cond + uncond batched as b=2).
N > 1 (round 4): the headline is north_star's FRAME-PARALLEL layout — ONE clip on all N GPUs, strong scaling:
N = 2 the CFG pair (cond | uncond forwards on 2 GPUs, eps all-gather per step), even N >= 4 the clip's frames sharded along T
over N/2 GPUs x the CFG pair, the exchanges inside a UNet forward executed by the library over its own RCCL communicator
(csrc/comm.hip).  That layout has never run on more than one GPU in the build environment, so it is measured FIRST, by rank 0,
as its own N-rank job under a timeout (own process group, killed as a group): >= 1 warm-up + K timed videos of the 24-frame
clip, then of configs[2]'s 125-frame clip (`clip_125f`), after a first-forward self-check (library collectives bit-equal to
the host executor the gloo tests pin).  If that job exits 0 its line IS this run's line (`scaling: "strong"`,
`config.layout: "pairs" | "tshard"`, `rccl_communicators` filled) and the N ranks then time `replicas` — one independent
24-frame video per GPU, no data-path collective — as the side figure.  If it fails or times out, `replicas` (weak scaling) is
the headline and `config.layout_fallback` carries the reason: a hang of the RCCL path can cost the strong-scaling figure, never
the run.  Odd N > 1 has no collective layout: replicas.  `--parallel replicas | pairs | tshard` select a layout explicitly.
`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment launches its own N ranks (re-exec under
torch.distributed.run on 127.0.0.1, the reference's launcher does the same: scripts/videocrafter/ddp_wrapper.py:9-13).
Weights are random-init of the exact ModelScope architecture (no checkpoints offline).

Prints ONE JSON line (rank 0) with the driver's fields (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, ...).
A plain run only sets up, warms up, times the K steps and prints that line.  `--dump-outputs DIR` also writes what the last timed
step returned (the uint8 frames, as float32) to DIR/frames.npy: same arguments, same inputs, so two builds compare output for output.
`--full` adds the side measurements below (and, at N > 1, configs[2]'s 125-frame clip beside the frame-parallel headline):
  roofline     — dominant kernel = the MFMA implicit-GEMM family (conv3x3 / temporal conv /
                 linear): algorithmic FLOPs of its launches in one UNet step / their summed
                 durations, measured live with HIP events on the launch stream
                 + `calibration`: an 8192^3 fp16 GEMM of the same kernel family on random data before and after the timed
                 region (TF/s) and the clocks / power amd-smi reports — boxes differ by +-5-10 %, this makes lines comparable
  cpu_baseline — the oracle port (oracle/torch_port.py, fp32, torch CPU) timed on the host
                 cores on a bounded sample of the same workload, extrapolated to frames/s; beside it the REAL reference's
                 own CPU timings recorded when the goldens were generated (tests/golden/*.npz `timing`)
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0      # dense fp16/bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
UNET_TFLOP_PER_FRAME = 0.3057  # algorithmic 2*MAC per frame per forward @256x256
VAE_TFLOP_PER_FRAME = 0.622


def random_weights_(module, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.ndim >= 2:
                p.normal_(0, 1.0 / p[0].numel() ** 0.5, generator=g)
            elif n.endswith("weight"):
                p.normal_(1.0, 0.1, generator=g)
            else:
                p.normal_(0.0, 0.05, generator=g)


DUMP_MAX_BYTES = 48 << 20      # --dump-outputs: an array larger than this in float32 is written as a seeded sample (values + indices <= this)


def dump_outputs(path, arrays):
    """--dump-outputs DIR: the arrays the timed path returned in its last step, as DIR/<name>.npy in float32.  An array of more than
    DUMP_MAX_BYTES in float32 (the 24-frame 256x256 video is 18 MiB) is written as a fixed, seeded sample of its flattened values
    (DIR/<name>.npy) together with the flat indices of that sample (DIR/<name>_index.npy, float64)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)      # (sample_text2video returns numpy)
        if a.size * 4 > DUMP_MAX_BYTES:
            idx = np.unique(np.random.default_rng(0).integers(0, a.size, DUMP_MAX_BYTES // 12))
            np.save(os.path.join(path, f"{name}_index.npy"), idx.astype(np.float64))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, f"{name}.npy"), a.astype(np.float32))


def _usable_cores():
    """Host cores this process may really use: affinity mask, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def cpu_baseline_worker(frames, ddim_steps):
    """Runs in a child process (bounded by a timeout in the parent): the oracle port
    (oracle/torch_port.py, fp32) on the host cores — ONE UNet forward of the workload's own clip (b=1, up to 24 frames
    @256x256: 7.3 TFLOP, the unit the sampling loop repeats 2 x steps times; rounds 1-3 timed 8 frames and scaled) and ONE VAE
    frame decode (0.62 TFLOP): ~10-15 s of CPU work on 16 cores.  frames/s for the whole workload is
    1 / (2*steps*t_unet_per_frame + t_vae_frame); for clips longer than 24 frames the UNet cost is linear in F.
    Weights are seeded synthetic (timing does not depend on their values)."""
    from oracle import configs, synth, torch_port as tp
    from sd_webui_text2video_amd import unet as U, vae as V
    cores = _usable_cores()
    threads = min(cores, 64)          # torch CPU ops stop scaling (and can thrash) far beyond this
    torch.set_num_threads(threads)
    cfg, ddcfg = configs.MODELSCOPE_UNET, configs.VAE_DDCONFIG
    t0 = time.time()
    spec = synth.param_spec(U.UNetSD(**cfg, init_weights=False))
    g = torch.Generator().manual_seed(0)
    sd = {}
    for n, shp in spec:
        if len(shp) > 1:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            sd[n] = torch.empty(shp).normal_(0, fan_in ** -0.5)
        else:
            sd[n] = torch.ones(shp) if n.endswith("weight") else torch.zeros(shp)
    t_w = time.time() - t0
    fs = max(1, min(int(frames), 24))
    x = torch.randn(1, 4, fs, 32, 32, generator=g)
    y = torch.randn(1, 77, 1024, generator=g)
    with torch.no_grad():
        t0 = time.time()
        tp.unet_forward(sd, cfg, x, torch.tensor([500]), y)
        t_unet = time.time() - t0
    del sd
    vspec = synth.param_spec(V.AutoencoderKL(ddcfg, 4, init_weights=False))
    vsd = synth.synth_state_dict(vspec, seed=3)
    z = torch.randn(1, 4, 32, 32, generator=g)
    with torch.no_grad():
        t0 = time.time()
        tp.vae_decode(vsd, ddcfg, z)
        t_vae = time.time() - t0
    per_frame = 2 * ddim_steps * (t_unet / fs) + t_vae
    print(json.dumps({"value": round(1.0 / per_frame, 5), "unit": "frames/s", "cores": threads, "kind": "port",
                      "sample": f"oracle/torch_port.py fp32, {threads} torch threads ({cores} usable host cores): 1 UNet forward "
                                f"b=1 {fs}f@256x256 = {t_unet:.2f}s + 1 VAE frame decode = {t_vae:.2f}s (weights built in "
                                f"{t_w:.0f}s, untimed); x {ddim_steps} steps x 2 (CFG) + decode of {frames} frames"}))


def reference_cpu_timing():
    """The REAL reference's CPU timings, recorded by tests/golden/make_golden_full.py when it ran the reference's own classes
    (fp32, torch CPU) in the build container: [seconds of one 24-frame forward, seconds of the 50-step DDIM_Gaussian CFG loop
    (100 forwards), torch threads].  /root/reference cannot travel to the GPU box, so this is a recorded figure of another
    host, reported beside the live port timing — not a measurement of this run."""
    try:
        import numpy as np
        path = os.path.join(ROOT, "tests", "golden", "modelscope_24f.npz")      # (the _w16 run shared the cores with other jobs)
        t_fwd, t50, threads = [float(v) for v in np.load(path)["timing"]]
        return {"value": round(24.0 / t50, 5), "unit": "frames/s", "cores": int(threads), "kind": "reference",
                "sample": f"kabachuha/sd-webui-text2video's own UNetSD + Txt2VideoSampler.sample_loop, fp32, {int(threads)} torch threads in "
                          f"the build container (recorded in {os.path.basename(path)}): 50 DDIM_Gaussian steps x 2 forwards of 24f@256x256 = "
                          f"{t50:.0f}s (one forward {t_fwd:.1f}s); VAE decode not included (< 1 %)"}
    except Exception as exc:                           # noqa: BLE001
        return {"value": None, "kind": "reference", "sample": f"no recorded timing: {exc}"}


def cpu_baseline(frames, ddim_steps, timeout_s=240):
    out = _cpu_baseline_port(frames, ddim_steps, timeout_s)
    out["reference_recorded"] = reference_cpu_timing()
    return out


def _cpu_baseline_port(frames, ddim_steps, timeout_s=240):
    import subprocess
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", "--frames", str(frames),
                              "--ddim-steps", str(ddim_steps)], capture_output=True, text=True, timeout=timeout_s,
                             env={**os.environ, "HIP_VISIBLE_DEVICES": "", "WORLD_SIZE": "1"})
        for line in reversed(out.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return {"value": None, "unit": "frames/s", "cores": _usable_cores(), "kind": "port",
                "sample": "cpu baseline worker failed: " + out.stderr[-300:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "frames/s", "cores": _usable_cores(), "kind": "port",
                "sample": f"cpu baseline worker exceeded {timeout_s}s"}


def pmc_traffic():
    """HBM bytes per launch of the GEMM family from the committed PMC passes (collected with
    tools/gpu_profile.sh -> tools/pmc_post.py; counters cannot be read from inside this process)."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    path = next((q for q in (os.path.join(here, f"r0{r}_pmc_traffic.json") for r in (5, 4, 3, 2, 1)) if os.path.exists(q)), "")
    try:
        with open(path) as fh:
            return round(json.load(fh)["hbm_bytes_per_launch"])
    except (OSError, KeyError, ValueError):
        return None


def gemm_algorithmic_bytes(op) -> int:
    """Unique operand + result bytes of one GEMM op: activations once (the 9 / 3 conv taps re-read the same
    rows), weights once, fp32 residual once, output once; split-K adds its fp32 slabs (written + read)."""
    i = op.i
    M, N, K, gather, epi, split = i[0], i[1], i[2], i[7], i[16], max(i[19], 1)
    if gather == 0:
        a = M * K * 2
    elif gather == 2:
        a = M * i[10] * 2
    else:
        a = (M * max(i[11], 1) ** 2 // (4 if i[12] else 1)) * i[10] * 2
    n_out = N // 2 if epi == 1 else N
    out = M * n_out * (4 if i[17] == 1 else 2)
    if epi == 4:           # T2V_EPI_GN: the normalised fp16 tensor (+ its low-order image); the result itself only if someone else reads it
        out = (0 if i[29] else out) + M * N * 2 * (2 if i[27] else 1)
    res = M * n_out * 4 if op.p[4].space != "null" else 0
    slabs = 2 * split * M * N * 4 if split > 1 else 0
    return a + N * K * 2 + out + res + slabs


def gemm_strict_bytes(op) -> int:
    """The floor any fp16 design pays: fp16 activations once + weights once + an fp16 result (no fp32 residual stream,
    no split-K slabs) — what VERDICT r01 asks the PMC traffic to be compared with."""
    i = op.i
    M, N, K, gather, epi = i[0], i[1], i[2], i[7], i[16]
    if gather == 0:
        a = M * K * 2
    elif gather == 2:
        a = M * i[10] * 2
    else:
        a = (M * max(i[11], 1) ** 2 // (4 if i[12] else 1)) * i[10] * 2
    return a + N * K * 2 + M * (N // 2 if epi == 1 else N) * 2


def smi_snapshot():
    """Clocks / power of GPU 0 as amd-smi (or rocm-smi) reports them right now; None when neither tool answers."""
    import subprocess
    for cmd in (["amd-smi", "metric", "-g", "0", "--clock", "--power", "--json"], ["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--json"]):
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=20)
            if out.returncode != 0 or "{" not in out.stdout:
                continue
            txt = out.stdout[out.stdout.index("{") if out.stdout.lstrip().startswith("{") else out.stdout.index("["):]
            doc = json.loads(txt)
            flat = {}

            def walk(prefix, node):
                if isinstance(node, dict):
                    if set(node) >= {"value", "unit"}:
                        flat[prefix] = f"{node['value']} {node['unit']}"
                        return
                    for k, v in node.items():
                        walk(f"{prefix}.{k}" if prefix else str(k), v)
                elif isinstance(node, list):
                    for k, v in enumerate(node):
                        walk(f"{prefix}[{k}]", v)
                elif node not in (None, "N/A", ""):
                    flat[prefix] = node
            walk("", doc)
            keep = {k: v for k, v in flat.items() if any(t in k.lower() for t in ("gfx_0.clk", "gfx_0.min", "gfx_0.max", "mem_0.clk", "socket_power",
                                                                                   "sclk", "mclk", "power"))}
            return {"tool": cmd[0], **dict(list(keep.items())[:12])}
        except Exception:                              # noqa: BLE001
            continue
    return None


def calibration_gemm(dev, n=8192, reps=8):
    """TF/s of an n^3 fp16 GEMM (256x256 tile of the product's own gemm2 kernel, N(0,1) operands): the box's sustained matrix
    rate under this chip's power limit, the quantity that differs between boxes of the pool."""
    from sd_webui_text2video_amd.program import BoundProgram, Program, Ref
    P = Program("calibration")
    P.force_tile = 1
    a, out = P.alloc(n, n, "f16"), P.alloc(n, n, "f16")
    P.gemm("calibration", a, Ref("weight", 0, "w"), n, n, out, allow_splitk=False)
    P.ops = P.ops * reps
    arena = torch.zeros(P.arena.high + 256, dtype=torch.uint8, device=dev)
    arena.view(torch.float16).normal_(0, 1)
    w = torch.empty(n, n, device=dev, dtype=torch.float16).normal_(0, 1)
    bp = BoundProgram(P, arena.data_ptr(), {"w": w.data_ptr()})
    st = torch.cuda.current_stream(dev).cuda_stream
    bp.run({}, st)
    ms = sorted(bp.run_timed({}, st))[reps // 2]
    torch.cuda.synchronize(dev)
    return round(2.0 * n ** 3 / ms / 1e9, 1)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _launch_env():
    """Environment of a self-launched job: no inherited rank variables, the dmabuf IPC setting RCCL needs on this pool."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK",
                                                            "ROLE_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def self_launch(n: int, argv, timeout_s=None, capture=False, stderr_path=None):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves, one process per GPU, under
    torch.distributed.run on 127.0.0.1 (ddp_wrapper.py:9-13 does the same for the reference's VideoCrafter sampling).
    -> (exit code, stdout or None)."""
    import subprocess
    if os.environ.get("T2V_BENCH_ONE_DEVICE") != "1" and "--launch-check" not in argv:
        have = torch.cuda.device_count()
        if have < n:
            print(f"[bench] --gpus {n} but this node exposes {have} GPU(s)", file=sys.stderr, flush=True)
            return 2, None
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    # The bounded side job (capture) gets its own session = its own process group: on a timeout the launcher AND every rank it
    # started are killed together (a hung RCCL call must not leave orphaned ranks holding the GPUs for whatever runs next).
    # The top-level self-launch stays in the caller's process group, so whoever stops `python bench.py` stops the ranks too.
    import signal
    errf = open(stderr_path, "w") if stderr_path else None      # the bounded job's stderr: kept for the fallback's `reason`
    proc = subprocess.Popen(cmd, env=_launch_env(), stdout=subprocess.PIPE if capture else None, stderr=errf, text=True,
                            start_new_session=capture)

    def stop():
        try:
            if capture:
                os.killpg(proc.pid, signal.SIGKILL)
            else:
                proc.kill()
        except ProcessLookupError:
            pass
    try:
        out, _ = proc.communicate(timeout=timeout_s)
        return proc.returncode, out
    except subprocess.TimeoutExpired:
        stop()
        out, _ = proc.communicate()
        return 124, out
    except BaseException:
        stop()
        raise


def collective_layout_job(n: int, args, timeout_s: int):
    """The frame-parallel layout of N GPUs (pairs at N = 2, T-shard x CFG pair for even N >= 4) as its OWN N-rank job, bounded
    by a timeout: a failure or hang of the RCCL path is reported, it cannot take the run down.  Called by rank 0 BEFORE the
    outer job's ranks touch their GPUs.  -> {"ok": True, "line": <the job's JSON line>, ...} | {"ok": False, "reason": ...}."""
    import tempfile
    mode = "pairs" if n == 2 else "tshard"
    argv = ["--gpus", str(n), "--parallel", mode, "--steps", str(args.steps), "--warmup", str(max(1, args.warmup)),
            "--ddim-steps", str(args.ddim_steps), "--height", str(args.height), "--width", str(args.width), "--no-cpu-baseline",
            "--also-batched", "0", "--no-collective-job", "--also-frames", str(args.also_frames)]
    if args.frames:
        argv += ["--frames", str(args.frames)]
    if args.full:
        argv += ["--full"]
    if args.dump_outputs:
        argv += ["--dump-outputs", args.dump_outputs]      # this job computes the headline: its rank 0 writes the outputs
    err_path = os.path.join(tempfile.gettempdir(), f"t2v_bench_collective_{os.getpid()}.err")
    t0 = time.time()
    rc, out = self_launch(n, argv, timeout_s=timeout_s, capture=True, stderr_path=err_path)
    job_s = round(time.time() - t0, 1)
    tail = ""
    try:
        with open(err_path) as fh:
            txt = fh.read()
        sys.stderr.write(txt)                      # the job's diagnostics stay visible in this run's stderr
        keep = [ln for ln in txt.splitlines() if ln.strip() and "Warning" not in ln]
        marked = [ln for ln in keep if "[bench]" in ln] or [ln for ln in keep if ("Error" in ln or "error" in ln) and "traceback" not in ln]
        tail = " | ".join((marked or keep)[-3:])[-600:]
        os.remove(err_path)
    except OSError:
        pass
    line = next((ln for ln in reversed((out or "").splitlines()) if ln.startswith("{")), None)
    if rc == 0 and line:
        return {"ok": True, "layout": mode, "line": json.loads(line), "job_s": job_s, "timeout_s": timeout_s}
    why = f"timed out after {timeout_s}s" if rc == 124 else (f"exit code {rc}" if rc != 0 else "printed no JSON line")
    return {"ok": False, "layout": mode, "exit_code": rc, "job_s": job_s, "timeout_s": timeout_s, "reason": f"{why}: {tail}" if tail else why}


def _handoff_path():
    """Where rank 0 publishes the collective job's result to the other ranks of THIS launch (one node: a local file; the ranks
    share their parent — the launcher agent — and the rendezvous port)."""
    import tempfile
    return os.path.join(tempfile.gettempdir(), f"t2v_bench_handoff_{os.getppid()}_{os.environ.get('MASTER_PORT', '0')}.json")


def collective_first(world: int, rank: int, args, t_start: float):
    """Every rank returns the same dict: rank 0 runs `collective_layout_job` while the others wait (idle, no GPU context yet)."""
    path = _handoff_path()
    if rank == 0:
        try:
            res = collective_layout_job(world, args, args.collective_timeout)
        except Exception as exc:                    # noqa: BLE001 — the other ranks are waiting for SOME answer
            res = {"ok": False, "layout": "pairs" if world == 2 else "tshard", "reason": f"launcher failed: {type(exc).__name__}: {exc}"}
        with open(path + ".tmp", "w") as fh:
            json.dump(res, fh)
        os.replace(path + ".tmp", path)
        return res
    deadline = time.time() + args.collective_timeout + 180
    while time.time() < deadline:
        try:
            if os.path.getmtime(path) >= t_start - 5:
                with open(path) as fh:
                    return json.load(fh)
        except (OSError, ValueError):
            pass
        time.sleep(0.5)
    return {"ok": False, "layout": "pairs" if world == 2 else "tshard", "reason": "rank 0 never published the collective job's result"}


LVDM_UNET_TFLOP_16F = 3.302     # UNetModel.forward, 16 frames @256x256 (2*MAC, conv + matmul)


def main_lvdm(args):
    """`bench.py --model lvdm`: BASELINE.json configs[4] — VideoCrafter LVDM fp16, 16 frames @256x256 — through the reference's
    own entry point for that model, `sample_text2video` (videocrafter/sample_text2video.py:92-152 as process_videocrafter.py:71-78
    calls it: n_samples = batch_size = 1, DDIM, CFG 7.5): 50 lvdm-DDIM steps (one b=2 UNetModel forward + one fused update kernel
    each) + decode_first_stage of the 16 frames + uint8 conversion.  One step = one whole video; 1 GPU."""
    assert args.gpus == 1, "the VideoCrafter line is a single-GPU configuration (configs[4])"
    from sd_webui_text2video_amd import configs, videocrafter as VC
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    frames = args.frames or 16
    ld = VC.LatentDiffusion(configs.LVDM_UNET, dict(ddconfig=configs.VAE_DDCONFIG, embed_dim=4), image_size=[args.height // 8, args.width // 8],
                            video_length=frames, init_weights=False, **configs.LVDM_SCHEDULE)
    ld = ld.half().to(dev).eval()
    net = ld.model.diffusion_model
    random_weights_(net, 0)
    random_weights_(ld.first_stage_model, 3)
    g = torch.Generator().manual_seed(1)
    table = {"a prompt": torch.randn(1, 77, 768, generator=g).half().to(dev), "": torch.randn(1, 77, 768, generator=g).half().to(dev)}

    class Clip:                      # the text tower is outside the timed path (text_encoder.py: 1.9 ms for cond + uncond)
        def encode(self, prompts):
            return torch.cat([table[p] for p in prompts], 0)
    ld.cond_stage_model = Clip()
    smp = VC.DDIMSampler(ld)

    def one(seed):
        smp.noise_gen.manual_seed(seed)
        return VC.sample_text2video(ld, "a prompt", "", 1, 1, sample_type="ddim", sampler=smp, ddim_steps=args.ddim_steps, eta=0.0,
                                    cfg_scale=7.5, decode_frame_bs=None, show_denoising_progress=False, num_frames=frames)
    one(0)
    for i in range(args.warmup):
        one(1 + i)
    torch.cuda.synchronize(dev)
    cal_before = calibration_gemm(dev) if args.full else None
    t0 = time.perf_counter()
    out = None
    for i in range(args.steps):
        out = one(100 + i)
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    assert out.shape == (1, frames, args.height, args.width, 3) and out.dtype.name == "uint8"
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"frames": out})
    ms_per_step = elapsed / args.steps * 1e3
    named = "BASELINE.json configs[4]" if (frames, args.height, args.width, args.ddim_steps) == (16, 256, 256, 50) else "custom geometry"
    result = {
        "metric": f"denoised frames/sec (UNet+VAE), VideoCrafter LVDM {frames}f@{args.width}x{args.height}",
        "value": round(frames * args.steps / elapsed, 4), "unit": "frames/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16",
        "data": "synthetic",
        "config": {"workload": f"VideoCrafter LVDM fp16 (random-init 0.96B UNetModel + VAE decoder), {frames} frames @ {args.width}x{args.height}, "
                               f"{args.ddim_steps} lvdm DDIM steps, CFG 7.5, eta 0 ({named}); one step = one whole video through sample_text2video",
                   "frames_per_video": frames, "videos_per_batch": 1, "layout": "single", "layout_requested": args.parallel,
                   "parallelism": "1 GPU: cond+uncond batched as b=2", "rccl_communicators": []},
    }
    if not args.full:
        emit(result)
        return
    cal_after = calibration_gemm(dev)
    px = (args.height // 8) * (args.width // 8) / 1024.0
    video_tflop = (2 * args.ddim_steps * LVDM_UNET_TFLOP_16F / 16 + VAE_TFLOP_PER_FRAME) * px * frames
    x = torch.randn(2, 4, frames, args.height // 8, args.width // 8, device=dev)
    y = torch.cat([table["a prompt"], table[""]], 0)
    t = torch.full((2,), 500, device=dev)
    net.forward_timed(x, t, y)
    _, ms, prog = net.forward_timed(x, t, y)
    gemm_ms = sum(m for op, m in zip(prog.ops, ms) if op.kind == 1)
    gemm_fl = sum(op.flops for op in prog.ops if op.kind == 1)
    n_gemm = sum(1 for op in prog.ops if op.kind == 1)
    step_ms = sum(ms)
    achieved = gemm_fl / (gemm_ms * 1e-3) / 1e12
    step_ms_b2b = forward_ms_back_to_back(net, x, t, y, dev, context_kw=True)
    fused, plain_ms, plain_fl = fused_norm_split(prog, ms, gemm_ms, gemm_fl)
    result["roofline"] = {
        "bound": "mfma", "kernel": "gemm2_kernel / gemm_kernel family (conv (1,3,3) / linear)", "achieved": round(achieved, 1),
        "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / MFMA_PEAK_TFLOPS, 4), "traffic": None,
        "launches_per_unet_step": n_gemm, "avg_launch_us": round(gemm_ms / n_gemm * 1e3, 2),
        "fused_norm_launches": len(fused),
        "achieved_launches_without_a_fused_norm": round(plain_fl / (plain_ms * 1e-3) / 1e12, 1) if plain_ms > 0 else None,
        "unet_step_ms_events": round(step_ms, 3),
        "unet_step_ms": round(step_ms_b2b, 3),
        "unet_step_frac_of_peak_back_to_back": round(prog.total_flops() / (step_ms_b2b * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
        "unet_step_frac_of_peak": round(prog.total_flops() / (step_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
        "calibration": {"gemm_8192_tflops_before": cal_before, "gemm_8192_tflops_after": cal_after, "smi_after": smi_snapshot()},
        "whole_video": {"tflop": round(video_tflop, 1), "tflops_per_gpu": round(video_tflop / (ms_per_step * 1e-3), 1),
                        "frac": round(video_tflop / (ms_per_step * 1e-3) / MFMA_PEAK_TFLOPS, 4)}}
    emit(result)


def forward_ms_back_to_back(net, x, t, y, dev, n=10, context_kw=False):
    """The same forward WITHOUT a HIP event after every op: two events on the launch stream around n back-to-back forwards."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once():
        net.single_timestep = True                   # (one timestep for the cond | uncond pair, as the samplers say: the prefix is shared)
        return net(x, t, context=y) if context_kw else net(x, t, y)
    once()
    ev0.record()
    for _ in range(n):
        once()
    ev1.record()
    torch.cuda.synchronize(dev)
    return ev0.elapsed_time(ev1) / n


def fused_norm_split(prog, ms, gemm_ms, gemm_fl):
    """Members of the GEMM family that also carry a normalisation in their epilogue (round 5: GroupNorm / LayerNorm of the result, statistics
    exchanged between the launch's workgroups) — their time includes that work, their FLOPs do not.  -> (those, ms of the rest, FLOPs of the rest)"""
    fused = [(op, m) for op, m in zip(prog.ops, ms) if op.kind == 1 and (op.i[16] == 4 or (op.i[7] == 0 and op.i[8] in (1, 2) and op.i[16] == 0))]
    return fused, gemm_ms - sum(m for _, m in fused), gemm_fl - sum(op.flops for op, _ in fused)


_REAL_STDOUT = None


def claim_stdout():
    """From here on file descriptor 1 carries NOTHING but the one JSON line: everything else a rank writes to stdout — the gloo /
    RCCL banners of process-group creation ("[Gloo] Rank 0 is connected to ..."), progress bars, library notices — is sent to
    stderr at the descriptor level (C++ libraries do not go through sys.stdout)."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def emit(obj):
    line = (json.dumps(obj) + "\n").encode()
    if _REAL_STDOUT is None:
        sys.stdout.write(line.decode())
        sys.stdout.flush()
    else:
        os.write(_REAL_STDOUT, line)


def choose_layout(world: int, requested: str, frames_arg: int = 0):
    """-> (layout of THIS job's ranks, frames per video).  The clip is configs[1]'s 24 frames in every layout (BASELINE.json's
    metric names it; configs[2]'s 125-frame clip is timed beside it: `--also-frames`).  auto: `single` on one GPU; on N > 1 the
    frame-parallel layout is measured first as its own bounded job (`collective_first`) and THIS job's ranks run `replicas` — the
    side figure, or the headline if that job failed.  `--parallel pairs | tshard | replicas` select a layout explicitly (tshard:
    ONE clip, frames sharded along T over world / 2 GPUs x the CFG pair — north_star's layout).  `--frames` overrides the clip."""
    mode = requested
    if mode == "auto":
        mode = "single" if world == 1 else "replicas"
    if world == 1:
        mode = "single"
    return mode, (frames_arg or 24)


def collective_layout_of(world: int):
    """The frame-parallel layout `auto` measures first at this N (None: there is none — odd N, one GPU)."""
    return "pairs" if world == 2 else ("tshard" if world >= 4 and world % 2 == 0 else None)


BASELINE_CONFIGS = {(24, 256, 256): "BASELINE.json configs[1]", (125, 256, 256): "BASELINE.json configs[2]",
                    (24, 576, 1024): "BASELINE.json configs[3]", (8, 256, 256): "BASELINE.json configs[0] geometry"}


def main():
    t_start = time.time()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed videos")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=0, help="frames per video; default 24 (configs[1], the clip BASELINE.json's metric names)")
    ap.add_argument("--also-frames", type=int, default=-1,
                    help="N > 1, frame-parallel layouts: also time a clip of this many frames in the same job and report it as `clip_125f` "
                         "(default: 125 = configs[2] with --full, else skipped; with --frames: skipped; 0 = skip)")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--videos", type=int, default=1,
                    help="independent videos per batch and GPU (default 1 = the reference's one-video pipeline; the UNet step "
                         "becomes one b=2*videos forward)")
    ap.add_argument("--also-batched", type=int, default=4,
                    help="at N=1 with --videos 1: also time one pass with this many videos per batch and report it as "
                         "`batched` beside the headline (0 / 1 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true", help="skip the per-op roofline / calibration section (launch-path rehearsals only)")
    ap.add_argument("--parallel", default="auto", choices=["auto", "replicas", "pairs", "tshard"],
                    help="N>1 layout; auto = the frame-parallel layout of that N (pairs at N=2, T-shard x CFG pair for even N>=4: ONE clip on "
                         "all GPUs) measured first as its own bounded job and reported as the headline, `replicas` (one video per GPU) "
                         "beside it — or as the headline, with the reason, if that job fails; replicas / pairs / tshard force a layout")
    ap.add_argument("--no-collective-job", action="store_true",
                    help="N>1, --parallel auto: do not run the bounded frame-parallel job; the headline is replicas")
    ap.add_argument("--collective-timeout", type=int, default=int(os.environ.get("T2V_BENCH_COLLECTIVE_TIMEOUT", 420)),
                    help="seconds the bounded frame-parallel job may take before it is abandoned (then: replicas headline + reason)")
    ap.add_argument("--model", default="modelscope", choices=["modelscope", "lvdm"],
                    help="modelscope (default; configs[1]-[3]) or lvdm = VideoCrafter, BASELINE.json configs[4]: 16 frames @256x256 through "
                         "sample_text2video (1 GPU; reported beside the headline, never the driver's default line)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline / per-kernel figures, GEMM calibration, the CPU baseline, "
                         "the batched pass (--also-batched) and, at N > 1, the second clip (--also-frames); off by default")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the uint8 frames) to DIR/frames.npy as float32")
    ap.add_argument("--cpu-baseline-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launch-check", action="store_true",
                    help="only check the launch path: ranks rendezvous over gloo, all-reduce their ranks, rank 0 prints one JSON line (no GPU)")
    args = ap.parse_args()
    if args.also_frames < 0:
        args.also_frames = 125 if args.full and not args.frames else 0
    if args.cpu_baseline_worker:
        cpu_baseline_worker(args.frames, args.ddim_steps)
        return

    if args.gpus == 1 or "WORLD_SIZE" in os.environ:
        claim_stdout()            # (the self-launching parent below keeps its stdout: its ranks inherit it and claim it themselves)
    if args.model == "lvdm":
        main_lvdm(args)
        return

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: start the ranks ourselves (one process per GPU); their rank 0 prints the JSON line
        rc, _ = self_launch(args.gpus, sys.argv[1:])
        sys.exit(rc)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.launch_check:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world > 1:
            dist.init_process_group(backend="gloo")
        v = torch.tensor([rank + 1], dtype=torch.int64)
        if world > 1:
            dist.all_reduce(v)
        assert world == args.gpus and int(v.item()) == world * (world + 1) // 2
        if rank == 0:
            emit({"launch_check": True, "n_gpus": world, "rank_sum": int(v.item())})
        if world > 1:
            dist.destroy_process_group()
        return
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE {world}"

    # ---- N > 1, auto: the frame-parallel layout FIRST, as its own bounded N-rank job (rank 0 launches it; nobody here has touched a GPU yet)
    requested = args.parallel
    coll = None
    if (world > 1 and requested == "auto" and not args.no_collective_job and collective_layout_of(world) is not None
            and os.environ.get("T2V_BENCH_COLLECTIVE_JOB", "1") != "0"):
        coll = collective_first(world, rank, args, t_start)
        if rank == 0:
            print(f"[bench] frame-parallel job ({coll.get('layout')}): " + ("ok, " + json.dumps({k: coll['line'][k] for k in ('value', 'ms_per_step')})
                                                                              if coll.get("ok") else "FAILED — " + str(coll.get("reason"))),
                  file=sys.stderr, flush=True)

    ctl = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # T2V_BENCH_ONE_DEVICE=1 (rehearsal of the N > 1 code path on a 1-GPU box): every rank on cuda:0, gloo instead of
        # RCCL (device buffers staged through the host, parallel.all_gather_into) — never a measurement configuration
        one_device = os.environ.get("T2V_BENCH_ONE_DEVICE") == "1"
        if one_device:
            # several processes share the GPU: the single-pass GroupNorm's grid barrier wants an otherwise idle device (its wait is
            # bounded — a co-tenant costs a reported fault, not a hang — but the rehearsal should not trip it) -> three-launch path
            os.environ.setdefault("T2V_GN_COOP", "0")
        dist.init_process_group(backend="gloo" if one_device else "nccl")      # "nccl" is RCCL on ROCm
        ctl = dist.new_group(backend="gloo")         # control plane (layout agreement), never on the data path
        if one_device:
            local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    from sd_webui_text2video_amd import _lib as L
    from sd_webui_text2video_amd import configs
    from sd_webui_text2video_amd import parallel, pipeline, unet as U, vae as V

    cfg, ddcfg = configs.MODELSCOPE_UNET, configs.VAE_DDCONFIG
    net = U.UNetSD(**cfg, init_weights=False).half().to(dev).eval()
    random_weights_(net, 0)
    ae = V.AutoencoderKL(ddcfg, 4, init_weights=False).half().to(dev).eval()
    random_weights_(ae, 3)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, autoencoder=ae, device=dev)
    pipe.diffusion.progress = False
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(1, 77, 1024, generator=g).half().to(dev)
    uncond = torch.randn(1, 77, 1024, generator=g).half().to(dev)

    mode, frames = choose_layout(world, requested, args.frames)

    def build(mode_, frames_, videos=args.videos):
        return parallel.make_runner(pipe, world, rank, frames=frames_, height=args.height, width=args.width,
                                    ddim_steps=args.ddim_steps, guidance=9.0, mode="pairs" if mode_ == "single" else mode_,
                                    videos=videos)

    def sync():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    def all_ok(ok: bool) -> bool:
        """Every rank learns whether ANY rank failed (gloo control group): the layout decision is collective."""
        if world == 1:
            return ok
        flag = torch.tensor([0 if ok else 1], dtype=torch.int32)
        dist.all_reduce(flag, group=ctl)
        return int(flag.item()) == 0

    def timed(runner_, n_warm, n_steps):
        for i in range(n_warm):
            runner_(cond, uncond, 1234 + i)
        sync()
        t0 = time.perf_counter()
        out_ = None
        for i in range(n_steps):
            out_ = runner_(cond, uncond, 1234 + i)
        sync()
        el = time.perf_counter() - t0
        L.async_status()                           # a kernel that gave up at a grid barrier invalidates the timing: fail loudly
        if world > 1:
            tmax = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            el = float(tmax.item())
        assert out_ is not None and out_.dtype == torch.uint8
        return el, out_

    # ---- this job's own layout: first pass (lowering, weight packing, communicator set-up) + the frame-parallel self-check
    runner, err, self_check = None, "", None
    try:
        runner = build(mode, frames)
        if os.environ.get("T2V_BENCH_INJECT_FAILURE") in ("all", str(rank)) and mode in ("pairs", "tshard"):   # rehearsal hook
            raise RuntimeError("injected failure (T2V_BENCH_INJECT_FAILURE)")
        if hasattr(runner, "self_check"):
            # first forward of the T-sharded UNet twice: exchanges inside the library (RCCL on the launch stream) vs the host
            # executor the gloo tests pin — bit-equal on every rank, or nothing is timed
            self_check = runner.self_check(cond)          # None: a layout without data-path collectives (replicas, one GPU)
            if self_check is not None and not self_check.get("ok", False):
                raise RuntimeError(f"frame-parallel self-check failed: {self_check}")
        runner(cond, uncond, 999)
        sync()
        ok = True
    except Exception as exc:                       # noqa: BLE001 — reported, never silent (below)
        ok, err = False, f"{type(exc).__name__}: {exc}"
    if not all_ok(ok):
        # Layouts are explicit in this job (auto's own ranks run replicas, which has no collective to fail): a layout that breaks
        # fails the job — the OUTER run, which launched it under a timeout, then reports replicas with this as the reason.
        print(f"[bench] rank {rank}: layout {mode!r} failed: {err or 'failure on another rank'}", file=sys.stderr, flush=True)
        raise RuntimeError(f"layout {mode!r} failed on rank {rank}: {err or 'another rank failed'}")
    side_only = bool(coll is not None and coll.get("ok"))     # the headline already exists: this job's replicas pass is the side figure
    cal_before = None
    if rank == 0 and args.full and not args.no_roofline and not side_only:
        try:
            cal_before = calibration_gemm(dev)
        except Exception:                          # noqa: BLE001
            cal_before = None
    n_warm, n_steps = (1, min(args.steps, 2)) if side_only else (args.warmup, args.steps)
    elapsed, out = timed(runner, n_warm, n_steps)
    if rank == 0 and args.dump_outputs and not side_only:     # (side_only: the frame-parallel job that computed the headline wrote them)
        dump_outputs(args.dump_outputs, {"frames": out})

    total_frames = runner.frames_per_video_all_ranks * n_steps
    value = total_frames / elapsed
    ms_per_step = elapsed / n_steps * 1e3
    geom = (frames, args.height, args.width)
    named = BASELINE_CONFIGS.get(geom, "not a BASELINE.json configuration") if args.ddim_steps == 50 else \
        f"{BASELINE_CONFIGS.get(geom, 'custom geometry')} with {args.ddim_steps} instead of 50 steps"
    rehearsal = world > 1 and os.environ.get("T2V_BENCH_ONE_DEVICE") == "1"

    if side_only:
        # ---- the frame-parallel job's line IS the line; this job adds the replicas figure --------------------------------
        result = coll["line"]
        result["config"]["layout_requested"] = requested
        result["replicas"] = {"value": round(value, 4), "unit": "frames/s", "ms_per_step": round(ms_per_step, 2), "scaling": "weak",
                              "videos_in_flight": world, "steps": n_steps, "warmup": n_warm,
                              "note": "one independent 24-frame video per GPU (no data-path collective), timed by the N ranks of the outer job "
                                      "after the frame-parallel job; not the headline"}
        result["collective_job"] = {"layout": coll["layout"], "job_s": coll["job_s"], "timeout_s": coll["timeout_s"],
                                    "note": "the headline was measured FIRST, by its own N-rank job under this timeout (own process group, "
                                            "killed as a group on expiry); had it failed, replicas would be the headline with the reason"}
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            try:
                os.remove(_handoff_path())
            except OSError:
                pass
            emit(result)
        return

    result = {
        "metric": f"denoised frames/sec (UNet+VAE), ModelScope {frames}f@{args.width}x{args.height}",
        "value": round(value, 4), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 2), "higher_is_better": True,
        "scaling": "weak" if mode in ("single", "replicas") else "strong", "vs_baseline": None,
        "dtype": "f16", "data": "synthetic",
        "config": {"workload": f"ModelScope t2v fp16 (random-init 1.41B UNetSD + VAE decoder), {frames} frames @ "
                               f"{args.width}x{args.height}, {args.ddim_steps} DDIM_Gaussian steps, CFG 9.0 "
                               f"({named}); one step = one whole video" + ("" if args.videos == 1 else f" x {args.videos} per batch"),
                   "frames_per_video": runner.frames_per_video_all_ranks, "videos_per_batch": args.videos,
                   "layout": mode, "layout_requested": requested, "parallelism": runner.describe},
    }
    if coll is not None:          # the frame-parallel job ran and failed: replicas is the headline, and the line says why
        result["config"]["layout_fallback"] = {"requested_layout": coll.get("layout"), "reason": coll.get("reason"),
                                               "exit_code": coll.get("exit_code"), "job_s": coll.get("job_s"),
                                               "timeout_s": coll.get("timeout_s")}
    if self_check is not None:
        result["config"]["self_check"] = self_check
    if rehearsal:
        result["data"] = "synthetic; REHEARSAL: all ranks on one GPU over gloo — not a measurement"
    result["config"]["rccl_communicators"] = runner.communicators() if hasattr(runner, "communicators") else []

    if world > 1 and mode in ("pairs", "tshard") and args.also_frames and args.also_frames != frames:
        # configs[2]'s clip (125 frames) in the same layout, same job: 1 warm-up + K timed videos
        key, ok2, note = ("clip_125f" if args.also_frames == 125 else "clip_other"), True, ""
        try:
            net.t_shard = None
            big = build(mode, args.also_frames, videos=1)
            big(cond, uncond, 998)
            sync()
            k2 = min(args.steps, 5)                # the second clip is a side figure: at most 5 timed clips, whatever K the driver asks for
            el, _ = timed(big, 1, k2)
            bgeom = (args.also_frames, args.height, args.width)
            result[key] = {
                "frames_per_video": args.also_frames, "value": round(args.also_frames * k2 / el, 4), "unit": "frames/s",
                "ms_per_step": round(el / k2 * 1e3, 2), "steps": k2, "warmup": 1, "scaling": "strong",
                "workload": BASELINE_CONFIGS.get(bgeom, "custom geometry") if args.ddim_steps == 50 else
                f"{BASELINE_CONFIGS.get(bgeom, 'custom geometry')} with {args.ddim_steps} instead of 50 steps",
                "parallelism": big.describe}
            del big
        except Exception as exc:                   # noqa: BLE001 — the headline stands; the side clip says what happened
            ok2, note = False, f"{type(exc).__name__}: {exc}"
            print(f"[bench] rank {rank}: {args.also_frames}-frame clip failed: {note}", file=sys.stderr, flush=True)
        if not all_ok(ok2):
            result[key] = {"frames_per_video": args.also_frames, "value": None, "note": "failed: " + (note or "on another rank")}

    cal0 = None
    if rank == 0 and args.full and not args.no_roofline:
        # ---- live roofline of the dominant kernel (HIP events on the launch stream) -------------
        try:
            cal0 = {"gemm_8192_tflops_after": calibration_gemm(dev), "smi_after": smi_snapshot()}
        except Exception as exc:                   # noqa: BLE001
            cal0 = {"error": f"{type(exc).__name__}: {exc}"}
        F_loc = runner.unet_frames
        net.t_shard = None
        # the program the sampler's guided step runs: ONE x_t for the cond | uncond pair (forward_cfg_pair: the prefix up to the first text
        # cross-attention is computed once, UNetSD.share_cfg_prefix) — b = 2 * videos contexts, `videos` latents
        x = torch.randn(max(1, runner.unet_batch // 2), 4, F_loc, args.height // 8, args.width // 8, device=dev)
        nv = max(1, runner.unet_batch // 2)
        y = torch.cat([cond.expand(nv, -1, -1), uncond.expand(nv, -1, -1)], 0)[: runner.unet_batch].contiguous()
        t = torch.full((runner.unet_batch,), 500, device=dev)
        net.forward_timed(x, t, y)
        _, ms, prog = net.forward_timed(x, t, y)
        gemm_ms = sum(m for op, m in zip(prog.ops, ms) if op.kind == 1)
        gemm_fl = sum(op.flops for op in prog.ops if op.kind == 1)
        n_gemm = sum(1 for op in prog.ops if op.kind == 1)
        alg_bytes = sum(gemm_algorithmic_bytes(op) for op in prog.ops if op.kind == 1)
        strict_bytes = sum(gemm_strict_bytes(op) for op in prog.ops if op.kind == 1)
        px = (args.height // 8) * (args.width // 8) / 1024.0
        video_tflop = (2 * args.ddim_steps * UNET_TFLOP_PER_FRAME + VAE_TFLOP_PER_FRAME) * px * runner.frames_per_video_all_ranks
        traffic = pmc_traffic() if (args.videos, frames, args.height, args.width, world) == (1, 24, 256, 256, 1) else None
        step_ms = sum(ms)
        achieved = gemm_fl / (gemm_ms * 1e-3) / 1e12
        step_ms_b2b = forward_ms_back_to_back(net, x, t, y, dev)
        fused, plain_ms, plain_fl = fused_norm_split(prog, ms, gemm_ms, gemm_fl)
        result["roofline"] = {
            "bound": "mfma", "kernel": "gemm2_kernel<WM,WN,TM,TN,BK,STAGES,MINW,GATHER,PP> + gemm_kernel<BM,BN,WM,WN,GATHER> (one implicit-GEMM family: conv3x3 / temporal conv / linear)",
            "achieved": round(achieved, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / MFMA_PEAK_TFLOPS, 4),
            # the committed PMC passes are of the b=2, 24-frame, 256x256 step
            "traffic": traffic,
            "launches_per_unet_step": n_gemm, "avg_launch_us": round(gemm_ms / n_gemm * 1e3, 2),
            "flops_per_unet_step_T": round(gemm_fl / 1e12, 3),
            "fused_norm_launches": len(fused),
            "achieved_launches_without_a_fused_norm": round(plain_fl / (plain_ms * 1e-3) / 1e12, 1) if plain_ms > 0 else None,
            "unet_step_ms_events": round(step_ms, 3),
            "unet_step_ms": round(step_ms_b2b, 3),
            "unet_step_frac_of_peak_back_to_back": round(prog.total_flops() / (step_ms_b2b * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
            "unet_step_tflops_all_kernels": round(prog.total_flops() / (step_ms * 1e-3) / 1e12, 1),
            "unet_step_frac_of_peak": round(prog.total_flops() / (step_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
            "geometry": f"one rank's UNet forward in this layout WITHOUT its exchanges: b={runner.unet_batch}, {F_loc} frames" +
                        ("; cond | uncond share the ops up to the first text cross-attention (executed FLOPs are counted, not the reference's 2 full forwards)"
                         if (runner.unet_batch == 2 and getattr(net, "share_cfg_prefix", False)) else ""),
            "traffic_unit": "HBM bytes per launch (FETCH_SIZE x2 + WRITE_SIZE, rocprofv3 --pmc, profiles/r0N_pmc_traffic.json)",
            # box calibration either side of the timed region: the same kernel family on an 8192^3 fp16 GEMM (random data)
            "calibration": {"gemm_8192_tflops_before": cal_before, **(cal0 or {}),
                            "note": "8192^3 fp16 GEMM, 256x256 tile of gemm2_kernel, N(0,1) operands, median of 8 launches (HIP events); "
                                    "boxes of the pool differ by +-5-10 % on it (power-limited clocks).  It identifies the box; it does NOT normalise "
                                    "the line (rounds 4-5: 1094 -> 17.75, 1108 -> 18.69, 1128 -> 17.04, 1160 -> 18.77 frames/s: sustained power under the "
                                    "real kernel mix differs too) — compare builds only by same-box A/B"},
            "algorithmic_bytes_per_launch": round(alg_bytes / n_gemm),
            "strict_bytes_per_launch": round(strict_bytes / n_gemm),
            "traffic_over_strict": round(traffic / (strict_bytes / n_gemm), 3) if traffic else None,
            "bytes_note": "algorithmic = this design (fp32 residual reads / fp32 stream outputs / split-K slabs included); strict = fp16 "
                          "activations once + weights once + fp16 result",
            # the WHOLE job against the matrix peak: SURVEY §8(d) FLOPs of every UNet forward and VAE frame / wall time / N GPUs
            "whole_video": {"tflop": round(video_tflop, 1), "tflops_per_gpu": round(video_tflop / (ms_per_step * 1e-3) / world, 1),
                            "frac": round(video_tflop / (ms_per_step * 1e-3) / world / MFMA_PEAK_TFLOPS, 4)},
        }
        if world == 1 and args.videos == 1:
            # `tflop` is the WORKLOAD's count (two full forwards per guided step); the program executes fewer where cond | uncond share
            # their prefix — both are printed so that neither rate is mistaken for the other
            executed = args.ddim_steps * prog.total_flops() / 1e12 + VAE_TFLOP_PER_FRAME * px * frames
            result["roofline"]["whole_video"].update(
                tflop_executed=round(executed, 1), frac_executed=round(executed / (ms_per_step * 1e-3) / MFMA_PEAK_TFLOPS, 4),
                note="tflop = SURVEY 8(d) count of the workload (2 UNet forwards per step + VAE); tflop_executed = what the program ran")
        if world == 1 and args.videos == 1 and args.also_batched > 1:
            # Reported beside the headline, never as `value`: the same workload with several videos per batch (the
            # reference's batch_count loop in one pass) — one warm-up pass, one timed pass.
            nv = args.also_batched
            r2 = parallel.make_runner(pipe, 1, 0, frames=frames, height=args.height, width=args.width,
                                      ddim_steps=args.ddim_steps, guidance=9.0, videos=nv)
            r2(cond, uncond, 4321)
            torch.cuda.synchronize(dev)
            tb = time.perf_counter()
            r2(cond, uncond, 4322)
            torch.cuda.synchronize(dev)
            tb = time.perf_counter() - tb
            result["batched"] = {"videos_per_batch": nv, "value": round(nv * frames / tb, 4), "unit": "frames/s",
                                 "ms_per_step": round(tb * 1e3, 2), "note": "same workload, several videos per batch; not the headline"}
        if not args.no_cpu_baseline and world == 1:       # the CPU leg is reported at N=1 only
            result["cpu_baseline"] = cpu_baseline(frames, args.ddim_steps)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        try:
            os.remove(_handoff_path())
        except OSError:
            pass
        emit(result)


if __name__ == "__main__":
    main()
