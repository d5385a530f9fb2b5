"""Full-size golden fixtures FROM THE REAL REFERENCE for BASELINE.json configs[1]..[4] (run in the build container).

    python tests/golden/make_golden_full.py [c1] [c2] [c3] [c4]      # default: all (~45 min on 8 cores)
    python tests/golden/make_golden_full.py w16 [c1] [c2] [c3] [c4]  # "deployed-weights" goldens  -> *_w16.npz
    python tests/golden/make_golden_full.py w16 c3x12                # 12-frame ZeroScope-XL forward -> zeroscope_xl_12f_w16.npz
    python tests/golden/make_golden_full.py w16 zs7                  # ZeroScope's native 576x320 (latent 40x72), 7 frames: one forward
                                                                     # -> zeroscope_40x72_7f_w16.npz
    python tests/golden/make_golden_full.py w16 c1s50                # round 4: 50-step "DDIM" / "UniPC" latents at the full size
    python tests/golden/make_golden_full.py w16 c1s c3s c2s          # round 4: OUTPUT-level goldens (sampled latents) for the other
                                                                     # two samplers at configs[1] and for configs[3] / configs[2]
    python tests/golden/make_golden_full.py w16 c2s50                # round 5, second half: configs[2] at its own 50 steps (~4.5 h)
    python tests/golden/make_golden_full.py w16 c0 c2s20             # round 5: configs[0] (8 f, 5 steps) on the deployed weights;
                                                                     # a 20-step configs[2] output (125 frames)

"w16" (round 3): the SAME reference classes, the SAME fp32 CPU arithmetic, but every parameter and the
text conditioning are first rounded to fp16 and back (`w.half().float()`).  The reference pipeline always deploys `.half()`
weights (t2v_pipeline.py:103-104), so these are the "identical inputs" north_star words: the product receives exactly these
fp16 values, and what the golden then measures is the product's ARITHMETIC, not the fp32 -> fp16 rounding of the inputs
that both the product and the reference's own GPU path perform before any kernel runs.

Same recipe as make_golden.py (reference classes imported read-only through oracle/ref_bootstrap.py, seeded
synthetic weights/inputs of oracle/synth.py, fp32 CPU arithmetic); only OUTPUTS are stored.  The large outputs
are stored as the sub-sets named below (whole frames / strided pixel grids) so the fixtures stay small; the GPU
tests compare exactly those sub-sets (tests/test_gpu_fullsize.py).

  modelscope_24f.npz   configs[1]  ModelScope 1.41 B, 24 frames @256x256: one forward (t=801), DDIM_Gaussian CFG 9
                                   x0 after 10 and after 50 steps, tensor2vid uint8 frames 0 / 23 of the 50-step video
  modelscope_125f.npz  configs[2]  125 frames @256x256: one forward, frames FRAMES_125 (the slice edges of the
                                   4-way T split 32+32+32+29 and both clip ends)
  zeroscope_xl.npz     configs[3]  ZeroScope-XL geometry @1024x576 (latent 72x128, spatial attention over 9216 tokens): one
                                   forward of N_FRAMES_XL = 4 frames, frames FRAMES_XL — the reference's CPU attention
                                   (F.scaled_dot_product_attention, t2v_model.py:566-569) needs 0.8 GB per (frame, head) at 9216
                                   tokens, so 24 frames (120 heads-batches) exceed this container's 62 GB; the 24-frame
                                   count itself is covered by configs[1]; one VAE frame decoded at 1024x576 (mid attention
                                   over 9216 tokens): stride-4 pixel grid + a crop
  lvdm_16f_ddim.npz    configs[4]  VideoCrafter 0.96 B, 16 frames @256x256: lvdm DDIM (CFG 7.5, eta 0) x0 after 10 and
                                   50 steps, VAE decode of frame 0 of the 50-step latent (stride-2 pixel grid)
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FRAMES_125 = [0, 31, 32, 63, 64, 95, 96, 124]
FRAMES_XL = [0, 1, 3]
N_FRAMES_XL = 4
XL_GRID = (slice(1, None, 4), slice(2, None, 4))            # [3, 144, 256] of the 576 x 1024 image
XL_CROP = (slice(128, 256), slice(384, 512))
N_FRAMES_XL12 = 12
FRAMES_XL12 = [0, 5, 11]
N_FRAMES_ZS7 = 7
W16 = False                 # set by "w16" on the command line
SUFFIX = ""


def _deploy(module):
    """fp16-representable parameters held in fp32 (the deployed values, fp32 arithmetic)."""
    if W16:
        with torch.no_grad():
            for p in module.parameters():
                p.copy_(p.half().float())
    return module


def _inputs(frames, h, w):
    noise, cond, uncond = synth.synth_inputs(frames, h, w)
    if W16:
        cond, uncond = cond.half().float(), uncond.half().float()
    return noise, cond, uncond


def _unet():
    t0 = time.time()
    unet, betas = rb.build_reference_unet(configs.MODELSCOPE_UNET)
    synth.load_synth(unet, seed=0)
    _deploy(unet)
    print(f"reference UNetSD + synthetic weights {time.time() - t0:.1f}s", flush=True)
    return unet, betas


def _sample(ref, unet, betas, frames, steps, cond, uncond, h=256, w=256):
    s = ref.samplers.Txt2VideoSampler(unet, torch.device("cpu"), betas=betas, sampler_name="DDIM_Gaussian")
    lat, nz, shape = s.get_noise(1, 4, frames, h, w, seed=1234)
    with torch.no_grad():
        return s.sample_loop(steps=steps, strength=None, conditioning=cond, unconditional_conditioning=uncond, batch_size=1,
                             latents=lat, shape=shape, noise=nz, guidance_scale=9.0, eta=0.0, sampler_name="DDIM_Gaussian")


def tensor2vid_ref(video):
    """The reference's own tensor2vid (t2v_pipeline.py:447-460) cannot be imported (module top imports open_clip /
    cv2); its arithmetic is four lines and is restated in oracle/torch_port.tensor2vid, pinned in test_oracle_pin."""
    from oracle import torch_port as tp
    return [np.asarray(f) for f in tp.tensor2vid_uint8(video)]


def c1():
    ref = rb.bootstrap()
    unet, betas = _unet()
    noise, cond, uncond = _inputs(24, 256, 256)
    with torch.no_grad():
        t0 = time.time()
        eps = unet(noise, torch.tensor([801]), cond)
        t_fwd = time.time() - t0
    print(f"c1 forward {t_fwd:.1f}s std {eps.std():.4f}", flush=True)
    t0 = time.time()
    x10 = _sample(ref, unet, betas, 24, 10, cond, uncond)
    print(f"c1 10 steps {time.time() - t0:.0f}s std {x10.std():.4f}", flush=True)
    t0 = time.time()
    x50 = _sample(ref, unet, betas, 24, 50, cond, uncond)
    t50 = time.time() - t0
    print(f"c1 50 steps {t50:.0f}s std {x50.std():.4f}", flush=True)
    del unet
    vae = rb.build_reference_vae(configs.VAE_DDCONFIG)
    synth.load_synth(vae, seed=3)
    _deploy(vae)
    with torch.no_grad():
        imgs = torch.cat([vae.decode(x50[:, :, f] / configs.SCALE_FACTOR) for f in (0, 23)], dim=0)   # [2,3,256,256]
    vid = imgs.permute(1, 0, 2, 3).unsqueeze(0)                # [1,3,F,H,W] as t2v_pipeline.py:355-357
    frames_u8 = np.stack(tensor2vid_ref(vid))                  # [2,256,256,3]
    np.savez_compressed(os.path.join(OUT, f"modelscope_24f{SUFFIX}.npz"), unet_eps=eps.numpy(), sampler_x0_10=x10.numpy(),
                        sampler_x0_50=x50.numpy(), frames_u8=frames_u8, vae_img=imgs.numpy().astype(np.float32)[:, :, ::2, ::2],
                        timing=np.array([t_fwd, t50, torch.get_num_threads()], dtype=np.float64))
    print("c1 done", flush=True)


def c2():
    unet, _ = _unet()
    noise, cond, _ = _inputs(125, 256, 256)
    with torch.no_grad():
        t0 = time.time()
        eps = unet(noise, torch.tensor([801]), cond)
        t_fwd = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"modelscope_125f{SUFFIX}.npz"), unet_eps_frames=eps[:, :, FRAMES_125].numpy(),
                        frames=np.array(FRAMES_125), eps_std=np.float64(eps.std()),
                        timing=np.array([t_fwd, torch.get_num_threads()], dtype=np.float64))
    print(f"c2 done forward {t_fwd:.1f}s std {eps.std():.4f}", flush=True)


def c3():
    unet, _ = _unet()
    noise, cond, _ = _inputs(N_FRAMES_XL, 576, 1024)
    with torch.no_grad():
        t0 = time.time()
        eps = unet(noise, torch.tensor([801]), cond)
        t_fwd = time.time() - t0
    print(f"c3 forward {t_fwd:.1f}s std {eps.std():.4f}", flush=True)
    del unet
    vae = rb.build_reference_vae(configs.VAE_DDCONFIG)
    synth.load_synth(vae, seed=3)
    _deploy(vae)
    z = noise[:, :, 0] / configs.SCALE_FACTOR
    with torch.no_grad():
        t0 = time.time()
        img = vae.decode(z)[0]                                 # [3,576,1024]
        t_vae = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"zeroscope_xl{SUFFIX}.npz"), unet_eps_frames=eps[:, :, FRAMES_XL].numpy(),
                        frames=np.array(FRAMES_XL), vae_grid=img[:, XL_GRID[0], XL_GRID[1]].numpy(),
                        vae_crop=img[:, XL_CROP[0], XL_CROP[1]].numpy(), vae_std=np.float64(img.std()),
                        timing=np.array([t_fwd, t_vae, torch.get_num_threads()], dtype=np.float64))
    print(f"c3 done vae {t_vae:.1f}s std {img.std():.4f}", flush=True)


def c4():
    import importlib
    import types
    rb.bootstrap()
    om = importlib.import_module("videocrafter.lvdm.models.modules.openaimodel3d")
    vu = importlib.import_module("videocrafter.lvdm.models.modules.util")
    dd = importlib.import_module("videocrafter.lvdm.samplers.ddim")
    dd.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    net = om.UNetModel(**configs.LVDM_UNET).eval()
    synth.load_synth(net, seed=0)
    _deploy(net)
    g = torch.Generator().manual_seed(1234)
    x_T = torch.randn(1, 4, 16, 32, 32, generator=g)
    ctx = torch.randn(2, 77, 768, generator=g)
    if W16:
        ctx = ctx.half().float()
    betas = vu.make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    model = types.SimpleNamespace(num_timesteps=1000, betas=f32(betas), alphas_cumprod=f32(ac),
                                  alphas_cumprod_prev=f32(np.append(1.0, ac[:-1])), device=torch.device("cpu"),
                                  apply_model=lambda xx, tt, c, **kw: net(xx, tt, context=c))
    out = {}
    for steps in (10, 50):
        smp = dd.DDIMSampler(model)
        smp.noise_gen.manual_seed(123)
        t0 = time.time()
        with torch.no_grad():
            x0, _ = smp.sample(S=steps, conditioning=ctx[0:1], batch_size=1, shape=list(x_T.shape[1:]), verbose=False,
                               unconditional_guidance_scale=7.5, unconditional_conditioning=ctx[1:2], eta=0.0, x_T=x_T)
        out[f"ddim_x0_{steps}"] = x0.numpy()
        print(f"c4 {steps} steps {time.time() - t0:.0f}s std {x0.std():.4f}", flush=True)
    del net
    vae = rb.build_reference_vae(configs.VAE_DDCONFIG)
    synth.load_synth(vae, seed=3)
    _deploy(vae)
    with torch.no_grad():       # decode_first_stage_2DAE: z = 1/scale_factor * z, per frame (ddpm3d.py:776-793)
        img = vae.decode(torch.from_numpy(out["ddim_x0_50"])[:, :, 0] / configs.SCALE_FACTOR)
    np.savez_compressed(os.path.join(OUT, f"lvdm_16f_ddim{SUFFIX}.npz"), vae_img_frame0=img.numpy()[:, :, ::2, ::2], **out)
    print("c4 done", flush=True)


def c3x12():
    """configs[3] at 12 frames (VERDICT r02 missing #3): batch 12 x 5 heads of the 9216-token attention = 60 score matrices
    of 0.34 GB (+ softmax copies) fit this container; 24 frames do not."""
    unet, _ = _unet()
    noise, cond, _ = _inputs(N_FRAMES_XL12, 576, 1024)
    with torch.no_grad():
        t0 = time.time()
        eps = unet(noise, torch.tensor([801]), cond)
        t_fwd = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"zeroscope_xl_12f{SUFFIX}.npz"), unet_eps_frames=eps[:, :, FRAMES_XL12].numpy(),
                        frames=np.array(FRAMES_XL12), eps_std=np.float64(eps.std()),
                        timing=np.array([t_fwd, torch.get_num_threads()], dtype=np.float64))
    print(f"c3x12 done forward {t_fwd:.1f}s std {eps.std():.4f}", flush=True)


def zs7():
    """ZeroScope's native 576 x 320 (a latent of 40 x 72) at 7 frames: ragged at every level of the UNet (20160, 5040, 1260 and 315 rows
    per sample), a geometry outside the other goldens' tile, split-K, GroupNorm and attention classes.  All 7 frames are stored."""
    unet, _ = _unet()
    noise, cond, _ = _inputs(N_FRAMES_ZS7, 320, 576)
    with torch.no_grad():
        t0 = time.time()
        eps = unet(noise, torch.tensor([801]), cond)
        t_fwd = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"zeroscope_40x72_7f{SUFFIX}.npz"), unet_eps_frames=eps.numpy(),
                        frames=np.arange(N_FRAMES_ZS7), eps_std=np.float64(eps.std()),
                        timing=np.array([t_fwd, torch.get_num_threads()], dtype=np.float64))
    print(f"zs7 done forward {t_fwd:.1f}s std {eps.std():.4f}", flush=True)


def _sample_named(ref, unet, betas, frames, steps, cond, uncond, name, h=256, w=256):
    """`name` in {"DDIM", "UniPC"}: the reference's own Txt2VideoSampler with that sampler (samplers_common.py:165-207 ->
    ddim/sampler.py:110-220 | uni_pc/uni_pc.py:683-743).  Both classes pin their buffers to torch.device("cuda")
    (ddim/sampler.py:11,18-22; uni_pc/sampler.py:13-17); as in make_golden.py the only change is to point that device at the CPU."""
    import samplers.uni_pc.sampler as ups
    ups.UniPCSampler.register_buffer = lambda self, name_, attr: setattr(self, name_, attr)
    cpu = torch.device("cpu")
    s = ref.samplers.Txt2VideoSampler(unet, cpu, betas=betas, sampler_name=name)
    s.sampler.device = cpu
    lat, nz, shape = s.get_noise(1, 4, frames, h, w, seed=1234)
    with torch.no_grad():
        return s.sample_loop(steps=steps, strength=None, conditioning=cond, unconditional_conditioning=uncond, batch_size=1,
                             latents=lat, shape=shape, noise=nz, guidance_scale=9.0, eta=0.0, sampler_name=name)


def c1s():
    """configs[1] geometry through the OTHER two samplers (VERDICT r03 missing #4): 10-step "DDIM" (LDM DDIMSampler) and 10-step
    "UniPC" latents of the full 1.41 B model, 24 frames @256x256, CFG 9."""
    ref = rb.bootstrap()
    unet, betas = _unet()
    _, cond, uncond = _inputs(24, 256, 256)
    out = {}
    for name in ("DDIM", "UniPC"):
        t0 = time.time()
        x0 = _sample_named(ref, unet, betas, 24, 10, cond, uncond, name)
        out[f"{name.lower()}_x0_10"] = x0.numpy()
        print(f"c1s {name} 10 steps {time.time() - t0:.0f}s std {x0.std():.4f}", flush=True)
    np.savez_compressed(os.path.join(OUT, f"modelscope_24f_samplers{SUFFIX}.npz"), **out)
    print("c1s done", flush=True)


def c1s50():
    """The other two samplers at the DEPLOYED step count: 50-step "DDIM" and 50-step "UniPC" latents of the full model (the 10-step
    goldens above sit in the few-step regime where the trajectory has not contracted yet)."""
    ref = rb.bootstrap()
    unet, betas = _unet()
    _, cond, uncond = _inputs(24, 256, 256)
    out = {}
    for name in ("DDIM", "UniPC"):
        t0 = time.time()
        x0 = _sample_named(ref, unet, betas, 24, 50, cond, uncond, name)
        out[f"{name.lower()}_x0_50"] = x0.numpy()
        out[f"{name.lower()}_timing"] = np.array([time.time() - t0, torch.get_num_threads()], dtype=np.float64)
        print(f"c1s50 {name} 50 steps {time.time() - t0:.0f}s std {x0.std():.4f}", flush=True)
        np.savez_compressed(os.path.join(OUT, f"modelscope_24f_samplers50{SUFFIX}.npz"), **out)
    print("c1s50 done", flush=True)


def c3s():
    """configs[3] OUTPUT-level golden (VERDICT r03 missing #2): 5-step DDIM_Gaussian CFG 9 latent of a 4-frame clip at the
    ZeroScope-XL geometry (latent 72x128, 9216-token spatial attention)."""
    ref = rb.bootstrap()
    unet, betas = _unet()
    _, cond, uncond = _inputs(N_FRAMES_XL, 576, 1024)
    t0 = time.time()
    x0 = _sample(ref, unet, betas, N_FRAMES_XL, 5, cond, uncond, h=576, w=1024)
    t5 = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"zeroscope_xl_s5{SUFFIX}.npz"), sampler_x0_5=x0.numpy(),
                        timing=np.array([t5, torch.get_num_threads()], dtype=np.float64))
    print(f"c3s done 5 steps {t5:.0f}s std {x0.std():.4f}", flush=True)


def c2s():
    """configs[2] OUTPUT-level golden (VERDICT r03 missing #2): 10-step DDIM_Gaussian CFG 9 latent of the 125-frame clip, frames
    FRAMES_125 (the slice edges of the 4-way T split and both clip ends)."""
    ref = rb.bootstrap()
    unet, betas = _unet()
    _, cond, uncond = _inputs(125, 256, 256)
    t0 = time.time()
    x0 = _sample(ref, unet, betas, 125, 10, cond, uncond)
    t10 = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"modelscope_125f_s10{SUFFIX}.npz"), sampler_x0_10_frames=x0[:, :, FRAMES_125].numpy(),
                        frames=np.array(FRAMES_125), x0_std=np.float64(x0.std()),
                        timing=np.array([t10, torch.get_num_threads()], dtype=np.float64))
    print(f"c2s done 10 steps {t10:.0f}s std {x0.std():.4f}", flush=True)


def c0():
    """configs[0] on the DEPLOYED weights: 8 frames @256x256, one forward, 5-step DDIM_Gaussian CFG 9, one VAE
    frame — the recipe of make_golden.modelscope() with fp16-representable parameters / conditioning (modelscope_8f_w16.npz)."""
    ref = rb.bootstrap()
    unet, betas = _unet()
    noise, cond, uncond = _inputs(8, 256, 256)
    with torch.no_grad():
        t0 = time.time()
        eps = unet(noise, torch.tensor([801]), cond)
        t_fwd = time.time() - t0
    t0 = time.time()
    x0 = _sample(ref, unet, betas, 8, 5, cond, uncond)
    t_loop = time.time() - t0
    del unet
    vae = rb.build_reference_vae(configs.VAE_DDCONFIG)
    synth.load_synth(vae, seed=3)
    _deploy(vae)
    with torch.no_grad():
        img = vae.decode(x0[:, :, 0] / configs.SCALE_FACTOR)
    np.savez_compressed(os.path.join(OUT, f"modelscope_8f{SUFFIX}.npz"), unet_eps=eps.numpy(), sampler_x0=x0.numpy(),
                        vae_img_frame0=img.numpy().astype(np.float32),
                        timing=np.array([t_fwd, t_loop, torch.get_num_threads()], dtype=np.float64))
    print(f"c0 done fwd {t_fwd:.1f}s loop {t_loop:.0f}s std {eps.std():.4f} {x0.std():.4f}", flush=True)


def c2s20():
    """configs[2] OUTPUT-level golden at 20 steps: DDIM_Gaussian CFG 9 latent of the 125-frame clip, frames
    FRAMES_125 — twice the step count of c2s, past the few-step regime (the 50 steps of the config are ~4.5 h of reference CPU time)."""
    ref = rb.bootstrap()
    unet, betas = _unet()
    _, cond, uncond = _inputs(125, 256, 256)
    t0 = time.time()
    x0 = _sample(ref, unet, betas, 125, 20, cond, uncond)
    t20 = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"modelscope_125f_s20{SUFFIX}.npz"), sampler_x0_20_frames=x0[:, :, FRAMES_125].numpy(),
                        frames=np.array(FRAMES_125), x0_std=np.float64(x0.std()),
                        timing=np.array([t20, torch.get_num_threads()], dtype=np.float64))
    print(f"c2s20 done 20 steps {t20:.0f}s std {x0.std():.4f}", flush=True)


def _c3s_steps(steps):
    """configs[3] OUTPUT-level golden past the few-step regime: `steps`-step DDIM_Gaussian CFG 9 latent of the 4-frame clip at the
    ZeroScope-XL geometry (latent 72x128) — the same clip as c3s (24 frames at this size do not fit the build container's memory)."""
    ref = rb.bootstrap()
    unet, betas = _unet()
    _, cond, uncond = _inputs(N_FRAMES_XL, 576, 1024)
    t0 = time.time()
    x0 = _sample(ref, unet, betas, N_FRAMES_XL, steps, cond, uncond, h=576, w=1024)
    dt = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"zeroscope_xl_s{steps}{SUFFIX}.npz"), **{f"sampler_x0_{steps}": x0.numpy()},
                        timing=np.array([dt, torch.get_num_threads()], dtype=np.float64))
    print(f"c3s{steps} done {steps} steps {dt:.0f}s std {x0.std():.4f}", flush=True)


def c3s50():
    _c3s_steps(50)


def c3s20():
    _c3s_steps(20)


def c2s50():
    """configs[2] OUTPUT-level golden at the config's OWN step count (VERDICT r04 missing #3): 50-step DDIM_Gaussian CFG 9 latent of the
    125-frame clip, frames FRAMES_125.  100 reference forwards of 125 frames: ~4.5 h on the build container's 8 cores."""
    ref = rb.bootstrap()
    unet, betas = _unet()
    _, cond, uncond = _inputs(125, 256, 256)
    t0 = time.time()
    x0 = _sample(ref, unet, betas, 125, 50, cond, uncond)
    t50 = time.time() - t0
    np.savez_compressed(os.path.join(OUT, f"modelscope_125f_s50{SUFFIX}.npz"), sampler_x0_50_frames=x0[:, :, FRAMES_125].numpy(),
                        frames=np.array(FRAMES_125), x0_std=np.float64(x0.std()),
                        timing=np.array([t50, torch.get_num_threads()], dtype=np.float64))
    print(f"c2s50 done 50 steps {t50:.0f}s std {x0.std():.4f}", flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    if "w16" in sys.argv[1:]:
        W16, SUFFIX = True, "_w16"
    which = [a for a in sys.argv[1:] if a in ("c1", "c2", "c3", "c4", "c3x12", "c1s", "c3s", "c2s", "c1s50", "c0", "c2s20", "c2s50", "c3s50", "c3s20", "zs7")] or ["c2", "c3", "c4", "c1"]
    for name in which:
        globals()[name]()
