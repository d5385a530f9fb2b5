"""TextToVideoSynthesis / process_modelscope — the reference's outer entry points (boundaries
B1/B2) over the MI355X hot path.

`TextToVideoSynthesis.infer` keeps the signature and return triple of
reference scripts/modelscope/t2v_pipeline.py:197-216,385:
    (frames_bgr_list, last_tensor, infotext)
and the same stages: conditioning -> seeded CPU noise -> sample_loop -> VAE decode of
x0/0.18215 -> tensor2vid (x*0.5+0.5, clamp, *255 truncated to uint8, RGB->BGR).

What is NOT rebuilt here (out of scope per SURVEY §2.1): the OpenCLIP text encoder
(clip_hardcode.py) — pass a `clip_encoder` callable/object, or call `infer_conditioned` with
pre-computed conditioning tensors; file / ffmpeg / Gradio plumbing of process_modelscope.py.

MI355X differences inside the stages: cond+uncond UNet evaluations are one batched forward,
and all frames are decoded by ONE batched VAE program (the reference decodes frame by frame and
copies each to the host, t2v_pipeline.py:329-355).
"""
from __future__ import annotations

import json
import os
import random
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from . import packing as pk
from .compiled import ProgramHost, _Compiled
from .program import Program, Ref
from .samplers import Txt2VideoSampler, available_samplers
from .unet import UNetSD
from .vae import AutoencoderKL

SCALE_FACTOR = 0.18215          # t2v_pipeline.py:297

VAE_DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                    ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)


def beta_schedule(schedule, num_timesteps=1000, init_beta=None, last_beta=None):
    """t2v_model.py:1240-1249."""
    if schedule == "linear_sd":
        return torch.linspace(init_beta ** 0.5, last_beta ** 0.5, num_timesteps, dtype=torch.float64) ** 2
    raise ValueError(f"Unsupported schedule: {schedule}")


def tensor2vid_device(video: torch.Tensor, bgr: bool = False) -> torch.Tensor:
    """[i,3,F,H,W] float video -> uint8 [F,H,(i W),3] on the same device with ONE T2V_OP_TO_UINT8 launch: x*0.5+0.5, clamp,
    *255 TRUNCATED like `(image.numpy()*255).astype('uint8')` (t2v_pipeline.py:447-460) — in fp32 for an fp32 video, in
    fp16 for an fp16 one (what `mul_` / `add_` / numpy do on the reference's half-precision VAE output).  Bit-exact
    with the reference for identical float input (tests/test_gpu_boundary.py)."""
    import ctypes
    from . import _lib as L
    if not video.is_cuda:
        raise L.T2VError("tensor2vid_device needs a device tensor on an AMD GPU (no CPU fallback)")
    if video.dtype not in (torch.float16, torch.float32):
        video = video.float()
    video = video.contiguous()
    NI, C, Fr, H, W = video.shape
    out = torch.empty((Fr, H, NI * W, C), dtype=torch.uint8, device=video.device)
    op = L.T2VOp()
    op.kind = L.OP_TO_UINT8
    half = video.dtype == torch.float16
    vals = [NI, C, Fr, H, W, L.F16 if half else L.F32, int(half), int(bgr)]
    si, sc, sf, sy, sx = C * Fr * H * W, Fr * H * W, H * W, W, 1
    vals += [si & 0xFFFFFFFF, si >> 32, sc, sf & 0xFFFFFFFF, sf >> 32, sy, sx]
    if sc >= 2 ** 31:
        raise L.T2VError("video too large for one uint8 conversion launch")
    for k, v in enumerate(vals):
        op.i[k] = v - (1 << 32) if v >= (1 << 31) else v       # low words as raw bits
    op.p[0], op.p[1] = video.data_ptr(), out.data_ptr()
    L.check(L.load().t2v_run_ops(ctypes.byref(op), 1, None, 0, ctypes.c_void_p(torch.cuda.current_stream(video.device).cuda_stream)))
    return out


def tensor2vid(video: torch.Tensor) -> List[np.ndarray]:
    frames = tensor2vid_device(video).cpu().numpy()
    return [frames[i] for i in range(frames.shape[0])]


def create_infotext(vars_: dict) -> str:
    vars_ = dict(vars_)
    prompt = vars_.pop("prompt", "")
    n_prompt = vars_.pop("n_prompt", "")
    params = ", ".join(f"{k}: {v}" for k, v in vars_.items() if v is not None)
    neg = "\nNegative prompt: " + n_prompt if len(n_prompt) > 0 else ""
    return f"{prompt}{neg}\n{params}".strip()


class TextToVideoSynthesis(object):
    def __init__(self, model_dir: Optional[str] = None, *, sd_model: Optional[UNetSD] = None,
                 autoencoder: Optional[AutoencoderKL] = None, clip_encoder=None, betas=None,
                 device=None, tokenizer=None, enable_emphasis=None, comma_padding_backtrack=None):
        """Either `model_dir` (configuration.json + checkpoints, as t2v_pipeline.py:45-146) or
        ready-made `sd_model` / `autoencoder` modules.  With a `model_dir` and no `clip_encoder`, the OpenCLIP text
        tower is built from `ckpt_clip` (t2v_pipeline.py:137-141) and runs on the GPU (text_encoder.py); `tokenizer` =
        open_clip's `_tokenizer` (BPE vocabulary; not part of this package).  `enable_emphasis` / `comma_padding_backtrack`: the two
        webui options of the reference's prompt syntax (`opts.enable_emphasis`, `opts.comma_padding_backtrack`; clip_hardcode.py:153,203),
        handed to the text encoder (None = leave the encoder's own setting: off / 0 for the one built here)."""
        self.model_dir = model_dir
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.keep_in_vram = "All"
        self.clip_encoder = clip_encoder
        if model_dir is not None and sd_model is None:
            with open(os.path.join(model_dir, "configuration.json"), "r") as f:
                self.config = SimpleNamespace(**json.load(f))
            cfg = self.config.model["model_cfg"]
            cfg["temporal_attention"] = True if cfg["temporal_attention"] == "True" else False
            sd_model = UNetSD(in_dim=cfg["unet_in_dim"], dim=cfg["unet_dim"], y_dim=cfg["unet_y_dim"],
                              context_dim=cfg["unet_context_dim"], out_dim=cfg["unet_out_dim"],
                              dim_mult=cfg["unet_dim_mult"], num_heads=cfg["unet_num_heads"],
                              head_dim=cfg["unet_head_dim"], num_res_blocks=cfg["unet_res_blocks"],
                              attn_scales=cfg["unet_attn_scales"], dropout=cfg["unet_dropout"],
                              parameterization=cfg["mean_type"], temporal_attention=cfg["temporal_attention"],
                              init_weights=False)
            args = self.config.model["model_args"]
            sd_model.load_state_dict(torch.load(os.path.join(model_dir, args["ckpt_unet"]), map_location="cpu"), strict=True)
            sd_model.eval().half()
            betas = beta_schedule("linear_sd", cfg["num_timesteps"], init_beta=0.00085, last_beta=0.0120)
            autoencoder = AutoencoderKL(VAE_DDCONFIG, 4, os.path.join(model_dir, args["ckpt_autoencoder"]), init_weights=False)
            clip_path = os.path.join(model_dir, args.get("ckpt_clip", ""))
            if clip_encoder is None and os.path.isfile(clip_path):
                from .text_encoder import FrozenOpenCLIPEmbedder
                self.clip_encoder = FrozenOpenCLIPEmbedder(version=clip_path, device=self.device, layer="penultimate",
                                                           tokenizer=tokenizer)
        self.set_prompt_options(enable_emphasis, comma_padding_backtrack)
        if betas is None:
            betas = beta_schedule("linear_sd", 1000, init_beta=0.00085, last_beta=0.0120)
        self.sd_model = sd_model
        self.autoencoder = autoencoder.eval() if autoencoder is not None else None
        self.betas = betas
        self.sd_model.register_schedule(given_betas=betas.numpy())
        self.diffusion = Txt2VideoSampler(self.sd_model, self.device, betas=betas)
        self.noise_gen = torch.Generator(device="cpu")
        self.last_tensor = None

    # ---- conditioning ----------------------------------------------------------------------------
    def set_prompt_options(self, enable_emphasis=None, comma_padding_backtrack=None):
        """Hand the prompt-syntax options to a text encoder that takes them (text_encoder.FrozenOpenCLIPEmbedder); None = unchanged."""
        enc = self.clip_encoder
        if enable_emphasis is not None and hasattr(enc, "enable_emphasis"):
            enc.enable_emphasis = bool(enable_emphasis)
        if comma_padding_backtrack is not None and hasattr(enc, "comma_padding_backtrack"):
            enc.comma_padding_backtrack = int(comma_padding_backtrack)

    def preprocess(self, prompt, n_prompt, steps):
        if self.clip_encoder is None:
            raise RuntimeError("no text encoder attached: pass clip_encoder=... (the reference's "
                               "FrozenOpenCLIPEmbedder) or call infer_conditioned(c, uc, ...)")
        enc = self.clip_encoder
        encode = (lambda text: enc([text])) if callable(enc) else (lambda text: enc.encode([text]))
        if isinstance(prompt, (list, tuple)) or isinstance(n_prompt, (list, tuple)):
            # a batch of different prompts: lists of contexts, one per video.  Every prompt goes through an encoder call of ITS OWN — the
            # reference's embedder pads all prompts of one call to the longest one's chunk count (clip_hardcode.py, chunk_count = max(...)),
            # which would change the shorter prompts' contexts.  A text that occurs several times is encoded once.
            prompts, n_prompts = _prompt_lists(prompt, n_prompt)
            done = {}
            one = lambda text: done[text] if text in done else done.setdefault(text, encode(text))
            return [one(t) for t in prompts], [one(t) for t in n_prompts]
        return encode(prompt), encode(n_prompt)

    # ---- the hot path ---------------------------------------------------------------------------
    @torch.no_grad()
    def infer_conditioned(self, c, uc, steps, frames, seed, scale, width=256, height=256, eta=0.0,
                          device=None, latents=None, strength=None, mask=None, is_vid2vid=False,
                          sampler=available_samplers[0].name, decode=True, to_host=True, _keep_sampler=False,
                          videos: int = 1, *, clamp=None, percentile=None, unipc=None, seeds=None, inversion=None, inpaint=None,
                          context_windows=None, freeu=None):
        """Stages 2-4 of `infer` for given conditioning tensors c, uc [1, 77k, 1024].
        A batch of DIFFERENT prompts: c / uc as lists of `videos` tensors [1, 77k_v, 1024] (a single tensor beside a list = that prompt for
        every video; lists of one entry = the tensor), contexts of any lengths — still one 2*videos forward per step, the text
        cross-attentions with one key count per sample.  `seeds`: a list of `videos` ints, video v starts from the noise of seeds[v]
        (default seed + v).  txt2vid and vid2vid on one device, as `videos` > 1.
        `unipc` (UniPC only; another sampler raises ValueError): a dict of the solver options of `samplers.UniPCSampler` (variant,
        skip_type, order, lower_order_final, initial_corrector, denoise_to_zero, thresholding); forwarded only when set.
        `clamp` / `percentile` (DDIM_Gaussian only; another sampler raises ValueError): the restriction of the predicted x0 of
        `GaussianDiffusion.sample` — percentile=0.995 is dynamic thresholding per video, clamp=<anything> clamps x0 to [-1, 1] (the
        reference's `clamp=True` quirk, gaussian_sampler.py:178); forwarded only when set.
        `inversion` (sampler "DDIM" with is_vid2vid only; anything else raises ValueError): True (the reference's encode: scale 1, UNet labels
        t = i) or a dict with guidance_scale and / or model_timesteps ("index" | "schedule", see `DDIMSampler.encode`) — the input latents are inverted by `DDIMSampler.encode` (deterministic, structure-preserving)
        instead of noised by `stochastic_encode`; the drawn noise is not used.  Forwarded only when set (`Txt2VideoSampler.sample_loop`).
        `inpaint` (DDIM_Gaussian only; another sampler raises ValueError): "legacy" lets `mask` hold the frames to `latents` and release them
        along the weights — the keyframe blend of the reference's legacy loop (`GaussianDiffusion.sample`); forwarded only when set.
        `context_windows` (every sampler): a `samplers.ContextWindows`, or {"length": 16, "overlap": 4[, "weights": "pyramid" | "flat",
        "batch": n]} — a clip of more than `length` frames is denoised through overlapping windows of `length` frames whose eps are blended
        per frame, so the UNet only sees clips of the length it was trained on; forwarded only when set.
        `freeu` (every sampler): {"b1": 1.2, "b2": 1.4, "s1": 0.9, "s2": 0.2} (the FreeU authors' ModelScope values) — FreeU in the UNet for
        this call (`UNetSD.enable_freeu`: half of the backbone channels amplified, the skips' low frequencies damped, at the decoder
        concatenations of 4 dim and 2 dim channels); the model is restored afterwards.  The four values are part of the UNet's program
        key (`max_programs` bounds a sweep).  A partial dict or a non-finite value raises ValueError; the T-shard and CFG-pair multi-GPU
        layouts raise NotImplementedError.  Forwarded only when set.
        Returns (frames, last_tensor): frames = list of HxWx3 uint8 BGR arrays (to_host) or a
        uint8 device tensor [F,H,W,3] RGB (to_host=False), or None when decode=False.
        `videos` > 1 (every sampler; txt2vid and vid2vid, where the ONE input clip's latents are repeated): that many independent videos of the same prompt in ONE batch — every
        UNet step is a single 2*videos forward; the frames come back side by side ([F, H, videos*W, 3], the layout
        `tensor2vid` gives a batch, t2v_pipeline.py:447-460).  Video v starts from the noise of seed + v, i.e. the batch is
        the reference's `batch_count` loop (process_modelscope.py:152-221: one video at a time, seed + batch) in one pass."""
        dev = torch.device(device) if device is not None else self.device
        c, uc, videos, seeds = _batch_arguments(c, uc, videos, seed, seeds)
        several = isinstance(c, list) or isinstance(uc, list)
        if several:
            if mask is not None or (latents is not None and not is_vid2vid):
                raise NotImplementedError("a batch of different prompts: text-to-video and vid2vid only — the img2vid route draws every "
                                          "video's latents from numpy's global generator (process_modelscope.py:205), one call per video")
            if getattr(self.sd_model, "t_shard", None) is not None:
                raise NotImplementedError("a batch of different prompts is not supported in the T-shard multi-GPU layout (a clip whose frames "
                                          "are split over ranks runs one video per batch)")
        self.device = dev
        self.diffusion.device = dev
        self.sd_model.to(dev)
        if not _keep_sampler:
            self.diffusion.get_sampler(sampler, return_sampler=False)
        if several and getattr(self.diffusion.sampler, "cfg_parallel", None) is not None and self.diffusion.sampler.cfg_parallel.size == 2:
            raise NotImplementedError("a batch of different prompts is not supported in the CFG-pair multi-GPU layout (it runs one video per pair)")
        latents, noise, shape = self.diffusion.get_noise(1, 4, frames, height, width, seed=seeds[0], latents=latents)
        if videos > 1:
            if mask is not None or (latents is not None and not is_vid2vid):
                raise NotImplementedError("several videos per batch: text-to-video and vid2vid only — the img2vid route draws every "
                                          "video's latents from numpy's global generator (process_modelscope.py:205), one call per video")
            if latents is not None and latents.shape[0] != 1:
                raise ValueError(f"several videos per batch start from ONE input clip, got latents of batch {latents.shape[0]}")
            one = (1,) + tuple(shape[1:])
            draws = []
            for v in range(videos):                      # each video from its own seed, as the batch_count loop draws them
                self.diffusion.noise_gen.manual_seed(seeds[v])
                draws.append(torch.randn(one, generator=self.diffusion.noise_gen))
            noise = torch.cat(draws, dim=0).to(dev)
            shape = (videos,) + tuple(shape[1:])
        x0 = self.diffusion.sample_loop(
            steps=steps, strength=strength, eta=eta, conditioning=_to(c, dev), unconditional_conditioning=_to(uc, dev),
            batch_size=videos, guidance_scale=scale, latents=latents, shape=shape, noise=noise, is_vid2vid=is_vid2vid,
            sampler_name=sampler, mask=mask, **_restriction(clamp, percentile, unipc, inversion, inpaint, context_windows, freeu))
        self.last_tensor = x0
        if not decode:
            return None, x0
        if not to_host:
            return self.decode_frames(x0), x0
        arr = self.decode_frames(x0, bgr=True).cpu().numpy()          # BGR like postprocess_video (t2v_pipeline.py:430-433)
        L.async_status()               # the copy above synchronised: a fault raised by any kernel of this video surfaces HERE
        return [arr[i] for i in range(arr.shape[0])], x0

    max_programs = 4          # resize programs kept (one per geometry; each owns a small device arena)

    @staticmethod
    def _as_u8_frames(frames, device) -> torch.Tensor:
        """uint8 [F, H, W, 3] frames, numpy or tensor -> contiguous device tensor (a device tensor is taken as it is: no host copy)."""
        t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(frames)))
        if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[-1] != 3:
            raise ValueError(f"expected uint8 frames [F, H, W, 3], got {t.dtype} {tuple(t.shape)}")
        return t.to(device).contiguous()

    @torch.no_grad()
    def resize_frames(self, frames, height: int, width: int) -> torch.Tensor:
        """uint8 RGB frames [F, H, W, 3] (numpy array or device tensor) -> device uint8 [F, height, width, 3]: the resize of
        process_modelscope.py:116-120,174-178 (`Image.resize((width, height), Image.ANTIALIAS)` = Pillow's Lanczos filter) on the
        GPU, bit-exact with Pillow (T2V_OP_RESAMPLE: a horizontal and a vertical integer pass).  Programs are cached per geometry."""
        x = self._as_u8_frames(frames, self.device)
        n, h0, w0, _ = x.shape
        if (h0, w0) == (height, width):
            return x

        def build():
            prog, packer = Program(f"resize n{n} {h0}x{w0} -> {height}x{width}"), pk.WeightPacker()
            prog.begin()
            prog.resample("frames.resample", Ref("ext", L.EXT_X), Ref("ext", L.EXT_OUT), packer, n=n, src_hw=(h0, w0), dst_hw=(height, width))
            prog.finish()
            return _Compiled(prog, packer)

        host = self.__dict__.get("_resize_host")          # made on first use: pipelines are also put together without __init__
        if host is None:
            host = self._resize_host = ProgramHost(self.max_programs)
            self._resize_programs = host._programs          # geometry -> _Compiled (the coefficient tables are the host's pack)
        host.max_programs = self.max_programs          # (read on every call: the bound may be changed on the pipeline at any time)
        comp = host._program((n, h0, w0, height, width), build)
        host._prepare(comp, x.device)
        out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=x.device)
        host._launch(comp, x.device, {L.EXT_X: x.data_ptr(), L.EXT_OUT: out.data_ptr()})
        return out

    @torch.no_grad()
    def compute_latents(self, vd_out, cpu_vae="GPU (half precision)", device=torch.device("cuda"), height=None, width=None):
        """vid2vid input side (t2v_pipeline.py:148-194): frames [b, 3, F, H, W] in [-1, 1] -> posterior mean x 0.18215,
        [b, 4, F, H/8, W/8] fp32 on the host.  All frames go through ONE batched encoder program (the reference
        encodes them one at a time).
        `vd_out` may also be uint8 RGB frames [F, H0, W0, 3] of ANY size (numpy array or device tensor; one clip): they are resized
        to (height, width) — default: their own size — with Pillow's Lanczos filter, mapped to [-1, 1] and encoded by ONE program
        (AutoencoderKL.encode_uint8); the frames make no float round trip through the host."""
        _note_cpu_vae(cpu_vae)                         # "CPU ..." modes: full-precision VAE, still on the GPU (see _note_cpu_vae)
        self.device = torch.device(device)
        self.autoencoder.to(self.device)
        if (isinstance(vd_out, np.ndarray) and vd_out.dtype == np.uint8) or (isinstance(vd_out, torch.Tensor) and vd_out.dtype == torch.uint8):
            x = self._as_u8_frames(vd_out, self.device)
            F = x.shape[0]
            h, w = (x.shape[1] if height is None else int(height)), (x.shape[2] if width is None else int(width))
            mean = self.autoencoder.encode_uint8(x, h, w).mean.float() * SCALE_FACTOR
            return mean.view(1, F, mean.shape[1], mean.shape[2], mean.shape[3]).permute(0, 2, 1, 3, 4).contiguous().cpu()
        bs, c, F, h, w = vd_out.shape
        x = vd_out.to(self.device).permute(0, 2, 1, 3, 4).reshape(bs * F, c, h, w).contiguous()
        if "half precision" in str(cpu_vae):
            x = x.half()
        mean = self.autoencoder.encode(x).mean.float() * SCALE_FACTOR
        return mean.view(bs, F, mean.shape[1], mean.shape[2], mean.shape[3]).permute(0, 2, 1, 3, 4).contiguous().cpu()

    @torch.no_grad()
    def decode_frames(self, x0: torch.Tensor, bgr: bool = False) -> torch.Tensor:
        """latent [b,4,F,h,w] -> uint8 [F,H,(b W),3] RGB (or BGR) on device: ONE batched VAE program over all
        frames of x0/0.18215 (t2v_pipeline.py:329-355 decodes them one at a time) + tensor2vid."""
        self.autoencoder.to(x0.device)
        bs, _, F, h, w = x0.shape
        z = (x0 * (1.0 / SCALE_FACTOR)).permute(0, 2, 1, 3, 4).reshape(bs * F, 4, h, w)   # '(b f) c h w'
        return self.autoencoder.decode_to_uint8(z, videos=bs, bgr=bgr)     # uint8 conversion = last op of the decoder program

    def infer(self, prompt, n_prompt, steps, frames, seed, scale, width=256, height=256, eta=0.0,
              cpu_vae="GPU (half precision)", device=torch.device("cuda"), latents=None, skip_steps=0,
              strength=0, mask=None, is_vid2vid=False, sampler=available_samplers[0].name, *, clamp=None, percentile=None, unipc=None, inversion=None,
              inpaint=None, context_windows=None, freeu=None):
        vars_ = dict(prompt=prompt, n_prompt=n_prompt, steps=steps, frames=frames, seed=seed, scale=scale,
                     width=width, height=height, eta=eta, cpu_vae=cpu_vae, device=str(device),
                     skip_steps=skip_steps, strength=strength, is_vid2vid=is_vid2vid, sampler=sampler)
        seed = seed if seed != -1 else random.randint(0, 2 ** 32 - 1)
        vars_["seed"] = seed
        _note_cpu_vae(cpu_vae)
        if "half precision" in str(cpu_vae):
            self.autoencoder.half()                      # t2v_pipeline.py:337-339
        steps = steps - skip_steps
        c, uc = self.preprocess(prompt, n_prompt, steps)
        strength = None if (strength == 0.0 and not is_vid2vid) else strength
        frames_bgr, x0 = self.infer_conditioned(c, uc, steps, frames, seed, scale, width, height, eta, device,
                                                latents, strength, mask, is_vid2vid, sampler,
                                                **_restriction(clamp, percentile, unipc, inversion, inpaint, context_windows, freeu))
        return frames_bgr, self.last_tensor, create_infotext(vars_)


def _to(c, dev):
    return [v.to(dev) for v in c] if isinstance(c, list) else c.to(dev)


def _prompt_lists(prompt, n_prompt):
    """prompts / negative prompts of a batch -> two lists of one length; a single text (or a list of one) on either side is broadcast."""
    prompts = list(prompt) if isinstance(prompt, (list, tuple)) else [prompt]
    n_prompts = list(n_prompt) if isinstance(n_prompt, (list, tuple)) else [n_prompt]
    n = max(len(prompts), len(n_prompts))
    if not prompts or not n_prompts or any(len(v) not in (1, n) for v in (prompts, n_prompts)):
        raise ValueError(f"{len(prompts)} prompts against {len(n_prompts)} negative prompts: give one negative prompt, or one per prompt")
    return prompts * (n // len(prompts)), n_prompts * (n // len(n_prompts))


def _batch_arguments(c, uc, videos, seed, seeds):
    """The conditioning / videos / seeds arguments of `infer_conditioned` in one form: -> (c, uc, videos, seeds) with c / uc tensors, or lists
    of `videos` tensors for a batch of different prompts, and seeds a list of `videos` ints."""
    lists = [v for v in (c, uc) if isinstance(v, (list, tuple))]
    n = max((len(v) for v in lists), default=1)
    if any(len(v) not in (1, n) for v in lists) or not all(len(v) for v in lists):
        raise ValueError(f"conditioning lists of {[len(v) for v in lists]} entries: give one tensor, or one per video")
    if n > 1:
        if videos not in (1, n):
            raise ValueError(f"videos={videos} with conditioning lists of {n} entries")
        videos = n
        c, uc = (list(v) * (n // len(v)) if isinstance(v, (list, tuple)) else v for v in (c, uc))
    else:
        c, uc = (v[0] if isinstance(v, (list, tuple)) else v for v in (c, uc))          # lists of one entry: today's path
    if seeds is None:
        seeds = [seed + v for v in range(videos)]
    seeds = [int(v) for v in seeds]
    if len(seeds) != videos:
        raise ValueError(f"seeds: {len(seeds)} seeds for {videos} videos")
    return c, uc, videos, seeds


def _restriction(clamp, percentile, unipc=None, inversion=None, inpaint=None, context_windows=None, freeu=None) -> dict:
    """The x0-restriction keywords, the UniPC options, the DDIM inversion option, the keyframe-inpainting option, the context windows and
    the FreeU values that are set — nothing is forwarded when none is, so a call without them is what it was."""
    return {k: v for k, v in (("clamp", clamp), ("percentile", percentile), ("unipc", unipc), ("inversion", inversion), ("inpaint", inpaint),
                              ("context_windows", context_windows), ("freeu", freeu)) if v is not None}


_CPU_VAE_NOTED = False


def _note_cpu_vae(cpu_vae) -> None:
    """The reference's "CPU (Low VRAM)" VAE modes (t2v_pipeline.py:154-158,302-327) move the autoencoder to the host and run it in
    fp32 there to save VRAM.  This build has no host arithmetic path (and 288 GB of HBM make the saving moot): the option is
    ACCEPTED — a saved webui setting keeps working — and means what it means numerically in the reference, a VAE that is not
    halved, executed by the same HIP decoder / encoder programs on the GPU.  Said once on stderr, never silently."""
    global _CPU_VAE_NOTED
    if "CPU" in str(cpu_vae) and not _CPU_VAE_NOTED:
        _CPU_VAE_NOTED = True
        import sys
        print(f"[sd-webui-text2video_amd] cpu_vae={cpu_vae!r}: the VAE stays on the GPU (full-precision mode); "
              "this build has no host arithmetic path", file=sys.stderr)


pipe: Optional[TextToVideoSynthesis] = None     # module-global model cache, as process_modelscope.py:29


def frames_to_video_tensor(frames) -> torch.Tensor:
    """[F, H, W, 3] uint8 RGB frames -> [1, 3, F, H, W] float32 in [-1, 1]: the array arithmetic of process_modelscope.py:117-131
    (`/ 255`, `2 * x - 1`, one sample).  Reading the frames (ffmpeg) is host plumbing left to the caller; frames of another size go
    through `TextToVideoSynthesis.resize_frames` first."""
    arr = np.asarray(frames)
    if arr.ndim != 4 or arr.shape[-1] != 3:
        raise ValueError(f"expected frames [F, H, W, 3], got {arr.shape}")
    bcfhw = arr[np.newaxis].transpose(0, 4, 1, 2, 3).astype(np.float32) / 255
    return 2 * torch.from_numpy(np.ascontiguousarray(bcfhw)) - 1


def process_modelscope(args_dict: dict, extra_args=None):
    """Entry point B1 (process_modelscope.py:34-266).  The reference body is webui file / ffmpeg / Gradio plumbing around
    the `batch_count` loop of `pipe.infer(...)` calls (:152-221) and returns `list[str]`: one `data:video/mp4;base64,`
    URL per video, made from the mp4 that ffmpeg stitched (:248-266).  Here:
      args_dict = {model_dir | pipe, prompt, n_prompt, steps, frames, seed, cfg_scale, width, height, eta, sampler,
                   batch_count, clip_encoder | (cond, uncond), stitch,
                   clamp, percentile,                                         # x0 restriction of DDIM_Gaussian (gaussian_sampler.py:110-120), below
                   unipc,                                                     # solver options of UniPC (uni_pc/uni_pc.py:314-343), below
                   inversion,                                                 # vid2vid through DDIM inversion (ddim/sampler.py:222-267), below
                   inpaint,                                                   # img2vid keyframe blend of the legacy loop (t2v_model.py:1555-1562), below
                   context_windows,                                           # long clips through overlapping frame windows, below
                   freeu,                                                     # FreeU in the UNet (Si et al.), below
                   enable_emphasis, comma_padding_backtrack,                  # webui's opts of the prompt syntax (clip_hardcode.py:153,203)
                   do_vid2vid, vid2vid_frames, strength,                      # :80-147
                   inpainting_frames, inpainting_image, inpainting_weights,   # :170-217
                   stable_lora}                                               # :69-71, below
    * `stable_lora` = {lora_files_selection, lora_alpha, use_bias, use_linear, use_conv, use_emb, use_multiplier, use_time[, lora_dir]},
      or the same eight values as an eight-element `extra_args` in that order (the reference's): `stable_lora.StableLoraScript.process`
      runs on the pipe before sampling — the selected files are merged into `pipe.sd_model` and the text encoder's transformer, or taken
      out again when the selection, the weight or an option changed since the last call.  With neither present nothing changes.
    * `percentile` (e.g. 0.995: dynamic thresholding, s = max(quantile(|x0|, p), 1) per video) / `clamp` (any value: x0 clamped to [-1, 1],
      the reference's `clamp=True` quirk) go to `GaussianDiffusion.sample` through `infer` / `infer_conditioned`; DDIM_Gaussian only, and
      with neither key present the call is what it was.
    * `unipc` = a dict of UniPC's solver options (variant, skip_type, order, lower_order_final, initial_corrector, denoise_to_zero,
      thresholding: `samplers.UniPCSampler`); UniPC only, and without the key the call is what it was.  webui's `shared.opts` is not read.
    * `inversion` = True or a dict with guidance_scale (default 1.0) and / or model_timesteps ("index", the default and the reference's
      labels, or "schedule") (sampler "DDIM" with `do_vid2vid` only): the clip is
      taken up the deterministic trajectory by `DDIMSampler.encode` instead of being noised (`Txt2VideoSampler.sample_loop`); without
      the key the call is what it was.
    * `inpaint` = "legacy" (sampler "DDIM_Gaussian" on the img2vid route only): the mask of the img2vid route takes effect — after every step
      but the last, frames whose weight is <= (steps - i - 1) / steps are reset to the re-noised image latents, so weight 0 holds a frame
      to the picture until the last blend and weight 1 leaves it free (`GaussianDiffusion.sample`); without the key the call is what
      it was.
    * `context_windows` = {"length": 16, "overlap": 4[, "weights": "pyramid" | "flat", "batch": n]} (every sampler): a clip of more than
      `length` frames is denoised through overlapping windows of `length` frames, blended per frame at every step
      (`samplers.ContextWindows`); a shorter clip, or a call without the key, is what it was.
    * `freeu` = {"b1": 1.2, "b2": 1.4, "s1": 0.9, "s2": 0.2} (every sampler; the authors' ModelScope values): FreeU in the UNet for this
      call (`infer_conditioned`, `UNetSD.enable_freeu`); without the key the call is what it was.
    * `prompts` = [...] / `n_prompts` = [...] (or `conds` = [...] / `unconds` = [...], lists of context tensors) and optionally
      `seeds` = [...]: a batch of DIFFERENT prompts in ONE pass, one video per entry (a single negative prompt, or `prompt` / `cond`
      beside a list, is broadcast; every prompt is encoded by an encoder call of its own).  Video v starts from seeds[v] (default
      seed + v).  Without `stitch` the frames come back side by side; with it they are split per video and every video is stitched:
      one data-URL per prompt.  txt2vid and vid2vid; refused together with batch_count > 1 and on the img2vid route.
    * `stitch(frames_bgr, infotext) -> bytes` (the ffmpeg stage, out of scope — e.g. the reference's own
      `ffmpeg_stitch_video` behind a temp directory) given: returns the reference's list of data-URLs, video b from
      seed + b (seed -1 stays random), exactly the reference loop;
    * no `stitch`: returns the BGR uint8 frames of the (last) video — what the reference writes as PNGs (:225-229);
      with (cond, uncond) tensors and batch_count > 1 the videos of seeds seed .. seed + batch_count - 1 are made in ONE
      batched pass, frames side by side — vid2vid (`do_vid2vid`) too: the input clip's latents are repeated, video b gets the noise of
      seed + b.  The img2vid route stays one call per video: it draws every video's latents from numpy's global generator.
    * vid2vid (`do_vid2vid`, :80-142): `vid2vid_frames` = the input clip as [F, H, W, 3] uint8 RGB frames of ANY size — a numpy
      array or a (device) tensor such as `infer_conditioned(..., to_host=False)` returns; frames not at (height, width) are
      resized on the GPU exactly as the reference's PIL `Image.ANTIALIAS` resize does (:116-120; `pipe.resize_frames`) — or a
      [1, 3, F, H, W] float video in [-1, 1], or
      ready latents [1, 4, F, h, w]; encoded by ONE batched VAE-encoder program (`compute_latents`), then
      `skip_steps = floor(steps * clamp(1 - strength, 0, 1))` and `infer(..., latents, strength, skip_steps, is_vid2vid=True)`.
    * img2vid inpainting (`inpainting_frames` > 0 with an `inpainting_image` [H, W, 3] uint8 RGB of any size, :170-217): the image
      is resized once like a vid2vid frame (:174-178) and encoded for every frame, `inpainting_weights` = the per-frame mask weights (a sequence of `frames` floats — the reference reads
      them from its deforum-style key string through T2VAnimKeys, host plumbing), latents = image * (1 - mask) + N(0,1) * mask
      with the noise from numpy's GLOBAL generator exactly like the reference (:205), `strength = 1`, and `mask` goes to the
      sampler.  There the reference's hook is inert and so, by default, is this build's: the video only starts near
      the picture.  `inpaint` = "legacy" (above) makes the mask work during sampling."""
    import math
    global pipe
    a = SimpleNamespace(**args_dict)
    if getattr(a, "pipe", None) is not None:
        pipe = a.pipe
    elif pipe is None:
        pipe = TextToVideoSynthesis(a.model_dir, clip_encoder=getattr(a, "clip_encoder", None))
    if hasattr(pipe, "set_prompt_options"):
        pipe.set_prompt_options(getattr(a, "enable_emphasis", None), getattr(a, "comma_padding_backtrack", None))
    # the Stable LoRA stage (process_modelscope.py:69-71 -> StableLoraScript.process): merge / un-merge before anything is encoded or sampled
    lora_settings = getattr(a, "stable_lora", None)
    if lora_settings is None and extra_args is not None and len(extra_args) == 8:
        lora_settings = list(extra_args)
    if lora_settings is not None:
        from . import stable_lora
        stable_lora.run_for_pipe(pipe, lora_settings)
    width, height = getattr(a, "width", 256), getattr(a, "height", 256)
    common = dict(frames=a.frames, scale=a.cfg_scale, width=width, height=height, eta=getattr(a, "eta", 0.0),
                  sampler=getattr(a, "sampler", available_samplers[0].name),
                  **_restriction(getattr(a, "clamp", None), getattr(a, "percentile", None), getattr(a, "unipc", None),
                                 getattr(a, "inversion", None), getattr(a, "inpaint", None), getattr(a, "context_windows", None),
                                 getattr(a, "freeu", None)))
    batch_count = int(getattr(a, "batch_count", 1))
    stitch = getattr(a, "stitch", None)
    cpu_vae = getattr(a, "cpu_vae", "GPU (half precision)")
    device = pipe.device
    do_vid2vid = bool(getattr(a, "do_vid2vid", False))
    inpainting = int(getattr(a, "inpainting_frames", 0) or 0) > 0 and getattr(a, "inpainting_image", None) is not None
    have_cond = getattr(a, "cond", None) is not None

    def sized(frames):
        """uint8 [F, H, W, 3] frames at (height, width): as given when they have that size, else resized by the pipeline on the
        GPU with Pillow's Lanczos filter (process_modelscope.py:116-120,174-178) — a device tensor; a pipeline object that cannot
        resize keeps the refusal.  (Two programs here: the resize with a uint8 result, then `compute_latents` on those frames, whose
        front end is a one-tap copy pass into the encoder's tokens.  A caller that wants the single fused program calls
        `pipe.compute_latents(frames, ..., height=, width=)` itself.)"""
        if tuple(frames.shape[1:3]) == (height, width):
            return frames
        if not hasattr(pipe, "resize_frames"):
            raise ValueError(f"input frames are {tuple(frames.shape[1:3])}, expected (height, width) = {(height, width)}: this pipeline "
                             "object has no resize_frames, resize the frames before the call")
        return pipe.resize_frames(frames, height, width)

    def to_latents(video):
        """frames / float video / latents -> [1, 4, F, h, w] on the host (compute_latents, t2v_pipeline.py:148-194)."""
        if isinstance(video, torch.Tensor) and video.ndim == 5 and video.shape[1] == 4:
            return video.float().cpu()
        if isinstance(video, torch.Tensor) and video.ndim == 5:
            vd = video
        elif isinstance(video, torch.Tensor) and video.dtype == torch.uint8:
            # a uint8 clip as a tensor (e.g. the device frames of infer_conditioned(..., to_host=False)): it stays where it is
            if video.ndim != 4 or video.shape[-1] != 3:
                raise ValueError(f"expected frames [F, H, W, 3], got {tuple(video.shape)}")
            return pipe.compute_latents(sized(video), cpu_vae, device)
        else:
            arr = np.asarray(video)
            if arr.ndim != 4 or arr.shape[-1] != 3:
                raise ValueError(f"expected frames [F, H, W, 3], got {arr.shape}")
            if arr.shape[1:3] != (height, width):
                return pipe.compute_latents(sized(arr), cpu_vae, device)       # resized on the device: encoded from there
            vd = frames_to_video_tensor(arr)
        if vd.shape[-2:] != (height, width):
            raise ValueError(f"the float video is {tuple(vd.shape[-2:])}, expected (height, width) = {(height, width)}: only uint8 frames "
                             "are resized (pass the clip as [F, H, W, 3] uint8 frames)")
        return pipe.compute_latents(vd, cpu_vae, device)

    mask = None
    if do_vid2vid:
        src = getattr(a, "vid2vid_frames", None)
        if src is None:
            raise FileNotFoundError("Please upload a video :()")          # process_modelscope.py:82
        latents = to_latents(src).to(device)
        strength = float(a.strength)
        skip_steps = int(math.floor(a.steps * max(0, min(1 - strength, 1))))
    else:
        latents, strength, skip_steps = None, 1, 0            # `args.strength = 1` (:145): UniPC starts at t_start = 1.0, like ns.T

    if any(getattr(a, k, None) is not None for k in ("prompts", "n_prompts", "conds", "unconds", "seeds")):
        # a batch of different prompts: ONE pass, one video per prompt
        if batch_count > 1:
            raise ValueError("prompts / conds lists make one pass with one video per entry: not together with batch_count > 1 "
                             "(repeat an entry to have several videos of it)")
        if inpainting:
            raise NotImplementedError("a batch of different prompts: text-to-video and vid2vid only — the img2vid route draws every "
                                      "video's latents from numpy's global generator (process_modelscope.py:205), one call per video")
        seed = a.seed if a.seed != -1 else random.randint(0, 2 ** 32 - 1)
        if have_cond or getattr(a, "conds", None) is not None or getattr(a, "unconds", None) is not None:
            pick = lambda many, one: getattr(a, many) if getattr(a, many, None) is not None else getattr(a, one)
            cs, ucs, texts = pick("conds", "cond"), pick("unconds", "uncond"), None
        else:
            texts = _prompt_lists(getattr(a, "prompts", None) if getattr(a, "prompts", None) is not None else a.prompt,
                                  getattr(a, "n_prompts", None) if getattr(a, "n_prompts", None) is not None else getattr(a, "n_prompt", ""))
            cs, ucs = pipe.preprocess(texts[0], texts[1], a.steps - skip_steps)
        seeds = getattr(a, "seeds", None)
        n = max([len(v) for v in (cs, ucs, seeds) if isinstance(v, (list, tuple))], default=1)
        seeds = [int(v) for v in seeds] if seeds is not None else [seed + v for v in range(n)]
        if "half precision" in str(cpu_vae) and getattr(pipe, "autoencoder", None) is not None:
            pipe.autoencoder.half()
        vid = dict(latents=latents, strength=strength, is_vid2vid=True, device=device) if do_vid2vid else {}
        frames, _ = pipe.infer_conditioned(cs, ucs, a.steps - skip_steps, seed=seeds[0], seeds=seeds, videos=n, **vid, **common)
        if stitch is None:
            return frames                       # side by side, video v in columns [v * width, (v + 1) * width)
        import base64
        urls = []
        for v in range(n):
            info = "" if texts is None else create_infotext(dict(prompt=texts[0][v], n_prompt=texts[1][v], steps=a.steps, frames=a.frames,
                                                                 seed=seeds[v], scale=a.cfg_scale, width=width, height=height,
                                                                 eta=common["eta"], sampler=common["sampler"]))
            own = [f[:, v * width:(v + 1) * width] for f in frames]
            urls.append("data:video/mp4;base64," + base64.b64encode(stitch(own, info)).decode())
        return urls
    if have_cond and stitch is None and not do_vid2vid and not inpainting:
        frames, _ = pipe.infer_conditioned(a.cond, a.uncond, steps=a.steps, seed=a.seed, videos=batch_count, **common)
        return frames
    if have_cond and stitch is None and do_vid2vid and not inpainting and batch_count > 1:
        # the batch_count loop below in ONE pass: the clip's latents repeated, video b from the noise of seed + b
        if "half precision" in str(cpu_vae) and getattr(pipe, "autoencoder", None) is not None:
            pipe.autoencoder.half()
        frames, _ = pipe.infer_conditioned(a.cond, a.uncond, a.steps - skip_steps, seed=a.seed if a.seed != -1 else random.randint(0, 2 ** 32 - 1),
                                           latents=latents, strength=strength, is_vid2vid=True, device=device, videos=batch_count, **common)
        return frames
    urls, frames = [], None
    inpaint_sized = None
    for batch in range(batch_count):
        seed = a.seed + batch if a.seed != -1 else -1
        if inpainting:
            img = a.inpainting_image if isinstance(a.inpainting_image, torch.Tensor) else np.asarray(a.inpainting_image)
            if img.ndim != 3 or img.shape[-1] != 3:
                raise ValueError(f"inpainting image is {tuple(img.shape)}, expected [H, W, 3]")
            if tuple(img.shape[:2]) != (height, width):
                if inpaint_sized is None:
                    inpaint_sized = sized(img[None])[0]                   # ONE image through the resize, then repeated per frame
                img = inpaint_sized
            if isinstance(img, torch.Tensor):
                clip = img[None].expand(a.frames, *img.shape).contiguous()
            else:
                clip = np.repeat(img[np.newaxis], a.frames, axis=0)
            image_latents = to_latents(clip).numpy()
            lh, lw = height // 8, width // 8
            latent_noise = np.random.normal(size=(1, 4, a.frames, lh, lw))            # the reference's unseeded draw (:205)
            weights = getattr(a, "inpainting_weights", None)
            if weights is None or isinstance(weights, str):
                raise ValueError("inpainting_weights: pass the per-frame mask weights as a sequence of floats (the key-string "
                                 "parser T2VAnimKeys is webui plumbing)")
            wts = [float(weights(i)) if callable(weights) else float(weights[i]) for i in range(a.frames)]
            m = np.ones(shape=(1, 4, a.frames, lh, lw))
            for i in range(a.frames):
                m[:, :, i, :, :] = wts[i]
            latents = torch.tensor(image_latents * (1 - m) + latent_noise * m).to(device)    # float64, like the reference
            mask = torch.tensor(m).to(device)
            strength = 1
        if have_cond:
            st = None if (strength == 0.0 and not do_vid2vid) else strength
            if "half precision" in str(cpu_vae) and getattr(pipe, "autoencoder", None) is not None:
                pipe.autoencoder.half()                      # what `infer` does before decoding (t2v_pipeline.py:337-339)
            frames, _ = pipe.infer_conditioned(a.cond, a.uncond, a.steps - skip_steps, seed=seed if seed != -1 else random.randint(0, 2 ** 32 - 1),
                                               latents=latents, strength=st, mask=mask, is_vid2vid=do_vid2vid, device=device, **common)
            info = ""
        else:
            frames, _, info = pipe.infer(a.prompt, getattr(a, "n_prompt", ""), a.steps, seed=seed, cpu_vae=cpu_vae, device=device,
                                         latents=latents, skip_steps=skip_steps, strength=strength, mask=mask, is_vid2vid=do_vid2vid,
                                         **common)
        if stitch is not None:
            import base64
            urls.append("data:video/mp4;base64," + base64.b64encode(stitch(frames, info)).decode())
    return urls if stitch is not None else frames
