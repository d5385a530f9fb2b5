"""UNetSD — drop-in for the reference's 3-D UNet denoiser (boundary B4).

Same constructor keywords, same `state_dict()` key set / shapes (1480 tensors for the
ModelScope config, including the reference's `temopral_conv` spelling), same
`forward(x, t, y)` contract and `register_schedule` buffers as
reference scripts/modelscope/t2v_model.py:98-501 — but `forward` does no torch arithmetic:
it lowers the network + input geometry once into a denoise program (program.py) and executes
it with the hand-written HIP kernels of libt2v_hip.so.

The nn.Module tree below exists only to hold parameters under the reference's names (so that
`load_state_dict(strict=True)`, `.half()`, `.to()` and the LoRA hook keep working); the
sub-modules' own `forward`s are never called.

Internal data layout (resident in HBM between kernels):
  * activations: channels-last tokens, row m = ((b*F + f)*H + y)*W + x, C contiguous.
    Residual-stream tensors are fp32, MFMA operands (outputs of norms / activations /
    projections feeding a GEMM or attention) are fp16.
  * weights: packed once to [N, K] fp16, reduction ordered (64-channel chunk, tap, channel) (packing.py).
Every `rearrange(...).contiguous()` of the reference (t2v_model.py:429,458,648,655,727-761,
1006-1008) is folded into GEMM addressing or attention strides.
"""
from __future__ import annotations

import os
from functools import partial
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import packing as pk
from .compiled import ProgramHost, _Compiled, _dt  # noqa: F401  (re-exported: tests and tools import them from here)
from .lowering import _UNetLowering, canonical_context_lengths
from .program import BoundProgram, Buf, Ref


# ------------------------------------------------------------------------------------------
# topology (shared by the parameter tree and the lowering)
# ------------------------------------------------------------------------------------------
def unet_layout(dim, dim_mult, num_res_blocks, attn_scales, temporal_attention=True):
    """Block list in execution order.  Each entry: (prefix, [(kind, cin, cout), ...]).
    Mirrors the constructor loop of the reference (t2v_model.py:148-318)."""
    enc = [dim * u for u in [1] + list(dim_mult)]
    dec = [dim * u for u in [dim_mult[-1]] + list(dim_mult[::-1])]
    shortcut = [dim]
    scale = 1.0
    inputs, middle, outputs = [], [], []
    stem = [("stem", None, dim)] + ([("tt", dim, dim)] if temporal_attention else [])
    inputs.append(("input_blocks.0", stem, False))
    idx = 1
    cout = dim
    for i, (cin, cout) in enumerate(zip(enc[:-1], enc[1:])):
        for j in range(num_res_blocks):
            parts = [("res", cin, cout)]
            if scale in attn_scales:
                parts.append(("st", cout, cout))
                if temporal_attention:
                    parts.append(("tt", cout, cout))
            cin = cout
            inputs.append((f"input_blocks.{idx}", parts, False))
            idx += 1
            shortcut.append(cout)
            if i != len(dim_mult) - 1 and j == num_res_blocks - 1:
                inputs.append((f"input_blocks.{idx}", [("down", cout, cout)], True))
                idx += 1
                shortcut.append(cout)
                scale /= 2.0
    middle = [("res", cout, cout), ("st", cout, cout)] + ([("tt", cout, cout)] if temporal_attention else []) + \
             [("res", cout, cout)]
    oidx = 0
    for i, (cin, cout) in enumerate(zip(dec[:-1], dec[1:])):
        for j in range(num_res_blocks + 1):
            parts = [("res", cin + shortcut.pop(), cout)]
            if scale in attn_scales:
                parts.append(("st", cout, cout))
                if temporal_attention:
                    parts.append(("tt", cout, cout))
            cin = cout
            if i != len(dim_mult) - 1 and j == num_res_blocks:
                parts.append(("up", cout, cout))
                scale *= 2.0
            outputs.append((f"output_blocks.{oidx}", parts, False))
            oidx += 1
    return inputs, middle, outputs, cout


# ------------------------------------------------------------------------------------------
# parameter containers (reference key names)
# ------------------------------------------------------------------------------------------
def _attn_params(query_dim, context_dim, heads, dim_head):
    inner = heads * dim_head
    m = nn.Module()
    m.to_q = nn.Linear(query_dim, inner, bias=False)
    m.to_k = nn.Linear(context_dim or query_dim, inner, bias=False)
    m.to_v = nn.Linear(context_dim or query_dim, inner, bias=False)
    m.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(0.0))
    return m


def _transformer_block_params(dim, heads, d_head, context_dim):
    m = nn.Module()
    m.attn1 = _attn_params(dim, None, heads, d_head)
    ff = nn.Module()
    geglu = nn.Module()
    geglu.proj = nn.Linear(dim, dim * 4 * 2)
    ff.net = nn.Sequential(geglu, nn.Dropout(0.0), nn.Linear(dim * 4, dim))
    m.ff = ff
    m.attn2 = _attn_params(dim, context_dim, heads, d_head)
    m.norm1, m.norm2, m.norm3 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)
    return m


def _spatial_transformer_params(channels, heads, d_head, context_dim):
    inner = heads * d_head
    m = nn.Module()
    m.norm = nn.GroupNorm(32, channels, eps=1e-6, affine=True)
    m.proj_in = nn.Linear(channels, inner)
    m.transformer_blocks = nn.ModuleList([_transformer_block_params(inner, heads, d_head, context_dim)])
    m.proj_out = nn.Linear(channels, inner)     # (in, out) order as in the reference, t2v_model.py:636
    return m


def _temporal_transformer_params(channels, heads, d_head):
    inner = heads * d_head
    m = nn.Module()
    m.norm = nn.GroupNorm(32, channels, eps=1e-6, affine=True)
    m.proj_in = nn.Conv1d(channels, inner, kernel_size=1)
    m.transformer_blocks = nn.ModuleList([_transformer_block_params(inner, heads, d_head, None)])
    m.proj_out = nn.Conv1d(inner, channels, kernel_size=1)
    return m


def _temporal_conv_params(c, dropout):
    m = nn.Module()
    m.conv1 = nn.Sequential(nn.GroupNorm(32, c), nn.SiLU(), nn.Conv3d(c, c, (3, 1, 1), padding=(1, 0, 0)))
    for name in ("conv2", "conv3", "conv4"):
        setattr(m, name, nn.Sequential(nn.GroupNorm(32, c), nn.SiLU(), nn.Dropout(dropout),
                                       nn.Conv3d(c, c, (3, 1, 1), padding=(1, 0, 0))))
    return m


def _res_block_params(cin, emb, cout, dropout):
    m = nn.Module()
    m.in_layers = nn.Sequential(nn.GroupNorm(32, cin), nn.SiLU(), nn.Conv2d(cin, cout, 3, padding=1))
    m.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb, cout))
    m.out_layers = nn.Sequential(nn.GroupNorm(32, cout), nn.SiLU(), nn.Dropout(dropout),
                                 nn.Conv2d(cout, cout, 3, padding=1))
    m.skip_connection = nn.Identity() if cin == cout else nn.Conv2d(cin, cout, 1)
    m.temopral_conv = _temporal_conv_params(cout, 0.1)
    return m


def _conv_holder(attr, cin, cout, **kw):
    m = nn.Module()
    setattr(m, attr, nn.Conv2d(cin, cout, 3, **kw))
    return m


def freeu_values(freeu) -> Tuple[float, float, float, float]:
    """A `freeu=` argument — a dict with exactly the keys b1, b2, s1, s2, finite numbers — as the tuple (b1, b2, s1, s2); anything
    else is a ValueError."""
    keys = ("b1", "b2", "s1", "s2")
    if not isinstance(freeu, dict) or set(freeu) != set(keys):
        raise ValueError(f"freeu takes a dict with exactly the keys {list(keys)}, got {sorted(freeu) if isinstance(freeu, dict) else type(freeu).__name__}")
    vals = []
    for k in keys:
        v = freeu[k]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"freeu['{k}'] must be a finite number, got {v!r}")
        vals.append(float(v))
    return tuple(vals)


class freeu_scope:
    """`with freeu_scope(model, freeu):` — FreeU with these values for the calls inside, the model's earlier state restored afterwards.
    freeu = None leaves the model alone.  A model without `enable_freeu`, or one whose layout has no FreeU, refuses by raising."""

    def __init__(self, model, freeu):
        self.model, self.freeu = model, freeu

    def __enter__(self):
        if self.freeu is None:
            return self
        vals = freeu_values(self.freeu)
        m = self.model
        if not hasattr(m, "enable_freeu"):
            raise NotImplementedError(f"freeu= needs a model with enable_freeu (UNetSD), got {type(m).__name__}")
        if getattr(m, "t_shard", None) is not None:
            raise NotImplementedError("freeu= is not implemented for the T-shard layout (a clip's frames split over ranks)")
        self.held = getattr(m, "_freeu", None)
        m.enable_freeu(s1=vals[2], s2=vals[3], b1=vals[0], b2=vals[1])
        return self

    def __exit__(self, *exc):
        if self.freeu is not None:
            self.model._freeu = self.held
        return False


class UNetSD(nn.Module, ProgramHost):
    """See module docstring.  Extra keyword (not in the reference): `init_weights=False` skips
    the (slow, 1.4 G parameter) default initialisation when a state dict is loaded right after."""

    supports_cfg_batch = True     # the sampler may stack cond/uncond into one b=2 call

    def __init__(self, in_dim=7, dim=512, y_dim=512, context_dim=512, out_dim=6, dim_mult=[1, 2, 3, 4],
                 num_heads=None, head_dim=64, num_res_blocks=3, attn_scales=[1 / 2, 1 / 4, 1 / 8],
                 use_scale_shift_norm=True, dropout=0.1, temporal_attn_times=2, temporal_attention=True,
                 use_checkpoint=False, use_image_dataset=False, use_fps_condition=False, use_sim_mask=False,
                 parameterization="eps", init_weights=True):
        super().__init__()
        if use_fps_condition or use_image_dataset:
            raise NotImplementedError("fps conditioning / image-dataset mode are not on the hot path")
        embed_dim = dim * 4
        num_heads = num_heads if num_heads else dim // 32
        self.in_dim, self.dim, self.y_dim, self.context_dim = in_dim, dim, y_dim, context_dim
        self.embed_dim, self.out_dim, self.dim_mult = embed_dim, out_dim, list(dim_mult)
        self.num_heads, self.head_dim, self.num_res_blocks = num_heads, head_dim, num_res_blocks
        self.attn_scales = list(attn_scales)
        self.temporal_attention = temporal_attention
        self.parameterization = parameterization
        self.v_posterior = 0
        if head_dim != 64:
            raise NotImplementedError("attention kernel is specialised for head_dim 64")

        self._layout = unet_layout(dim, dim_mult, num_res_blocks, attn_scales, temporal_attention)
        inputs, middle, outputs, last = self._layout

        ctx = torch.device("meta") if not init_weights else torch.device("cpu")
        with ctx:
            self.time_embed = nn.Sequential(nn.Linear(dim, embed_dim), nn.SiLU(), nn.Linear(embed_dim, embed_dim))
            self.input_blocks = nn.ModuleList()
            self.middle_block = nn.ModuleList()
            self.output_blocks = nn.ModuleList()
            for prefix, parts, bare in inputs:
                mods = [self._make(kind, cin, cout, dropout, decoder=False, stem=(prefix == "input_blocks.0"))
                        for kind, cin, cout in parts]
                self.input_blocks.append(mods[0] if bare else nn.ModuleList(mods))
            for kind, cin, cout in middle:
                self.middle_block.append(self._make(kind, cin, cout, dropout, decoder=False))
            for prefix, parts, bare in outputs:
                self.output_blocks.append(nn.ModuleList(
                    [self._make(kind, cin, cout, dropout, decoder=True) for kind, cin, cout in parts]))
            self.out = nn.Sequential(nn.GroupNorm(32, last), nn.SiLU(), nn.Conv2d(last, out_dim, 3, padding=1))
        if not init_weights:
            self.to_empty(device="cpu")
        else:
            self._zero_init()

        self._init_runtime()

    def _init_runtime(self):
        """Runtime state (not part of the state dict); shared with videocrafter.UNetModel."""
        # compiled geometries kept: each owns a device arena (0.4 GiB per 24-frame sample, GiBs for long clips)
        self._init_programs(max_programs=4, fingerprint=True)
        self._param_slots = None
        self.last_repack = None       # images rewritten by the last refresh_weights (-1 = full pack)
        self.debug_taps = False
        # Storage type of tensors that are consumed ONLY by a GroupNorm (ResBlock's first conv output
        # and the three inner temporal-conv outputs): "f16" halves their HBM traffic (what the
        # reference's .half() path stores everywhere), "f32" keeps them in the fp32 stream.
        self.norm_input_dtype = L.knob("T2V_NORM_INPUT", "f16")
        # GroupNorm statistics as a by-product of the GEMM that produces the normalised tensor (T2V_EPI_STATS strips, round 4): the
        # ResBlock's conv -> norm pairs and the temporal-conv chain then run "fold strips + apply" instead of the statistics pass /
        # the single-pass kernel with its grid barrier.  Part of the program cache key.
        # MEASURED SLOWER than the single-pass kernel it replaces (same box, round 4: 31.8 vs 25.2 us at the 32x32 level, 22.9 vs 18.8 us at
        # 8x8, GroupNorm 3.40 vs 3.21 ms per step) — two launches cost what one grid barrier costs — so it is OFF by default.
        self.gn_producer_stats = L.knob("T2V_GN_STRIPS", "0") != "0"
        self.context_token = None     # one-shot hint consumed by the next forward (see forward_cfg_pair)
        self._pair_lens = None        # one-shot: (Lc, Lu) of a packed [cond | uncond] context (forward_cfg_pair)
        self._pair_ctx = None         # (context token, packed context, lengths) of the last unequal pair / batch of different prompts
        self._sample_lens = None      # one-shot: the length of every sample of a packed batch of different contexts (`_context_batch`)
        # one-shot hint consumed by the next forward: every sample of the batch has the SAME timestep (forward_cfg_pair and the samplers
        # of this package set it).  Only then may the cond | uncond pair share its prefix — the shared ops use sample 0's time embedding,
        # and forward(x[1], t = [t0, t1], ctx[2]) with t0 != t1 must keep each sample's own t
        self.single_timestep = False
        self._share_now = False
        # Precision option (off by default): weights whose packed-image name starts with one of these prefixes are applied as
        # hi + lo fp16 images in two MFMA passes (fp32 weights only; e.g. ("input_blocks.0", "input_blocks.1") — the blocks
        # that produce 46 % of the weight-rounding error).  Set before the first forward.
        self.split_weight_prefixes = ()
        # Precision (on by default): the fp32 -> fp16 operand casts whose rounding error reaches the output un-normalised — the
        # latent at the entry and the residual stream in front of the 1x1 skip convolutions — are emitted as hi + lo fp16
        # images and their (small) GEMMs run twice: 23 % of the activation-rounding error variance of a forward for ~15 extra
        # launches and +1.5 % FLOPs (tests/precision_probe.py; DESIGN.md "Precision").  Part of the program cache key.
        # Round 4 adds the next two classes of that ranking: the GroupNorm output in front of every transformer's proj_in and the
        # feed-forward output x4 in front of proj_out (rows [hi | lo] written by the producing kernel, K doubled in the C -> C
        # linear that consumes them) — at the input-resolution level, where the probe puts their whole gain; "all" = at every level
        # (+0.7 ms per step for ~1 % less error), "r3" = the round-3 subset only (A/B).
        self.precise_operands = {"0": False, "r3": "r3", "all": "all"}.get(os.environ.get("T2V_PRECISE", "1"), True)
        # Two more classes of the same ranking, built and parity-tested but OFF by default (ModelScope's outputs are inside north_star's
        # 1e-3 without them at +0.4 / +0.6 ms per step; on VideoCrafter they move the 10-step output 1.08e-3 -> 0.92e-3 but the 50-step
        # output only 1.07e-3 -> 1.04e-3): the attention output in front of to_out (input-resolution level) and the fp32 -> fp16 cast in
        # front of the Down / Upsample convolutions, both as rows [hi | lo] against [W | W].  Part of the program cache key.
        # (`precise_attn_out` is read by the VideoCrafter lowering only — videocrafter._LvdmLowering; the ModelScope lowering has no
        #  [hi | lo] attention output, so the flag does not enter ITS cache key: `_lowering_options`.)
        self.precise_attn_out = L.knob("T2V_PRECISE_ATTN", "0") != "0"
        self.precise_resample = L.knob("T2V_PRECISE_RESAMPLE", "0") != "0"
        # TemporalTransformer self-attention as ONE launch per attention (QKV projection + attention of every pixel's frame
        # sequence in the GEMM epilogue, T2V_EPI_TATTN): Q / K / V never reach HBM.  Clips of 2..32 frames; longer clips (and the
        # K/V-gather form of a T-sharded clip) keep the projection GEMM + attention kernel pair, and so do clips whose sequences fill
        # less than 144 of the tile's 192 rows (fewer than 12 frames) unless the option is "force".  Part of the program cache key.
        self.fused_temporal_attention = {"0": False, "force": "force"}.get(L.knob("T2V_FUSED_TATTN", "1"), True)
        self.t_shard = None           # parallel.TShard: this rank holds a contiguous slice of the clip's frames
        # Output dtype override for the package's own samplers.  `forward` returns what the reference's autocast path returns (fp16
        # for a `.half()` model) — but a guided step combines the two predictions as u + s (c - u): the INDEPENDENT fp16 roundings of
        # c and u (2.8e-4 each) come out multiplied by sqrt(s^2 + (s - 1)^2) ~ 12 at s = 9, which made the eps rounding the largest
        # single term of every sampled OUTPUT's error (round 4).  The samplers therefore set this to torch.float32 inside their loops
        # (the last convolution's result is fp32 in the arena anyway; the exit op writes 0.4 MB instead of 0.2 MB) and restore it.
        self.eps_out_dtype = None
        # Guided steps (forward_cfg_pair: one x_t, one t, [cond | uncond] contexts): everything up to the FIRST text cross-attention —
        # the stem, input_blocks.0's TemporalTransformer, the first ResBlock with its temporal convolutions, the first
        # SpatialTransformer's GroupNorm / proj_in / self-attention / to_q — is identical for the two samples.  With this option
        # (default on) the lowering computes that prefix ONCE (one sample's rows) and the first per-sample GEMMs read it through a row
        # wrap (T2V_OP_GEMM i[12]); the reference runs the two forwards separately and computes it twice (gaussian_sampler.py:161-162).
        # Same arithmetic on the same values; 31 of 725 ops run at half their rows.  Part of the program cache key.
        self.share_cfg_prefix = L.knob("T2V_SHARE_PREFIX", "1") != "0"
        # to_q projection + text cross-attention as ONE launch (T2V_EPI_XATTN, round 5): Q never reaches HBM; part of the program cache key.
        # Built, parity-tested and MEASURED NEUTRAL: per-op events say -6 us (32x32 level) / -12 us (16x16) per site, but the back-to-back step
        # is 26.09 vs 26.03 ms and 26.51 vs 26.37 ms on two boxes (the epilogue's K / V^T fragment loads from L2 are latency-bound: the fused
        # launch takes 53 us where projection + attention take 28 + 32) -> opt-in (T2V_XATTN=1)
        self.fused_cross_attention = L.knob("T2V_XATTN", "0") != "0"
        self._freeu = None            # (b1, b2, s1, s2) while FreeU is on (`enable_freeu`); part of the program cache key
        self.auto_refresh = True      # re-check parameter versions on every forward (~1 ms); the sampler
                                      # turns this off inside its loop after one explicit refresh
        self.device = torch.device("cpu")   # SamplerBase.register_buffers_to_model overwrites it (samplers_common.py:82)

    # ---- FreeU ------------------------------------------------------------------------------
    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"), diffusers' name and argument order: at every decoder skip
        concatenation whose stream has 4 dim channels the first half of the stream is multiplied by b1 and the low frequencies of the
        skip by s1; at 2 dim channels by b2 and s2; other widths are untouched (T2V_OP_FREEU, one in-place launch per concatenation).
        The authors' ModelScope values: b1 1.2, b2 1.4, s1 0.9, s2 0.2.  Stays on until `disable_freeu`.
        The four floats are part of the program key: every distinct set of values is a program of its own (with its own arena), and
        `max_programs` bounds how many a sweep over values keeps compiled — the oldest is evicted and lowered again when it returns."""
        if type(self) is not UNetSD:
            raise NotImplementedError(f"FreeU is implemented for the ModelScope UNet (UNetSD) only, not for the VideoCrafter path ({type(self).__name__})")
        self._freeu = freeu_values(dict(s1=s1, s2=s2, b1=b1, b2=b2))

    def disable_freeu(self):
        self._freeu = None

    @property
    def freeu(self) -> Optional[Dict[str, float]]:
        """The FreeU values in force, {"b1", "b2", "s1", "s2"}, or None (read-only: `enable_freeu` / `disable_freeu`)."""
        return dict(zip(("b1", "b2", "s1", "s2"), self._freeu)) if getattr(self, "_freeu", None) is not None else None

    # ---- parameter tree -------------------------------------------------------------------
    def _make(self, kind, cin, cout, dropout, decoder, stem=False):
        if kind == "stem":
            return nn.Conv2d(self.in_dim, cout, 3, padding=1)
        if kind == "res":
            return _res_block_params(cin, self.embed_dim, cout, dropout)
        if kind == "st":
            # decoder SpatialTransformers hard-code context_dim=1024 in the reference (:293)
            return _spatial_transformer_params(cout, cout // self.head_dim, self.head_dim,
                                               1024 if decoder else self.context_dim)
        if kind == "tt":
            # the stem TemporalTransformer gets (num_heads, head_dim) from the config (:171-179),
            # all others cout // head_dim heads
            heads = self.num_heads if stem else cout // self.head_dim
            return _temporal_transformer_params(cout, heads, self.head_dim)
        if kind == "down":
            return _conv_holder("op", cin, cout, stride=2, padding=1)
        if kind == "up":
            return _conv_holder("conv", cin, cout, padding=1)
        raise ValueError(kind)

    def _zero_init(self):
        """The reference zero-initialises the last layer of every residual branch
        (t2v_model.py:326,631-636,708-713,955-956,1215-1216)."""
        with torch.no_grad():
            for n, m in self.named_modules():
                if n.endswith("proj_out") or n.endswith("out_layers.3"):
                    for p in m.parameters():
                        p.zero_()
                if n.endswith("temopral_conv.conv4.3"):
                    m.weight.zero_(); m.bias.zero_()
            self.out[-1].weight.zero_()

    # ---- schedule buffers (t2v_model.py:329-384) --------------------------------------------
    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        if given_betas is None:
            raise NotImplementedError("pass given_betas (the pipeline always does, t2v_pipeline.py:113)")
        betas = np.asarray(given_betas, dtype=np.float64)
        alphas = 1.0 - betas
        ac = np.cumprod(alphas, axis=0)
        ac_prev = np.append(1.0, ac[:-1])
        self.num_timesteps = int(betas.shape[0])
        self.linear_start, self.linear_end = linear_start, linear_end
        t32 = partial(torch.tensor, dtype=torch.float32)
        reg = self.register_buffer
        reg("betas", t32(betas)); reg("alphas_cumprod", t32(ac)); reg("alphas_cumprod_prev", t32(ac_prev))
        reg("sqrt_alphas_cumprod", t32(np.sqrt(ac)))
        reg("sqrt_one_minus_alphas_cumprod", t32(np.sqrt(1.0 - ac)))
        reg("log_one_minus_alphas_cumprod", t32(np.log(1.0 - ac)))
        reg("sqrt_recip_alphas_cumprod", t32(np.sqrt(1.0 / ac)))
        reg("sqrt_recipm1_alphas_cumprod", t32(np.sqrt(1.0 / ac - 1)))
        pv = (1 - self.v_posterior) * betas * (1.0 - ac_prev) / (1.0 - ac) + self.v_posterior * betas
        reg("posterior_variance", t32(pv))
        reg("posterior_log_variance_clipped", t32(np.log(np.maximum(pv, 1e-20))))
        reg("posterior_mean_coef1", t32(betas * np.sqrt(ac_prev) / (1.0 - ac)))
        reg("posterior_mean_coef2", t32((1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac)))

    # ---- weights --------------------------------------------------------------------------
    def _named_params(self):
        """Walks the cached per-module `_parameters` dicts (the module tree is fixed; re-assigned or added Parameters are still seen)
        instead of `named_parameters()`: the signature is taken before every forward when `auto_refresh` is on."""
        if self._param_slots is None:
            self._param_slots = [(n + "." if n else "", m._parameters) for n, m in self.named_modules() if m._parameters]
        return [(prefix + k, p) for prefix, pd in self._param_slots for k, p in pd.items() if p is not None]

    def _bytes_changed(self, device, changed, fingerprints):
        """`verify_weights` found edited bytes: instead of dropping the pack, re-pack the images that read a changed tensor through
        the partial path of `refresh_weights` (same device addresses, cached text K/V dropped; `last_repack` reports it).  The samplers
        call `verify_weights` once per sampling call; code that edits weights in place between bare forwards calls it itself."""
        self._refresh_weights(device, also_changed=changed, fingerprints=fingerprints)

    def refresh_weights(self, device=None):
        self._refresh_weights(device)

    def _refresh_weights(self, device=None, also_changed=(), fingerprints=None):
        """(Re)pack weights if any parameter object / version changed since the last pack (or `also_changed` names a parameter whose
        bytes changed: `verify_weights`).  When only some
        parameters changed (the LoRA merge / un-merge of lora_processor.py:202-246 replaces `.weight` of the
        matched Linear / Conv modules), only the packed images that read them are rewritten, in place
        (`last_repack` = number of images, -1 for a full pack).  The packed set is the UNION of the images of every
        compiled program (a T-sharded lowering declares `:kv` / `.to_q:lin` images the unsharded one does not, and
        vice versa)."""
        device = torch.device(device) if device is not None else self._packed_device
        if device is None:
            return
        sig = self._param_signature()
        same_dev = self._packed is not None and device == self._packed_device
        if same_dev and sig == self._packed_sig and not also_changed:
            return
        packer = self._union_packer()
        sd = {k: v for k, v in self.state_dict().items()}
        if same_dev and sig.keys() == self._packed_sig.keys():
            changed = [n for n, v in sig.items() if self._packed_sig[n] != v] + list(also_changed)
            n = packer.update(self._packed, sd, device, changed, deps=self._packed_deps)
            if n >= 0:
                # images that only an EVICTED program declared are not refreshed by `update`: drop them, a re-compiled
                # geometry packs them again (`_pack_missing`) instead of finding a stale copy
                for k in [k for k in self._packed if k not in packer._names]:
                    del self._packed[k]
                    self._packed_deps.pop(k, None)
                self._packed_sig, self.last_repack = sig, n
                for c in self._programs.values():
                    c.ctx_token = None          # cached context K/V were made with the old projection weights
                self._record_fingerprints(device, fingerprints)
                return
        elif same_dev:
            extra = sorted(set(sig) - set(self._packed_sig))
            if extra:
                # e.g. a LoRA file with bias terms for bias-free projections (lora_processor.py:219-222): the
                # compiled programs have no slot for them; refuse rather than silently ignore
                raise L.T2VError("parameters were added after the denoise programs were built: "
                                 f"{extra[:4]}{' ...' if len(extra) > 4 else ''} — not supported")
        self._packed = packer.materialise(sd, device)
        self._packed_deps = dict(packer.deps)
        self._packed_sig, self._packed_device, self.last_repack = sig, device, -1
        for c in self._programs.values():
            c.bound = None
            c.ctx_token = None
        self._record_fingerprints(device, fingerprints)

    def _union_packer(self) -> pk.WeightPacker:
        if not self._programs:
            self._get_compiled_any()
        packer = pk.WeightPacker()
        for comp in self._programs.values():
            for name, dtype, fn in comp.packer.recipes:
                packer.add(name, dtype, fn)
        return packer

    def _get_compiled_any(self):
        if self._programs:
            return next(iter(self._programs.values()))
        key = (1, 1, 8, 8, 77, "f32", "f32", "f32")          # same layout as forward()'s keys
        self._programs[key] = self._compile(1, 1, 8, 8, 77, "f32", "f32")
        return self._programs[key]

    # ---- forward --------------------------------------------------------------------------
    def forward(self, x, t, y, fps=None, video_mask=None, focus_present_mask=None, prob_focus_present=0.0,
                mask_last_frame_num=0, *, adapter=None):
        """eps = model(x[b,4,F,h,w], t[b], y[b,L,ctx])  — reference t2v_model.py:386-459.
        Output dtype follows the reference under autocast: fp16 for fp16 weights, else x.dtype.
        adapter (videocrafter.UNetModel only): (samples, {ext slot: device pointer}) of the adapter features of this call — part of the
        program key, handed to `_compile`, and added to the external pointers of the run."""
        # one-shot hint of the samplers ("every sample of this call has the same timestep"): consumed before anything can raise, so that
        # a failed call never leaves it set for a later call with genuinely different timesteps
        hint_single, self.single_timestep = bool(self.single_timestep), False
        # one-shot too (`forward_cfg_pair` with unequal lengths): y is the packed context [V * Lc + V * Lu, ctx] of a [cond | uncond] batch
        pair_lens, self._pair_lens = getattr(self, "_pair_lens", None), None
        sample_lens, self._sample_lens = getattr(self, "_sample_lens", None), None
        if isinstance(y, (list, tuple)):          # an unguided batch of different contexts: one [1, L_v, ctx] or [L_v, ctx] per sample
            y, pair_lens, sample_lens = self._context_batch(list(y), self.context_token)
        if not x.is_cuda:
            raise L.T2VError("UNetSD.forward needs device tensors on an AMD GPU (no CPU fallback); "
                             "use oracle/torch_port.py for a CPU reference")
        Bx, C, F, H, W = x.shape
        if sample_lens is not None:
            assert y.ndim == 2 and y.shape[0] == sum(sample_lens)
            B, Lctx = len(sample_lens), tuple(sample_lens)
        elif pair_lens is None:
            B, Lctx = y.shape[0], y.shape[1]
        else:
            assert y.ndim == 2 and y.shape[0] % sum(pair_lens) == 0
            B, Lctx = 2 * (y.shape[0] // sum(pair_lens)), tuple(pair_lens)
        # x with fewer samples than the context: sample b of the batch reads x[b % Bx] (`forward_cfg_pair`)
        assert C == self.in_dim and B % Bx == 0 and y.shape[-1] == self.context_dim
        x = x.contiguous()
        y = y.contiguous()
        if x.dtype not in (torch.float16, torch.float32):
            x = x.float()
        if y.dtype not in (torch.float16, torch.float32):
            y = y.float()
        p0 = next(self.parameters())
        out_dtype = torch.float16 if p0.dtype == torch.float16 else torch.float32
        if getattr(self, "eps_out_dtype", None) is not None:
            out_dtype = self.eps_out_dtype              # the samplers of this package ask for fp32 (see `eps_out_dtype`)
        tf = t.to(device=x.device, dtype=torch.float32).contiguous()
        if tf.ndim == 0:
            tf = tf.expand(B).contiguous()
        shard = None
        if self.t_shard is not None and self.t_shard.size > 1:
            shard = self.t_shard.spec                             # x holds only this rank's frames
            if shard.frames != F:
                raise L.T2VError(f"T-sharded forward: this rank holds {shard.frames} of {shard.total} frames, got {F}")
            if pair_lens is not None:
                raise L.T2VError(f"T-sharded forward: cond and uncond contexts of different lengths ({pair_lens[0]} and {pair_lens[1]} tokens) "
                                 "are not supported; run one role per rank, or pad the prompts to one length")
            if sample_lens is not None:
                raise L.T2VError(f"T-sharded forward: a batch of contexts of different lengths ({list(sample_lens)} tokens) is not supported; "
                                 "run the prompts one after another, or pad them to one length")
        single = hint_single or tf.numel() == 1 or t.ndim == 0
        if not single and not tf.is_cuda:
            single = bool((tf == tf.reshape(-1)[0]).all())
        self._share_now = bool(getattr(self, "share_cfg_prefix", False)) and single
        key = self._program_key(B, F, H, W, Lctx, x.dtype, y.dtype, out_dtype, shard, Bx) + ((("adapter", adapter[0]),) if adapter else ())
        build = lambda: self._compile(B, F, H, W, Lctx, _dt(x.dtype), _dt(out_dtype), _dt(y.dtype), shard=shard,
                                      x_batch=Bx if Bx != B else 0, **({"adapter": adapter[0]} if adapter else {}))
        held = self._programs.get(key)
        if held is not None and held.prog.gn_epilogue and L.exchange_disabled():
            # an asynchronous fault was reported: lower again, without the norms fused into GEMM epilogues (_lib.exchange_disabled).
            # Assigned in place, not through `_program`: the key keeps its position in the eviction order and nothing is evicted
            self._programs[key] = build()
        comp = self._program(key, build)
        if self._packed is None or self._packed_device != x.device or self.auto_refresh:
            self.refresh_weights(x.device)
        self._pack_missing(comp, x.device)
        comp.ensure_bound(self._packed, x.device, t_shard=self.t_shard if shard is not None else None)
        out = torch.empty((B, self.out_dim, F, H, W), device=x.device, dtype=out_dtype)
        ext = {L.EXT_X: x.data_ptr(), L.EXT_T: tf.data_ptr(), L.EXT_CTX: y.data_ptr(), L.EXT_OUT: out.data_ptr()}
        if adapter:
            ext.update(adapter[1])                                # T2V_EXT_ADAPTER + k
        # step-invariant prologue: skipped only when the caller passed the token of the previous run of THIS binding
        token, self.context_token = self.context_token, None
        reuse = token is not None and comp.ctx_token == token and comp.ctx_bound is comp.bound
        if isinstance(comp.bound, BoundProgram):
            comp.bound.run(ext, torch.cuda.current_stream(x.device).cuda_stream, skip_invariant=reuse)   # one host call
        else:
            comp.bound.run(ext, torch.cuda.current_stream(x.device).cuda_stream)
        comp.ctx_token, comp.ctx_bound = token, comp.bound
        return out

    def _program_key(self, B, F, H, W, Lctx, x_dtype, y_dtype, out_dtype, shard=None, Bx=None):
        """Cache key of a compiled geometry (one helper for forward and forward_timed)."""
        return (B, F, H, W, Lctx, _dt(x_dtype), _dt(y_dtype), _dt(out_dtype)) + ((shard,) if shard else ()) + \
            ((("xb", Bx),) if (Bx is not None and Bx != B) else ()) + \
            ((("split",) + tuple(self.split_weight_prefixes),) if self.split_weight_prefixes else ()) + self._lowering_options()

    def _lowering_options(self) -> tuple:
        """Lowering switches that change the program (part of the cache key)."""
        return ((("strips",),) if getattr(self, "gn_producer_stats", False) else ()) + \
            ((("share",),) if getattr(self, "_share_now", False) else ()) + \
            ((("xattn",),) if getattr(self, "fused_cross_attention", False) else ()) + \
            ((("pattn",),) if (getattr(self, "precise_attn_out", False) and type(self) is not UNetSD) else ()) + ((("presample",),) if getattr(self, "precise_resample", False) else ()) + \
            ((("precise", str(self.precise_operands)),) if getattr(self, "precise_operands", False) else ()) + \
            ((("tattn", str(self.fused_temporal_attention)),) if getattr(self, "fused_temporal_attention", False) else ()) + \
            ((("freeu",) + tuple(self._freeu),) if getattr(self, "_freeu", None) is not None else ())

    def forward_cfg_pair(self, x, t, ctx_pair, context_token=None, single_t=None):
        """One guided step's two evaluations (gaussian_sampler.py:161-162) as ONE forward: x [V,4,F,h,w] is read twice by
        the entry op (no torch.cat([x, x])), ctx_pair = [cond (V) | uncond (V)]; -> eps [2V,...].  `context_token`: any
        hashable the caller changes whenever ctx_pair's CONTENT changes — equal to the previous call's token, the
        text-context K/V projections of that call are reused (they do not depend on x or t).
        ctx_pair may also be the pair (cond [V, Lc, ctx], uncond [V, Lu, ctx]).  Equal lengths: the same as their concatenation.
        Unequal lengths (a prompt of several 77-token chunks against a short negative prompt): still ONE program — the two contexts
        are packed without padding (V * Lc rows, then V * Lu rows; built once per `context_token`), every text cross-attention is one
        launch whose samples take the key count and K / V rows of their role, as the reference's two forwards do."""
        pair_lens = sample_lens = None
        if isinstance(ctx_pair, (tuple, list)) and any(isinstance(v, (tuple, list)) for v in ctx_pair):
            # a batch of different prompts: conds / unconds as lists of V contexts [1, L_v, ctx] or [L_v, ctx] (a tensor [V, L, ctx] beside
            # a list counts as its V rows).  Lengths that one tensor or the pair describes take those paths, bit for bit.
            c, uc = ([v for v in side] if isinstance(side, (tuple, list)) else list(side.unbind(0)) for side in ctx_pair)
            assert len(c) == len(uc), f"{len(c)} cond contexts against {len(uc)} uncond contexts"
            ctx_pair, pair_lens, sample_lens = self._context_batch(c + uc, context_token)
        if isinstance(ctx_pair, (tuple, list)):
            c, uc = ctx_pair
            assert c.ndim == 3 and uc.ndim == 3 and c.shape[0] == uc.shape[0] and c.shape[2] == uc.shape[2]
            if c.shape[1] == uc.shape[1]:
                ctx_pair = torch.cat([c, uc], dim=0)
            else:
                pair_lens = (c.shape[1], uc.shape[1])
                held = getattr(self, "_pair_ctx", None)
                if context_token is None or held is None or held[0] != context_token or held[2] != pair_lens:
                    dt = torch.promote_types(c.dtype, uc.dtype)
                    packed = torch.cat([c.to(dt).reshape(-1, c.shape[2]), uc.to(dt).reshape(-1, uc.shape[2])], dim=0)
                    held = self._pair_ctx = (context_token, packed, pair_lens)
                ctx_pair = held[1]
        B = ctx_pair.shape[0] if pair_lens is None else 2 * (ctx_pair.shape[0] // sum(pair_lens))
        if sample_lens is not None:
            B = len(sample_lens)
        tt = t.to(device=x.device, dtype=torch.float32).reshape(-1)
        if single_t is None:          # one t for every sample?  (a [1] tensor: yes; per-sample values: compared — the samplers say it outright)
            single_t = tt.shape[0] == 1 or bool((tt == tt[0]).all())
        tt = tt.repeat(B // tt.shape[0]) if tt.shape[0] != B else tt
        self.context_token = context_token
        self.single_timestep = bool(single_t)
        self._pair_lens = pair_lens
        self._sample_lens = sample_lens
        return UNetSD.forward(self, x, tt, ctx_pair)

    def _context_batch(self, seqs, context_token):
        """The contexts of a batch, one tensor [1, L, ctx] or [L, ctx] per sample -> (y, pair_lens, sample_lens) as `forward` takes them:
        one length: y [B, L, ctx]; the lengths of a pair: the packed pair and pair_lens; else every sample's rows in batch order without
        padding, [sum L, ctx], and sample_lens.  The packed tensor is built once per `context_token` (as the pair's)."""
        seqs = [v.reshape(-1, v.shape[-1]) for v in seqs]
        assert seqs and all(v.shape[1] == seqs[0].shape[1] and v.shape[0] > 0 for v in seqs)
        lens = canonical_context_lengths([v.shape[0] for v in seqs], len(seqs))
        key = ("batch", tuple(v.shape[0] for v in seqs))
        held = getattr(self, "_pair_ctx", None)
        if context_token is None or held is None or held[0] != context_token or held[2] != key:
            dt = seqs[0].dtype
            for v in seqs[1:]:
                dt = torch.promote_types(dt, v.dtype)
            held = self._pair_ctx = (context_token, torch.cat([v.to(dt) for v in seqs], dim=0), key)
        packed = held[1]
        if isinstance(lens, int):
            return packed.reshape(len(seqs), lens, -1), None, None
        if len(lens) == 2:
            return packed, lens, None
        return packed, None, lens

    def forward_timed(self, x, t, y):
        """Like forward, but returns (eps, per-op milliseconds) using HIP events around every op
        on the launch stream (bench.py roofline measurement)."""
        single = bool((t.reshape(-1) == t.reshape(-1)[0]).all())      # (a profiling entry point: the comparison may synchronise)
        self.single_timestep = single
        out = UNetSD.forward(self, x, t, y)
        comp = self._programs[self._program_key(y.shape[0], x.shape[2], x.shape[3], x.shape[4], y.shape[1], x.dtype, y.dtype, out.dtype,
                                                Bx=x.shape[0])]
        xs, ys = x.contiguous(), y.contiguous()
        tf = t.to(device=x.device, dtype=torch.float32).contiguous()
        ext = {L.EXT_X: xs.data_ptr(), L.EXT_T: tf.data_ptr(), L.EXT_CTX: ys.data_ptr(), L.EXT_OUT: out.data_ptr()}
        ms = comp.bound.run_timed(ext, torch.cuda.current_stream(x.device).cuda_stream)
        return out, ms, comp.prog

    # ---- lowering -------------------------------------------------------------------------
    def _compile(self, B, F, H, W, Lctx, x_dt, out_dt, ctx_dt="f32", shard=None, x_batch=0):
        low = _Lowering(self, B, F, H, W, Lctx, x_dt, out_dt, ctx_dt, keep_taps=self.debug_taps, shard=shard, x_batch=x_batch)
        prog = low.build()
        return _Compiled(prog, low.packer)


# ------------------------------------------------------------------------------------------
# lowering: network + geometry -> denoise program
# ------------------------------------------------------------------------------------------
class _Lowering(_UNetLowering):
    def __init__(self, net: UNetSD, *args, **kwargs):
        super().__init__(net, *args, **kwargs)
        self.fused_tattn = bool(getattr(net, "fused_temporal_attention", False))
        self.freeu = getattr(net, "_freeu", None)
        if self.freeu is not None and self.shard is not None:
            raise NotImplementedError("FreeU is not implemented for the T-shard layout (a clip's frames split over ranks)")
        # fused to_q + text cross-attention (T2V_EPI_XATTN, round 5): V^T of every site, [B][sum of inner][keys padded], step-invariant
        self.vt_all: Optional[Buf] = None
        self.vt_slices: Dict[str, int] = {}

    # -- packed-weight declarations ------------------------------------------------------------
    def w_tconv(self, key) -> Ref:
        return Ref("weight", 0, self.packer.add(key + ":t3", "f16", lambda sd, k=key: pk.tconv3(sd[k + ".weight"])))

    def w_qkv_heads(self, prefix) -> Ref:
        def fn(sd, p=prefix):
            return pk.qkv_head_major(sd[p + ".to_q.weight"], sd[p + ".to_k.weight"], sd[p + ".to_v.weight"])
        return Ref("weight", 0, self.packer.add(prefix + ":qkvh", "f16", fn))

    # -- building blocks ------------------------------------------------------------------------
    def res_block(self, prefix, x: Buf, cin, cout, h, w, dest: Optional[Buf] = None) -> Buf:
        P = self.P
        # The 1x1 skip convolution (cin != cout) reads the block input as an fp16 operand.  Where the in_layers norm is its own op anyway
        # (its input is a skip-connection concat: two producers), that norm writes the cast as a second output — no separate pass over the
        # concat tensor (round 5).  Elsewhere (the norm is fused into its producer's epilogue) the cast op stays.
        x16 = None
        cast_in_norm = (cin != cout and self.shard is None and x.cols % 8 == 0 and L.knob("T2V_GN_CAST", "1") != "0"
                        and not (P.ops and P.ops[-1].kind == L.OP_GEMM and P.ops[-1].out is x))
        if cast_in_norm:
            x16 = P.alloc(x.rows, 2 * cin if self.precise else cin, "f16")
        b = self.res_front(prefix, x, cout, h, w, per_frame=True, strips_k=9 * cin, cast=x16, cast_lo=self.precise and cast_in_norm)
        skip = self.skip_projection(prefix, x, cin, cout, x16) if cin != cout else x
        st = self.strips_for(x.rows, cout, self.F * h * w, 9 * cout, L.GATHER_CONV3X3)
        # T-sharded: every tensor a cross-frame GroupNorm + (3,1,1) convolution pair reads lives in a buffer with one halo frame either
        # side, RAW: the statistics exchange of that norm carries the boundary frames along (T2V_OP_STATS_HALO) and the norm's apply pass
        # normalises them on arrival — one exchange per temporal convolution instead of two (T2V_STATS_HALO=0: the two-exchange form)
        merged = self.shard is not None and L.knob("T2V_STATS_HALO", "1") != "0"
        hwp = h * w
        raw = P.alloc((self.F + 2) * hwp, cout, "f32") if merged else None
        h2 = self.conv3(prefix + ".out_layers.3", b, prefix + ".out_layers.3", cout, h, w, residual=skip, stats=st,
                        dest=raw.row_slice(hwp, (self.F + 1) * hwp) if merged else None)
        st_live = self.last_stats
        P.free(b)
        if skip is not x:
            P.free(skip)
        # temporal convolution block: 4 x (GN over all frames + SiLU + (3,1,1) conv), identity residual
        t = h2
        tp = prefix + ".temopral_conv"
        for name, idx in (("conv1", 2), ("conv2", 3), ("conv3", 3), ("conv4", 3)):
            if self.shard is None:
                nrm = self.gn(f"{tp}.{name}.0", t, f"{tp}.{name}.0", per_frame=False, eps=1e-5, silu=True, stats=st_live, x_dead=t is not h2)
                P.free(st)
                st = st_live = None
            else:
                # T-sharded: normalised activations go into a buffer with one halo frame either side;
                # neighbours fill the halos (zeros at the two ends of the clip = the conv's zero padding)
                R, r = self.shard.size, self.shard.index
                nrm = P.alloc((self.F + 2) * hwp, cout, "f16")
                if r == 0:
                    P.memset(f"{tp}.{name}.halo0", nrm.row_slice(0, hwp))
                if r == R - 1:
                    P.memset(f"{tp}.{name}.halo1", nrm.row_slice((self.F + 1) * hwp, (self.F + 2) * hwp))
                self.gn(f"{tp}.{name}.0", t, f"{tp}.{name}.0", per_frame=False, eps=1e-5, silu=True,
                        out=nrm.row_slice(hwp, (self.F + 1) * hwp), halo_raw=raw, stats=st_live)
                P.free(st)
                st = st_live = None
                if not merged:
                    P.halo_exchange(f"{tp}.{name}.halo", nrm, hwp, self.F, self.shard)
            if t is not h2:
                P.free(t)
            if name == "conv4":
                t = self._dest(dest, h2.rows, cout, "f32")
            elif merged:
                raw = P.alloc((self.F + 2) * hwp, cout, self.net.norm_input_dtype)
                t = raw.row_slice(hwp, (self.F + 1) * hwp)
            else:
                t = P.alloc(h2.rows, cout, self.net.norm_input_dtype)
            key = f"{tp}.{name}.{idx}"
            if name != "conv4":
                st = self.strips_for(h2.rows, cout, self.F * h * w, 3 * cout, L.GATHER_TCONV3)    # conv1 .. conv3 feed the next cross-frame GroupNorm
            op = P.gemm(key, nrm, self.w_tconv(key), cout, 3 * cout, t, bias=self.vec(key + ".bias"),
                        gather=L.GATHER_TCONV3, conv=dict(F=self.F, HW=h * w, Cin=cout),
                        residual=h2 if name == "conv4" else None, halo=self.shard is not None, stats=st if name != "conv4" else None)
            st_live = st if (st is not None and name != "conv4" and op.meta.get("stats")) else None
            P.free(nrm)
        P.free(h2)
        return t

    def transformer_block(self, prefix, x1: Buf, n1: Optional[Buf], inner, heads, kind, h, w, geom=None) -> Buf:
        """x1: fp32 [M, inner] residual stream (consumed); n1 = LayerNorm1(x1) fp16, written by the proj_in GEMM (None in the
        K/V-gather lowering of a T-sharded temporal block, which normalises on its own).  Returns fp16 [M, inner] (feeds proj_out).
        geom = (frames, pixels per frame) of x1's rows when they are NOT this rank's frame slice: the pixel-sharded
        layout of a T-sharded TemporalTransformer — all frames of the clip, hw / R pixels — where the block is local."""
        P, Mrows, hw, F, B = self.P, x1.rows, h * w, self.F, self.Bc
        local = geom is not None
        if local:
            F, hw = geom
            assert B == 1 and Mrows == F * hw
        scale = 64 ** -0.5

        def self_attention(tag, xin: Buf, n: Buf, next_norm: str) -> Tuple[Buf, Buf]:
            """n = LayerNorm{tag}(xin) (made by the op that produced xin).  Returns (x + attention, LayerNorm{next_norm} of it):
            the to_out GEMM writes the fp32 stream AND — fused into its epilogue where the tile holds whole rows — the next
            LayerNorm's fp16 output."""
            # (measured, b=2 x 24 frames: 63 vs 61 + 38 us at the 32x32 level, 55 vs 49 + 21 us at 16x16; at K = 1280 the 192x192
            #  tile's main loop loses more than the fusion saves — 60 vs 43 + 13 us — so the 8x8 / 4x4 levels keep the pair)
            #  The tile holds min(12, 192 // F) pixels x F frames: below 144 of its 192 rows (clips shorter than 12 frames: 50 % at 8 frames,
            #  25 % at 4) the padding rows cost more MFMA time than the fusion saves, and the projection + attention pair is kept; so it is
            #  when this attention's weights are hi + lo split (`split_weight_prefixes`: the fused op has no second weight pass).
            split_here = bool(self.net.split_weight_prefixes) and f"{prefix}.attn{tag}".startswith(tuple(self.net.split_weight_prefixes))
            min_rows = 1 if getattr(self.net, "fused_temporal_attention", False) == "force" else 144      # "force": tests of short clips
            if kind != "spatial" and self.fused_tattn and P.tattn_pixels_per_tile(F) * F >= min_rows and inner % 64 == 0 and inner <= 640 \
                    and not split_here:
                # temporal self-attention: QKV projection + attention in ONE launch (q / k / v never reach HBM)
                a = P.alloc(Mrows, inner, "f16")
                P.qkv_temporal_attention(f"{prefix}.attn{tag}.qkv_attn", n, self.w_qkv_heads(f"{prefix}.attn{tag}"), a, samples=B, frames=F,
                                         hw=hw, heads=heads, k=inner, scale=scale)
                P.free(n)
                xo = P.alloc(Mrows, inner, "f32")
                nn_ = P.alloc(Mrows, inner, "f16")
                P.gemm(f"{prefix}.attn{tag}.to_out", a, self.w_linear(f"{prefix}.attn{tag}.to_out.0"), inner, inner, xo,
                       bias=self.vec(f"{prefix}.attn{tag}.to_out.0.bias"), residual=xin, ln=self.ln_arg(f"{prefix}.{next_norm}", nn_))
                P.free(a, xin)
                return xo, nn_
            qkv = P.alloc(Mrows, 3 * inner, "f16")
            P.gemm(f"{prefix}.attn{tag}.qkv", n, self.w_qkv(f"{prefix}.attn{tag}"), 3 * inner, inner, qkv)
            P.free(n)
            a = P.alloc(Mrows, inner, "f16")
            ld = 3 * inner
            q, k, v = qkv.col_slice(0, inner), qkv.col_slice(inner, 2 * inner), qkv.col_slice(2 * inner, 3 * inner)
            if kind == "spatial":
                # >= 1024 tokens (the 32x32 level; the two upper levels of a 1024x576 clip): V transposed once per launch into a scratch,
                # K / V^T tiles staged by LDS-DMA, 8 waves per tile (csrc/attention.hip attn2_kernel, round 6: 656 -> 877 TF/s at 9216
                # tokens, 454 -> 560 at 1024 incl. the transposition; bit-identical results).  Fewer tokens: the extra launch costs more
                # (576 tokens: 337 vs 366 TF/s, 256: 260 vs 292 — tools/attn_probe.py).
                vt = None
                if hw >= 1024 and L.knob("T2V_ATTN2", "1") != "0":
                    vt = P.alloc(B * F * heads * 64, -(-hw // 64) * 64, "f16")
                P.attention(f"{prefix}.attn{tag}", q.ref, k.ref, v.ref, a.ref, out_buf=a, nq=hw, nk=hw, heads=heads,
                            b_outer=B * F, b_inner=1, q_strides=(ld, hw * ld, 0), kv_strides=(ld, hw * ld, 0),
                            o_strides=(inner, hw * inner, 0), scale=scale, vt_scratch=vt)
                P.free(vt)
            else:   # temporal: sequence = frames of one pixel
                P.attention(f"{prefix}.attn{tag}", q.ref, k.ref, v.ref, a.ref, out_buf=a, nq=F, nk=F, heads=heads,
                            b_outer=B, b_inner=hw, q_strides=(hw * ld, F * hw * ld, ld),
                            kv_strides=(hw * ld, F * hw * ld, ld),
                            o_strides=(hw * inner, F * hw * inner, inner), scale=scale)
            P.free(qkv)
            xo = P.alloc(Mrows, inner, "f32")
            nn_ = P.alloc(Mrows, inner, "f16")
            P.gemm(f"{prefix}.attn{tag}.to_out", a, self.w_linear(f"{prefix}.attn{tag}.to_out.0"), inner, inner, xo,
                   bias=self.vec(f"{prefix}.attn{tag}.to_out.0.bias"), residual=xin, ln=self.ln_arg(f"{prefix}.{next_norm}", nn_))
            P.free(a, xin)
            return xo, nn_

        sharded_temporal = kind == "temporal" and self.shard is not None and not local
        if sharded_temporal:
            # K/V-gather lowering (pixel count not divisible by the T group): LayerNorms as separate ops
            x2 = self.kv_gather_attention(f"{prefix}.attn1", f"{prefix}.norm1", x1, inner, heads, hw, scale)
            x3 = self.kv_gather_attention(f"{prefix}.attn2", f"{prefix}.norm2", x2, inner, heads, hw, scale)
            n3 = P.alloc(Mrows, inner, "f16")
            P.layernorm(f"{prefix}.norm3", x3, self.vec(f"{prefix}.norm3.weight"), self.vec(f"{prefix}.norm3.bias"), n3)
        else:
            x2, n2 = self_attention(1, x1, n1, "norm2")
            if kind == "spatial":
                a, Mshared = self.text_cross_attention(f"{prefix}.attn2", inner, heads, hw, scale, nrm=n2)
                Mrows = a.rows                # (B samples from here on, also where the block's input was the shared single sample)
                x3 = P.alloc(Mrows, inner, "f32")
                n3 = P.alloc(Mrows, inner, "f16")
                P.gemm(f"{prefix}.attn2.to_out", a, self.w_linear(f"{prefix}.attn2.to_out.0"), inner, inner, x3,
                       bias=self.vec(f"{prefix}.attn2.to_out.0.bias"), residual=x2, ln=self.ln_arg(f"{prefix}.norm3", n3), res_wrap=Mshared)
                P.free(a, x2)
            else:
                x3, n3 = self_attention(2, x2, n2, "norm3")
        return self.ff_tail(prefix, n3, x3, inner, h, w)

    def to_q_attention(self, attn, nrm: Buf, a: Buf, inner, heads, hw, scale, wrap: int) -> bool:
        """to_q + the 77-key attention as ONE launch (round 5): q never reaches HBM.  (At the parting site the projection runs
        for both samples from the one sample's rows: the A-operand row wrap.)"""
        if self.vt_all is None or (self.F * hw) % 32 != 0 or self.Lctx > 96 or self.Lpair is not None or self.Lsamples is not None:
            return False
        k0, _ = self.kv_slices[attn]
        vt = self.vt_all.row_slice(self.vt_slices[attn], self.vt_all.rows)           # this site's rows first; sample stride = all rows of a sample
        vt_site = Buf(vt.ref, self.vt_all.rows, self.vt_all.cols, self.vt_all.ld, "f16", owns=False)
        return self.P.to_q_cross_attention(attn + ".q_attn", nrm, self.w_linear(attn + ".to_q"), a, k=inner, heads=heads,
                                           kbuf=self.kv_all.col_slice(k0, k0 + inner), vt=vt_site, n_keys=self.Lctx, rows_per_sample=self.F * hw,
                                           samples=self.B, scale=scale, a_wrap=wrap) is not None

    def spatial_transformer(self, prefix, x: Buf, c, h, w, dest: Optional[Buf] = None) -> Buf:
        P = self.P
        heads = c // 64
        n = self.gn(prefix + ".norm", x, prefix + ".norm", per_frame=True, eps=1e-6, silu=False, lo=self.precise_at(self.precise_gn, h, w))
        x1 = P.alloc(x.rows, c, "f32")
        n1 = P.alloc(x.rows, c, "f16")
        tb = prefix + ".transformer_blocks.0"
        P.gemm(prefix + ".proj_in", n, self.w_proj(prefix + ".proj_in", n.cols // c), c, n.cols, x1, bias=self.vec(prefix + ".proj_in.bias"),
               ln=self.ln_arg(tb + ".norm1", n1), k_alg=c)
        P.free(n)
        x4 = self.transformer_block(tb, x1, n1, c, heads, "spatial", h, w)
        out = self._dest(dest, x4.rows, c, "f32")          # (x4 has B samples even when the block's input x was the shared single sample)
        P.gemm(prefix + ".proj_out", x4, self.w_proj(prefix + ".proj_out", x4.cols // c), c, x4.cols, out,
               bias=self.vec(prefix + ".proj_out.bias"), residual=x, k_alg=c, res_wrap=x.rows if x.rows != x4.rows else 0)
        P.free(x4)
        return out

    def temporal_transformer(self, prefix, x: Buf, c, heads, h, w, dest: Optional[Buf] = None) -> Buf:
        P = self.P
        inner = heads * 64
        if self.shard is not None and (h * w) % self.shard.size == 0:
            return self.temporal_transformer_resharded(prefix, x, c, heads, h, w, dest)
        n = self.gn(prefix + ".norm", x, prefix + ".norm", per_frame=False, eps=1e-6, silu=False, lo=self.precise_at(self.precise_gn, h, w))
        x1 = P.alloc(x.rows, inner, "f32")
        tb = prefix + ".transformer_blocks.0"
        n1 = None if self.shard is not None else P.alloc(x.rows, inner, "f16")
        P.gemm(prefix + ".proj_in", n, self.w_proj(prefix + ".proj_in", n.cols // c), inner, n.cols, x1, bias=self.vec(prefix + ".proj_in.bias"),
               ln=None if n1 is None else self.ln_arg(tb + ".norm1", n1), k_alg=c)
        P.free(n)
        x4 = self.transformer_block(tb, x1, n1, inner, heads, "temporal", h, w)
        out = self._dest(dest, x.rows, c, "f32")
        P.gemm(prefix + ".proj_out", x4, self.w_proj(prefix + ".proj_out", x4.cols // inner), c, x4.cols, out,
               bias=self.vec(prefix + ".proj_out.bias"), residual=x, k_alg=inner)
        P.free(x4)
        return out

    def temporal_transformer_resharded(self, prefix, x: Buf, c, heads, h, w, dest: Optional[Buf] = None) -> Buf:
        """T-sharded clip: everything between the block's GroupNorm and its `+ x` is local to a PIXEL (its tokens are the
        frames of one pixel, t2v_model.py:716-767), so instead of gathering K/V of all frames twice (6 slice-units received
        per rank) the block is resharded once: frame split -> pixel split (all frames of hw / R pixels) of the normalised
        fp16 tokens, the unsharded block lowering on that geometry, and the fp32 result back to the frame split where the
        residual is added — 0.75 + 1.5 slice-units moved per rank, and the rows are balanced even for uneven frame slices.
        Layouts: frame-sharded row = f_local * hw + pixel; pixel-sharded row = f_clip * (hw / R) + pixel_local."""
        P, sh = self.P, self.shard
        R, r, hw = sh.size, sh.index, h * w
        hwr, Ft, Fl, cb = hw // R, sh.total, self.F, sh.counts[0]          # pixels per rank, clip frames, my frames, frames per slice
        inner = heads * 64
        n = self.gn(prefix + ".norm", x, prefix + ".norm", per_frame=False, eps=1e-6, silu=False)     # [Fl*hw, c] fp16, frame split
        # ---- frames -> pixels: part q of `n` (pixels [q*hwr, (q+1)*hwr) of my frames) goes to rank q
        xp = P.alloc(Ft * hwr, c, "f16")
        stage = P.alloc(R * Fl * hwr, c, "f16")
        # (round 6: the R packs are ONE launch — part q = pixels [q*hwr, (q+1)*hwr) of my frames -> stage slot q; my own part straight
        #  into its place in xp)
        P.reshard_parts(prefix + ".f2p.pack", n, stage, parts=R, rows=Fl * hwr, chunk=hwr, s_src=hw, s_dst=hwr, part_rows_src=hwr,
                        part_rows_dst=Fl * hwr, own=r, own_other=xp.row_slice(sh.offset * hwr, (sh.offset + Fl) * hwr), own_is_src=False)
        P.alltoall(prefix + ".f2p", stage, xp, hwr * c * 2, sh, 0)
        P.free(n, stage)
        x1 = P.alloc(Ft * hwr, inner, "f32")
        n1 = P.alloc(Ft * hwr, inner, "f16")
        tb = prefix + ".transformer_blocks.0"
        P.gemm(prefix + ".proj_in", xp, self.w_linear(prefix + ".proj_in"), inner, c, x1, bias=self.vec(prefix + ".proj_in.bias"),
               ln=self.ln_arg(tb + ".norm1", n1))
        P.free(xp)
        x4 = self.transformer_block(tb, x1, n1, inner, heads, "temporal", h, w, geom=(Ft, hwr))
        yp = P.alloc(Ft * hwr, c, "f32")
        P.gemm(prefix + ".proj_out", x4, self.w_proj(prefix + ".proj_out", x4.cols // inner), c, x4.cols, yp, bias=self.vec(prefix + ".proj_out.bias"),
               k_alg=inner)
        P.free(x4)
        # ---- pixels -> frames: frames of slice q (rows [q*cb*hwr, ...) of yp) go to rank q; then unpack + residual
        back = P.alloc(R * Fl * hwr, c, "f32")
        P.alltoall(prefix + ".p2f", yp, back, hwr * c * 4, sh, 1)
        out = self._dest(dest, x.rows, c, "f32")
        P.reshard_parts(prefix + ".p2f.unpack", back, out, parts=R, rows=Fl * hwr, chunk=hwr, s_src=hwr, s_dst=hw, part_rows_src=Fl * hwr,
                        part_rows_dst=hwr, own=r, own_other=yp.row_slice(sh.offset * hwr, (sh.offset + Fl) * hwr), own_is_src=True, residual=x)
        P.free(yp, back)
        return out

    # -- whole network: the hooks of _UNetLowering.build -----------------------------------------------
    def layout(self):
        inputs, middle, outputs, _ = self.net._layout
        norm = lambda blocks: [(prefix, [(prefix if bare else f"{prefix}.{i}", *part) for i, part in enumerate(parts)])
                               for prefix, parts, bare in blocks]
        inputs, (middle,), outputs = norm(inputs), norm([("middle_block", middle, False)]), norm(outputs)
        return inputs, middle, outputs, inputs + [middle] + outputs

    def time_freqs(self) -> Ref:
        return Ref("weight", 0, self.packer.add("time_freqs", "f32", lambda sd, d=self.net.dim: torch.pow(
            10000, -torch.arange(d // 2).to(torch.float32).div(d // 2))))

    def prologue_alloc(self, sites):
        # V^T of the text context for the fused to_q + cross-attention launches: rows = the value channels of every site, keys contiguous
        # (padded to a multiple of 32, zero beyond the context length: allocated here, never freed before the end, zero from the bind)
        if not (self.shard is None and self.Lctx <= 96 and self.Lpair is None and self.Lsamples is None and bool(getattr(self.net, "fused_cross_attention", True))
                and all(c % 64 == 0 for _, c in sites)):
            return []
        off = 0
        for p, c in sites:
            self.vt_slices[p + ".transformer_blocks.0.attn2"] = off
            off += c
        self.vt_all = self.P.alloc(self.B * off, -(-self.Lctx // 32) * 32, "f16")
        return [self.vt_all]

    def prologue_extra(self, sites, ctx16: Buf):
        if self.vt_all is None:
            return
        P, B, net = self.P, self.B, self.net
        n_vt = self.vt_all.rows // B
        n4 = -(-self.Lctx // 4) * 4                 # keys of the V^T GEMMs (N % 4 == 0)
        # V^T [value channels of all sites, keys] = W_v x context^T per sample: swapped operands (the weights are the "token" operand).
        # The GEMM wants N % 4 == 0 keys: every sample's tokens are copied into its own zero-padded [n4, ctx] block, and the whole V^T
        # buffer is zeroed first, so that key columns Lctx .. lcp-1 are exactly 0 whatever the arena held and whatever the NEXT
        # sample's context contains (0 x Inf = NaN: a non-finite context must not leak into its neighbour's output).
        P.memset("attn2.vT.zero", self.vt_all).meta["step_invariant"] = True
        ctx_pad = ctx16
        if n4 > self.Lctx:
            ctx_pad = P.alloc(B * n4, net.context_dim, "f16")
            P.memset("context.pad", ctx_pad).meta["step_invariant"] = True
            for b in range(B):
                P.copy2d(f"context.pad.{b}", ctx16.row_slice(b * self.Lctx, (b + 1) * self.Lctx),
                         ctx_pad.row_slice(b * n4, b * n4 + self.Lctx)).meta["step_invariant"] = True
        w_v = Ref("weight", 0, self.packer.add("v_all:lin", "f16", lambda sd, ps=tuple(p for p, _ in sites): torch.cat(
            [sd[p + ".transformer_blocks.0.attn2.to_v.weight"] for p in ps], dim=0)))
        wv_as_a = Buf(w_v, n_vt, net.context_dim, net.context_dim, "f16")
        for b in range(B):
            P.gemm(f"attn2.vT.all.{b}", wv_as_a, ctx_pad.row_slice(b * n4, (b + 1) * n4).ref, n4, net.context_dim,
                   self.vt_all.row_slice(b * n_vt, (b + 1) * n_vt).col_slice(0, n4), ldw=net.context_dim, allow_splitk=False,
                   step_invariant=True)
        if ctx_pad is not ctx16:
            P.free(ctx_pad)

    def lower_part(self, kind, p, x: Buf, cin, cout, h, w, dest, inject) -> Buf:
        if kind == "res":
            return self.res_block(p, x, cin, cout, h, w, dest=dest)
        if kind == "st":
            return self.spatial_transformer(p, x, cout, h, w, dest=dest)
        if kind == "tt":
            heads = self.net.num_heads if p == "input_blocks.0.1" else cout // 64
            return self.temporal_transformer(p, x, cout, heads, h, w, dest=dest)
        return super().lower_part(kind, p, x, cin, cout, h, w, dest, inject)
