"""VideoCrafter (LVDM) hot path — drop-in for the denoiser, sampler and latent-diffusion wrapper of
reference scripts/videocrafter (BASELINE.json configs[4]):

  UNetModel                  lvdm/models/modules/openaimodel3d.py:310-670   (same ctor keywords, same
                             622-tensor state-dict key set incl. `attn1_tmp.relative_position_k.embeddings_table`)
  DDIMSampler                lvdm/samplers/ddim.py:9-279
  LatentDiffusion (subset)   lvdm/models/ddpm3d.py: apply_model :849-865, decode_first_stage(_2DAE) :776-793,
                             register_schedule buffers
  sample_text2video          videocrafter/sample_text2video.py:92-152

As for ModelScope (unet.py) the nn.Module tree only holds parameters under the reference's names;
`forward` lowers the network to a denoise program executed by the HIP kernels of libt2v_hip.so:
Conv3d (1,3,3) -> implicit-GEMM conv3x3 per frame, GroupNorm32 / Normalize over (c/g, t, h, w) ->
cross-frame GroupNorm, spatial self / text cross attention with 8 heads of C/8 = 40 / 80 / 160 channels ->
the MFMA flash-attention kernel, TemporalCrossAttention with relative-position terms -> T2V_OP_RELPOS_ATTN.
"""
from __future__ import annotations

import math
from base64 import b64encode
from functools import partial
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import packing as pk
from .program import Buf, Program, Ref
from .lowering import _UNetLowering
from .compiled import ProgramHost, _Compiled, _dt
from .unet import UNetSD, _attn_params


# ------------------------------------------------------------------------------------------
# topology (openaimodel3d.py:411-589)
# ------------------------------------------------------------------------------------------
def lvdm_layout(model_channels, channel_mult, num_res_blocks, attention_resolutions):
    """-> (inputs, middle, outputs, last_ch): lists of (prefix, [(kind, cin, cout), ...]); part j of a block
    lives under '<prefix>.<j>'.  kinds: stem | res | st | down | up."""
    mc = model_channels
    inputs = [("input_blocks.0", [("stem", None, mc)])]
    chans = [mc]
    ch, ds, idx = mc, 1, 1
    for level, mult in enumerate(channel_mult):
        for _ in range(num_res_blocks):
            parts = [("res", ch, mult * mc)]
            ch = mult * mc
            if ds in attention_resolutions:
                parts.append(("st", ch, ch))
            inputs.append((f"input_blocks.{idx}", parts))
            idx += 1
            chans.append(ch)
        if level != len(channel_mult) - 1:
            inputs.append((f"input_blocks.{idx}", [("down", ch, ch)]))
            idx += 1
            chans.append(ch)
            ds *= 2
    middle = [("res", ch, ch), ("st", ch, ch), ("res", ch, ch)]
    outputs = []
    oidx = 0
    for level, mult in list(enumerate(channel_mult))[::-1]:
        for i in range(num_res_blocks + 1):
            ich = chans.pop()
            parts = [("res", ch + ich, mc * mult)]
            ch = mc * mult
            if ds in attention_resolutions:
                parts.append(("st", ch, ch))
            if level and i == num_res_blocks:
                parts.append(("up", ch, ch))
                ds //= 2
            outputs.append((f"output_blocks.{oidx}", parts))
            oidx += 1
    return inputs, middle, outputs, ch


# ------------------------------------------------------------------------------------------
# parameter containers (reference key names)
# ------------------------------------------------------------------------------------------
def _conv133(cin, cout):
    return nn.Conv3d(cin, cout, (1, 3, 3), padding=(0, 1, 1))


def _lvdm_res_params(cin, emb, cout):
    m = nn.Module()
    m.in_layers = nn.Sequential(nn.GroupNorm(32, cin), nn.SiLU(), _conv133(cin, cout))
    m.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb, cout))
    m.out_layers = nn.Sequential(nn.GroupNorm(32, cout), nn.SiLU(), nn.Dropout(0.0), _conv133(cout, cout))
    m.skip_connection = nn.Identity() if cin == cout else nn.Conv3d(cin, cout, 1)
    return m


def _rel_pos_params(d_head, max_rel):
    m = nn.Module()
    m.embeddings_table = nn.Parameter(torch.empty(2 * max_rel + 1, d_head))
    nn.init.xavier_uniform_(m.embeddings_table)
    return m


def _temporal_attn_params(dim, heads, d_head, temporal_length):
    m = _attn_params(dim, None, heads, d_head)
    m.relative_position_k = _rel_pos_params(d_head, temporal_length)
    m.relative_position_v = _rel_pos_params(d_head, temporal_length)
    return m


def _st_block_params(dim, heads, d_head, context_dim, temporal_length):
    m = nn.Module()
    m.attn1 = _attn_params(dim, None, heads, d_head)
    m.attn2 = _attn_params(dim, context_dim, heads, d_head)
    ff = nn.Module()
    geglu = nn.Module()
    geglu.proj = nn.Linear(dim, dim * 4 * 2)
    ff.net = nn.Sequential(geglu, nn.Dropout(0.0), nn.Linear(dim * 4, dim))
    m.ff = ff
    m.norm1, m.norm2, m.norm3 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)
    m.attn1_tmp = _temporal_attn_params(dim, heads, d_head, temporal_length)
    m.attn2_tmp = _temporal_attn_params(dim, heads, d_head, temporal_length)
    m.norm4, m.norm5 = nn.LayerNorm(dim), nn.LayerNorm(dim)
    return m


def _st_transformer_params(channels, heads, d_head, context_dim, temporal_length):
    inner = heads * d_head
    m = nn.Module()
    m.norm = nn.GroupNorm(32, channels, eps=1e-6, affine=True)
    m.proj_in = nn.Conv3d(channels, inner, 1)
    m.transformer_blocks = nn.ModuleList([_st_block_params(inner, heads, d_head, context_dim, temporal_length)])
    m.proj_out = nn.Conv3d(inner, channels, 1)
    return m


def _holder(attr, mod):
    m = nn.Module()
    setattr(m, attr, mod)
    return m


class UNetModel(UNetSD):
    """LVDM 3-D UNet (openaimodel3d.py:310).  Supported configuration = the released VideoCrafter base model
    (base_t2v/model_config.yaml): dims=3, kernel_size_t=1, transformer_depth=1, SpatialTemporalTransformer with
    relative positions, no class / fps conditioning, no scale-shift norm, conv resampling."""

    supports_cfg_batch = True

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=3, num_classes=None, use_checkpoint=False,
                 use_fp16=False, num_heads=-1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False,
                 resblock_updown=False, transformer_depth=1, context_dim=None, legacy=True, kernel_size_t=1, padding_t=1,
                 use_temporal_transformer=True, temporal_length=None, use_relative_position=False,
                 cross_attn_on_tempoal=False, temporal_crossattn_type="crossattn", order="stst", nonlinearity_type="silu",
                 temporalcrossfirst=False, split_stcontext=False, temporal_context_dim=None, use_tempoal_causal_attn=False,
                 ST_transformer_module="attention_temporal", ST_transformer_class="SpatialTemporalTransformer",
                 init_weights=True, **kwargs):
        nn.Module.__init__(self)
        unsupported = [("num_classes", num_classes is not None), ("use_scale_shift_norm", use_scale_shift_norm),
                       ("resblock_updown", resblock_updown), ("kernel_size_t != 1", kernel_size_t != 1),
                       ("transformer_depth != 1", transformer_depth != 1), ("dims != 3", dims != 3),
                       ("conv_resample=False", not conv_resample), ("num_head_channels", num_head_channels != -1),
                       ("use_relative_position=False", not use_relative_position),
                       ("cross_attn_on_tempoal", cross_attn_on_tempoal), ("use_tempoal_causal_attn", use_tempoal_causal_attn),
                       ("nonlinearity_type", nonlinearity_type != "silu"),
                       ("ST_transformer_class", ST_transformer_class != "SpatialTemporalTransformer")]
        bad = [n for n, b in unsupported if b]
        if bad or num_heads <= 0 or temporal_length is None or context_dim is None:
            raise NotImplementedError(f"UNetModel: configuration outside the built hot path: {bad or 'num_heads/temporal_length/context_dim'}")
        self.image_size, self.in_channels, self.model_channels, self.out_channels = image_size, in_channels, model_channels, out_channels
        self.num_res_blocks, self.attention_resolutions = num_res_blocks, list(attention_resolutions)
        self.channel_mult, self.num_heads, self.temporal_length = list(channel_mult), num_heads, temporal_length
        self.use_relative_position, self.dtype = True, torch.float32
        self.time_embed_dim = model_channels * 4
        # names the shared runtime (UNetSD.forward) reads
        self.in_dim, self.out_dim, self.dim, self.embed_dim = in_channels, out_channels, model_channels, model_channels * 4
        self.context_dim = context_dim[0] if isinstance(context_dim, (list, tuple)) else context_dim
        self.parameterization, self.v_posterior = "eps", 0
        for ch in {model_channels * m for m in channel_mult}:
            if ch // num_heads not in (40, 64, 80, 160):
                raise NotImplementedError(f"attention head_dim {ch // num_heads} (kernels: 40, 64, 80, 160)")
        self._layout = lvdm_layout(model_channels, self.channel_mult, num_res_blocks, self.attention_resolutions)
        inputs, middle, outputs, last = self._layout
        emb = self.time_embed_dim

        def make(kind, cin, cout):
            if kind == "stem":
                return _conv133(in_channels, cout)
            if kind == "res":
                return _lvdm_res_params(cin, emb, cout)
            if kind == "st":
                return _st_transformer_params(cout, num_heads, cout // num_heads, self.context_dim, temporal_length)
            if kind == "down":
                return _holder("op", nn.Conv3d(cin, cout, (1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1)))
            if kind == "up":
                return _holder("conv", _conv133(cin, cout))
            raise ValueError(kind)

        ctx = torch.device("meta") if not init_weights else torch.device("cpu")
        with ctx:
            self.time_embed = nn.Sequential(nn.Linear(model_channels, emb), nn.SiLU(), nn.Linear(emb, emb))
            self.input_blocks = nn.ModuleList([nn.ModuleList([make(*p) for p in parts]) for _, parts in inputs])
            self.middle_block = nn.ModuleList([make(*p) for p in middle])
            self.output_blocks = nn.ModuleList([nn.ModuleList([make(*p) for p in parts]) for _, parts in outputs])
            self.out = nn.Sequential(nn.GroupNorm(32, last), nn.SiLU(), _conv133(model_channels, out_channels))
        if not init_weights:
            self.to_empty(device="cpu")
        else:
            self._zero_init()
        self._init_runtime()
        # Measured on this model (round 4, 16 f @256x256, deployed-weights golden): the attention-output and resample-cast splits move the
        # 10-step output 1.077e-3 -> 0.92e-3 but the 50-step output only 1.069e-3 -> 1.035e-3, for +0.3 / +0.6 ms on a 17.9 ms step — the
        # 50-step error of this model is not an operand-rounding term (DESIGN.md "Precision") — so they stay opt-in here too
        # (T2V_PRECISE_ATTN=1 / T2V_PRECISE_RESAMPLE=1, inherited defaults of UNetSD).

    def _zero_init(self):
        """zero_module(...) sites of the reference: ResBlock out conv (:209-213), transformer proj_out
        (attention_temporal.py:375-379), the q/k/v/out projections of the temporal attentions (:96-100), head conv."""
        with torch.no_grad():
            for n, m in self.named_modules():
                if n.endswith("out_layers.3") or n.endswith(".proj_out") or n == "out.2":
                    for p in m.parameters():
                        p.zero_()
                if n.endswith("attn1_tmp") or n.endswith("attn2_tmp"):
                    for q in (m.to_q, m.to_k, m.to_v, m.to_out[0]):
                        for p in q.parameters():
                            p.zero_()

    def register_schedule(self, *a, **k):
        raise AttributeError("the LVDM schedule lives on LatentDiffusion, not on the UNet")

    # ---- forward (openaimodel3d.py:632-670) ------------------------------------------------------
    def forward(self, x, timesteps=None, time_emb_replace=None, context=None, features_adapter=None, y=None, **kwargs):
        """features_adapter (openaimodel3d.py:654-663): one [b, c, t, h, w] device tensor (fp16 / fp32) per input block k with
        (k + 1) % 3 == 0, added to that block's result — the running activation and the skip connection alike.  b is the number of
        samples of `x`; when the context holds more samples (the [cond | uncond] batch of a guided step on one x_t) every role
        receives the same feature.  The list is converted to the program's layout once per distinct list (identity and `_version` of
        its tensors, as the context K/V cache is keyed); afterwards a step costs only the adds."""
        if time_emb_replace is not None or y is not None:
            raise NotImplementedError("time_emb_replace / class labels are not on the hot path")
        if features_adapter is None:
            return UNetSD.forward(self, x, timesteps, context)
        if self.t_shard is not None and self.t_shard.size > 1:
            raise L.T2VError("T-sharded forward with adapter features: sharding the features along T is not built")
        if context.shape[0] not in (x.shape[0], 2 * x.shape[0]):
            raise ValueError("adapter features: the context holds one sample per sample of x, or the [cond | uncond] pair of each")
        toks = self._adapter_tokens(list(features_adapter), x)
        return UNetSD.forward(self, x, timesteps, context,
                              adapter=(int(x.shape[0]), {L.EXT_ADAPTER + k: t.data_ptr() for k, t in enumerate(toks)}))

    def adapter_sites(self, H: int, W: int) -> List[tuple]:
        """(channels, h, w) of the result of every input block that takes an adapter feature, for an H x W latent: block k with
        (k + 1) % 3 == 0 (openaimodel3d.py:657) — the end of each level for the released two-ResBlock UNet."""
        sites, h, w = [], H, W
        for k, (_, parts) in enumerate(self._layout[0]):
            for kind, _, _ in parts:
                if kind == "down":
                    h, w = (h + 1) // 2, (w + 1) // 2
            if (k + 1) % 3 == 0:
                sites.append((parts[-1][2], h, w))
        return sites

    def _adapter_tokens(self, feats: list, x) -> List[torch.Tensor]:
        """The features as channels-last fp32 tokens [(b t h w), c] (what the injection reads), cached on the list's identity."""
        Bx, _, F, H, W = x.shape
        sites = self.adapter_sites(H, W)
        if len(feats) != len(sites):
            raise AssertionError("Mismatch features adapter")
        if len(sites) > L.EXT_SLOTS - L.EXT_ADAPTER:
            raise NotImplementedError(f"{len(sites)} adapter sites (at most {L.EXT_SLOTS - L.EXT_ADAPTER})")
        for k, (f, (c, h, w)) in enumerate(zip(feats, sites)):          # checked on every call: the same list may meet another x
            if not torch.is_tensor(f) or tuple(f.shape) != (Bx, c, F, h, w):
                raise ValueError(f"adapter feature {k}: expected shape {(Bx, c, F, h, w)} for input block {3 * k + 2}, "
                                 f"got {tuple(f.shape) if torch.is_tensor(f) else type(f).__name__}")
            if f.device != x.device or f.dtype not in (torch.float16, torch.float32):
                raise ValueError(f"adapter feature {k}: an fp16 / fp32 tensor on {x.device} is required (got {f.dtype} on {f.device})")
        key = tuple((id(f), f._version, f.data_ptr(), tuple(f.shape), tuple(f.stride()), f.dtype, f.device) for f in feats)
        cache = getattr(self, "_adapter_cache", None)
        if cache is not None and cache[0] == key:
            return cache[2]
        toks = []
        for k, (f, (c, h, w)) in enumerate(zip(feats, sites)):
            # 'b c t h w -> (b t h w) c'; what Adapter.forward / get_adapter_features return is already stored that way: no copy
            toks.append(f.permute(0, 2, 3, 4, 1).to(torch.float32).contiguous().reshape(Bx * F * h * w, c))
        self._adapter_cache = (key, feats, toks)          # (`feats` kept alive: an id() is only unique among live objects)
        self.adapter_conversions = getattr(self, "adapter_conversions", 0) + 1
        return toks

    def _compile(self, B, F, H, W, Lctx, x_dt, out_dt, ctx_dt="f32", shard=None, x_batch=0, adapter=None):
        """shard (program.TShardSpec): the clip's frames are split over a T group.  Every GroupNorm32 of this UNet spans
        all frames (all-gather of statistics partials) and the temporal attentions gather K/V along T; the (1,3,3)
        convolutions, spatial / text attention and feed-forward are frame-local (no halo exchange: kernel_size_t = 1).
        adapter: samples of the adapter features (None / 0: a program without injection sites)."""
        low = _LvdmLowering(self, B, F, H, W, Lctx, x_dt, out_dt, ctx_dt, keep_taps=self.debug_taps, shard=shard, x_batch=x_batch,
                            adapter=adapter or 0)
        return _Compiled(low.build(), low.packer)


# ------------------------------------------------------------------------------------------
# lowering
# ------------------------------------------------------------------------------------------
class _LvdmLowering(_UNetLowering):
    head_per_frame = False         # every GroupNorm32 of this UNet spans all frames of a sample

    def __init__(self, *args, adapter: int = 0, **kwargs):
        """adapter: samples of the adapter features this program adds at its injection sites (0: none — the op list is then exactly
        the one of a lowering that knows nothing of adapters)."""
        super().__init__(*args, **kwargs)
        self.adapter_fb = int(adapter)
        self.n_feat = 0               # injection sites met so far
        assert not self.adapter_fb or self.shard is None, "adapter features are not sharded along T"

    def conv3_kernel(self, key):
        """Conv3d (1, 3, 3): the 3x3 kernel of its one temporal tap."""
        return (lambda sd, k=key: sd[k + ".weight"][:, :, 0]), ":c133"

    def table(self, key) -> Ref:
        return Ref("weight", 0, self.packer.add(key + ":tab", "f32", lambda sd, k=key: sd[k]))

    def table16(self, key, frames: int, transposed: bool) -> Optional[Ref]:
        """The same table packed for the persistent MFMA kernel (whole clips of <= 16 frames, no clipping of s - t): packing.relpos_table16."""
        if frames > 16 or self.net.temporal_length < frames - 1:
            return None
        return Ref("weight", 0, self.packer.add(f"{key}:tab16{'T' if transposed else ''}.{frames}", "f16",
                                                lambda sd, k=key, f=frames, t=transposed: pk.relpos_table16(sd[k].float(), f, t)))

    def table_long(self, key, frames: int, transposed: bool) -> Optional[Ref]:
        """The same table packed for the MFMA kernel of clips of any length (packing.relpos_table_long): needed beyond 32 frames, and
        at <= 32 frames only when the T2V_RELPOS_MFMA=3 experiment selects that kernel."""
        if frames <= 32 and str(L.knob("T2V_RELPOS_MFMA", "2")) != "3":
            return None
        return Ref("weight", 0, self.packer.add(f"{key}:tabL{'T' if transposed else ''}", "f16",
                                                lambda sd, k=key, t=transposed: pk.relpos_table_long(sd[k].float(), t)))

    def plus_feature(self, name, res: Buf, feat: Buf) -> Buf:
        """res + adapter feature as a new fp32 buffer (ONE launch: T2V_OP_RESHARD_ROWS with a zero source stride — the feature's rows repeat
        for every role of a [cond | uncond] batch).  It becomes the residual of the block's last GEMM, so the block's result, written in
        place into the concat buffer, already holds the feature for both of its consumers."""
        assert res.dtype == "f32" and res.cols == feat.cols and res.rows % feat.rows == 0
        out = self.P.alloc(res.rows, res.cols, "f32")
        self.P.reshard_rows(name, feat, out, rows=res.rows, chunk=feat.rows, s_src=0, s_dst=feat.rows, residual=res)
        return out

    def res_block(self, prefix, x: Buf, cin, cout, h, w, dest: Optional[Buf] = None, inject: Optional[Buf] = None) -> Buf:
        """ResBlock._forward (openaimodel3d.py:244-271): GroupNorm32 statistics span all frames of a sample."""
        P = self.P
        b = self.res_front(prefix, x, cout, h, w, per_frame=False)
        skip = self.skip_projection(prefix, x, cin, cout) if cin != cout else x
        if inject is not None:
            with_feat = self.plus_feature(prefix + ".adapter", skip, inject)
            if skip is not x:
                P.free(skip)
            skip = with_feat
        out = self.conv3(prefix + ".out_layers.3", b, prefix + ".out_layers.3", cout, h, w, residual=skip, dest=dest)
        P.free(b)
        if skip is not x:
            P.free(skip)
        return out

    def st_transformer(self, prefix, x: Buf, c, h, w, dest: Optional[Buf] = None, inject: Optional[Buf] = None) -> Buf:
        """SpatialTemporalTransformer.forward + BasicTransformerBlockST._forward (attention_temporal.py:301-335,
        386-399): s-self, t-self (rel-pos), s-cross (text), t-self (rel-pos), GEGLU feed-forward."""
        P, net, B, F, hw = self.P, self.net, self.Bc, self.F, h * w
        heads, d = net.num_heads, c // net.num_heads
        scale = d ** -0.5
        M = x.rows
        n = self.gn(prefix + ".norm", x, prefix + ".norm", per_frame=False, eps=1e-6, silu=False, lo=self.precise_at(self.precise_gn, h, w))
        tb = prefix + ".transformer_blocks.0"
        # LayerNorms as a second output of the GEMM that produces their input (fused into the epilogue of the 192x320 tile where
        # the tile holds whole rows, C = 320: the 32x32 level; a separate LayerNorm op elsewhere — Program.gemm decides).  The
        # T-sharded lowering keeps explicit LayerNorm ops (its temporal attentions normalise inside their K/V-gather form).
        fuse = self.shard is None

        def ln_of(tag) -> Optional[tuple]:
            return self.ln_arg(f"{tb}.{tag}", P.alloc(M, c, "f16")) if fuse else None

        def layer_norm(tag, src: Buf) -> Buf:
            o = P.alloc(M, c, "f16")
            P.layernorm(f"{tb}.{tag}", src, self.vec(f"{tb}.{tag}.weight"), self.vec(f"{tb}.{tag}.bias"), o)
            return o

        cur = P.alloc(M, c, "f32")
        ln = ln_of("norm1")
        P.gemm(prefix + ".proj_in", n, self.w_proj(prefix + ".proj_in", n.cols // c), c, n.cols, cur, bias=self.vec(prefix + ".proj_in.bias"), ln=ln,
               k_alg=c)
        P.free(n)
        nxt = ln[3] if ln is not None else None          # LayerNorm(cur) for the next consumer, when already produced

        attn_lo = self.precise_at(self.precise_attn, h, w)     # attention outputs as rows [hi | lo], to_out on K = 2c against [W | W]

        def attn_out() -> Buf:
            return P.alloc(M, 2 * c if attn_lo else c, "f16")

        def out_proj(attn, a: Buf, res: Buf, next_norm: str, res_wrap: int = 0):
            o = P.alloc(M, c, "f32")
            ln = ln_of(next_norm)
            P.gemm(f"{tb}.{attn}.to_out", a, self.w_proj(f"{tb}.{attn}.to_out.0", a.cols // c), c, a.cols, o,
                   bias=self.vec(f"{tb}.{attn}.to_out.0.bias"), residual=res, ln=ln, k_alg=c, res_wrap=res_wrap)
            P.free(a, res)
            return o, (ln[3] if ln is not None else None)

        def temporal_attn_sharded(attn, norm, src: Buf):
            """The K/V-gather form; the relative position of key s to local query t is s - (t + first frame of this slice)."""
            sh = self.shard
            return self.kv_gather_attention(f"{tb}.{attn}", f"{tb}.{norm}", src, c, heads, hw, scale, out_cols=2 * c if attn_lo else c,
                                            extras=lambda: dict(
                head_dim=d, lo_off=c if attn_lo else 0,
                rel_k=self.table(f"{tb}.{attn}.relative_position_k.embeddings_table"),
                rel_v=self.table(f"{tb}.{attn}.relative_position_v.embeddings_table"),
                rel_k_long=self.table_long(f"{tb}.{attn}.relative_position_k.embeddings_table", sh.total, False),
                rel_vT_long=self.table_long(f"{tb}.{attn}.relative_position_v.embeddings_table", sh.total, True),
                max_rel=net.temporal_length, q_offset=sh.offset)), None

        def self_attn(attn, norm, src: Buf, nrm: Optional[Buf], temporal: bool, next_norm: str):
            if temporal and self.shard is not None:
                return temporal_attn_sharded(attn, norm, src)
            nrm = layer_norm(norm, src) if nrm is None else nrm
            qkv = P.alloc(M, 3 * c, "f16")
            P.gemm(f"{tb}.{attn}.qkv", nrm, self.w_qkv(f"{tb}.{attn}"), 3 * c, c, qkv)
            P.free(nrm)
            a = attn_out()
            ld, lo = 3 * c, a.ld
            q, k, v = qkv.col_slice(0, c), qkv.col_slice(c, 2 * c), qkv.col_slice(2 * c, 3 * c)
            if not temporal:
                P.attention(f"{tb}.{attn}", q.ref, k.ref, v.ref, a.ref, out_buf=a, nq=hw, nk=hw, heads=heads, b_outer=B * F,
                            b_inner=1, q_strides=(ld, hw * ld, 0), kv_strides=(ld, hw * ld, 0), o_strides=(lo, hw * lo, 0),
                            scale=scale, head_dim=d, lo_off=c if attn_lo else 0)
            else:
                P.attention(f"{tb}.{attn}", q.ref, k.ref, v.ref, a.ref, out_buf=a, nq=F, nk=F, heads=heads, b_outer=B,
                            b_inner=hw, q_strides=(hw * ld, F * hw * ld, ld), kv_strides=(hw * ld, F * hw * ld, ld),
                            o_strides=(hw * lo, F * hw * lo, lo), scale=scale, head_dim=d, lo_off=c if attn_lo else 0,
                            rel_k=self.table(f"{tb}.{attn}.relative_position_k.embeddings_table"),
                            rel_v=self.table(f"{tb}.{attn}.relative_position_v.embeddings_table"),
                            rel_k16=self.table16(f"{tb}.{attn}.relative_position_k.embeddings_table", F, False),
                            rel_vT16=self.table16(f"{tb}.{attn}.relative_position_v.embeddings_table", F, True),
                            rel_k_long=self.table_long(f"{tb}.{attn}.relative_position_k.embeddings_table", F, False),
                            rel_vT_long=self.table_long(f"{tb}.{attn}.relative_position_v.embeddings_table", F, True),
                            max_rel=net.temporal_length)
            P.free(qkv)
            return out_proj(attn, a, src, next_norm)

        cur, nxt = self_attn("attn1", "norm1", cur, nxt, temporal=False, next_norm="norm4")
        cur, nxt = self_attn("attn1_tmp", "norm4", cur, nxt, temporal=True, next_norm="norm2")
        # text cross-attention: K/V of all transformers come from ONE projection GEMM of the context
        nrm = layer_norm("norm2", cur) if nxt is None else nxt
        q = P.alloc(M, c, "f16")
        P.gemm(f"{tb}.attn2.to_q", nrm, self.w_linear(f"{tb}.attn2.to_q"), c, c, q)
        P.free(nrm)
        a, shared_rows = self.text_cross_attention(f"{tb}.attn2", c, heads, hw, scale, q=q, out_cols=2 * c if attn_lo else c, head_dim=d,
                                                   lo_off=c if attn_lo else 0)
        B, M = self.Bc, a.rows         # (cond and uncond have parted: B samples' rows from here on)
        cur, nxt = out_proj("attn2", a, cur, "norm5", res_wrap=shared_rows)
        cur, nxt = self_attn("attn2_tmp", "norm5", cur, nxt, temporal=True, next_norm="norm3")
        x4 = self.ff_tail(tb, layer_norm("norm3", cur) if nxt is None else nxt, cur, c, h, w)
        out = self._dest(dest, M, c, "f32")
        res = x
        if inject is not None:
            assert x.rows == M, "an adapter site inside the shared cond | uncond prefix must end in a convolution"
            res = self.plus_feature(prefix + ".adapter", x, inject)
        P.gemm(prefix + ".proj_out", x4, self.w_proj(prefix + ".proj_out", x4.cols // c), c, x4.cols, out, bias=self.vec(prefix + ".proj_out.bias"),
               residual=res, k_alg=c, res_wrap=x.rows if x.rows != M else 0)
        P.free(x4)
        if res is not x:
            P.free(res)
        return out

    # -- whole network: the hooks of _UNetLowering.build -----------------------------------------------
    def layout(self):
        inputs, middle, outputs, _ = self.net._layout
        norm = lambda blocks: [(prefix, [(f"{prefix}.{j}", *part) for j, part in enumerate(parts)]) for prefix, parts in blocks]
        inputs, (middle,), outputs = norm(inputs), norm([("middle_block", middle)]), norm(outputs)
        return inputs, middle, outputs, inputs + outputs + [middle]

    def time_freqs(self) -> Ref:
        """util.py:142-162: cos | sin, base 10000."""
        return Ref("weight", 0, self.packer.add("time_embed.freqs", "f32", lambda sd, half=self.net.model_channels // 2: torch.exp(
            -math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)))

    def lower_part(self, kind, p, x: Buf, cin, cout, h, w, dest, inject) -> Buf:
        if kind == "res":
            return self.res_block(p, x, cin, cout, h, w, dest=dest, inject=inject)
        if kind == "st":
            return self.st_transformer(p, x, cout, h, w, dest=dest, inject=inject)
        return super().lower_part(kind, p, x, cin, cout, h, w, dest, inject)

    def inject_for(self, k: int, c, h, w) -> Optional[Buf]:
        """The adapter feature of encoder block k (openaimodel3d.py:657-660 adds it to the block's result before `hs.append`)."""
        if not self.adapter_fb or (k + 1) % 3 != 0:
            return None
        self.n_feat += 1
        return Buf(Ref("ext", L.EXT_ADAPTER + self.n_feat - 1), self.adapter_fb * self.F * h * w, c, c, "f32")


# ------------------------------------------------------------------------------------------
# depth adapter (lvdm/models/modules/adapter.py — the T2I-Adapter network of "VideoControl")
# ------------------------------------------------------------------------------------------
def _pad64(c: int) -> int:
    return (c + 63) // 64 * 64


_BICUBIC = ProgramHost(max_programs=4)          # the tap tables are its pack
_BICUBIC_PROGRAMS = _BICUBIC._programs          # (planes, H, W, size, dtype) -> _Compiled


def _bicubic_compile(planes: int, src_hw, dst_hw, x_dt: str) -> _Compiled:
    prog, packer = Program(f"bicubic p{planes} {src_hw[0]}x{src_hw[1]} -> {dst_hw[0]}x{dst_hw[1]}"), pk.WeightPacker()
    prog.begin()
    prog.bicubic("bicubic", Ref("ext", L.EXT_X), x_dt, Ref("ext", L.EXT_OUT), packer, planes=planes, src_hw=src_hw, dst_hw=dst_hw)
    prog.finish()
    return _Compiled(prog, packer)


@torch.no_grad()
def bicubic_resize(x, size):
    """x [n, c, H, W] (fp16 / fp32, on the device) -> fp32 [n, c, *size]: the package's `F.interpolate(x, size=size, mode="bicubic",
    align_corners=False)` — the resizes the reference wraps around its depth estimator (ddpm3d.py:1443-1462) — as ONE launch of
    T2V_OP_RESAMPLE's float bicubic mode over all n c planes, both axes at once.  The taps and weights are torch's, built on the host
    in float64 (packing.bicubic_table); the arithmetic is fixed (include/t2v_hip.h), so results repeat bit for bit.  Equal sizes
    return `x.float()` without a launch (the tables would give the weights (0, 1, 0, 0): the same values for finite input).
    Programs are cached per (n c, H, W, size, dtype), at most 4 kept.  There is no CPU fallback."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise L.T2VError("bicubic_resize needs a device tensor on an AMD GPU (no CPU fallback)")
    size = tuple(int(v) for v in size)
    if x.dim() != 4 or min(x.shape) < 1 or len(size) != 2 or min(size) < 1:
        raise ValueError(f"bicubic_resize: x [n, c, H, W] and size (h, w) with positive extents are required, got {tuple(x.shape)} -> {size}")
    if x.dtype not in (torch.float16, torch.float32):
        x = x.float()
    n, c, H, W = x.shape
    if (H, W) == size:
        return x.float()
    x = x.contiguous()
    comp = _BICUBIC._program((n * c, H, W, size, x.dtype), lambda: _bicubic_compile(n * c, (H, W), size, _dt(x.dtype)))
    _BICUBIC._prepare(comp, x.device)
    out = torch.empty((n, c) + size, dtype=torch.float32, device=x.device)
    _BICUBIC._launch(comp, x.device, {L.EXT_X: x.data_ptr(), L.EXT_OUT: out.data_ptr()})
    return out


def _adapter_block_params(in_c, out_c, down, ksize, sk, use_conv):
    """ResnetBlock (adapter.py:39-71): same sub-module names, same registration order."""
    ps = ksize // 2
    m = nn.Module()
    m.in_conv = nn.Conv2d(in_c, out_c, ksize, 1, ps) if (in_c != out_c or not sk) else None
    m.block1 = nn.Conv2d(out_c, out_c, 3, 1, 1)
    m.act = nn.ReLU()
    m.block2 = nn.Conv2d(out_c, out_c, ksize, 1, ps)
    m.skep = nn.Conv2d(in_c, out_c, ksize, 1, ps) if not sk else None
    m.down = down
    if down:
        m.down_opt = _holder("op", nn.Conv2d(in_c, in_c, 3, stride=2, padding=1) if use_conv else nn.AvgPool2d(2, 2))
    return m


class Adapter(nn.Module, ProgramHost):
    """Drop-in for lvdm.models.modules.adapter.Adapter: same constructor, same state-dict keys (`load_state_dict(strict=True)` takes the
    reference's), `forward(x[n, 1, H, W]) -> [features [n, c_i, H / 2^(3+i), W / 2^(3+i)]]` — computed by ONE program of HIP kernels
    over all n frames (PixelUnshuffle(8) front end, convolutions as implicit GEMMs with ReLU / the skip as fused epilogues).  The
    module tree only holds the parameters; there is no CPU fallback.  Each feature is stored as channels-last fp32 tokens — the layout
    UNetModel's injection reads — and returned as an [n, c, h, w] view of it."""

    def __init__(self, channels=[320, 640, 1280, 1280], nums_rb=3, cin=64, ksize=3, sk=False, use_conv=True, init_weights=True):
        super().__init__()
        channels = list(channels)
        if cin != 64:
            raise NotImplementedError(f"Adapter: cin = {cin}; the front end is PixelUnshuffle(8) of ONE depth channel (cin = 64)")
        if ksize not in (1, 3):
            raise NotImplementedError(f"Adapter: ksize = {ksize} (1 or 3)")
        if not 1 <= len(channels) <= L.EXT_SLOTS - L.EXT_ADAPTER or nums_rb < 1:
            raise NotImplementedError(f"Adapter: 1 .. {L.EXT_SLOTS - L.EXT_ADAPTER} levels of at least one block")
        if not sk and any(a != b for a, b in zip(channels[:-1], channels[1:])):
            raise NotImplementedError(
                "Adapter(sk=False) with a change of channel count between levels: the reference fails too — its ResnetBlock applies "
                "skep = Conv2d(in_c, out_c) to the output of in_conv, which already has out_c channels (adapter.py:50-52,66-69)")
        self.channels, self.nums_rb, self.cin, self.ksize, self.sk, self.use_conv = channels, nums_rb, cin, ksize, bool(sk), bool(use_conv)
        with (torch.device("meta") if not init_weights else torch.device("cpu")):
            body = []
            for i in range(len(channels)):
                for j in range(nums_rb):
                    down = i != 0 and j == 0
                    body.append(_adapter_block_params(channels[i - 1] if down else channels[i], channels[i], down, ksize, sk, use_conv))
            self.body = nn.ModuleList(body)
            self.conv_in = nn.Conv2d(cin, channels[0], 3, 1, 1)
        if not init_weights:
            self.to_empty(device="cpu")
        self._init_programs(max_programs=4)          # each program owns a device arena

    def feature_shapes(self, H: int, W: int) -> List[tuple]:
        """(channels, h, w) of every feature for H x W depth frames."""
        out, h, w = [], H // 8, W // 8
        for i, c in enumerate(self.channels):
            if i:
                h, w = ((h + 1) // 2, (w + 1) // 2) if self.use_conv else (h // 2, w // 2)
            out.append((c, h, w))
        return out

    def _compile(self, n, H, W, x_dt="f32", normalise=False, front_only=False, src_hw=None) -> _Compiled:
        low = _AdapterLowering(self, n, H, W, x_dt, normalise, front_only, src_hw)
        return _Compiled(low.build(), low.packer)

    def _run(self, x, normalise: bool, front_only: bool = False, size=None):
        """size (front end only): the frames arrive at another size and are first resized to `size` with the bicubic pass, in the same program."""
        if not torch.is_tensor(x) or not x.is_cuda:
            raise L.T2VError("Adapter needs a device tensor on an AMD GPU (no CPU fallback)")
        src_hw = None
        if size is not None and x.dim() == 4 and tuple(x.shape[2:]) != tuple(size):
            assert front_only
            src_hw, size = tuple(int(v) for v in x.shape[2:]), tuple(int(v) for v in size)
            if x.shape[1] != 1 or min(src_hw) < 1 or len(size) != 2 or size[0] % 8 or size[1] % 8 or min(size) < 8:
                raise ValueError(f"Adapter: depth frames [n, 1, H', W'] and a target size of multiples of 8 are required, got {tuple(x.shape)} -> {size}")
        elif x.dim() != 4 or x.shape[1] != 1 or x.shape[2] % 8 or x.shape[3] % 8 or x.shape[2] < 8 or x.shape[3] < 8:
            raise ValueError(f"Adapter: depth frames [n, 1, H, W] with H, W multiples of 8 are required, got {tuple(x.shape)}")
        if x.dtype not in (torch.float16, torch.float32):
            x = x.float()
        x = x.contiguous()
        n = x.shape[0]
        H, W = size if src_hw is not None else x.shape[2:]
        shapes = self.feature_shapes(H, W)
        if not front_only and min(min(h, w) for _, h, w in shapes) < 1:
            raise ValueError(f"Adapter: {H} x {W} frames are too small for {len(self.channels)} levels")
        key = (n, H, W, x.dtype, bool(normalise), front_only) + ((src_hw,) if src_hw is not None else ())
        comp = self._program(key, lambda: self._compile(n, H, W, _dt(x.dtype), normalise, front_only, src_hw))
        self._prepare(comp, x.device)
        ext = {L.EXT_X: x.data_ptr()}
        if front_only:
            outs = [torch.empty(n * (H // 8) * (W // 8), 64, device=x.device, dtype=torch.float16)]
        else:
            outs = [torch.empty(n * h * w, _pad64(c), device=x.device, dtype=torch.float32) for c, h, w in shapes]
        ext.update({L.EXT_ADAPTER + k: o.data_ptr() for k, o in enumerate(outs)})
        self._launch(comp, x.device, ext)
        self.last_program = comp.prog
        return outs, shapes

    @torch.no_grad()
    def forward(self, x, normalise: bool = False):
        """x [n, 1, H, W] (fp16 / fp32, on the device) -> list of [n, c_i, h_i, w_i] fp32 features.  normalise (not in the reference's
        signature): map each frame to 2 (d - min) / (max - min + 1e-7) - 1 first, inside the front-end launch — raw depth in,
        what `T2VAdapterDepth.get_batch_depth` + `get_adapter_features` compute in two calls."""
        outs, shapes = self._run(x, normalise)
        n = x.shape[0]
        return [o.view(n, h, w, o.shape[1])[..., :c].permute(0, 3, 1, 2) for o, (c, h, w) in zip(outs, shapes)]

    @torch.no_grad()
    def normalise_depth(self, depth, size=None):
        """depth [n, 1, H, W] -> the per-frame min-max normalised depth in [-1, 1] (ddpm3d.py:1463-1464) as fp32 [n, 1, H, W]: the
        front-end op alone, its PixelUnshuffle(8) tokens folded back.  The values are the fp16 numbers the adapter's first convolution
        reads, so `forward(normalise_depth(d))` and `forward(d, normalise=True)` give the same features bit for bit.
        size (H, W) other than the depth's own: the depth maps [n, 1, H', W'] of any size are first resized to it as
        `F.interpolate(mode="bicubic", align_corners=False)` does (ddpm3d.py:1458-1462) by a bicubic pass of the SAME program, into an
        fp32 arena buffer the front end reads — no host round trip; the bits of `normalise_depth(bicubic_resize(depth, size))`."""
        (tok,), _ = self._run(depth, True, front_only=True, size=size)
        n = depth.shape[0]
        H, W = depth.shape[2:] if size is None else size
        return tok.view(n, H // 8, W // 8, 8, 8).permute(0, 1, 3, 2, 4).reshape(n, 1, H, W).float()


class _AdapterLowering:
    """Adapter.forward (adapter.py:93-105) for all n frames as one program: front end, conv_in, then every ResnetBlock = optional
    Downsample, optional in_conv, block1 + ReLU (epilogue), block2 + skip (fused residual).  Activations are channels-last tokens
    [n * h * w, C padded to 64] — fp32 for the residual stream, an fp16 cast of it as the next convolution's operand; padding channels
    meet zero weight rows / columns and stay zero.  The last block2 of level k writes feature k straight to ext slot T2V_EXT_ADAPTER + k."""

    def __init__(self, net: Adapter, n, H, W, x_dt, normalise, front_only=False, src_hw=None):
        """src_hw (front end only; the opt-in depth path): the frames arrive as [n, 1, *src_hw] and a bicubic pass resizes them to H x W first."""
        assert src_hw is None or (front_only and tuple(src_hw) != (H, W))
        self.net, self.n, self.H, self.W, self.x_dt, self.normalise, self.front_only = net, n, H, W, x_dt, normalise, front_only
        self.src_hw = src_hw
        self.P = Program(f"adapter n{n} {H}x{W}")
        self.packer = pk.WeightPacker()

    def vec(self, key, cout_p) -> Ref:
        return Ref("weight", 0, self.packer.add(key + ":v", "f32", lambda sd, k=key, c=cout_p: nn.functional.pad(sd[k].float(), (0, c - sd[k].shape[0]))))

    def weight(self, key, cout_p, cin_p, ksize) -> Ref:
        def fn(sd, k=key):
            w = sd[k + ".weight"].float()
            w = nn.functional.pad(w, (0, 0, 0, 0, 0, cin_p - w.shape[1], 0, cout_p - w.shape[0]))
            return pk.conv3x3(w) if ksize == 3 else pk.linear(w)
        return Ref("weight", 0, self.packer.add(f"{key}:{'c3' if ksize == 3 else 'lin'}", "f16", fn))

    def conv(self, key, a: Buf, cin, cout, ksize, h, w, out: Buf, *, stride=1, act=0, residual=None):
        cip, cop = _pad64(cin), _pad64(cout)
        assert a.cols == cip and out.cols == cop and a.dtype == "f16"
        if ksize == 3:
            ho, wo = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
            self.P.gemm(key, a, self.weight(key, cop, cip, 3), cop, 9 * cip, out, bias=self.vec(key + ".bias", cop), gather=L.GATHER_CONV3X3,
                        conv=dict(Hin=h, Win=w, Cin=cip, stride=stride, up=0, Hout=ho, Wout=wo), residual=residual, act=act)
        else:
            assert stride == 1
            self.P.gemm(key, a, self.weight(key, cop, cip, 1), cop, cip, out, bias=self.vec(key + ".bias", cop), residual=residual, act=act)

    def cast(self, name, x32: Buf) -> Buf:
        x16 = self.P.alloc(x32.rows, x32.cols, "f16")
        self.P.copy2d(name, x32, x16)
        return x16

    def build(self) -> Program:
        net, P, n = self.net, self.P, self.n
        h, w = self.H // 8, self.W // 8
        P.begin()
        if self.front_only:
            tok = Buf(Ref("ext", L.EXT_ADAPTER), n * h * w, 64, 64, "f16")
            src, src_dt = Ref("ext", L.EXT_X), self.x_dt
            if self.src_hw is not None:          # depth maps of another size: the bicubic pass into an fp32 arena buffer, read by the front end
                big = P.alloc(n * self.H, self.W, "f32")
                P.bicubic("resize", src, src_dt, big.ref, self.packer, planes=n, src_hw=self.src_hw, dst_hw=(self.H, self.W))
                src, src_dt = big.ref, "f32"
            P.depth_tokens("unshuffle", src, src_dt, tok, n=n, H=self.H, W=self.W, normalise=self.normalise)
            P.finish()
            return P
        tok = P.alloc(n * h * w, 64, "f16")
        P.depth_tokens("unshuffle", Ref("ext", L.EXT_X), self.x_dt, tok, n=n, H=self.H, W=self.W, normalise=self.normalise)
        ch = net.channels
        x32 = P.alloc(n * h * w, _pad64(ch[0]), "f32")
        self.conv("conv_in", tok, net.cin, ch[0], 3, h, w, x32)
        P.free(tok)
        x16 = self.cast("conv_in.cast", x32)
        last = len(ch) * net.nums_rb - 1
        for i, c in enumerate(ch):
            for j in range(net.nums_rb):
                idx = i * net.nums_rb + j
                key = f"body.{idx}"
                down = i != 0 and j == 0
                in_c = ch[i - 1] if down else c
                if down:
                    if net.use_conv:
                        ho, wo = (h + 1) // 2, (w + 1) // 2
                        d32 = P.alloc(n * ho * wo, _pad64(in_c), "f32")
                        self.conv(key + ".down_opt.op", x16, in_c, in_c, 3, h, w, d32, stride=2)
                        P.free(x16, x32)
                        x32, x16 = d32, self.cast(key + ".down_opt.cast", d32)
                    else:
                        ho, wo = h // 2, w // 2
                        d32, d16 = P.alloc(n * ho * wo, _pad64(in_c), "f32"), P.alloc(n * ho * wo, _pad64(in_c), "f16")
                        P.avgpool2(key + ".down_opt", x32, n=n, H=h, W=w, out32=d32, out16=d16)
                        P.free(x16, x32)
                        x32, x16 = d32, d16
                    h, w = ho, wo
                M = n * h * w
                if in_c != c or not net.sk:
                    y32 = P.alloc(M, _pad64(c), "f32")
                    self.conv(key + ".in_conv", x16, in_c, c, net.ksize, h, w, y32)
                    P.free(x16, x32)
                    x32, x16 = y32, self.cast(key + ".in_conv.cast", y32)
                h16 = P.alloc(M, _pad64(c), "f16")
                self.conv(key + ".block1", x16, c, c, 3, h, w, h16, act=L.ACT_RELU)
                res = x32
                if not net.sk:
                    res = P.alloc(M, _pad64(c), "f32")
                    self.conv(key + ".skep", x16, c, c, net.ksize, h, w, res)
                P.free(x16)
                out = Buf(Ref("ext", L.EXT_ADAPTER + i), M, _pad64(c), _pad64(c), "f32") if j == net.nums_rb - 1 else P.alloc(M, _pad64(c), "f32")
                self.conv(key + ".block2", h16, c, c, net.ksize, h, w, out, residual=res)
                P.free(h16, x32)
                if res is not x32:
                    P.free(res)
                x32 = out
                if idx != last:
                    x16 = self.cast(key + ".cast", x32)
        P.finish()
        return P


# ------------------------------------------------------------------------------------------
# latent-diffusion wrapper (the subset of lvdm/models/ddpm3d.py the sampling path touches)
# ------------------------------------------------------------------------------------------
class DiffusionWrapper(nn.Module):
    """ddpm3d.py:1362-1380 — only the 'crossattn' (released model) and unconditional keys are on the path."""

    def __init__(self, diffusion_model: UNetModel, conditioning_key="crossattn"):
        super().__init__()
        self.diffusion_model = diffusion_model
        self.conditioning_key = conditioning_key

    def forward(self, x, t, c_concat: list = None, c_crossattn: list = None, **kwargs):
        if self.conditioning_key != "crossattn":
            raise NotImplementedError(f"conditioning_key {self.conditioning_key!r}")
        return self.diffusion_model(x, t, context=torch.cat(c_crossattn, 1), **kwargs)


class LatentDiffusion(nn.Module):
    """State-dict layout of the released checkpoint for the parts on the path: 'model.diffusion_model.*'
    (UNetModel), 'first_stage_model.*' (AutoencoderKL) and the schedule buffers.  The text encoder
    ('cond_stage_model.*', FrozenCLIPEmbedder) is outside the hot path: pass any object with `.encode(prompts)`."""

    def __init__(self, unet_config: dict, first_stage_config: Optional[dict] = None, cond_stage_model=None, timesteps=1000,
                 linear_start=0.00085, linear_end=0.012, image_size=(32, 32), video_length=16, channels=4,
                 scale_factor=0.18215, shift_factor=0.0, conditioning_key="crossattn", init_weights=True, **ignored):
        super().__init__()
        from .vae import AutoencoderKL
        self.model = DiffusionWrapper(UNetModel(**unet_config, init_weights=init_weights), conditioning_key)
        self.first_stage_model = None
        if first_stage_config is not None:
            self.first_stage_model = AutoencoderKL(first_stage_config["ddconfig"], first_stage_config.get("embed_dim", 4),
                                                   init_weights=init_weights)
        self.cond_stage_model = cond_stage_model
        self.image_size, self.video_length, self.channels = image_size, video_length, channels
        self.scale_factor, self.shift_factor = scale_factor, shift_factor
        self.conditioning_key = conditioning_key
        self.parameterization, self.v_posterior, self.encoder_type = "eps", 0.0, "2d"
        self.cond_stage2_config = None
        self.register_schedule(timesteps=timesteps, linear_start=linear_start, linear_end=linear_end)

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4, linear_end=2e-2,
                          cosine_s=8e-3):
        """DDPM.register_schedule (ddpm3d.py:125-165): 'linear' = linspace(sqrt(s), sqrt(e), T, f64)^2, fp32 buffers."""
        if given_betas is not None:
            betas = np.asarray(given_betas, dtype=np.float64)
        elif beta_schedule == "linear":
            betas = (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=torch.float64) ** 2).numpy()
        else:
            raise NotImplementedError(beta_schedule)
        alphas = 1.0 - betas
        ac = np.cumprod(alphas, axis=0)
        ac_prev = np.append(1.0, ac[:-1])
        self.num_timesteps = int(betas.shape[0])
        self.linear_start, self.linear_end = linear_start, linear_end
        t32 = partial(torch.tensor, dtype=torch.float32)
        for name, val in (("betas", betas), ("alphas_cumprod", ac), ("alphas_cumprod_prev", ac_prev),
                          ("sqrt_alphas_cumprod", np.sqrt(ac)), ("sqrt_one_minus_alphas_cumprod", np.sqrt(1.0 - ac)),
                          ("log_one_minus_alphas_cumprod", np.log(1.0 - ac)), ("sqrt_recip_alphas_cumprod", np.sqrt(1.0 / ac)),
                          ("sqrt_recipm1_alphas_cumprod", np.sqrt(1.0 / ac - 1))):
            self.register_buffer(name, t32(val))
        self._schedule_names = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                                "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")

    def _apply(self, fn, *args, **kwargs):
        """`.half()` puts the NETWORKS in fp16; the schedule stays fp32 (the reference registers it as fp32 and never halves this
        module: ddpm3d.py:125-165, sample_text2video.py).  A schedule rounded to fp16 is a 3e-4 error of every DDIM coefficient that
        is the same for all pixels and does not average out over the steps — measured on configs[4]: 50-step output 1.06e-3 with the
        rounded schedule, 4.96e-4 with this one (10 steps: 1.08e-3 -> 9.4e-4)."""
        keep = {n: self._buffers[n] for n in getattr(self, "_schedule_names", ()) if self._buffers.get(n) is not None}
        super()._apply(fn, *args, **kwargs)
        for n, v in keep.items():
            cur = self._buffers[n]
            # only a cast to a LOWER-precision float is undone (.half() / .bfloat16()); .double() / .to(torch.float64) take effect
            if cur.dtype != v.dtype and cur.dtype in (torch.float16, torch.bfloat16):
                self._buffers[n] = v.to(cur.device)
        return self

    @property
    def device(self):
        return self.betas.device

    def get_learned_conditioning(self, c):
        """ddpm3d.py:647-658."""
        m = self.cond_stage_model
        if m is None:
            raise RuntimeError("no cond_stage_model (text encoder) attached")
        if hasattr(m, "encode") and callable(m.encode):
            return m.encode(c)
        return m(c)

    def apply_model(self, x_noisy, t, cond, return_ids=False, **kwargs):
        """ddpm3d.py:849-865."""
        if not isinstance(cond, dict):
            cond = {"c_crossattn": cond if isinstance(cond, list) else [cond]}
        out = self.model(x_noisy, t, **cond, **kwargs)
        return out[0] if isinstance(out, tuple) and not return_ids else out

    def q_sample(self, x_start, t, noise=None):
        """ddpm3d.py:283-286: sqrt(ac[t]) * x_start + sqrt(1 - ac[t]) * noise, t a long tensor [b], from the fp32 schedule buffers.
        noise=None draws torch.randn(x_start.shape) from the CPU default generator and moves it to x_start's device: the stream the
        reference's `randn_like` gives on its CPU path, and the same on any device (the convention of DDIMSampler.noise_gen)."""
        if noise is None:
            noise = torch.randn(tuple(x_start.shape)).to(x_start.device)
        t = t.to(device=self.sqrt_alphas_cumprod.device, dtype=torch.long)
        bshape = (t.shape[0],) + (1,) * (x_start.dim() - 1)          # extract_into_tensor (util.py)
        a = self.sqrt_alphas_cumprod.gather(-1, t).reshape(bshape).to(x_start.device)
        s = self.sqrt_one_minus_alphas_cumprod.gather(-1, t).reshape(bshape).to(x_start.device)
        return a * x_start + s * noise

    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """ddpm3d.py:636-644: a posterior is sampled (with `noise` if given), a tensor is taken as z; -> scale_factor * (z + shift_factor)."""
        from .vae import DiagonalGaussianDistribution
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample(noise=noise)
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * (z + self.shift_factor)

    @torch.no_grad()
    def encode_first_stage_2DAE(self, x, encode_bs=16):
        """ddpm3d.py:796-810: x [b, 3, t, H, W] in [-1, 1] -> sampled, scaled latent [b, 4, t, H/8, W/8].  The reference encodes the
        (b t) frames in chunks of encode_bs and samples each chunk's posterior with torch.randn on the CPU default generator
        (distributions.py:16-21).  Here ONE encoder program covers all frames (frames are independent); the posterior noise is
        still drawn chunk by chunk, in the reference's chunk shapes and order — chunked draws need not equal one big draw."""
        if encode_bs is None:
            raise NotImplementedError("encode_first_stage_2DAE(encode_bs=None) hands a posterior object to rearrange "
                                      "(autoencoder.py:95-100, ddpm3d.py:799-800, :809): the reference fails too")
        if x.dim() != 5:
            raise ValueError(f"x must be [b, 3, t, H, W], got {tuple(x.shape)}")
        b, _, t, _, _ = x.shape
        frames = x.permute(0, 2, 1, 3, 4).reshape(b * t, x.shape[1], x.shape[3], x.shape[4])
        posterior = self.first_stage_model.encode(frames)
        n, shape = b * t, tuple(posterior.mean.shape[1:])
        noise = torch.cat([torch.randn((min(encode_bs, n - k),) + shape) for k in range(0, n, encode_bs)], dim=0)
        z = self.get_first_stage_encoding(posterior, noise=noise.to(device=posterior.mean.device, dtype=posterior.mean.dtype))
        return z.reshape(b, t, *z.shape[1:]).permute(0, 2, 1, 3, 4)

    @torch.no_grad()
    def encode_first_stage(self, x):
        raise NotImplementedError("encode_first_stage hands a posterior object to rearrange (autoencoder.py:95-100, "
                                  "ddpm3d.py:817-818): the reference fails too — use encode_first_stage_2DAE(x, encode_bs)")

    @torch.no_grad()
    def decode(self, z, **kwargs):
        z = 1.0 / self.scale_factor * z - self.shift_factor
        return self.first_stage_model.decode(z)

    @torch.no_grad()
    def decode_first_stage_2DAE(self, z, decode_bs=16, return_cpu=True, **kwargs):
        """ddpm3d.py:776-788: frames decoded in chunks of decode_bs (None = all at once)."""
        b, _, t, _, _ = z.shape
        zf = z.permute(0, 2, 1, 3, 4).reshape(b * t, z.shape[1], z.shape[3], z.shape[4])
        chunks = [zf] if decode_bs is None else torch.split(zf, decode_bs, dim=0)
        outs = [self.decode(c) for c in chunks]
        res = torch.cat([o.cpu() for o in outs] if return_cpu else outs, dim=0)
        return res.reshape(b, t, *res.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()

    @torch.no_grad()
    def decode_first_stage(self, z, decode_bs=16, return_cpu=True, **kwargs):
        assert self.encoder_type == "2d" and z.dim() == 5
        return self.decode_first_stage_2DAE(z, decode_bs=decode_bs, return_cpu=return_cpu, **kwargs)

    @torch.no_grad()
    def decode_first_stage_uint8(self, z, decode_bs=16, to_host=True):
        """z [b, 4, t, h, w] -> uint8 [b, t, H, W, 3]: the bytes of `torch_to_np(decode_first_stage(z, decode_bs, return_cpu=False))`
        without a float video.  The frames are decoded in the chunks `decode_first_stage_2DAE` takes (None = all at once, a ragged last
        chunk allowed); each chunk's decoder program ends in T2V_OP_TO_UINT8 form 1 in place of the NCHW store and writes its slice of
        the one output tensor, so 3 bytes per pixel cross to the host (`to_host`) instead of 12 (fp32 weights) or 6 (fp16)."""
        assert self.encoder_type == "2d" and z.dim() == 5
        b, _, t, h, w = z.shape
        zf = z.permute(0, 2, 1, 3, 4).reshape(b * t, z.shape[1], h, w)
        zf = 1.0 / self.scale_factor * zf - self.shift_factor
        ae = self.first_stage_model
        out = torch.empty((b * t, 8 * h, 8 * w, ae.ddconfig["out_ch"]), device=z.device, dtype=torch.uint8)
        step = b * t if decode_bs is None else decode_bs
        for k in range(0, b * t, step):
            ae.decode_to_uint8(zf[k:k + step], videos=1, form="np", out=out[k:k + step])
        out = out.view(b, t, *out.shape[1:])
        return out.cpu() if to_host else out


class T2VAdapterDepth(LatentDiffusion):
    """ddpm3d.py:1436-1484 — LatentDiffusion + the depth adapter ("VideoControl").  The reference builds its parts from configs;
    here `adapter_config` is an `Adapter` or a dict {"params": {Adapter keywords}, "cond_name": "depth"}, and `depth_stage_config`
    an optional depth estimator: any callable frames [n, 3, H, W] -> depth [n, 1, H, W] on the device (the MiDaS network itself is
    outside this package).  State-dict keys of the adapter: 'adapter.*', as in the released checkpoint.
    depth_resize (keyword, or set the attribute later; default None): the size (h, w) the estimator works at — the reference's MiDaS
    takes (384, 384).  `get_batch_depth(videos, target_size)` then wraps the estimator in the reference's two bicubic resizes
    (ddpm3d.py:1443-1468), on the GPU.  None: the estimator is called on the frames as they are and must answer at target_size."""

    def __init__(self, depth_stage_config=None, adapter_config=None, *args, depth_resize=None, **kwargs):
        init_weights = kwargs.get("init_weights", True)
        super().__init__(*args, **kwargs)
        self.depth_resize = None if depth_resize is None else tuple(int(v) for v in depth_resize)
        if isinstance(adapter_config, Adapter):
            self.adapter, self.condtype = adapter_config, "depth"
        else:
            cfg = dict(adapter_config or {})
            self.adapter = Adapter(**dict(cfg.get("params", {})), init_weights=init_weights)
            self.condtype = cfg.get("cond_name", "depth")
        self.depth_stage_model = depth_stage_config

    def prepare_midas_input(self, batch_x):
        """ddpm3d.py:1443-1447: frames [n, 3, H, W] -> fp32 [n, 3, 384, 384], MiDaS' input size, by the bicubic launch."""
        return bicubic_resize(batch_x, (384, 384))

    @torch.no_grad()
    def get_batch_depth(self, batch_x=None, target_size=None, encode_bs=1, depth=None):
        """videos batch_x [b, 3, t, h, w] -> min-max normalised depth [b, 1, t, H, W] in [-1, 1] (ddpm3d.py:1449-1469).
        `depth_stage_model` is called ONCE on all (b t) frames.  With `self.depth_resize = (h, w)` (the reference: (384, 384)) the call
        is the reference's: the frames are resized to h x w (`prepare_midas_input`, one bicubic launch), the estimator may answer
        [b t, 1, H', W'] at any size, and its answer is resized to `target_size` (multiples of 8) and normalised by ONE program (a
        bicubic pass into the arena + the front-end kernel; no resize when the answer already has target_size) — bit for bit
        `adapter.normalise_depth(bicubic_resize(d, target_size))`.  With `depth_resize = None` (the default) the estimator is called on
        the frames as they are and must return [b t, 1, H, W] at `target_size` already.  Alternatively pass
        the depth itself, `get_batch_depth(depth=d)` with d [b, 1, t, H, W]: only the normalisation runs (the front-end kernel)."""
        resize = getattr(self, "depth_resize", None) if depth is None else None
        if depth is None:
            if self.depth_stage_model is None:
                raise RuntimeError("no depth_stage_model attached: pass depth=[b, 1, t, H, W] instead")
            b, _, t, _, _ = batch_x.shape
            merged = batch_x.permute(0, 2, 1, 3, 4).reshape(b * t, batch_x.shape[1], batch_x.shape[3], batch_x.shape[4])
            d = self.depth_stage_model(merged if resize is None else bicubic_resize(merged, resize))
        else:
            if depth.dim() != 5 or depth.shape[1] != 1:
                raise ValueError(f"depth must be [b, 1, t, H, W], got {tuple(depth.shape)}")
            b, _, t, _, _ = depth.shape
            d = depth.permute(0, 2, 1, 3, 4).reshape(b * t, 1, depth.shape[3], depth.shape[4])
        if d.dim() != 4 or d.shape[0] != b * t or d.shape[1] != 1:
            raise ValueError(f"the depth model must return [{b * t}, 1, H, W], got {tuple(d.shape)}")
        if resize is not None:
            H, W = (int(v) for v in (target_size if target_size is not None else d.shape[2:]))
            if H % 8 or W % 8 or min(H, W) < 8:
                raise ValueError(f"target_size {(H, W)}: the adapter's PixelUnshuffle(8) front end needs multiples of 8")
            out = self.adapter.normalise_depth(d, size=(H, W))
            return out.reshape(b, t, 1, H, W).permute(0, 2, 1, 3, 4).contiguous()
        if target_size is not None and tuple(d.shape[2:]) != tuple(target_size):
            raise ValueError(f"depth maps of {tuple(d.shape[2:])} for target_size {tuple(target_size)}: with depth_resize = None nothing is "
                             "resized — depth must arrive at target_size (set depth_resize = (h, w), the reference: (384, 384), for the bicubic "
                             "resizes around the depth model)")
        out = self.adapter.normalise_depth(d)
        return out.reshape(b, t, 1, d.shape[2], d.shape[3]).permute(0, 2, 1, 3, 4).contiguous()

    @torch.no_grad()
    def get_adapter_features(self, extra_cond, encode_bs=1):
        """extra_cond [b, 1, t, h, w] -> list of [b, c_i, t, h_i, w_i] (ddpm3d.py:1471-1484).  The reference runs the adapter frame
        by frame (`encode_bs`); here ONE program covers all b t frames — the results are per frame either way.  The returned tensors
        are views of channels-last storage, the layout UNetModel's injection reads without a copy."""
        b, c, t, h, w = extra_cond.shape
        feats = self.adapter(extra_cond.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w))
        return [f.reshape(b, t, *f.shape[1:]).permute(0, 2, 1, 3, 4) for f in feats]


# ------------------------------------------------------------------------------------------
# DDIM sampler (lvdm/samplers/ddim.py)
# ------------------------------------------------------------------------------------------
class DDIMSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.counter = 0
        self.noise_gen = torch.Generator(device="cpu")      # seeded by process_videocrafter.py:70
        # one CPU generator per video of the batch (None: the single `noise_gen` above for the whole batch).  Video v's per-step noise
        # is then torch.randn((1, *shape[1:]), generator=noise_gens[v]): the stream a batch-of-one run seeded like noise_gens[v] draws,
        # which is what lets `process_videocrafter` make the reference's batch_count videos in one batch
        self.noise_gens = None

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        """ddim.py:24-53 with make_ddim_timesteps / make_ddim_sampling_parameters (util.py:36-63) on fp32 cumprods."""
        if ddim_discretize != "uniform":
            raise NotImplementedError(ddim_discretize)
        T = self.ddpm_num_timesteps
        self.ddim_timesteps = np.asarray(list(range(0, T, T // ddim_num_steps))) + 1
        ac = self.model.alphas_cumprod.detach().cpu()
        assert ac.shape[0] == T, "alphas have to be defined for each timestep"
        alphas = ac[self.ddim_timesteps]
        alphas_prev = torch.cat([ac[0:1], ac[self.ddim_timesteps[:-1]]])
        a64, p64 = alphas.double(), alphas_prev.double()        # (util.py:52-63 does this in numpy float64 on the fp32 values)
        self.ddim_sigmas = ddim_eta * torch.sqrt((1 - p64) / (1 - a64) * (1 - a64 / p64))
        self.ddim_alphas, self.ddim_alphas_prev = alphas, alphas_prev
        self.ddim_sqrt_one_minus_alphas = torch.sqrt(1.0 - alphas)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, img_callback=None, quantize_x0=False, eta=0.0,
               mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None,
               verbose=True, schedule_verbose=False, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, postprocess_fn=None, sample_noise=None, cond_fn=None, **kwargs):
        """ddim.py:56-132 -> (samples, intermediates)."""
        if quantize_x0 or noise_dropout or score_corrector is not None or postprocess_fn is not None \
                or cond_fn is not None or kwargs.get("uc_type") is not None:
            raise NotImplementedError("quantisation / noise dropout / score correctors are not on the hot path")
        if kwargs.get("freeu") is not None:
            raise NotImplementedError("freeu: FreeU is implemented for the ModelScope UNet only, not for the VideoCrafter path (UNetModel)")
        if kwargs.get("context_windows") is not None:
            raise L.T2VError("context_windows: context windows exist for the ModelScope samplers only; the VideoCrafter loop evaluates "
                             "through LatentDiffusion.apply_model and is out of scope")
        size = (batch_size, *shape)
        assert len(size) == 5
        if mask is not None:
            # mask blending (ddim.py:188-195): img = q_sample(x0, step - 1) * mask + (1 - mask) * img after every step.  The mask is
            # 5-D and broadcastable to the latent, [b|1, c|1, t|1, h|1, w|1], any float values; a mask of another rank would
            # broadcast from the right (a 1-D one along the width) and is refused
            if not isinstance(mask, torch.Tensor) or mask.dim() != 5:
                raise NotImplementedError("mask blending needs a 5-D mask [b|1, c|1, t|1, h|1, w|1]; masks of another rank are not on the hot path")
            if x0 is None:
                raise ValueError("mask needs x0: the known latent that the masked region is held to")
            if any(m not in (1, s) for m, s in zip(mask.shape, size)):
                raise ValueError(f"mask {tuple(mask.shape)} does not broadcast to the latent {size}")
            if not isinstance(x0, torch.Tensor) or tuple(x0.shape) != size:
                raise ValueError(f"x0 must have the latent's shape {size}, got {tuple(getattr(x0, 'shape', ()))}")
        # features_adapter: forwarded to every apply_model call (ddim.py:221-229 passes its **kwargs on for both evaluations of a
        # guided step); temporal_length: accepted and ignored, as in the reference (ddim.py:80: the shape carries the length)
        if kwargs.get("conditional_guidance_scale_temporal") is not None:
            raise NotImplementedError("conditional_guidance_scale_temporal (temporal guidance) is not on the hot path")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=schedule_verbose)
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback, temperature=temperature,
                                  x_T=x_T, log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, sample_noise=sample_noise, verbose=verbose,
                                  features_adapter=kwargs.get("features_adapter"), mask=mask, x0=x0 if mask is not None else None)

    @staticmethod
    def _ctx(c):
        if isinstance(c, dict):
            return torch.cat(c["c_crossattn"], 1)
        if isinstance(c, list):
            return torch.cat(c, 1)
        return c

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, callback=None, img_callback=None, log_every_t=100, temperature=1.0,
                      unconditional_guidance_scale=1.0, unconditional_conditioning=None, sample_noise=None, verbose=True,
                      features_adapter=None, mask=None, x0=None, **kw):
        """ddim.py:135-206, p_sample_ddim :209-279 fused into one kernel launch per step (T2V_OP_DDIM_STEP mode 1).  With a mask
        (5-D, broadcastable to `shape`; x0 of `shape`) the blend of :188-195 rides in the same launch (i[7] = 1)."""
        from . import samplers as S
        device = self.model.betas.device
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device)
        img = img.float().contiguous().clone()
        timesteps = self.ddim_timesteps
        total_steps = timesteps.shape[0]
        intermediates = {"x_inter": [img.clone()], "pred_x0": [img.clone()]}
        c, uc = self._ctx(cond), self._ctx(unconditional_conditioning) if unconditional_conditioning is not None else None
        guide = unconditional_guidance_scale
        guided = uc is not None and guide != 1.0
        unet = self.model.model.diffusion_model
        nxt = torch.empty_like(img)
        extra = {} if features_adapter is None else {"features_adapter": features_adapter}     # the same list object every step: converted once
        nb, C = img.shape[0], img.shape[1]          # nb videos per batch (sample_text2video's batch_size)
        gens = getattr(self, "noise_gens", None)
        if gens is not None and len(gens) != nb:
            raise ValueError(f"noise_gens holds {len(gens)} generators for a batch of {nb}: one per video")
        f32 = torch.float32
        if mask is not None:                        # expanded once per call: the kernel reads x0, mask and q-noise dense, like x
            known = x0.to(device=device, dtype=f32).contiguous()
            mask_d = mask.to(device=device, dtype=f32).expand(img.shape).contiguous()
            q_a, q_s = self.model.sqrt_alphas_cumprod.detach().cpu(), self.model.sqrt_one_minus_alphas_cumprod.detach().cpu()
        S.state.sampling_steps = total_steps
        iterator = np.flip(timesteps)
        if verbose and S.tqdm is not None:
            iterator = S.tqdm(iterator, desc="DDIM Sampler", total=total_steps)
        # (a LoRA merged the reference's way, `weight.data += ...`, moves no version counter: the guard verifies the bytes)
        with S._sampling_run(unet, device):
            for i, step in enumerate(iterator):
                S.state.sampling_step = i
                if S.state.interrupted:
                    raise S.InterruptedException
                index = total_steps - i - 1
                ts = torch.full((nb,), int(step), device=device, dtype=torch.long)
                if guided:
                    # ONE x_t for the [cond | uncond] pair (the reference builds torch.cat([x] * 2), lvdm/samplers/ddim.py:206-209): the
                    # entry op reads it for both samples, and with UNetSD.share_cfg_prefix every op up to the first text
                    # cross-attention is computed once
                    xin = img if hasattr(unet, "share_cfg_prefix") else torch.cat([img, img])      # (a foreign model gets the reference's batch)
                    if hasattr(unet, "single_timestep"):
                        unet.single_timestep = True        # [ts | ts]: one timestep for the pair -> the prefix may be shared
                    eps = self.model.apply_model(xin, torch.cat([ts, ts]), torch.cat([c, uc]), **extra).contiguous()
                else:
                    eps = self.model.apply_model(img, ts, c, **extra).contiguous()
                coef = S._ddim_coef(self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sigmas, self.ddim_sqrt_one_minus_alphas, index,
                                    guide if guided else None)
                coef[4] = coef[4] * float(temperature)        # in double, rounded to fp32 when the record stores it
                if sample_noise is not None:
                    noise = sample_noise.to(device=device, dtype=f32).contiguous()
                elif gens is None:            # noise_like(..., noise_gen): CPU generator -> same stream on any device
                    noise = torch.randn(tuple(img.shape), generator=self.noise_gen).to(device)
                else:                         # one stream per video, each drawn as a batch of one
                    noise = torch.cat([torch.randn((1, *img.shape[1:]), generator=g) for g in gens]).to(device)
                want_x0 = img_callback is not None or index % log_every_t == 0 or index == total_steps - 1
                if want_x0:                   # pred_x0 = (x - sqrt(1-a_t) e) / sqrt(a_t), e = u + g (c - u)
                    px0 = torch.empty_like(img)
                    ia = 1.0 / coef[1]
                    if guided:
                        g = float(guide)
                        S._lincomb(px0, [(ia, img), (-coef[0] * g * ia, eps[0:nb]), (-coef[0] * (1.0 - g) * ia, eps[nb:2 * nb])])
                    else:
                        S._lincomb(px0, [(ia, img), (-coef[0] * ia, eps[0:nb])])
                if mask is None:
                    S._ddim_update(nxt, img, eps, noise, coef, C if guided else 0, mode=1)
                else:
                    # q_sample(x0, step - 1) (ddim.py:193-194): its noise is `randn_like(x0)` on the default generator, drawn after
                    # the UNet forward — from the CPU generator here, the same stream on any device
                    qnoise = torch.randn(tuple(known.shape)).to(device)
                    tq = int(step) - 1
                    qcoef = (float(q_a[tq]), float(q_s[tq]))
                    S._ddim_update_blend(nxt, img, eps, noise, coef, C if guided else 0, known, mask_d, qnoise, qcoef)
                img, nxt = nxt, img
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(px0, i)
                if index % log_every_t == 0 or index == total_steps - 1:
                    intermediates["x_inter"].append(img.clone())
                    intermediates["pred_x0"].append(px0)
                if S.state.skipped:
                    break
        return img, intermediates


# ------------------------------------------------------------------------------------------
# merged LoRA (lvdm/models/modules/lora.py:620-755)
# ------------------------------------------------------------------------------------------
def _lora_resolve(net, state_dict):
    """First half of the reference's loop, for ALL keys before any weight is touched: -> ([(key, layer, up, down)], visited keys).
    Keys with '.alpha' are skipped unread; the target is reached from `net` by the names of key.split('.')[:-2] (module children, so
    ModuleList / Sequential indices too); a target whose class is not exactly nn.Linear / nn.Conv2d prints 'missing param at:' and is
    skipped; the partner key swaps lora_down <-> lora_up and a pair is taken once, at whichever key comes first.  A name that does not
    resolve, a missing partner or factors that do not fit the weight raise T2VError naming the key (the reference dies half-merged)."""
    visited, todo = [], []
    for key in state_dict:
        if ".alpha" in key or key in visited:
            continue
        names = key.split(".")[:-2]
        if not names:
            raise L.T2VError(f"LoRA key {key!r} names no layer")
        layer = net
        for k, name in enumerate(names):
            try:
                if not isinstance(layer, nn.Module):
                    raise AttributeError(name)
                layer = nn.Module.__getattr__(layer, name)
            except AttributeError:
                where = ".".join(names[:k]) or "the model"
                raise L.T2VError(f"LoRA key {key!r} cannot be resolved: {where} ({type(layer).__name__}) has no module {name!r}; "
                                 "no weight was changed") from None
        if layer.__class__ not in [nn.Linear, nn.Conv2d]:
            print("missing param at:", key)
            continue
        if "lora_down" in key:
            pair = [key.replace("lora_down", "lora_up"), key]
        else:
            pair = [key, key.replace("lora_up", "lora_down")]
        for k in pair:
            if k not in state_dict:
                raise L.T2VError(f"LoRA key {key!r} has no partner {k!r}; no weight was changed")
        up, down = state_dict[pair[0]], state_dict[pair[1]]
        if len(up.shape) == 4:
            up, down = up.squeeze(3).squeeze(2), down.squeeze(3).squeeze(2)
        w = layer.weight
        if (len(state_dict[pair[0]].shape) == 4) != (w.dim() == 4):      # (the reference picks the conv form by the FACTORS' rank)
            raise L.T2VError(f"LoRA key {key!r}: {len(state_dict[pair[0]].shape)}-D factors for a {w.dim()}-D weight; no weight was changed")
        if up.dim() != 2 or down.dim() != 2 or up.shape[1] != down.shape[0] or (up.shape[0], down.shape[1]) != tuple(w.shape[:2]):
            raise L.T2VError(f"LoRA key {key!r}: factors {tuple(up.shape)} x {tuple(down.shape)} do not fit the weight {tuple(w.shape)}; "
                             "no weight was changed")
        todo.append((key, layer, up, down))
        visited.extend(pair)
    return todo, visited


def _lora_load(checkpoint_path, device):
    state_dict = torch.load(checkpoint_path)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in state_dict.items()}


def _lora_delta(layer, up, down, alpha):
    delta = alpha * torch.mm(up.to(torch.float32), down.to(torch.float32))
    return delta.unsqueeze(2).unsqueeze(3) if layer.weight.dim() == 4 else delta      # a k x k kernel receives it on every tap (broadcast)


@torch.no_grad()
def net_load_lora(net, checkpoint_path, alpha=1.0, remove=False):
    """lora.py:620-672: merge (remove=True: subtract) the LoRA file's `alpha * up @ down` into the Linear / Conv2d weights it names,
    in the parameter's own dtype.  Two differences from the reference: every key is resolved before any weight changes (`_lora_resolve`),
    and the weights are written with in-place ops on the parameter instead of through `.data` — the same bytes, but the version counter
    moves, so the next `refresh_weights` re-packs exactly the images that read the touched tensors."""
    state_dict = _lora_load(checkpoint_path, net.device)
    todo, visited = _lora_resolve(net, state_dict)
    for key, layer, up, down in todo:
        delta = _lora_delta(layer, up, down, alpha)
        if remove:
            layer.weight.sub_(delta)
        else:
            layer.weight.add_(delta)
    print("load_weight_num:", len(visited))
    return


def change_lora(model, inject_lora=False, lora_scale=1.0, lora_path='', last_time_lora='', last_time_lora_scale=1.0):
    """lora.py:674-680: take the previous LoRA out (at its scale), then put the new one in."""
    if last_time_lora != '':
        net_load_lora(model, last_time_lora, alpha=last_time_lora_scale, remove=True)
    if inject_lora:
        net_load_lora(model, lora_path, alpha=lora_scale)


@torch.no_grad()
def net_load_lora_v2(net, checkpoint_path, alpha=1.0, remove=False, origin_weight=None):
    """lora.py:683-746: like `net_load_lora`, but the weight of every target is cloned into `origin_weight` (under the key with
    lora_down / lora_up replaced by 'lora') the first time it is touched, and remove=True restores the clone.  -> origin_weight."""
    state_dict = _lora_load(checkpoint_path, net.device)
    todo, visited = _lora_resolve(net, state_dict)
    for key, layer, up, down in todo:
        if origin_weight is None:
            origin_weight = dict()
        storage_key = key.replace("lora_down", "lora").replace("lora_up", "lora")
        if storage_key not in origin_weight.keys():
            origin_weight[storage_key] = layer.weight.detach().clone()
        if remove:
            layer.weight.copy_(origin_weight[storage_key])
        else:
            layer.weight.add_(_lora_delta(layer, up, down, alpha))
    print("load_weight_num:", len(visited))
    return origin_weight


def change_lora_v2(model, inject_lora=False, lora_scale=1.0, lora_path='', last_time_lora='', last_time_lora_scale=1.0, origin_weight=None):
    """lora.py:748-755."""
    if last_time_lora != '':
        origin_weight = net_load_lora_v2(model, last_time_lora, alpha=last_time_lora_scale, remove=True, origin_weight=origin_weight)
    if inject_lora:
        origin_weight = net_load_lora_v2(model, lora_path, alpha=lora_scale, origin_weight=origin_weight)
    return origin_weight


# ------------------------------------------------------------------------------------------
# entry point (videocrafter/sample_text2video.py:92-152, sample_utils.py)
# ------------------------------------------------------------------------------------------
def get_conditions(prompts, model, batch_size):
    if isinstance(prompts, (str, int)):
        prompts = [prompts]
    if len(prompts) == 1:
        prompts = prompts * batch_size
    assert len(prompts) == batch_size, f"invalid prompts length: {len(prompts)}"
    return {"c_crossattn": [model.get_learned_conditioning(prompts)]}


def make_model_input_shape(model, batch_size, T=None):
    image_size = [model.image_size, model.image_size] if isinstance(model.image_size, int) else list(model.image_size)
    unet = model.model.diffusion_model
    return [batch_size, unet.in_channels, unet.temporal_length if T is None else T, *image_size]


def torch_to_np(x):
    """sample_utils.py:104-114: ((x + 1) * 127.5).clamp(0, 255) -> uint8, channels last."""
    sample = ((x.detach().float().cpu() + 1) * 127.5).clamp(0, 255).to(torch.uint8)
    return (sample.permute(0, 2, 3, 4, 1) if sample.dim() == 5 else sample.permute(0, 2, 3, 1)).contiguous()


def torch_to_np_device(x):
    """`torch_to_np` of a float video that is on the device, there: [b, c, t, h, w] -> uint8 [b, t, h, w, c] (or [b, c, h, w] ->
    [b, h, w, c]) with ONE T2V_OP_TO_UINT8 launch of form 1 — (x + 1) * 127.5 in fp32, clamped to [0, 255], truncated.  Bit-exact with
    `torch_to_np` for the same input (a NaN aside: torch's cast of it is undefined, the kernel stores 0).  The counterpart of
    `pipeline.tensor2vid_device`; a decoded latent never needs it: `LatentDiffusion.decode_first_stage_uint8`."""
    import ctypes
    if not x.is_cuda:
        raise L.T2VError("torch_to_np_device needs a device tensor on an AMD GPU (no CPU fallback)")
    if x.dim() not in (4, 5):
        raise ValueError(f"expected [b, c, t, h, w] or [b, c, h, w], got {tuple(x.shape)}")
    if x.dtype not in (torch.float16, torch.float32):
        x = x.float()
    v = (x if x.dim() == 5 else x.unsqueeze(2)).contiguous()
    NI, C, Fr, H, W = v.shape
    out = torch.empty((NI, Fr, H, W, C), dtype=torch.uint8, device=v.device)
    op = L.T2VOp()
    op.kind = L.OP_TO_UINT8
    half = v.dtype == torch.float16
    si, sc, sf, sy, sx = C * Fr * H * W, Fr * H * W, H * W, W, 1
    if sc >= 2 ** 31 or not 1 <= C <= 4:
        raise L.T2VError("video too large for one uint8 conversion launch (or more than 4 channels)")
    vals = [NI, C, Fr, H, W, L.F16 if half else L.F32, 0, 0, si & 0xFFFFFFFF, si >> 32, sc, sf & 0xFFFFFFFF, sf >> 32, sy, sx, 1]
    for k, val in enumerate(vals):
        op.i[k] = val - (1 << 32) if val >= (1 << 31) else val       # low words as raw bits
    op.p[0], op.p[1] = v.data_ptr(), out.data_ptr()
    L.check(L.load().t2v_run_ops(ctypes.byref(op), 1, None, 0, ctypes.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)))
    return out if x.dim() == 5 else out[:, 0]


@torch.no_grad()
def sample_text2video(model, prompt, n_prompt, n_samples, batch_size, sample_type="ddim", sampler=None, ddim_steps=50, eta=1.0,
                      cfg_scale=7.5, decode_frame_bs=1, ddp=False, all_gather=True, batch_progress=True,
                      show_denoising_progress=False, num_frames=None, *, mask=None, x0=None, init_video=None, device_uint8=False):
    """-> np.uint8 [n, T, H, W, 3].  `decode_frame_bs=None` decodes all frames in one VAE launch sequence.
    device_uint8 (not in the reference's signature): the frames leave the decoder programs as uint8 (`decode_first_stage_uint8`, same
    `decode_frame_bs` chunks) — the same array, a quarter (fp32 weights) or half (fp16) of the bytes copied to the host.
    mask / x0 (not in the reference's signature): held regions, as `DDIMSampler.sample` takes them, applied to every batch;
    init_video [b, 3, t, H, W] in [-1, 1] is encoded with `encode_first_stage_2DAE` and stands in for x0."""
    if sample_type != "ddim" or sampler is None:
        raise NotImplementedError("only the DDIM path of the webui (process_videocrafter.py:57-79) is built")
    if init_video is not None:
        if x0 is not None:
            raise ValueError("give x0 (a latent) or init_video (frames to encode), not both")
        x0 = model.encode_first_stage_2DAE(init_video.to(model.device))
    cond = get_conditions(prompt, model, batch_size)
    uncond = get_conditions(n_prompt, model, batch_size) if cfg_scale != 1.0 else None
    videos = []
    for _ in range(math.ceil(n_samples / batch_size)):
        noise_shape = make_model_input_shape(model, batch_size, T=num_frames)
        latent, _ = sampler.sample(S=ddim_steps, conditioning=cond, batch_size=noise_shape[0], shape=noise_shape[1:],
                                   verbose=show_denoising_progress, unconditional_guidance_scale=cfg_scale,
                                   unconditional_conditioning=uncond, eta=eta, mask=mask, x0=x0)
        if device_uint8:
            videos.append(model.decode_first_stage_uint8(latent, decode_bs=decode_frame_bs).numpy())
            continue
        samples = model.decode_first_stage(latent, decode_bs=decode_frame_bs, return_cpu=False)
        videos.append(torch_to_np(samples).numpy())
    out = np.concatenate(videos, axis=0)
    assert out.shape[0] >= n_samples
    return out


def process_videocrafter(args_dict: dict):
    """The driver of the VideoCrafter route (process_videocrafter.py:12-98), the counterpart of `pipeline.process_modelscope`.  The
    reference body is config / checkpoint loading and mp4 plumbing around a `batch_count` loop of single-video `sample_text2video`
    calls (:55-98).  Here:
      args_dict = {model (a LatentDiffusion), sampler (a DDIMSampler; one is made when absent),
                   prompt, n_prompt, steps, frames, seed, cfg_scale, eta, batch_count, fps,
                   stitch, one_pass (True), decode_frame_bs (1, what the reference passes)}
    * `width` / `height` are ignored as in the reference: the model's `image_size` rules.  `sample_type` other than "ddim" is refused
      like `sample_text2video` refuses it; masks and init videos are `sample_text2video`'s, not this seam's.
    * loop route (`one_pass=False` or one video), the reference's loop: video b from `noise_gen.manual_seed(seed + b)` (seed -1: -1 for
      every video, the reference's own quirk), `sample_text2video(model, prompt, n_prompt, 1, 1, ...)`, with `state.job_count` /
      `job_no` / `job`, the `skipped` reset and the break on `interrupted`.
    * one pass (default for batch_count > 1): the conditions once, x_T = the batch_count device draws of one video's shape that the
      loop would make, in its order, `sampler.noise_gens[v]` seeded seed + v, ONE `sampler.sample` of batch batch_count and ONE
      `decode_first_stage_uint8` — the loop's videos up to what a larger batch changes in the GEMM tiling.
    * either way the frames leave the decoder programs as uint8.
    * no `stitch`: returns the list of batch_count videos, uint8 [T, H, W, 3] RGB (fewer after an interrupt).
      `stitch(frames, fps) -> bytes` (mp4 writing, out of scope: the reference's `npz_to_video_grid` and its soundtrack stage) given:
      every video is handed to it and the reference's own return value comes back, `[dataurl]` of the LAST video only (:92-98)."""
    from . import samplers as S
    a = SimpleNamespace(**args_dict)
    model = a.model
    if getattr(a, "sample_type", "ddim") != "ddim":
        raise NotImplementedError("only the DDIM path of the webui (process_videocrafter.py:57-79) is built")
    if getattr(a, "freeu", None) is not None:
        raise NotImplementedError("freeu: FreeU is implemented for the ModelScope UNet only, not for the VideoCrafter path (process_videocrafter)")
    sampler = getattr(a, "sampler", None)
    if sampler is None:
        sampler = DDIMSampler(model)
    batch_count = int(getattr(a, "batch_count", 1))
    n_prompt, eta, cfg_scale = getattr(a, "n_prompt", ""), getattr(a, "eta", 1.0), getattr(a, "cfg_scale", 7.5)
    stitch, fps = getattr(a, "stitch", None), getattr(a, "fps", None)
    decode_frame_bs = getattr(a, "decode_frame_bs", 1)
    frames = getattr(a, "frames", None)
    state = S.state
    state.job_count = batch_count
    videos, urls = [], []

    def emit(vid):            # (the reference writes and reads back vid.mp4 inside its loop, :85-93)
        videos.append(vid)
        if stitch is not None:
            urls[:] = ["data:video/mp4;base64," + b64encode(stitch(vid, fps)).decode()]

    if batch_count > 1 and getattr(a, "one_pass", True):
        state.job_no = 1
        if state.skipped:
            state.skipped = False
        if not state.interrupted:
            state.job = f"Batches 1-{batch_count} out of {batch_count}"
            cond = get_conditions(a.prompt, model, 1)["c_crossattn"][0]
            cond = {"c_crossattn": [cond.repeat(batch_count, *([1] * (cond.dim() - 1)))]}
            uncond = None
            if cfg_scale != 1.0:
                uncond = get_conditions(n_prompt, model, 1)["c_crossattn"][0]
                uncond = {"c_crossattn": [uncond.repeat(batch_count, *([1] * (uncond.dim() - 1)))]}
            shape = make_model_input_shape(model, 1, T=frames)
            x_T = torch.cat([torch.randn(tuple(shape), device=model.device) for _ in range(batch_count)])
            gens = [torch.Generator(device="cpu") for _ in range(batch_count)]
            for v, g in enumerate(gens):
                g.manual_seed(a.seed + v if a.seed != -1 else -1)
            prev, sampler.noise_gens = getattr(sampler, "noise_gens", None), gens
            try:
                latent, _ = sampler.sample(S=a.steps, conditioning=cond, batch_size=batch_count, shape=shape[1:], verbose=False,
                                           unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uncond, eta=eta, x_T=x_T)
            finally:
                sampler.noise_gens = prev
            u8 = model.decode_first_stage_uint8(latent, decode_bs=decode_frame_bs).numpy()
            for v in range(batch_count):
                emit(u8[v])
            state.job_no = batch_count
    else:
        for batch in range(batch_count):
            state.job_no = batch + 1
            if state.skipped:
                state.skipped = False
            if state.interrupted:
                break
            state.job = f"Batch {batch + 1} out of {batch_count}"
            sampler.noise_gen.manual_seed(a.seed + batch if a.seed != -1 else -1)
            samples = sample_text2video(model, a.prompt, n_prompt, 1, 1, "ddim", sampler, a.steps, eta, cfg_scale, decode_frame_bs,
                                        num_frames=frames, device_uint8=True)
            emit(samples[0])
    return videos if stitch is None else urls


@torch.no_grad()
def adapter_guided_synthesis(model, prompts, videos, noise_shape, n_samples=1, ddim_steps=50, ddim_eta=1.,
                             unconditional_guidance_scale=1.0, unconditional_guidance_scale_temporal=None, sampler=None, depth=None,
                             **kwargs):
    """videocrafter/sample_text2video_adapter.py:96-137: depth of `videos` [b, 3, t, h, w] -> adapter features -> DDIM with the
    features at every step -> decoded clips.  -> (batch_variants [b, n_samples, c, t, H, W], extra_cond [b, 1, t, h, w]).
    `model`: a T2VAdapterDepth.  sampler: a DDIMSampler to use (e.g. with a seeded `noise_gen`), as `sample_text2video` takes one;
    default a fresh one.  depth [b, 1, t, h, w]: the depth clip itself instead of `videos` + the model's depth estimator."""
    ddim_sampler = DDIMSampler(model) if sampler is None else sampler
    batch_size = noise_shape[0]
    if isinstance(prompts, str):
        prompts = [prompts]
    cond = model.get_learned_conditioning(prompts)
    uc = model.get_learned_conditioning(batch_size * [""]) if unconditional_guidance_scale != 1.0 else None
    if depth is not None:
        extra_cond = model.get_batch_depth(depth=depth)
    else:
        b, c, t, h, w = videos.shape
        extra_cond = model.get_batch_depth(videos, (h, w))
    features_adapter = model.get_adapter_features(extra_cond)
    batch_variants = []
    for _ in range(n_samples):
        samples, _ = ddim_sampler.sample(S=ddim_steps, conditioning=cond, batch_size=noise_shape[0], shape=noise_shape[1:], verbose=False,
                                         unconditional_guidance_scale=unconditional_guidance_scale, unconditional_conditioning=uc,
                                         eta=ddim_eta, temporal_length=noise_shape[2],
                                         conditional_guidance_scale_temporal=unconditional_guidance_scale_temporal,
                                         features_adapter=features_adapter, **kwargs)
        batch_variants.append(model.decode_first_stage(samples, decode_bs=1, return_cpu=False))
    batch_variants = torch.stack(batch_variants)
    return batch_variants.permute(1, 0, 2, 3, 4, 5), extra_cond
