"""What the lowerings share.  `_Declarations`: the program, the weight packer and the packed-weight recipes every network declares
(unet, videocrafter, vae).  `_UNetLowering`: the skeleton of a denoising UNet's program — step-level prologue, entry, the block list with
its skip-connection concats, head — and the building blocks the ModelScope (unet._Lowering) and LVDM (videocrafter._LvdmLowering)
UNets have in common.  What differs between the two networks is a method the subclass overrides or an argument its caller passes."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import _lib as L
from . import packing as pk
from .program import Buf, Program, Ref, TShardSpec


class _Declarations:
    def __init__(self, label: str, keep_taps: bool = False):
        self.P = Program(label)
        self.P.keep_taps = keep_taps
        self.packer = pk.WeightPacker()

    def w_linear(self, key) -> Ref:
        return Ref("weight", 0, self.packer.add(key + ":lin", "f16", lambda sd, k=key: pk.pad_rows(pk.linear(sd[k + ".weight"]))))

    def conv3_kernel(self, key) -> Tuple[Callable, str]:
        """(state dict -> the [Cout, Cin, 3, 3] kernel of the convolution `key`, suffix of its packed images' names)."""
        return (lambda sd, k=key: sd[k + ".weight"]), ":c3"

    def w_conv3(self, key, cin_pad=0, form="") -> Ref:
        """form "": plain (input channels padded to `cin_pad`); "d": the 4 input channels repeated in the 4 padding channels of the
        8-channel token rows (precise_operands stem); "hl": for an operand of 2 Cin channels = [hi (Cin) | lo (Cin)], [W | W] along
        the input channels."""
        kernel, suffix = self.conv3_kernel(key)
        pack = {"": lambda w: pk.conv3x3(w, cin_pad), "d": pk.conv3x3_c8_dup, "hl": lambda w: pk.conv3x3(torch.cat([w] * 2, dim=1))}[form]
        return Ref("weight", 0, self.packer.add(key + suffix + form, "f16", lambda sd: pk.pad_rows(pack(kernel(sd)))))

    def vec(self, key) -> Ref:
        """fp32 vector (bias / norm affine), zero-padded to a multiple of 4."""
        return Ref("weight", 0, self.packer.add(key + ":v", "f32", lambda sd, k=key: pk.pad_rows(sd[k])))

    def _dest(self, dest: Optional[Buf], rows, cols, dtype) -> Buf:
        if dest is None:
            return self.P.alloc(rows, cols, dtype)
        assert (dest.rows, dest.cols, dest.dtype) == (rows, cols, dtype), (dest, rows, cols, dtype)
        return dest


def canonical_context_lengths(Lctx, B: int):
    """The one form of a batch's context lengths (it is part of the program key): an int where every sample has that length, the pair
    (Lc, Lu) where the first half of an even batch has Lc and the second half Lu, else the tuple of B lengths."""
    if not isinstance(Lctx, (tuple, list)):
        return int(Lctx)
    lens = tuple(int(v) for v in Lctx)
    if len(lens) == 2 and B != 2:
        return lens[0] if lens[0] == lens[1] else lens
    assert len(lens) == B, f"{len(lens)} context lengths for a batch of {B} samples"
    if len(set(lens)) == 1:
        return lens[0]
    if B % 2 == 0 and len(set(lens[: B // 2])) == 1 and len(set(lens[B // 2:])) == 1:
        return (lens[0], lens[-1])
    return lens


class _UNetLowering(_Declarations):
    head_per_frame = True          # statistics of the head's GroupNorm: per frame, or over all frames of a sample

    def __init__(self, net, B, F, H, W, Lctx, x_dt, out_dt, ctx_dt, keep_taps=False, shard=None, x_batch=0):
        """F = frames held by THIS rank.  shard = TShardSpec: the clip's frames are split contiguously over the ranks
        of a T group (slices of ceil(F_total / R) frames, a shorter last one); temporal ops then exchange data
        (SURVEY §5.7): cross-frame GroupNorm -> all-gather of statistics partials, temporal conv -> +-1 frame halo,
        temporal attention -> all-gather of K/V.  Everything else is frame-local.
        Lctx: the context length of every sample, or a pair (Lc, Lu) — the first B / 2 samples (cond) have Lc context rows each, the
        others (uncond) Lu; the context then arrives packed, B / 2 * Lc rows followed by B / 2 * Lu rows.  Equal lengths are the int.
        Or a tuple of B lengths, one per sample (a batch of different prompts): the context arrives packed in batch order, sum(Lctx)
        rows, and every text cross-attention carries a per-sample table.  Lengths that the int or the pair describes ARE the int or
        the pair (`canonical_context_lengths`): the program is then the one those forms compile to."""
        super().__init__(f"unet b{B} f{F} {H}x{W}", keep_taps)
        self.Lpair: Optional[Tuple[int, int]] = None
        self.Lsamples: Optional[Tuple[int, ...]] = None
        Lctx = canonical_context_lengths(Lctx, B)
        if isinstance(Lctx, tuple) and len(Lctx) == 2:          # (two samples with their own lengths are the pair too)
            Lc, Lu = Lctx
            if shard is not None and shard.size > 1:
                raise L.T2VError(f"a T-sharded forward takes one context length for cond and uncond, got {Lc} and {Lu}")
            assert B % 2 == 0, "a pair of context lengths describes a [cond | uncond] batch"
            self.Lpair, Lctx = (Lc, Lu), max(Lc, Lu)
        elif isinstance(Lctx, tuple):
            if shard is not None and shard.size > 1:
                raise L.T2VError(f"a T-sharded forward takes one context length for every sample, got {list(Lctx)}")
            self.Lsamples, Lctx = Lctx, max(Lctx)
        # rows of the text context (and of its K / V projections) over the whole batch
        self.ctx_rows = B * Lctx if self.Lpair is None else B // 2 * sum(self.Lpair)
        if self.Lsamples is not None:
            self.ctx_rows = sum(self.Lsamples)
        self.shard: Optional[TShardSpec] = shard if (shard is not None and shard.size > 1) else None
        if self.shard is not None:
            assert B == 1, "T-sharded forwards run one sample per rank (the CFG pair is split over ranks)"
            assert F == self.shard.frames
        self.net, self.B, self.F, self.H, self.W, self.Lctx = net, B, F, H, W, Lctx
        # cond | uncond prefix sharing (UNetSD.share_cfg_prefix): while `sharing`, activations hold Bc = 1 sample; the first spatial
        # transformer's text cross-attention is where the two samples part (text_cross_attention) and Bc becomes B
        # (`_share_now`: forward() sets it from `share_cfg_prefix` AND the single-timestep hint; a direct _compile keeps the attribute's value)
        self.sharing = bool(getattr(net, "_share_now", False)) and B == 2 and x_batch == 1 and self.shard is None
        self.Bc = 1 if self.sharing else B
        self.x_dt, self.out_dt, self.ctx_dt = x_dt, out_dt, ctx_dt
        self.x_batch = x_batch if 0 < x_batch < B else 0      # x holds fewer samples than the batch: sample b reads x[b % x_batch]
        self.precise = bool(getattr(net, "precise_operands", False))
        # round 4: the two next classes of the operand ranking (DESIGN.md "Precision") — GroupNorm -> proj_in and x4 -> proj_out.
        # Their consumers are the C -> C linears (HBM-bound at the 32x32 level: a doubled K costs bytes, not MFMA time)
        # Measured on MI355X (same box): every doubled C -> C linear costs ~12 us at every level (+1.04 ms per step for all 66), and the
        # probe by level (tests/precision_probe.py ... levels) puts 9.7 of the 10 % / 10.7 of the 13 % of these two classes' gain at
        # the INPUT resolution (its 11 + 11 sites) -> by default only the transformers of the top level are split; "all" = every level
        level = getattr(net, "precise_operands", False)
        self.precise_gn = self.precise and level != "r3"
        self.precise_ff = self.precise and level != "r3"
        self.precise_all_levels = level == "all"
        self.precise_attn = self.precise and bool(getattr(net, "precise_attn_out", False))
        self.precise_rs = self.precise and bool(getattr(net, "precise_resample", False))
        # GroupNorm statistics from the producing GEMM's epilogue (ResBlock conv -> norm, the temporal-conv chain): opt-in (measured slower)
        self.gn_strips = bool(getattr(net, "gn_producer_stats", False))
        self.last_stats: Optional[Buf] = None
        # FreeU at the decoder's skip concatenations (`skip_concat`): (b1, b2, s1, s2) or None.  The lowering of a network that has it sets it.
        self.freeu: Optional[Tuple[float, float, float, float]] = None
        self.stem_dup = False
        self.P.small_rank_tiles = self.shard is not None       # (Program.choose_tile: no temporal convolution of a rank program carries a norm epilogue)
        prefixes = tuple(getattr(net, "split_weight_prefixes", ()) or ())
        if prefixes:
            self.P.weight_lo = lambda ref: (Ref("weight", 0, self.packer.add_lo(ref.name))
                                            if ref.name.startswith(prefixes) and ref.name.rsplit(":", 1)[-1] in ("lin", "lin2", "c3", "c3d", "t3", "qkv", "kv")
                                            else None)
        self.emb_slices: Dict[str, Tuple[int, int]] = {}
        self.kv_slices: Dict[str, Tuple[int, int]] = {}
        self.kv_all: Optional[Buf] = None

    # -- packed-weight declarations ------------------------------------------------------------
    def precise_at(self, flag: bool, h: int, w: int) -> bool:
        """Is a round-4 operand split (flag) applied at the level whose frames are h x w?"""
        return bool(flag) and (self.precise_all_levels or (h == self.H and w == self.W))

    def w_proj(self, key, copies: int) -> Ref:
        """Linear weights for an operand stored as `copies` column blocks (1: plain; 2: rows [hi | lo] -> [W | W])."""
        assert copies in (1, 2)
        return self.w_linear(key) if copies == 1 else self.w_linear_dup(key)

    def w_linear_dup(self, key) -> Ref:
        return Ref("weight", 0, self.packer.add(key + ":lin2", "f16", lambda sd, k=key: pk.pad_rows(pk.linear_dup(sd[k + ".weight"]))))

    def w_qkv(self, prefix) -> Ref:
        def fn(sd, p=prefix):
            return torch.cat([sd[p + ".to_q.weight"], sd[p + ".to_k.weight"], sd[p + ".to_v.weight"]], dim=0)
        return Ref("weight", 0, self.packer.add(prefix + ":qkv", "f16", fn))

    def w_kv(self, prefix) -> Ref:
        def fn(sd, p=prefix):
            return torch.cat([sd[p + ".to_k.weight"], sd[p + ".to_v.weight"]], dim=0)
        return Ref("weight", 0, self.packer.add(prefix + ":kv", "f16", fn))

    def w_geglu(self, key) -> Tuple[Ref, Ref]:
        def wfn(sd, k=key):
            w = sd[k + ".weight"]
            return w[pk.geglu_perm(w.shape[0] // 2, w.device)]
        def bfn(sd, k=key):
            b = sd[k + ".bias"]
            return b[pk.geglu_perm(b.shape[0] // 2, b.device)]
        return (Ref("weight", 0, self.packer.add(key + ":geglu", "f16", wfn)),
                Ref("weight", 0, self.packer.add(key + ":geglu_b", "f32", bfn)))

    def attention_table(self, lens, starts) -> Ref:
        """The per-sample table of a text cross-attention, int32 [samples][2] = {key count, first row}: read-only program data, so it
        lives in the packed weight image (as the tap tables of T2V_OP_RESAMPLE) and the arena holds nothing new."""
        rows = [[int(n), int(r)] for n, r in zip(lens, starts)]
        name = "context.table:" + ",".join(f"{n}@{r}" for n, r in rows)
        return Ref("weight", 0, self.packer.add(name, "i32", lambda sd, rows=rows: torch.tensor(rows, dtype=torch.int32)))

    def ln_arg(self, key, out: Buf, eps: float = 1e-5) -> tuple:
        """`ln=` argument of Program.gemm for the LayerNorm `key` applied to a GEMM's fp32 result: fused into the epilogue of the
        192x320 tile (one fp32 [2C] vector gamma | beta), a separate LayerNorm op otherwise."""
        gb = Ref("weight", 0, self.packer.add(key + ":ln_gb", "f32", lambda sd, k=key: torch.cat([sd[k + ".weight"], sd[k + ".bias"]])))
        return (gb, self.vec(key + ".weight"), self.vec(key + ".bias"), out, eps)

    # -- geometry helpers ----------------------------------------------------------------------
    def M(self, h, w):
        """Token rows of an activation at h x w in the CURRENT batch (one sample while the cond | uncond prefix is shared)."""
        return self.Bc * self.F * h * w

    # -- building blocks ------------------------------------------------------------------------
    def gn_gb(self, key) -> Ref:
        """gamma | beta of the GroupNorm `key` as ONE fp32 [2C] vector (the T2V_EPI_GN epilogue reads both from one pointer)."""
        return Ref("weight", 0, self.packer.add(key + ":gn_gb", "f32", lambda sd, k=key: torch.cat([sd[k + ".weight"], sd[k + ".bias"]])))

    def gn(self, name, x: Buf, key, *, per_frame: bool, eps, silu, out: Optional[Buf] = None, lo: bool = False,
           stats: Optional[Buf] = None, x_dead: bool = False, cast: Optional[Buf] = None, cast_lo: bool = False,
           halo_raw: Optional[Buf] = None) -> Buf:
        """lo (precise_operands): the result is a [rows, 2C] buffer of rows [hi | lo] — fp16(y) and the low-order image of that
        rounding — for a consumer GEMM with weights [W | W] (K = 2C)."""
        if lo:
            assert out is None
            full = self.P.alloc(x.rows, 2 * x.cols, "f16")
            out = full.col_slice(0, x.cols)
        else:
            full = out = self.P.alloc(x.rows, x.cols, "f16") if out is None else out
        n_inst = self.Bc * self.F if per_frame else self.Bc
        shard = None if per_frame else self.shard
        if stats is not None and (x.rows // n_inst) % 32 != 0:
            stats = None                  # (strips are 32 rows; a T-sharded cross-frame norm folds ITS part from them, round 6)
        # (x produced by the op emitted last, on a tile with the instantiation: the norm becomes that GEMM's epilogue — Program._fuse_groupnorm;
        #  x_dead: only this norm reads x)
        self.P.groupnorm(name, x, self.vec(key + ".weight"), self.vec(key + ".bias"), out, n_inst=n_inst, eps=eps, silu=silu,
                         shard=shard, lo=lo, stats=stats, gb=self.gn_gb(key) if shard is None and x.cols % 4 == 0 else None, x_dead=x_dead,
                         cast=cast, cast_lo=cast_lo, halo_raw=halo_raw if shard is not None else None)
        return full

    def strips_for(self, rows: int, n: int, inst_rows: int, k: Optional[int] = None, gather: int = L.GATHER_PLAIN) -> Optional[Buf]:
        """Buffer for the column statistics a GEMM's epilogue leaves for the GroupNorm that consumes its output (T2V_EPI_STATS:
        fp32 [rows / 32][2][n]) — round 4, VERDICT r03 next #4: that GroupNorm then needs neither a statistics pass over the
        tensor nor a grid barrier.  None when the option is off or the consumer's statistics instances (`inst_rows` rows each) are
        not whole 32-row strips."""
        if inst_rows % 32 != 0:
            return None
        if self.shard is not None and inst_rows == self.F * (rows // (self.Bc * self.F)):
            # T-sharded cross-frame norm (never an epilogue: its statistics cross ranks): this rank's part folded from the producer's
            # strips instead of a statistics pass over the tensor (round 6) — one small launch instead of two, per norm
            if L.knob("T2V_TSHARD_STRIPS", "1") == "0":
                return None
        elif not self.gn_strips:
            # round 6: automatically where the consuming norm can NOT run in its producer's epilogue because ONE statistics instance
            # has more row tiles than the device holds co-resident (cross-frame norms of 125-frame / 1024x576 clips): strips + fold +
            # one apply pass instead of the three-launch GroupNorm (two passes over the tensor + one)
            if k is None or not self.P.gn_instance_too_large(rows, n, k, gather, inst_rows) or L.knob("T2V_GN_STRIPS_AUTO", "1") == "0":
                return None
        return self.P.alloc(-(-rows // 32), 2 * n, "f32")

    def conv3(self, name, a: Buf, key, cout, h, w, *, stride=1, up=0, out_dtype="f32", rowbias=None,
              residual=None, cin=None, dest: Optional[Buf] = None, dup_c8: bool = False, stats: Optional[Buf] = None,
              hilo: bool = False, res_wrap: int = 0) -> Buf:
        """`dest`: write the result into this (sub-)buffer instead of a fresh allocation — the producers of the two
        halves of a skip-connection concat write straight into the concat buffer (no copy ops)."""
        cin = a.cols if cin is None else cin
        ho, wo = (h * 2, w * 2) if up else ((h + 1) // 2 if stride == 2 else h, (w + 1) // 2 if stride == 2 else w)
        Mo = self.Bc * self.F * ho * wo
        n = (cout + 3) // 4 * 4
        out = self._dest(dest, Mo, n, out_dtype)
        gather = L.GATHER_CONV3X3_C8 if cin == 8 else L.GATHER_CONV3X3
        wref = self.w_conv3(key, form="hl") if hilo else (self.w_conv3(key, form="d") if dup_c8 else self.w_conv3(key, 8 if cin == 8 else 0))
        op = self.P.gemm(name, a, wref, n, 9 * cin, out, bias=self.vec(key + ".bias"),
                         gather=gather, conv=dict(Hin=h, Win=w, Cin=cin, stride=stride, up=up, Hout=ho, Wout=wo),
                         rowbias=rowbias, rows_per_batch=self.F * ho * wo if rowbias is not None else 0,
                         residual=residual, stats=stats, k_alg=9 * cin // 2 if hilo else None, res_wrap=res_wrap)
        self.last_stats = stats if (stats is not None and op.meta.get("stats")) else None     # None: the op ran with split-K
        return out

    def operand16(self, name, x: Buf, c, hilo: bool) -> Buf:
        """The fp32 stream `x` cast to an fp16 GEMM operand: plain [rows, c], or (precise_operands) rows [hi (c) | lo (c)] — the value
        and the low-order image of its fp16 rounding — for a consumer that runs K = 2c deep against [W | W]."""
        x16 = self.P.alloc(x.rows, 2 * c if hilo else c, "f16")
        if hilo:
            self.P.copy2d(name, x, x16.col_slice(0, c), lo=x16.col_slice(c, 2 * c))
        else:
            self.P.copy2d(name, x, x16)
        return x16

    def res_front(self, prefix, x: Buf, cout, h, w, *, per_frame: bool, strips_k: Optional[int] = None, cast: Optional[Buf] = None,
                  cast_lo: bool = False) -> Buf:
        """ResBlock in_layers -> out_layers.0: norm + SiLU, 3x3 conv with the timestep embedding as a row bias, norm + SiLU.
        strips_k: the conv's reduction length where `strips_for` may choose producer statistics on its own; cast / cast_lo: `gn`."""
        P = self.P
        a = self.gn(prefix + ".in_layers.0", x, prefix + ".in_layers.0", per_frame=per_frame, eps=1e-5, silu=True, cast=cast, cast_lo=cast_lo)
        e0, e1 = self.emb_slices[prefix]
        st = self.strips_for(x.rows, cout, (1 if per_frame else self.F) * h * w, strips_k, L.GATHER_CONV3X3)
        h1 = self.conv3(prefix + ".in_layers.2", a, prefix + ".in_layers.2", cout, h, w,
                        rowbias=self.emb_out.col_slice(e0, e1), out_dtype=self.net.norm_input_dtype, stats=st)
        P.free(a)
        b = self.gn(prefix + ".out_layers.0", h1, prefix + ".out_layers.0", per_frame=per_frame, eps=1e-5, silu=True, stats=self.last_stats,
                    x_dead=True)
        P.free(h1, st)
        return b

    def skip_projection(self, prefix, x: Buf, cin, cout, x16: Optional[Buf] = None) -> Buf:
        """The 1x1 skip convolution of a ResBlock with cin != cout.  x16: the block input as an fp16 operand when a norm already wrote
        it; otherwise cast here — with precise_operands as rows [hi | lo] in ONE pass against [W | W], K = 2 cin."""
        P = self.P
        skip = P.alloc(x.rows, cout, "f32")
        if x16 is None:
            x16 = self.operand16(prefix + ".skip.cast", x, cin, self.precise)
        P.gemm(prefix + ".skip_connection", x16, self.w_proj(prefix + ".skip_connection", x16.cols // cin), cout, x16.cols, skip,
               bias=self.vec(prefix + ".skip_connection.bias"), k_alg=cin)
        P.free(x16)
        return skip

    def kv_gather_attention(self, attn, norm, xin: Buf, inner, heads, hw, scale, *, out_cols: Optional[int] = None,
                            extras: Callable[[], dict] = dict) -> Buf:
        """Temporal self-attention `attn` over a T-sharded clip, on LayerNorm `norm` of the fp32 stream `xin` (consumed): queries =
        local frames, keys/values = ALL frames (K/V projections of the local tokens are all-gathered along T).
        Returns xin + to_out(attention).  out_cols = 2 inner: the attention output as rows [hi | lo]; extras() -> the attention's
        further keyword arguments, called where the attention is emitted (its packed images are declared there)."""
        P, sh, M, F = self.P, self.shard, xin.rows, self.F
        Mmax, Ftot = sh.max_frames * hw, sh.total     # rows of the largest slice; frames of the clip
        n = P.alloc(M, inner, "f16")
        P.layernorm(norm, xin, self.vec(norm + ".weight"), self.vec(norm + ".bias"), n)
        q = P.alloc(M, inner, "f16")
        P.gemm(attn + ".to_q", n, self.w_linear(attn + ".to_q"), inner, inner, q)
        # slice q of the gathered buffer starts at frame q * max_frames: only the LAST slice can be short, so the
        # clip's frames are contiguous from row 0 and the padding rows at the very end are never addressed
        kv_all = P.alloc(sh.size * Mmax, 2 * inner, "f16")
        mine = kv_all.row_slice(sh.index * Mmax, sh.index * Mmax + M)
        P.gemm(attn + ".kv", n, self.w_kv(attn), 2 * inner, inner, mine)
        P.free(n)
        full = Buf(kv_all.ref, sh.size * Mmax * 2 * inner * 2, 1, 1, "u8", kv_all.alloc_off)
        P.allgather(attn + ".kv.allgather", full, Mmax * 2 * inner * 2, sh)
        a = P.alloc(M, out_cols or inner, "f16")
        ldk, lo = 2 * inner, a.ld
        k, v = kv_all.col_slice(0, inner), kv_all.col_slice(inner, 2 * inner)
        P.attention(attn, q.ref, k.ref, v.ref, a.ref, out_buf=a, nq=F, nk=Ftot, heads=heads,
                    b_outer=1, b_inner=hw, q_strides=(hw * inner, 0, inner), kv_strides=(hw * ldk, 0, ldk),
                    o_strides=(hw * lo, 0, lo), scale=scale, **extras())
        P.free(q, kv_all)
        xo = P.alloc(M, inner, "f32")
        P.gemm(attn + ".to_out", a, self.w_proj(attn + ".to_out.0", a.cols // inner), inner, a.cols, xo,
               bias=self.vec(attn + ".to_out.0.bias"), residual=xin, k_alg=inner)
        P.free(a, xin)
        return xo

    def to_q_attention(self, attn, nrm: Buf, a: Buf, inner, heads, hw, scale, wrap: int) -> bool:
        """Hook of `text_cross_attention`: emit to_q + attention as ONE launch where the network has one.  The base has none."""
        return False

    def text_cross_attention(self, attn, inner, heads, hw, scale, *, nrm: Optional[Buf] = None, q: Optional[Buf] = None,
                             out_cols: Optional[int] = None, **attn_kw) -> Tuple[Buf, int]:
        """Attention `attn` of the current tokens over the text context (K / V: this site's columns of `kv_all`).  The caller passes
        the queries `q` (consumed), or the normalised tokens `nrm` (consumed) to have them projected here — after the output's
        allocation, and only then `to_q_attention` may take both steps.
        This is where cond and uncond part.  While the prefix is shared, q / the residual stream hold ONE sample's rows: the attention
        reads q with a zero sample stride against each sample's own K / V, and from here on every tensor has B samples.  Returns (the
        attention output, `res_wrap` with which to_out adds the one-sample residual stream to it)."""
        P, F, Lc = self.P, self.F, self.Lctx
        k0, k1 = self.kv_slices[attn]
        kv = self.kv_all
        kbuf, vbuf = kv.col_slice(k0, k0 + inner), kv.col_slice(k0 + inner, k1)
        Mq = self.Bc * F * hw
        parting = self.sharing
        q_b_stride, shared_rows = (0, Mq) if parting else (F * hw * inner, 0)
        if parting:
            self.sharing, self.Bc = False, self.B
        a = P.alloc(self.Bc * F * hw, out_cols or inner, "f16")
        lo = a.ld
        if q is None and not self.to_q_attention(attn, nrm, a, inner, heads, hw, scale, shared_rows):
            q = P.alloc(Mq, inner, "f16")
            P.gemm(attn + ".to_q", nrm, self.w_linear(attn + ".to_q"), inner, inner, q)
        if q is not None:
            if self.Lsamples is not None:
                # every sample with its own context length, still ONE launch: sample s reads Lsamples[s] rows behind those of samples 0 .. s-1
                starts = [sum(self.Lsamples[:b]) for b in range(self.B)]
                attn_kw = dict(attn_kw, table=(self.attention_table(self.Lsamples, starts), self.Lsamples, starts))
            if self.Lpair is not None:
                # cond | uncond with their own context lengths, still ONE launch: samples V .. B-1 read the rows behind the V * Lc cond rows
                V, (Lc, Lu) = self.B // 2, self.Lpair
                k2, v2 = kbuf.row_slice(V * Lc, V * (Lc + Lu)), vbuf.row_slice(V * Lc, V * (Lc + Lu))
                attn_kw = dict(attn_kw, alt=(V, Lu, k2.ref, v2.ref, Lu * kv.ld))
            P.attention(attn, q.ref, kbuf.ref, vbuf.ref, a.ref, out_buf=a, nq=hw, nk=Lc, heads=heads,
                        b_outer=self.Bc, b_inner=F, q_strides=(inner, q_b_stride, hw * inner),
                        kv_strides=(kv.ld, 0 if self.Lsamples is not None else Lc * kv.ld, 0), o_strides=(lo, F * hw * lo, hw * lo), scale=scale, **attn_kw)
            P.free(q)
        P.free(nrm)
        return a, shared_rows

    def ff_tail(self, tb, n: Buf, x3: Buf, inner, h, w) -> Buf:
        """Feed-forward of transformer block `tb` on n = LayerNorm3(x3) (both consumed): GEGLU fused in the first GEMM's epilogue.
        x4 = x3 + FF feeds proj_out as an fp16 operand: with precise_operands it is stored as rows [hi | lo] (the low-order image
        of the fp16 rounding beside the value) and proj_out runs with K doubled against [W | W]."""
        P, M = self.P, n.rows
        wg, bg = self.w_geglu(f"{tb}.ff.net.0.proj")
        g = P.alloc(M, 4 * inner, "f16")
        P.gemm(f"{tb}.ff.geglu", n, wg, 8 * inner, inner, g, bias=bg, epi=L.EPI_GEGLU)
        P.free(n)
        hilo = self.precise_at(self.precise_ff, h, w)
        x4 = P.alloc(M, 2 * inner if hilo else inner, "f16")
        P.gemm(f"{tb}.ff.net.2", g, self.w_linear(f"{tb}.ff.net.2"), inner, 4 * inner, x4.col_slice(0, inner) if hilo else x4,
               bias=self.vec(f"{tb}.ff.net.2.bias"), residual=x3, out_lo=hilo)
        P.free(g, x3)
        return x4

    def resample(self, prefix, attr, x: Buf, c, h, w, *, up, dest: Optional[Buf] = None, **conv_kw) -> Buf:
        """Down / Upsample convolution `prefix.attr` on the stream's fp16 cast — with precise_resample as rows [hi | lo] (2c channels),
        the convolution on K = 9 * 2c against [W | W].  conv_kw: further `conv3` arguments (the residual of an adapter site)."""
        hilo = bool(self.precise_rs and c % 64 == 0)
        x16 = self.operand16(prefix + ".cast", x, c, hilo)
        out = self.conv3(f"{prefix}.{attr}", x16, f"{prefix}.{attr}", c, h, w, stride=1 if up else 2, up=1 if up else 0, dest=dest, hilo=hilo,
                         **conv_kw)
        self.P.free(x16)
        return out

    # -- whole network ------------------------------------------------------------------------------
    def layout(self) -> Tuple[list, list, list, list]:
        """-> (inputs, middle, outputs, packed): the network's blocks as (block prefix, [(part prefix, kind, cin, cout), ...]) —
        encoder blocks, the middle block, decoder blocks — and all of them again in the order in which the step-level prologue
        concatenates their timestep-embedding and text K/V projections."""
        raise NotImplementedError

    def time_freqs(self) -> Ref:
        """The packed frequency vector of the sinusoidal timestep embedding."""
        raise NotImplementedError

    def prologue_alloc(self, sites: List[Tuple[str, int]]):
        """Hook: buffers the network keeps for the whole program beside `kv_all`, allocated right after it so that no other buffer
        can alias them between two runs.  sites: (prefix, channels) of the text cross-attention sites.  -> the buffers."""
        return []

    def prologue_extra(self, sites: List[Tuple[str, int]], ctx16: Buf):
        """Hook: further step-invariant ops on the fp16 text context."""

    def lower_part(self, kind, p, x: Buf, cin, cout, h, w, dest: Optional[Buf], inject: Optional[Buf]) -> Buf:
        """One part of a block.  The base knows the convolutions; a convolution has no residual of its own: an injected feature IS
        its residual (no extra launch), wrapped over the batch's roles when it holds fewer samples than the batch."""
        if kind not in ("stem", "down", "up"):
            raise ValueError(kind)
        ho, wo = {"stem": (h, w), "down": ((h + 1) // 2, (w + 1) // 2), "up": (h * 2, w * 2)}[kind]
        res = dict(residual=inject, res_wrap=inject.rows if inject.rows < self.M(ho, wo) else 0) if inject is not None else {}
        if kind == "stem":
            return self.conv3(p, x, p, cout, h, w, cin=8, dest=dest, dup_c8=self.stem_dup, **res)
        return self.resample(p, "op" if kind == "down" else "conv", x, cout, h, w, up=kind == "up", dest=dest, **res)

    def skip_concat(self, prefix: str, cat: Buf, c_h: int, h: int, w: int):
        """The concat buffer `cat` = [stream (c_h channels) | skip] of decoder block `prefix` is complete — both halves written, the
        copies of a shared cond | uncond prefix included — and nothing has read it yet (its readers are the block's first ResBlock:
        the in_layers GroupNorm, the 1x1 skip_connection, any fp16 operand cast).  With FreeU on, a stream of 4 dim channels takes
        (b1, s1) and one of 2 dim channels (b2, s2), in place, one T2V_OP_FREEU; any other width is left alone (the channel-keyed rule
        of the FreeU authors' code).  The op is its own record between the producers and the readers, so whatever a producer recorded
        about these columns — statistics strips, a norm in its epilogue, a low-order fp16 image — describes another buffer or is
        never consulted here: no reader of `cat` takes anything from the op in front of it unless that op's output IS `cat`."""
        if self.freeu is None:
            return
        b1, b2, s1, s2 = self.freeu
        gains = {4 * self.net.dim: (b1, s1), 2 * self.net.dim: (b2, s2)}.get(c_h)
        if gains is not None:
            self.P.freeu(prefix + ".freeu", cat, c_h=c_h, frames=self.B * self.F, h=h, w=w, b=gains[0], s=gains[1])

    def inject_for(self, k: int, c, h, w) -> Optional[Buf]:
        """Hook: the feature added to the result (c channels at h x w) of encoder block k.  The base has none."""
        return None

    def build(self) -> Program:
        net, P, B, F = self.net, self.P, self.B, self.F
        inputs, middle, outputs, packed = self.layout()
        dim, emb = net.dim, net.embed_dim
        h, w = self.H, self.W
        P.begin()
        if self.sharing and not any(kind == "st" for _, parts in inputs for _, kind, _, _ in parts):
            self.sharing, self.Bc = False, B           # no text cross-attention on the way down: nothing to share up to

        # ---- step-level prologue: time embedding, all ResBlock emb projections, all cross-attn K/V
        res_prefixes = [(p, cout) for _, parts in packed for p, kind, _, cout in parts if kind == "res"]
        st_prefixes = [(p, cout) for _, parts in packed for p, kind, _, cout in parts if kind == "st"]
        off = 0
        for p, cout in res_prefixes:
            self.emb_slices[p] = (off, off + cout)
            off += cout
        n_emb = off
        off = 0
        for p, c in st_prefixes:
            self.kv_slices[p + ".transformer_blocks.0.attn2"] = (off, off + 2 * c)
            off += 2 * c
        n_kv = off

        # The text-context K/V projections do not depend on x or t: they are the program's step-invariant prologue
        # (Op.meta['step_invariant']), skipped when the caller vouches that the context is the one of the previous run
        # (UNetSD.context_token).  Their buffer is allocated FIRST and freed last, so no other
        # buffer of the program can alias it between two runs.
        if n_kv:
            self.kv_all = P.alloc(self.ctx_rows, n_kv, "f16")
        kept = self.prologue_alloc(st_prefixes) if n_kv else []
        te = P.alloc(B, dim, "f16")
        P.time_embed("time_embed.sincos", Ref("ext", L.EXT_T), self.time_freqs(), te)
        e1 = P.alloc(B, emb, "f16")
        P.gemm("time_embed.0", te, self.w_linear("time_embed.0"), emb, dim, e1, bias=self.vec("time_embed.0.bias"), act=1)
        P.free(te)
        e_silu = P.alloc(B, emb, "f16")       # SiLU(e): the only form in which e is consumed (emb_layers = SiLU -> Linear)
        P.gemm("time_embed.2", e1, self.w_linear("time_embed.2"), emb, emb, e_silu, bias=self.vec("time_embed.2.bias"), act=1)
        P.free(e1)
        w_emb = Ref("weight", 0, self.packer.add("emb_all:lin", "f16", lambda sd, ps=tuple(p for p, _ in res_prefixes):
                                                 torch.cat([sd[p + ".emb_layers.1.weight"] for p in ps], dim=0)))
        b_emb = Ref("weight", 0, self.packer.add("emb_all:v", "f32", lambda sd, ps=tuple(p for p, _ in res_prefixes):
                                                 torch.cat([sd[p + ".emb_layers.1.bias"] for p in ps], dim=0)))
        self.emb_out = P.alloc(B, n_emb, "f32")
        P.gemm("emb_layers.all", e_silu, w_emb, n_emb, emb, self.emb_out, bias=b_emb)
        P.free(e_silu)

        ctx16 = P.alloc(self.ctx_rows, net.context_dim, "f16")
        ctx_src = Buf(Ref("ext", L.EXT_CTX), self.ctx_rows, net.context_dim, net.context_dim, self.ctx_dt)
        P.copy2d("context.cast", ctx_src, ctx16).meta["step_invariant"] = True
        if n_kv:
            w_kv = Ref("weight", 0, self.packer.add("kv_all:lin", "f16", lambda sd, ps=tuple(p for p, _ in st_prefixes): torch.cat(
                [torch.cat([sd[p + ".transformer_blocks.0.attn2.to_k.weight"], sd[p + ".transformer_blocks.0.attn2.to_v.weight"]], dim=0)
                 for p in ps], dim=0)))
            P.gemm("attn2.kv.all", ctx16, w_kv, n_kv, net.context_dim, self.kv_all, step_invariant=True)
            self.prologue_extra(st_prefixes, ctx16)
        P.free(ctx16)

        # ---- entry layout conversion: b c f h w -> tokens x 8 channels (4 real + 4 zero)
        xin = P.alloc(self.M(h, w), 8, "f16")
        # precise operands: the low-order fp16 images of the 4 latent channels ride in the 4 padding channels of the 8-channel
        # token rows, the stem's weights repeat W there — (x_hi + x_lo) . W in the one GEMM pass, no extra launch
        self.stem_dup = self.precise and self.x_dt == "f32" and net.in_dim == 4
        P.ncthw_to_cl("x.to_tokens", Ref("ext", L.EXT_X), self.x_dt, xin, B=self.Bc, C=net.in_dim, F=F, HW=h * w,
                      src_batch=self.x_batch if self.x_batch != self.Bc else 0, lo_in_pad=self.stem_dup)

        def out_hw(parts, h, w):
            for _, kind, _, _ in parts:
                if kind == "down":
                    h, w = (h + 1) // 2, (w + 1) // 2
                elif kind == "up":
                    h, w = h * 2, w * 2
            return h, w

        def run_parts(parts, x, h, w, dest=None, inject=None):
            """inject: a feature added to this block's result (a residual operand of its last GEMM — the result lands in the concat
            buffer with the feature in it)."""
            for i, (p, kind, cin, cout) in enumerate(parts):
                last = i == len(parts) - 1
                d = dest if last else None         # the block's result goes straight into a concat buffer
                # shared cond | uncond prefix: this part's result has ONE sample's rows; a skip-connection window wants it for every
                # sample -> the part writes its own buffer and two row-block copies fill the window (one site: input_blocks.0)
                spread = d if (self.sharing and d is not None and kind != "st") else None
                if spread is not None:
                    d = None
                y = self.lower_part(kind, p, x, cin, cout, h, w, d, inject if last else None)
                h, w = out_hw(parts[i:i + 1], h, w)
                if spread is not None:
                    assert spread.rows == self.B * y.rows and spread.cols == y.cols
                    for b in range(self.B):
                        P.copy2d(f"{p}.to_skip.{b}", y, spread.row_slice(b * y.rows, (b + 1) * y.rows))
                P.tap(p, y)
                P.free(x)              # borrowed windows of a concat buffer are ignored by free()
                x = y
            return x, h, w

        # Skip connections (`torch.cat([x, xs.pop()], dim=1)`): the concat buffer of decoder block j
        # is allocated when its encoder half is produced; encoder block k writes the right window, the op that produces
        # the decoder stream (middle block / previous decoder block) writes the left one — no copy kernels.
        n_skip = len(inputs)
        skip_c = [parts[-1][3] for _, parts in inputs]              # channels each encoder block leaves for its decoder block
        cats: List[Buf] = []
        x = xin
        for k, (_, parts) in enumerate(inputs):
            cin_total = outputs[n_skip - 1 - k][1][0][2]            # input channels of the consuming decoder ResBlock
            ho, wo = out_hw(parts, h, w)
            cat = P.alloc(self.B * self.F * ho * wo, cin_total, "f32")        # (every sample, whatever the current batch of the prefix)
            cats.append(cat)
            x, h, w = run_parts(parts, x, h, w, dest=cat.borrow_cols(cin_total - skip_c[k], cin_total),
                                inject=self.inject_for(k, skip_c[k], ho, wo))
        cat = cats.pop()
        x, h, w = run_parts(middle[1], x, h, w, dest=cat.borrow_cols(0, cat.cols - skip_c[-1]))
        for j, (prefix, parts) in enumerate(outputs):
            self.skip_concat(prefix, cat, cat.cols - skip_c[n_skip - 1 - j], h, w)
            nxt = cats.pop() if cats else None
            dest = nxt.borrow_cols(0, nxt.cols - skip_c[n_skip - 2 - j]) if nxt is not None else None
            x, h, w = run_parts(parts, cat, h, w, dest=dest)
            cat = nxt

        assert not self.sharing and self.Bc == B, "the shared cond | uncond prefix never reached a text cross-attention"
        # ---- head: GN + SiLU + conv 3x3 -> out_dim, then tokens -> b c f h w
        a = self.gn("out.0", x, "out.0", per_frame=self.head_per_frame, eps=1e-5, silu=True)
        P.free(x)
        y = self.conv3("out.2", a, "out.2", net.out_dim, h, w)
        P.free(a)
        P.cl_to_ncthw("eps.from_tokens", y, Ref("ext", L.EXT_OUT), self.out_dt, B=B, C=net.out_dim, F=F, HW=h * w)
        P.free(y, self.emb_out)
        if n_kv:
            P.free(self.kv_all, *kept)
        P.finish()
        return P
