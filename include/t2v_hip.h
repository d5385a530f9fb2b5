/*
 * t2v_hip.h — C ABI of libt2v_hip.so, the MI355X (gfx950) implementation of the
 * ModelScope / ZeroScope text-to-video denoising hot path.
 *
 * The reference (kabachuha/sd-webui-text2video) has no FFI: its seam is Python duck-typing
 * (SURVEY.md §8b).  This header is the boundary a maintainer binds with ctypes
 *  to replace the torch.nn delegation layer under
 *   - UNetSD.forward / _forward_single      scripts/modelscope/t2v_model.py:386-501   (B4)
 *   - AutoencoderKL.decode                  scripts/modelscope/t2v_model.py:1646-1649 (B5)
 *   - GaussianDiffusion.sample step update  scripts/samplers/ddim/gaussian_sampler.py:257-283
 *
 * Design: the host (Python) lowers a model + shape into a flat *denoise program* — an array
 * of t2v_op records over one activation arena and one packed-weight arena — and this library
 * executes the program by launching hand-written HIP kernels on the caller's HIP stream.
 * Plain pointers and sizes only; no torch types.  All device memory is owned by the caller;
 * pointers are borrowed for the duration of a call.  No internal threads; one in-flight call
 * per plan.  Every function returns 0 on success or a negative T2V_ERR_* code; the message of
 * the last failure is available from t2v_last_error().
 */
#ifndef T2V_HIP_H
#define T2V_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2V_ABI_VERSION 11  /* 11: VideoCrafter depth adapter (additive: no existing record changes) — T2V_OP_DEPTH_TOKENS (depth frames -> PixelUnshuffle(8)
                               tokens, optional per-frame min-max normalisation), T2V_OP_AVGPOOL2 (2x2 mean of channels-last fp32 tokens), GEMM i[18] = 2
                               (ReLU), GEMM i[30] (residual row wrap for every gather mode, split-K allowed), T2V_EXT_ADAPTER (feature slots);
                               still 11: DDIM_STEP i[7] / p[4..6] / f[6..7] (mask blend of a VideoCrafter step) — additive on fields that every earlier
                               record leaves zero, so the version does not move;
                               still 11: DDIM_STEP i[8] / i[9] / p[7..8] / f[6..7] in mode 0 (clamp / percentile restriction of x0 with its measure pass, and the
                               classifier-guidance term of DDIM_Gaussian) — additive on fields that every earlier record leaves zero;
                               still 11: DDIM_STEP i[5] = 2 (UniPC's thresholded data prediction: a measure and an apply record) — a mode value that every earlier
                               library refuses, records with i[5] in {0, 1} are validated and run as before;
                               still 11: DDIM_STEP i[5] = 3 (the DDIM inversion step of DDIMSampler.encode, with the optional second destination p[4]) — a mode
                               value that every earlier library refuses, records with i[5] in {0, 1, 2} are validated and run as before;
                               still 11: DDIM_STEP i[5] = 4 (the DDIM_Gaussian step followed by the keyframe blend of the legacy img2vid loop, with p[4..6], f[6..7]
                               and the threshold's bits in i[10]) — a mode value that every earlier library refuses, records with i[5] in {0, 1, 2, 3} are
                               validated and run as before;
                               still 11: T2V_OP_EMPHASIS (a new kind: no existing record changes, and a library without it refuses the record as an unknown op kind) and
                               ATTENTION i[19..21] / p[4..5] (a second role; additive on fields every earlier record leaves zero);
                               still 11: T2V_OP_FINGERPRINT (a new kind, stand-alone: 64-bit fingerprints of a table of byte ranges; no existing record changes);
                               still 11: T2V_OP_LORA_MERGE (a new kind, stand-alone: W += alpha * (B A) over a table of weights, in place, one launch; no existing record
                               changes, and a library without it refuses the record as an unknown op kind);
                               still 11: RESAMPLE i[9] = 1 / i[10] / i[11] (a float bicubic resize of planar images in one launch — the resizes around the depth
                               estimator of the VideoCrafter depth adapter; additive on fields that every earlier record leaves zero);
                               still 11: TO_UINT8 i[15] = 1 (torch_to_np's arithmetic and per-video output blocks — the VideoCrafter driver's frames; additive on
                               a field that every earlier record leaves zero);
                               still 11: T2V_OP_FREEU (a new kind: FreeU at a decoder skip concatenation, in place, one launch; no existing record changes, and
                               a library without it refuses the record as an unknown op kind);
                               10: T2V_OP_RESAMPLE — one pass of Pillow's 8-bit Lanczos resize of uint8 frames (vid2vid / inpainting input of any size), the last pass
                               optionally writing the VAE encoder's entry tokens (additive: no existing record changes);
                               9: RELPOS_ATTN i[17] = 3 — relative-position attention for clips of up to T2V_RELPOS_MAX_FRAMES frames (tables packed
                               for it in p[6] / p[7], layout below);
                               8 (round 6): peer windows (t2v_comm_window_create / _open / t2v_comm_counters): exchanges as device-initiated stores into IPC-mapped mailboxes;
                               7 (round 6): ATTENTION p[6] / i[17] / i[18] (V^T scratch: spatial self-attention with LDS-DMA tiles); T2V_ERR_RESIDENCY — a launch that needs its whole grid co-resident was refused by the occupancy check (the caller
                               lowers again without norms fused into GEMM epilogues); a launch refused because a fault was raised mid-run reports T2V_ERR_ASYNC;
                               6 (round 5, second half): T2V_OP_STATS_HALO — the statistics parts of a T-sharded cross-frame GroupNorm and the RAW boundary
                               frames of the temporal convolution behind it in ONE grouped exchange; GROUPNORM i[21] / i[22] (phase 2 also normalises the
                               received boundary frames); t2v_comm_all_gather (eps pair / frame gathers over the library's communicators);
                               5 (round 5): T2V_OP_NI 32 / T2V_OP_NP 12 (record grew), T2V_EPI_GN — GroupNorm (+SiLU) of a GEMM's result fused into its epilogue;
                               4 (round 4): t2v_async_status, t2v_sync_reset, T2V_ERR_ASYNC (bounded grid barrier of the single-pass GroupNorm);
                               3 (round 3): T2V_EPI_TATTN + tile 10, GROUPNORM i[15] / p[5], GEMM p[7] tickets, RELPOS i[17], low-order outputs of the cast ops, T2V_SYNC_* */

/* error codes */
#define T2V_OK 0
#define T2V_ERR_BAD_ARG (-1)
#define T2V_ERR_UNSUPPORTED (-2)
#define T2V_ERR_LAUNCH (-3)
#define T2V_ERR_NO_DEVICE (-4)
#define T2V_ERR_COMM (-5)      /* RCCL not loadable / communicator call failed */
#define T2V_ERR_ASYNC (-6)     /* a kernel of an EARLIER run raised a fault (bounded grid barrier timed out): that run's results are invalid */
#define T2V_ERR_RESIDENCY (-7) /* a fused-norm launch (T2V_EPI_GN, cross-tile LayerNorm, cooperative GroupNorm) does not fit co-resident on this device */

/* RELPOS_ATTN i[17] = 3: longest clip, and the Ev^T table layout it reads (see RELPOS_ATTN below) */
#define T2V_RELPOS_MAX_FRAMES 1024
#define T2V_RELPOS_LONG_PADL 72
#define T2V_RELPOS_LONG_COLS(R) ((2 * (R) + 158) / 8 * 8)

/* FINGERPRINT: bytes of one segment that one workgroup reads (the unit of the host's chunk table), and the multiplier of the length term */
#define T2V_FINGERPRINT_CHUNK 65536
#define T2V_FINGERPRINT_LEN 0x9E3779B97F4A7C15ull

/* LORA_MERGE: elements of one segment (one weight) that one workgroup updates (the unit of the host's tile table), and the two forms of the product */
#define T2V_LORA_TILE 4096
#define T2V_LORA_DIRECT 0    /* delta[n, j] = sum_k B[n, k] A[k, j]                                   (Linear, Conv2d)            */
#define T2V_LORA_TEMPORAL 1  /* delta[n, j] = mean_s d[n, 3 j + s], d = B A of 3 J columns            (Conv3d [o, i, 3, 1, 1])    */

/* ---- op kinds ------------------------------------------------------------------------- */
enum t2v_op_kind {
  T2V_OP_GEMM = 1,        /* implicit-GEMM conv / linear on MFMA, fused epilogue            */
  T2V_OP_GROUPNORM = 2,   /* GroupNorm(32) (+SiLU), per-frame or cross-frame statistics     */
  T2V_OP_LAYERNORM = 3,   /* row LayerNorm fp32 -> fp16                                     */
  T2V_OP_ATTENTION = 4,   /* softmax(QK^T * scale) V, head_dim 40|64|80|160, strided batch  */
  T2V_OP_SOFTMAX = 5,     /* row softmax fp32 -> fp16 (VAE single-head attention)           */
  T2V_OP_NCTHW_TO_CL = 6, /* [B,C,F,H,W] -> channels-last fp16 tokens [B*F*H*W, ld]         */
  T2V_OP_CL_TO_NCTHW = 7, /* channels-last fp32 tokens -> [B,C,F,H,W]                       */
  T2V_OP_TIME_EMBED = 8,  /* sinusoidal timestep embedding (cos | sin) -> fp16              */
  T2V_OP_COPY2D = 9,      /* strided 2-D copy / cast / SiLU (concat, fp32->fp16 staging)    */
  T2V_OP_DDIM_STEP = 10,  /* DDIM_Gaussian update with half-channel CFG                     */
  T2V_OP_MEMSET = 11,     /* zero a byte range                                              */
  T2V_OP_LINCOMB = 12,    /* out = sum_i c_i * T_i (<= 6 latent-sized tensors): UniPC / DDIM updates */
  T2V_OP_RELPOS_ATTN = 13, /* LVDM temporal attention with relative-position K / V terms (frames <= 32; <= T2V_RELPOS_MAX_FRAMES with i[17] = 3) */
  T2V_OP_EMBED_ROWS = 14,  /* token + positional embedding lookup (CLIP text towers) */
  T2V_OP_TO_UINT8 = 15,    /* tensor2vid: float video -> uint8 frames [F,H,(i W),3], truncating (t2v_pipeline.py:447-460); form 1: torch_to_np (sample_utils.py:98-107) */
  T2V_OP_ALLGATHER = 16,   /* in-place all-gather of equal byte parts over the plan's communicator (RCCL, launch stream) */
  T2V_OP_HALO_EXCHANGE = 17, /* +-1 frame neighbour exchange of a [F+2]-frame token buffer over the plan's communicator */
  T2V_OP_RESHARD_ROWS = 18,  /* chunked row regrouping (pack / unpack of a frame <-> pixel resharding), optional fp32 residual */
  T2V_OP_ALLTOALL = 19,      /* frame <-> pixel resharding of a T-sharded clip over the plan's communicator */
  T2V_OP_STATS_HALO = 20,    /* GroupNorm statistics parts to every rank + raw boundary frames to the two neighbours: one grouped exchange */
  T2V_OP_RESAMPLE = 21,      /* one separable pass of a table-driven uint8 image resize (Pillow's 8-bit resampler, bit-exact), optional float token output; i[9] = 1: a float bicubic resize of planar images */
  T2V_OP_DEPTH_TOKENS = 22,  /* depth frames [n,1,H,W] -> PixelUnshuffle(8) channels-last fp16 tokens, optional per-frame min-max normalisation (T2I-Adapter entry) */
  T2V_OP_AVGPOOL2 = 23,      /* 2x2 / stride 2 average pooling of channels-last fp32 tokens (mean in fp32), fp32 and / or fp16 out */
  T2V_OP_EMPHASIS = 24,      /* prompt emphasis of a batch of text-encoder chunks: per-token multipliers, then the batch mean restored (fp64 sums, one workgroup) */
  T2V_OP_FINGERPRINT = 25,   /* one 64-bit fingerprint per byte range of a device table (in-place edits of packed parameters); stand-alone, never part of a plan */
  T2V_OP_LORA_MERGE = 26,    /* W += alpha * (B A) for every weight of a device table, in place (Stable LoRA merge / un-merge); stand-alone, never part of a plan */
  T2V_OP_KIND_MAX = 27,      /* end of the kinds 1 .. 26, the range the record-path tables classify; kinds added since follow it */
  T2V_OP_FREEU = 27          /* FreeU (Si et al.) at one decoder skip concatenation: half of the stream's channels times b, the skip's low frequencies times s; in place */
};

/* GEMM gather modes: how row m / reduction index k of the A operand are addressed          */
enum t2v_gather {
  T2V_GATHER_PLAIN = 0,   /* A[m*lda + k]                                   (nn.Linear, 1x1) */
  T2V_GATHER_CONV3X3 = 1, /* 3x3 spatial conv, pad 1, stride 1|2, optional nearest-2x
                             upsample folded in; K = 9*Cin, Cin % 64 == 0, reduction order
                             (64-channel chunk, tap, channel)                                */
  T2V_GATHER_TCONV3 = 2,  /* (3,1,1) temporal conv over frames, pad (1,0,0); K = 3*Cin       */
  T2V_GATHER_CONV3X3_C8 = 3 /* 3x3 spatial conv with Cin == 8 (4 real + 4 zero channels)     */
};

/* GEMM epilogues */
#define T2V_EPI_NONE 0
#define T2V_EPI_GEGLU 1   /* out[m, j] = (a_j + b_j) * gelu(g_j + c_j); weight rows interleaved
                             in blocks of 16 = 8 value rows | 8 gate rows                    */
#define T2V_EPI_TATTN 2   /* fused QKV projection + temporal self-attention (tile 10): W = [heads][q 64 | k 64 | v 64][K]
                             (head-major), N = 192 * heads; the tile's rows are i[10] pixels x F (= i[8] <= 32) frames of
                             one sample (input / output row of (sample s, frame f, pixel x) = (s*F + f)*HW + x, HW = i[9]);
                             M = samples * ceil(HW / i[10]) * 192 (tile rows, not tokens); out fp16 [samples*F*HW, ldc]:
                             softmax(q k^T f[1]) v of every pixel's frame sequence, head h at columns 64 h .. 64 h + 63 */

#define T2V_EPI_STATS 3   /* = T2V_EPI_NONE, and p[7] (fp32 [ceil(M/32)][2][N]) receives per 32-row strip the column sums and sums of squares of the
                             STORED result (after bias / row bias / activation / residual; fp16 outputs: of the rounded values) — the input of a
                             GROUPNORM phase 3, which then needs no pass over the tensor for its statistics.  No split-K, no fused LayerNorm. */

#define T2V_EPI_GN 4      /* = T2V_EPI_NONE, and the GroupNorm (+SiLU) that consumes the result runs INSIDE the epilogue (round 5): every workgroup keeps
                             its bias / row-bias / residual-added fp32 tile in registers, publishes {sum, sum of squares} per (statistics instance, group
                             piece), all workgroups of the launch meet at a bounded grid barrier (p[11]: T2V_SYNC_BARRIER_INTS words, as GROUPNORM p[5]),
                             fold the partials of their instances in a fixed order (bit-identical statistics everywhere) and write
                             p[9] = fp16 [M, i[25]] = (silu)((v - mean) * rstd * gamma + beta) — no statistics pass, no second launch, and for a
                             result that only the norm consumes (i[29] = 1) no fp16 / fp32 round trip of the tensor at all.
                             i[24] rows per statistics instance (a frame: H*W; all frames of a sample: F*H*W; multiple of 32, >= the tile's rows),
                             i[25] ld of the normalised output, i[26] SiLU, i[27] = 1: low-order fp16 image at column N + n (ld >= 2N, as GROUPNORM i[16]),
                             i[28] groups (N % groups == 0), i[29] = 1: `out` (p[5]) is NOT written; f[2] eps;
                             p[8] gamma | beta fp32 [2N], p[9] normalised output fp16, p[10] scratch fp64 [tiles_m][2][tiles_n][T2V_GN_PIECES][2],
                             p[11] grid-barrier words.  No split-K / GEGLU / fused LayerNorm; tiles 8 / 11 (whole rows, N == 320), 0, 3, 5 — the
                             grid must be co-resident on the device (the library checks with the occupancy API and refuses otherwise). */
#define T2V_EPI_XATTN 5   /* fused to_q projection + text cross-attention (round 5): out fp16 [M, ldc] = softmax(q k^T f[1]) v per (sample, head of 64
                             channels), q = A W^T (no bias), keys = the i[25] (<= 96) text tokens.  p[8] = K fp16 [samples][i[25]][i[24]] (this
                             site's N columns; i[27] elements between samples), p[9] = V^T fp16 [samples][N][i[26]] (keys contiguous, finite
                             beyond i[25]; i[28] elements between samples), both written by step-invariant ops; the sample of row m is
                             m / i[15].  N % 64 == 0; tiles 8 / 11 (N == 320) and 0 / 5 (N % 128 == 0); plain gather, no split-K, fp16 out. */
#define T2V_GN_PIECES 36  /* group pieces (group x column tile intersections) per column tile in the T2V_EPI_GN scratch */

/* dtype tags */
#define T2V_F16 0
#define T2V_F32 1

/* external pointer slots: a pointer field whose value is < T2V_EXT_SLOTS is replaced at run
 * time by ext[value] (value 0 = null). */
#define T2V_EXT_SLOTS 16
#define T2V_EXT_X 1      /* UNet: x [B,4,F,h,w]   | VAE: z [n,4,h,w]   | text tower: token ids int32 [B,L] */
#define T2V_EXT_T 2      /* UNet: timesteps, float32 [B]                                     */
#define T2V_EXT_CTX 3    /* UNet: context [B,L,ctx_dim]                                      */
#define T2V_EXT_OUT 4    /* UNet: eps [B,4,F,h,w] | VAE: image [n,3,8h,8w] | text tower: z fp32 [B,L,width] */
#define T2V_EXT_XT 5     /* DDIM: x_t in                                                     */
#define T2V_EXT_XT_OUT 6 /* DDIM: x_{t-1} out                                                */
#define T2V_EXT_NOISE 7  /* DDIM: eta-noise (may be null when sigma == 0)                    */
#define T2V_EXT_EPS 8    /* DDIM: stacked UNet outputs [2,C,F,h,w] (cond, uncond)            */
#define T2V_EXT_ADAPTER 9 /* first of T2V_EXT_SLOTS - 9 slots: adapter feature k at slot 9 + k, channels-last fp32 tokens [samples*F*h_k*w_k, C_k]
                             (UNet: read as a residual at injection site k | adapter program: written by level k's last convolution)       */

/* GroupNorm pass-1 granularity: rows of one statistics instance reduced per workgroup.  The
 * caller sizes the scratch as nparts*n_inst*ceil(rows/16)*groups*16 + n_inst*groups*8 bytes. */
#define T2V_GN_ROWS_PER_BLOCK 64

/* Device-side synchronisation words a program may hand to its ops: T2V_SYNC_INTS int32 arrival counters for the split-K fold
 * (GEMM p[7]) followed by T2V_SYNC_BARRIER_INTS more for the two-level grid barrier of the single-pass GroupNorm (GROUPNORM
 * p[5] points at the first of them).  All zero before the first launch; the kernels leave them zero (counters) or monotonic
 * (barrier generation).  They must not alias any buffer an op of the program writes.  t2v_sync_reset() zeroes the region on a
 * stream (call it when the program is bound to an arena, before the first run — never while a run is in flight). */
#define T2V_SYNC_INTS 4096
#define T2V_SYNC_BARRIER_INTS 512
#define T2V_GN_PART_BYTES 2097152 /* bytes of the statistics-exchange scratch (GEMM p[10]) every fused-norm launch may use: the launcher sizes its row chunks by it */

#define T2V_OP_NI 32
#define T2V_OP_NF 8
#define T2V_OP_NP 12

/* One program record.  Field meaning per kind:
 *
 * GEMM:  out[M,N] = epi( gather(A)[M,K] * W[N,K]^T )       fp16 operands, fp32 accumulate
 *   i: 0 M, 1 N, 2 K, 3 lda, 4 ldw, 5 ldc, 6 ldr, 7 gather, 8 Hin|F, 9 Win|HW, 10 Cin,
 *      11 stride, 12 upsample, 13 Hout, 14 Wout, 15 rows_per_batch, 16 epilogue,
 *      17 out dtype, 18 act (0 none, 1 SiLU, 2 ReLU), 19 split_k, 20 bias_along_m, 21 ldrb,
 *      22 tile (0 = 128x128-class kernel; 1 256x256, 2 256x320, 3 128x256 (8 waves, 3-stage ring), 4 / 5 128x128 with a 4-deep
 *         ring on 4 / 8 waves, 8 / 9 192x320 / 192x256 on 12 waves, 10 = 192x192 on 12 waves, T2V_EPI_TATTN only; 11 = 128x320
 *         on 8 waves, 12 = 64x64 on 4 waves with a 4-deep ring; any other id is refused; which tile has which fused epilogue:
 *         T2V_TILES in csrc/t2v_kernels.h, the table the library dispatches and validates from),
 *      23 tconv halo (input rows are [clip][F+2][HW]: one halo frame either side, T-sharding);
 *         for CONV3X3: 1 = zero padding (0,1,0,1) instead of (1,1,1,1) (LDM encoder Downsample, taps at +0..+2)
 *      30 = R > 0 (ABI 11; every gather mode, split-K allowed, plain / statistics / GroupNorm epilogues): the residual has R rows and row
 *         m >= R reads residual row m - R (M <= 2 R) — an adapter feature shared by the cond | uncond pair as the residual of a convolution;
 *      PLAIN gather only: 12 = R > 0 -> the residual has R rows and row m >= R reads residual row m - R; 13 = R > 0 -> likewise for the A
 *         operand (M <= 2R, no split-K): tensors shared by the cond | uncond pair of a guided step are computed once and wrapped;
 *      PLAIN gather only: 11 = 1 -> hi + lo fp16 output (fp16 out, plain epilogue, ldc >= 2N): out[m, N + n] = fp16(v - float(fp16(v)))
 *         beside out[m, n] = fp16(v) — a consumer GEMM over rows [hi | lo] with weights [W | W] (K = 2N) sees v with ~22 bits;
 *      PLAIN gather only: 8 = 1 -> fused LayerNorm second output (tile 8 or 11, N == 320, fp32 out, no split-K): p[7] fp16 [M, i[9]] =
 *         LayerNorm(out row, eps f[0]) * gamma + beta with p[3] = fp32 [2N] gamma | beta (instead of a row bias)
 *   p: 0 A fp16, 1 W fp16 [N,K], 2 bias fp32 [N] (or [M] if bias_along_m), 3 rowbias fp32
 *      [M/rows_per_batch, ldrb], 4 residual fp32 [M,ldr], 5 out, 6 split-K workspace fp32 [split_k, M, N],
 *      7 split-K (epilogue NONE): T2V_SYNC_INTS zeroed int32 tile tickets -> the last workgroup of a tile to arrive folds the
 *        slabs in split order and applies the epilogue (no reduction launch); 0 -> a reduction kernel follows;
 *      8 .. 11 and i[24 .. 29], f[2]: T2V_EPI_GN (above)
 *   Fused feed-forward pair (plans only; env T2V_FF_FUSE, read once, default on; 0 = off): when a plan is created, records k, k + 1 that
 *      are a GEGLU GEMM (plain gather, no split-K, N = 2560, K = 320, fp16 out, nothing but a bias) and a projection whose A operand is
 *      EXACTLY that result (same pointer, leading dimension and M; plain gather and epilogue, no split-K, N = 320, K = 1280, no fused
 *      norm) run as ONE launch, bit-identical to the two, provided M >= 49152, the result not lying over the GEGLU GEMM's operands, and no later record of the plan reaches — by the extent of
 *      any of its pointer slots, a window that starts below the tensor included — into bytes of the hidden tensor that no record has rewritten since.  THE HIDDEN BUFFER (record k's p[5]) IS NOT WRITTEN BY A FUSED PAIR.
 *      t2v_plan_run_timed reports the launch on record k and exactly 0.0f on record k + 1.  t2v_run_ops never fuses.
 *      i[31] = 1 on the GEGLU record (a word no validation reads; test hook): the M cut-off is waived.
 *   3x3 convolutions, stride 1, width <= 32 (env T2V_CONV_HALO, read once, default on; 0 = off): the A operand is staged once per 64-channel
 *      chunk for all nine taps instead of tap by tap; bit-identical.  i[31] = 1 on a CONV3X3 record (test hook): tap by tap for that record.
 * GROUPNORM: i: 0 n_inst, 1 rows_per_inst, 2 C, 3 ld_in, 4 groups, 5 in dtype, 6 silu,
 *      7 ld_out, 8 phase (0 whole op | 1 statistics only | 2 fold gathered parts + normalise | 3 statistics from the producing GEMM:
 *         p[6] = its T2V_EPI_STATS strips fp32 [n_inst * rows / 32][2][i[17]], rows % 32 == 0 — a fold of the strips + ONE apply pass),
 *      9 nparts, 10 this rank's part, 11 rows per workgroup (0: T2V_GN_ROWS_PER_BLOCK; sizes the scratch),
 *      12 single-launch variant (phase 0 only, (C/groups) % 4 == 0): one workgroup per (instance, group);
 *      14 rows of the whole instance over all parts (0 = rows * nparts; T-sharded clips with uneven slices);
 *      15 single-PASS cooperative variant allowed (phase 0, groups <= 32, p[5] given): grid <= one workgroup per CU, the tensor
 *         is read once into registers, statistics meet at a grid barrier (p[5] = T2V_SYNC_BARRIER_INTS zero-initialised uint32 words); the library
 *         uses it when the instance chunks fit (else the launches above on the same scratch);
 *      16 = 1 (phases 0 / 2, ld_out >= 2C): hi + lo operand split — the low-order fp16 image fp16(y - float(fp16(y))) of every output
 *         value goes to column C + c of the same output row (consumer: a GEMM with K = 2C against weights [W | W]);
 *      21 / 22 (phase 2, n_inst == 1): rows in front of / behind x that are normalised with the same statistics and written in front of /
 *         behind `out` — the neighbours' RAW boundary frames of a halo-padded buffer (T2V_OP_STATS_HALO); i[1] stays this rank's own rows
 *         (it sizes the scratch), i[14] the rows the statistics cover;
 *      scratch, phase 0: block partials [n_inst][nblk][groups][2] fp64, then {mean, rstd} fp32;  phases 1 / 2: gathered parts
 *      [nparts][n_inst][groups][2] fp64 (phase 1 folds this rank's block partials into its part; ALLGATHER of
 *      n_inst*groups*16 bytes per part), then this rank's block partials, then {mean, rstd};
 *      f: 0 eps;  p: 0 x, 1 gamma, 2 beta, 3 out fp16, 4 scratch, 5 grid-barrier words (i[15]), 6 producer strips (phase 3),
 *      8 (optional; phases 0 / 2 / 3) second output: the RAW input as fp16 [n_inst * rows, i[19]] (+ its low-order image at column i[20] > 0) — the
 *        operand of a 1x1 convolution that reads the same tensor (ResBlock skip_connection beside in_layers, t2v_model.py:965)
 *      7 (i[15], optional) exchange-record region of i[18] bytes that nothing but fused-norm launches ever writes (zero at bind time): the
 *        single-pass kernel then exchanges TAGGED records (no grid barrier) — the same region GEMM p[10] names
 * LAYERNORM: i: 0 M, 1 C, 2 ld_in, 3 ld_out, 4 workgroup cap (0 = 2048; rows beyond 4 x cap are walked grid-stride); f: 0 eps;
 *      p: 0 x fp32, 1 gamma, 2 beta, 3 out fp16
 * ATTENTION: i: 0 nq, 1 nk, 2 heads, 3 batch_outer, 4 batch_inner, 5..7 q strides (seq,
 *      outer, inner), 8..10 k/v strides, 11..13 out strides (elements; head h at +head_dim*h),
 *      14 head_dim (0 = 64), 15 causal (1: key s visible to query t iff s <= t), 16 low-order output offset (elements, 0 = none): also
 *      store fp16(o - float(fp16(o))) at out + i[16] — rows [hi | lo] for a K-doubled output projection;  f: 0 scale; p: 0 q, 1 k, 2 v, 3 out (all fp16)
 *      ABI 7, optional: p 6 = scratch fp16 [batch_outer * batch_inner * heads * 64, i[17]] with i[17] = nk rounded up to a multiple of 64
 *      (head_dim 64, not causal): V is transposed into it once per launch and the K / V^T tiles are staged by LDS-DMA (same bits as without
 *      the scratch; pays from ~512 keys); i[18] = waves per 64-key tile (0 = 8 | 4 | 8)
 *      Second role, optional (all zero = none): i[19] = alt_from (0 < alt_from < batch_outer), i[20] = its key count, i[21] = its K / V stride
 *      per outer sample (elements), p[4] / p[5] = its K / V bases — outer samples s >= alt_from attend to i[20] keys at
 *      p[4] / p[5] + (s - alt_from) * i[21] + inner * i[10] (sequence stride i[8] as the first role); everything else as for the other
 *      samples, in the same launch (the cond | uncond pair of a guided step whose prompts have different lengths).  Not for causal
 *      launches, the p[6] scratch path or RELPOS_ATTN: refused at plan creation.
 *      Per-sample table, optional (all zero = none; ABI 11, additive): i[22] = rows of the table (== batch_outer), i[23] = the largest
 *      key count in it, i[24] = the K / V rows it spans (every row: first + count <= i[24]), p[7] = the table, int32 [batch_outer][2] =
 *      {key count, first row} in device memory that nothing writes while the record runs (program data: the lowering keeps it in the
 *      packed weight image) — outer sample s attends to table[s][0] keys at p[1] / p[2] + table[s][1] * i[8] + inner * i[10]: one key
 *      count and one K / V location per sample, the text contexts of a batch of different prompts packed one after another without
 *      padding.  i[1] and the outer K / V stride i[9] are not read (i[1] > 0 as always; the lowering stores i[23] there); sequence
 *      stride, inner stride, heads and everything else as for a plain record, in the same launch; the kernel variant is chosen by i[23].
 *      A table row outside what i[23] / i[24] allow gives that sample NaN, never a read outside the i[24] rows.  Not together with the
 *      second role, causal launches, the p[6] scratch path or RELPOS_ATTN; a null table, i[22] != batch_outer, i[23] <= 0 or
 *      i[24] < i[23] likewise: refused, with a message, before anything is launched.  A record without the table runs the code it ran.
 * RELPOS_ATTN: i: as ATTENTION with nk == frames of the clip (<= 32 for i[17] = 0 | 1 | 2; <= T2V_RELPOS_MAX_FRAMES for i[17] = 3),
 *      14 head_dim (multiple of 8, <= 160; 40 | 64 | 80 | 160 for i[17] = 3),
 *      15 max relative position R, 16 q_off: the nq queries are frames [q_off, q_off + nq) of the clip (nq == nk, q_off == 0
 *      unless the clip is T-sharded: then s - t below is s - (t + q_off)); 17 = 1: use the MFMA kernel where it applies (nq == nk,
 *      q_off == 0, nk - 1 <= R <= 31, head_dim 40 | 64 | 80 | 160; the relative tables are staged as fp16) — else the VALU kernel;
 *      17 = 2 (round 5): the persistent MFMA kernel for whole clips of nk <= 16 frames (nq == nk, q_off == 0, R >= nk - 1, same head
 *      dims), with the tables ALSO given packed for it: p[6] = fp16 [32][DK] rows jl = Ek[jl + R - (nk-1)] (DK = head_dim rounded up
 *      to 16; zero beyond the table / head_dim), p[7] = fp16 [DV][32] = Ev transposed, column jl = Ev[jl + R - (nk-1)] (DV = head_dim
 *      rounded up to 32) — where it does not apply the VALU kernel runs on p[4], p[5];
 *      17 = 3 (ABI 9): the MFMA kernel for clips of ANY length 1 <= nk <= T2V_RELPOS_MAX_FRAMES, any R >= 0, T-sharded queries (any
 *      nq <= nk, q_off), head_dim 40 | 64 | 80 | 160 — the only kernel for nk > 32; no fall-back: its tables are REQUIRED packed for it:
 *      p[6] = fp16 [2R+1][DK] = Ek (zero columns beyond head_dim), p[7] = fp16 [DV][T2V_RELPOS_LONG_COLS(R)] = Ev transposed with
 *      replicated edges: column c = Ev[clamp(c - T2V_RELPOS_LONG_PADL, 0, 2R)] (zero rows beyond head_dim);
 *      18 low-order output offset (as ATTENTION i[16]);  f: 0 scale;  p: 0 q, 1 k, 2 v, 3 out (fp16), 4 Ek fp32 [2R+1, head_dim],
 *      5 Ev fp32 [2R+1, head_dim]:  sim[t,s] = scale * q[t].(k[s] + Ek[clip(s-t)]),
 *      out[t] = sum_s softmax_s(sim)[t,s] * (v[s] + Ev[clip(s-t)])   (attention_temporal.py:107-144)
 * SOFTMAX: i: 0 rows, 1 cols, 2 ld_in, 3 ld_out; f: 0 scale; p: 0 in fp32, 1 out fp16
 * NCTHW_TO_CL: i: 0 B, 1 C, 2 F, 3 HW, 4 ld_out, 5 in dtype, 6 samples in the source (0 = B; fewer: output sample b reads
 *      source sample b % i[6] — the cond | uncond pair of a guided step shares x_t); f: 0 scale; p: 0 in, 1 out fp16,
 *      2 (optional) low-order fp16 image, same layout: out_lo = fp16(v - float(fp16(v))) — hi + lo operand split of a consumer GEMM;
 *      i[7] = 1 (ld_out >= 2C): the low-order images are written into channels C .. 2C-1 of the same row instead (a consumer whose
 *      weights repeat W for those channels computes (hi + lo) . W in one pass)
 * CL_TO_NCTHW: i: 0 B, 1 C, 2 F, 3 HW, 4 ld_in, 5 out dtype; p: 0 in fp32, 1 out
 * TIME_EMBED: i: 0 B, 1 dim; p: 0 t fp32 [B], 1 freqs fp32 [dim/2], 2 out fp16 [B,dim]
 * COPY2D: i: 0 rows, 1 cols, 2 ld_src, 3 ld_dst, 4 src dtype, 5 dst dtype, 6 act (0 none, 1 SiLU, 2 GELU(erf),
 *      3 quick-GELU x*sigmoid(1.702x)); p: 0 src, 1 dst, 2 (optional, fp32 -> fp16 only) low-order fp16 image of the cast, ld_dst
 * DDIM_STEP: i: 0 C (= samples * channels), 1 inner (F*h*w), 2 guided channels (per sample), 3 eps dtype, 4 x dtype, 5 mode,
 *      6 channels per sample (0 = C: one video per batch); x [samples, channels, inner], eps [2, samples, channels, inner];
 *      mode 0 (DDIM_Gaussian, gaussian_sampler.py:103-108,199-211,269-283):
 *        f: 0 sqrt_recip_ac, 1 sqrt_recipm1_ac, 2 sqrt(a_prev), 3 dir coef, 4 sigma (masked), 5 guidance scale
 *      mode 1 (LDM DDIM, samplers/ddim/sampler.py:197-219):  x0 = (x - f0*e)/f1;  out = f2*x0 + f3*e + f4*noise
 *        f: 0 sqrt(1-a_t), 1 sqrt(a_t), 2 sqrt(a_prev), 3 sqrt(1-a_prev-sigma^2), 4 sigma, 5 guidance scale
 *      p: 0 xt, 1 eps pair, 2 noise, 3 out
 *      i[7] = 1 (mode 1, fp32 x): the known-region blend of a masked step (lvdm/samplers/ddim.py:188-195) in the same launch, after
 *        the update above (eta noise included), in fp32 and in the reference's order:
 *          known = f6 * x0 + f7 * qnoise;   out = known * mask + (1 - mask) * out
 *        f: 6 sqrt_alphas_cumprod[t'], 7 sqrt_one_minus_alphas_cumprod[t'] (t' = step - 1: q_sample of the known content)
 *        p: 4 known x0, 5 mask, 6 q-noise (may be null when f7 == 0) — fp32, dense, shaped like x [samples, channels, inner]
 *        i[7] = 0: p[4..6] and f[6..7] are not read
 *      i[8] (mode 0, fp32 x, i[7] = 0): restriction of x0 before the update continues from it (restrict_range_x0, gaussian_sampler.py:110-120);
 *        all of it in fp32 with every operation rounded by itself, as the reference's tensor arithmetic
 *          0  none — p[7..8] and f[6..7] are not read (unless i[9] = 1), the record is the plain step
 *          1  x0 = clamp(x0, -f6, f6)                      (a NaN stays a NaN, as torch.clamp)
 *          2  x0 = min(s, max(-s, x0)) / s,  s = table[sample][0] read from p[7]   (NaN in s or x0 -> NaN, as torch.min / torch.max)
 *          3  the MEASURE pass: writes table[sample] = {max(q, 1), q, v_lo, v_hi} (four fp32) into p[7] for every sample and nothing else
 *             (p[3] may be null, p[2] is not read).  Over the n = channels * inner values |x0| of a sample (x0 recomputed from x and the eps
 *             pair exactly as the apply pass computes it; -0.0 counts as 0, +-inf are ordinary values): rank = f6 * (float)(n - 1) in fp32,
 *             v_lo / v_hi = the order statistics floor(rank) / ceil(rank), w = rank - floor(rank),
 *             q = w < 0.5 ? v_lo + w (v_hi - v_lo) : v_hi - (v_hi - v_lo)(1 - w)  — torch.quantile(|x0|, f6) on fp32, by an exact integer radix
 *             select (no floating-point accumulation: the result does not depend on scheduling); a NaN in the sample gives q = s = NaN.
 *             n <= 16 777 216 (torch.quantile's limit), f6 = float32(percentile) in (0, 1]
 *        f: 6 clamp bound (i[8] = 1) or percentile (i[8] = 3);  p: 7 threshold table fp32 [samples, 4] (i[8] = 2 reads, 3 writes)
 *      i[9] = 1 (mode 0, fp32 x, i[7] = 0): the classifier-guidance term of get_eps (gaussian_sampler.py:199-211), after the restriction and
 *        eps = (f0 x - x0) / f1:   eps -= f7 * g;   x0 = f0 x - f1 eps;   then the update as above
 *        f: 7 sqrt(1 - a_t);  p: 8 g = condition_fn(x_t, t), fp32, dense, shaped like x
 *      mode 2 (UniPC's thresholded data prediction, uni_pc/uni_pc.py:351-364 with the guidance combine of :304-307; fp32 x, i[7] = i[9] = 0):
 *          e = eu + f5 * (ec - eu)  (i[2] = channels per sample: guided; 0: e = ec);   x0 = (x - f0 * e) / f1
 *        in fp32 with every operation rounded by itself.  The record is one of two passes, both over that x0:
 *          i[8] = 3  the MEASURE pass exactly as in mode 0 (same select, same rank arithmetic, same table row), quantile f6
 *          i[8] = 2  out = min(max(x0, -s), s) / s,  s = table[sample][0]   (torch.clamp with tensor bounds; NaN in s or x0 -> NaN)
 *        i[8] = 0 | 1 are refused: the plain data prediction is a LINCOMB, and the class has no clamp.  n = channels * inner <= 16 777 216.
 *        f: 0 sigma_t, 1 alpha_t, 5 guidance scale, 6 quantile (i[8] = 3);  p: 0 x, 1 eps pair, 3 out (i[8] = 2), 7 table [samples, 4]
 *      mode 3 (DDIM inversion, one step of DDIMSampler.encode, samplers/ddim/sampler.py:242-254; fp32 x, i[7] = i[8] = i[9] = 0 or refused):
 *          e = eu + f5 * (ec - eu)  (i[2] = channels per sample: guided; 0: e = ec, the unconditional half is not read);
 *          out = f0 * x + f1 * e
 *        in fp32 with every operation rounded by itself: both products, then their sum.  i[2] between 0 and the channel count is refused.
 *        f: 0 sqrt(a_next / a), 1 sqrt(a_next) * (sqrt(1 / a_next - 1) - sqrt(1 / a - 1)), 5 guidance scale
 *        p: 0 x fp32, 1 eps pair (fp16 or fp32), 3 out fp32, 4 (optional) a second fp32 destination that receives the same values — the
 *           intermediate a caller keeps, at no extra launch; p[2] is not read.  Four elements per thread with 128-bit accesses when
 *           every pointer is 16-byte aligned, one element per thread otherwise.
 *      mode 4 (DDIM_Gaussian with the keyframe blend of the legacy img2vid loop, modelscope/t2v_model.py:1555-1562; fp32 x, the eps pair fp16
 *        or fp32, i[2] as in mode 0, i[7] = i[8] = i[9] = 0 or refused): the mode-0 update x1 — bit for bit what the mode-0 record gives
 *        on the same operands, eta noise included — and, in the same launch,
 *          bin = mask <= v ? 0 : 1  (fp32 comparison; a NaN weight compares false: free);   known = f6 * orig + f7 * n;
 *          out = known * (1 - bin) + x1 * bin
 *        in fp32 with every operation rounded by itself (both products, then their sum, twice).  Arithmetic, not a select: a non-finite
 *        value on either side reaches out, as in torch.  Weight 1 means free, weight <= v means reset to the re-noised original.
 *        f: 0..5 as mode 0, 6 sqrt_alphas_cumprod[t'], 7 sqrt_one_minus_alphas_cumprod[t'] (t' = the next step's timestep)
 *        i: 10 the bits of the fp32 threshold v (a word that every other DDIM_STEP record leaves zero)
 *        p: 0 x, 1 eps pair, 2 eta noise, 3 out, 4 the original latent, 5 the mask, 6 the blend noise n (may be null only when f7 == 0;
 *           read whenever it is given) — p[4..6] fp32, dense, shaped like x [samples, channels, inner].  Four elements per thread with
 *           128-bit accesses when every pointer that is read is 16-byte aligned, one element per thread otherwise.
 * LINCOMB: i: 0 n elements, 1 n terms (<= 6), 2 out dtype, 3..8 term dtypes; f: 0..5 coefficients;
 *      p: 0..5 terms, 6 out;  i[9] = 0 (every record before the context windows leaves it zero).
 *      The two context-window forms live here because the blend IS a linear combination, with a per-frame coefficient table instead of
 *      f[0..5], and the gather is its transpose; the kind, its output slot p[6] and the ABI stay what they were.  Both share
 *        i: 0 V videos, 1 C channels, 2 dtype of p[0] (fp16 | fp32), 3 F frames of the clip, 4 HW pixels per frame, 5 window length
 *           (2 .. F), 6 nW windows per video;  p: 1 starts, int32 [nW] on the device: window w holds frames starts[w] .. starts[w] + length - 1
 *      and batch row v * nW + w of a windowed forward is window w of video v (the window index runs fastest).  A start is clamped into
 *      [0, F - length] where it is read; the table is validated by the host that builds it (every frame in some window).
 *      form i[9] = 2, window gather: xw[r, c, j, :] = x[v, c, starts[w] + j, :] for the i[8] batch rows from row i[7] on, bit-exact.
 *        i: 7 first batch row, 8 rows (i[7] + i[8] <= V * nW);  p: 0 x [V, C, F, HW], 6 xw [i[8], C, length, HW] of the same dtype.
 *        16-byte units when HW * sizeof is a multiple of 16 and both bases are 16-byte aligned, one element per thread otherwise.
 *      form i[9] = 1, window blend: out[role, v, c, f, :] = (sum_w wgt[f - starts[w]] * e[role, v * nW + w, c, f - starts[w], :]) / (sum_w wgt[f - starts[w]])
 *        over the windows that hold frame f, in ascending w: acc = fma(wgt, e, acc) and wsum += wgt in fp32, then one division.  One
 *        thread per output, no atomics: the value depends on the eps values alone.
 *        i: 7 roles (2: [cond | uncond], 1: conditional only), 8 zero;  p: 0 e [roles, V * nW, C, length, HW] (dtype i[2]), 2 wgt fp32 [length],
 *        6 out fp32 [roles, V, C, F, HW] — the eps pair every DDIM_STEP record reads.  Four neighbours per thread (16-byte stores) when
 *        HW % 4 == 0 and the bases allow it, one element per thread otherwise.
 * MEMSET: i: 0 bytes (lo), 1 bytes (hi); p: 0 dst
 * EMBED_ROWS: out[r,:] = table[ids[r],:] + pos[r % L,:]   i: 0 rows, 1 width, 2 L, 3 vocab, 4 table dtype;
 *      p: 0 ids int32 [rows], 1 table [vocab,width], 2 pos fp32 [L,width], 3 out fp32 [rows,width]
 * TO_UINT8: out[f, y, i*W + x, c] = trunc(clamp(v*0.5 + 0.5, 0, 1) * 255), v = in[i*si + c*sc + f*sf + y*sy + x*sx]
 *      i: 0 NI (videos side by side), 1 C, 2 F, 3 H, 4 W, 5 in dtype, 6 arithmetic (0 fp32 | 1 every intermediate rounded
 *      to fp16, the reference's half-precision VAE path), 7 channel order reversed (RGB -> BGR), 8/9 si (lo, hi), 10 sc,
 *      11/12 sf (lo, hi), 13 sy, 14 sx (element strides), 15 form (0: the above);  p: 0 in, 1 out uint8
 *      form i[15] = 1 (torch_to_np, videocrafter/sample_utils.py:98-107): out[i, f, y, x, c] = trunc(clamp((v + 1) * 127.5, 0, 255)) — one
 *      [F, H, W, C] block per video instead of videos side by side.  fp32, `v + 1` and `* 127.5` each rounded by itself (no fma); +-inf -> 0 | 255,
 *      a NaN stores 0 (torch's cast is undefined there).  i[6] = 1: the input element is rounded to fp16 FIRST and the arithmetic stays fp32
 *      (an fp16 model's video under torch_to_np's `.float()`), not the fp16 chain of form 0.  i[7] must be 0.  Same strides, same byte extents.
 * ALLGATHER: part q of `nparts` equal parts lives at base + q*bytes; this rank's part is already in place.
 *      i: 0/1 bytes per part (lo, hi), 2 nparts, 3 this rank's part;  p: 0 base.   nparts == 1: no-op.
 * HALO_EXCHANGE: token buffer of F+2 frames (frame = `bytes`): frame 1 -> previous rank's frame F+1 slot ... i.e. this rank
 *      sends its first real frame to `prev` and its last to `next`, and receives their boundary frames into frame 0 / F+1.
 *      i: 0/1 bytes per frame (lo, hi), 2 F (local frames), 3 prev rank in the communicator (-1 none), 4 next rank (-1 none);
 *      p: 0 base.   The collectives need t2v_plan_set_comm unless they are no-ops.
 * STATS_HALO: ALLGATHER of the statistics parts and HALO_EXCHANGE of the RAW (not yet normalised) boundary frames as ONE group of
 *      point-to-point transfers: every rank sends its part (p0 + part*bytes) to every other rank; frame 1 of the halo-padded raw buffer
 *      p1 goes to `prev`, frame F to `next`, theirs arrive in frame 0 / F + 1.  The consumer (GROUPNORM phase 2 with i[21] / i[22]) then
 *      normalises its own frames AND the received ones with the same gathered statistics — bit-identical to what the neighbour wrote for
 *      itself — so a T-sharded temporal convolution costs one exchange instead of two (t2v_model.py:1202-1229).
 *      i: 0/1 bytes per statistics part (lo, hi), 2 nparts, 3 this rank's part, 4/5 bytes per frame (lo, hi), 6 F (local frames),
 *      7 prev rank (-1 none), 8 next rank (-1 none);  p: 0 gathered parts, 1 raw buffer of F + 2 frames
 * RESHARD_ROWS: row r reads src row (r / P) * S_src + r % P and writes dst row (r / P) * S_dst + r % P (+ residual at the dst row)
 *      i: 0 rows, 1 cols, 2 P (rows per chunk), 3 S_src, 4 S_dst (chunk strides in rows), 5 ld_src, 6 ld_dst, 7 dtype (src == dst;
 *      fp16: cols % 8 == 0, fp32: cols % 4 == 0), 8 ld_res;  p: 0 src, 1 dst, 2 residual fp32 (optional, fp32 only)
 *      ABI 8: i[9] = nparts > 1: that many regroupings of this shape in ONE launch — part q reads p0 + q*i[10] elements, writes p1 + q*i[11]
 *      elements (residual p2 + q*i[12]); part i[13] (-1: none) is the rank's own, which does not travel: its source (i[14] = 1) or its
 *      destination (i[14] = 0) is p3 instead (the R packs in front of a frames -> pixels ALLTOALL, the R unpacks behind the way back)
 * ALLTOALL: slice q of the clip holds cnt(q) frames (i[4] each, i[5] on the LAST slice); chunk = bytes of one frame's share for one
 *      rank.  direction 0 (frames -> pixels): send cnt(me) chunks to every peer q from p0 + q*cnt(me)*chunk, receive cnt(q) chunks
 *      from q at p1 + q*i[4]*chunk;  direction 1 (pixels -> frames): send cnt(q) chunks to q from p0 + q*i[4]*chunk, receive cnt(me)
 *      chunks from q at p1 + q*cnt(me)*chunk.  The rank's own part is moved by RESHARD_ROWS ops.
 *      i: 0/1 chunk bytes (lo, hi), 2 nparts, 3 this rank's part, 4 frames per slice, 5 frames of the last slice, 6 direction;
 *      p: 0 send base, 1 receive base
 * RESAMPLE (ABI 10): one pass of a separable resize of uint8 images src [N, H, W, 3] (interleaved RGB) along one axis, as Pillow's 8-bit
 *      resampler runs it (Resample.c, PRECISION_BITS 22; `Image.resize(..., Image.LANCZOS)` = a horizontal pass into a uint8 intermediate,
 *      then a vertical pass; a pass whose sizes are equal is left out by the host).  For output index o along the axis:
 *        acc = 2^21 + sum_{j < count(o)} src[first(o) + j] * coef[o][j]   (int32),   value = clamp(acc >> 22, 0, 255)   (arithmetic shift)
 *      axis 0: out [N, H, i[4], 3], o = output column;  axis 1: out [N, i[4], W, 3], o = output row.  first / count are clamped to the
 *      source axis and count to the table row length before use: a malformed table cannot make the kernel read outside the image.
 *      Output forms (i[7]): 0 = the uint8 value;  1 / 2 = lut[value] as fp32 / fp16 (the fp16 rounding of the fp32 entry) written as
 *      channels-last tokens [N * rows * columns, i[8]] with channels 3 .. i[8]-1 zeroed — with lut[u] = 2 * (u / 255) - 1 evaluated on
 *      the host in float32 (process_modelscope.py:129,137) the last pass writes the VAE encoder's entry buffer itself.
 *      i: 0 N, 1 H, 2 W (of the source), 3 channels (= 3), 4 output size along the axis, 5 axis (0 horizontal | 1 vertical),
 *      6 table row length (ksize), 7 output form, 8 ld of the token forms (>= 3);
 *      p: 0 src uint8, 1 dst, 2 coef int32 [i[4]][i[6]], 3 bounds int32 [i[4]][2] = {first, count}, 4 lut fp32 [256] (forms 1 / 2)
 *      i[9] = 0 (every record before this mode): all of the above.  i[9] = 1 (ABI 11): FLOAT BICUBIC mode — P planar single-channel images
 *      src [P, H, W] (fp16 | fp32) -> dst fp32 [P, Ho, Wo], both axes in ONE launch: torch's F.interpolate(mode="bicubic", align_corners=False)
 *      without antialiasing, enlarging or reducing (lvdm/models/ddpm3d.py:1443-1468: frames to the depth estimator's size, depth maps back).
 *      The host builds the tables (packing.bicubic_table, per axis, in float64, weights rounded once to fp32): for output index o,
 *        real = (in / out) * (o + 0.5) - 0.5 (not clamped at 0), i0 = floor(real), t = real - i0, taps i0 - 1 .. i0 + 2 each clamped to
 *        [0, in - 1], weights c2(t + 1), c1(t), c1(1 - t), c2(2 - t) with A = -0.75, c1(x) = ((A + 2) x - (A + 3)) x^2 + 1,
 *        c2(x) = ((A x - 5 A) x + 8 A) x - 4 A.
 *      One output (the arithmetic contract; tests/interp_bicubic.py mirrors it):
 *        out[p][y][x] = sum_{a = 0..3} wy[y][a] * ( sum_{b = 0..3} wx[x][b] * fp32(src[p][iy[y][a]][ix[x][b]]) )
 *      both sums in ascending order starting from the first product, EVERY multiply and add rounded to fp32 on its own (no contraction):
 *      bitwise reproducible, independent of the grid.  A NaN / inf source pixel reaches exactly the outputs whose 4 x 4 footprint names it
 *      (nothing is special-cased: 0 * NaN is NaN, as in torch).  The kernel clamps the table's indices to the image again before use: a
 *      malformed table cannot make it read outside the source.  No byte outside dst [P, Ho, Wo] is written.
 *      i: 0 P, 1 H, 2 W (of the source), 3 = 1 (channels), 4 Ho, 5 = 0, 6 = 4 (taps), 7 = 1 (fp32 out), 8 unused, 9 = 1, 10 Wo,
 *         11 input dtype (T2V_F16 | T2V_F32);  H * W and Ho * Wo <= 2^28, P * Ho * ceil(Wo / 256) <= 2^24 - 1 (one launch)
 *      p: 0 src, 1 dst fp32, 2 weights fp32: wy [Ho][4] followed by wx [Wo][4], 3 indices int32: iy [Ho][4] followed by ix [Wo][4]
 * DEPTH_TOKENS (ABI 11): out[(f*(H/8) + y/8)*(W/8) + x/8, (y%8)*8 + x%8] = fp16(v(f, y, x)) — nn.PixelUnshuffle(8) of n single-channel frames
 *      [n, 1, H, W] as channels-last tokens, the A operand of the adapter's conv_in (lvdm/models/modules/adapter.py:93-99).  With i[4] = 1
 *      v = 2 * (d - min_f) / (max_f - min_f + 1e-7) - 1 with the frame's own minimum / maximum (NaN if any pixel is NaN, as torch.amin / amax), evaluated in fp32 in that operation order
 *      (ddpm3d.py:1463-1464; a constant frame gives exactly -1); with i[4] = 0 v = d.  One workgroup per frame; the reduction uses wavefront
 *      shuffles and LDS.  Columns 64 .. i[5]-1 of the output rows are not written.
 *      i: 0 n frames, 1 H, 2 W (multiples of 8), 3 in dtype, 4 normalise, 5 ld_out (>= 64, multiple of 8);  p: 0 in, 1 out fp16 (16-byte aligned)
 * AVGPOOL2 (ABI 11): nn.AvgPool2d(2, 2) of n channels-last images: out[(f*Ho + y)*Wo + x, c] = 0.25 * (in[2y, 2x] + in[2y, 2x+1] + in[2y+1, 2x] +
 *      in[2y+1, 2x+1])[c] in fp32, Ho = H / 2, Wo = W / 2 (a last odd row / column is dropped, as torch does)
 *      i: 0 n images, 1 H, 2 W, 3 C (% 4 == 0), 4 ld_in, 5 ld of the fp32 output, 6 ld of the fp16 output;
 *      p: 0 in fp32, 1 out fp32 (optional), 2 out fp16 (optional; the fp16 rounding of the fp32 mean) — at least one
 * EMPHASIS: prompt emphasis of one batch of text-encoder chunks with the mean restored (clip_hardcode.py:413-420):
 *      out[r, c] = fp32(fp32(z[r, c] * m[r]) * ratio),  ratio = fp32(sum z / sum (z * m)), both sums over ALL rows and columns (the reference's
 *      z.mean() of the batch), accumulated in fp64 in a fixed order by ONE workgroup: results repeat bit for bit, and with every m = 1 the
 *      ratio is exactly 1.  A zero sum of z * m is not special-cased (IEEE inf / NaN, as the reference).
 *      i: 0 rows (B * L), 1 W (% 4 == 0), 2 ld of z, 3 ld of out (% 4 == 0), 4 dtype of z;  p: 0 z, 1 m fp32 [rows], 2 out fp32 (16-byte aligned)
 * FINGERPRINT (ABI 11, t2v_run_ops only: t2v_plan_create refuses it): out[s] = a 64-bit function of the bytes of segment s of a device table, every segment
 *      by itself.  A segment {address, nbytes} (both even, nbytes may be 0) is read as n = nbytes / 2 little-endian 16-bit words v_0 .. v_{n-1}:
 *          out[s] = sum_j v_j * (2 j + 1)  +  2^32 * sum_j v_j^2  +  (n + 1) * T2V_FINGERPRINT_LEN      (mod 2^64)
 *      One changed word always changes the value ((a - b) times an odd number is not 0 mod 2^64), two unequal words swapped too (2 (a - b)(j - k)),
 *      and equal bytes of different lengths differ by the last term.  Wrap-around integer adds only: bitwise reproducible, independent of the
 *      grid and of the alignment of the address.  The chunk table lists {uint32 segment, uint32 chunk} pairs: chunk c of segment s = its bytes
 *      [c * T2V_FINGERPRINT_CHUNK, (c + 1) * T2V_FINGERPRINT_CHUNK), one workgroup each; EVERY chunk of every segment exactly once, and chunk 0 of
 *      every segment (an empty one included: it carries the length term).  `out` is zeroed by the op (a memset on the stream), then one launch.
 *      i: 0 n segments, 1 n chunks (>= n);  p: 0 table: n x {uint64 address, uint64 nbytes}, 1 out uint64 [n], 2 chunk table: n chunks x {uint32, uint32} (all 8-byte aligned)
 * LORA_MERGE (ABI 11, t2v_run_ops only: t2v_plan_create refuses it): the Stable LoRA merge (stable_lora/stable_utils/lora_processor.py:50-101) of every
 *      weight of a device table in ONE launch, in place.  A segment = one weight W, row-major [N, J] of dtype T (T2V_F16 | T2V_F32), with its factors
 *      A [r, Jf] and B [N, r] (row-major, dtype T).  Per element, every step rounded once to T (the arithmetic contract):
 *          d = T(sum over ascending k of B[n, k] * A[k, j'])            fp32 accumulation (fp16 factors: every product is exact in fp32)
 *          T2V_LORA_DIRECT   (Jf = J):    j' = j
 *          T2V_LORA_TEMPORAL (Jf = 3 J):  d = T((d(3 j) + d(3 j + 1) + d(3 j + 2)) / 3), summed in fp32 in that order, IEEE division
 *          e = T(fp32(d) * f[0]);   W[n, j] = T(fp32(W[n, j]) + fp32(e))
 *      Un-merging is the same record with -f[0] (x - y is x + (-y)).  Any r >= 1 (a loop over k).  W, A and B may sit at any element-aligned address;
 *      16-byte accesses are used where the addresses allow.  No byte outside [W, W + N J) is written.  The tile table lists {uint32 segment, uint32 tile}
 *      pairs: tile t of segment s = its elements [t * T2V_LORA_TILE, (t + 1) * T2V_LORA_TILE) of the flat row-major weight, one workgroup each; EVERY
 *      tile of every segment exactly once (a tile listed twice is merged twice), and the segments of one table must not overlap (the host's check).
 *      segment record (48 bytes): {uint64 W, uint64 A, uint64 B, int32 N, int32 J, int32 r, int32 form, int32 dtype, int32 0}
 *      i: 0 n segments, 1 n tiles (>= n);  f: 0 alpha;  p: 0 segment table, 1 tile table: n tiles x {uint32, uint32} (both 8-byte aligned)
 * FREEU (ABI 11, additive): FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net") at ONE decoder skip concatenation — the reference's
 *      torch.cat([x, xs.pop()], dim=1), t2v_model.py:444 — in place on the fp32 channels-last concat buffer X [rows, ld], rows = frames * h * w
 *      (row = (frame * h + y) * w + x), whose columns [0, C_h) hold the stream and [C_h, C_total) the skip.  One launch:
 *        X[:, 0 .. C_h/2)      *= f[0]                      one fp32 multiply per element
 *        X[:, C_h/2 .. C_h)    untouched, as every column >= C_total (ld > C_total is fine) and every byte outside the buffer
 *        X[:, C_h .. C_total)   = fourier_filter(., scale f[1], threshold 1) per (frame, channel) plane [h, w]:
 *          V = fftshift(fftn(v));  V[h/2 - 1 : h/2 + 1, w/2 - 1 : w/2 + 1] *= scale  (Python slices);  out = real(ifftn(ifftshift(V)))
 *        i.e. the frequency bins u in {-1, 0} x v in {-1, 0}, taken as DISTINCT indices modulo the axis length (an axis of length 1 has one
 *        bin, an axis of length 2 both of its bins), are scaled — evaluated in closed form, no FFT:
 *          out(y, x) = v(y, x) + (scale - 1) / (h w) * sum_bins ( Re c cos(theta) - Im c sin(theta) ),
 *          theta = 2 pi (u y / h + v x / w),  c = sum_{y, x} v(y, x) e^{-i theta}
 *        with the sums and the correction in fp64 and ONE rounding to fp32 at the store.  f[0] = f[1] = 1 leaves every finite value as it
 *        was.  Sums are taken in a fixed order without atomics: results repeat bit for bit.  A non-finite value reaches the (frame,
 *        channel) plane it sits in and no other.  16-byte accesses when X is 16-byte aligned, ld % 4 == 0, C_h % 8 == 0 and
 *        (C_total - C_h) % 4 == 0; one element per lane otherwise.
 *      i: 0 rows, 1 C_total, 2 ld (>= C_total), 3 C_h (even, 0 < C_h <= C_total), 4 frames, 5 h, 6 w (h, w <= 1024; rows == frames * h * w);
 *      f: 0 b, 1 s (both finite);  p: 0 X fp32 (4-byte aligned).  Anything else is refused, with a message, before anything is launched.
 */
typedef struct t2v_op {
  int32_t kind;
  int32_t tag;                 /* free for the host (debug id) */
  int32_t i[T2V_OP_NI];
  float f[T2V_OP_NF];
  uint64_t p[T2V_OP_NP];
} t2v_op;

typedef struct t2v_plan t2v_plan; /* opaque: a validated copy of a program */

/* library / device */
int t2v_abi_version(void);
const char* t2v_last_error(void);
/* fills name (<= len bytes), number of CUs and total HBM bytes of the current HIP device */
int t2v_device_info(char* name, int len, int* compute_units, uint64_t* hbm_bytes);

/* Asynchronous faults.  The single-pass GroupNorm synchronises its workgroups with a grid barrier; the library only launches it when
 * the occupancy API says the whole grid is co-resident, and the wait is bounded: a workgroup that sees no release within 0.25 s
 * (another client of the device holds compute units) raises a flag in host-mapped memory and falls through instead of hanging the
 * device.  The run in flight then produced invalid results; the NEXT t2v_run_ops / t2v_plan_run* call returns T2V_ERR_ASYNC (once)
 * and the three-launch GroupNorm is used for the rest of the process.  t2v_async_status() reports the same condition without running
 * anything (call it after synchronising the stream at the end of a job): T2V_OK or T2V_ERR_ASYNC. */
int t2v_async_status(void);
/* test hook: the next `n` fused-norm launches (single-pass GroupNorm, T2V_EPI_GN, cross-tile LayerNorm) wait for exchange records that
 * nobody publishes — every waiter gives up after 0.25 s and the asynchronous fault is reported as above.  Never call it in production. */
void t2v_debug_poison_exchange(int n);
/* zero the T2V_SYNC_INTS + T2V_SYNC_BARRIER_INTS int32 words at `sync_words` on `stream` */
int t2v_sync_reset(void* sync_words, void* stream);

/* Execute `n` ops in order on `stream` (a hipStream_t; null = default stream). */
int t2v_run_ops(const t2v_op* ops, int n, const uint64_t* ext, int n_ext, void* stream);

/* Plans: validate + copy a program once, run it many times. */
int t2v_plan_create(const t2v_op* ops, int n, t2v_plan** out);
int t2v_plan_num_ops(const t2v_plan* plan);
/* records minus the feed-forward pairs that run as one launch (the GEMM section above): what the plan-time recognition decided */
int t2v_plan_num_launches(const t2v_plan* plan);
int t2v_plan_run(t2v_plan* plan, const uint64_t* ext, int n_ext, void* stream);
/* Same, bracketing every op with HIP events on `stream`; ms[i] = duration of op i.
 * Synchronises the stream.  Used by bench.py for the live roofline measurement. */
int t2v_plan_run_timed(t2v_plan* plan, const uint64_t* ext, int n_ext, void* stream, float* ms);
void t2v_plan_destroy(t2v_plan* plan);

/* Communicators (T-axis sharding, one process per GPU): RCCL is dlopen'ed on first use, the library itself does not link
 * it.  Rank 0 of a group calls t2v_comm_unique_id and hands the 128 bytes to the others out of band (the host uses
 * torch.distributed's store); every rank then calls t2v_comm_create on its own device.  Collective ops of a plan run on
 * the launch stream, in program order with the kernels: a sharded UNet forward is ONE host call. */
typedef struct t2v_comm t2v_comm;
int t2v_comm_unique_id(unsigned char id[128]);
int t2v_comm_create(const unsigned char id[128], int nranks, int rank, t2v_comm** out);
int t2v_comm_size(const t2v_comm* comm);
void t2v_comm_destroy(t2v_comm* comm);
int t2v_plan_set_comm(t2v_plan* plan, t2v_comm* comm);   /* borrowed; must outlive the plan's runs */
/* Peer windows (ABI 8, csrc/comm.hip): device-initiated exchanges instead of RCCL calls.  Every rank creates a window on its
 * communicator (memory of the library on the current device; each message gets one of two slots of `slot_bytes` per peer) and
 * receives its 64-byte hipIpcMemHandle; the host gathers the handles of all ranks ([nranks][64], communicator order — the reference's
 * launcher has the same out-of-band channel, ddp_wrapper.py:9-13) and every rank opens them.  From then on a collective op of a plan
 * (and t2v_comm_all_gather) whose largest message fits a slot is ONE kernel of this library: workgroups store their share of the
 * message into the peer's window over xGMI, raise a sequence flag there, and wait (bounded: T2V_PEER_TIMEOUT_MS, default 20 s ->
 * T2V_ERR_ASYNC at the next call) for the peer's flag in their own window.  Larger ops keep going through RCCL.
 * t2v_comm_window_open(comm, NULL) releases the window again (the group found a rank that could not map a peer: nobody uses them).
 * t2v_comm_counters: out[0] = exchanges that went over the window, out[1] = exchanges that went through RCCL since creation. */
int t2v_comm_window_create(t2v_comm* comm, uint64_t slot_bytes, unsigned char handle_out[64]);
int t2v_comm_window_open(t2v_comm* comm, const unsigned char* handles);
void t2v_comm_counters(const t2v_comm* comm, uint64_t out[2]);
/* "uncached" | "finegrained" | "default": the kind of device memory the window got (uncached first — peers write it through the fabric and
 * this device polls it, so its L2 must not keep lines of it; T2V_PEER_WINDOW_MEM forces one); "" without a window */
const char* t2v_comm_window_kind(const t2v_comm* comm);
/* In-place all-gather outside a plan, on `stream`: part q of t2v_comm_size(comm) equal parts of `bytes` bytes lives at base + q*bytes,
 * the caller's own part is in place.  The per-step exchanges around the UNet — the eps of a classifier-free-guidance pair
 * (gaussian_sampler.py:161-163 evaluates the two forwards one after the other), the uint8 frames of the decoded clip
 * (lvdm/utils/dist_utils.py:13-19) — use it, so a sharded run's data path has ONE collective stack.
 * `base` needs no alignment: a gather the peer window carries (16-byte units) from a base off 16 bytes runs on an aligned copy owned by
 * the communicator (two extra device copies on `stream`); use one stream per communicator for such gathers.  The collective ops of a
 * PLAN are different: their buffers must be 16-byte aligned when a window is open (arena offsets are), else T2V_ERR_BAD_ARG. */
int t2v_comm_all_gather(t2v_comm* comm, void* base, uint64_t bytes, void* stream);

/* Drop-in entry points for the reference's call sites (thin wrappers over t2v_plan_run that
 * fix the external-slot convention):
 *   t2v_unet_forward  <->  eps = UNetSD.forward(x, t, y)      t2v_model.py:386
 *   t2v_vae_decode    <->  img = AutoencoderKL.decode(z)      t2v_model.py:1646
 *   t2v_ddim_step     <->  loop body of GaussianDiffusion.sample  gaussian_sampler.py:257-283 */
int t2v_unet_forward(t2v_plan* plan, const void* x, const float* t, const void* ctx, void* eps_out,
                     void* stream);
int t2v_vae_decode(t2v_plan* plan, const void* z, void* img_out, void* stream);
int t2v_ddim_step(t2v_plan* plan, const void* xt, const void* eps_pair, const void* noise,
                  void* xt_out, const float coef[6], void* stream);

#ifdef __cplusplus
}
#endif
#endif /* T2V_HIP_H */
