// C-ABI of libt2v_hip.so (see include/t2v_hip.h): validates a denoise program and executes it
// by launching the HIP kernels of this directory on the caller's stream.  No torch types, no
// allocation on the data path, no CPU fallback: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "t2v_kernels.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

inline bool resolve_ptrs(t2v_op& op, const uint64_t* ext, int n_ext) {
  for (int k = 0; k < T2V_OP_NP; ++k) {
    const uint64_t v = op.p[k];
    if (v != 0 && v < T2V_EXT_SLOTS) {
      if ((int)v >= n_ext || ext == nullptr) return false;
      op.p[k] = ext[v];
    }
  }
  return true;
}

// ---- the GEMM record, decoded once -------------------------------------------------------------------------------------------------------
// What a T2V_OP_GEMM record is, or why it is none (include/t2v_hip.h): gemm_decode is the ONE function that reads the record's words and
// pointer slots — i[8..14], i[24..28], p[3], p[7], p[8], p[9] mean different things under different gathers and epilogues.  Validation,
// the parameter block, the slot extents, the output slots and the feed-forward recognition all ask the view and read nothing again.
enum GemmForm {
  GEMM_MALFORMED,
  GEMM_PLAIN, GEMM_GEGLU,            // bias / row bias / activation / residual, hi + lo output, split-K (tickets or a reduction launch); GEGLU
  GEMM_STATS,                        // column statistics strips beside the result (T2V_EPI_STATS)
  GEMM_LN_ROW, GEMM_LN_CROSS,        // LayerNorm second output: the row inside one tile (plain gather, i[8] = 1); across the column tiles (i[8] = 2)
  GEMM_GN_TILE, GEMM_GN_SPLITK,      // GroupNorm (+SiLU) of the result (T2V_EPI_GN): in the tile epilogue; in the split-K reduction launch
  GEMM_TATTN, GEMM_XATTN,            // fused QKV projection + temporal attention; fused to_q projection + text cross-attention
};
inline bool gemm_writes_gn(GemmForm f) { return f == GEMM_GN_TILE || f == GEMM_GN_SPLITK; }
struct GemmView {
  GemmForm form;
  const char* why;              // the refusal (GEMM_MALFORMED), else null
  const t2v_tile* tile;
  int M, N, K, lda, ldw, ldc, ldr, ldrb;
  int gather, epi, act, out_dtype, out_item, split, bias_m, halo, rows_per_batch;
  // The words i[8..14] under the gather's names.  TCONV3: F, HW (Hin = Win = 0); TATTN: F, HW, tpix (Hin = Win = Cin = 0); else Hin, Win.
  // Under the plain gather the 3x3 names carry the record's words as they stand (the parameter block always has; no kernel reads them
  // there) and what the words mean is named beside them: ln_mode / ld_ln, hilo, res_wrap, a_wrap.
  int Hin, Win, Cin, stride, up, Hout, Wout, F, HW, tpix;
  int ln_mode, ld_ln;           // plain gather, i[8] / i[9]: 1 whole-row, 2 cross-tile LayerNorm output (other values name none); its leading dimension
  int hilo, out_lo;             // plain gather, i[11]; out_lo: the word is 1 — rows [hi | lo] of 2 N halfs
  int res_wrap, a_wrap;         // rows after which the residual / the A operand wrap (0: none); i[30], or i[12] / i[13] of a plain gather
  int64_t n_out;                // stored columns (GEGLU: N / 2)
  int gn_rows, ld_gn, gn_silu, gn_lo, gn_groups, gn_skip_out;      // i[24..29] of every form but XATTN
  int xa_ldk, xa_lc, xa_lcp, xa_k_sample, xa_vt_sample;            // i[24..28] under XATTN
  float ln_eps, attn_scale, gn_eps;
  bool waive_min_m;             // i[31] = 1, a word no check reads: the tests' way to the fused feed-forward pair at a few hundred rows
  bool conv_legacy;             // the same word on a 3x3 convolution: per-tap A staging where the halo staging would apply (gemm2.hip)
  // the pointer slots by role; a role that the form does not have is 0
  uint64_t A, W, bias, rowbias, ln_gb, res, out, ws;               // p[0..6]; p[3] is gamma | beta under the LayerNorm forms
  uint64_t tickets, ln_out, stats;                                 // p[7]
  uint64_t gn_gb, gn_out, xa_k, xa_vt;                             // p[8], p[9]
  uint64_t scratch, barrier;                                       // p[10], p[11]
};

GemmView gemm_decode(const t2v_op& op) {
  const int32_t* I = op.i;
  const uint64_t* P = op.p;
  GemmView v;
  memset(&v, 0, sizeof v);
  const int M = v.M = I[0], N = v.N = I[1], K = v.K = I[2], g = v.gather = I[7], epi = v.epi = I[16];
  const bool plain = g == T2V_GATHER_PLAIN, conv = g == T2V_GATHER_CONV3X3 || g == T2V_GATHER_CONV3X3_C8;
  v.lda = I[3]; v.ldw = I[4]; v.ldc = I[5]; v.ldr = I[6]; v.ldrb = I[21];
  v.act = I[18]; v.out_dtype = I[17]; v.out_item = I[17] == T2V_F32 ? 4 : 2; v.split = I[19] > 1 ? I[19] : 1; v.bias_m = I[20]; v.halo = I[23];
  v.rows_per_batch = I[15] > 0 ? I[15] : 1;
  if (g == T2V_GATHER_TCONV3 || (plain && epi == T2V_EPI_TATTN)) { v.F = I[8]; v.HW = I[9]; }
  else { v.Hin = I[8]; v.Win = I[9]; }
  if (plain && epi == T2V_EPI_TATTN) v.tpix = I[10]; else v.Cin = I[10];
  v.stride = I[11]; v.up = I[12]; v.Hout = I[13]; v.Wout = I[14];
  if (plain) { v.ln_mode = I[8]; v.ld_ln = I[9]; v.hilo = I[11]; v.out_lo = I[11] == 1; }
  if (plain && epi != T2V_EPI_TATTN) { v.res_wrap = I[12]; v.a_wrap = I[13]; }
  if (I[30] > 0) v.res_wrap = I[30];                          // (checked below: not beside i[12])
  v.n_out = epi == T2V_EPI_GEGLU ? N / 2 : N;
  if (epi == T2V_EPI_XATTN) { v.xa_ldk = I[24]; v.xa_lc = I[25]; v.xa_lcp = I[26]; v.xa_k_sample = I[27]; v.xa_vt_sample = I[28]; v.xa_k = P[8]; v.xa_vt = P[9]; }
  else { v.gn_rows = I[24]; v.ld_gn = I[25]; v.gn_silu = I[26]; v.gn_lo = I[27]; v.gn_groups = I[28]; v.gn_skip_out = I[29]; v.gn_gb = P[8]; v.gn_out = P[9]; }
  v.ln_eps = op.f[0]; v.attn_scale = op.f[1]; v.gn_eps = op.f[2];
  v.waive_min_m = I[31] == 1;
  v.conv_legacy = g == T2V_GATHER_CONV3X3 && I[31] == 1;
  const bool ln = plain && epi != T2V_EPI_TATTN && (I[8] == 1 || I[8] == 2);
  v.form = epi == T2V_EPI_TATTN ? GEMM_TATTN : epi == T2V_EPI_XATTN ? GEMM_XATTN : epi == T2V_EPI_GN ? (v.split > 1 ? GEMM_GN_SPLITK : GEMM_GN_TILE)
         : epi == T2V_EPI_GEGLU ? GEMM_GEGLU : epi == T2V_EPI_STATS ? GEMM_STATS : !ln ? GEMM_PLAIN : I[8] == 1 ? GEMM_LN_ROW : GEMM_LN_CROSS;
  v.A = P[0]; v.W = P[1]; v.bias = P[2]; v.res = P[4]; v.out = P[5]; v.ws = P[6]; v.scratch = P[10]; v.barrier = P[11];
  (ln ? v.ln_gb : v.rowbias) = P[3];
  (ln ? v.ln_out : v.form == GEMM_STATS ? v.stats : v.tickets) = P[7];      // tickets: T2V_SYNC_INTS zeroed ints -> the split-K fold runs in the GEMM's last-arriving workgroups; 0 -> reduction launch

  // ---- the checks, in the order a caller sees their messages
  auto bad = [&](const char* why) { v.form = GEMM_MALFORMED; v.why = why; return v; };
  if (M <= 0 || N <= 0 || K <= 0) return bad("empty GEMM");
  if (N % 4 != 0) return bad("N must be a multiple of 4");
  if (K % 8 != 0 || v.lda % 8 != 0 || v.ldw % 8 != 0) return bad("K, lda, ldw must be multiples of 8");
  if (v.ldc % 4 != 0) return bad("ldc must be a multiple of 4");
  if (g == T2V_GATHER_CONV3X3 || g == T2V_GATHER_TCONV3) {
    if (v.Cin % 64 != 0) return bad("conv Cin must be a multiple of 64");
    if (K != (g == T2V_GATHER_CONV3X3 ? 9 : 3) * v.Cin) return bad("K != taps*Cin");
  } else if (g == T2V_GATHER_CONV3X3_C8) {
    if (v.Cin != 8 || K != 72 || v.lda != 8) return bad("C8 conv needs Cin == lda == 8, K == 72");
  } else if (!plain) {
    return bad("unknown gather mode");
  }
  if (conv) {
    if (v.stride != 1 && v.stride != 2) return bad("stride must be 1 or 2");
    if (v.up != 0 && v.up != 1) return bad("upsample must be 0 or 1");
    if (v.Hout <= 0 || v.Wout <= 0 || M % (v.Hout * v.Wout) != 0) return bad("M not a multiple of Hout*Wout");
  }
  if (g == T2V_GATHER_TCONV3 && (v.F <= 0 || v.HW <= 0 || M % (v.F * v.HW) != 0)) return bad("M not a multiple of F*HW");
  if (epi == T2V_EPI_GEGLU && (N % 32 != 0 || v.out_dtype != T2V_F16)) return bad("GEGLU needs N % 32 == 0, fp16 out");
  if (epi == T2V_EPI_STATS && (P[7] == 0 || v.split > 1 || v.ln_mode == 1))
    return bad("column statistics (T2V_EPI_STATS): strips pointer p[7], no split-K, no fused LayerNorm");
  if (epi < 0 || epi > T2V_EPI_XATTN) return bad("unknown epilogue");
  if (v.act < 0 || v.act > 2) return bad("unknown activation (0 none, 1 SiLU, 2 ReLU)");
  const t2v_tile* tile = v.tile = t2v_tile_of(I[22]);          // geometry and fused epilogues of the tile: the table in t2v_kernels.h
  if (tile == nullptr) return bad("unknown tile id");
  if (I[30] != 0) {       // residual row wrap for every gather mode (ABI 11)
    if (I[30] < 0 || M > 2 * I[30] || v.res == 0) return bad("residual row wrap i[30]: positive, M <= 2 * wrap, and a residual");
    if (epi == T2V_EPI_GEGLU || epi == T2V_EPI_TATTN || epi == T2V_EPI_XATTN || (plain && (I[12] != 0 || v.ln_mode != 0)))
      return bad("residual row wrap i[30]: plain / statistics / GroupNorm epilogues only, not beside i[12] or a fused LayerNorm");
  }
  if (epi == T2V_EPI_XATTN) {
    if (!plain || N % 64 != 0 || K % 64 != 0 || v.out_dtype != T2V_F16 || v.split > 1 || v.act != 0 || v.ln_mode != 0 || v.out_lo)
      return bad("fused cross-attention: plain gather, N = 64 * heads, K % 64 == 0, fp16 out, no split-K / activation / LayerNorm / hi + lo output");
    if (!t2v_tile_fuses(tile, T2V_TILE_XATTN, N)) return bad("fused cross-attention: tile 8 / 11 with N == 320, or tile 0 / 5 with N % 128 == 0");
    if (v.bias != 0 || P[3] != 0 || v.res != 0 || v.xa_k == 0 || v.xa_vt == 0 || !(v.attn_scale > 0.f)) return bad("fused cross-attention: no bias / row bias / residual; K, V^T and a positive scale are required");
    if (v.xa_lc < 1 || v.xa_lc > 96 || v.xa_ldk < N || v.xa_ldk % 8 != 0 || v.xa_lcp < ((v.xa_lc + 31) / 32) * 32 || v.xa_lcp % 8 != 0 || I[15] <= 0 || I[15] % 32 != 0 || v.xa_k_sample < 0 || v.xa_vt_sample < 0)
      return bad("fused cross-attention: 1 .. 96 keys, ld(K) >= N, V^T rows of >= ceil32(keys) halfs, rows per sample a multiple of 32");
    if (v.ldc < N || v.ldc % 4 != 0) return bad("fused cross-attention: ldc");
    if (I[12] != 0) return bad("fused cross-attention: no residual wrap");
    return v;
  }
  if (epi == T2V_EPI_GN) {
    // GroupNorm (+SiLU) of the result inside the epilogue: the tiles with an instantiation, whole 32-row strips per statistics
    // instance, at most two instances per row tile, whole groups, every pointer of the exchange
    const int rows = v.gn_rows, groups = v.gn_groups, bm = tile->bm, bn = tile->bn;
    if (g == T2V_GATHER_CONV3X3_C8 || (g == T2V_GATHER_CONV3X3 && v.up != 0)) return bad("fused GroupNorm: not for the C8 stem / the upsampling gather");
    if (v.bias_m != 0 || K % 64 != 0 || v.act != 0) return bad("fused GroupNorm: no bias along M, no activation, K % 64 == 0");
    if (plain && (v.ln_mode != 0 || v.out_lo)) return bad("fused GroupNorm: no fused LayerNorm / hi + lo output on the same op");
    if (groups <= 0 || N % groups != 0 || rows <= 0 || M % rows != 0) return bad("fused GroupNorm: N % groups == 0, rows per instance must divide M");
    if (v.split > 1) {
      // split-K: the norm runs in the reduction's launch (one thread per row x 8 channels, any tile)
      if (groups > 32 || N % 8 != 0 || N / 8 > 512 || v.ws == 0) return bad("fused GroupNorm on a split-K GEMM: groups <= 32, N % 8 == 0, N <= 4096, a slab workspace");
    } else {
      if (!tile->has(T2V_TILE_GN)) return bad("fused GroupNorm: tile must be 8, 11, 3, 5 or 0");
      if (!t2v_tile_fuses(tile, T2V_TILE_GN, N)) return bad("fused GroupNorm on the 128x128-class kernel: N % 128 == 0");
      if (N / groups > bn || (bn + N / groups - 1) / (N / groups) + 1 > T2V_GN_PIECES) return bad("fused GroupNorm: a group no wider than the tile");
      if (rows % 32 != 0 || !(rows >= bm || 2 * rows == bm))
        return bad("fused GroupNorm: rows per instance must be a multiple of 32 and >= the tile's rows (or exactly half of them): at most two instances per row tile");
    }
    if (v.gn_gb == 0 || v.gn_out == 0 || v.scratch == 0 || v.barrier == 0) return bad("fused GroupNorm: gamma|beta, output, scratch and barrier words are required");
    if (v.ld_gn < N * (v.gn_lo ? 2 : 1) || v.ld_gn % 4 != 0) return bad("fused GroupNorm: leading dimension of the normalised output");
    if (v.gn_skip_out == 0 && v.out == 0) return bad("fused GroupNorm: `out` is null but i[29] asks for it");
    if (v.ldc < N || (v.res != 0 && (v.ldr < N || v.ldr % 4 != 0))) return bad("fused GroupNorm: ldc / ldr must be >= N and multiples of 4");
  }
  if (v.split > 1 && v.ws == 0) return bad("split-K without workspace");
  if (P[3] != 0 && I[15] <= 0 && !(v.ln_mode == 1 || v.ln_mode == 2)) return bad("rowbias without rows_per_batch");
  if ((epi == T2V_EPI_TATTN) != tile->has(T2V_TILE_TATTN_ONLY)) return bad("tile 10 is the fused QKV + temporal attention tile (T2V_EPI_TATTN), and only that");
  if (epi == T2V_EPI_TATTN) {
    const int F = v.F, HW = v.HW, tpix = v.tpix;          // (decoded under the plain gather, which is the first thing asked)
    if (!plain || N % 192 != 0 || K % 64 != 0 || v.out_dtype != T2V_F16 || v.split > 1 || v.act != 0)
      return bad("fused temporal attention: plain gather, N = 192 * heads, K % 64 == 0, fp16 out, no split-K / activation");
    if (F < 2 || F > 32 || HW < 1 || tpix < 1 || tpix > 12 || tpix * F > 192) return bad("fused temporal attention: 2 <= F <= 32, 1 <= pixels per tile <= 12, pixels * F <= 192");
    const int tiles_ps = (HW + tpix - 1) / tpix;
    if (M % 192 != 0 || (M / 192) % tiles_ps != 0) return bad("fused temporal attention: M must be samples * ceil(HW / pixels per tile) * 192");
    if (v.bias != 0 || P[3] != 0 || v.res != 0 || v.A == 0 || v.W == 0 || v.out == 0 || !(v.attn_scale > 0.f))
      return bad("fused temporal attention: no bias / row bias / residual; A, W, out and a positive scale are required");
    if (v.ldc < (N / 192) * 64 || v.ldc % 4 != 0) return bad("fused temporal attention: ldc < heads * 64");
    return v;
  }
  if (plain && (I[12] != 0 || I[13] != 0)) {       // row wrap of the residual / the A operand
    if (I[12] < 0 || I[13] < 0 || v.split > 1 || epi == T2V_EPI_GEGLU) return bad("row wrap: non-negative, no split-K, plain epilogue");
    if ((I[12] != 0 && (M > 2 * I[12] || v.res == 0)) || (I[13] != 0 && M > 2 * I[13])) return bad("row wrap: M <= 2 * wrap (and a residual for the residual wrap)");
  }
  if (v.out_lo) {       // hi + lo fp16 output
    if (v.out_dtype != T2V_F16 || epi != T2V_EPI_NONE || v.ln_mode == 1 || v.ldc < 2 * N) return bad("hi + lo output: fp16 out, plain epilogue, no fused LayerNorm, ldc >= 2 N");
  }
  if (v.ln_mode == 2) {         // LayerNorm second output across the column tiles (grid barrier)
    if (!t2v_tile_fuses(tile, T2V_TILE_LNX, N) || v.split > 1 || epi != T2V_EPI_NONE || v.out_dtype != T2V_F32 || v.act != 0 || v.bias_m != 0 || K % 64 != 0 || v.out_lo)
      return bad("cross-tile LayerNorm output: tile 0 (N % 128 == 0), 3, 5, 9 or 12, fp32 out, plain epilogue, no split-K / activation");
    if (v.ln_gb == 0 || v.ln_out == 0 || v.scratch == 0 || v.barrier == 0 || v.ld_ln < N || v.ld_ln % 4 != 0)
      return bad("cross-tile LayerNorm output: gamma|beta, output, scratch, barrier words or leading dimension");
    if (v.ldc < N || (v.res != 0 && (v.ldr < N || v.ldr % 4 != 0))) return bad("cross-tile LayerNorm output: ldc / ldr must be >= N and multiples of 4");
  }
  if (v.ln_mode == 1) {
    if (!t2v_tile_fuses(tile, T2V_TILE_LN, N) || v.split > 1 || epi != T2V_EPI_NONE || v.out_dtype != T2V_F32 || v.act != 0 || v.bias_m != 0 || K % 64 != 0)
      return bad("fused LayerNorm output needs a whole-row tile (192x320, 128x320 or 256x320), N == 320, fp32 out, no split-K / activation");
    if (v.ln_gb == 0 || v.ln_out == 0 || v.ld_ln < N || v.ld_ln % 4 != 0) return bad("fused LayerNorm output: gamma|beta, output pointer or leading dimension");
    // the epilogue moves whole f32x4 / f16x4 groups without tail guards
    if (v.ldc < N || (v.res != 0 && (v.ldr < N || v.ldr % 4 != 0))) return bad("fused LayerNorm output: ldc / ldr must be >= N and multiples of 4");
  }
  return v;
}

int validate_op(const t2v_op& op, int idx) {
  char buf[160];
  auto bad = [&](const char* why) {
    snprintf(buf, sizeof buf, "op %d (kind %d, tag %d): %s", idx, op.kind, op.tag, why);
    return fail(T2V_ERR_BAD_ARG, buf);
  };
  switch (op.kind) {
    case T2V_OP_GEMM: {
      const GemmView g = gemm_decode(op);
      return g.form == GEMM_MALFORMED ? bad(g.why) : 0;
    }
    case T2V_OP_GROUPNORM: {
      const int C = op.i[2], groups = op.i[4], phase = op.i[8], nparts = op.i[9] > 0 ? op.i[9] : 1;
      if (op.i[0] <= 0 || op.i[1] <= 0 || C <= 0 || groups <= 0) return bad("empty GroupNorm");
      if (C % groups != 0 || C % 8 != 0 || op.i[3] % 8 != 0 || op.i[7] % 8 != 0 || groups > 256) return bad("GroupNorm needs C % groups == 0, C / ld % 8 == 0, groups <= 256");
      if (phase < 0 || phase > 3 || op.i[10] < 0 || op.i[10] >= nparts) return bad("bad GroupNorm phase / part");
      if (phase == 3 && (op.p[6] == 0 || op.i[1] % 32 != 0 || op.i[17] < C || nparts != 1)) return bad("GroupNorm phase 3: producer strips p[6], rows % 32 == 0, strip row length i[17] >= C");
      if (op.i[13] != 0 && op.i[13] < op.i[1]) return bad("rows of the largest part < rows");
      if (op.i[12] != 0 && (phase != 0 || (C / groups) % 4 != 0)) return bad("single-launch GroupNorm: phase 0, (C/groups) % 4 == 0");
      if (op.i[16] != 0 && (phase == 1 || op.i[7] < 2 * C)) return bad("GroupNorm low-order output: not for the statistics-only phase, ld_out >= 2 C");
      if (op.p[8] != 0 && (phase == 1 || op.i[19] % 8 != 0 || op.i[20] % 8 != 0 || op.i[19] < C + (op.i[20] ? C : 0) || (op.i[20] != 0 && op.i[20] < C)))
        return bad("GroupNorm cast output: not for the statistics-only phase; leading dimension >= C (+ C for the low-order image), multiples of 8");
      if (op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0 || op.p[4] == 0 || (phase != 1 && op.p[3] == 0)) return bad("null GroupNorm pointer");
      return 0;
    }
    case T2V_OP_LAYERNORM:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[1] % 4 != 0 || op.i[1] > 64 * 4 * 8) return bad("LayerNorm needs 0 < C <= 2048, C % 4 == 0");
      if (op.i[2] < op.i[1] || op.i[3] < op.i[1]) return bad("LayerNorm leading dimension < C");
      if (op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0 || op.p[3] == 0) return bad("null LayerNorm pointer");
      return 0;
    case T2V_OP_ATTENTION: {
      const t2v_attention_class c = t2v_attention_classify(op);
      return c.form == T2V_ATTN_MALFORMED ? bad(c.why) : 0;
    }
    case T2V_OP_RELPOS_ATTN:
      if (op.i[17] == 3) {
        if (op.i[1] <= 0 || op.i[1] > T2V_RELPOS_MAX_FRAMES || op.i[0] <= 0 || op.i[16] < 0 || op.i[16] + op.i[0] > op.i[1])
          return bad("relative-position attention i[17] = 3 needs nk <= T2V_RELPOS_MAX_FRAMES (1024) and queries [q_off, q_off + nq) inside the keys");
        if (op.i[14] != 40 && op.i[14] != 64 && op.i[14] != 80 && op.i[14] != 160) return bad("relative-position attention i[17] = 3: head_dim 40, 64, 80 or 160");
        if (!(op.f[0] > 0.f)) return bad("relative-position attention i[17] = 3: scale must be > 0");
      } else if (op.i[1] <= 0 || op.i[1] > 32 || op.i[0] <= 0 || op.i[16] < 0 || op.i[16] + op.i[0] > op.i[1])
        return bad("relative-position attention needs nk <= 32 (longer clips: i[17] = 3) and queries [q_off, q_off + nq) inside the keys");
      if (op.i[14] <= 0 || op.i[14] % 8 != 0 || op.i[14] > 160) return bad("relative-position attention head_dim: multiple of 8, <= 160");
      if (op.i[2] <= 0 || op.i[3] <= 0 || op.i[4] <= 0 || op.i[15] < 0 || op.i[18] < 0) return bad("empty relative-position attention");
      for (int k = 5; k <= 13; ++k)
        if (op.i[k] < 0) return bad("negative attention stride");
      for (int k = 0; k < 6; ++k)
        if (op.p[k] == 0) return bad("null relative-position attention pointer");
      if (op.i[19] != 0 || op.i[20] != 0 || op.i[21] != 0) return bad("relative-position attention takes no second role (i[19..21])");
      if (op.i[22] != 0 || op.i[23] != 0 || op.i[24] != 0) return bad("relative-position attention takes no per-sample table (i[22..24])");
      if (op.i[17] < 0 || op.i[17] > 3) return bad("relative-position attention kernel selector i[17]: 0 | 1 | 2 | 3");
      if (op.i[17] == 2 && (op.p[6] == 0 || op.p[7] == 0)) return bad("relative-position attention i[17] = 2 needs the packed fp16 tables p[6], p[7]");
      if (op.i[17] == 3 && (op.p[6] == 0 || op.p[7] == 0)) return bad("relative-position attention i[17] = 3 needs the packed fp16 tables p[6], p[7]");
      return 0;
    case T2V_OP_SOFTMAX:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[2] < op.i[1] || op.i[3] < op.i[1] || op.p[0] == 0 || op.p[1] == 0) return bad("bad softmax shape / pointer");
      return 0;
    case T2V_OP_NCTHW_TO_CL:
    case T2V_OP_CL_TO_NCTHW:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[2] <= 0 || op.i[3] <= 0 || op.i[4] < op.i[1]) return bad("bad layout-conversion shape");
      if (op.p[0] == 0 || op.p[1] == 0) return bad("null layout-conversion pointer");
      return 0;
    case T2V_OP_TIME_EMBED:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[1] % 2 != 0 || op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0) return bad("bad time-embedding op");
      return 0;
    case T2V_OP_COPY2D:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[1] % 4 != 0) return bad("copy2d needs cols % 4 == 0");
      if (op.i[2] < op.i[1] || op.i[3] < op.i[1] || op.i[6] < 0 || op.i[6] > 3) return bad("copy2d leading dimension / activation");
      if (op.p[0] == 0 || op.p[1] == 0) return bad("null copy2d pointer");
      if (op.p[2] != 0 && !(op.i[4] == T2V_F32 && op.i[5] == T2V_F16)) return bad("copy2d: the low-order output exists for fp32 -> fp16 casts only");
      return 0;
    case T2V_OP_DDIM_STEP: {
      const t2v_ddim_class c = t2v_ddim_classify(op);
      return c.form == T2V_DDIM_MALFORMED ? bad(c.why) : 0;
    }
    case T2V_OP_MEMSET:
      if (op.p[0] == 0) return bad("null memset pointer");
      return 0;
    case T2V_OP_LINCOMB:
      if (op.i[9] == 1 || op.i[9] == 2) {      // the context-window forms: blend, gather
        const char* why = t2v_window_refusal(op);
        return why != nullptr ? bad(why) : 0;
      }
      if (op.i[9] != 0) return bad("lincomb: form i[9] must be 0 (linear combination), 1 (window blend) or 2 (window gather)");
      if (op.i[0] <= 0 || op.i[1] < 1 || op.i[1] > 6 || op.p[6] == 0) return bad("lincomb needs n > 0, 1..6 terms, an output");
      for (int k = 0; k < op.i[1]; ++k)
        if (op.p[k] == 0) return bad("null lincomb term");
      return 0;
    case T2V_OP_EMBED_ROWS:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[2] <= 0 || op.i[3] <= 0) return bad("empty embedding lookup");
      for (int k = 0; k < 4; ++k)
        if (op.p[k] == 0) return bad("null embedding pointer");
      return 0;
    case T2V_OP_TO_UINT8:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[1] > 4 || op.i[2] <= 0 || op.i[3] <= 0 || op.i[4] <= 0) return bad("empty uint8 conversion");
      if (op.p[0] == 0 || op.p[1] == 0) return bad("null uint8-conversion pointer");
      if (op.i[15] != 0 && op.i[15] != 1) return bad("uint8 conversion: form i[15] must be 0 (tensor2vid) or 1 (torch_to_np)");
      if (op.i[15] == 1 && op.i[7] != 0) return bad("uint8 conversion: the torch_to_np form has no reversed channel order (i[7] = 0)");
      return 0;
    case T2V_OP_RESAMPLE: {
      const int out = op.i[4], axis = op.i[5], form = op.i[7], ld = op.i[8];
      const t2v_resample_grid grid = t2v_resample_grid_of(op);
      if (op.i[9] != 0 && op.i[9] != 1) return bad("resample: mode i[9] must be 0 (uint8 pass) or 1 (float bicubic)");
      if (op.i[9] == 1) {          // float bicubic: planes [P, H, W] -> fp32 [P, Ho, Wo], one launch
        const int Wo = op.i[10];
        if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[2] <= 0 || out <= 0 || Wo <= 0) return bad("bicubic resample: planes, rows, columns and both output sizes must be positive");
        if (op.i[3] != 1) return bad("bicubic resample: planar single-channel images only (i[3] = 1)");
        if (op.i[6] != 4) return bad("bicubic resample: four taps per axis (i[6] = 4)");
        if (form != 1) return bad("bicubic resample: the output form is fp32 (i[7] = 1)");
        if (op.i[11] != T2V_F16 && op.i[11] != T2V_F32) return bad("bicubic resample: unknown input dtype i[11] (fp16 | fp32)");
        if (op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0 || op.p[3] == 0) return bad("null bicubic resample pointer (source, destination, weights, indices)");
        if ((long)op.i[1] * op.i[2] > (1L << 28) || (long)out * Wo > (1L << 28)) return bad("bicubic resample: image too large");
        // one workgroup of 256 threads per (plane, output row, tile of 256 columns): HIP refuses a launch of 2^32 threads or more
        if (grid.rows * grid.tiles > 0xffffffL) return bad("bicubic resample: too many rows for one launch (planes x rows x tiles of 256 columns <= 2^24 - 1)");
        return 0;
      }
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[2] <= 0 || out <= 0 || op.i[6] <= 0) return bad("resample: images, rows, columns, output size and table row length must be positive");
      if (op.i[3] != 3) return bad("resample: interleaved RGB only (3 channels)");
      if (axis != 0 && axis != 1) return bad("resample: axis must be 0 (horizontal) or 1 (vertical)");
      if (form < 0 || form > 2) return bad("resample: unknown output form (0 uint8, 1 fp32 tokens, 2 fp16 tokens)");
      if (form != 0 && (ld < 3 || op.p[4] == 0)) return bad("resample: the token forms need ld >= 3 and the 256-entry value table p[4]");
      if (op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0 || op.p[3] == 0) return bad("null resample pointer (source, destination, coefficients, bounds)");
      const long row_px = axis == 0 ? out : op.i[2];
      if (row_px > (1 << 28)) return bad("resample: row too long");
      // one workgroup of 256 threads per (row, tile): HIP refuses a launch of 2^32 threads or more
      if (grid.rows * grid.tiles > 0xffffffL) return bad("resample: too many rows for one launch (rows x tiles of 256 units <= 2^24 - 1)");
      return 0;
    }
    case T2V_OP_DEPTH_TOKENS:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[2] <= 0 || op.i[1] % 8 != 0 || op.i[2] % 8 != 0) return bad("depth tokens: frames > 0, H and W positive multiples of 8");
      if ((long)op.i[1] * op.i[2] > (1L << 28)) return bad("depth tokens: frame too large");
      if ((op.i[3] != T2V_F16 && op.i[3] != T2V_F32) || (op.i[4] != 0 && op.i[4] != 1) || op.i[5] < 64 || op.i[5] % 8 != 0)
        return bad("depth tokens: input dtype, normalise flag (0 | 1), ld_out >= 64 and a multiple of 8");
      if (op.p[0] == 0 || op.p[1] == 0) return bad("null depth-token pointer");
      if (op.p[1] >= T2V_EXT_SLOTS && op.p[1] % 16 != 0) return bad("depth tokens: the output must be 16-byte aligned");
      return 0;
    case T2V_OP_AVGPOOL2:
      if (op.i[0] <= 0 || op.i[1] < 2 || op.i[2] < 2 || op.i[3] <= 0 || op.i[3] % 4 != 0) return bad("average pooling: images > 0, H and W >= 2, C % 4 == 0");
      if (op.i[4] < op.i[3] || op.i[4] % 4 != 0) return bad("average pooling: ld_in >= C and a multiple of 4");
      if (op.p[0] == 0 || (op.p[1] == 0 && op.p[2] == 0)) return bad("average pooling: an input and at least one output");
      if ((op.p[1] != 0 && (op.i[5] < op.i[3] || op.i[5] % 4 != 0)) || (op.p[2] != 0 && (op.i[6] < op.i[3] || op.i[6] % 4 != 0)))
        return bad("average pooling: output leading dimensions >= C and multiples of 4");
      return 0;
    case T2V_OP_EMPHASIS:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[1] % 4 != 0 || (long)op.i[0] * op.i[1] > (1L << 28)) return bad("emphasis: rows > 0, W a positive multiple of 4, rows * W <= 2^28");
      if (op.i[2] < op.i[1] || op.i[3] < op.i[1] || op.i[3] % 4 != 0 || (op.i[4] != T2V_F16 && op.i[4] != T2V_F32))
        return bad("emphasis: leading dimensions >= W (the output's a multiple of 4), input dtype fp16 | fp32");
      if (op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0) return bad("null emphasis pointer");
      if (op.p[2] >= T2V_EXT_SLOTS && op.p[2] % 16 != 0) return bad("emphasis: the output must be 16-byte aligned");
      return 0;
    case T2V_OP_FINGERPRINT:
      if (op.i[0] <= 0 || op.i[1] < op.i[0]) return bad("fingerprint: n segments > 0, at least one chunk per segment");
      if (op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0) return bad("null fingerprint pointer");
      for (int k = 0; k < 3; ++k)
        if (op.p[k] >= T2V_EXT_SLOTS && op.p[k] % 8 != 0) return bad("fingerprint: the tables and the output must be 8-byte aligned");
      return 0;
    case T2V_OP_LORA_MERGE:
      if (op.i[0] <= 0 || op.i[1] < op.i[0]) return bad("lora merge: n segments > 0, at least one tile per segment");
      if (op.p[0] == 0 || op.p[1] == 0) return bad("null lora merge pointer");
      for (int k = 0; k < 2; ++k)
        if (op.p[k] >= T2V_EXT_SLOTS && op.p[k] % 8 != 0) return bad("lora merge: the tables must be 8-byte aligned");
      return 0;
    case T2V_OP_FREEU: {
      const t2v_freeu_view v = t2v_freeu_decode(op);
      return v.ok ? 0 : bad(v.why);
    }
    case T2V_OP_ALLGATHER:
      if (op.i[2] < 1 || op.i[3] < 0 || op.i[3] >= op.i[2] || op.p[0] == 0) return bad("bad all-gather record");
      return 0;
    case T2V_OP_HALO_EXCHANGE:
      if (op.i[2] < 1 || op.p[0] == 0 || op.i[3] < -1 || op.i[4] < -1) return bad("bad halo-exchange record");
      return 0;
    case T2V_OP_STATS_HALO:
      if (op.i[2] < 1 || op.i[3] < 0 || op.i[3] >= op.i[2] || op.p[0] == 0 || op.p[1] == 0) return bad("bad statistics + halo record");
      if (op.i[6] < 1 || op.i[7] < -1 || op.i[8] < -1 || op.i[7] >= op.i[2] || op.i[8] >= op.i[2]) return bad("bad statistics + halo neighbours");
      return 0;
    case T2V_OP_RESHARD_ROWS:
      if (op.i[0] <= 0 || op.i[1] <= 0 || op.i[2] <= 0 || op.i[3] < 0 || op.i[4] < 0) return bad("bad row-resharding shape");
      if (op.i[5] < op.i[1] || op.i[6] < op.i[1] || op.p[0] == 0 || op.p[1] == 0) return bad("row resharding: leading dimension / pointer");
      if (op.p[2] != 0 && op.i[7] != T2V_F32) return bad("row resharding: the residual form is fp32");
      if (op.i[9] > 1 && (op.i[9] > 64 || op.i[10] < 0 || op.i[11] < 0 || op.i[12] < 0 || op.i[13] < -1 || op.i[13] >= op.i[9] ||
                          (op.i[14] != 0 && op.i[14] != 1) || (op.i[13] >= 0 && op.p[3] == 0)))
        return bad("row resharding: bad multi-part record (parts, part strides, own part)");
      return 0;
    case T2V_OP_ALLTOALL:
      if (op.i[2] < 1 || op.i[3] < 0 || op.i[3] >= op.i[2] || op.i[4] < 1 || op.i[5] < 1 || op.i[5] > op.i[4]) return bad("bad all-to-all record");
      if ((op.i[6] != 0 && op.i[6] != 1) || op.p[0] == 0 || op.p[1] == 0) return bad("bad all-to-all direction / pointer");
      return 0;
    default:
      return bad("unknown op kind");
  }
}

// The parameter block of a decoded GEMM record, complete for every form (a fused-norm form draws its launch's exchange sequence number here)
GemmParams gemm_params(const GemmView& v) {
  GemmParams p;
  memset(&p, 0, sizeof p);
  p.M = v.M; p.N = v.N; p.K = v.K;
  p.lda = v.lda; p.ldw = v.ldw; p.ldc = v.ldc; p.ldr = v.ldr; p.ldrb = v.ldrb;
  p.gather = v.gather;
  p.Hin = v.Hin; p.Win = v.Win; p.Cin = v.Cin; p.stride = v.stride; p.up = v.up; p.Hout = v.Hout; p.Wout = v.Wout; p.F = v.F; p.HW = v.HW;
  p.rows_per_batch = v.rows_per_batch;
  p.epi = v.form == GEMM_GEGLU || v.form == GEMM_TATTN ? v.epi : T2V_EPI_NONE;      // statistics, GroupNorm, cross-attention: the plain epilogue + their pointers
  p.out_f32 = v.out_dtype == T2V_F32; p.act = v.act; p.splitk = v.split; p.bias_m = v.bias_m; p.halo = v.halo; p.conv_legacy = v.conv_legacy;
  auto ptr = [](auto& dst, uint64_t a) { dst = reinterpret_cast<std::remove_reference_t<decltype(dst)>>(a); };
  ptr(p.A, v.A); ptr(p.W, v.W); ptr(p.bias, v.bias); ptr(p.rowbias, v.rowbias); ptr(p.res, v.res); ptr(p.out, v.out); ptr(p.ws, v.ws); ptr(p.stats, v.stats);
  if (v.split > 1) ptr(p.tickets, v.tickets);
  p.out_lo = v.out_lo; p.res_wrap = v.res_wrap; p.a_wrap = v.a_wrap;
  const bool gn = gemm_writes_gn(v.form), ln = v.form == GEMM_LN_ROW || v.form == GEMM_LN_CROSS;
  if (gn) {
    ptr(p.gn_gb, v.gn_gb); ptr(p.gn_out, v.gn_out);
    p.gn_rows = v.gn_rows; p.ld_gn = v.ld_gn; p.gn_silu = v.gn_silu; p.gn_lo = v.gn_lo ? v.N : 0;
    p.gn_cpg = v.N / v.gn_groups; p.gn_store_out = v.gn_skip_out ? 0 : 1; p.gn_eps = v.gn_eps;
  }
  if (ln) {       // a whole-row tile, N == its columns — or, GEMM_LN_CROSS, across the column tiles
    ptr(p.ln_gb, v.ln_gb); ptr(p.ln_out, v.ln_out);
    p.ld_ln = v.ld_ln; p.ln_eps = v.ln_eps; p.ln_x = v.form == GEMM_LN_CROSS;
  }
  if (gn || v.form == GEMM_LN_CROSS) {       // the exchange between the tiles of the launch
    ptr(p.gn_part, v.scratch); ptr(p.gn_bar, v.barrier);
    p.gn_fault = t2v_coop_fault_word();
    t2v_exchange_ids(&p.gn_seq, &p.gn_want);
  }
  if (v.form == GEMM_XATTN) {
    ptr(p.xa_k, v.xa_k); ptr(p.xa_vt, v.xa_vt);
    p.xa_ldk = v.xa_ldk; p.xa_lc = v.xa_lc; p.xa_lcp = v.xa_lcp; p.xa_k_sample = v.xa_k_sample; p.xa_vt_sample = v.xa_vt_sample;
  }
  if (v.form == GEMM_TATTN) { p.tpix = v.tpix; p.tiles_ps = (v.HW + v.tpix - 1) / v.tpix; }
  if (v.form == GEMM_TATTN || v.form == GEMM_XATTN) p.attn_scale_log2 = v.attn_scale * 1.44269504088896340736f;
  return p;
}
hipError_t launch_op(const t2v_op& op, hipStream_t s) {
  switch (op.kind) {
    case T2V_OP_GEMM: {
      const GemmView v = gemm_decode(op);
      if (v.form == GEMM_MALFORMED) return hipErrorInvalidValue;      // (every caller has validated the record)
      // the large-tile kernel advances its source pointers by whole k-tiles: needs K % BK == 0; the fused temporal attention has its own tile there
      const bool gemm2 = v.form == GEMM_TATTN || (v.tile->has(T2V_TILE_GEMM2) && v.gather != T2V_GATHER_CONV3X3_C8 && v.K % 64 == 0);
      return gemm2 ? t2v_launch_gemm2(gemm_params(v), v.tile->id, s) : t2v_launch_gemm(gemm_params(v), s);
    }
    case T2V_OP_GROUPNORM: return t2v_launch_groupnorm(op, s);
    case T2V_OP_LAYERNORM: return t2v_launch_layernorm(op, s);
    case T2V_OP_ATTENTION: return t2v_launch_attention(op, s);
    case T2V_OP_SOFTMAX: return t2v_launch_softmax(op, s);
    case T2V_OP_NCTHW_TO_CL: return t2v_launch_ncthw_to_cl(op, s);
    case T2V_OP_CL_TO_NCTHW: return t2v_launch_cl_to_ncthw(op, s);
    case T2V_OP_TIME_EMBED: return t2v_launch_time_embed(op, s);
    case T2V_OP_COPY2D: return t2v_launch_copy2d(op, s);
    case T2V_OP_DDIM_STEP: return t2v_launch_ddim_step(op, s);
    case T2V_OP_LINCOMB: return t2v_launch_lincomb(op, s);
    case T2V_OP_RELPOS_ATTN: return t2v_launch_relpos_attention(op, s);
    case T2V_OP_EMBED_ROWS: return t2v_launch_embed_rows(op, s);
    case T2V_OP_TO_UINT8: return t2v_launch_to_uint8(op, s);
    case T2V_OP_RESAMPLE: return t2v_launch_resample(op, s);
    case T2V_OP_RESHARD_ROWS: return t2v_launch_reshard_rows(op, s);
    case T2V_OP_DEPTH_TOKENS: return t2v_launch_depth_tokens(op, s);
    case T2V_OP_AVGPOOL2: return t2v_launch_avgpool2(op, s);
    case T2V_OP_EMPHASIS: return t2v_launch_emphasis(op, s);
    case T2V_OP_FINGERPRINT: return t2v_launch_fingerprint(op, s);
    case T2V_OP_LORA_MERGE: return t2v_launch_lora_merge(op, s);
    case T2V_OP_FREEU: return t2v_launch_freeu(op, s);
    case T2V_OP_MEMSET: {
      const size_t bytes = (size_t)(uint32_t)op.i[0] | ((size_t)(uint32_t)op.i[1] << 32);
      return hipMemsetAsync(reinterpret_cast<void*>(op.p[0]), 0, bytes, s);
    }
    default: return hipErrorInvalidValue;
  }
}

// ---- the fused C = 320 GEGLU feed-forward pair (gemm2.hip, t2v_launch_ff_fused) --------------------------------------------------------
// T2V_FF_FUSE (read once): 0 = every plan runs its records one launch each; T2V_FF_FUSE_MIN_M: the row cut-off of the recognition.
constexpr int FF_FUSE_DEFAULT = 1;
constexpr int FF_MIN_M_DEFAULT = 49152;      // a whole round of 192-row workgroups on 256 CUs.  Measured (profiles/ff_fused.txt): at 32768 rows (171
                                             // workgroups) the pair's time is unchanged and the VideoCrafter line 0.5 - 1 % slower, at 24576 the pair is 15 us slower
bool ff_fuse_enabled() {
  static int mode = -1;
  if (mode < 0) {
    const char* e = getenv("T2V_FF_FUSE");
    mode = e != nullptr ? (strcmp(e, "0") != 0 ? 1 : 0) : FF_FUSE_DEFAULT;
  }
  return mode == 1;
}
int ff_min_m() {
  static int min_m = -1;
  if (min_m < 0) {
    const char* e = getenv("T2V_FF_FUSE_MIN_M");
    const long v = e != nullptr ? atol(e) : 0;
    min_m = v > 0 && v < (1L << 30) ? (int)v : FF_MIN_M_DEFAULT;
  }
  return min_m;
}

// Pointer slots of a record that are ONLY written (outputs, workspaces, synchronisation words), as a bit mask — from the field lists
// validate_op checks.  Every other non-null slot counts as read: a slot whose role is in doubt (in-place collectives, the own part of
// a resharding, the K / V^T operands that share numbers with the fused GroupNorm's output) is an input.
unsigned output_slots(const t2v_op& op) {
  auto bits = [](std::initializer_list<int> l) { unsigned m = 0; for (int k : l) m |= 1u << k; return m; };
  const t2v_ddim_form ddim = op.kind == T2V_OP_DDIM_STEP ? t2v_ddim_classify(op).form : T2V_DDIM_MALFORMED;
  if (ddim == T2V_DDIM_MEASURE) return bits({7});      // the measure pass writes the threshold table and nothing else
  if (ddim == T2V_DDIM_INVERT) return bits({3, 4});    // the inversion step: p[4] is a second destination (the kept intermediate), not the blend's known x0
  switch (op.kind) {
    case T2V_OP_GEMM: return bits({5, 6, 7, 10, 11}) | (gemm_writes_gn(gemm_decode(op).form) ? bits({9}) : 0u);      // p[9] is V^T, an input, under XATTN
    case T2V_OP_GROUPNORM: return bits({3, 4, 5, 7, 8});
    case T2V_OP_LAYERNORM: return bits({3});
    case T2V_OP_ATTENTION: return bits({3, 6});
    case T2V_OP_RELPOS_ATTN: return bits({3});
    case T2V_OP_SOFTMAX: return bits({1});
    case T2V_OP_NCTHW_TO_CL: return bits({1, 2});
    case T2V_OP_CL_TO_NCTHW: return bits({1});
    case T2V_OP_TIME_EMBED: return bits({2});
    case T2V_OP_COPY2D: return bits({1, 2});
    case T2V_OP_DDIM_STEP: return bits({3});
    case T2V_OP_MEMSET: return bits({0});
    case T2V_OP_LINCOMB: return bits({6});      // also the context-window forms (i[9] = 1 | 2): their tables p[1], p[2] are read
    case T2V_OP_EMBED_ROWS: return bits({3});
    case T2V_OP_TO_UINT8: return bits({1});
    case T2V_OP_RESAMPLE: return bits({1});
    case T2V_OP_DEPTH_TOKENS: return bits({1});
    case T2V_OP_AVGPOOL2: return bits({1, 2});
    case T2V_OP_EMPHASIS: return bits({2});
    case T2V_OP_FINGERPRINT: return bits({1});
    case T2V_OP_RESHARD_ROWS: return bits({1});
    case T2V_OP_ALLTOALL: return bits({1});
    default: return 0u;      // ALLGATHER / HALO_EXCHANGE / STATS_HALO / FREEU work in place: their slots are read
  }
}

// The bytes a record addresses through pointer slot q, as a bounding range [b, e) from the field lists of include/t2v_hip.h, and whether the
// range is DENSE (every byte of it belongs to the slot: a flat run, or rows whose leading dimension equals their length).  false: the slot
// is not used by this record.  The bound is never smaller than what the kernels touch; only a dense range proves that bytes were written.
// rows > 0: the range is exactly `rows` rows of `rowb` bytes, `pitch` bytes apart (rows == 1: one flat run); rows == 0: only the bound is known.
struct SlotRange { uint64_t b, e; bool dense; int64_t rows, pitch, rowb; };
// Is every byte of r inside w (both with known geometry)?  Sufficient, never wrong: what a record reads there, an earlier record wrote.
bool range_inside(const SlotRange& r, const SlotRange& w) {
  if (r.rows <= 0 || w.rows <= 0 || r.b < w.b || r.e > w.e) return false;
  if (w.rows == 1) return true;
  const uint64_t off = r.b - w.b, i0 = off / (uint64_t)w.pitch, c = off % (uint64_t)w.pitch;
  if (c + (uint64_t)r.rowb > (uint64_t)w.rowb) return false;
  if (r.rows == 1) return i0 < (uint64_t)w.rows;
  return r.pitch == w.pitch && i0 + (uint64_t)r.rows <= (uint64_t)w.rows;
}
bool slot_range(const t2v_op& op, int q, SlotRange* out) {
  const uint64_t v = op.p[q];
  if (v == 0) return false;
  const int32_t* I = op.i;
  auto u64 = [&](int lo, int hi) { return (uint64_t)(uint32_t)I[lo] | ((uint64_t)(uint32_t)I[hi] << 32); };
  auto flat = [&](uint64_t bytes) { const uint64_t n = bytes > 0 ? bytes : 1; *out = {v, v + n, true, 1, 0, (int64_t)n}; return true; };
  auto mat = [&](int64_t rows, int64_t cols, int64_t ld, int item) {
    if (rows <= 0 || cols <= 0) return false;
    if (rows == 1 || ld == cols) return flat((uint64_t)((rows - 1) * ld + cols) * item);
    *out = {v, v + (uint64_t)((rows - 1) * ld + cols) * item, false, rows, ld * item, cols * item};
    return true;
  };
  auto span = [&](uint64_t bytes) { *out = {v, v + (bytes > 0 ? bytes : 1), false, 0, 0, 0}; return true; };
  const int f32 = T2V_F32;
  switch (op.kind) {
    case T2V_OP_GEMM: {
      const GemmView g = gemm_decode(op);
      const int64_t M = g.M, N = g.N, K = g.K;
      if (q == 1 && g.form != GEMM_MALFORMED) return mat(N, K, g.ldw, 2);
      switch (g.form) {
        case GEMM_MALFORMED: return span(~0ull >> 2);
        case GEMM_TATTN: {
          const int64_t tiles_ps = (g.HW + g.tpix - 1) / g.tpix, T = M / 192 / tiles_ps * g.F * g.HW;
          if (q == 0) return mat(T, K, g.lda, 2);
          if (q == 5) return mat(T, N / 192 * 64, g.ldc, 2);
          return span(~0ull >> 2);
        }
        case GEMM_XATTN: {
          const int64_t samples = M / g.rows_per_batch, Lc = g.xa_lc;
          if (q == 0) return mat(g.a_wrap ? g.a_wrap : M, K, g.lda, 2);
          if (q == 5) return mat(M, N, g.ldc, 2);
          if (q == 8) return span((uint64_t)((samples - 1) * g.xa_k_sample + (Lc - 1) * g.xa_ldk + N) * 2);
          if (q == 9) return span((uint64_t)((samples - 1) * g.xa_vt_sample + (N - 1) * g.xa_lcp + g.xa_lcp) * 2);
          return span(~0ull >> 2);
        }
        default: break;
      }
      switch (q) {       // every other form: the slot's role is the one the view gave it
        case 0:
          if (g.gather == T2V_GATHER_PLAIN) return mat(g.a_wrap ? g.a_wrap : M, K, g.lda, 2);
          if (g.gather == T2V_GATHER_TCONV3) return mat(M / ((int64_t)g.F * g.HW) * (g.F + (g.halo ? 2 : 0)) * g.HW, g.Cin, g.lda, 2);
          return mat(M / ((int64_t)g.Hout * g.Wout) * g.Hin * g.Win, g.Cin, g.lda, 2);
        case 2: return flat((uint64_t)(g.bias_m ? M : N) * 4);
        case 3: return g.ln_gb != 0 ? flat((uint64_t)2 * N * 4) : mat((M + g.rows_per_batch - 1) / g.rows_per_batch, N, g.ldrb, 4);
        case 4: return mat(g.res_wrap ? g.res_wrap : M, g.n_out, g.ldr, 4);
        case 5:
          if (g.out_lo) { mat(M, 2 * N, g.ldc, 2); return true; }
          return mat(M, g.n_out, g.ldc, g.out_item);
        case 6: return flat((uint64_t)g.split * M * N * 4);
        case 7:
          if (g.ln_out != 0) return mat(M, N, g.ld_ln, 2);
          if (g.stats != 0) return flat((uint64_t)((M + 31) / 32) * 2 * N * 4);
          return flat((uint64_t)T2V_SYNC_INTS * 4);
        case 8: return flat((uint64_t)2 * N * 4);                                  // GroupNorm gamma | beta
        case 9: return mat(M, N * (g.gn_lo ? 2 : 1), g.ld_gn, 2);                  // GroupNorm output
        case 10: return flat(T2V_GN_PART_BYTES);
        case 11: return flat((uint64_t)T2V_SYNC_BARRIER_INTS * 4);
      }
      return span(~0ull >> 2);
    }
    case T2V_OP_GROUPNORM: {
      const int64_t n_inst = I[0], rows = I[1], C = I[2], ld_in = I[3], groups = I[4], ld_out = I[7], nparts = I[9] > 0 ? I[9] : 1;
      const int item = I[5] == f32 ? 4 : 2, phase = I[8];
      const int64_t before = phase == 2 ? I[21] : 0, after = phase == 2 ? I[22] : 0, total = n_inst * rows + before + after;
      const int64_t rpb = I[11] > 0 ? I[11] : T2V_GN_ROWS_PER_BLOCK, nblk = (rows + rpb - 1) / rpb;
      switch (q) {
        case 0: if (!mat(total, C, ld_in, item)) return false; out->b -= (uint64_t)before * ld_in * item; out->e -= (uint64_t)before * ld_in * item; return true;
        case 1: case 2: return flat((uint64_t)C * 4);
        case 3: if (!mat(total, C * (I[16] ? 2 : 1), ld_out, 2)) return false; out->b -= (uint64_t)before * ld_out * 2; out->e -= (uint64_t)before * ld_out * 2; return true;
        case 4: return flat((uint64_t)((phase == 1 || phase == 2 ? nparts * n_inst * groups * 16 : 0) + n_inst * nblk * groups * 16 + n_inst * groups * 8));
        case 5: return flat((uint64_t)T2V_SYNC_BARRIER_INTS * 4);
        case 6: return flat((uint64_t)n_inst * (rows / 32) * 2 * I[17] * 4);
        case 7: return flat((uint64_t)(I[18] > 0 ? I[18] : 1));
        case 8: return mat(n_inst * rows, I[20] > 0 ? I[20] + C : C, I[19], 2);
      }
      return span(~0ull >> 2);
    }
    case T2V_OP_LAYERNORM:
      if (q == 0) return mat(I[0], I[1], I[2], 4);
      if (q == 1 || q == 2) return flat((uint64_t)I[1] * 4);
      if (q == 3) return mat(I[0], I[1], I[3], 2);
      return span(~0ull >> 2);
    case T2V_OP_ATTENTION:
    case T2V_OP_RELPOS_ATTN: {
      const bool rel = op.kind == T2V_OP_RELPOS_ATTN;
      const int64_t nq = I[0], nk = I[1], heads = I[2], bo = I[3], bi = I[4], D = I[14] > 0 ? I[14] : 64;
      auto seq = [&](int64_t n, int s0, int64_t outer, int64_t outer_stride) {
        return span((uint64_t)((outer - 1) * outer_stride + (bi - 1) * I[s0 + 2] + (n - 1) * I[s0] + heads * D) * 2);
      };
      if (q == 0) return seq(nq, 5, bo, I[6]);
      if (!rel && t2v_attention_classify(op).form == T2V_ATTN_TABLE) {     // K / V are the I[24] packed rows the table spans; the table itself is I[22] pairs of int32
        if (q == 1 || q == 2) return seq(I[24], 8, 1, 0);
        if (q == 7) return flat((uint64_t)I[22] * 8);
      }
      if (q == 1 || q == 2) return seq(nk, 8, bo, I[9]);
      if (q == 3) { if (!seq(nq, 11, bo, I[12])) return false; out->e += (uint64_t)(rel ? I[18] : I[16]) * 2; return true; }
      if (rel) {
        const int64_t R = I[15], DK = (D + 15) / 16 * 16, DV = (D + 31) / 32 * 32;
        if (q == 4 || q == 5) return flat((uint64_t)(2 * R + 1) * D * 4);
        if (q == 6) return flat((uint64_t)(I[17] == 3 ? 2 * R + 1 : 32) * DK * 2);
        if (q == 7) return flat((uint64_t)DV * (I[17] == 3 ? T2V_RELPOS_LONG_COLS(R) : 32) * 2);
      } else {
        if (q == 4 || q == 5) return seq(I[20], 8, bo - I[19], I[21]);
        if (q == 6) return flat((uint64_t)bo * bi * heads * 64 * I[17] * 2);
      }
      return span(~0ull >> 2);
    }
    case T2V_OP_SOFTMAX:
      if (q == 0) return mat(I[0], I[1], I[2], 4);
      if (q == 1) return mat(I[0], I[1], I[3], 2);
      return span(~0ull >> 2);
    case T2V_OP_NCTHW_TO_CL: {
      const int64_t B = I[0], Bsrc = (I[6] > 0 && I[6] < I[0]) ? I[6] : I[0], tokens = B * I[2] * I[3];
      if (q == 0) return flat((uint64_t)Bsrc * I[1] * I[2] * I[3] * (I[5] == f32 ? 4 : 2));
      if (q == 1 || q == 2) return flat((uint64_t)tokens * I[4] * 2);
      return span(~0ull >> 2);
    }
    case T2V_OP_CL_TO_NCTHW:
      if (q == 0) return mat((int64_t)I[0] * I[2] * I[3], I[1], I[4], 4);
      if (q == 1) return flat((uint64_t)I[0] * I[1] * I[2] * I[3] * (I[5] == f32 ? 4 : 2));
      return span(~0ull >> 2);
    case T2V_OP_TIME_EMBED:
      if (q == 0) return flat((uint64_t)I[0] * 4);
      if (q == 1) return flat((uint64_t)I[1] / 2 * 4);
      if (q == 2) return flat((uint64_t)I[0] * I[1] * 2);
      return span(~0ull >> 2);
    case T2V_OP_COPY2D:
      if (q == 0) return mat(I[0], I[1], I[2], I[4] == f32 ? 4 : 2);
      if (q == 1) return mat(I[0], I[1], I[3], I[5] == f32 ? 4 : 2);
      if (q == 2) return mat(I[0], I[1], I[3], 2);
      return span(~0ull >> 2);
    case T2V_OP_MEMSET: return flat(u64(0, 1));
    case T2V_OP_LINCOMB:
      if (I[9] == 1 || I[9] == 2) {      // context windows: p0 the clip (gather) or the windows' eps (blend), p1 starts, p2 weights, p6 out
        const uint64_t item = I[2] == f32 ? 4 : 2, roles = I[9] == 1 ? (uint64_t)I[7] : 1;
        const uint64_t clip = (uint64_t)I[0] * I[1] * I[3] * I[4], win_row = (uint64_t)I[1] * I[5] * I[4];
        if (q == 1) return flat((uint64_t)I[6] * 4);
        if (I[9] == 1) {
          if (q == 0) return flat(roles * I[0] * I[6] * win_row * item);
          if (q == 2) return flat((uint64_t)I[5] * 4);
          if (q == 6) return flat(roles * clip * 4);
        } else {
          if (q == 0) return flat(clip * item);
          if (q == 6) return flat((uint64_t)I[8] * win_row * item);
        }
        return span(~0ull >> 2);
      }
      if (q < I[1]) return flat((uint64_t)I[0] * (I[3 + q] == f32 ? 4 : 2));
      if (q == 6) return flat((uint64_t)I[0] * (I[2] == f32 ? 4 : 2));
      return span(~0ull >> 2);
    case T2V_OP_EMBED_ROWS:
      if (q == 0) return flat((uint64_t)I[0] * 4);
      if (q == 1) return flat((uint64_t)I[3] * I[1] * (I[4] == f32 ? 4 : 2));
      if (q == 2) return flat((uint64_t)I[2] * I[1] * 4);
      if (q == 3) return flat((uint64_t)I[0] * I[1] * 4);
      return span(~0ull >> 2);
    case T2V_OP_ALLGATHER: return flat(u64(0, 1) * (uint64_t)I[2]);
    case T2V_OP_HALO_EXCHANGE: return flat(u64(0, 1) * (uint64_t)(I[2] + 2));
    case T2V_OP_STATS_HALO:
      if (q == 0) return flat(u64(0, 1) * (uint64_t)I[2]);
      if (q == 1) return flat(u64(4, 5) * (uint64_t)(I[6] + 2));
      return span(~0ull >> 2);
    case T2V_OP_ALLTOALL: return flat(u64(0, 1) * (uint64_t)I[2] * (uint64_t)I[4]);
    case T2V_OP_RESHARD_ROWS: {
      const int64_t rows = I[0], cols = I[1], P = I[2], chunks = (rows + P - 1) / P, nparts = I[9] > 1 ? I[9] : 1;
      const int item = I[7] == f32 ? 4 : 2;
      auto grid = [&](int64_t stride, int64_t ld, int it, int64_t part_stride, int64_t parts) {
        return span((uint64_t)(((chunks - 1) * stride + (rows < P ? rows : P) - 1) * ld + cols + (parts - 1) * part_stride) * it);
      };
      if (q == 0) return grid(I[3], I[5], item, I[10], nparts);
      if (q == 1) return grid(I[4], I[6], item, I[11], nparts);
      if (q == 2) return grid(I[4], I[8], 4, I[12], nparts);
      if (q == 3) return I[14] ? grid(I[3], I[5], item, 0, 1) : grid(I[4], I[6], item, 0, 1);
      return span(~0ull >> 2);
    }
    case T2V_OP_AVGPOOL2: {
      const int64_t n = I[0], H = I[1], W = I[2], C = I[3], out_rows = n * (H / 2) * (W / 2);
      if (q == 0) return mat(n * H * W, C, I[4], 4);
      if (q == 1) return mat(out_rows, C, I[5], 4);
      if (q == 2) return mat(out_rows, C, I[6], 2);
      return span(~0ull >> 2);
    }
    case T2V_OP_DEPTH_TOKENS:
      if (q == 0) return flat((uint64_t)I[0] * I[1] * I[2] * (I[3] == f32 ? 4 : 2));
      if (q == 1) return mat((int64_t)I[0] * (I[1] / 8) * (I[2] / 8), 64, I[5], 2);
      return span(~0ull >> 2);
    case T2V_OP_EMPHASIS:
      if (q == 0) return mat(I[0], I[1], I[2], I[4] == f32 ? 4 : 2);
      if (q == 1) return flat((uint64_t)I[0] * 4);
      if (q == 2) return mat(I[0], I[1], I[3], 4);
      return span(~0ull >> 2);
    case T2V_OP_RESAMPLE:
      if (I[9] == 1) {            // float bicubic: its destination may be an arena buffer (the depth path reads it with DEPTH_TOKENS)
        if (q == 0) return flat((uint64_t)I[0] * I[1] * I[2] * (I[11] == f32 ? 4 : 2));
        if (q == 1) return flat((uint64_t)I[0] * I[4] * I[10] * 4);
        if (q == 2 || q == 3) return flat((uint64_t)(I[4] + I[10]) * 4 * 4);
      }
      return span(~0ull >> 2);    // the uint8 passes: as the default below
    case T2V_OP_FREEU: {
      const t2v_freeu_view f = t2v_freeu_decode(op);
      if (q == 0 && f.ok) return mat(f.rows, f.c_total, f.ld, 4);
      return span(~0ull >> 2);
    }
    default:
      // DDIM_STEP, TO_UINT8, RESAMPLE (uint8 passes) work on the caller's tensors in every lowering; should one name arena memory, its extent is in doubt
      return span(~0ull >> 2);
  }
}

// Are ops[k] and ops[k + 1] the GEGLU GEMM and the projection of a C = 320 feed-forward whose hidden tensor nothing else reads?  When in
// doubt: no.  (i[31] = 1 on the GEGLU record, a word no validation reads: the row cut-off is waived — the tests' way to the kernel at
// a few hundred rows.)
bool ff_pair(const t2v_op* ops, int n, int k) {
  if (!ff_fuse_enabled() || k + 1 >= n) return false;
  if (ops[k].kind != T2V_OP_GEMM || ops[k + 1].kind != T2V_OP_GEMM) return false;
  const GemmView a = gemm_decode(ops[k]), b = gemm_decode(ops[k + 1]);          // (validated records: a wrap is never negative, never given twice)
  const int M = a.M;
  // the GEGLU GEMM: plain gather, 2560 x 320, fp16 out, no split-K, nothing beside a bias — no LayerNorm or hi + lo word, wrap, activation, row bias, residual
  if (a.form != GEMM_GEGLU || a.gather != T2V_GATHER_PLAIN || a.split > 1 || a.N != 2560 || a.K != 320 || a.out_dtype != T2V_F16) return false;
  if (a.lda < 320 || a.ldw < 320 || a.ldc < 1280 || a.ln_mode != 0 || a.hilo != 0 || a.res_wrap != 0 || a.a_wrap != 0 || a.act != 0 || a.bias_m != 0) return false;
  if (a.A == 0 || a.W == 0 || a.rowbias != 0 || a.res != 0 || a.out < T2V_EXT_SLOTS) return false;
  // the projection: plain gather and epilogue, 320 x 1280, no split-K, no fused norm, A = exactly that hidden tensor
  if (b.form != GEMM_PLAIN || b.gather != T2V_GATHER_PLAIN || b.split > 1 || b.N != 320 || b.K != 1280 || b.ln_mode != 0) return false;
  if (b.M != M || b.A != a.out || b.lda != a.ldc || b.ldw < 1280 || b.a_wrap != 0 || b.bias_m != 0 || b.W == 0 || b.out == 0) return false;
  if (M < (a.waive_min_m ? 1 : ff_min_m())) return false;
  // One launch reads X, W1 and b1 until its last workgroup is done, while the first ones already store their rows of the result: the
  // result must not lie over them.  (The lowerings do hand the projection the dead X buffer as its output, with rows twice as long:
  // as two launches that is safe, as one launch a workgroup would store over rows another one has yet to read.)
  {
    if (a.A < T2V_EXT_SLOTS || a.W < T2V_EXT_SLOTS || (a.bias != 0 && a.bias < T2V_EXT_SLOTS) || b.out < T2V_EXT_SLOTS) return false;
    const uint64_t o0 = b.out, o1 = o0 + ((uint64_t)(M - 1) * b.ldc + 320 * (b.out_lo ? 2 : 1)) * b.out_item;
    auto apart = [&](uint64_t r0, uint64_t bytes) { return r0 == 0 || o1 <= r0 || o0 >= r0 + bytes; };
    if (!apart(a.A, ((uint64_t)(M - 1) * a.lda + 320) * 2) || !apart(a.W, ((uint64_t)2559 * a.ldw + 320) * 2) || !apart(a.bias, 2560 * 4)) return false;
  }
  // nothing else may read the hidden tensor: scan the records behind the GEGLU GEMM, by EXTENT (slot_range), until the whole tensor has
  // been rewritten.  A record that reaches into bytes of it that no record has rewritten since — through a window that starts below it
  // as well as through a pointer inside it — reads what a fused pair never stored.  Only a dense output range proves a rewrite.
  const uint64_t lo = a.out, hi = lo + ((uint64_t)(M - 1) * a.ldc + 1280) * 2;
  std::vector<std::pair<uint64_t, uint64_t>> left{{lo, hi}};          // bytes of the hidden tensor not rewritten yet
  std::vector<SlotRange> strided;                                      // strided output ranges that reached into them since
  for (int j = k + 1; j < n && !left.empty(); ++j) {
    const unsigned outs = output_slots(ops[j]);
    SlotRange r[T2V_OP_NP];
    bool used[T2V_OP_NP];
    for (int q = 0; q < T2V_OP_NP; ++q) used[q] = ops[j].p[q] >= T2V_EXT_SLOTS && slot_range(ops[j], q, &r[q]);
    for (int q = 0; q < T2V_OP_NP; ++q) {
      if (!used[q] || (j == k + 1 && q == 0)) continue;                // (the projection's A operand)
      bool touches = false;
      for (const auto& s : left) touches = touches || (r[q].b < s.second && s.first < r[q].e);
      if (!touches) continue;
      if (((outs >> q) & 1u) && j != k + 1) continue;                  // an output (the projection's own: never over its operand)
      bool rewritten = false;                                          // a read: fine if an earlier strided output wrote every byte of it
      for (const auto& w : strided) rewritten = rewritten || range_inside(r[q], w);
      if (!rewritten) return false;                                    // read by someone else
    }
    for (int q = 0; q < T2V_OP_NP; ++q) {
      if (!used[q] || !((outs >> q) & 1u)) continue;
      SlotRange w = r[q];
      if (!w.dense) {
        if (w.rows <= 0 || w.b >= hi || lo >= w.e) continue;
        // column slices of one buffer written by several records (a concat, hi | lo halves): adjacent slices of the same rows join, and
        // slices that fill the pitch are a dense run
        for (size_t t = 0; t < strided.size();) {
          const SlotRange& o = strided[t];
          const bool after = o.rows == w.rows && o.pitch == w.pitch && o.b + (uint64_t)o.rowb == w.b;
          const bool before = o.rows == w.rows && o.pitch == w.pitch && w.b + (uint64_t)w.rowb == o.b;
          if (!after && !before) { ++t; continue; }
          if (after) w.b = o.b;
          w.rowb += o.rowb;
          w.e = w.b + (uint64_t)((w.rows - 1) * w.pitch + w.rowb);
          strided.erase(strided.begin() + t);
          t = 0;
        }
        if (w.rowb < w.pitch) { strided.push_back(w); continue; }
        w.dense = true;
      }
      std::vector<std::pair<uint64_t, uint64_t>> rest;
      for (const auto& s : left) {
        if (w.e <= s.first || w.b >= s.second) { rest.push_back(s); continue; }
        if (s.first < w.b) rest.push_back({s.first, w.b});
        if (w.e < s.second) rest.push_back({w.e, s.second});
      }
      left.swap(rest);
    }
  }
  return true;
}

hipError_t launch_ff_pair(const t2v_op& a, const t2v_op& b, hipStream_t s) { return t2v_launch_ff_fused(gemm_params(gemm_decode(a)), gemm_params(gemm_decode(b)), s); }

// fused (plans only): fused[k] != 0 -> ops k and k + 1 run as ONE launch (ff_pair); ms[k] is that launch, ms[k + 1] exactly 0
int run_resolved(const t2v_op* ops, int n, const uint64_t* ext, int n_ext, hipStream_t s, float* ms, t2v_comm* comm = nullptr,
                 const unsigned char* fused = nullptr) {
  {
    // a kernel of an EARLIER run gave up at a grid barrier (norm.hip): that run's results are invalid — say so now, once
    std::string why;
    if (t2v_async_fault_consume(&why)) return fail(T2V_ERR_ASYNC, why);
  }
  std::vector<hipEvent_t> ev;
  if (ms) {
    ev.resize(n + 1);
    for (auto& e : ev)
      if (hipEventCreate(&e) != hipSuccess) return fail(T2V_ERR_LAUNCH, "hipEventCreate failed");
    (void)hipEventRecord(ev[0], s);
  }
  for (int k = 0; k < n; ++k) {
    t2v_op op = ops[k];
    if (!resolve_ptrs(op, ext, n_ext)) {
      char buf[96];
      snprintf(buf, sizeof buf, "op %d (tag %d): unresolved external pointer slot", k, op.tag);
      return fail(T2V_ERR_BAD_ARG, buf);
    }
    if (op.kind == T2V_OP_ALLGATHER || op.kind == T2V_OP_HALO_EXCHANGE || op.kind == T2V_OP_ALLTOALL || op.kind == T2V_OP_STATS_HALO) {
      const size_t bytes = (size_t)(uint32_t)op.i[0] | ((size_t)(uint32_t)op.i[1] << 32);
      std::string err;
      const int rc = op.kind == T2V_OP_STATS_HALO
                         ? t2v_comm_stats_halo(comm, reinterpret_cast<void*>(op.p[0]), bytes, op.i[2], op.i[3], reinterpret_cast<void*>(op.p[1]),
                                               (size_t)(uint32_t)op.i[4] | ((size_t)(uint32_t)op.i[5] << 32), op.i[6], op.i[7], op.i[8], s, err)
                     : op.kind == T2V_OP_ALLGATHER
                         ? t2v_comm_allgather(comm, reinterpret_cast<void*>(op.p[0]), bytes, op.i[2], op.i[3], s, err)
                         : op.kind == T2V_OP_HALO_EXCHANGE
                               ? t2v_comm_halo(comm, reinterpret_cast<void*>(op.p[0]), bytes, op.i[2], op.i[3], op.i[4], s, err)
                               : t2v_comm_alltoall(comm, reinterpret_cast<void*>(op.p[0]), reinterpret_cast<void*>(op.p[1]), bytes, op.i[2],
                                                   op.i[3], op.i[4], op.i[5], op.i[6], s, err);
      if (rc != T2V_OK) {
        char buf[300];
        snprintf(buf, sizeof buf, "op %d (kind %d, tag %d): %s", k, op.kind, op.tag, err.c_str());
        return fail(rc, buf);
      }
      if (ms) (void)hipEventRecord(ev[k + 1], s);
      continue;
    }
    hipError_t e;
    if (fused != nullptr && fused[k]) {
      t2v_op nxt = ops[k + 1];
      if (!resolve_ptrs(nxt, ext, n_ext)) {
        char buf[96];
        snprintf(buf, sizeof buf, "op %d (tag %d): unresolved external pointer slot", k + 1, nxt.tag);
        return fail(T2V_ERR_BAD_ARG, buf);
      }
      e = launch_ff_pair(op, nxt, s);
      if (e == hipSuccess) {
        if (ms) { (void)hipEventRecord(ev[k + 1], s); (void)hipEventRecord(ev[k + 2], s); }
        ++k;
        continue;
      }
    } else {
      e = launch_op(op, s);
    }
    if (e == hipErrorCooperativeLaunchTooLarge) {
      // A launch that needs its whole grid co-resident was refused.  Either a workgroup of an EARLIER launch of this run gave up waiting
      // and raised the fault word (the co-resident path switches off mid-run): that is the asynchronous fault, report it as such now —
      // or the lowering's occupancy table disagrees with this device (other architecture / LDS size / T2V_DEVICE_CUS): a distinct code,
      // so that the caller lowers again without fused norms instead of failing the same way on every call.
      std::string why;
      if (t2v_async_fault_consume(&why)) return fail(T2V_ERR_ASYNC, why);
      char buf[260];
      snprintf(buf, sizeof buf, "op %d (kind %d, tag %d): the launch needs its whole grid co-resident and the occupancy check refused it", k, op.kind, op.tag);
      return fail(T2V_ERR_RESIDENCY, buf);
    }
    if (e != hipSuccess) {
      char buf[200];
      snprintf(buf, sizeof buf, "op %d (kind %d, tag %d) launch failed: %s", k, op.kind, op.tag, hipGetErrorString(e));
      return fail(T2V_ERR_LAUNCH, buf);
    }
    if (ms) (void)hipEventRecord(ev[k + 1], s);
  }
  if (ms) {
    if (hipStreamSynchronize(s) != hipSuccess) return fail(T2V_ERR_LAUNCH, "stream sync failed");
    for (int k = 0; k < n; ++k) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
    for (int k = 0; fused != nullptr && k + 1 < n; ++k)
      if (fused[k]) ms[k + 1] = 0.0f;
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
  return T2V_OK;
}

}  // namespace

struct t2v_plan {
  std::vector<t2v_op> ops;
  std::vector<unsigned char> fused;   // fused[k]: ops k, k + 1 are a feed-forward pair that runs as one launch (ff_pair)
  t2v_comm* comm = nullptr;   // borrowed (t2v_plan_set_comm)
};

extern "C" {

int t2v_abi_version(void) { return T2V_ABI_VERSION; }

const char* t2v_last_error(void) { return g_err.c_str(); }

int t2v_device_info(char* name, int len, int* compute_units, uint64_t* hbm_bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(T2V_ERR_NO_DEVICE, "no HIP device");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(T2V_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
  if (name && len > 0) {
    strncpy(name, prop.gcnArchName, (size_t)len - 1);
    name[len - 1] = 0;
  }
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (uint64_t)prop.totalGlobalMem;
  return T2V_OK;
}

int t2v_async_status(void) {
  std::string why;
  if (t2v_async_fault_consume(&why)) return fail(T2V_ERR_ASYNC, why);
  return T2V_OK;
}

int t2v_sync_reset(void* sync_words, void* stream) {
  if (!sync_words) return fail(T2V_ERR_BAD_ARG, "null sync words");
  const hipError_t e = hipMemsetAsync(sync_words, 0, sizeof(int32_t) * (T2V_SYNC_INTS + T2V_SYNC_BARRIER_INTS), reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(T2V_ERR_LAUNCH, std::string("hipMemsetAsync of the sync words failed: ") + hipGetErrorString(e));
  return T2V_OK;
}

int t2v_run_ops(const t2v_op* ops, int n, const uint64_t* ext, int n_ext, void* stream) {
  if (ops == nullptr || n < 0) return fail(T2V_ERR_BAD_ARG, "null program");
  for (int k = 0; k < n; ++k) {
    const int rc = validate_op(ops[k], k);
    if (rc != 0) return rc;
  }
  return run_resolved(ops, n, ext, n_ext, reinterpret_cast<hipStream_t>(stream), nullptr);
}

int t2v_plan_create(const t2v_op* ops, int n, t2v_plan** out) {
  if (ops == nullptr || n <= 0 || out == nullptr) return fail(T2V_ERR_BAD_ARG, "null program");
  for (int k = 0; k < n; ++k) {
    const int rc = validate_op(ops[k], k);
    if (rc != 0) return rc;
    if (ops[k].kind == T2V_OP_FINGERPRINT) return fail(T2V_ERR_BAD_ARG, "fingerprint: a stand-alone op (t2v_run_ops), not part of a plan");
    if (ops[k].kind == T2V_OP_LORA_MERGE) return fail(T2V_ERR_BAD_ARG, "lora merge: a stand-alone op (t2v_run_ops), not part of a plan");
  }
  t2v_plan* p = new t2v_plan();
  p->ops.assign(ops, ops + n);
  p->fused.assign(n, 0);
  for (int k = 0; k + 1 < n; ++k)
    if (ff_pair(ops, n, k)) { p->fused[k] = 1; ++k; }
  *out = p;
  return T2V_OK;
}

int t2v_plan_num_ops(const t2v_plan* plan) { return plan ? (int)plan->ops.size() : 0; }

int t2v_plan_num_launches(const t2v_plan* plan) {
  if (!plan) return 0;
  int fused = 0;
  for (unsigned char f : plan->fused) fused += f;
  return (int)plan->ops.size() - fused;
}

int t2v_plan_run(t2v_plan* plan, const uint64_t* ext, int n_ext, void* stream) {
  if (!plan) return fail(T2V_ERR_BAD_ARG, "null plan");
  return run_resolved(plan->ops.data(), (int)plan->ops.size(), ext, n_ext, reinterpret_cast<hipStream_t>(stream), nullptr, plan->comm, plan->fused.data());
}

int t2v_plan_run_timed(t2v_plan* plan, const uint64_t* ext, int n_ext, void* stream, float* ms) {
  if (!plan || !ms) return fail(T2V_ERR_BAD_ARG, "null plan / ms");
  return run_resolved(plan->ops.data(), (int)plan->ops.size(), ext, n_ext, reinterpret_cast<hipStream_t>(stream), ms, plan->comm, plan->fused.data());
}

void t2v_plan_destroy(t2v_plan* plan) { delete plan; }

int t2v_plan_set_comm(t2v_plan* plan, t2v_comm* comm) {
  if (!plan) return fail(T2V_ERR_BAD_ARG, "null plan");
  plan->comm = comm;
  return T2V_OK;
}

int t2v_comm_unique_id(unsigned char id[128]) {
  if (!id) return fail(T2V_ERR_BAD_ARG, "null id");
  std::string err;
  const int rc = t2v_comm_impl_unique_id(id, err);
  return rc == T2V_OK ? rc : fail(rc, err);
}

int t2v_comm_create(const unsigned char id[128], int nranks, int rank, t2v_comm** out) {
  if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks) return fail(T2V_ERR_BAD_ARG, "bad communicator arguments");
  std::string err;
  const int rc = t2v_comm_impl_create(id, nranks, rank, out, err);
  return rc == T2V_OK ? rc : fail(rc, err);
}

int t2v_comm_size(const t2v_comm* comm) { return t2v_comm_impl_size(comm); }

int t2v_comm_window_create(t2v_comm* comm, uint64_t slot_bytes, unsigned char handle_out[64]) {
  if (!comm || !handle_out || slot_bytes == 0) return fail(T2V_ERR_BAD_ARG, "window_create needs a communicator, a slot size and room for the handle");
  std::string err;
  const int rc = t2v_comm_impl_window_create(comm, (size_t)slot_bytes, handle_out, err);
  return rc == T2V_OK ? rc : fail(rc, err);
}

int t2v_comm_window_open(t2v_comm* comm, const unsigned char* handles) {
  if (!comm) return fail(T2V_ERR_BAD_ARG, "window_open needs a communicator");
  std::string err;
  const int rc = t2v_comm_impl_window_open(comm, handles, err);
  return rc == T2V_OK ? rc : fail(rc, err);
}

const char* t2v_comm_window_kind(const t2v_comm* comm) { return t2v_comm_impl_window_kind(comm); }

void t2v_comm_counters(const t2v_comm* comm, uint64_t out[2]) {
  unsigned long long v[2];
  t2v_comm_impl_counters(comm, v);
  out[0] = v[0];
  out[1] = v[1];
}

void t2v_comm_destroy(t2v_comm* comm) { t2v_comm_impl_destroy(comm); }

int t2v_comm_all_gather(t2v_comm* comm, void* base, uint64_t bytes, void* stream) {
  if (!comm || !base || bytes == 0) return fail(T2V_ERR_BAD_ARG, "all-gather needs a communicator, a base pointer and a part size");
  std::string err;
  const int rc = t2v_comm_impl_all_gather(comm, base, (size_t)bytes, reinterpret_cast<hipStream_t>(stream), err);
  return rc == T2V_OK ? rc : fail(rc, err);
}

int t2v_unet_forward(t2v_plan* plan, const void* x, const float* t, const void* ctx, void* eps_out, void* stream) {
  uint64_t ext[T2V_EXT_SLOTS] = {0};
  ext[T2V_EXT_X] = (uint64_t)x;
  ext[T2V_EXT_T] = (uint64_t)t;
  ext[T2V_EXT_CTX] = (uint64_t)ctx;
  ext[T2V_EXT_OUT] = (uint64_t)eps_out;
  return t2v_plan_run(plan, ext, T2V_EXT_SLOTS, stream);
}

int t2v_vae_decode(t2v_plan* plan, const void* z, void* img_out, void* stream) {
  uint64_t ext[T2V_EXT_SLOTS] = {0};
  ext[T2V_EXT_X] = (uint64_t)z;
  ext[T2V_EXT_OUT] = (uint64_t)img_out;
  return t2v_plan_run(plan, ext, T2V_EXT_SLOTS, stream);
}

int t2v_ddim_step(t2v_plan* plan, const void* xt, const void* eps_pair, const void* noise, void* xt_out,
                  const float coef[6], void* stream) {
  if (!plan || plan->ops.size() != 1 || plan->ops[0].kind != T2V_OP_DDIM_STEP)
    return fail(T2V_ERR_BAD_ARG, "t2v_ddim_step needs a single DDIM_STEP plan");
  t2v_op op = plan->ops[0];
  for (int k = 0; k < 6; ++k) op.f[k] = coef[k];
  uint64_t ext[T2V_EXT_SLOTS] = {0};
  ext[T2V_EXT_XT] = (uint64_t)xt;
  ext[T2V_EXT_EPS] = (uint64_t)eps_pair;
  ext[T2V_EXT_NOISE] = (uint64_t)noise;
  ext[T2V_EXT_XT_OUT] = (uint64_t)xt_out;
  return run_resolved(&op, 1, ext, T2V_EXT_SLOTS, reinterpret_cast<hipStream_t>(stream), nullptr);
}

}  // extern "C"
