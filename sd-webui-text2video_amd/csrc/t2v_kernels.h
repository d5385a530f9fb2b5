// Internal launch interface between executor.hip and the kernel translation units.
// gfx950 (MI355X / CDNA4) only: wave64, MFMA 32x32x16 f16, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/t2v_hip.h"

typedef _Float16 f16;
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GemmParams {
  const f16* A;
  const f16* W;
  const float* bias;
  const float* rowbias;
  const float* res;
  void* out;
  float* ws;
  int M, N, K;
  int m_begin;                                 // the launch covers token rows [m_begin, M) (0 except in the row chunks of a fused-norm launch larger than
                                               // the device holds co-resident: t2v_launch_coresident); every row index below stays GLOBAL
  int lda, ldw, ldc, ldr, ldrb;
  int gather;
  int Hin, Win, Cin, stride, up, Hout, Wout;  // conv3x3: input / output spatial dims
  int F, HW;                                   // tconv3: frames per clip, pixels per frame
  int rows_per_batch;
  int epi, out_f32, act, splitk, bias_m;
  int kt_per_split;                            // k-tiles (of 64) per split
  int halo;                                    // tconv3: input has one halo frame before and after each clip
                                               // ([B][F+2][HW] rows, T-sharded forward); all 3 taps are in range.
                                               // conv3x3: 1 = asymmetric (0,1,0,1) zero padding (taps at +0..+2)
  int panel;                                   // tile columns per panel of the XCD-aware tile order (set by the launcher)
  int conv_legacy;                             // conv3x3: 1 = per-tap A staging even where the halo staging applies (gemm2.hip; t2v_op i[31], the tests' way to both)
  // fused LayerNorm second output (192x320 tile, N == 320 == one tile row, no split-K): ln_out = LN(out row) * gamma + beta
  const float* ln_gb;                          // fp32 [2 N]: gamma | beta
  f16* ln_out;
  int ld_ln;
  float ln_eps;
  // fused QKV + temporal attention (T2V_EPI_TATTN, 192x192 tile): tile rows = tpix pixels x F frames of one sample
  int tpix, tiles_ps;                          // pixels per tile, row tiles per sample (ceil(HW / tpix))
  float attn_scale_log2;                       // softmax scale * log2(e)
  // split-K without a reduction launch (EPI_NONE): one arrival counter per output tile (T2V_SYNC_INTS ints, all zero between
  // launches); the LAST workgroup of a tile to arrive folds the slabs in split order and runs the fused epilogue
  int* tickets;
  // hi + lo fp16 output (PLAIN gather, fp16 out, EPI_NONE): out[m, N + n] = fp16(v - float(fp16(v))) beside out[m, n] = fp16(v) — the
  // consumer GEMM reads rows [hi | lo] against weights [W | W] (K doubled) and so sees the value with ~22 bits (precise_operands)
  int out_lo;
  // Column statistics of the stored result for a GroupNorm that consumes it (T2V_EPI_STATS; no split-K): stats[m / 32][0][n] = sum over
  // the 32-row strip of out[m, n], stats[m / 32][1][n] = sum of squares — fp32 [ceil(M / 32)][2][N].  The GroupNorm then needs no
  // statistics pass over the tensor (and no grid barrier): a small fold of the strips + one apply pass (norm.hip, phase 3).
  float* stats;
  // Row wrap (M <= 2 * wrap; a_wrap: PLAIN gather, no split-K; res_wrap: any gather — t2v_op i[12] / i[30]): operand row m >= a_wrap reads A row m - a_wrap; residual row m >= res_wrap reads
  // residual row m - res_wrap.  The cond | uncond pair of a guided step shares every tensor up to the first text cross-attention
  // (same x_t, same t): those are computed ONCE (one sample's rows) and the first per-sample GEMMs read them through the wrap.
  int a_wrap, res_wrap;
  // GroupNorm (+SiLU) of the result inside the epilogue (T2V_EPI_GN, round 5; t2v_epilogue_rows_gn below): the tile stays in registers,
  // the statistics meet at a grid barrier — the launch must be co-resident (checked by the launcher)
  const float* gn_gb;                          // fp32 [2 N]: gamma | beta
  f16* gn_out;                                 // fp16 [M, ld_gn] (+ low-order image at column gn_lo)
  double* gn_part;                             // fp64 [tiles_m][2][tiles_n][T2V_GN_PIECES][2]
  unsigned* gn_bar;                            // T2V_SYNC_BARRIER_INTS grid-barrier words
  unsigned* gn_fault;                          // host-mapped fault word of the bounded barrier
  int ld_gn, gn_rows, gn_cpg, gn_silu, gn_lo, gn_store_out;
  float gn_eps;
  // LayerNorm second output ACROSS column tiles (t2v_epilogue_rows_lnx: ln_gb / ln_out / ld_ln / ln_eps as above, partial row sums
  // through gn_part, the grid barrier on gn_bar): any N, the launch must be co-resident
  int ln_x;
  // Exchange mode of the fused-norm kernels: gn_seq != 0 -> TAGGED RECORDS (every published {sum, sum of squares} pair carries the
  // launch's 32-bit sequence number in the low mantissa bits; consumers poll the records they need until the tags match: no barrier);
  // gn_seq == 0 -> the grid barrier on gn_bar.  gn_want = the number consumers expect (== gn_seq except in the fault-injection test).
  unsigned gn_seq, gn_want;
  // fused to_q projection + text cross-attention (T2V_EPI_XATTN, t2v_epilogue_xattn): K [samples][Lc][ldk] (this site's columns), V^T
  // [samples][N][lcp] (keys contiguous, zero beyond Lc), both step-invariant; the sample of a row = m / rows_per_batch
  const f16* xa_k;
  const f16* xa_vt;
  int xa_ldk, xa_lc, xa_lcp, xa_k_sample, xa_vt_sample;
};


// The device-scope helpers below are gfx942 / gfx950 assembly (`sc1` cache-policy bits, stores counted by vmcnt): on other targets
// they would either not assemble (gfx90a spells the bits glc / slc) or — where stores are counted by vscnt — be silently unordered.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "libt2v_hip is written for gfx950 (MI355X); the device-scope exchange helpers assume gfx94x / gfx950 memory semantics"
#endif

// Device-scope data exchange between workgroups of ONE launch.  The 8 XCDs have private, mutually non-coherent L2s; an
// agent-scope fence makes that safe by writing back / invalidating the WHOLE L2 of the XCD (buffer_wbl2 sc1 / buffer_inv sc1)
// — measured here: every workgroup doing that turned 26 us split-K GEMMs into 72 us ones and gave every cooperative GroupNorm
// a 35 us floor, because the co-running workgroups lost their cached operands.  So the exchanged data itself moves with
// device-scope accesses (sc1: stores write through to the device's coherence point, loads do not hit non-coherent lines),
// ordered by s_waitcnt vmcnt(0) and RELAXED device-scope atomics on the flag words: no cache-wide operation anywhere.
__device__ __forceinline__ void t2v_st_dev(float* p, f32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ f32x4 t2v_ld_dev(const float* p) {
  f32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(v) : "v"(p) : "memory");      // completion: t2v_wait_dev below
  return v;
}
// the loads issued by t2v_ld_dev have landed; the operands tie the consumers of the four values to this point
__device__ __forceinline__ void t2v_wait_dev(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
__device__ __forceinline__ void t2v_wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- XCD-aware tile order -----------------------------------------------------------------------------
// Workgroup b of a launch runs on XCD b % 8 (round-robin dispatch) and each of the 8 XCDs has a private L2:
// operand bytes needed on several XCDs are fetched from the fabric once PER XCD (measured with FETCH_SIZE:
// the 8x8-level convolutions re-fetched their 30-60 MB weight matrices 8 times).  Tiles are therefore
// numbered panel by panel — a panel = `pw` tile columns, inside it m-major with n fastest — and each XCD
// takes ONE contiguous run of that numbering.  A run covers ~(tiles_m / xm) x pw tiles with xm * xn = 8,
// xn = ceil(tiles_n / pw): the chip fetches ~xn * A + xm * W bytes instead of A + 8 W (pw = tiles_n) or
// 8 A + W (pw = 1).  The launcher picks xn in 1..8 minimising xn * A + (8 / xn) * W.
__device__ __forceinline__ void t2v_tile_of_block(int b, int tiles_m, int tiles_n, int pw, int& tile_m, int& tile_n) {
  const int ntiles = tiles_m * tiles_n;
  const int q = ntiles >> 3, r = ntiles & 7, xcd = b & 7, j = b >> 3;
  const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;   // bijective for any ntiles
  const int per_panel = tiles_m * pw;
  const int pnl = lin / per_panel, rem = lin - pnl * per_panel;
  const int n_start = pnl * pw;
  const int w_here = min(pw, tiles_n - n_start);
  tile_m = rem / w_here;
  tile_n = n_start + rem - tile_m * w_here;
}

inline int t2v_choose_panel(const GemmParams& p, int tiles_m, int tiles_n) {
  const double a_rows = p.gather == T2V_GATHER_CONV3X3 ? (double)p.M * p.stride * p.stride / (p.up ? 4.0 : 1.0) : (double)p.M;
  const double Ab = a_rows * (p.gather == T2V_GATHER_PLAIN ? p.K : p.Cin) * 2.0;
  const double Wb = (double)p.N * p.K * 2.0;
  int best_xn = 1;
  double best = 1e300;
  for (int xn = 1; xn <= 8 && xn <= tiles_n; ++xn) {
    const double cost = xn * Ab + (8.0 / xn) * Wb;
    if (cost < best) { best = cost; best_xn = xn; }
  }
  return (tiles_n + best_xn - 1) / best_xn;
}

// ---- per-device host state ---------------------------------------------------------------------------
// One process may drive several GPUs (or CPX / SPX partitions with different CU counts): everything the launchers cache about
// "the device" is keyed by the device of the launch stream, never by whichever device was current on the first call.
constexpr int T2V_MAX_DEVICES = 64;
inline int t2v_device_of(hipStream_t s) {
  int d = 0;
  hipDevice_t sd;
  if (s != nullptr && hipStreamGetDevice(s, &sd) == hipSuccess) d = (int)sd;
  else (void)hipGetDevice(&d);
  return (d >= 0 && d < T2V_MAX_DEVICES) ? d : 0;
}
struct t2v_device_flags { bool set[T2V_MAX_DEVICES] = {}; };
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device): `flags` is a function-local static
// of the instantiation's launcher (the call costs microseconds on the host)
inline hipError_t t2v_set_dynamic_lds(const void* kernel, int lds_bytes, t2v_device_flags& flags, hipStream_t s) {
  const int d = t2v_device_of(s);
  if (flags.set[d]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e == hipSuccess) flags.set[d] = true;
  return e;
}
int t2v_num_cus(hipStream_t s);                         // compute units of the stream's device (norm.hip, cached per device)
// makes the stream's device current for the lifetime of the object (occupancy queries answer for the CURRENT device)
struct t2v_device_guard {
  int prev = -1;
  explicit t2v_device_guard(hipStream_t s) {
    const int d = t2v_device_of(s);
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != d && hipSetDevice(d) == hipSuccess) prev = cur;
  }
  ~t2v_device_guard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// A kernel whose workgroups meet at a grid barrier must be wholly resident: `nwg` workgroups of `threads` threads and `lds` dynamic
// bytes against what the occupancy API grants `kernel` per CU on the stream's device (cache[device]: 0 = not asked yet, -1 = failed).
inline bool t2v_grid_fits(const void* kernel, int threads, size_t lds, long nwg, hipStream_t s, int* cache) {
  const int d = t2v_device_of(s);
  if (cache[d] == 0) {
    t2v_device_guard guard(s);
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, lds) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
    cache[d] = nb > 0 ? nb : -1;
  }
  return cache[d] > 0 && nwg <= (long)cache[d] * t2v_num_cus(s);
}

// workgroups of `kernel` the stream's device holds at once (occupancy API x compute units; 0: unknown)
inline long t2v_grid_capacity(const void* kernel, int threads, size_t lds, hipStream_t s, int* cache) {
  return t2v_grid_fits(kernel, threads, lds, 0, s, cache) ? (long)cache[t2v_device_of(s)] * t2v_num_cus(s) : 0;
}

// Asynchronous faults (norm.hip): a kernel that gives up waiting for a co-resident workgroup (bounded grid barrier of the
// single-pass GroupNorm) raises a flag in host-mapped memory instead of hanging the device.  The executor reads it at the entry
// of every run: the run that raised it produced invalid results, the NEXT call reports it (t2v_async_status() reports it at once)
// and the cooperative path stays off for the rest of the process.
void t2v_exchange_ids(unsigned* seq, unsigned* want);     // sequence number of the next fused-norm launch (0, 0: barrier mode — T2V_EXCHANGE=barrier)
unsigned* t2v_coop_fault_word();                        // the host-mapped fault word of the bounded grid barriers (null: unavailable)
unsigned* t2v_peer_fault_word();                        // its neighbour: raised by a peer-window wait that gave up (comm.hip)
bool t2v_coop_allowed();                                // false once a barrier timed out in this process (or the word could not be mapped)
int t2v_async_fault_pending();                          // 1 = a fault was raised and not yet reported
int t2v_async_fault_consume(std::string* msg);          // returns 1 (and clears "pending", keeps the path disabled) if a fault was raised

// A GEMM whose epilogue exchanges statistics between its workgroups (fused GroupNorm / cross-tile LayerNorm) needs the grid of ONE launch
// co-resident.  A problem with more tiles than the device holds (125-frame clips, 1024x576, round 6) is cut into ROW CHUNKS of whole units —
// unit_rows is a multiple of the tile's rows and of the statistics instance's rows, so that no tile and no instance straddles a chunk —
// each chunk its own launch over rows [m_begin, M) with its own exchange sequence number (the scratch records are re-used: stream order).
// launch(q, tiles) launches `tiles` workgroups for the parameter block q.  capacity: t2v_grid_capacity of the instantiation.
template <typename LaunchFn>
inline hipError_t t2v_launch_coresident(const GemmParams& p, int BM, int tiles_n, long capacity, long unit_rows, long scratch_per_tile, LaunchFn launch) {
  const long rows = (long)p.M - p.m_begin, tiles_all = ((rows + BM - 1) / BM) * tiles_n;
  if (capacity > T2V_GN_PART_BYTES / scratch_per_tile) capacity = T2V_GN_PART_BYTES / scratch_per_tile;   // the exchange records of ONE launch (p.gn_part)
  if (capacity <= 0) return hipErrorCooperativeLaunchTooLarge;
  if (tiles_all <= capacity) return launch(p, (int)tiles_all);
  const long unit_tiles = (unit_rows / BM) * tiles_n;
  if (unit_rows <= 0 || unit_rows % BM != 0 || unit_tiles > capacity) return hipErrorCooperativeLaunchTooLarge;
  const long chunk_rows = (capacity / unit_tiles) * unit_rows;
  for (long m = p.m_begin; m < p.M; m += chunk_rows) {
    GemmParams q = p;
    q.m_begin = (int)m;
    q.M = (int)(m + chunk_rows < p.M ? m + chunk_rows : p.M);
    if (m != p.m_begin && p.gn_seq != 0u) t2v_exchange_ids(&q.gn_seq, &q.gn_want);
    const hipError_t e = launch(q, (int)((((long)q.M - m + BM - 1) / BM) * tiles_n));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
inline long t2v_lcm(long a, long b) { long x = a, y = b; while (y) { const long t = x % y; x = y; y = t; } return a / x * b; }

// Split-K state of a GEMM launch (both launchers): `splitk` clamped to [1, k-tiles of `bk`], `kt_per_split` derived from it, empty
// splits removed.  The ticket buffer survives only where the in-kernel fold applies (t2v_epilogue_rows: the last-arriving workgroup
// of a tile folds the slabs) — plain epilogue, one counter per output tile, no GroupNorm behind it; elsewhere the reduction kernel runs.
inline void t2v_normalize_splitk(GemmParams& p, int bk, long tiles) {
  const int KT = (p.K + bk - 1) / bk;
  if (p.splitk > KT) p.splitk = KT;
  if (p.splitk < 1) p.splitk = 1;
  p.kt_per_split = (KT + p.splitk - 1) / p.splitk;
  p.splitk = (KT + p.kt_per_split - 1) / p.kt_per_split;  // no empty splits
  if (p.splitk <= 1 || p.epi != T2V_EPI_NONE || tiles > T2V_SYNC_INTS || p.gn_out != nullptr) p.tickets = nullptr;
}

// ---- the GEMM tiles (t2v_op.i[22]) ----------------------------------------------------------------------------------------------------
// ONE entry per tile id that has a kernel: its geometry and the fused epilogues it has an instantiation for.  The dispatchers (gemm.hip,
// gemm2.hip) instantiate from it and executor.hip validates against it; GEMM_TILES in program.py is the same table for the lowering
// (tests/test_tile_table.py holds the two together through the validator).
// XE, the extra epilogue of a T2V_EPI_NONE instantiation (an int template parameter of gemm_kernel / gemm2_kernel):
enum : int {
  T2V_XE_NONE = 0,
  T2V_XE_LN = 1,       // LayerNorm second output, whole rows in the tile (t2v_epilogue_rows_ln)
  T2V_XE_GN = 2,       // GroupNorm (+SiLU) of the result, statistics across the launch at a grid barrier (T2V_EPI_GN, t2v_epilogue_rows_gn)
  T2V_XE_LNX = 3,      // LayerNorm second output across the column tiles of the launch (t2v_epilogue_rows_lnx)
  T2V_XE_XATTN = 4,    // to_q projection + text cross-attention (T2V_EPI_XATTN, t2v_epilogue_xattn)
};
enum : unsigned {
  T2V_TILE_GN = 1u << 0,           // has the T2V_XE_GN instantiations (plain, 3x3 and temporal gathers)
  T2V_TILE_LNX = 1u << 1,          // ... T2V_XE_LNX (plain gather)
  T2V_TILE_LN = 1u << 2,           // ... T2V_XE_LN: a whole-row tile (N == columns)
  T2V_TILE_XATTN = 1u << 3,        // ... T2V_XE_XATTN
  T2V_TILE_TATTN_ONLY = 1u << 4,   // runs T2V_EPI_TATTN and nothing else
  T2V_TILE_GEMM2 = 1u << 5,        // a configuration of gemm2.hip (else gemm.hip's kernel)
};
struct t2v_tile {
  int id, bm, bn, waves;
  int per_cu;                      // workgroups per CU the lowering's co-residency bound assumes
  unsigned features;
  constexpr bool has(unsigned f) const { return (features & f) != 0; }
};
inline constexpr t2v_tile T2V_TILES[] = {
    // Tile 0 is the 128x128-class kernel of gemm.hip.  It ALSO has a narrow 128x64 form, taken when the last 128-wide column tile would
    // be at most half full (t2v_tile0_narrow); that form has no fused instantiation, so the fused epilogues of tile 0 need N % 128 == 0.
    {0, 128, 128, 4, 2, T2V_TILE_GN | T2V_TILE_LNX | T2V_TILE_XATTN},
    {1, 256, 256, 8, 1, T2V_TILE_GEMM2},
    {2, 256, 320, 8, 1, T2V_TILE_GEMM2 | T2V_TILE_LN},
    {3, 128, 256, 8, 1, T2V_TILE_GEMM2 | T2V_TILE_GN | T2V_TILE_LNX},
    {4, 128, 128, 4, 1, T2V_TILE_GEMM2},
    {5, 128, 128, 8, 1, T2V_TILE_GEMM2 | T2V_TILE_GN | T2V_TILE_LNX | T2V_TILE_XATTN},
    {8, 192, 320, 12, 1, T2V_TILE_GEMM2 | T2V_TILE_GN | T2V_TILE_LN | T2V_TILE_XATTN},
    {9, 192, 256, 12, 1, T2V_TILE_GEMM2 | T2V_TILE_LNX},
    {10, 192, 192, 12, 1, T2V_TILE_GEMM2 | T2V_TILE_TATTN_ONLY},
    {11, 128, 320, 8, 1, T2V_TILE_GEMM2 | T2V_TILE_GN | T2V_TILE_LN | T2V_TILE_XATTN},
    {12, 64, 64, 4, 2, T2V_TILE_GEMM2 | T2V_TILE_LNX},
};
constexpr int T2V_TILE0_NARROW_BN = 64;
constexpr bool t2v_tile0_narrow(int N) { return N % 128 != 0 && N % 128 <= T2V_TILE0_NARROW_BN; }
// the entry of a tile id; nullptr for an id without a kernel
constexpr const t2v_tile* t2v_tile_of(int id) {
  for (const t2v_tile& t : T2V_TILES)
    if (t.id == id) return &t;
  return nullptr;
}
// May a GEMM of N columns run fused epilogue `feature` (ONE bit) on tile t?
constexpr bool t2v_tile_fuses(const t2v_tile* t, unsigned feature, int N) {
  if (t == nullptr || !t->has(feature)) return false;
  if (feature == T2V_TILE_LN || (feature == T2V_TILE_XATTN && t->has(T2V_TILE_LN))) return N == t->bn;   // whole rows in the tile
  if (feature == T2V_TILE_XATTN) return N % t->bn == 0;                                                   // whole heads per column tile
  return t->has(T2V_TILE_GEMM2) || N % t->bn == 0;                                                        // gemm.hip's kernel: see tile 0 above
}

// Each returns hipSuccess or the launch error.
hipError_t t2v_launch_gemm(const GemmParams& p, hipStream_t s);             // 128x128 / 128x64 tiles (any N, C8 stem)
hipError_t t2v_launch_gemm2(const GemmParams& p, int tile, hipStream_t s);  // 256/128 x 256/320 tiles, deep DMA ring
hipError_t t2v_launch_ff_fused(const GemmParams& geglu, const GemmParams& proj, hipStream_t s);   // the C = 320 GEGLU feed-forward pair as one launch (gemm2.hip)
hipError_t t2v_launch_splitk_reduce(const GemmParams& p, hipStream_t s);
hipError_t t2v_launch_splitk_reduce_gn(const GemmParams& p, hipStream_t s);   // split-K reduction + the GroupNorm (+SiLU) that consumes the result, one cooperative launch (norm.hip)
hipError_t t2v_launch_groupnorm(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_layernorm(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_attention(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_relpos_attention(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_softmax(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_ncthw_to_cl(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_cl_to_ncthw(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_to_uint8(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_resample(const t2v_op& op, hipStream_t s);            // uint8 Lanczos pass (i[9] = 0) | float bicubic resize (i[9] = 1)
hipError_t t2v_launch_depth_tokens(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_avgpool2(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_emphasis(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_fingerprint(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_lora_merge(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_reshard_rows(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_time_embed(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_copy2d(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_ddim_step(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_lincomb(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_embed_rows(const t2v_op& op, hipStream_t s);
hipError_t t2v_launch_freeu(const t2v_op& op, hipStream_t s);               // freeu.hip

// The T2V_OP_FREEU record, decoded once (freeu.hip): validation, the slot extents and the launcher all ask here.  ok = false: the record
// is refused, `why` says why
struct t2v_freeu_view { bool ok; const char* why; int rows, c_total, ld, c_h, frames, h, w; float b, s; uint64_t buf; };
t2v_freeu_view t2v_freeu_decode(const t2v_op& op);

// What a T2V_OP_DDIM_STEP record is (elementwise.hip): validation, the output slots and the launcher all ask here.  x0_form: which x0
// the measure pass ranks (0 the DDIM_Gaussian step, 1 UniPC's data prediction); why: the reason a T2V_DDIM_MALFORMED record is refused
enum t2v_ddim_form { T2V_DDIM_MALFORMED, T2V_DDIM_PLAIN, T2V_DDIM_BLEND, T2V_DDIM_RESTRICT, T2V_DDIM_MEASURE, T2V_DDIM_THRESHOLD, T2V_DDIM_INVERT, T2V_DDIM_KEYFRAME };
struct t2v_ddim_class { t2v_ddim_form form; int x0_form; const char* why; };
t2v_ddim_class t2v_ddim_classify(const t2v_op& op);
// Why a context-window form of T2V_OP_LINCOMB (i[9] = 1 blend, 2 gather; elementwise.hip) is refused, or null: validation and the launcher ask here
const char* t2v_window_refusal(const t2v_op& op);
// What a T2V_OP_ATTENTION record is (attention.hip): validation, the slot extents and the launcher ask here.  vt_waves: attn2_kernel's waves
enum t2v_attention_form { T2V_ATTN_MALFORMED, T2V_ATTN_PLAIN, T2V_ATTN_SECOND_ROLE, T2V_ATTN_TABLE, T2V_ATTN_VT };
struct t2v_attention_class { t2v_attention_form form; int head_dim, vt_waves; const char* why; };
t2v_attention_class t2v_attention_classify(const t2v_op& op);
// The launch grid of a T2V_OP_RESAMPLE record (elementwise.hip), uint8 pass or bicubic: rows x tiles workgroups of 256 units
struct t2v_resample_grid { long rows, units, tiles; };
t2v_resample_grid t2v_resample_grid_of(const t2v_op& op);

// x * sigmoid(x) as 5 VALU instructions (v_exp_f32 and v_rcp_f32 are 1-ulp; an IEEE divide would be ~12 more)
__device__ __forceinline__ float t2v_silu(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896340736f));
}

// ---- the two pieces every GroupNorm form shares (norm.hip's kernels, t2v_epilogue_rows_gn; t2v_mean_rstd also t2v_epilogue_rows_lnx) ----
template <int N> using f32xN = float __attribute__((ext_vector_type(N)));
template <int N> using f16xN = f16 __attribute__((ext_vector_type(N)));
// {mean, rstd} of n = 1 / inv_n values from their fp64 sum and sum of squares.  The statistics of one instance must come out bit-identical
// in every workgroup of a launch and on every T-shard rank: this is the ONLY place the expression is written.
__device__ __forceinline__ float2 t2v_mean_rstd(double s, double q, double inv_n, float eps) {
  const double m = s * inv_n;
  double var = q * inv_n - m * m;
  var = var < 0.0 ? 0.0 : var;
  return float2{(float)m, (float)(1.0 / sqrt(var + (double)eps))};
}
// y = v * a + b (+SiLU) for N = 4 / 8 consecutive channels of one row -> fp16 at dst, and, lo_off != 0, the low-order image y - (float)hi
// at dst + lo_off (hi + lo operand split): one or two N-wide stores.  `silu` is a constant at every call site but the GEMM epilogue's.
template <int N>
__device__ __forceinline__ void t2v_norm_store(f16* dst, int lo_off, const f32xN<N>& v, const f32xN<N>& a, const f32xN<N>& b, bool silu) {
  f16xN<N> o, l;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    float y = v[e] * a[e] + b[e];
    if (silu) y = t2v_silu(y);
    o[e] = (f16)y;
    l[e] = (f16)(y - (float)o[e]);
  }
  *reinterpret_cast<f16xN<N>*>(dst) = o;
  if (lo_off) *reinterpret_cast<f16xN<N>*>(dst + lo_off) = l;
}

// 16-byte LDS-DMA of the GEMM operand stages: lane l's 16 bytes at gsrc land at lds_wave_base + 16 l
#define T2V_AS1 __attribute__((address_space(1)))
#define T2V_AS3 __attribute__((address_space(3)))
__device__ __forceinline__ void t2v_glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const T2V_AS1 void*)gsrc, (T2V_AS3 void*)lds_wave_base, 16, 0, 0);
}

// Per-lane split-K slab store of a wave's TM x TN accumulator blocks (rows from m_wave, packed columns from n_wave) into slab
// `split_idx` of p.ws: the whole tail of both GEMM kernels — the epilogue proper then runs in splitk_reduce_kernel.  (The plain
// epilogue writes its slabs row-coalesced in t2v_epilogue_rows below and never gets here.)
template <int TM, int TN>
__device__ __forceinline__ void t2v_store_splitk_slab(const GemmParams& p, const f32x16 (&acc)[TM][TN], int lane, int m_wave, int n_wave,
                                                      int split_idx) {
  const int mlane = lane & 31, nhalf = (lane >> 5) * 4;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int m = m_wave + a * 32 + mlane;
    if (m >= p.M) continue;
    float* ws = p.ws + ((size_t)split_idx * p.M + m) * p.N;
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n_wave + b * 32 + 8 * q + nhalf;
        if (n < p.N) {
          f32x4 o = {acc[a][b][4 * q], acc[a][b][4 * q + 1], acc[a][b][4 * q + 2], acc[a][b][4 * q + 3]};
          *reinterpret_cast<f32x4*>(ws + n) = o;
        }
      }
  }
}

// ---- row-coalesced GEMM epilogue (shared by gemm.hip and gemm2.hip) -----------------------------------
// In the MFMA accumulator layout a lane owns 4 consecutive channels of ONE token row, so a wave-wide store (or
// residual load) touches 32 rows x 32 bytes: 32 cache lines per instruction, and the memory pipeline — not the
// bytes — bounds the epilogue (measured: fp16 and fp32 outputs cost the same, the residual read adds as much again).
// Every 32x32 accumulator block is therefore turned through a small per-wave LDS buffer (32 x T2V_EPI_SP floats) so
// that 8 lanes cover one whole 128-byte row: 8 lines per instruction for the stores, the residual and the row-bias
// loads alike.  Same-box A/B on the 24-frame UNet step: 31.4 ms vs 31.9 ms with per-lane row-strided stores.
// Handles T2V_EPI_NONE (bias / row bias / SiLU / fp32 residual / fp16|fp32 out) and the split-K slab stores.
// The fp32 residual stream: read once by the GEMM that adds to it, written once for the next residual GEMM (tens of MB per launch at the
// 32x32 / 16x16 levels).  (Non-temporal hints on these accesses were measured neutral in round 4 and are gone.)
__device__ __forceinline__ f32x4 t2v_ld_stream(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void t2v_st_stream(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

constexpr int T2V_EPI_SP = 36;     // floats per staged row: 16-lane phases of the 16-byte LDS accesses hit disjoint banks

template <int TM, int TN>
__device__ __forceinline__ void t2v_epilogue_rows(const GemmParams& p, const f32x16 (&acc)[TM][TN], float* stg, int lane,
                                                  int m_wave, int n_wave, int split_idx, int tile_id = 0) {
  const int wrow = lane & 31, wcol = (lane >> 5) * 4;
  const int rrow = lane >> 3, rcol = (lane & 7) * 4;
  // Residual prefetch: the four row loads of a 32x32 block are issued TOGETHER and one block ahead of their use (always
  // from a readable address: rows / columns outside the matrix park on the first element), so the epilogue keeps
  // 8 KiB of residual reads per wave in flight instead of paying one dependent load -> add -> store chain per row
  // (same-box A/B on the 24-frame UNet step: the C = 320 residual Linears 50.5 -> 44 us, step 34.05 -> 33.5 ms).
  const bool has_res = p.splitk == 1 && p.res != nullptr;
  auto res_load = [&](int blk, f32x4 (&r)[4]) {
    const int mt = m_wave + (blk / TN) * 32, n = n_wave + (blk % TN) * 32 + rcol;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mt + rrow + 8 * i;
      const int mr = (p.res_wrap && m >= p.res_wrap) ? m - p.res_wrap : m;          // shared (one-sample) residual: rows wrap once
      const float* src = (m < p.M && n < p.N) ? p.res + (size_t)mr * p.ldr + n : p.res;
      r[i] = t2v_ld_stream(src);
    }
  };
  f32x4 rcur[4], rnxt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { rcur[i] = f32x4{0.f, 0.f, 0.f, 0.f}; rnxt[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  if (has_res) res_load(0, rcur);
#pragma unroll
  for (int blk = 0; blk < TM * TN; ++blk) {
    const int a = blk / TN, b = blk % TN;
    if (has_res && blk + 1 < TM * TN) res_load(blk + 1, rnxt);
    const int mt = m_wave + a * 32;
    const int nt = n_wave + b * 32;
    if (mt < p.M && nt < p.N) {                                // wave-uniform
      f32x4 ssum = {0.f, 0.f, 0.f, 0.f}, ssq = {0.f, 0.f, 0.f, 0.f};   // T2V_EPI_STATS: this lane's 4 rows x 4 columns of the block
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = {acc[a][b][4 * q], acc[a][b][4 * q + 1], acc[a][b][4 * q + 2], acc[a][b][4 * q + 3]};
        *reinterpret_cast<f32x4*>(stg + wrow * T2V_EPI_SP + 8 * q + wcol) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the same wave reads back: LDS ops stay in program order
      const int n = nt + rcol;
      const bool ncol = n < p.N;
      f32x4 cb = {0.f, 0.f, 0.f, 0.f};                         // this lane's 4 columns are the same for all its rows
      if (p.splitk == 1 && p.bias && !p.bias_m && ncol) cb = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = rrow + 8 * i;
        f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * T2V_EPI_SP + rcol);
        const int m = mt + row;
        if (m < p.M && ncol) {
          if (p.splitk > 1) {
            float* slab = p.ws + ((size_t)split_idx * p.M + m) * p.N + n;
            if (p.tickets) t2v_st_dev(slab, v);                  // read by another workgroup of this launch: write through
            else *reinterpret_cast<f32x4*>(slab) = v;            // read by the reduction kernel that follows
            continue;
          }
          v += cb;
          if (p.bias && p.bias_m) { const float bm = p.bias[m]; v[0] += bm; v[1] += bm; v[2] += bm; v[3] += bm; }
          if (p.rowbias) v += *reinterpret_cast<const f32x4*>(p.rowbias + (size_t)(m / p.rows_per_batch) * p.ldrb + n);
          if (p.act == 1) { v[0] = t2v_silu(v[0]); v[1] = t2v_silu(v[1]); v[2] = t2v_silu(v[2]); v[3] = t2v_silu(v[3]); }
          else if (p.act == 2) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
          if (has_res) v += rcur[i];
          if (p.out_f32) {
            t2v_st_stream(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n, v);
            if (p.stats) { ssum += v; ssq += v * v; }
          } else {
            f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
            f16* dst = reinterpret_cast<f16*>(p.out) + (size_t)m * p.ldc + n;
            *reinterpret_cast<f16x4*>(dst) = o;
            if (p.out_lo) {
              const f16x4 l = {(f16)(v[0] - (float)o[0]), (f16)(v[1] - (float)o[1]), (f16)(v[2] - (float)o[2]), (f16)(v[3] - (float)o[3])};
              *reinterpret_cast<f16x4*>(dst + p.N) = l;
            }
            if (p.stats) {                                       // statistics of the STORED (fp16-rounded) values: what the GroupNorm normalises
              const f32x4 sv = {(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
              ssum += sv; ssq += sv * sv;
            }
          }
        }
      }
      if (p.stats) {                                             // wave-uniform
        // the 8 lanes with the same (lane & 7) hold the other rows of these 4 columns: fixed butterfly over lane bits 3, 4, 5
#pragma unroll
        for (int o = 8; o < 64; o <<= 1)
#pragma unroll
          for (int e = 0; e < 4; ++e) { ssum[e] += __shfl_xor(ssum[e], o); ssq[e] += __shfl_xor(ssq[e], o); }
        if (lane < 8 && ncol) {
          float* st = p.stats + (size_t)(mt >> 5) * 2 * p.N + n;
          *reinterpret_cast<f32x4*>(st) = ssum;
          *reinterpret_cast<f32x4*>(st + p.N) = ssq;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) rcur[i] = rnxt[i];
  }
  if (p.splitk > 1 && p.tickets != nullptr) {
    // ---- split-K fold by the last-arriving workgroup of this output tile (no splitk_reduce launch) -------------------------
    // Every workgroup has stored its slab above (device-scope write-through stores).  stores complete -> ticket -> the last
    // arrival (ticket == splitk - 1) re-arms the counter and sums ALL slabs in split order 0 .. splitk-1 with device-scope
    // loads (its own included): the same values in the same order as the reduction kernel this replaces, whichever workgroup
    // happens to be last — bitwise reproducible.
    __shared__ int s_last;
    t2v_wait_vm0();
    __syncthreads();
    if (threadIdx.x == 0) {
      const int t = __hip_atomic_fetch_add(p.tickets + tile_id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = t == p.splitk - 1;
      if (s_last) __hip_atomic_store(p.tickets + tile_id, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last) return;
#pragma unroll
    for (int blk = 0; blk < TM * TN; ++blk) {
      const int mt = m_wave + (blk / TN) * 32, nt = n_wave + (blk % TN) * 32;
      if (mt >= p.M || nt >= p.N) continue;                    // wave-uniform
      const int n = nt + rcol;
      if (n >= p.N) continue;
      f32x4 cb = {0.f, 0.f, 0.f, 0.f};
      if (p.bias && !p.bias_m) cb = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mt + rrow + 8 * i;
        if (m >= p.M) continue;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const float* col = p.ws + (size_t)m * p.N + n;
        const size_t zs = (size_t)p.M * p.N;
        for (int z = 0; z < p.splitk; z += 4) {                  // four slabs in flight; missing ones re-read slab 0 and are dropped
          f32x4 t0 = t2v_ld_dev(col + (size_t)z * zs);
          f32x4 t1 = t2v_ld_dev(col + (size_t)(z + 1 < p.splitk ? z + 1 : 0) * zs);
          f32x4 t2 = t2v_ld_dev(col + (size_t)(z + 2 < p.splitk ? z + 2 : 0) * zs);
          f32x4 t3 = t2v_ld_dev(col + (size_t)(z + 3 < p.splitk ? z + 3 : 0) * zs);
          t2v_wait_dev(t0, t1, t2, t3);
          v += t0;
          if (z + 1 < p.splitk) v += t1;
          if (z + 2 < p.splitk) v += t2;
          if (z + 3 < p.splitk) v += t3;
        }
        v += cb;
        if (p.bias && p.bias_m) { const float bm = p.bias[m]; v[0] += bm; v[1] += bm; v[2] += bm; v[3] += bm; }
        if (p.rowbias) v += *reinterpret_cast<const f32x4*>(p.rowbias + (size_t)(m / p.rows_per_batch) * p.ldrb + n);
        if (p.act == 1) { v[0] = t2v_silu(v[0]); v[1] = t2v_silu(v[1]); v[2] = t2v_silu(v[2]); v[3] = t2v_silu(v[3]); }
        else if (p.act == 2) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
        if (p.res) v += *reinterpret_cast<const f32x4*>(p.res + (size_t)((p.res_wrap && m >= p.res_wrap) ? m - p.res_wrap : m) * p.ldr + n);
        if (p.out_f32) {
          t2v_st_stream(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n, v);
        } else {
          f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
          f16* dst = reinterpret_cast<f16*>(p.out) + (size_t)m * p.ldc + n;
          *reinterpret_cast<f16x4*>(dst) = o;
          if (p.out_lo) {
            const f16x4 l = {(f16)(v[0] - (float)o[0]), (f16)(v[1] - (float)o[1]), (f16)(v[2] - (float)o[2]), (f16)(v[3] - (float)o[3])};
            *reinterpret_cast<f16x4*>(dst + p.N) = l;
          }
        }
      }
    }
  }
}
// Epilogue of the 192x320 tile (12 waves: 6 row strips x 2 column halves, TM = 1, TN = 5) with a fused LayerNorm: the tile
// holds WHOLE rows (N == 320), so after bias / residual the fp32 result goes to `out` as usual and, from the values kept
// in the accumulator registers, LayerNorm(row) * gamma + beta goes to `ln_out` (fp16) — the separate LayerNorm launch
// (read fp32, write fp16: 94 MB at the 32x32 level) and its launch boundary disappear.  Two-pass statistics (mean, then
// centred squares) like the stand-alone kernel; the two waves of a row strip exchange their half-row sums through LDS.
template <int TN>
__device__ __forceinline__ void t2v_epilogue_rows_ln(const GemmParams& p, f32x16 (&acc)[1][TN], float* stg, float* xch, int lane,
                                                     int wave, int m_wave, int n_wave) {
  const int wrow = lane & 31, wcol = (lane >> 5) * 4;
  const int rrow = lane >> 3, rcol = (lane & 7) * 4;
  const bool has_res = p.res != nullptr;
  auto res_load = [&](int blk, f32x4 (&r)[4]) {
    const int n = n_wave + blk * 32 + rcol;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m_wave + rrow + 8 * i;
      const int mr = (p.res_wrap && m >= p.res_wrap) ? m - p.res_wrap : m;
      const float* src = (m < p.M && n < p.N) ? p.res + (size_t)mr * p.ldr + n : p.res;
      r[i] = t2v_ld_stream(src);
    }
  };
  f32x4 rcur[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rcur[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    if (has_res) res_load(b, rcur);                    // four row loads in flight while the block turns through LDS
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = {acc[0][b][4 * q], acc[0][b][4 * q + 1], acc[0][b][4 * q + 2], acc[0][b][4 * q + 3]};
      *reinterpret_cast<f32x4*>(stg + wrow * T2V_EPI_SP + 8 * q + wcol) = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const int n = n_wave + b * 32 + rcol;
    f32x4 cb = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) cb = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rrow + 8 * i;
      f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * T2V_EPI_SP + rcol);
      const int m = m_wave + row;
      v += cb;
      if (has_res) v += rcur[i];
      if (m < p.M) t2v_st_stream(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n, v);
      acc[0][b][4 * i] = v[0]; acc[0][b][4 * i + 1] = v[1]; acc[0][b][4 * i + 2] = v[2]; acc[0][b][4 * i + 3] = v[3];   // row-major now
      rs[i] += (v[0] + v[1]) + (v[2] + v[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }
  // half-row sums -> whole-row mean: 8 lanes share a row (xor 1, 2, 4), the partner wave (other column half) through LDS
  float* mine = xch + wave * 32;
  float* other = xch + (wave ^ 1) * 32;
  float mean[4], rstd[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float s = rs[i];
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
    rs[i] = s;
    if ((lane & 7) == 0) mine[rrow + 8 * i] = s;
  }
  __syncthreads();
  const float inv_n = 1.0f / (float)p.N;
#pragma unroll
  for (int i = 0; i < 4; ++i) mean[i] = (rs[i] + other[rrow + 8 * i]) * inv_n;
  float rq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < TN; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = acc[0][b][4 * i + e] - mean[i]; rq[i] += d * d; }
  __syncthreads();                                   // every wave has read its partner's sums: the slots are reused
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float q = rq[i];
    q += __shfl_xor(q, 1); q += __shfl_xor(q, 2); q += __shfl_xor(q, 4);
    rq[i] = q;
    if ((lane & 7) == 0) mine[rrow + 8 * i] = q;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) rstd[i] = rsqrtf((rq[i] + other[rrow + 8 * i]) * inv_n + p.ln_eps);
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int n = n_wave + b * 32 + rcol;
    const f32x4 g = *reinterpret_cast<const f32x4*>(p.ln_gb + n);
    const f32x4 be = *reinterpret_cast<const f32x4*>(p.ln_gb + p.N + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m_wave + rrow + 8 * i;
      if (m < p.M) {
        f16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (f16)((acc[0][b][4 * i + e] - mean[i]) * rstd[i] * g[e] + be[e]);
        *reinterpret_cast<f16x4*>(p.ln_out + (size_t)m * p.ld_ln + n) = o;
      }
    }
  }
}

// ---- bounded two-level grid barrier (shared by the single-pass GroupNorm of norm.hip and the fused-norm GEMM epilogues) -----------
// Sense-reversing on words of the program's zero-initialised sync buffer.  Two levels, because atomics on ONE address serialise at
// ~25 ns each (256 arrivals = 6 us): workgroup b arrives at counter b % 8 (its own 128-byte line), the last arrival of each counter
// re-arms it and arrives at the top counter, the last of those re-arms that and bumps the generation word every waiter polls.
// Counters return to 0 and the generation only grows, so nothing needs a reset between launches.  All flag accesses are relaxed
// device-scope atomics (no cache-wide write-back / invalidate); the data exchanged around it moves with device-scope (sc1) stores
// that their writers waited for (s_waitcnt vmcnt(0)) before arriving, and device-scope loads after it.
// Split in two so that work which does not depend on the other workgroups (the fp32 stream store of the fused-norm epilogues) can be
// issued between arriving and waiting.
// (Round 5 measured a single-round variant — eight monotonic 64-bit counters, a fire-and-forget arrival, every waiter polling all
// eight — and it was SLOWER: +8 us on the 240 / 480-workgroup launches of the 8x8 / 16x16 levels, equal at 256 workgroups: hundreds of
// pollers on the lines the arrivals go to delay the arrivals.  Here the waiters poll ONE word that nobody writes until the release.)
// The wait is BOUNDED: a waiter that sees no release within GNB_TIMEOUT_TICKS of the constant 100 MHz clock (0.25 s; a healthy
// barrier takes microseconds) raises the fault word in host-mapped memory and falls through — this launch's output is invalid, the
// device is not hung, the host reports the fault at its next call.
constexpr int GNB_STRIDE = 32;                       // ints between level-1 counters (one 128-byte line each)
constexpr int GNB_TOP = 8 * GNB_STRIDE, GNB_GEN = 9 * GNB_STRIDE;
constexpr unsigned long long GNB_TIMEOUT_TICKS = 25000000ull;
// thread 0 of every workgroup, any time before it arrives: the generation word (it cannot change before this workgroup has arrived)
__device__ __forceinline__ unsigned t2v_grid_epoch(unsigned* bar) { return __hip_atomic_load(bar + GNB_GEN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// arrive (callers: every wave has waited for its own published stores, t2v_wait_vm0(), before).  Returns, in thread 0, whether this
// workgroup was the last to arrive — hand it to t2v_grid_wait.
__device__ __forceinline__ bool t2v_grid_arrive(unsigned* bar, unsigned nwg) {
  __syncthreads();
  bool release = false;
  if (threadIdx.x == 0) {
    const unsigned grp = blockIdx.x & 7u;
    const unsigned ngrp = nwg < 8u ? nwg : 8u;
    const unsigned in_grp = (nwg - grp + 7u) >> 3;                                   // workgroups b with b % 8 == grp
    t2v_wait_vm0();
    if (__hip_atomic_fetch_add(bar + grp * GNB_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_grp - 1) {
      __hip_atomic_store(bar + grp * GNB_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__hip_atomic_fetch_add(bar + GNB_TOP, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngrp - 1) {
        __hip_atomic_store(bar + GNB_TOP, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        release = true;
      }
    }
    if (release) {
      t2v_wait_vm0();                                                                // every counter re-armed before anyone leaves
      __hip_atomic_fetch_add(bar + GNB_GEN, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  return release;
}
__device__ __forceinline__ void t2v_grid_wait(unsigned* bar, unsigned gen, bool released, unsigned* fault) {
  if (threadIdx.x == 0 && !released) {
    const unsigned long long t0 = wall_clock64();
    unsigned polls = 0;
    while (__hip_atomic_load(bar + GNB_GEN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) {
      __builtin_amdgcn_s_sleep(8);
      if ((++polls & 63u) == 0u && wall_clock64() - t0 > GNB_TIMEOUT_TICKS) {        // give up: flag it, never hang the device
        __hip_atomic_store(fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void t2v_grid_barrier(unsigned* bar, unsigned nwg, unsigned gen, unsigned* fault) {
  const bool released = t2v_grid_arrive(bar, nwg);
  t2v_grid_wait(bar, gen, released, fault);
}

// ---- tagged records: the exchange without a barrier (round 5) ------------------------------------------------------------------------
// What the workgroups of a fused-norm launch exchange is small: one {sum, sum of squares} fp64 pair per (tile, group) or per row.  With
// the barrier the chain publish -> s_waitcnt -> returning atomic -> second-level atomic -> generation bump -> poll -> fold loads is
// ~7 dependent device-scope round trips (measured: +9 .. 12 us on the producing GEMM).  A record that says by itself whether it is the
// one of THIS launch needs none of that: the 16-byte record carries the launch's 32-bit sequence number (handed out by the library,
// never 0, never repeated within 2^32 launches) in the 16 low mantissa bits of each double — 2^-36 relative, far below the fp32
// inputs of the sums — and a consumer simply loads the records it needs (device-scope loads) and re-loads the ones whose tag is not
// this launch's yet: publish -> (flight) -> load.  Tearing: the record leaves as ONE 16-byte store and is read by ONE 16-byte load (observed
// untorn on gfx950, not an architectural guarantee), so BOTH 8-byte halves carry bits that change on every launch — double 0 the low 16
// bits of the sequence number, double 1 those bits XOR the high 16 (the pair still encodes all 32 bits): a record torn at the 8-byte
// boundary between two launches (new {sum, tag} beside a stale {sum of squares, tag}) fails the test and is just re-polled.  Every
// consumer strips the tags the same way and adds the records in index order only once ALL of a round are fresh: bit-identical
// statistics in every workgroup, run to run.  The wait is bounded exactly as the barrier's (fault word, 0.25 s).
__device__ __forceinline__ f32x4 t2v_rec_pack(double a, double b, unsigned seq) {
  union { double d[2]; unsigned long long u[2]; f32x4 v; } r;
  r.d[0] = a;
  r.d[1] = b;
  r.u[0] = (r.u[0] & ~0xFFFFull) | (unsigned long long)(seq & 0xFFFFu);
  r.u[1] = (r.u[1] & ~0xFFFFull) | (unsigned long long)((seq ^ (seq >> 16)) & 0xFFFFu);
  return r.v;
}
__device__ __forceinline__ bool t2v_rec_fresh(const f32x4& v, unsigned want) {
  union { f32x4 v; unsigned long long u[2]; } r;
  r.v = v;
  return (unsigned)(r.u[0] & 0xFFFFull) == (want & 0xFFFFu) && (unsigned)(r.u[1] & 0xFFFFull) == ((want ^ (want >> 16)) & 0xFFFFu);
}
__device__ __forceinline__ void t2v_rec_add(const f32x4& v, double& a, double& b) {
  union { f32x4 v; unsigned long long u[2]; double d[2]; } r;
  r.v = v;
  r.u[0] &= ~0xFFFFull;
  r.u[1] &= ~0xFFFFull;
  a += r.d[0];
  b += r.d[1];
}
// Fetch the first `n` (<= NR) of the records addr(0 .. NR-1) into t[]: all loads in flight together; want != 0: re-load those whose tag is
// not `want` yet (bounded); want == 0: the caller has synchronised otherwise (barrier mode), one round.
// Four device-scope 16-byte loads AND their completion in ONE asm statement: the values are valid when it ends.  (A load in its own
// asm statement is only safe while nothing touches its destination before the separate s_waitcnt — under register pressure the compiler
// spills or copies the destination in between and reads it before the data has landed: measured, tile 8 of the first tagged build.)
__device__ __forceinline__ void t2v_ld_dev4(const float* p0, const float* p1, const float* p2, const float* p3, f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
  asm volatile(
      "global_load_dwordx4 %0, %4, off sc1\n\t"
      "global_load_dwordx4 %1, %5, off sc1\n\t"
      "global_load_dwordx4 %2, %6, off sc1\n\t"
      "global_load_dwordx4 %3, %7, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
      : "v"(p0), "v"(p1), "v"(p2), "v"(p3)
      : "memory");
}
// Fetch the first `n` (1 .. NR) of the records addr(0 .. NR-1) into t[] (slots >= n hold a copy of record 0); want != 0: poll until
// every one of them carries this launch's tag (bounded); want == 0: the caller has synchronised otherwise (barrier mode), one round.
template <int NR, typename F>
__device__ __forceinline__ void t2v_rec_fetch(F addr, int n, unsigned want, unsigned* fault, f32x4 (&t)[NR]) {
  static_assert(NR == 4 || NR == 8, "4 or 8 records in flight");
  const float* a[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) a[j] = addr(j < n ? j : 0);
  unsigned long long t0 = 0;
  unsigned polls = 0;
  for (;;) {
    t2v_ld_dev4(a[0], a[1], a[2], a[3], t[0], t[1], t[2], t[3]);
    if constexpr (NR == 8) t2v_ld_dev4(a[4], a[5], a[6], a[7], t[4], t[5], t[6], t[7]);
    if (want == 0u) break;
    bool fresh = true;
#pragma unroll
    for (int j = 0; j < NR; ++j) fresh = fresh && t2v_rec_fresh(t[j], want);
    if (fresh) break;
    if (polls == 0) t0 = wall_clock64();
    __builtin_amdgcn_s_sleep(2);
    if ((++polls & 63u) == 0u && wall_clock64() - t0 > GNB_TIMEOUT_TICKS) {         // give up: flag it, never hang the device
      __hip_atomic_store(fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      break;
    }
  }
}
template <typename F>
__device__ __forceinline__ void t2v_rec_fetch8(F addr, int n, unsigned want, unsigned* fault, f32x4 (&t)[8]) { t2v_rec_fetch<8>(addr, n, want, fault, t); }

// ---- GroupNorm (+SiLU) of a GEMM's result inside its epilogue (T2V_EPI_GN, round 5) -----------------------------------------------
// Replaces nn.GroupNorm(32, C) [+ SiLU] where its input is the result of ONE convolution / linear of this library (reference:
// ResBlock in_layers conv -> out_layers norm t2v_model.py:929-957, TemporalConvBlock_v2 conv_i -> conv_{i+1} norm :1201-1212, block
// output -> next block's norm): the stand-alone kernel re-reads the tensor the GEMM just wrote (and, for a tensor only the norm
// consumes, the GEMM wrote it only for that) and pays a launch boundary; here the workgroup's fp32 tile never leaves its registers.
//   A  every 32x32 accumulator block is turned through the per-wave LDS buffer (as t2v_epilogue_rows), bias / row bias / residual
//      added, the fp32 (fp16) stream stored if anyone else needs it, the value kept in the accumulator registers (now row-major),
//      its 32-row column sums and sums of squares folded over the 8 lanes that share a column quad -> LDS [strip][2][BN];
//   B  per (instance slot, group piece) — a tile of BM <= rows-per-instance rows touches at most 2 statistics instances, a column
//      tile cuts a group into at most 2 pieces — 4 lanes fold strips x channels in fp64 in a fixed order and publish ONE
//      {sum, sum of squares} pair with a device-scope store: [tile_m][slot][tile_n][piece];
//   C  bounded grid barrier (every workgroup of the launch is resident: checked by the launcher);
//   D  8 lanes per (slot, group) fold the published pairs of every tile of the instance (and of both column tiles of a cut group)
//      in a fixed order — every workgroup the same values in the same order: bit-identical statistics, no atomics on data — then
//      t2v_mean_rstd, the expression the stand-alone kernels of norm.hip use;
//   E  scale / shift per (slot, column) in LDS, normalise (+SiLU) from registers, fp16 out (+ low-order image): t2v_norm_store.
// Rows >= M / columns >= N contribute zeros to the sums and are not stored.
template <int WM, int WN, int TM, int TN>
__device__ __forceinline__ void t2v_epilogue_rows_gn(const GemmParams& p, f32x16 (&acc)[TM][TN], unsigned char* smem, int lane, int wave,
                                                     int m0, int n0, int tile_m, int tile_n, int tiles_m, int tiles_n) {
  constexpr int NW = WM * WN, NT = NW * 64, S = WM * TM, BM = S * 32, BN = WN * TN * 32;
  const int tid = threadIdx.x;
  const int wm = wave / WN, wn = wave % WN;
  float* stg = reinterpret_cast<float*>(smem) + wave * (32 * T2V_EPI_SP);
  float* colsum = reinterpret_cast<float*>(smem) + NW * (32 * T2V_EPI_SP);       // [S][2][BN]
  float* scsf = colsum + S * 2 * BN;                                             // [2 slots][scale | shift][BN]
  float* stat = scsf + 4 * BN;                                                   // [2 slots][T2V_GN_PIECES][mean | rstd]
  const int wrow = lane & 31, wcol = (lane >> 5) * 4;
  const int rrow = lane >> 3, rcol = (lane & 7) * 4;
  const bool tags = p.gn_seq != 0u;
  unsigned gen0 = 0;
  if (!tags && tid == 0) gen0 = t2v_grid_epoch(p.gn_bar);
  const bool has_res = p.res != nullptr;
  // ---- A
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int mt = m0 + (wm * TM + a) * 32;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int n = n0 + (wn * TN + b) * 32 + rcol;
      const bool ncol = n < p.N;
      f32x4 r[4];
      if (has_res) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = mt + rrow + 8 * i;
          const int mr = (p.res_wrap && m >= p.res_wrap) ? m - p.res_wrap : m;
          const float* src = (m < p.M && ncol) ? p.res + (size_t)mr * p.ldr + n : p.res;
          r[i] = t2v_ld_stream(src);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = {acc[a][b][4 * q], acc[a][b][4 * q + 1], acc[a][b][4 * q + 2], acc[a][b][4 * q + 3]};
        *reinterpret_cast<f32x4*>(stg + wrow * T2V_EPI_SP + 8 * q + wcol) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      f32x4 cb = {0.f, 0.f, 0.f, 0.f};
      if (p.bias && !p.bias_m && ncol) cb = *reinterpret_cast<const f32x4*>(p.bias + n);
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = rrow + 8 * i;
        f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * T2V_EPI_SP + rcol);
        const int m = mt + row;
        if (m < p.M && ncol) {
          v += cb;
          if (p.bias && p.bias_m) { const float bm = p.bias[m]; v[0] += bm; v[1] += bm; v[2] += bm; v[3] += bm; }
          if (p.rowbias) v += *reinterpret_cast<const f32x4*>(p.rowbias + (size_t)(m / p.rows_per_batch) * p.ldrb + n);
          if (p.act == 1) { v[0] = t2v_silu(v[0]); v[1] = t2v_silu(v[1]); v[2] = t2v_silu(v[2]); v[3] = t2v_silu(v[3]); }
          else if (p.act == 2) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
          if (has_res) v += r[i];
        } else {
          v = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        acc[a][b][4 * i] = v[0]; acc[a][b][4 * i + 1] = v[1]; acc[a][b][4 * i + 2] = v[2]; acc[a][b][4 * i + 3] = v[3];   // row-major now
        s4 += v;
        q4 += v * v;
      }
      // the 8 lanes with the same (lane & 7) hold the other rows of these 4 columns: fixed butterfly over lane bits 3, 4, 5
#pragma unroll
      for (int o = 8; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s4[e] += __shfl_xor(s4[e], o); q4[e] += __shfl_xor(q4[e], o); }
      if (lane < 8) {
        float* cs = colsum + (size_t)(wm * TM + a) * 2 * BN + (wn * TN + b) * 32 + rcol;
        *reinterpret_cast<f32x4*>(cs) = s4;
        *reinterpret_cast<f32x4*>(cs + BN) = q4;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
  }
  __syncthreads();
  // ---- B
  const int R = p.gn_rows, cpg = p.gn_cpg;
  const int n_hi = min(n0 + BN, p.N);
  const int g_lo = n0 / cpg, npc = (n_hi - 1) / cpg - g_lo + 1;                    // groups (pieces) this column tile touches
  const int inst0 = m0 / R;
  for (int base = 0; base < 2 * npc; base += NT / 4) {
    const int item = base + (tid >> 2), sub = tid & 3;
    const bool active = item < 2 * npc;
    const int slot = active ? item / npc : 0, pc = active ? item - slot * npc : 0;
    const int g = g_lo + pc;
    const int c_lo = max(g * cpg, n0) - n0, c_hi = min((g + 1) * cpg, n_hi) - n0;
    double ds = 0.0, dq = 0.0;
    if (active) {
      for (int st = 0; st < S; ++st) {
        if ((m0 + st * 32) / R - inst0 != slot) continue;
        const float* cs = colsum + (size_t)st * 2 * BN;
        for (int c = c_lo + sub; c < c_hi; c += 4) { ds += (double)cs[c]; dq += (double)cs[BN + c]; }
      }
    }
    ds += __shfl_xor(ds, 1); dq += __shfl_xor(dq, 1);
    ds += __shfl_xor(ds, 2); dq += __shfl_xor(dq, 2);
    if (active && sub == 0) {
      double* dst = p.gn_part + ((((size_t)tile_m * 2 + slot) * tiles_n + tile_n) * T2V_GN_PIECES + pc) * 2;
      t2v_st_dev(reinterpret_cast<float*>(dst), t2v_rec_pack(ds, dq, p.gn_seq));      // one 16-byte device-scope (write-through) store
    }
  }
  // ---- C: (barrier mode: arrive;) then — under the exchange's latency — the result itself goes out if anyone else reads it (from the
  // registers, row-major)
  bool released = false;
  if (!tags) {
    t2v_wait_vm0();                                                // ... complete before this workgroup arrives
    released = t2v_grid_arrive(p.gn_bar, gridDim.x);
  }
  if (p.gn_store_out) {
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      const int mt = m0 + (wm * TM + a) * 32;
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        const int n = n0 + (wn * TN + b) * 32 + rcol;
        if (n >= p.N) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = mt + rrow + 8 * i;
          if (m >= p.M) continue;
          const f32x4 v = {acc[a][b][4 * i], acc[a][b][4 * i + 1], acc[a][b][4 * i + 2], acc[a][b][4 * i + 3]};
          if (p.out_f32) {
            t2v_st_stream(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n, v);
          } else {
            const f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
            *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(p.out) + (size_t)m * p.ldc + n) = o;
          }
        }
      }
    }
  }
  if (!tags) t2v_grid_wait(p.gn_bar, gen0, released, p.gn_fault);
  // ---- D: as many lanes per (slot, group) as the workgroup has (a power of two, 8 .. 64): one round of loads in flight where possible
  const int last_inst = (min(m0 + BM, p.M) - 1) / R;               // instance of the tile's last real row (>= inst0, <= inst0 + 1)
  const double inv_n = 1.0 / ((double)R * cpg);
  const int nitems = (last_inst - inst0 + 1) * npc;
  int lpi = 8;
  while (lpi < 64 && nitems * (lpi * 2) <= NT) lpi *= 2;
  for (int base = 0; base < nitems; base += NT / lpi) {
    const int item = base + tid / lpi, sub = tid % lpi;
    const int slot = item < nitems ? item / npc : 2, pc = item < nitems ? item - slot * npc : 0;
    const bool active = slot < 2;
    double ds = 0.0, dq = 0.0;
    if (active) {
      const int g = g_lo + pc, inst = inst0 + slot;
      const int tb = p.m_begin / BM;                              // first (global) row tile of this launch: the records are indexed by LOCAL tile
      const int t_lo = (int)(((long)inst * R) / BM), t_hi = min((int)((((long)inst + 1) * R - 1) / BM), tb + tiles_m - 1);
      const int tn_a = (g * cpg) / BN, ntn = ((g + 1) * cpg - 1) / BN - tn_a + 1;
      const int count = (t_hi - t_lo + 1) * ntn;
      auto src = [&](int u) {
        const int t = t_lo + u / ntn, tn = tn_a + u % ntn;
        const int sl = inst - (int)(((long)t * BM) / R);            // slot of this instance in tile t
        const int pp = g - (tn * BN) / cpg;                         // piece of this group in column tile tn
        return reinterpret_cast<const float*>(p.gn_part + ((((size_t)(t - tb) * 2 + sl) * tiles_n + tn) * T2V_GN_PIECES + pp) * 2);
      };
      constexpr int NREC = 4;                                       // records in flight per lane and round (register room: the tile is live)
      for (int u = sub; u < count; u += NREC * lpi) {
        f32x4 t[NREC];
#pragma unroll
        for (int j = 0; j < NREC; ++j) t[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int nrec = min(NREC, (count - u + lpi - 1) / lpi);
        t2v_rec_fetch<NREC>([&](int j) { return src(u + lpi * j); }, nrec, p.gn_want, p.gn_fault, t);
#pragma unroll
        for (int j = 0; j < NREC; ++j)
          if (j < nrec) t2v_rec_add(t[j], ds, dq);
      }
    }
    for (int o = 1; o < lpi; o <<= 1) { ds += __shfl_xor(ds, o); dq += __shfl_xor(dq, o); }      // (lpi is workgroup-uniform)
    if (active && sub == 0) {
      const float2 mr = t2v_mean_rstd(ds, dq, inv_n, p.gn_eps);
      stat[(slot * T2V_GN_PIECES + pc) * 2] = mr.x;
      stat[(slot * T2V_GN_PIECES + pc) * 2 + 1] = mr.y;
    }
  }
  __syncthreads();
  // ---- E
  const int bnv = n_hi - n0;
  for (int idx = tid; idx < 2 * bnv; idx += NT) {
    const int slot = idx / bnv, c = idx - slot * bnv, n = n0 + c;
    if (inst0 + slot > last_inst) continue;
    const int pc = n / cpg - g_lo;
    const float a = stat[(slot * T2V_GN_PIECES + pc) * 2 + 1] * p.gn_gb[n];
    scsf[(slot * 2) * BN + c] = a;
    scsf[(slot * 2 + 1) * BN + c] = p.gn_gb[p.N + n] - stat[(slot * T2V_GN_PIECES + pc) * 2] * a;
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int mt = m0 + (wm * TM + a) * 32;
    if (mt >= p.M) continue;                                       // wave-uniform
    const int slot = mt / R - inst0;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int cl = (wn * TN + b) * 32 + rcol, n = n0 + cl;
      if (n >= p.N) continue;
      const f32x4 sc = *reinterpret_cast<const f32x4*>(scsf + (slot * 2) * BN + cl);
      const f32x4 sf = *reinterpret_cast<const f32x4*>(scsf + (slot * 2 + 1) * BN + cl);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mt + rrow + 8 * i;
        if (m < p.M)
          t2v_norm_store<4>(p.gn_out + (size_t)m * p.ld_gn + n, p.gn_lo, f32x4{acc[a][b][4 * i], acc[a][b][4 * i + 1], acc[a][b][4 * i + 2], acc[a][b][4 * i + 3]},
                            sc, sf, p.gn_silu != 0);
      }
    }
  }
}
// ---- LayerNorm of a GEMM's result rows ACROSS the column tiles of the launch (round 5) ------------------------------------------------
// The fused LayerNorm second output of t2v_epilogue_rows_ln needs a tile that holds whole rows (N == 320).  At the 16x16 / 8x8 / 4x4
// levels (C = 640 / 1280) a row is cut into 5 - 20 column tiles and the norm was its own launch (read fp32, write fp16, ~10-12 us for
// <= 31 MB).  Same exchange as the GroupNorm epilogue above, along the other axis: every workgroup keeps its tile in registers, stores
// the fp32 stream, publishes {sum, sum of squares} per ROW of its column range, the launch meets at the grid barrier, every workgroup
// sums the tiles_n pairs of its rows in fp64 in tile order (bit-identical for every column tile of a row) and writes
// LayerNorm(row) * gamma + beta for its columns.  Scratch: fp64 records [tiles_m][tiles_n][BM][2] (p.gn_part).
template <int WM, int WN, int TM, int TN>
__device__ __forceinline__ void t2v_epilogue_rows_lnx(const GemmParams& p, f32x16 (&acc)[TM][TN], unsigned char* smem, int lane, int wave,
                                                      int m0, int n0, int tile_m, int tile_n, int tiles_n) {
  constexpr int NW = WM * WN, NT = NW * 64, S = WM * TM, BM = S * 32;
  static_assert(BM <= NT, "one thread per row");
  const int tid = threadIdx.x;
  const int wm = wave / WN, wn = wave % WN;
  float* stg = reinterpret_cast<float*>(smem) + wave * (32 * T2V_EPI_SP);
  float* rowsum = reinterpret_cast<float*>(smem) + NW * (32 * T2V_EPI_SP);       // [WN][BM][2]
  float* rowstat = rowsum + WN * BM * 2;                                         // [BM][mean | rstd]
  const int wrow = lane & 31, wcol = (lane >> 5) * 4;
  const int rrow = lane >> 3, rcol = (lane & 7) * 4;
  const bool tags = p.gn_seq != 0u;
  unsigned gen0 = 0;
  if (!tags && tid == 0) gen0 = t2v_grid_epoch(p.gn_bar);
  const bool has_res = p.res != nullptr;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int mt = m0 + (wm * TM + a) * 32;
    float rs[4] = {0.f, 0.f, 0.f, 0.f}, rq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int n = n0 + (wn * TN + b) * 32 + rcol;
      const bool ncol = n < p.N;
      f32x4 r[4];
      if (has_res) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = mt + rrow + 8 * i;
          const int mr = (p.res_wrap && m >= p.res_wrap) ? m - p.res_wrap : m;
          const float* src = (m < p.M && ncol) ? p.res + (size_t)mr * p.ldr + n : p.res;
          r[i] = t2v_ld_stream(src);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = {acc[a][b][4 * q], acc[a][b][4 * q + 1], acc[a][b][4 * q + 2], acc[a][b][4 * q + 3]};
        *reinterpret_cast<f32x4*>(stg + wrow * T2V_EPI_SP + 8 * q + wcol) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      f32x4 cb = {0.f, 0.f, 0.f, 0.f};
      if (p.bias && ncol) cb = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = rrow + 8 * i;
        f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * T2V_EPI_SP + rcol);
        const int m = mt + row;
        if (m < p.M && ncol) {
          v += cb;
          if (has_res) v += r[i];
        } else {
          v = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        acc[a][b][4 * i] = v[0]; acc[a][b][4 * i + 1] = v[1]; acc[a][b][4 * i + 2] = v[2]; acc[a][b][4 * i + 3] = v[3];   // row-major now
        rs[i] += (v[0] + v[1]) + (v[2] + v[3]);
        rq[i] += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    // 8 lanes share a row (xor 1, 2, 4); the WN column waves of the strip meet in LDS
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s1 = rs[i], s2 = rq[i];
      s1 += __shfl_xor(s1, 1); s2 += __shfl_xor(s2, 1);
      s1 += __shfl_xor(s1, 2); s2 += __shfl_xor(s2, 2);
      s1 += __shfl_xor(s1, 4); s2 += __shfl_xor(s2, 4);
      if ((lane & 7) == 0) {
        float* dst = rowsum + ((size_t)wn * BM + (wm * TM + a) * 32 + rrow + 8 * i) * 2;
        dst[0] = s1;
        dst[1] = s2;
      }
    }
  }
  __syncthreads();
  if (tid < BM) {                                                  // row tid of the tile: one 16-byte device-scope record {sum, sum of squares}
    double ds = 0.0, dq = 0.0;
#pragma unroll
    for (int w = 0; w < WN; ++w) { ds += (double)rowsum[((size_t)w * BM + tid) * 2]; dq += (double)rowsum[((size_t)w * BM + tid) * 2 + 1]; }
    t2v_st_dev(reinterpret_cast<float*>(p.gn_part + (((size_t)tile_m * tiles_n + tile_n) * BM + tid) * 2), t2v_rec_pack(ds, dq, p.gn_seq));
  }
  // (barrier mode: arrive;) then — under the exchange's latency — the fp32 stream goes out (from the registers, row-major)
  bool released = false;
  if (!tags) {
    t2v_wait_vm0();
    released = t2v_grid_arrive(p.gn_bar, gridDim.x);
  }
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int mt = m0 + (wm * TM + a) * 32;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int n = n0 + (wn * TN + b) * 32 + rcol;
      if (n >= p.N) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mt + rrow + 8 * i;
        if (m < p.M)
          t2v_st_stream(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n,
                        f32x4{acc[a][b][4 * i], acc[a][b][4 * i + 1], acc[a][b][4 * i + 2], acc[a][b][4 * i + 3]});
      }
    }
  }
  if (!tags) t2v_grid_wait(p.gn_bar, gen0, released, p.gn_fault);
  if (tid < BM) {
    double ds = 0.0, dq = 0.0;
    const double* base = p.gn_part + ((size_t)tile_m * tiles_n * BM + tid) * 2;
    for (int tn = 0; tn < tiles_n; tn += 8) {                      // EIGHT records in flight per round, summed in tile order
      f32x4 t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int nrec = min(8, tiles_n - tn);
      t2v_rec_fetch8([&](int j) { return reinterpret_cast<const float*>(base + (size_t)(tn + j) * BM * 2); }, nrec, p.gn_want, p.gn_fault, t);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nrec) t2v_rec_add(t[j], ds, dq);
    }
    const float2 mr = t2v_mean_rstd(ds, dq, 1.0 / (double)p.N, p.ln_eps);
    rowstat[tid * 2] = mr.x;
    rowstat[tid * 2 + 1] = mr.y;
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int mt = m0 + (wm * TM + a) * 32;
    if (mt >= p.M) continue;                                       // wave-uniform
    float mean[4], rstd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mean[i] = rowstat[((wm * TM + a) * 32 + rrow + 8 * i) * 2];
      rstd[i] = rowstat[((wm * TM + a) * 32 + rrow + 8 * i) * 2 + 1];
    }
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int n = n0 + (wn * TN + b) * 32 + rcol;
      if (n >= p.N) continue;
      const f32x4 g = *reinterpret_cast<const f32x4*>(p.ln_gb + n);
      const f32x4 be = *reinterpret_cast<const f32x4*>(p.ln_gb + p.N + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mt + rrow + 8 * i;
        if (m < p.M) {
          f16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (f16)((acc[a][b][4 * i + e] - mean[i]) * rstd[i] * g[e] + be[e]);
          *reinterpret_cast<f16x4*>(p.ln_out + (size_t)m * p.ld_ln + n) = o;
        }
      }
    }
  }
}
constexpr int t2v_lnx_epilogue_lds(int nw, int wn, int bm) { return nw * 32 * T2V_EPI_SP * 4 + (wn * bm * 2 + bm * 2) * 4; }

// ---- to_q projection + text cross-attention in ONE launch (T2V_EPI_XATTN, round 5; VERDICT r04 next #1b) --------------------------------
// Reference: CrossAttention of a BasicTransformerBlock's attn2 (t2v_model.py:540-584 called from :807): q = to_q(LayerNorm(x)), 77 text
// keys.  The text K / V projections are step-invariant (one GEMM per sampling run, the program's prologue), so after the to_q main loop a
// workgroup holds everything an attention over its rows needs: the accumulators go to LDS as fp16 Q [BM][BN] (BN = 64 * heads of the
// tile; re-using the operand ring), and every wave takes (32-row strip, head) items: S^T = K Q^T with the key on the MFMA row axis (<= 96
// keys = 3 blocks; K fragments straight from global memory — 10 KB per head, L2-resident), in-lane softmax, P from the accumulator
// registers, O^T = V^T P^T with V^T fragments from the transposed copy the prologue keeps ([N][lcp], keys contiguous).  Q never reaches
// HBM (one [M, C] fp16 round trip and one launch less per site).  Same fragment conventions as the fused temporal attention (gemm2.hip).
template <int WM, int WN, int TM, int TN>
__device__ __forceinline__ void t2v_epilogue_xattn(const GemmParams& p, const f32x16 (&acc)[TM][TN], unsigned char* smem, int lane, int wave,
                                                   int m0, int n0) {
  constexpr int NW = WM * WN, S = WM * TM, BN = WN * TN * 32, HEADS = BN / 64, PITCH = BN * 2 + 16;
  static_assert(BN % 64 == 0, "whole heads per column tile");
  const int wm = wave / WN, wn = wave % WN;
  const int frow = lane & 31, fhalf = lane >> 5;
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = (wm * TM + a) * 32 + frow, col = (wn * TN + b) * 32 + 8 * q + 4 * fhalf;
        const f16x4 v = {(f16)acc[a][b][4 * q], (f16)acc[a][b][4 * q + 1], (f16)acc[a][b][4 * q + 2], (f16)acc[a][b][4 * q + 3]};
        *reinterpret_cast<f16x4*>(smem + row * PITCH + col * 2) = v;
      }
  __syncthreads();
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int Lc = p.xa_lc;
  // 32-key blocks that hold a key (uniform over the launch).  The blocks behind them are not loaded: V^T has only ceil32(Lc) columns, so for
  // Lc <= 64 their fragments would come from the following V^T rows — past the end of the buffer for the last rows of the last sample — and
  // a NaN there survives its zero probability (0 x NaN).  Their scores stay 0 and are masked below: no part in the maximum or the sum.
  const int nkb = (Lc + 31) >> 5;
  for (int item = wave; item < S * HEADS; item += NW) {
    const int st = item / HEADS, hh = item - st * HEADS;
    const int mt = m0 + st * 32, h = n0 / 64 + hh;
    if (mt >= p.M || h * 64 >= p.N) continue;                      // wave-uniform
    const int smp = mt / p.rows_per_batch;
    const f16* K = p.xa_k + (size_t)smp * p.xa_k_sample + h * 64;
    const f16* VT = p.xa_vt + (size_t)smp * p.xa_vt_sample + (size_t)h * 64 * p.xa_lcp;
    const unsigned char* qrow = smem + (st * 32 + frow) * PITCH + hh * 128;
    f32x16 sc[3] = {zero16, zero16, zero16};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const f16x8 qf = *reinterpret_cast<const f16x8*>(qrow + ((kk * 2 + fhalf) << 4));
#pragma unroll
      for (int kb = 0; kb < 3; ++kb) {
        if (kb >= nkb) continue;
        const int key = min(kb * 32 + frow, Lc - 1);               // rows past the last key: a finite copy, masked below
        const f16x8 kf = *reinterpret_cast<const f16x8*>(K + (size_t)key * p.xa_ldk + (kk * 2 + fhalf) * 8);
        sc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf, sc[kb], 0, 0, 0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 3; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fhalf;
        if (key >= Lc) sc[kb][r] = -INFINITY;
        mx = fmaxf(mx, sc[kb][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float neg_m = -mx * p.attn_scale_log2;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 3; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kb][r], p.attn_scale_log2, neg_m));
        sc[kb][r] = pv;
        psum += pv;
      }
    psum += __shfl_xor(psum, 32);
    f32x16 oacc[2] = {zero16, zero16};
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const int kb = t >> 1, tt = t & 1;
      if (kb >= nkb) continue;
      f16x8 pf;
#pragma unroll
      for (int e = 0; e < 8; ++e) pf[e] = (f16)sc[kb][8 * tt + e];
      const int kofs = kb * 32 + tt * 16 + 4 * fhalf;
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const f16* vrow = VT + (size_t)(d * 32 + frow) * p.xa_lcp + kofs;
        const f16x4 lo = *reinterpret_cast<const f16x4*>(vrow);
        const f16x4 hi = *reinterpret_cast<const f16x4*>(vrow + 8);
        const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[d], 0, 0, 0);
      }
    }
    const int m = mt + frow;
    if (m < p.M) {
      const float inv = 1.0f / psum;
      f16* orow = reinterpret_cast<f16*>(p.out) + (size_t)m * p.ldc + h * 64;
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          f16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (f16)(oacc[d][4 * qd + r] * inv);
          *reinterpret_cast<f16x4*>(orow + d * 32 + 8 * qd + 4 * fhalf) = o;
        }
    }
  }
}
constexpr int t2v_xattn_epilogue_lds(int bm, int bn) { return bm * (bn * 2 + 16); }

// bytes of LDS the T2V_EPI_GN epilogue needs for a tile of NW waves, S 32-row strips, BN columns
constexpr int t2v_gn_epilogue_lds(int nw, int s, int bn) { return nw * 32 * T2V_EPI_SP * 4 + (s * 2 * bn + 4 * bn + 2 * T2V_GN_PIECES * 2) * 4; }

// exact-erf GELU (nn.GELU default, reference GEGLU t2v_model.py:817-821).  erfc(|z|) by Abramowitz-Stegun
// 7.1.26 (|abs err| < 1.5e-7, far below the fp16 output rounding); the negative side uses erfc directly, so
// the tail keeps its relative accuracy.  ~14 instructions, branch-free (the epilogue of the GEGLU GEMMs
// evaluates this 63 M times per UNet forward).
__device__ __forceinline__ float t2v_gelu_erf(float x) {
  const float z = x * 0.70710678118654752440f;
  const float az = __builtin_fabsf(z);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * az);
  float poly = 1.061405429f;
  poly = poly * t - 1.453152027f;
  poly = poly * t + 1.421413741f;
  poly = poly * t - 0.284496736f;
  poly = poly * t + 0.254829592f;
  const float e = poly * t * __builtin_amdgcn_exp2f(-az * az * 1.44269504088896340736f);   // erfc(|z|)
  return 0.5f * x * (z >= 0.f ? 2.0f - e : e);
}

// ---- communicators (comm.hip): RCCL is dlopen'ed on first use --------------------------------------------------
struct t2v_comm;
int t2v_comm_impl_unique_id(unsigned char id[128], std::string& err);
int t2v_comm_impl_create(const unsigned char id[128], int nranks, int rank, t2v_comm** out, std::string& err);
void t2v_comm_impl_destroy(t2v_comm* c);
int t2v_comm_impl_size(const t2v_comm* c);
int t2v_comm_impl_window_create(t2v_comm* c, size_t slot_bytes, unsigned char handle_out[64], std::string& err);
int t2v_comm_impl_window_open(t2v_comm* c, const unsigned char* handles, std::string& err);
void t2v_comm_impl_counters(const t2v_comm* c, unsigned long long out[2]);
const char* t2v_comm_impl_window_kind(const t2v_comm* c);
int t2v_comm_allgather(t2v_comm* c, void* base, size_t bytes, int nparts, int part, hipStream_t s, std::string& err);
int t2v_comm_impl_all_gather(t2v_comm* c, void* base, size_t bytes, hipStream_t s, std::string& err);
int t2v_comm_halo(t2v_comm* c, void* base, size_t frame_bytes, int F, int prev, int next, hipStream_t s, std::string& err);
int t2v_comm_stats_halo(t2v_comm* c, void* parts, size_t part_bytes, int nparts, int part, void* raw, size_t frame_bytes, int F,
                        int prev, int next, hipStream_t s, std::string& err);
int t2v_comm_alltoall(t2v_comm* c, void* send, void* recv, size_t chunk, int nparts, int part, int base_cnt, int last_cnt, int dir,
                      hipStream_t s, std::string& err);
