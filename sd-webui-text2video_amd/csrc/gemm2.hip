// Second-generation implicit-GEMM kernel (large tiles, deep LDS-DMA ring) for gfx950.
//
// Same contract as gemm.hip (out[M,N] = epilogue(gather(A)[M,K] · W[N,K]^T), fp16 operands,
// fp32 accumulate, swapped MFMA operands so a lane owns 4 consecutive output channels), but
// built for the regime the UNet lives in: a 128x128 tile needs ~64 B/clk/CU of operand
// traffic at MFMA peak — above what one CU gets from L2 — so tiles here are 256x256,
// 256x320, 128x256 and 128x320 (29-45 B/clk/CU).  N = 320*k (every C-output GEMM of the
// ModelScope UNet: 320, 640, 960, 1280, 1920, 2560 ...) uses the 320-wide tile with no padded
// columns.
//
// Pipeline: k-tiles of 32 (64-byte LDS rows), STAGES-deep ring filled by `global_load_lds`
// 16-byte LDS-DMA; STAGES-1 k-tiles are always in flight.  Per k-tile each wave executes
//     s_waitcnt vmcnt(LPS*(STAGES-2))   -> its own DMA pieces of the tile to compute have landed
//     s_barrier                          -> everyone's have; everyone finished the previous tile
//     issue the DMA of tile t+STAGES-1 into the slot just freed
//     ds_read_b128 fragments + MFMA 32x32x16
// i.e. ONE barrier per k-tile and no vmcnt(0) drain anywhere in the main loop (the loads of
// k-tiles past the end are redirected to a zero page so the outstanding-load count is constant).
// LDS image: row r, 16-byte chunk c at r*64 + ((c ^ ((r>>2)&3))<<4): conflict-free for the
// fragment reads; the XOR is applied to the per-lane DMA *source* (the destination is
// lane-linear) and again on the read.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "t2v_kernels.h"

namespace {

__device__ __attribute__((aligned(256))) unsigned char g2_zero_page[256];

// internal gather id: 3x3 conv with the nearest-2x upsample folded in (no affine tap offset)
constexpr int G_CONV_UP = 100;

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// WM x WN waves; each wave owns TM x TN MFMA tiles (32 tokens x 32 channels each).
// XE: extra epilogue of the plain (T2V_EPI_NONE) path, one of T2V_XE_* (t2v_kernels.h); separate instantiations, so the plain kernels
// keep their register budgets.
template <int WM, int WN, int TM, int TN, int BK, int STAGES, int MINW, int GATHER, int XE = T2V_XE_NONE, bool TAT = false>
__global__ __launch_bounds__(WM * WN * 64, MINW) void gemm2_kernel(const GemmParams p) {
  constexpr int NW = WM * WN;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int ROW_BYTES = BK * 2;                          // 64 (BK=32) or 128 (BK=64) bytes per LDS row
  constexpr int RPS = 1024 / ROW_BYTES;                      // rows per 1-KiB DMA piece: 16 or 8
  constexpr int CPR = BK / 8;                                // 16-byte chunks per row: 4 or 8
  constexpr int XSLABS = BM / RPS, WSLABS = BN / RPS;        // 1-KiB DMA pieces per tile
  static_assert(XSLABS % NW == 0, "token slabs must divide evenly over the waves");
  constexpr int XPW = XSLABS / NW;
  constexpr int WPW = (WSLABS + NW - 1) / NW;                // the last may be a dummy piece
  constexpr int LPS = XPW + WPW;                             // DMA instructions per wave per stage
  constexpr int STAGE_BYTES = (XSLABS + WSLABS) * 1024;
  constexpr int DUMMY_OFF = STAGES * STAGE_BYTES;            // 1 KiB scratch for dummy pieces
  static_assert(LPS * (STAGES - 1) < 64, "vmcnt is a 6-bit counter");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  // ---- XCD-aware tile order (t2v_kernels.h): each XCD walks one contiguous run of the panel numbering
  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles_m = (p.M - p.m_begin + BM - 1) / BM;        // (m_begin: row chunk of a fused-norm launch, t2v_launch_coresident; else 0)
  int tile_m, tile_n;
  t2v_tile_of_block(blockIdx.x, tiles_m, tiles_n, p.panel, tile_m, tile_n);
  const int m0 = p.m_begin + tile_m * BM, n0 = tile_n * BN;

  const int KT = (p.K + BK - 1) / BK;
  const int kt_begin = blockIdx.y * p.kt_per_split;          // in units of BK-wide k-tiles
  const int kt_end = min(KT, kt_begin + p.kt_per_split);
  const int nkt = kt_end - kt_begin;

  const unsigned char* zero = g2_zero_page;

  // ---- per-lane DMA state -------------------------------------------------------------------
  // Every lane keeps ONE running source pointer per DMA piece; a k-tile costs one 64-bit add per
  // piece.  Conv gathers recompute the pointers only when the filter tap changes (9 / 3 times per
  // workgroup); rows that fall into padding, past M / N, or belong to a dummy piece park on the
  // zero page with step 0.  (K % BK == 0 is guaranteed by the dispatcher.)
  const int lrow = lane / CPR;     // row inside a 1-KiB piece
  const int pchunk = lane % CPR;   // physical 16-B chunk inside the row
  auto swz = [](int r) { return BK == 64 ? ((r >> 1) & 7) : ((r >> 2) & 3); };
  constexpr int STEP = BK * 2;     // bytes per k-tile along a row

  constexpr int TAPS = (GATHER == T2V_GATHER_CONV3X3 || GATHER == G_CONV_UP) ? 9 : (GATHER == T2V_GATHER_TCONV3 ? 3 : 1);
  constexpr bool general = GATHER == G_CONV_UP;
  const unsigned char* xptr[XPW];  // PLAIN: running pointer; conv: pointer of the CENTRE tap, chunk 0
  int xstep[XPW];                  // PLAIN only
  unsigned xmask[XPW];             // conv: bit t set <=> tap t of this row is inside the image / clip
  long xoff[general ? XPW : 1];    // only the upsample path keeps per-row coordinates
  int xy[general ? XPW : 1], xx[general ? XPW : 1];
  // first tile row of DMA piece j of this wave: the pieces are interleaved over the tile, piece s = wave + j * NW
  auto xrow0 = [&](int j) { return (wave + j * NW) * RPS; };
  auto wrow0 = [&](int j) { return (wave + j * NW) * RPS; };
#pragma unroll
  for (int j = 0; j < XPW; ++j) {
    const int r = xrow0(j) + lrow;                // row inside the token tile
    const int m = m0 + r;
    const int lc = pchunk ^ swz(r);
    const bool valid = m < p.M;
    xmask[j] = 0; xstep[j] = 0;
    xptr[j] = zero;
    if (GATHER == T2V_GATHER_PLAIN) {
      if constexpr (TAT) {
        // fused QKV + temporal attention: the tile's rows are p.tpix pixels x p.F frames of ONE sample (row r = pixel r / F,
        // frame r % F), so that every sequence (the frames of a pixel) is complete inside the workgroup
        const int pl = r / p.F, f = r - pl * p.F;
        const int smp = tile_m / p.tiles_ps, pix = (tile_m - smp * p.tiles_ps) * p.tpix + pl;
        if (pl < p.tpix && pix < p.HW) {
          const long mm = ((long)smp * p.F + f) * p.HW + pix;
          xptr[j] = reinterpret_cast<const unsigned char*>(p.A + mm * p.lda + (long)kt_begin * BK + lc * 8);
          xstep[j] = STEP;
        }
      } else if (valid) {
        const int ma = (p.a_wrap && m >= p.a_wrap) ? m - p.a_wrap : m;     // shared (one-sample) operand: rows wrap once
        xptr[j] = reinterpret_cast<const unsigned char*>(p.A + (long)ma * p.lda + (long)kt_begin * BK + lc * 8);
        xstep[j] = STEP;
      }
    } else if (GATHER == T2V_GATHER_CONV3X3 || GATHER == G_CONV_UP) {
      const int hw = p.Hout * p.Wout;
      const int img = m / hw, rem = m - img * hw;
      const int yo = rem / p.Wout, xo = rem - yo * p.Wout;
      const long ibase = (long)img * p.Hin * p.Win;
      const int ys = yo * p.stride, xs = xo * p.stride;
      xptr[j] = reinterpret_cast<const unsigned char*>(p.A + (ibase + (long)ys * p.Win + xs) * p.lda + lc * 8);
      const int pl = p.halo ? 0 : 1;     // conv3x3: halo = 1 -> taps at +0..+2 (LDM encoder Downsample pads only bottom / right)
      for (int t = 0; t < 9; ++t) {
        const int yv = ys + t / 3 - pl, xv = xs + t % 3 - pl;
        if (valid && yv >= 0 && yv < (p.Hin << p.up) && xv >= 0 && xv < (p.Win << p.up)) xmask[j] |= 1u << t;
      }
      if (general) {
        xoff[j] = ibase;
        xy[j] = ys;
        xx[j] = xs | (lc << 24);     // keep the chunk too (coordinates are < 2^24)
      }
    } else {  // TCONV3
      const int clip = m / (p.HW * p.F);
      const int f = (m / p.HW) - clip * p.F;
      // halo layout: input rows are [clip][F+2][HW]; output row m reads input frames f, f+1, f+2
      const long in_row = p.halo ? (long)m + (long)(2 * clip + 1) * p.HW : (long)m;
      xptr[j] = reinterpret_cast<const unsigned char*>(p.A + in_row * p.lda + lc * 8);
      for (int t = 0; t < 3; ++t)
        if (valid && (p.halo || (f + t - 1 >= 0 && f + t - 1 < p.F))) xmask[j] |= 1u << t;
    }
  }
  int tap = 0, chunk = 0;          // wave-uniform position of the NEXT k-tile to be staged
  if (GATHER != T2V_GATHER_PLAIN) {
    chunk = kt_begin / TAPS;
    tap = kt_begin - chunk * TAPS;
  }
  const unsigned char* wptr[WPW];
  int wstep[WPW];
  bool wdummy[WPW];
#pragma unroll
  for (int j = 0; j < WPW; ++j) {
    const int r = wrow0(j) + lrow;               // row inside the weight tile
    const int n = n0 + r;
    wdummy[j] = wrow0(j) >= BN;                  // wave-uniform
    const bool ok = !wdummy[j] && n < p.N;
    wptr[j] = ok ? reinterpret_cast<const unsigned char*>(p.W + (size_t)n * p.ldw + kt_begin * BK + (pchunk ^ swz(r)) * 8) : zero;
    wstep[j] = ok ? STEP : 0;
  }

  // Staging one k-tile = LPS DMA instructions per wave.  They are issued as `pieces` so that the
  // main loop can spread them between the MFMA k-steps: an LDS-DMA instruction holds the wave's
  // issue port for ~60+ cycles while the TA walks its 64 addresses, so issuing all of them
  // back-to-back before the MFMAs (as a monolithic stage() would) serialises DMA issue and MFMA
  // execution — measured: 27 GB/s/CU of operand delivery, 50 % of wave cycles parked.
  int staged = 0;                  // k-tiles whose staging has been started (wave-uniform)
  bool live = true;                // staging position still inside [kt_begin, kt_end)
  long boff = 0;                   // conv: wave-uniform byte offset of the k-tile being staged
  int ktap = 0;
  auto stage_begin = [&]() {
    live = staged < nkt;
    if (GATHER != T2V_GATHER_PLAIN) {
      ktap = tap;
      long delta = 0;
      if (GATHER == T2V_GATHER_CONV3X3) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const int pl = p.halo ? 0 : 1;
        delta = ((long)(ky - pl) * p.Win + (kx - pl)) * p.lda;
      } else if (GATHER == T2V_GATHER_TCONV3) {
        delta = (long)(tap - 1) * p.HW * p.lda;
      }
      boff = (delta + (long)chunk * BK) * 2;
    }
  };
  // source of piece j of the k-tile being staged (per-lane pointer; advances the running pointers) and its 1-KiB LDS destination
  auto piece_src = [&](int j) -> const void* {     // j in [0, LPS): token pieces first, then weights
    const void* src = zero;
    if (j < XPW) {
      if (GATHER == T2V_GATHER_PLAIN) {
        if (live) { src = xptr[j]; xptr[j] += xstep[j]; }
      } else if (!general) {
        if (live && ((xmask[j] >> ktap) & 1u)) src = xptr[j] + boff;
      } else if (general) {
        // nearest-2x upsample folded into the gather (3 convs per forward): per-lane recompute
        const int ky = ktap / 3, kx = ktap - ky * 3;
        const int lc = xx[j] >> 24, x0 = xx[j] & 0xFFFFFF;
        const int yv = xy[j] + ky - 1, xv = x0 + kx - 1;      // (upsample path: symmetric padding only)
        const long row = xoff[j] + (long)(yv >> 1) * p.Win + (xv >> 1);
        if (live && ((xmask[j] >> ktap) & 1u)) src = p.A + row * p.lda + (long)chunk * BK + lc * 8;
      }
    } else {
      const int jw = j - XPW;
      if (live) { src = wptr[jw]; wptr[jw] += wstep[jw]; }
    }
    return src;
  };
  auto piece_dst = [&](int slot, int j) -> unsigned char* {
    unsigned char* base = smem + slot * STAGE_BYTES;
    if (j < XPW) return base + (xrow0(j) / RPS) * 1024;
    const int jw = j - XPW;
    return wdummy[jw] ? (smem + DUMMY_OFF) : (base + (XSLABS + wrow0(jw) / RPS) * 1024);
  };
  auto stage_piece = [&](int slot, int j) {
    const void* src = piece_src(j);
    t2v_glds16(src, piece_dst(slot, j));
  };
  auto stage_end = [&]() {
    if (GATHER != T2V_GATHER_PLAIN && live) {
      if (++tap == TAPS) { tap = 0; ++chunk; }
    }
    ++staged;
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // prologue: STAGES-1 k-tiles in flight
#pragma unroll
  for (int g = 0; g < STAGES - 1; ++g) {
    stage_begin();
#pragma unroll
    for (int j = 0; j < LPS; ++j) stage_piece(g, j);
    stage_end();
  }

  // fragment read addressing: lane reads row (tile_row0 + lane&31), logical chunk kk*2 + (lane>>5);
  // per tile-row keep the byte base and the swizzle term, one xor-add per read
  const int frow = lane & 31, fhalf = lane >> 5;
  int xbase[TM], xsw[TM], wbase[TN], wsw[TN];
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int r = (wm * TM + a) * 32 + frow;
    xbase[a] = r * ROW_BYTES;
    xsw[a] = swz(r) << 4;
  }
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int r = (wn * TN + b) * 32 + frow;
    wbase[b] = XSLABS * 1024 + r * ROW_BYTES;
    wsw[b] = swz(r) << 4;
  }

  // Main loop: ONE schedule, lock-step — every wave waits for its own pieces, meets the barrier, then interleaves the next tile's DMA with
  // this tile's fragment reads and MFMAs.  Four other schedules were built, parity-tested, measured against it and not selected:
  //   round 1: two wave groups one barrier apart, the next k-tile's DMA drained with vmcnt(0) (tiles 6 / 7)                     = lock-step +-3 %
  //   round 5: the next k-tile's first fragments prefetched across the barrier (tiles 13-17)                                       -1.5 .. +3.7 %
  //   round 5: operands staged through registers instead of LDS-DMA (tiles 18-21)                                                    +4 % / -1 .. -11 %
  //   round 6: two staggered groups, region-granular staging two k-tiles ahead, counted vmcnt only (tiles 22-24)                    +-3 % long K, -7 .. -20 % short K
  // Why none of them moves the number: profiles/r05_gemm_mainloop_findings.txt and profiles/r06_gemm_mainloop_findings.txt (the loop
  // runs the same cycles at ~62 % MFMA busy under every schedule; on random operands the chip clocks 1.55-1.68 GHz against 2.3 GHz on
  // zeros — the ceiling is power).  Their code (this file's experiments .inc and the build switches around this loop) last existed
  // in commit d7cc668.
  constexpr int KSTEPS = BK / 16;
  int slot = 0;
  for (int t = 0; t < nkt; ++t) {
    wait_vmcnt<LPS*(STAGES - 2)>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int fs = slot + STAGES - 1;
    if (fs >= STAGES) fs -= STAGES;
    stage_begin();
    const unsigned char* st = smem + slot * STAGE_BYTES;
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
      const int lc4 = (kk * 2 + fhalf) << 4;
      f16x8 xf[TM], wf[TN];
#pragma unroll
      for (int a = 0; a < TM; ++a) xf[a] = *reinterpret_cast<const f16x8*>(st + xbase[a] + (lc4 ^ xsw[a]));
#pragma unroll
      for (int b = 0; b < TN; ++b) wf[b] = *reinterpret_cast<const f16x8*>(st + wbase[b] + (lc4 ^ wsw[b]));
      // this k-step's share of the next tile's DMA, issued between the fragment reads and the MFMAs.
      // With a 2-deep ring the pieces must land before the next barrier, so they go out in the first
      // half of the k-tile; with 3 stages they have a whole extra k-tile and are spread over all steps.
      constexpr int SPREAD = STAGES == 2 ? KSTEPS / 2 : KSTEPS;
      if (kk < SPREAD) {
#pragma unroll
        for (int j = (LPS * kk) / SPREAD; j < (LPS * (kk + 1)) / SPREAD; ++j) stage_piece(fs, j);
      }
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[b], xf[a], acc[a][b], 0, 0, 0);
    }
    stage_end();
    slot = slot + 1 == STAGES ? 0 : slot + 1;
  }
  wait_vmcnt<0>();   // drain the zero-page loads of the dead stages before the LDS goes away

  // ---- epilogue ---------------------------------------------------------------------------------
  // Invariant (enforced on the host, launch_cfg): in here p.epi is T2V_EPI_NONE or T2V_EPI_GEGLU — or T2V_EPI_TATTN, in the TAT
  // instantiation only.  Everything else the executor has folded into NONE plus the pointers of the XE epilogues.
  if constexpr (TAT) {
    // Fused temporal self-attention (t2v_model.py:716-767 with CrossAttention :540-584): this tile holds q | k | v (64 channels
    // each: ONE head, the weight rows are packed head-major) of all F frames of p.tpix pixels.  The accumulators go to LDS as
    // fp16 (q | k row-major, V transposed: [pixel][d][frame slot]), then one wave per pixel runs the 32-key attention tile of
    // attention.hip (S^T = K Q^T with the key on the MFMA row axis, in-lane softmax, P from the accumulator registers) and
    // writes O for its F frames.  Q, K, V never reach HBM: 3 x the tensor written + read per attention before.
    static_assert(TM == 1 && TN == 3 && WM == 6 && WN == 2, "the fused attention epilogue is written for the 192x192 tile");
    constexpr int QK_PITCH = 272;                          // bytes per row: q (128 B) | k (128 B) + 16
    constexpr int VT_PITCH = 72;                           // bytes per V^T row: 32 frame slots x 2 B + 8
    __syncthreads();                                       // every wave is done reading the operand stages
    unsigned char* qk = smem;
    unsigned char* vt = smem + BM * QK_PITCH;
    const int F = p.F;
    {
      const int wrow = wm * 32 + (lane & 31);              // tile row of this lane's accumulator column
      const int pl = wrow / F, f = wrow - pl * F;
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = wn * (TN * 32) + b * 32 + 8 * q + 4 * (lane >> 5);
          const f16x4 v = {(f16)acc[0][b][4 * q], (f16)acc[0][b][4 * q + 1], (f16)acc[0][b][4 * q + 2], (f16)acc[0][b][4 * q + 3]};
          if (col < 128) {
            *reinterpret_cast<f16x4*>(qk + wrow * QK_PITCH + col * 2) = v;
          } else if (pl < p.tpix) {
            const int d = col - 128;
#pragma unroll
            for (int e = 0; e < 4; ++e) *reinterpret_cast<f16*>(vt + (pl * 64 + d + e) * VT_PITCH + f * 2) = v[e];
          }
        }
      // frame slots F .. 31 of V^T: zero (they meet probabilities that are exactly 0, but must not hold NaN patterns)
      for (int u = tid; u < p.tpix * 64; u += NW * 64)
        for (int k = F; k < 32; ++k) *reinterpret_cast<f16*>(vt + u * VT_PITCH + k * 2) = (f16)0.f;
    }
    __syncthreads();
    const int frow = lane & 31, fhalf = lane >> 5;
    const int smp = tile_m / p.tiles_ps;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int pl = wave; pl < p.tpix; pl += NW) {
      const int pix = (tile_m - smp * p.tiles_ps) * p.tpix + pl;
      if (pix >= p.HW) continue;                           // wave-uniform
      const unsigned char* rowp = qk + (pl * F + frow) * QK_PITCH;    // rows >= F of the pixel: next pixel / V^T bytes, finite, masked below
      f32x16 sc = zero16;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const f16x8 qf = *reinterpret_cast<const f16x8*>(rowp + ((kk * 2 + fhalf) << 4));
        const f16x8 kf = *reinterpret_cast<const f16x8*>(rowp + 128 + ((kk * 2 + fhalf) << 4));
        sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf, sc, 0, 0, 0);
      }
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = (r & 3) + 8 * (r >> 2) + 4 * fhalf;
        if (key >= F) sc[r] = -INFINITY;
        mx = fmaxf(mx, sc[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      if (frow >= F) mx = 0.f;                             // padded queries: any finite reference, the result is dropped
      const float neg_m = -mx * p.attn_scale_log2;
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[r], p.attn_scale_log2, neg_m));
        sc[r] = pv;
        psum += pv;
      }
      psum += __shfl_xor(psum, 32);
      f32x16 oacc[2] = {zero16, zero16};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f16x8 pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) pf[e] = (f16)sc[8 * t + e];
        const int kofs = (t * 16 + 4 * fhalf) * 2;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const unsigned char* vrow = vt + (pl * 64 + d * 32 + frow) * VT_PITCH + kofs;
          const f16x4 lo = *reinterpret_cast<const f16x4*>(vrow);
          const f16x4 hi = *reinterpret_cast<const f16x4*>(vrow + 16);
          const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[d], 0, 0, 0);
        }
      }
      if (frow < F) {
        const float inv = 1.0f / psum;
        f16* orow = reinterpret_cast<f16*>(p.out) + (((long)smp * F + frow) * p.HW + pix) * p.ldc + tile_n * 64;
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
    return;
  }
  if (p.epi == T2V_EPI_NONE) {      // row-coalesced through a per-wave LDS buffer (t2v_kernels.h); also the split-K slabs
    __builtin_amdgcn_s_barrier();   // every wave is done reading the operand stages
    if constexpr (XE == T2V_XE_GN) {        // GroupNorm (+SiLU) of the result inside the epilogue: statistics meet at a grid barrier (t2v_kernels.h)
      t2v_epilogue_rows_gn<WM, WN, TM, TN>(p, acc, smem, lane, wave, m0, n0, tile_m, tile_n, tiles_m, tiles_n);
      return;
    }
    if constexpr (XE == T2V_XE_XATTN) {        // to_q projection + text cross-attention: the accumulators are Q (T2V_EPI_XATTN, t2v_kernels.h)
      t2v_epilogue_xattn<WM, WN, TM, TN>(p, acc, smem, lane, wave, m0, n0);
      return;
    }
    if constexpr (XE == T2V_XE_LNX) {        // LayerNorm second output across the column tiles of the launch (partial row sums meet at the grid barrier)
      t2v_epilogue_rows_lnx<WM, WN, TM, TN>(p, acc, smem, lane, wave, m0, n0, tile_m, tile_n, tiles_n);
      return;
    }
    if constexpr (XE == T2V_XE_LN) {        // whole rows in this tile (N == its columns, validated by the executor): fused LayerNorm output
      float* fs = reinterpret_cast<float*>(smem);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {            // (TM == 2: the 256x320 tile, round 6 — a wave's two 32-row blocks one after the other)
        if (tm > 0) __syncthreads();                // the partner wave has read this wave's row sums of the previous block
        t2v_epilogue_rows_ln<TN>(p, reinterpret_cast<f32x16 (&)[1][TN]>(acc[tm]), fs + wave * (32 * T2V_EPI_SP), fs + NW * (32 * T2V_EPI_SP), lane, wave,
                                 m0 + (wm * TM + tm) * 32, n0 + wn * TN * 32);
      }
      return;
    }
    t2v_epilogue_rows<TM, TN>(p, acc, reinterpret_cast<float*>(smem) + wave * (32 * T2V_EPI_SP), lane, m0 + wm * TM * 32,
                              n0 + wn * TN * 32, blockIdx.y, tile_m * tiles_n + tile_n);
    return;
  }
  const int mlane = lane & 31, nhalf = (lane >> 5) * 4;
  if (p.epi == T2V_EPI_GEGLU && p.splitk == 1) {
    // GEGLU through a per-wave LDS strip: a lane's (value + bias) * gelu(gate + bias) results are 4 channels of ONE row
    // (8-byte stores scattered over 32 rows); staged as [32 rows][TN * 16 channels] they leave as whole 16-byte chunks of
    // TN * 32-byte row segments (6 rows per store instruction at TN = 5).  Same-box A/B: the 32x32-level GEGLU GEMM
    // 153 -> 142 us, the 16x16-level one 116 -> 111 us.
    constexpr int PITCH = TN * 32 + 16;                   // bytes per staged row (+16: rows start on different banks)
    constexpr int CPRW = TN * 2;                          // 16-byte chunks per row
    __builtin_amdgcn_s_barrier();                         // every wave is done reading the operand stages
    unsigned char* strip = smem + wave * (32 * PITCH);
    const int nw = n0 + wn * TN * 32;                     // first packed column of this wave
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      const int mt = m0 + (wm * TM + a) * 32;
      if (mt >= p.M) continue;                            // wave-uniform
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        const int nt = nw + b * 32;
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
          const int n_val = nt + 16 * qq + nhalf;
          f16x4 o = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
          if (n_val < p.N) {
            float bv[4] = {0, 0, 0, 0}, bg[4] = {0, 0, 0, 0};
            if (p.bias) {
              const f32x4 ba = *reinterpret_cast<const f32x4*>(p.bias + n_val);
              const f32x4 bb = *reinterpret_cast<const f32x4*>(p.bias + n_val + 8);
#pragma unroll
              for (int r = 0; r < 4; ++r) { bv[r] = ba[r]; bg[r] = bb[r]; }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (f16)((acc[a][b][8 * qq + r] + bv[r]) * t2v_gelu_erf(acc[a][b][8 * qq + 4 + r] + bg[r]));
          }
          *reinterpret_cast<f16x4*>(strip + mlane * PITCH + (b * 16 + 8 * qq + nhalf) * 2) = o;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      const int c_out0 = nw >> 1;                         // first output channel of the strip
#pragma unroll
      for (int u = lane; u < 32 * CPRW; u += 64) {
        const int row = u / CPRW, ch = u - row * CPRW;
        const int m = mt + row, c = c_out0 + ch * 8;
        if (m < p.M && c < (p.N >> 1)) {
          const f16x8 v = *reinterpret_cast<const f16x8*>(strip + row * PITCH + ch * 16);
          *reinterpret_cast<f16x8*>(reinterpret_cast<f16*>(p.out) + (size_t)m * p.ldc + c) = v;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    return;
  }
  // GEGLU with split-K: the slab of this split; value * gelu(gate) runs in splitk_reduce_kernel (gemm.hip)
  t2v_store_splitk_slab<TM, TN>(p, acc, lane, m0 + wm * TM * 32, n0 + wn * TN * 32, blockIdx.y);
}

// ---- 3x3 convolution, "halo" A staging --------------------------------------------------------------------------------------------------
// K is ordered (64-channel chunk, tap, channel): the nine k-tiles of one chunk read the SAME activation rows shifted by at most
// +-(Win + 1) rows, and gemm2_kernel stages each of the nine with its own DMA pieces (padding taps from the zero page).  Here the
// distinct rows of a chunk — the tile's BM rows and a fixed pad of 40 >= Win + 1 rows on either side — are staged ONCE per chunk:
//   LDS    two halo buffers (double-buffered by chunk) of BM + 80 rows x 128 B: LDS row h = flattened token row m0 - 40 + h, channels
//          [64 c, 64 c + 64), swizzled by h as gemm2_kernel's rows are by r; rows outside the input repeat its first / last row.  The weight
//          ring keeps its STAGES slots of BN x 128 B.  Behind them the 1-KiB dummy piece and one 128-byte row of zeros.
//   reads  tap (ky, kx) of tile row r reads LDS row r + 40 + (ky - 1) Win + (kx - 1).  Padding: a lane keeps the 9-bit tap mask of each
//          32-row block it reads (the predicate of gemm2_kernel's xmask, for the fragment row) and reads the row of zeros where the bit is
//          clear — rows of a neighbouring image (or garbage past the input) are only ever reached by masked taps.
//   order  the k order, and so every accumulator and every epilogue, is gemm2_kernel's: the results are bit-identical.
// Schedule: the nine taps of a chunk are unrolled; at tap T a wave issues the WPW weight pieces of k-tile t + STAGES - 1 (as gemm2_kernel)
// and halo_geom::count(T) pieces of the NEXT chunk's halo, which are spread over the first 11 - STAGES taps: loads retire in order, so the
// counted wait of tap 0 of chunk c + 1 (everything but the pieces of the last STAGES - 2 iterations has landed) covers the whole halo of
// chunk c + 1, the barrier behind it covers every wave's, and the buffer is re-staged only behind the barrier of tap 0 of chunk c + 2,
// which every wave reaches after its last read of chunk c + 1.  Every wave issues the same number of pieces at a given tap (a piece
// that does not exist goes from the zero page to the dummy KiB), so each s_waitcnt keeps an immediate.
template <int NW, int BM, int BN, int STAGES>
struct halo_geom {
  static constexpr int PAD = 40;
  static constexpr int HROWS = BM + 2 * PAD, HSLABS = HROWS / 8, HPW = (HSLABS + NW - 1) / NW, HBYTES = HROWS * 128;
  static constexpr int WSLABS = BN / 8, WPW = (WSLABS + NW - 1) / NW, WSLOT = BN * 128;
  static constexpr int W_OFF = 2 * HBYTES, DUMMY_OFF = W_OFF + STAGES * WSLOT, ZERO_OFF = DUMMY_OFF + 1024, LDS = ZERO_OFF + 128;
  static constexpr int HTAPS = 11 - STAGES;                    // taps of chunk c at which pieces of chunk c + 1's halo go out
  static constexpr int tap_of(int i) { return (i * HTAPS) / HPW; }
  static constexpr int count(int tap) { int n = 0; for (int i = 0; i < HPW; ++i) n += tap_of(i) == tap; return n; }
  static constexpr int first(int tap) { int n = 0; for (int i = 0; i < HPW; ++i) n += tap_of(i) < tap; return n; }
  // pieces a wave may have outstanding at the wait of `tap`: those of the previous STAGES - 2 iterations
  static constexpr int wait_at(int tap) { int n = 0; for (int d = 1; d <= STAGES - 2; ++d) n += WPW + count((tap + 9 - d) % 9); return n; }
  static_assert(STAGES >= 2 && STAGES <= 4 && HROWS % 8 == 0 && tap_of(HPW - 1) < HTAPS, "halo schedule");
  static_assert(HPW + (STAGES - 1) * WPW + WPW + HPW < 64, "vmcnt is a 6-bit counter");
  static_assert(LDS <= 160 * 1024, "LDS");
};

template <int WM, int WN, int TM, int TN, int STAGES, int MINW, int XE = T2V_XE_NONE>
__global__ __launch_bounds__(WM * WN * 64, MINW) void gemm2_halo_kernel(const GemmParams p) {
  constexpr int NW = WM * WN;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  using HG = halo_geom<NW, BM, BN, STAGES>;
  constexpr int HPW = HG::HPW, WPW = HG::WPW;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles_m = (p.M - p.m_begin + BM - 1) / BM;
  int tile_m, tile_n;
  t2v_tile_of_block(blockIdx.x, tiles_m, tiles_n, p.panel, tile_m, tile_n);
  const int m0 = p.m_begin + tile_m * BM, n0 = tile_n * BN;

  // (the launcher has checked: K = 9 Cin, Cin % 64 == 0, and a split starts on a chunk boundary — nkt is a multiple of 9)
  const int KT = p.K / 64;
  const int kt_begin = blockIdx.y * p.kt_per_split;
  const int nkt = min(KT, kt_begin + p.kt_per_split) - kt_begin;
  const int nch = nkt / 9;

  const unsigned char* zero = g2_zero_page;
  if (tid < 32) reinterpret_cast<int*>(smem + HG::ZERO_OFF)[tid] = 0;      // (visible behind the first barrier of the main loop)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- per-lane DMA state
  const int lrow = lane >> 3, pchunk = lane & 7;
  auto swz = [](int r) { return (r >> 1) & 7; };
  const int hw = p.Hin * p.Win;
  const long a_rows = (long)((p.M + hw - 1) / hw) * hw;        // whole images: the rows a live tap of a row < M can reach
  // halo pieces: a 32-bit lane offset per piece from the wave-uniform base of the chunk (the DMA address stays scalar base + lane
  // offset).  Rows outside the input — and the rows of a piece that does not exist — read the nearest input row instead: finite or not,
  // only masked taps ever reach them.
  unsigned hoff[HPW];
#pragma unroll
  for (int i = 0; i < HPW; ++i) {
    const int h = (wave + i * NW) * 8 + lrow;                  // piece wave + i NW = rows h .. of the halo buffer, a lane's row
    const long g = min(max((long)m0 - HG::PAD + h, 0L), a_rows - 1);
    hoff[i] = (unsigned)(g * p.lda * 2) + (unsigned)((pchunk ^ swz(h)) * 16);
  }
  // wave-uniform base of the chunk whose halo is staged next (past the split's end: the last chunk again, into a buffer nobody reads)
  const unsigned char* hnext = reinterpret_cast<const unsigned char*>(p.A) + (long)(kt_begin / 9) * 128;
  // weight pieces: one running pointer per piece, advanced by one k-tile (128 bytes) where its bit of wok is set (else: the zero page)
  const unsigned char* wptr[WPW];
  unsigned wok = 0;
#pragma unroll
  for (int j = 0; j < WPW; ++j) {
    const int sl = wave + j * NW, r = sl * 8 + lrow;
    const int n = n0 + r;
    const bool ok = sl < HG::WSLABS && n < p.N;
    wptr[j] = ok ? reinterpret_cast<const unsigned char*>(p.W + (size_t)n * p.ldw + kt_begin * 64 + (pchunk ^ swz(r)) * 8) : zero;
    wok |= (ok ? 1u : 0u) << j;
  }
  // piece i of the next chunk's halo into the buffer at byte offset buf; piece j of a weight k-tile into ring slot fs.  `live`: the k-tile
  // exists (past the end the pieces read the zero page: the outstanding-load count stays what the waits assume)
  auto stage_h = [&](int buf, int i) {
    const int sl = wave + i * NW;
    unsigned char* dst = ((i + 1) * NW <= HG::HSLABS || sl < HG::HSLABS) ? smem + buf + sl * 1024 : smem + HG::DUMMY_OFF;
    const unsigned char* base = hnext;
    asm volatile("" : "+s"(base));
    t2v_glds16(base + (size_t)hoff[i], dst);
  };
  auto stage_w = [&](int fs, int j, bool live) {
    const int sl = wave + j * NW;
    unsigned char* dst = ((j + 1) * NW <= HG::WSLABS || sl < HG::WSLABS) ? smem + HG::W_OFF + fs * HG::WSLOT + sl * 1024 : smem + HG::DUMMY_OFF;
    const void* src = live ? wptr[j] : zero;
    wptr[j] += ((wok >> j) & 1u) << 7;
    t2v_glds16(src, dst);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // prologue: chunk 0's halo, then STAGES - 1 weight k-tiles (nkt >= 9: all exist) — the order the waits of the first iterations count on
#pragma unroll
  for (int i = 0; i < HPW; ++i) stage_h(0, i);
  if (nch > 1) hnext += 128;
#pragma unroll
  for (int g = 0; g < STAGES - 1; ++g)
#pragma unroll
    for (int j = 0; j < WPW; ++j) stage_w(g, j, true);

  // fragment addressing: lane reads tile row (block row0 + lane & 31), logical chunk kk * 2 + (lane >> 5)
  const int frow = lane & 31, fhalf = lane >> 5;
  int hrow[TM];                    // halo-buffer row of the centre tap
  unsigned fmask[TM];              // bit t set <=> tap t of this row is inside its image (and the row inside M)
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int r = (wm * TM + a) * 32 + frow;
    const int m = m0 + r;
    hrow[a] = r + HG::PAD;
    const int img = m / hw, rem = m - img * hw;
    const int yo = rem / p.Win, xo = rem - yo * p.Win;
    fmask[a] = 0;
    for (int t = 0; t < 9; ++t) {
      const int yv = yo + t / 3 - 1, xv = xo + t % 3 - 1;
      if (m < p.M && yv >= 0 && yv < p.Hin && xv >= 0 && xv < p.Win) fmask[a] |= 1u << t;
    }
  }
  // (every 32-row block of weight rows starts on a multiple of 32: the swizzle term depends on the lane alone)
  const int wb0 = (wn * TN * 32 + frow) * 128, wsw = swz(frow) << 4;

  int slot = 0;
  auto tap_body = [&](auto tap_c, int c, int hcur) {
    constexpr int tap = decltype(tap_c)::value;
    wait_vmcnt<HG::wait_at(tap)>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int fs = slot + STAGES - 1;
    if (fs >= STAGES) fs -= STAGES;
    const bool wlive = c * 9 + tap + STAGES - 1 < nkt;
    // (opaque to the optimiser: the nine taps' row addresses and mask bits are formed here, tap by tap — hoisted out of the chunk loop
    //  they would be 18 registers per 32-row block, which no tile has)
    int shift = (tap / 3 - 1) * p.Win + (tap % 3 - 1);
    asm volatile("" : "+s"(shift));
    int xb[TM], xs[TM];
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      const int h = hrow[a] + shift;
      unsigned fm = fmask[a];
      asm volatile("" : "+v"(fm));
      const bool on = (fm >> tap) & 1u;
      xb[a] = on ? hcur + h * 128 : HG::ZERO_OFF;
      xs[a] = on ? swz(h) << 4 : 0;
    }
    const unsigned char* st = smem + HG::W_OFF + slot * HG::WSLOT + wb0;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int lc4 = (kk * 2 + fhalf) << 4;
      f16x8 xf[TM], wf[TN];
#pragma unroll
      for (int a = 0; a < TM; ++a) xf[a] = *reinterpret_cast<const f16x8*>(smem + xb[a] + (lc4 ^ xs[a]));
#pragma unroll
      for (int b = 0; b < TN; ++b) wf[b] = *reinterpret_cast<const f16x8*>(st + b * 4096 + (lc4 ^ wsw));
      // this k-step's share of the iteration's pieces (next chunk's halo first, then the weights), placed as gemm2_kernel places its own:
      // with a 2-deep ring they must land before the next barrier and go out in the first half of the k-tile
      constexpr int NH = HG::count(tap), H0 = HG::first(tap), NP = NH + WPW;
      constexpr int SPREAD = STAGES == 2 ? 2 : 4;
      if (kk < SPREAD) {
#pragma unroll
        for (int q = (NP * kk) / SPREAD; q < (NP * (kk + 1)) / SPREAD; ++q) {
          if (q < NH) stage_h(HG::HBYTES - hcur, H0 + q);
          else stage_w(fs, q - NH, wlive);
        }
      }
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[b], xf[a], acc[a][b], 0, 0, 0);
    }
    slot = slot + 1 == STAGES ? 0 : slot + 1;
  };
  int hcur = 0;                    // byte offset of the halo buffer the current chunk reads
  for (int c = 0; c < nch; ++c) {
    tap_body(std::integral_constant<int, 0>{}, c, hcur);
    tap_body(std::integral_constant<int, 1>{}, c, hcur);
    tap_body(std::integral_constant<int, 2>{}, c, hcur);
    tap_body(std::integral_constant<int, 3>{}, c, hcur);
    tap_body(std::integral_constant<int, 4>{}, c, hcur);
    tap_body(std::integral_constant<int, 5>{}, c, hcur);
    tap_body(std::integral_constant<int, 6>{}, c, hcur);
    tap_body(std::integral_constant<int, 7>{}, c, hcur);
    tap_body(std::integral_constant<int, 8>{}, c, hcur);
    hcur = HG::HBYTES - hcur;
    if (c + 2 < nch) hnext += 128;
  }
  wait_vmcnt<0>();   // drain the zero-page loads of the dead stages before the LDS goes away

  // ---- epilogue: the launcher admits T2V_EPI_NONE only (gemm2_kernel's plain tail, with or without the fused GroupNorm)
  __builtin_amdgcn_s_barrier();   // every wave is done reading the operand stages
  if constexpr (XE == T2V_XE_GN) {
    t2v_epilogue_rows_gn<WM, WN, TM, TN>(p, acc, smem, lane, wave, m0, n0, tile_m, tile_n, tiles_m, tiles_n);
    return;
  }
  t2v_epilogue_rows<TM, TN>(p, acc, reinterpret_cast<float*>(smem) + wave * (32 * T2V_EPI_SP), lane, m0 + wm * TM * 32,
                            n0 + wn * TN * 32, blockIdx.y, tile_m * tiles_n + tile_n);
}

// The tiles with a halo instantiation: the table entries the stride-1 ResBlock convolutions of widths <= 32 run on.
constexpr bool conv_halo_tile(int tile) { return tile == 1 || tile == 3 || tile == 5 || tile == 8 || tile == 9 || tile == 11; }
// T2V_CONV_HALO (read once): 0 = every 3x3 convolution of the process takes gemm2_kernel's per-tap staging.
constexpr int CONV_HALO_DEFAULT = 1;
bool conv_halo_enabled() {
  static int mode = -1;
  if (mode < 0) {
    const char* e = getenv("T2V_CONV_HALO");
    mode = e != nullptr ? (strcmp(e, "0") != 0 ? 1 : 0) : CONV_HALO_DEFAULT;
  }
  return mode == 1;
}
// May this launch (split-K already normalised) stage its A operand through the halo buffers?  Anything else: gemm2_kernel, unchanged.
bool conv_halo_eligible(const GemmParams& p) {
  return conv_halo_enabled() && !p.conv_legacy && p.gather == T2V_GATHER_CONV3X3 && p.epi == T2V_EPI_NONE && p.stride == 1 && p.up == 0 &&
         p.halo == 0 && p.a_wrap == 0 && p.Hin == p.Hout && p.Win == p.Wout && p.Win >= 1 && p.Win <= 32 && p.Hin >= 1 && p.Cin % 64 == 0 &&
         p.K == 9 * p.Cin && (p.splitk == 1 || p.kt_per_split % 9 == 0) &&
         ((long)p.M + (long)p.Hin * p.Win) * p.lda * 2 < (1L << 31);      // (the halo pieces' lane offsets are 32-bit byte counts)
}

template <int WM, int WN, int TM, int TN, int BK, int STAGES, int MINW, int GATHER, int XE = T2V_XE_NONE, bool TAT = false, bool HALO = false>
hipError_t launch_cfg_gather(const GemmParams& p, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  static_assert(!HALO || (GATHER == T2V_GATHER_CONV3X3 && BK == 64 && !TAT), "the halo staging is a form of the 3x3 gather");
  // TAT: the attention epilogue re-uses the operand ring for q | k (BM x 272 B) and V^T (<= 12 pixels x 64 x 72 B)
  constexpr int ring = [] {
    if constexpr (HALO) return halo_geom<WM * WN, BM, BN, STAGES>::LDS;
    else return STAGES * (BM + BN) * BK * 2 + 1024;
  }();
  constexpr int gn_lds = t2v_gn_epilogue_lds(WM * WN, WM * TM, BN);
  constexpr int lnx_lds = t2v_lnx_epilogue_lds(WM * WN, WN, BM);
  constexpr int xa_lds = t2v_xattn_epilogue_lds(BM, BN);
  constexpr int lds = TAT ? (BM * 272 + 12 * 64 * 72 > ring ? BM * 272 + 12 * 64 * 72 : ring)
                          : (XE == T2V_XE_GN && gn_lds > ring ? gn_lds : (XE == T2V_XE_LNX && lnx_lds > ring ? lnx_lds : (XE == T2V_XE_XATTN && xa_lds > ring ? xa_lds : ring)));
  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles = ((p.M - p.m_begin + BM - 1) / BM) * tiles_n;
  void (*k)(const GemmParams) = [] {
    if constexpr (HALO) return gemm2_halo_kernel<WM, WN, TM, TN, STAGES, MINW, XE>;
    else return gemm2_kernel<WM, WN, TM, TN, BK, STAGES, MINW, GATHER, XE, TAT>;
  }();
  static t2v_device_flags attr_set;    // once per (instantiation, device): the call costs microseconds on the host
  {
    const hipError_t e = t2v_set_dynamic_lds(reinterpret_cast<const void*>(k), lds, attr_set, s);
    if (e != hipSuccess) return e;
  }
  if constexpr (XE == T2V_XE_GN || XE == T2V_XE_LNX) {
    // the epilogue's grid barrier needs every workgroup of the launch resident: no split-K, and the grid within what the occupancy
    // API grants this instantiation on the stream's device (cached); a process in which a barrier already timed out stays off it
    // (round 6: a grid larger than that is cut into row chunks of whole tiles AND whole statistics instances, one launch each)
    static int occ[T2V_MAX_DEVICES] = {};
    if (p.splitk != 1 || !t2v_coop_allowed()) return hipErrorCooperativeLaunchTooLarge;
    const long cap = t2v_grid_capacity(reinterpret_cast<const void*>(k), WM * WN * 64, lds, s, occ);
    return t2v_launch_coresident(p, BM, tiles_n, cap, XE == T2V_XE_GN ? t2v_lcm(BM, p.gn_rows) : BM, XE == T2V_XE_GN ? 2 * T2V_GN_PIECES * 16 : BM * 16,
                                 [&](const GemmParams& q, int nwg) {
      hipLaunchKernelGGL(k, dim3(nwg, 1), dim3(WM * WN * 64), lds, s, q);
      return hipGetLastError();
    });
  }
  hipLaunchKernelGGL(k, dim3(tiles, p.splitk > 1 ? p.splitk : 1), dim3(WM * WN * 64), lds, s, p);
  return hipGetLastError();
}

// One configuration of the kernel = one entry of the tile table (t2v_kernels.h): which fused epilogues it is instantiated with is the
// entry's feature mask, and the executor has validated the record against the same entry.
template <int TILE, int WM, int WN, int TM, int TN, int BK, int STAGES, int MINW>
hipError_t launch_cfg(const GemmParams& pin, hipStream_t s) {
  constexpr t2v_tile T = *t2v_tile_of(TILE);
  static_assert(T.has(T2V_TILE_GEMM2) && T.bm == WM * TM * 32 && T.bn == WN * TN * 32 && T.waves == WM * WN, "the configuration is not the table's tile");
  GemmParams p = pin;
  // the kernel's epilogue knows these and no other (the executor folds STATS / GN / XATTN into NONE + their pointers before it launches);
  // TATTN: the plain gather only, and below only the temporal-attention tile takes it
  if (p.epi != T2V_EPI_NONE && p.epi != T2V_EPI_GEGLU && !(p.epi == T2V_EPI_TATTN && p.gather == T2V_GATHER_PLAIN)) return hipErrorInvalidValue;
  {
    const int tiles_m = (p.M + T.bm - 1) / T.bm, tiles_n = (p.N + T.bn - 1) / T.bn;
    p.panel = t2v_choose_panel(p, tiles_m, tiles_n);
    t2v_normalize_splitk(p, BK, (long)tiles_m * tiles_n);
  }
  // (with split-K the norm runs in the reduction's launch instead: any tile, t2v_launch_splitk_reduce_gn below)
  const bool gn_here = p.gn_out != nullptr && p.splitk == 1;
  if (gn_here && (!T.has(T2V_TILE_GN) || (p.gather == T2V_GATHER_CONV3X3 && p.up))) return hipErrorInvalidValue;
  if (p.ln_x && (!T.has(T2V_TILE_LNX) || p.gather != T2V_GATHER_PLAIN)) return hipErrorInvalidValue;      // cross-tile LayerNorm: plain gather only
  hipError_t e;
  switch (p.gather) {
    case T2V_GATHER_PLAIN:
      if constexpr (T.has(T2V_TILE_TATTN_ONLY)) {
        if (p.epi != T2V_EPI_TATTN || p.splitk != 1 || p.tpix < 1 || p.tpix > 12 || p.tpix * p.F > T.bm || p.F > 32) return hipErrorInvalidValue;
        e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_PLAIN, T2V_XE_NONE, true>(p, s);
        break;
      }
      if (p.epi == T2V_EPI_TATTN) return hipErrorInvalidValue;
      if constexpr (T.has(T2V_TILE_XATTN)) {
        if (p.xa_k != nullptr) {      // fused to_q + text cross-attention (validated: whole heads per column tile, fp16 out, no split-K)
          e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_PLAIN, T2V_XE_XATTN>(p, s);
          break;
        }
      }
      if (p.xa_k != nullptr) return hipErrorInvalidValue;
      if constexpr (T.has(T2V_TILE_LN)) {
        if (p.ln_out != nullptr) {
          e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_PLAIN, T2V_XE_LN>(p, s);
          break;
        }
      }
      if constexpr (T.has(T2V_TILE_GN)) {
        if (gn_here) { e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_PLAIN, T2V_XE_GN>(p, s); break; }
      }
      if constexpr (T.has(T2V_TILE_LNX)) {
        if (p.ln_x) { e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_PLAIN, T2V_XE_LNX>(p, s); break; }
      }
      e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_PLAIN>(p, s);
      break;
    case T2V_GATHER_CONV3X3:
      if constexpr (conv_halo_tile(TILE)) {
        if (conv_halo_eligible(p)) {
          if constexpr (T.has(T2V_TILE_GN)) {
            if (gn_here) { e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_CONV3X3, T2V_XE_GN, false, true>(p, s); break; }
          }
          e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_CONV3X3, T2V_XE_NONE, false, true>(p, s);
          break;
        }
      }
      if constexpr (T.has(T2V_TILE_GN)) {
        if (gn_here && !p.up) { e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_CONV3X3, T2V_XE_GN>(p, s); break; }
      }
      if (p.up) e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, G_CONV_UP>(p, s);
      else e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_CONV3X3>(p, s);
      break;
    case T2V_GATHER_TCONV3:
      if constexpr (T.has(T2V_TILE_GN)) {
        if (gn_here) { e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_TCONV3, T2V_XE_GN>(p, s); break; }
      }
      e = launch_cfg_gather<WM, WN, TM, TN, BK, STAGES, MINW, T2V_GATHER_TCONV3>(p, s);
      break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  // (split-K whose result feeds a fused GroupNorm: the reduction is the loader of a cooperative GroupNorm launch, norm.hip)
  if (p.splitk > 1 && p.tickets == nullptr) e = p.gn_out != nullptr ? t2v_launch_splitk_reduce_gn(p, s) : t2v_launch_splitk_reduce(p, s);
  return e;
}

// ---- fused GEGLU feed-forward pair (C = 320, hidden = 1280) ---------------------------------------------------------------------------
// out = epilogue2(geglu(X W1^T + b1) W2^T): the GEGLU GEMM (N = 2560, K = 320) and the projection that consumes its result (N = 320,
// K = 1280) as ONE launch — the [M, 1280] fp16 hidden tensor (126 MB written and read back at M = 49152) never reaches HBM.  A workgroup
// owns 192 rows like tile 8 (12 waves, 6 row strips x 2 column halves) and keeps the 192x320 fp32 result in accumulators for the whole
// launch (80 registers per lane); the hidden dimension is walked in 20 chunks of 64 channels = 128 packed value | gate columns:
//   stage 1   5 k-tiles of 64: X rows (24 KiB) + the chunk's 128 W1 rows (16 KiB) -> a 192x128 accumulator (32 registers per lane), in
//             ascending k like the GEGLU GEMM; then bias, value * gelu(gate) and the fp16 rounding of the hidden tensor, exactly where
//             the two-launch form rounds it, into a 192x64 fp16 LDS buffer;
//   stage 2   ONE k-tile of 64: that buffer against the chunk's W2 columns (320 rows x 64 = 40 KiB) into the result accumulators — the
//             same MFMA and the same k order as the projection on tile 8.
// Both kinds of k-tile are 40 KiB, so they go through ONE 3-deep LDS-DMA ring as a stream of 120 tiles with the schedule of
// gemm2_kernel (two tiles in flight, one barrier per tile, counted vmcnt): chunk j + 1's first operands arrive under chunk j's GELU
// and stage 2.  X is streamed again per chunk (from L2).  The tail is the projection's own (t2v_epilogue_rows: bias, row bias, fp32
// residual with its wrap, fp16 hi + lo / fp32 store).  Because no rounding point and no accumulation order moves, the result is
// bit-identical to the two launches.
constexpr int FF_C = 320, FF_HID = 1280, FF_BM = 192, FF_CH = 64, FF_NCHUNK = FF_HID / FF_CH, FF_KT1 = FF_C / 64, FF_TPC = FF_KT1 + 1;
constexpr int FF_NW = 12, FF_SLOT = 40 * 1024, FF_STAGES = 3, FF_LPS = 4;       // 40 1-KiB DMA pieces per tile: 4 per wave, the last 8 are dummies
constexpr int FF_W1_OFF = FF_BM * 128;                                          // W1 rows of a stage-1 tile, behind the 192 X rows
constexpr int FF_HP = FF_CH * 2 + 16;                                           // bytes per row of the hidden chunk (+16: rows start on different banks)
constexpr int FF_H_OFF = FF_STAGES * FF_SLOT, FF_B_OFF = FF_H_OFF + FF_BM * FF_HP, FF_DUMMY_OFF = FF_B_OFF + 2 * FF_HID * 4;
constexpr int FF_LDS = FF_DUMMY_OFF + 1024;                                      // 158 KiB: ring 120, hidden chunk 27, b1 10, dummy piece 1
static_assert(FF_NW * 32 * T2V_EPI_SP * 4 <= FF_H_OFF, "the epilogue strips alias the ring");

__global__ __launch_bounds__(FF_NW * 64, 3) void ff_fused_kernel(const GemmParams p1, const GemmParams p2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * FF_BM;

  // b1 (value | gate interleaved by eights, as the weight rows) -> LDS once: the GELU phase reads it 20 times
  float* b1s = reinterpret_cast<float*>(smem + FF_B_OFF);
  for (int i = tid; i < 2 * FF_HID; i += FF_NW * 64) b1s[i] = p1.bias ? p1.bias[i] : 0.f;

  // ---- per-lane DMA sources (LDS image of gemm2_kernel with 128-byte rows: row r, chunk c at r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) ----
  // piece s = wave + 12 j, j = 0 .. 3, covers rows 8 s .. 8 s + 7 of the tile; stage-1 tile: pieces 0 .. 23 X, 24 .. 39 W1; stage-2 tile:
  // pieces 0 .. 39 W2; pieces 40 .. 47 (j = 3 of waves 4 .. 11) are dummies in both
  const int lrow = lane >> 3, pchunk = lane & 7;
  auto swz = [](int r) { return (r >> 1) & 7; };
  const bool last_real = wave < 4;                             // wave-uniform
  // (a piece's rows move by 96 from j to j + 1: the same swizzle term, so the W offsets of j > 0 are wave-uniform steps from j = 0;
  //  X rows past M read row M - 1 instead — finite operands for rows the epilogue never stores)
  unsigned xoffs[2];               // (unsigned 32-bit lane offsets from wave-uniform bases: the DMA addresses stay scalar base + lane offset)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = (wave + FF_NW * j) * 8 + lrow;
    xoffs[j] = (min(m0 + r, p1.M - 1) * p1.lda + (pchunk ^ swz(r)) * 8) * 2;
  }
  const int wr0 = wave * 8 + lrow, wlc = (pchunk ^ swz(wr0)) * 8;
  const unsigned w1off = (wr0 * p1.ldw + wlc) * 2, w2off = (wr0 * p2.ldw + wlc) * 2;
  const int w1step = 96 * p1.ldw * 2, w2step = 96 * p2.ldw * 2;
  const unsigned char* xb = reinterpret_cast<const unsigned char*>(p1.A);
  const unsigned char* w1b = reinterpret_cast<const unsigned char*>(p1.W);
  const unsigned char* w2b = reinterpret_cast<const unsigned char*>(p2.W);
  const long w1chunk = (long)(2 * FF_CH) * p1.ldw * 2;         // bytes between the W1 rows of consecutive chunks
  // piece j of tile (chunk sc, k-tile sk; sk == FF_KT1: the W2 tile) into ring slot `slot`.  The two tiles staged past the end read the last
  // chunk's again (into slots nobody computes on): the outstanding-load count stays constant and no address needs a per-lane select.
  auto stage_piece = [&](int slot, int sc, int sk, int j) {
    unsigned char* dst = smem + slot * FF_SLOT + (wave + FF_NW * j) * 1024;
    const int scl = min(sc, FF_NCHUNK - 1);
    const bool dummy = j == 3 && !last_real;                  // wave-uniform: rows 320 .. 383 do not exist — the piece re-reads piece 0's source
    const int jj = dummy ? 0 : j;
    const unsigned char* base;                                // wave-uniform part of the address
    unsigned off;                                             // this lane's part
    if (sk == FF_KT1) { base = w2b + (scl * (FF_CH * 2) + jj * w2step); off = w2off; }
    else if (jj < 2) { base = xb + sk * 128; off = xoffs[jj]; }
    else { base = w1b + (scl * w1chunk + sk * 128 + (jj - 2) * w1step); off = w1off; }
    if (dummy) dst = smem + FF_DUMMY_OFF;
    // the base stays in scalar registers and the sum is formed by the instruction (a per-lane 64-bit sum hoisted out of the loop would
    // cost two registers per piece, which this kernel does not have)
    asm volatile("" : "+s"(base));
    const unsigned char* src = base + (size_t)off;
    t2v_glds16(src, dst);
  };

  f32x16 acc2[1][5], acc1[2];
#pragma unroll
  for (int b = 0; b < 5; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[0][b][r] = 0.f;

  // prologue: tiles 0 and 1 in flight
#pragma unroll
  for (int g = 0; g < FF_STAGES - 1; ++g)
#pragma unroll
    for (int j = 0; j < FF_LPS; ++j) stage_piece(g, 0, g, j);

  // fragment addressing: every tile row base of a wave is a multiple of 32, so the swizzle term depends on the lane alone
  const int frow = lane & 31, fhalf = lane >> 5;
  const int fsw = swz(frow) << 4;
  const int xoff = (wm * 32 + frow) * 128;                     // X rows of a stage-1 tile and rows of the hidden chunk
  const int w1o = FF_W1_OFF + (wn * 64 + frow) * 128;          // + b * 4096
  const int w2o = (wn * 160 + frow) * 128;                     // + b * 4096
  unsigned char* hrow = smem + FF_H_OFF + (wm * 32 + frow) * FF_HP + fhalf * 16;   // this lane's row of the hidden chunk, its half of a k-step

  int slot = 0;
  for (int chunk = 0; chunk < FF_NCHUNK; ++chunk) {
#pragma unroll
    for (int kt = 0; kt < FF_TPC; ++kt) {
      wait_vmcnt<FF_LPS*(FF_STAGES - 2)>();                    // this wave's pieces of the tile to compute have landed
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // ... and its stores into the hidden chunk / b1 are done
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      int fs = slot + FF_STAGES - 1;
      if (fs >= FF_STAGES) fs -= FF_STAGES;
      const int sk = (kt + FF_STAGES - 1) % FF_TPC, sc = chunk + (kt + FF_STAGES - 1) / FF_TPC;
      const unsigned char* st = smem + slot * FF_SLOT;
      if (kt < FF_KT1) {
        if (kt == 0) {
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc1[b][r] = 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int lc4 = ((kk * 2 + fhalf) << 4) ^ fsw;
          const f16x8 xf = *reinterpret_cast<const f16x8*>(st + xoff + lc4);
          f16x8 wf[2];
#pragma unroll
          for (int b = 0; b < 2; ++b) wf[b] = *reinterpret_cast<const f16x8*>(st + w1o + b * 4096 + lc4);
          stage_piece(fs, sc, sk, kk);
#pragma unroll
          for (int b = 0; b < 2; ++b) acc1[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[b], xf, acc1[b], 0, 0, 0);
        }
        if (kt == FF_KT1 - 1) {
          // GEGLU of the chunk (the arithmetic of gemm2_kernel's GEGLU epilogue): a lane holds value and gate of 4 hidden channels of
          // ONE row per (b, qq); the fp16 results go to the hidden chunk in the operand image stage 2 reads
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int qq = 0; qq < 2; ++qq) {
              const int n_val = chunk * (2 * FF_CH) + wn * 64 + b * 32 + 16 * qq + 4 * fhalf;
              const f32x4 bv = *reinterpret_cast<const f32x4*>(b1s + n_val);
              const f32x4 bg = *reinterpret_cast<const f32x4*>(b1s + n_val + 8);
              f16x4 o;
#pragma unroll
              for (int r = 0; r < 4; ++r) o[r] = (f16)((acc1[b][8 * qq + r] + bv[r]) * t2v_gelu_erf(acc1[b][8 * qq + 4 + r] + bg[r]));
              const int lc = wn * 4 + b * 2 + qq;              // 16-byte chunk of hidden channels 8 lc .. 8 lc + 7 of the chunk
              *reinterpret_cast<f16x4*>(hrow + lc * 16 - fhalf * 8) = o;
            }
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int lc4 = ((kk * 2 + fhalf) << 4) ^ fsw;
          const f16x8 xf = *reinterpret_cast<const f16x8*>(hrow + kk * 32);
          f16x8 wf[5];
#pragma unroll
          for (int b = 0; b < 5; ++b) wf[b] = *reinterpret_cast<const f16x8*>(st + w2o + b * 4096 + lc4);
          stage_piece(fs, sc, sk, kk);
#pragma unroll
          for (int b = 0; b < 5; ++b) acc2[0][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[b], xf, acc2[0][b], 0, 0, 0);
        }
      }
      slot = slot + 1 == FF_STAGES ? 0 : slot + 1;
    }
  }
  wait_vmcnt<0>();   // drain the loads of the dead stages before the strips alias the ring
  __builtin_amdgcn_s_barrier();
  int elane = lane;
  asm volatile("" : "+v"(elane));      // the tail's per-lane addresses are formed here, not ahead of the loop (where they would be spilled)
  GemmParams q = p2;
  q.splitk = 1; q.tickets = nullptr; q.stats = nullptr;       // (checked by the launcher: the tail's split-K and statistics branches fold away)
  t2v_epilogue_rows<1, 5>(q, acc2, reinterpret_cast<float*>(smem) + wave * (32 * T2V_EPI_SP), elane, m0 + wm * 32, wn * 160, 0, 0);
}

}  // namespace

// The GEGLU GEMM p1 (N = 2560, K = 320, fp16 hidden out) and the projection p2 that reads exactly that result (N = 320, K = 1280) in one
// launch; p1.out is NOT written.  The executor has checked the shapes (executor.hip, ff_pair); anything else is refused here too.
hipError_t t2v_launch_ff_fused(const GemmParams& p1, const GemmParams& p2, hipStream_t s) {
  if (p1.N != 2 * FF_HID || p1.K != FF_C || p2.N != FF_C || p2.K != FF_HID || p1.M != p2.M || p1.M <= 0 || p1.epi != T2V_EPI_GEGLU ||
      p2.epi != T2V_EPI_NONE || p1.splitk != 1 || p2.splitk != 1 || p1.gather != T2V_GATHER_PLAIN || p2.gather != T2V_GATHER_PLAIN ||
      p1.a_wrap || p2.a_wrap || p1.lda < FF_C || p1.ldw < FF_C || p2.ldw < FF_HID || p1.out_f32 || p2.stats != nullptr || p2.tickets != nullptr ||
      (long)p1.M * p1.lda >= (1L << 30) || p2.ldw > 65536 || p1.ldw > 65536)        // (the DMA's lane offsets are 32-bit byte counts)
    return hipErrorInvalidValue;
  static t2v_device_flags attr_set;
  const hipError_t e = t2v_set_dynamic_lds(reinterpret_cast<const void*>(ff_fused_kernel), FF_LDS, attr_set, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ff_fused_kernel, dim3((p1.M + FF_BM - 1) / FF_BM), dim3(FF_NW * 64), FF_LDS, s, p1, p2);
  return hipGetLastError();
}

// One case per gemm2.hip entry of the tile table (t2v_kernels.h: geometry and fused epilogues; launch_cfg checks the numbers below
// against it): waves as WM x WN, MFMA tiles per wave as TM x TN, 64-wide k-tiles (full 128-byte lines per row = one conv reduction
// chunk), ring depth, waves per SIMD.
hipError_t t2v_launch_gemm2(const GemmParams& p, int tile, hipStream_t s) {
  switch (tile) {
    case 1: return launch_cfg<1, 2, 4, 4, 2, 64, 2, 2>(p, s);   // 2 x 64 KiB
    case 2: return launch_cfg<2, 4, 2, 2, 5, 64, 2, 2>(p, s);   // 2 x 72 KiB
    case 3: return launch_cfg<3, 2, 4, 2, 2, 64, 3, 2>(p, s);   // 3 x 48 KiB
    case 4: return launch_cfg<4, 2, 2, 2, 2, 64, 4, 1>(p, s);   // 4 x 32 KiB: 3 k-tiles in flight (few-row levels: latency-bound, keep 96 KiB per CU in flight)
    case 5: return launch_cfg<5, 2, 4, 2, 1, 64, 4, 2>(p, s);   // 4 x 32 KiB
    case 8: return launch_cfg<8, 6, 2, 1, 5, 64, 2, 3>(p, s);   // 3 waves per SIMD, 2 x 64 KiB: M = 49152 -> exactly 256 workgroups
    case 9: return launch_cfg<9, 6, 2, 1, 4, 64, 2, 3>(p, s);   // 2 x 56 KiB (N = 256 * j where 256-row grids fill badly)
    case 10: return launch_cfg<10, 6, 2, 1, 3, 64, 2, 3>(p, s); // fused QKV projection + temporal attention
    case 12: return launch_cfg<12, 2, 2, 1, 1, 64, 4, 2>(p, s); // 4 x 16 KiB (2 workgroups per CU): the 4x4 level (M = 768) as 240 tiles with the
                                                                // FULL reduction each — no split-K slabs, no reduction launch (experiment, round 4)
    case 11: return launch_cfg<11, 4, 2, 1, 5, 64, 2, 2>(p, s); // 2 per SIMD, 2 x 56 KiB: M = 32768 (VideoCrafter, 16 frames) -> exactly
                                                                // 256 workgroups where 192-row tiles make 171; also the b = 1 per-GPU shapes (M = 24576 -> 192)
    default: return hipErrorInvalidValue;
  }
}
