// GroupNorm(32)(+SiLU) and LayerNorm on channels-last tokens, gfx950 (wave64).
//
// Replaces nn.GroupNorm(32, C) [+ nn.SiLU] at every site of the reference UNet / VAE
// (SURVEY.md §2.3 K9): ResBlock in/out layers (4-D input => per-frame statistics, eps 1e-5,
// t2v_model.py:927,952), TemporalConvBlock_v2 and TemporalTransformer.norm (5-D input =>
// statistics over ALL frames of a sample, t2v_model.py:1202-1211, :690), SpatialTransformer
// .norm (eps 1e-6, :612), VAE Normalize (eps 1e-6, autoencoder_modules.py:34-35); and
// nn.LayerNorm(C) of BasicTransformerBlock (t2v_model.py:798-800, K10).
//
// A statistics "instance" is a contiguous run of `rows` token rows (one frame, or all F frames
// of one sample) x one of 32 channel groups.  Input is the fp32 (or fp16) residual stream
// [rows, C]; output is fp16 — the operand format of the following MFMA GEMM.  Four forms, all selected by the lowering:
//   three launches   gn_stats_kernel (block partials) -> gn_finalize_kernel ({mean, rstd}) -> gn_apply_kernel; the statistics may instead
//                    come from the producing GEMM's strips (gn_finalize_strips*_kernel) or, T-sharded clips, from the gathered parts of
//                    all ranks (phases 1 / 2, see t2v_launch_groupnorm).  4 B + 4 B read, 2 B written per element: HBM-bound.
//   single launch    gn_fused_kernel, one workgroup per (instance, group), for small statistics slices.
//   cooperative      gn_coop_kernel: one pass, the tensor in registers across a statistics exchange between the launch's workgroups.
//   split-K + GN     splitk_gn_kernel: the same with the split-K slab reduction as its loader.
// Every form is built from the helpers below, each written ONCE — LoadN, t2v_mean_rstd / t2v_norm_store (t2v_kernels.h, shared with the GEMM
// epilogues), gn_cast_store, gn_fold_parked, gn_publish, gn_scale_shift, gn_coop_core: the statistics of an instance must be bit-identical
// in every workgroup and on every T-shard rank, and no two copies of the arithmetic exist that could drift apart.
// No atomics on data, every fold in a fixed order in fp64: bitwise reproducible run to run.
#include <climits>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "t2v_kernels.h"

namespace {

// N (4 / 8) consecutive channels of one token row as fp32: 16-byte loads for fp32, one 2N-byte load for fp16
template <typename T, int N> struct LoadN;
template <int N> struct LoadN<float, N> {
  static __device__ __forceinline__ f32xN<N> ld(const float* __restrict__ p) {
    f32xN<N> r;
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p + i);
      r[i] = a[0]; r[i + 1] = a[1]; r[i + 2] = a[2]; r[i + 3] = a[3];
    }
    return r;
  }
};
template <int N> struct LoadN<f16, N> {
  static __device__ __forceinline__ f32xN<N> ld(const f16* __restrict__ p) {
    const f16xN<N> h = *reinterpret_cast<const f16xN<N>*>(p);
    f32xN<N> r;
#pragma unroll
    for (int e = 0; e < N; ++e) r[e] = (float)h[e];
    return r;
  }
};

// Optional second output of a GroupNorm op (round 5): the RAW input cast to fp16 (+ its low-order image at column `lo`) — the operand of the
// 1x1 skip convolution of a ResBlock whose input the norm reads anyway (t2v_model.py:965: skip_connection(x) beside in_layers(x)); the
// separate cast pass (read 4 B + write 2-4 B per element of the concat tensor) disappears.
struct GnCast {
  f16* out;      // null: none
  int ld, lo;    // leading dimension; column offset of the low-order image (0: none)
};
template <int N>
__device__ __forceinline__ void gn_cast_store(const GnCast& c, size_t row, int col, const f32xN<N>& v) {
  f16xN<N> o, l;
#pragma unroll
  for (int e = 0; e < N; ++e) { o[e] = (f16)v[e]; l[e] = (f16)(v[e] - (float)o[e]); }
  f16* dst = c.out + row * c.ld + col;
  *reinterpret_cast<f16xN<N>*>(dst) = o;
  if (c.lo) *reinterpret_cast<f16xN<N>*>(dst + c.lo) = l;
}

__device__ __forceinline__ void gn_store_pair(double* st, double s, double q) {
  st[0] = s;
  st[1] = q;
}

// The per-thread fp32 sums of a workgroup, parked in LDS as psum / psq [R][C], folded per group in fp64 in a fixed order: LANES adjacent
// lanes per group (group tid / LANES) each take a fixed strided subset of the group's R x cpg sums, then a fixed xor tree.  Every thread
// calls (the shuffles are wave-wide); the sums are complete in the first lane of each group.
template <int LANES>
__device__ __forceinline__ void gn_fold_parked(const float* psum, const float* psq, int R, int C, int cpg, int groups, int tid, double& s,
                                               double& q) {
  const int g = tid / LANES, sub = tid % LANES;
  s = 0.0;
  q = 0.0;
  if (g < groups) {
    const int n = R * cpg;
    for (int i = sub; i < n; i += LANES) {
      const int k = i / cpg, c = g * cpg + (i - k * cpg);
      s += (double)psum[k * C + c];
      q += (double)psq[k * C + c];
    }
  }
  for (int o = 1; o < LANES; o <<= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
}

// Tail of the three finalize kernels, (instance, group) pair idx: {mean, rstd} into finals[], or — raw != nullptr: a T-sharded clip's local
// fold — this rank's {sum, sum of squares} for the all-gather.
__device__ __forceinline__ void gn_publish(int idx, double s, double q, double inv_n, float eps, float* finals, double* raw) {
  if (raw != nullptr) { gn_store_pair(raw + 2 * idx, s, q); return; }
  const float2 mr = t2v_mean_rstd(s, q, inv_n, eps);
  finals[2 * idx] = mr.x;
  finals[2 * idx + 1] = mr.y;
}

// scale[c] = rstd * gamma[c] and shift[c] = beta[c] - mean * scale[c] of one instance into LDS, from stat = {mean, rstd}[groups], by the
// `nthreads` threads of the workgroup (the caller synchronises before and after).
__device__ __forceinline__ void gn_scale_shift(float* sc, float* sf, const float* stat, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, int C, int cpg, int nthreads) {
  for (int c = threadIdx.x; c < C; c += nthreads) {
    const int grp = c / cpg;
    const float a = stat[2 * grp + 1] * gamma[c];
    sc[c] = a;
    sf[c] = beta[c] - stat[2 * grp] * a;
  }
}

constexpr int GN_UNROLL = 8;   // token rows a thread keeps in flight (HBM-bound: ~48 KiB per CU must be outstanding)

// Launch 1 — grid (nblk, n_inst), nblk = ceil(rows / rpb).  Threads form R row-replicas x TPR column slots of 8 channels.  Per-thread fp32
// partials are parked in LDS [2][R][C]; gn_fold_parked (8 lanes per group; more than 32 groups: one thread per group walks its sums in
// order) then stores ONE partial per (instance, block, group).
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ x, double* partials, int rows, int C,
                                                       int ld, int groups, int rpb) {
  extern __shared__ float sh[];  // [2][R][C] floats
  const int tid = threadIdx.x;
  const int inst = blockIdx.y;
  const int r0 = blockIdx.x * rpb;
  const int r1 = min(rows, r0 + rpb);
  const T* base = x + ((size_t)inst * rows) * ld;
  const int cv = C >> 3;                       // 8-channel units per row
  const int TPR = cv < 256 ? cv : 256;
  const int R = 256 / TPR;
  const int cs = tid % TPR, rr = tid / TPR;
  float* psum = sh;
  float* psq = sh + R * C;
  if (rr < R) {
    for (int u = cs; u < cv; u += TPR) {
      const int c8 = u * 8;
      f32x8 s = 0.f, q = 0.f;
      for (int r = r0 + rr; r < r1; r += R * GN_UNROLL) {
        f32x8 v[GN_UNROLL];
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) {
          const int rk = r + k * R;
          if (rk < r1) v[k] = LoadN<T, 8>::ld(base + (size_t)rk * ld + c8);
          else v[k] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) { s += v[k]; q += v[k] * v[k]; }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) { psum[rr * C + c8 + e] = s[e]; psq[rr * C + c8 + e] = q[e]; }
    }
  }
  __syncthreads();
  const int cpg = C / groups;
  double* part = partials + ((size_t)inst * gridDim.x + blockIdx.x) * groups * 2;
  if (groups * 8 <= 256) {
    double s, q;
    gn_fold_parked<8>(psum, psq, R, C, cpg, groups, tid, s, q);
    if (tid < groups * 8 && (tid & 7) == 0) gn_store_pair(part + (tid >> 3) * 2, s, q);
  } else if (tid < groups) {
    double s = 0.0, q = 0.0;
    for (int k = 0; k < R; ++k)
      for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { s += (double)psum[k * C + c]; q += (double)psq[k * C + c]; }
    gn_store_pair(part + tid * 2, s, q);
  }
}

// Launch 2 — one wave per (instance, group): ordered fold of the block partials, then gn_publish.
// `nparts` > 1: the partials of all T-shard ranks, gathered as [part][inst][blk][group][2]; the fold
// order (part-major, then block) is the same on every rank, so all ranks get identical statistics.
// (A ticket-elected fold inside launch 1 was measured: same-line L2 atomics serialise at ~25 ns each and the fence + fold tail costs as
// much as this 4-5 us launch — not kept.)
__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* partials, float* finals, int n_inst, int nblk,
                                                          int groups, double inv_n, float eps, int nparts, double* raw) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);  // (inst, group) pair
  if (idx >= n_inst * groups) return;
  const int inst = idx / groups, g = idx - inst * groups;
  double s = 0.0, q = 0.0;
  const int total = nblk * nparts;
  auto at = [&](int u) {
    const int part = u / nblk, b = u - part * nblk;
    return partials + ((((size_t)part * n_inst + inst) * nblk + b) * groups + g) * 2;
  };
  int u = lane;
  for (; u + 192 < total; u += 256) {   // four strided (one cache line each) loads in flight; same summation order
    const double *p0 = at(u), *p1 = at(u + 64), *p2 = at(u + 128), *p3 = at(u + 192);
    const double a0 = p0[0], b0 = p0[1], a1 = p1[0], b1 = p1[1], a2 = p2[0], b2 = p2[1], a3 = p3[0], b3 = p3[1];
    s += a0; q += b0; s += a1; q += b1; s += a2; q += b2; s += a3; q += b3;
  }
  for (; u < total; u += 64) {
    const double* st = at(u);
    s += st[0];
    q += st[1];
  }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
  if (lane == 0) gn_publish(idx, s, q, inv_n, eps, finals, raw);
}

// Phase 3 — statistics from the producing GEMM's epilogue (T2V_EPI_STATS): strips[(inst * nstrips + s)][0 | 1][c] = sum / sum of squares
// of one 32-row strip of column c.  One wave per (instance, group) folds nstrips x cpg pairs in a fixed order in fp64, then gn_publish
// (raw: a T-sharded clip's part, round 6).
__global__ __launch_bounds__(256) void gn_finalize_strips_kernel(const float* __restrict__ strips, float* finals, int n_inst, int nstrips,
                                                                 int groups, int cpg, int ldn, double inv_n, float eps, double* raw) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= n_inst * groups) return;
  const int inst = idx / groups, g = idx - inst * groups;
  const float* base = strips + (size_t)inst * nstrips * 2 * ldn + g * cpg;
  const int total = nstrips * cpg;
  double s = 0.0, q = 0.0;
  for (int u = lane; u < total; u += 64) {
    const int st = u / cpg, c = u - st * cpg;
    const float* p = base + (size_t)st * 2 * ldn + c;
    s += (double)p[0];
    q += (double)p[ldn];
  }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
  if (lane == 0) gn_publish(idx, s, q, inv_n, eps, finals, raw);
}

// The same fold with a whole workgroup per (instance, group), for instances of many strips (cross-frame statistics: 768 strips x 10
// channels at the 32x32 level — one wave per pair walked them in 120 dependent-latency rounds, 46 us; 256 threads keep ~60 independent
// loads each in flight).  Thread t takes strips t, t + 256, ...; fixed reduction order (wave xor-tree, then the 4 waves in order).
__global__ __launch_bounds__(256) void gn_finalize_strips_wg_kernel(const float* __restrict__ strips, float* finals, int nstrips, int groups,
                                                                    int cpg, int ldn, double inv_n, float eps, double* raw) {
  __shared__ double red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int idx = blockIdx.x, inst = idx / groups, g = idx - inst * groups;
  const float* base = strips + (size_t)inst * nstrips * 2 * ldn + g * cpg;
  double s = 0.0, q = 0.0;
  for (int st = tid; st < nstrips; st += 256) {
    const float* p = base + (size_t)st * 2 * ldn;
    float fs = 0.f, fq = 0.f;
    for (int c = 0; c < cpg; ++c) { fs += p[c]; fq += p[ldn + c]; }
    s += (double)fs;
    q += (double)fq;
  }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
  if (lane == 0) { red[2 * wave] = s; red[2 * wave + 1] = q; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < 4; ++w) { a += red[2 * w]; b += red[2 * w + 1]; }
    gn_publish(idx, a, b, inv_n, eps, finals, raw);
  }
}

// Launch 3 — grid (ceil(rows / (R*GN_UNROLL)), n_inst), the thread layout of launch 1.  The workgroup takes the instance's {mean, rstd}
// from `finals`, builds scale / shift in LDS (gn_scale_shift), and every thread then normalises GN_UNROLL rows of its 8 channels per
// column unit (16-byte loads issued together, t2v_norm_store, the raw cast beside it).
// parts != nullptr (phase 2 of a T-sharded norm, round 6): {mean, rstd} come instead from the gathered {sum, sum of squares} parts of all
// ranks ([part][inst][group][2] doubles, part stride part_len), folded HERE, in rank order, by `groups` threads of every workgroup — no
// finalize launch in front of the pass; every rank and every workgroup folds the same values in the same order.
template <typename T, bool SILU>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, const float* __restrict__ finals,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       f16* __restrict__ out, int rows, int C, int ld_in, int ld_out,
                                                       int groups, int lo_off, GnCast cast, const double* parts, int nparts, long part_len,
                                                       double inv_n, float eps) {
  extern __shared__ float sh[];   // scale[C], shift[C] (+ {mean, rstd}[groups] with parts)
  const int tid = threadIdx.x;
  const int inst = blockIdx.y;
  const int cv = C >> 3;
  const float* stat = finals + (size_t)inst * groups * 2;
  if (parts != nullptr) {
    float* fin = sh + 2 * C;
    for (int g = tid; g < groups; g += 256) {
      double s = 0.0, q = 0.0;
      for (int pz = 0; pz < nparts; ++pz) {
        const double* st = parts + (size_t)pz * part_len + ((size_t)inst * groups + g) * 2;
        s += st[0];
        q += st[1];
      }
      const float2 mr = t2v_mean_rstd(s, q, inv_n, eps);
      fin[2 * g] = mr.x;
      fin[2 * g + 1] = mr.y;
    }
    __syncthreads();
    stat = fin;
  }
  gn_scale_shift(sh, sh + C, stat, gamma, beta, C, C / groups, 256);
  __syncthreads();
  const int TPR = cv < 256 ? cv : 256;
  const int R = 256 / TPR;
  const int cs = tid % TPR, rr = tid / TPR;
  if (rr >= R) return;
  const int r0 = blockIdx.x * (R * GN_UNROLL) + rr;
  const T* xb = x + (size_t)inst * rows * ld_in;
  f16* ob = out + (size_t)inst * rows * ld_out;
  for (int u = cs; u < cv; u += TPR) {
    const int c8 = u * 8;
    f32x8 v[GN_UNROLL];
#pragma unroll
    for (int k = 0; k < GN_UNROLL; ++k) {
      const int rk = r0 + k * R;
      if (rk < rows) v[k] = LoadN<T, 8>::ld(xb + (size_t)rk * ld_in + c8);
    }
    const f32x8 a = LoadN<float, 8>::ld(sh + c8), b = LoadN<float, 8>::ld(sh + C + c8);
#pragma unroll
    for (int k = 0; k < GN_UNROLL; ++k) {
      const int rk = r0 + k * R;
      if (rk < rows) {
        t2v_norm_store<8>(ob + (size_t)rk * ld_out + c8, lo_off, v[k], a, b, SILU);     // lo_off: hi + lo operand split (op.i[16])
        if (cast.out) gn_cast_store<8>(cast, (size_t)inst * rows + rk, c8, v[k]);
      }
    }
  }
}

// Single-launch GroupNorm for small statistics slices (op.i[12] = 1; the 16x16 / 8x8 / 4x4 levels, where the three
// launches above cost more than the data movement): one workgroup per (instance, group), XCD-contiguous, streams its
// [rows x C/groups] slice twice — sums, then normalise; the second pass hits L2.  4-channel units (C/groups % 4 == 0),
// 4 rows in flight per thread, fp32 per-thread sums folded in fp64 in a fixed order (wave xor-tree, then waves in
// order); scale / shift of the thread's 4 channels stay in registers.
constexpr int GNF_THREADS = 512;
constexpr int GNF_UNROLL = 4;

template <typename T, bool SILU>
__global__ __launch_bounds__(GNF_THREADS) void gn_fused_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, f16* __restrict__ out, int rows,
                                                               int C, int ld_in, int ld_out, int groups, float eps, int lo_off, GnCast cast) {
  __shared__ double red[2 * (GNF_THREADS / 64)];
  __shared__ float stat[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Workgroup i runs on XCD i % 8 and neighbouring groups share 128-byte lines of every row: give each XCD (= each
  // private L2) a contiguous range of (instance, group) pairs.
  const int nwg = gridDim.x;
  const int pair = (nwg % 8 == 0) ? (int)(blockIdx.x % 8) * (nwg / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int inst = pair / groups, g = pair - inst * groups;
  const int cpg = C / groups;
  const int nu = cpg >> 2;                    // 4-channel units per row of this group
  const int R = GNF_THREADS / nu;             // row replicas
  const int cs = tid % nu, rr = tid / nu;
  const bool live = rr < R;
  const int c0 = g * cpg + cs * 4;
  const T* xb = x + (size_t)inst * rows * ld_in + c0;
  f32x4 s = 0.f, q = 0.f;
  if (live) {
    for (int r = rr; r < rows; r += R * GNF_UNROLL) {
      f32x4 v[GNF_UNROLL];
#pragma unroll
      for (int k = 0; k < GNF_UNROLL; ++k) {
        const int rk = r + k * R;
        if (rk < rows) v[k] = LoadN<T, 4>::ld(xb + (size_t)rk * ld_in);
        else v[k] = 0.f;
      }
#pragma unroll
      for (int k = 0; k < GNF_UNROLL; ++k) { s += v[k]; q += v[k] * v[k]; }
    }
  }
  double ds = (double)s[0] + (double)s[1] + (double)s[2] + (double)s[3];
  double dq = (double)q[0] + (double)q[1] + (double)q[2] + (double)q[3];
  for (int o = 32; o > 0; o >>= 1) { ds += __shfl_xor(ds, o); dq += __shfl_xor(dq, o); }
  if (lane == 0) { red[2 * wave] = ds; red[2 * wave + 1] = dq; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < GNF_THREADS / 64; ++w) { a += red[2 * w]; b += red[2 * w + 1]; }
    const float2 mr = t2v_mean_rstd(a, b, 1.0 / ((double)rows * cpg), eps);
    stat[0] = mr.x;
    stat[1] = mr.y;
  }
  __syncthreads();
  if (!live) return;
  const float mean = stat[0], rstd = stat[1];
  const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c0), bt = *reinterpret_cast<const f32x4*>(beta + c0);
  f32x4 sc, sf;
#pragma unroll
  for (int e = 0; e < 4; ++e) { sc[e] = rstd * gm[e]; sf[e] = bt[e] - mean * sc[e]; }
  f16* ob = out + (size_t)inst * rows * ld_out + c0;
  for (int r = rr; r < rows; r += R * GNF_UNROLL) {
    f32x4 v[GNF_UNROLL];
#pragma unroll
    for (int k = 0; k < GNF_UNROLL; ++k) {
      const int rk = r + k * R;
      if (rk < rows) v[k] = LoadN<T, 4>::ld(xb + (size_t)rk * ld_in);
    }
#pragma unroll
    for (int k = 0; k < GNF_UNROLL; ++k) {
      const int rk = r + k * R;
      if (rk < rows) {
        t2v_norm_store<4>(ob + (size_t)rk * ld_out, lo_off, v[k], sc, sf, SILU);
        if (cast.out) gn_cast_store<4>(cast, (size_t)inst * rows + rk, c0, v[k]);
      }
    }
  }
}


// ---- single-pass cooperative GroupNorm (op.i[15] = 1) and split-K reduction + GroupNorm: one core, two loaders ---------------------------
// The three launches above read the tensor twice (4 + 4 B read, 2 B written per element at 2.6 TB/s aggregate) and pay two
// launch boundaries per site.  Here the grid is at most ONE workgroup per CU, every workgroup loads its rows x C chunk ONCE into
// registers (KR rows x 8 channels per thread: the chip's register files hold the whole tensor, 63 MB at the 32x32 level against
// 128 MB of VGPRs), publishes its {sum, sum of squares} partial per group, meets the others at a grid-wide barrier (or waits for their
// tagged records), folds the partials of its instance (every workgroup the same values in the same order: bit-identical statistics
// everywhere, no atomics on data), and normalises from registers: 4 B read + 2 B written per element, one launch.
// Co-residency: grid <= number of CUs and <= half a CU's threads / registers per workgroup, so all workgroups of the launch
// are resident once earlier kernels on the GPU drain (a spinning workgroup never waits for one that cannot be scheduled).
// With MORE than two processes sharing one GPU that guarantee is gone — such set-ups (the one-GPU multi-process rehearsals)
// select the three-launch path with T2V_GN_COOP=0.
// The grid barrier (sense-reversing, two levels, bounded wait) and the tagged records are t2v_grid_barrier / t2v_rec_* of t2v_kernels.h,
// shared with the fused-norm GEMM epilogues.
constexpr int GNC_THREADS = 512;

// A workgroup's place in the launch: chunk `chunk` (rows r0 .. r1 - 1, rc rows per chunk) of instance `inst`; its threads form R
// row-replicas x C / 8 column slots, thread (rr, c8) holds rows r0 + rr + k * R, k < KR, of channels c8 .. c8 + 7 (live: rr < R).
struct GnCoopTile {
  int inst, chunk, R, rr, c8, r0, r1;
  bool live;
};
__device__ __forceinline__ GnCoopTile gn_coop_tile(int rows, int C, int nchunk, int rc) {
  const int tid = threadIdx.x, cv = C >> 3;
  GnCoopTile t;
  t.inst = blockIdx.x / nchunk;
  t.chunk = blockIdx.x - t.inst * nchunk;
  t.R = GNC_THREADS / cv;
  t.rr = tid / cv;
  t.c8 = (tid % cv) * 8;
  t.live = t.rr < t.R;
  t.r0 = t.chunk * rc;
  t.r1 = min(rows, t.r0 + rc);
  return t;
}
struct GnExchange {
  double* partials;          // records [inst][chunk][group], 16 bytes each
  unsigned *bar, *fault;     // grid barrier words (seq == 0); the host-mapped fault word of the bounded waits
  unsigned seq, want;        // tagged records instead of the grid barrier: this launch's tag / the tag to wait for (0: barrier)
  unsigned gen0;             // barrier mode, thread 0: t2v_grid_epoch, read by the kernel BEFORE its loads
};
struct GnAffine {
  const float *gamma, *beta;
  f16* out;                  // row 0 of the op's output [n_inst * rows, ld]
  int ld, lo_off;
};

// Everything after the loader: v[KR] holds the thread's rows (zeros beyond r1).
//   per-thread sums -> LDS [2][R][C] -> gn_fold_parked, 16 lanes per group (groups <= 32) -> ONE tagged 16-byte record per (chunk, group);
//   grid barrier, or nothing (tags: the fetch below re-polls a record until it carries this launch's number);
//   fold of the instance's nchunk records in a fixed order (the same on every workgroup), EIGHT 16-byte device-scope loads in flight per
//   round — one load-use round trip at a time made this fold the longest phase of the kernel (8 dependent ~2 us latencies);
//   t2v_mean_rstd -> gn_scale_shift into the LDS the parked sums occupied -> t2v_norm_store (and the raw cast, stand-alone op only) per row.
template <bool SILU, int KR>
__device__ __forceinline__ void gn_coop_core(const f32x8 (&v)[KR], const GnCoopTile& t, float* sh, int rows, int C, int groups, int cpg,
                                             int nchunk, const GnExchange& x, double inv_n, float eps, const GnAffine& o, const GnCast& cast) {
  __shared__ float stat[2 * 32];           // {mean, rstd} per group
  const int tid = threadIdx.x;
  const bool tags = x.seq != 0u;
  if (t.live) {
    f32x8 s = 0.f, q = 0.f;
#pragma unroll
    for (int k = 0; k < KR; ++k) { s += v[k]; q += v[k] * v[k]; }
#pragma unroll
    for (int e = 0; e < 8; ++e) { sh[t.rr * C + t.c8 + e] = s[e]; sh[(t.R + t.rr) * C + t.c8 + e] = q[e]; }
  }
  __syncthreads();
  const int g = tid >> 4, sub = tid & 15;
  double ds, dq;
  gn_fold_parked<16>(sh, sh + t.R * C, t.R, C, cpg, groups, tid, ds, dq);
  if (g < groups && sub == 0) {
    double* st = x.partials + (((size_t)t.inst * nchunk + t.chunk) * groups + g) * 2;
    t2v_st_dev(reinterpret_cast<float*>(st), t2v_rec_pack(ds, dq, x.seq));         // one 16-byte device-scope (write-through) store,
    if (!tags) t2v_wait_vm0();                                                     // (barrier mode) complete before this workgroup arrives
  }
  if (!tags) t2v_grid_barrier(x.bar, gridDim.x, x.gen0, x.fault);
  ds = 0.0;
  dq = 0.0;
  if (g < groups) {
    const double* base = x.partials + ((size_t)t.inst * nchunk * groups + g) * 2;
    for (int c = sub; c < nchunk; c += 128) {
      f32x4 rec[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) rec[j] = 0.f;
      const int nrec = min(8, (nchunk - c + 15) / 16);
      t2v_rec_fetch8([&](int j) { return reinterpret_cast<const float*>(base + (size_t)(c + 16 * j) * groups * 2); }, nrec, x.want, x.fault, rec);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nrec) t2v_rec_add(rec[j], ds, dq);
    }
  }
  for (int o2 = 1; o2 < 16; o2 <<= 1) { ds += __shfl_xor(ds, o2); dq += __shfl_xor(dq, o2); }
  if (g < groups && sub == 0) {
    const float2 mr = t2v_mean_rstd(ds, dq, inv_n, eps);
    stat[2 * g] = mr.x;
    stat[2 * g + 1] = mr.y;
  }
  __syncthreads();                                            // (also: everyone is done with the parked sums)
  gn_scale_shift(sh, sh + C, stat, o.gamma, o.beta, C, cpg, GNC_THREADS);
  __syncthreads();
  if (!t.live) return;
  const f32x8 a = LoadN<float, 8>::ld(sh + t.c8), b = LoadN<float, 8>::ld(sh + C + t.c8);
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const int r = t.r0 + t.rr + k * t.R;
    if (r < t.r1) {
      const size_t row = (size_t)t.inst * rows + r;
      t2v_norm_store<8>(o.out + row * o.ld + t.c8, o.lo_off, v[k], a, b, SILU);
      if (cast.out) gn_cast_store<8>(cast, row, t.c8, v[k]);
    }
  }
}

// Loader: plain rows of x.
template <typename T, bool SILU, int KR>
__global__ __launch_bounds__(GNC_THREADS) void gn_coop_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, f16* __restrict__ out, double* partials,
                                                              unsigned* bar, unsigned* fault, int rows, int C, int ld_in, int ld_out,
                                                              int groups, int nchunk, int rc, double inv_n, float eps, int lo_off,
                                                              unsigned seq, unsigned want, GnCast cast) {
  extern __shared__ float sh[];            // parked sums [2][R][C], then scale[C] | shift[C]
  const GnCoopTile t = gn_coop_tile(rows, C, nchunk, rc);
  GnExchange ex = {partials, bar, fault, seq, want, 0u};
  if (seq == 0u && threadIdx.x == 0) ex.gen0 = t2v_grid_epoch(bar);
  f32x8 v[KR];
  if (t.live) {
    const T* xb = x + (size_t)t.inst * rows * ld_in + t.c8;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int r = t.r0 + t.rr + k * t.R;
      if (r < t.r1) v[k] = LoadN<T, 8>::ld(xb + (size_t)r * ld_in);
      else v[k] = 0.f;
    }
  }
  gn_coop_core<SILU, KR>(v, t, sh, rows, C, groups, C / groups, nchunk, ex, inv_n, eps, GnAffine{gamma, beta, out, ld_out, lo_off}, cast);
}

// Loader: the split-K reduction (T2V_EPI_GN on a split-K GEMM, round 5).  The long-K convolutions of the 8x8 / 4x4 levels run split-K: fp32
// slabs, then splitk_reduce_kernel (sum + bias + row bias + residual -> the result), then the GroupNorm that consumes it (one more launch,
// one more read).  Here every thread sums its rows x 8 channels over the slabs into registers (+ bias / row bias / wrapped residual) and
// stores the fp32 (fp16) result only if someone else reads it.
template <bool SILU, int KR>
__global__ __launch_bounds__(GNC_THREADS) void splitk_gn_kernel(const GemmParams p, int nchunk, int rc) {
  extern __shared__ float sh[];            // parked sums [2][R][C], then scale[C] | shift[C]
  const int C = p.N, rows = p.gn_rows;
  const GnCoopTile t = gn_coop_tile(rows, C, nchunk, rc);
  GnExchange ex = {p.gn_part, p.gn_bar, p.gn_fault, p.gn_seq, p.gn_want, 0u};
  if (p.gn_seq == 0u && threadIdx.x == 0) ex.gen0 = t2v_grid_epoch(p.gn_bar);
  f32x8 v[KR];
  if (t.live) {
    const int c8 = t.c8;
    f32x8 cb = 0.f;
    if (p.bias) cb = LoadN<float, 8>::ld(p.bias + c8);
    const size_t zs = (size_t)p.M * p.N;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int r = t.r0 + t.rr + k * t.R;
      if (r < t.r1) {
        const size_t m = (size_t)t.inst * rows + r;
        const float* col = p.ws + m * p.N + c8;
        f32x8 a = LoadN<float, 8>::ld(col);
        for (int z = 1; z < p.splitk; ++z) a += LoadN<float, 8>::ld(col + (size_t)z * zs);      // split order, as the reduction kernel
        a += cb;
        if (p.rowbias) a += LoadN<float, 8>::ld(p.rowbias + (m / p.rows_per_batch) * p.ldrb + c8);
        if (p.res) a += LoadN<float, 8>::ld(p.res + ((p.res_wrap && m >= (size_t)p.res_wrap) ? m - (size_t)p.res_wrap : m) * p.ldr + c8);
        if (p.gn_store_out) {
          if (p.out_f32) {
            float* dst = reinterpret_cast<float*>(p.out) + m * p.ldc + c8;
            *reinterpret_cast<f32x4*>(dst) = f32x4{a[0], a[1], a[2], a[3]};
            *reinterpret_cast<f32x4*>(dst + 4) = f32x4{a[4], a[5], a[6], a[7]};
          } else {
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (f16)a[e];
            *reinterpret_cast<f16x8*>(reinterpret_cast<f16*>(p.out) + m * p.ldc + c8) = o;
          }
        }
        v[k] = a;
      } else {
        v[k] = 0.f;
      }
    }
  }
  gn_coop_core<SILU, KR>(v, t, sh, rows, C, C / p.gn_cpg, p.gn_cpg, nchunk, ex, 1.0 / ((double)rows * p.gn_cpg), p.gn_eps,
                         GnAffine{p.gn_gb, p.gn_gb + C, p.gn_out, p.ld_gn, p.gn_lo}, GnCast{nullptr, 0, 0});
}

// Host-side state of the cooperative path: the fault word (host-mapped, one per process), and per (instantiation, device) the
// number of workgroups of that kernel the occupancy API allows per CU.
struct CoopState {
  unsigned* fault = nullptr;     // hipHostMalloc'ed, mapped: written by a timed-out waiter, read by the host
  bool tried = false, disabled = false, reported = false, peer_reported = false;
};
CoopState g_coop;

unsigned* coop_fault_word() {
  if (!g_coop.tried) {
    g_coop.tried = true;
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess && p != nullptr) {
      g_coop.fault = static_cast<unsigned*>(p);
      g_coop.fault[0] = 0u;      // word 0: a fused-norm wait gave up;  word 1: a peer-window wait gave up (comm.hip)
      g_coop.fault[1] = 0u;
    } else {
      (void)hipGetLastError();
      g_coop.disabled = true;      // no way to report a timeout -> never take the barrier path
    }
  }
  return g_coop.fault;
}

// true when the launch may rely on co-residency: t2v_coop_allowed() (the flag word exists, no earlier fault), and `nwg` workgroups of this
// instantiation fit the stream's device at the occupancy the runtime computes for it (registers, LDS, waves)
template <typename K>
bool coop_fits(K kernel, int nwg, size_t lds, hipStream_t s, int* cache) {
  return t2v_coop_allowed() && t2v_grid_fits(reinterpret_cast<const void*>(kernel), GNC_THREADS, lds, nwg, s, cache);
}

// Run-time value -> template argument: f(std::true_type / std::false_type), and f(std::integral_constant<int, K>) for the K of KS... that
// equals kr (false: none does).  A `static` inside the generic lambda f is one object per instantiation — the per-device occupancy caches.
template <typename F>
void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
template <int... KS, typename F>
bool dispatch_kr(int kr, std::integer_sequence<int, KS...>, F&& f) {
  return ((kr == KS && (f(std::integral_constant<int, KS>{}), true)) || ...);
}

// Chunking of the cooperative kernels: with kr rows per thread a workgroup covers rc = (GNC_THREADS / cv) * kr rows of an instance.  Returns
// the first kr of kr_list (ascending) whose grid, n_inst * nchunk workgroups, is at most one workgroup per CU with at most max_chunk
// chunks per instance; 0: none.
int coop_chunking(int rows, int n_inst, int cv, int ncu, int max_chunk, std::initializer_list<int> kr_list, int* rc_out, int* nchunk_out) {
  for (int kr : kr_list) {
    const int rc = (GNC_THREADS / cv) * kr, nchunk = (rows + rc - 1) / rc;
    if ((long)n_inst * nchunk <= ncu && nchunk <= max_chunk) { *rc_out = rc; *nchunk_out = nchunk; return kr; }
  }
  return 0;
}

template <typename T>
bool gn_coop_launch(bool silu, int kr, dim3 grid, size_t lds, hipStream_t s, const T* x, const float* gamma, const float* beta, f16* out,
                    double* partials, unsigned* bar, int rows, int C, int ld_in, int ld_out, int groups, int nchunk, int rc, double inv_n,
                    float eps, int lo_off, double* records, GnCast cast) {
  bool done = false;
  dispatch_kr(kr, std::integer_sequence<int, 4, 8, 12, 16, 20>{}, [&](auto K) {
    dispatch_bool(silu, [&](auto S) {
      static int occ[T2V_MAX_DEVICES] = {};
      auto kern = gn_coop_kernel<T, decltype(S)::value, decltype(K)::value>;
      if (!coop_fits(kern, (int)grid.x, lds, s, occ)) return;
      // tagged records need a region that only ever holds records (a recycled arena block could hold a matching bit pattern by chance):
      // op.p[7], the program's exchange scratch; without it the grid barrier synchronises and the per-op scratch carries the partials
      unsigned seq = 0, want = 0;
      if (records != nullptr) t2v_exchange_ids(&seq, &want);
      hipLaunchKernelGGL(kern, grid, dim3(GNC_THREADS), lds, s, x, gamma, beta, out, seq != 0u ? records : partials, bar, g_coop.fault, rows, C,
                         ld_in, ld_out, groups, nchunk, rc, inv_n, eps, lo_off, seq, want, cast);
      done = true;
    });
  });
  return done;
}

// LayerNorm: one wave per row, row held in registers (C <= 64*4*MAXV).  A wave walks several rows (grid-stride): gamma / beta
// stay in registers and the NEXT row's loads are issued before the current row's two reductions, so the wave always has a
// row in flight (12 k single-row workgroups per launch were latency-bound: 3.8 TB/s at the 32x32 level).
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* x, const float* gamma, const float* beta,
                                                             f16* out, int M, int C, int ld_in, int ld_out, float eps) {
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * 4;
  int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int cv = C >> 2;
  f32x4 g[MAXV], b[MAXV], v[MAXV], nx[MAXV];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int u = lane + i * 64;
    if (u < cv) {
      g[i] = *reinterpret_cast<const f32x4*>(gamma + u * 4);
      b[i] = *reinterpret_cast<const f32x4*>(beta + u * 4);
      nx[i] = *reinterpret_cast<const f32x4*>(x + (size_t)row * ld_in + u * 4);
    }
  }
  const float inv_c = 1.0f / (float)C;
  for (; row < M; row += nwaves) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) v[i] = nx[i];
    const int nrow = row + nwaves;
    if (nrow < M) {                                   // wave-uniform
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int u = lane + i * 64;
        if (u < cv) nx[i] = *reinterpret_cast<const f32x4*>(x + (size_t)nrow * ld_in + u * 4);
      }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
      if (lane + i * 64 < cv) s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * inv_c;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
      if (lane + i * 64 < cv) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; q += d * d; }
      }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q * inv_c + eps);
    f16* yr = out + (size_t)row * ld_out;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int u = lane + i * 64;
      if (u < cv) {
        f16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (f16)((v[i][e] - mean) * rstd * g[i][e] + b[i][e]);
        *reinterpret_cast<f16x4*>(yr + u * 4) = o;
      }
    }
  }
}

// Wide rows (C > 768: the 8x8 / 4x4 levels, few rows): one row per wave, no register double-buffering.
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* x, const float* gamma, const float* beta,
                                                        f16* out, int M, int C, int ld_in, int ld_out, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (size_t)row * ld_in;
  const int cv = C >> 2;
  f32x4 v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int u = lane + i * 64;
    if (u < cv) {
      v[i] = *reinterpret_cast<const f32x4*>(xr + u * 4);
      s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int u = lane + i * 64;
    if (u < cv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; q += d * d; }
    }
  }
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = rsqrtf(q / (float)C + eps);
  f16* yr = out + (size_t)row * ld_out;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int u = lane + i * 64;
    if (u < cv) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + u * 4);
      const f32x4 b = *reinterpret_cast<const f32x4*>(beta + u * 4);
      f16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (f16)((v[i][e] - mean) * rstd * g[e] + b[e]);
      *reinterpret_cast<f16x4*>(yr + u * 4) = o;
    }
  }
}

}  // namespace

int t2v_num_cus(hipStream_t s) {
  static int ncu[T2V_MAX_DEVICES] = {};
  const int d = t2v_device_of(s);
  if (ncu[d] == 0) {
    hipDeviceProp_t prop;
    ncu[d] = (hipGetDeviceProperties(&prop, d) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 1;
  }
  return ncu[d];
}

hipError_t t2v_launch_splitk_reduce_gn(const GemmParams& p, hipStream_t s) {
  const int cv = p.N / 8;
  if (p.N % 8 != 0 || cv > GNC_THREADS || p.gn_cpg <= 0 || p.N / p.gn_cpg > 32 || p.gn_rows <= 0 || p.M % p.gn_rows != 0)
    return hipErrorCooperativeLaunchTooLarge;
  const int n_inst = p.M / p.gn_rows;
  // the FEWEST rows per thread whose grid is still resident at once: the loader sums `splitk` slabs per element, and at the 4x4 level
  // (768 rows) 4 rows per thread left 64 workgroups to read 8 slabs — measured slower than the reduction kernel + the norm it replaces
  int rc = 0, nchunk = 0;
  const int kr = coop_chunking(p.gn_rows, n_inst, cv, t2v_num_cus(s), INT_MAX, {1, 2, 4, 8, 12, 16, 20}, &rc, &nchunk);
  if (kr == 0 || !t2v_coop_allowed() || p.epi != T2V_EPI_NONE || p.act != 0 || p.bias_m) return hipErrorCooperativeLaunchTooLarge;
  const size_t lds = (size_t)2 * (GNC_THREADS / cv) * p.N * sizeof(float);
  const dim3 grid(n_inst * nchunk);
  hipError_t err = hipErrorInvalidValue;
  dispatch_kr(kr, std::integer_sequence<int, 1, 2, 4, 8, 12, 16, 20>{}, [&](auto K) {
    dispatch_bool(p.gn_silu != 0, [&](auto S) {
      static int occ[T2V_MAX_DEVICES] = {};
      auto kern = splitk_gn_kernel<decltype(S)::value, decltype(K)::value>;
      if (!t2v_grid_fits(reinterpret_cast<const void*>(kern), GNC_THREADS, lds, grid.x, s, occ)) { err = hipErrorCooperativeLaunchTooLarge; return; }
      hipLaunchKernelGGL(kern, grid, dim3(GNC_THREADS), lds, s, p, nchunk, rc);
      err = hipGetLastError();
    });
  });
  return err;
}

// Sequence numbers of the tagged-record exchange: process-wide, never 0, never repeated within 2^32 fused-norm launches (a record slot
// is rewritten by every launch that uses it, long before the numbers wrap).  T2V_EXCHANGE=barrier selects the grid barrier instead
// (seq = want = 0).  t2v_debug_poison_exchange(n): the next n launches expect a number nobody publishes — the bounded wait's test.
static unsigned g_seq = 0;
static int g_poison = 0;
static int g_exchange_mode = -1;      // 1 = tagged records, 0 = grid barrier
void t2v_exchange_ids(unsigned* seq, unsigned* want) {
  if (g_exchange_mode < 0) {
    const char* e = getenv("T2V_EXCHANGE");
    g_exchange_mode = (e != nullptr && strcmp(e, "barrier") == 0) ? 0 : 1;
  }
  if (g_exchange_mode == 0) { *seq = *want = 0u; return; }
  unsigned v = __atomic_add_fetch(&g_seq, 1u, __ATOMIC_RELAXED);
  if (v == 0u) v = __atomic_add_fetch(&g_seq, 1u, __ATOMIC_RELAXED);
  *seq = v;
  *want = v;
  if (__atomic_load_n(&g_poison, __ATOMIC_RELAXED) > 0) {
    __atomic_sub_fetch(&g_poison, 1, __ATOMIC_RELAXED);
    *want = v ^ 0x80008000u;
  }
}
extern "C" void t2v_debug_poison_exchange(int n) { __atomic_store_n(&g_poison, n, __ATOMIC_RELAXED); }

unsigned* t2v_coop_fault_word() { return coop_fault_word(); }

bool t2v_coop_allowed() {
  if (g_coop.disabled || coop_fault_word() == nullptr) return false;
  if (__atomic_load_n(g_coop.fault, __ATOMIC_RELAXED) != 0u) { g_coop.disabled = true; return false; }
  return true;
}

unsigned* t2v_peer_fault_word() {
  unsigned* f = coop_fault_word();
  return f ? f + 1 : nullptr;
}

int t2v_async_fault_pending() {
  if (g_coop.fault == nullptr) return 0;
  if (__atomic_load_n(g_coop.fault + 1, __ATOMIC_RELAXED) != 0u && !g_coop.peer_reported) return 1;
  return __atomic_load_n(g_coop.fault, __ATOMIC_RELAXED) != 0u && !g_coop.reported;
}

int t2v_async_fault_consume(std::string* msg) {
  if (!t2v_async_fault_pending()) return 0;
  if (__atomic_load_n(g_coop.fault + 1, __ATOMIC_RELAXED) != 0u && !g_coop.peer_reported) {
    g_coop.peer_reported = true;
    if (msg) *msg = "peer exchange: a workgroup gave up waiting for a peer rank's message in its window (T2V_PEER_TIMEOUT_MS; the peer died, "
                    "ran a different program, or its stores are not visible here); the results of the run that was in flight are invalid.  "
                    "The exchanges of this process go through RCCL from now on (T2V_PEER_WINDOW=0 selects that from the start)";
    return 1;
  }
  g_coop.reported = true;
  g_coop.disabled = true;
  if (msg) *msg = "fused normalisation: a workgroup gave up waiting for the statistics of the other workgroups of its launch (the device is "
                  "shared with another client that holds compute units); the results of the run that was in flight are invalid.  The "
                  "three-launch GroupNorm is used from now on; programs with norms fused into GEMM epilogues must be lowered again with "
                  "T2V_GN_COOP=0 (which selects the unfused forms from the start)";
  return 1;
}

// Scratch (op.p[4], owned by the caller): fp64 partials [nparts][n_inst][nblk][groups][2] followed by
// fp32 finals [n_inst][groups][2], nblk = ceil(rows / rpb), rpb = op.i[11] (0: T2V_GN_ROWS_PER_BLOCK).
// op.i[8] = phase: 0 = whole op; 1 = statistics only (writes this rank's partials into part op.i[10]);
//                  2 = fold the op.i[9] gathered parts + normalise (after the partials all-gather).
hipError_t t2v_launch_groupnorm(const t2v_op& op, hipStream_t s) {
  const int n_inst = op.i[0], rows = op.i[1], C = op.i[2], ld_in = op.i[3], groups = op.i[4];
  const int in_dt = op.i[5], silu = op.i[6], ld_out = op.i[7];
  const int phase = op.i[8], nparts = op.i[9] > 0 ? op.i[9] : 1, part = op.i[10];
  const int rpb = op.i[11] > 0 ? op.i[11] : T2V_GN_ROWS_PER_BLOCK;
  if (C % 8 != 0 || ld_in % 8 != 0 || ld_out % 8 != 0 || C % groups != 0 || groups > 256 || n_inst <= 0 || rows <= 0 ||
      op.p[4] == 0 || part < 0 || part >= nparts || phase < 0 || phase > 3)
    return hipErrorInvalidValue;
  if (phase == 3 && (op.p[6] == 0 || rows % 32 != 0 || op.i[17] < C || nparts != 1)) return hipErrorInvalidValue;
  // phase 1 with producer strips (p[6] != 0, round 6): this rank's part of a T-sharded cross-frame norm comes from the T2V_EPI_STATS strips of
  // the GEMM that produced x — ONE small fold launch instead of a statistics pass over the tensor + a fold
  const bool strips1 = phase == 1 && op.p[6] != 0;
  if (strips1 && (rows % 32 != 0 || op.i[17] < C)) return hipErrorInvalidValue;
  if ((op.i[21] != 0 || op.i[22] != 0) && (phase != 2 || n_inst != 1 || op.i[21] < 0 || op.i[22] < 0 || op.p[8] != 0)) return hipErrorInvalidValue;
  // T-sharded clips (phase 1 / 2): every rank folds ITS OWN block partials to one {sum, sum of squares} pair per
  // (instance, group) — 512 bytes per instance — and only those are all-gathered; phase 2 sums the parts in rank order
  // (every rank: same values, same order => bit-identical statistics) over the rows of the whole clip (i[14]).
  const long rows_total = op.i[14] > 0 ? (long)op.i[14] : (long)rows * nparts;
  const int nblk = (rows + rpb - 1) / rpb;
  const bool whole = phase == 0 || phase == 3;         // scratch layout of an unsharded op: [block partials][finals]
  const size_t part_len = whole ? (size_t)n_inst * nblk * groups * 2 : (size_t)n_inst * groups * 2;        // doubles per gathered part
  double* partials = reinterpret_cast<double*>(op.p[4]);
  double* local = whole ? partials : partials + part_len * nparts;                                         // block partials of this rank
  float* finals = reinterpret_cast<float*>(local + (size_t)n_inst * nblk * groups * 2);
  const dim3 g1(nblk, n_inst);
  const int cv = C / 8;
  const int R = cv < 256 ? 256 / cv : 1;
  const size_t lds = 2 * (size_t)R * C * sizeof(float);
  const int g2 = (n_inst * groups + 3) / 4;
  const double inv_n = 1.0 / ((double)rows_total * (C / groups));
  const float* gamma = reinterpret_cast<const float*>(op.p[1]);
  const float* beta = reinterpret_cast<const float*>(op.p[2]);
  f16* out = reinterpret_cast<f16*>(op.p[3]);
  const bool fused = op.i[12] != 0;
  const int lo_off = op.i[16] != 0 ? C : 0;        // hi + lo operand split: low-order images at columns C .. 2C-1 of the output rows
  // second output: the raw input as fp16 (+ low-order image), p[8] [n_inst * rows, i[19]], i[20] = column of the low-order image (0: none)
  const GnCast cast = {reinterpret_cast<f16*>(op.p[8]), op.i[19], op.i[20]};
  if (cast.out != nullptr && (phase == 1 || cast.ld < C + (cast.lo ? C : 0) || cast.ld % 8 != 0 || cast.lo % 8 != 0)) return hipErrorInvalidValue;
  if (lo_off && (phase == 1 || ld_out < 2 * C)) return hipErrorInvalidValue;
  if (fused && (phase != 0 || (C / groups) % 4 != 0 || (C / groups) / 4 > GNF_THREADS)) return hipErrorInvalidValue;
  // single-pass cooperative variant: the smallest rows-per-thread count whose grid still fits one workgroup per CU, with no more chunks than
  // the three-launch path has blocks (its scratch carries the partials in barrier mode)
  int coop_kr = 0, coop_rc = 0, coop_nchunk = 0;
  if (op.i[15] != 0 && op.p[5] != 0 && phase == 0 && !fused && groups <= 32 && cv <= GNC_THREADS)
    coop_kr = coop_chunking(rows, n_inst, cv, t2v_num_cus(s), nblk, {4, 8, 12, 16, 20}, &coop_rc, &coop_nchunk);
  auto run = [&](auto* x) {
    using T = typename std::remove_cv<typename std::remove_pointer<decltype(x)>::type>::type;
    if (coop_kr) {
      const size_t ldsc = (size_t)2 * (GNC_THREADS / cv) * C * sizeof(float);
      unsigned* bar = reinterpret_cast<unsigned*>(op.p[5]);
      const dim3 grid(n_inst * coop_nchunk);
      double* records = ((size_t)n_inst * coop_nchunk * groups * 16 <= (size_t)op.i[18]) ? reinterpret_cast<double*>(op.p[7]) : nullptr;
      if (gn_coop_launch(silu != 0, coop_kr, grid, ldsc, s, x, gamma, beta, out, partials, bar, rows, C, ld_in, ld_out, groups, coop_nchunk, coop_rc,
                         inv_n, op.f[0], lo_off, records, cast))
        return;                     // else: not provably co-resident (or a fault was raised earlier) -> the three launches below
    }
    if (fused) {
      dispatch_bool(silu != 0, [&](auto S) {
        hipLaunchKernelGGL((gn_fused_kernel<T, decltype(S)::value>), dim3(groups * n_inst), dim3(GNF_THREADS), 0, s, x, gamma, beta, out, rows, C,
                           ld_in, ld_out, groups, op.f[0], lo_off, cast);
      });
      return;
    }
    double* raw_part = strips1 ? partials + part_len * part : nullptr;
    if ((phase == 3 || strips1) && (long)(rows / 32) * (C / groups) > 1024)
      hipLaunchKernelGGL(gn_finalize_strips_wg_kernel, dim3(n_inst * groups), dim3(256), 0, s, reinterpret_cast<const float*>(op.p[6]), finals,
                         rows / 32, groups, C / groups, op.i[17], inv_n, op.f[0], raw_part);
    else if (phase == 3 || strips1)
      hipLaunchKernelGGL(gn_finalize_strips_kernel, dim3(g2), dim3(256), 0, s, reinterpret_cast<const float*>(op.p[6]), finals, n_inst, rows / 32,
                         groups, C / groups, op.i[17], inv_n, op.f[0], raw_part);
    else if (phase != 2)
      hipLaunchKernelGGL(gn_stats_kernel<T>, g1, dim3(256), lds, s, x, local, rows, C, ld_in, groups, rpb);
    if (phase == 1 && !strips1)
      hipLaunchKernelGGL(gn_finalize_kernel, dim3(g2), dim3(256), 0, s, local, finals, n_inst, nblk, groups, 0.0, 0.f, 1,
                         partials + part_len * part);
    if (phase != 1) {
      // phase 2 (round 6): the gathered parts are folded inside the apply pass (no finalize launch)
      const double* parts2 = phase == 2 ? partials : nullptr;
      if (phase == 0)
        hipLaunchKernelGGL(gn_finalize_kernel, dim3(g2), dim3(256), 0, s, partials, finals, n_inst, nblk, groups,
                           inv_n, op.f[0], nparts, static_cast<double*>(nullptr));
      const int rpa = R * GN_UNROLL;    // rows per normalise workgroup
      // phase 2 of a T-sharded clip (T2V_OP_STATS_HALO): i[21] / i[22] rows in front of / behind x hold the neighbours' RAW boundary
      // frames; they take the same statistics and land in front of / behind `out` (what the neighbour wrote for itself, bit for bit)
      const int before = phase == 2 ? op.i[21] : 0, after = phase == 2 ? op.i[22] : 0;
      const int arows = rows + before + after;
      const T* ax = x - (size_t)before * ld_in;
      f16* aout = out - (size_t)before * ld_out;
      const dim3 g3((arows + rpa - 1) / rpa, n_inst);
      const size_t lds3 = (2 * (size_t)C + (parts2 ? 2 * (size_t)groups : 0)) * sizeof(float);
      dispatch_bool(silu != 0, [&](auto S) {
        hipLaunchKernelGGL((gn_apply_kernel<T, decltype(S)::value>), g3, dim3(256), lds3, s, ax, finals, gamma, beta, aout, arows, C, ld_in, ld_out, groups,
                           lo_off, cast, parts2, nparts, (long)part_len, inv_n, op.f[0]);
      });
    }
  };
  if (in_dt == T2V_F32) run(reinterpret_cast<const float*>(op.p[0]));
  else run(reinterpret_cast<const f16*>(op.p[0]));
  return hipGetLastError();
}

hipError_t t2v_launch_layernorm(const t2v_op& op, hipStream_t s) {
  const int M = op.i[0], C = op.i[1], ld_in = op.i[2], ld_out = op.i[3];
  if (C % 4 != 0 || C > 64 * 4 * 8) return hipErrorInvalidValue;
  const float* x = reinterpret_cast<const float*>(op.p[0]);
  const float* gamma = reinterpret_cast<const float*>(op.p[1]);
  const float* beta = reinterpret_cast<const float*>(op.p[2]);
  f16* out = reinterpret_cast<f16*>(op.p[3]);
  // C <= 768 (the 32x32 / 16x16 levels: many rows): at most 8 workgroups per CU, longer tensors are walked grid-stride
  // (~6 rows per wave at the 32x32 level); wider rows: one row per wave
  const int wgs = (M + 3) / 4;
  const int cap = op.i[4] > 0 ? op.i[4] : 8 * 256;
  const dim3 grid_rows(wgs < cap ? wgs : cap), grid(wgs);
  auto launch = [&](auto kern, dim3 g) { hipLaunchKernelGGL(kern, g, dim3(256), 0, s, x, gamma, beta, out, M, C, ld_in, ld_out, op.f[0]); };
  if (C <= 64 * 4 * 2) launch(layernorm_rows_kernel<2>, grid_rows);
  else if (C <= 64 * 4 * 3) launch(layernorm_rows_kernel<3>, grid_rows);
  else if (C <= 64 * 4 * 5) launch(layernorm_kernel<5>, grid);
  else launch(layernorm_kernel<8>, grid);
  return hipGetLastError();
}
