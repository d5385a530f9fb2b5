// T2V_OP_FREEU (include/t2v_hip.h): FreeU at one decoder skip concatenation, in place on the fp32 channels-last concat buffer
// [frames * h * w, ld]: columns [0, C_h / 2) of the stream are multiplied by b, the skip columns [C_h, C_total) pass through the Fourier
// filter of scale s (threshold 1), columns [C_h / 2, C_h) and everything beyond C_total are not touched.  One launch.
//
// The filter scales the frequency bins u in {-1, 0} x v in {-1, 0} (distinct indices modulo the axis length) of every (frame, channel)
// plane, so it needs no FFT:
//     out(y, x) = in(y, x) + (s - 1) / (h w) * sum over the (at most 4) bins of  Re c cos(theta) - Im c sin(theta)
// with c = sum_{y, x} in(y, x) e^{-i theta}, theta = 2 pi (u y / h + v x / w) — at most 7 real sums per plane.
//
// One workgroup of 256 threads per (frame, slab of FREEU_SLAB channels).  Lanes run along the channels (16-byte loads where the
// record's alignment allows, FREEU_SLAB * 4 contiguous bytes per row), the rows of the frame are split over the lanes' row groups.
// Pass 1 adds every thread's rows in ascending order into fp64 partials; the row groups of a wave meet through shuffles, the four
// waves through LDS, both in a fixed order — no atomics, so a result repeats bit for bit.  Pass 2 reads the slab again (it is still
// in cache) and stores in(y, x) + delta, formed in fp64 and rounded once.  cos / sin of 2 pi y / h and 2 pi x / w come from one LDS
// table per workgroup, each entry from sincospi of the exact ratio 2 y / h (never from an accumulated angle).  A channel's sums are
// its own: a non-finite value reaches the plane it sits in and no other.  Slabs of the scaled half are the same grid's first slabs.
#include <hip/hip_runtime.h>

#include "t2v_kernels.h"

namespace {

constexpr int FREEU_SLAB = 64;        // channels per workgroup
constexpr int FREEU_THREADS = 256;
constexpr int FREEU_MAX_AXIS = 1024;  // h, w <= this (the trig table lives in LDS: 2 * (h + w) doubles, 32 KiB at the most)

template <int VEC>
__global__ __launch_bounds__(FREEU_THREADS) void freeu_kernel(float* __restrict__ buf, int hw, int h, int w, long ld, int c_h, int c_total,
                                                              int scale_slabs, float b, float s) {
  constexpr int LPR = FREEU_SLAB / VEC;             // lanes of one row
  constexpr int RPP = FREEU_THREADS / LPR;          // rows per trip of the workgroup
  constexpr int WAVES = FREEU_THREADS / 64;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int t = threadIdx.x, lane_c = t % LPR, r0 = t / LPR;
  const int frame = blockIdx.x, slab = blockIdx.y;
  float* base = buf + (long)frame * hw * ld;

  if (slab < scale_slabs) {
    // ---- the amplified half of the stream: x *= b
    const int col = slab * FREEU_SLAB + lane_c * VEC;
    if (col < c_h / 2) {
      for (int r = r0; r < hw; r += RPP) {
        float* p = base + (long)r * ld + col;
        if constexpr (VEC == 4) {
          f32xN<4> v = *reinterpret_cast<const f32xN<4>*>(p);
          v = v * b;
          *reinterpret_cast<f32xN<4>*>(p) = v;
        } else {
          p[0] = p[0] * b;
        }
      }
    }
    return;
  }

  // ---- the filtered skip columns
  const int c_s = c_total - c_h;
  const int col = (slab - scale_slabs) * FREEU_SLAB + lane_c * VEC;
  const bool live = col < c_s;
  base += c_h + col;
  double* cy = lds;                 // cos(2 pi y / h), y < h
  double* sy = cy + h;
  double* cx = sy + h;              // cos(2 pi x / w), x < w
  double* sx = cx + w;
  double* red = sx + w;             // [WAVES][7][FREEU_SLAB]
  for (int k = t; k < h + w; k += FREEU_THREADS) {
    const bool row = k < h;
    const int idx = row ? k : k - h, n = row ? h : w;
    double sn, cs;
    sincospi(2.0 * (double)idx / (double)n, &sn, &cs);
    (row ? cy : cx)[idx] = cs;
    (row ? sy : sx)[idx] = sn;
  }
  __syncthreads();
  // bins beside (0, 0): (-1, 0) when h >= 2, (0, -1) when w >= 2, (-1, -1) when both (an axis of length 1 has the one bin 0)
  const bool by = h >= 2, bx = w >= 2;

  // sums: 0 = sum v;  1, 2 = sum v cos / sin (2 pi y / h);  3, 4 = sum v cos / sin (2 pi x / w);  5, 6 = sum v cos / sin (2 pi (y / h + x / w))
  double acc[7][VEC];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[k][e] = 0.0;
  if (live) {
    int y = r0 / w, x = r0 - y * w;
    for (int r = r0; r < hw; r += RPP) {
      const float* p = base + (long)r * ld;
      float v[VEC];
      if constexpr (VEC == 4) {
        const f32xN<4> q = *reinterpret_cast<const f32xN<4>*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = q[e];
      } else {
        v[0] = p[0];
      }
      const double cyy = cy[y], syy = sy[y], cxx = cx[x], sxx = sx[x];
      const double cb = cyy * cxx - syy * sxx, sb = syy * cxx + cyy * sxx;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double d = (double)v[e];
        acc[0][e] += d;
        acc[1][e] += d * cyy;
        acc[2][e] += d * syy;
        acc[3][e] += d * cxx;
        acc[4][e] += d * sxx;
        acc[5][e] += d * cb;
        acc[6][e] += d * sb;
      }
      x += RPP;                       // (RPP may exceed w: carry as often as needed)
      while (x >= w) { x -= w; ++y; }
    }
  }
  // the row groups of one wave (lanes that differ by a multiple of LPR), then the waves through LDS: a fixed order
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1)
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[k][e] += __shfl_xor(acc[k][e], off, 64);
  const int wave = t / 64;
  if ((t % 64) < LPR) {
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) red[(wave * 7 + k) * FREEU_SLAB + lane_c * VEC + e] = acc[k][e];
  }
  __syncthreads();
  if (!live) return;
  const double gain = ((double)s - 1.0) / ((double)h * (double)w);
  double tot[7][VEC];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      double a = red[k * FREEU_SLAB + lane_c * VEC + e];
#pragma unroll
      for (int wv = 1; wv < WAVES; ++wv) a += red[(wv * 7 + k) * FREEU_SLAB + lane_c * VEC + e];
      tot[k][e] = a;
    }
  int y = r0 / w, x = r0 - y * w;
  for (int r = r0; r < hw; r += RPP) {
    float* p = base + (long)r * ld;
    float v[VEC];
    if constexpr (VEC == 4) {
      const f32xN<4> q = *reinterpret_cast<const f32xN<4>*>(p);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = q[e];
    } else {
      v[0] = p[0];
    }
    const double cyy = cy[y], syy = sy[y], cxx = cx[x], sxx = sx[x];
    const double cb = cyy * cxx - syy * sxx, sb = syy * cxx + cyy * sxx;
    float o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      double d = tot[0][e];
      if (by) d += tot[1][e] * cyy + tot[2][e] * syy;
      if (bx) d += tot[3][e] * cxx + tot[4][e] * sxx;
      if (by && bx) d += tot[5][e] * cb + tot[6][e] * sb;
      o[e] = (float)((double)v[e] + gain * d);
    }
    if constexpr (VEC == 4) {
      *reinterpret_cast<f32xN<4>*>(p) = f32xN<4>{o[0], o[1], o[2], o[3]};
    } else {
      p[0] = o[0];
    }
    x += RPP;
    while (x >= w) { x -= w; ++y; }
  }
}

}  // namespace

t2v_freeu_view t2v_freeu_decode(const t2v_op& op) {
  t2v_freeu_view v{};
  v.rows = op.i[0]; v.c_total = op.i[1]; v.ld = op.i[2]; v.c_h = op.i[3]; v.frames = op.i[4]; v.h = op.i[5]; v.w = op.i[6];
  v.b = op.f[0]; v.s = op.f[1];
  v.buf = op.p[0];
  auto bad = [&](const char* why) { v.why = why; return v; };
  if (v.rows <= 0 || v.c_total <= 0 || v.frames <= 0 || v.h <= 0 || v.w <= 0) return bad("freeu: rows, C_total, frames, h and w must be positive");
  if (v.h > FREEU_MAX_AXIS || v.w > FREEU_MAX_AXIS) return bad("freeu: h and w <= 1024");
  if (v.c_h <= 0 || v.c_h % 2 != 0) return bad("freeu: the stream width C_h must be positive and even (half of it is scaled)");
  if (v.c_h > v.c_total) return bad("freeu: the stream width C_h exceeds C_total");
  if (v.ld < v.c_total) return bad("freeu: leading dimension < C_total");
  if ((long)v.frames * v.h * v.w != (long)v.rows) return bad("freeu: rows != frames * h * w");
  if ((v.c_total + FREEU_SLAB - 1) / FREEU_SLAB + 1 > 65535) return bad("freeu: too many channels for one launch");
  if (!(v.b == v.b) || !(v.s == v.s) || v.b - v.b != 0.f || v.s - v.s != 0.f) return bad("freeu: b and s must be finite");
  if (v.buf == 0) return bad("null freeu pointer");
  if (v.buf >= T2V_EXT_SLOTS && v.buf % 4 != 0) return bad("freeu: the buffer must be 4-byte aligned");
  v.ok = true;
  return v;
}

hipError_t t2v_launch_freeu(const t2v_op& op, hipStream_t s) {
  const t2v_freeu_view v = t2v_freeu_decode(op);
  if (!v.ok) return hipErrorInvalidValue;      // (every caller has validated the record)
  const int half = v.c_h / 2, c_s = v.c_total - v.c_h;
  const int scale_slabs = (half + FREEU_SLAB - 1) / FREEU_SLAB, filter_slabs = (c_s + FREEU_SLAB - 1) / FREEU_SLAB;
  // 16-byte accesses when every vector the kernel forms is whole and aligned: the buffer, the row pitch, the first skip column, both widths
  const bool vec = v.buf % 16 == 0 && v.ld % 4 == 0 && v.c_h % 8 == 0 && c_s % 4 == 0;
  const size_t lds = sizeof(double) * (2 * (size_t)(v.h + v.w) + (size_t)(FREEU_THREADS / 64) * 7 * FREEU_SLAB);
  const dim3 grid((unsigned)v.frames, (unsigned)(scale_slabs + filter_slabs));
  float* buf = reinterpret_cast<float*>(v.buf);
  if (vec)
    hipLaunchKernelGGL(freeu_kernel<4>, grid, dim3(FREEU_THREADS), lds, s, buf, v.h * v.w, v.h, v.w, (long)v.ld, v.c_h, v.c_total, scale_slabs, v.b, v.s);
  else
    hipLaunchKernelGGL(freeu_kernel<1>, grid, dim3(FREEU_THREADS), lds, s, buf, v.h * v.w, v.h, v.w, (long)v.ld, v.c_h, v.c_total, scale_slabs, v.b, v.s);
  return hipGetLastError();
}
