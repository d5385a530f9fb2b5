// Layout, pointwise and sampler-update kernels (HBM-bound, vectorised), gfx950.
//
//   ncthw_to_cl   'b c f h w -> (b f h w) c' entry conversion of the 4-channel latent
//                 (reference does this as rearrange + .contiguous(), t2v_model.py:429)
//   cl_to_ncthw   exit conversion of eps / decoded RGB            (t2v_model.py:456-458)
//   time_embed    sinusoidal_embedding (cos | sin), t2v_model.py:504-515
//   copy2d        strided 2-D copy / fp32->fp16 cast / SiLU: torch.cat of skip connections
//                 (t2v_model.py:444), operand staging, SiLU(e) of emb_layers (:936)
//   ddim_step     DDIM_Gaussian update incl. half-channel classifier-free guidance
//                 (samplers/ddim/gaussian_sampler.py:125-136, 103-108, 199-211, 269-283); a compile-time variant adds the
//                 known-region blend of a masked LVDM step (lvdm/samplers/ddim.py:188-195) to the same launch
//   the strict forms of a DDIM_STEP record (t2v_ddim_classify names a record's form once, for validation, output slots and launch); they
//   share one view of the record (DdimView), one guidance combine (ddim_combine) and one x0 (ddim_x0_of), every operation rounded by itself:
//     ddim_restrict   the DDIM_Gaussian step with its x0 clamped or thresholded by a per-video quantile of |x0| (restrict_range_x0,
//                     gaussian_sampler.py:110-120) and / or the classifier-guidance term (get_eps, :199-211); its x0 form 1 is the apply
//                     pass of UniPC's thresholded data prediction (uni_pc/uni_pc.py:351-364), clamp(x0, -s, s) / s
//     ddim_measure    the quantile of |x0| per video, of either x0 form: torch.quantile on fp32, exactly, by a radix select in one workgroup
//     ddim_keyframe   the DDIM_Gaussian step and the keyframe blend of the legacy img2vid loop (modelscope/t2v_model.py:1555-1562)
//     ddim_invert     the DDIM inversion step of DDIMSampler.encode (samplers/ddim/sampler.py:242-254), four elements per thread
//   resample      one pass of Pillow's 8-bit Lanczos resize of the vid2vid / inpainting input, bit-exact
//                 (process_modelscope.py:116-120, 174-178); the last pass can write the VAE encoder's tokens
//   bicubic       torch's F.interpolate(mode="bicubic", align_corners=False) of planar float images, both axes in one launch: the resizes
//                 around the depth estimator of the VideoCrafter depth adapter (ddpm3d.py:1443-1462); T2V_OP_RESAMPLE with i[9] = 1
//   depth_tokens  entry of the VideoCrafter depth adapter: per-frame min-max normalisation (ddpm3d.py:1463-1464) + PixelUnshuffle(8)
//                 (adapter.py:93-99) of the depth frames, as the fp16 tokens conv_in reads
//   avgpool2      the adapter's Downsample(use_conv=False): nn.AvgPool2d(2, 2) on channels-last fp32 tokens
//   fingerprint   one 64-bit value per byte range of a table (the parameters of a model): which tensors were edited in place since
//                 the weight images were packed (packing.ParamFingerprint)
//   lora_merge    W += alpha * (B A) for every weight of a table, in place: the Stable LoRA merge / un-merge of one file in one launch
//                 (stable_lora/stable_utils/lora_processor.py:50-101, 202-246; stable_lora.py)
#include <type_traits>

#include "t2v_kernels.h"

namespace {

template <typename TIN>
__global__ __launch_bounds__(256) void ncthw_to_cl_kernel(const TIN* in, f16* out, int B, int C, int F, int HW,
                                                          int ld, float scale, int Bsrc, f16* out_lo, int lo_in_pad) {
  // one thread per output token; writes ld (>= C, multiple of 4) channels, zero padded.  Bsrc < B: the source holds
  // Bsrc samples and output sample b reads source sample b % Bsrc (the cond | uncond pair of a guided step shares x_t,
  // gaussian_sampler.py:161-162 — no torch.cat([x, x]) on the host)
  const long total = (long)B * F * HW;
  for (long tkn = (long)blockIdx.x * 256 + threadIdx.x; tkn < total; tkn += (long)gridDim.x * 256) {
    const long bf = tkn / HW;
    const int pix = (int)(tkn - bf * HW);
    const int b = (int)(bf / F), f = (int)(bf - (long)b * F);
    const int bs = b % Bsrc;
    f16* o = out + tkn * ld;
    for (int c = 0; c < ld; ++c) {
      float v = 0.f;
      if (c < C) v = (float)in[(((size_t)bs * C + c) * F + f) * HW + pix] * scale;
      const f16 hi = (f16)v;
      o[c] = hi;
      if (out_lo) out_lo[tkn * ld + c] = (f16)(v - (float)hi);      // low-order image: hi + lo carries the fp32 value (p[2])
    }
    if (lo_in_pad) {     // i[7]: the low-order images go into the padding channels C .. 2C-1 of the SAME row (ld >= 2C): a consumer
                         // whose weights repeat W for those channels computes (hi + lo) . W in one pass
      for (int c = 0; c < C; ++c) {
        const float v = (float)in[(((size_t)bs * C + c) * F + f) * HW + pix] * scale;
        o[C + c] = (f16)(v - (float)(f16)v);
      }
    }
  }
}

template <typename TOUT>
__global__ __launch_bounds__(256) void cl_to_ncthw_kernel(const float* in, TOUT* out, int B, int C, int F, int HW,
                                                          int ld) {
  // one thread per output element (coalesced along pixels)
  const long total = (long)B * C * F * HW;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int pix = (int)(idx % HW);
    long r = idx / HW;
    const int f = (int)(r % F); r /= F;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    out[idx] = (TOUT)in[(((size_t)b * F + f) * HW + pix) * ld + c];
  }
}

__global__ __launch_bounds__(256) void time_embed_kernel(const float* t, const float* freqs, f16* out, int B,
                                                         int dim) {
  const int half = dim / 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * half) return;
  const int b = idx / half, i = idx - b * half;
  const float a = t[b] * freqs[i];
  out[(size_t)b * dim + i] = (f16)cosf(a);
  out[(size_t)b * dim + half + i] = (f16)sinf(a);
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void copy2d_kernel(const TS* src, TD* dst, int rows, int cols, int lds_,
                                                     int ldd, int act, f16* dst_lo) {
  const int cv = cols >> 2;
  const long total = (long)rows * cv;
  for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long)gridDim.x * 256) {
    const long r = u / cv;
    const int c = (int)(u - r * cv) * 4;
    const TS* s = src + r * lds_ + c;
    TD* d = dst + r * ldd + c;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)s[e];
    if (act == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = t2v_silu(v[e]);
    } else if (act == 2) {            // nn.GELU (erf): OpenCLIP ViT-H text MLP
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = t2v_gelu_erf(v[e]);
    } else if (act == 3) {            // quick GELU x * sigmoid(1.702 x): OpenAI CLIP-L text MLP
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f + __expf(-1.702f * v[e]));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = (TD)v[e];
    if (dst_lo) {                     // low-order fp16 image of an fp32 -> fp16 cast (same leading dimension): hi + lo = v to ~2^-22
#pragma unroll
      for (int e = 0; e < 4; ++e) dst_lo[r * ldd + c + e] = (f16)(v[e] - (float)(f16)v[e]);
    }
  }
}

// out[r, :] = table[ids[r], :] + pos[r % L, :]   (token + positional embedding of the CLIP text towers);
// ids outside [0, vocab) write zeros + pos so that a bad token cannot read out of bounds
template <typename TT>
__global__ __launch_bounds__(256) void embed_rows_kernel(const int* ids, const TT* table, const float* pos, float* out,
                                                         int rows, int W, int L, int vocab) {
  const int r = blockIdx.x;
  const int id = ids[r];
  const bool ok = id >= 0 && id < vocab;
  const TT* t = table + (size_t)(ok ? id : 0) * W;
  const float* pr = pos + (size_t)(r % L) * W;
  for (int c = threadIdx.x; c < W; c += 256) out[(size_t)r * W + c] = (ok ? (float)t[c] : 0.f) + pr[c];
}

struct DdimParams {
  const void* xt; const void* eps; const float* noise; void* out;
  int C, inner, guided, eps_f32, x_f32, mode, cps;
  float a_recip, a_recipm1, sqrt_aprev, dir_coef, sigma, gscale;
};

// i[7] = 1: the known-region blend of a masked LVDM step (lvdm/samplers/ddim.py:188-195), all fp32 and dense like x
struct DdimBlend {
  const float* x0; const float* mask; const float* qnoise;
  float sqrt_ac, sqrt_1mac;
};

// BLEND is empty (the plain step: no extra kernel argument, no extra instruction) or one DdimBlend
template <typename TX, typename TE, typename... BLEND>
__global__ __launch_bounds__(256) void ddim_step_kernel(const DdimParams p, const BLEND... blend) {
  // x_t [S,Cs,inner] with C = S*Cs rows; eps [2,S,Cs,inner] (0 = conditional, 1 = unconditional); S videos per batch
  const TX* xt = reinterpret_cast<const TX*>(p.xt);
  const TE* ec = reinterpret_cast<const TE*>(p.eps);
  const TE* eu = ec + (size_t)p.C * p.inner;
  TX* out = reinterpret_cast<TX*>(p.out);
  const long total = (long)p.C * p.inner;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx / p.inner);
    const float x = (float)xt[idx];
    const float y = (float)ec[idx];
    float o = y;
    if (c % p.cps < p.guided) {
      const float u = (float)eu[idx];
      o = u + p.gscale * (y - u);
    }
    // same operation order as the reference (all fp32)
    float xn;
    if (p.mode == 0) {                       // DDIM_Gaussian
      const float x0 = p.a_recip * x - p.a_recipm1 * o;
      const float eps = (p.a_recip * x - x0) / p.a_recipm1;
      xn = p.sqrt_aprev * x0 + p.dir_coef * eps;
    } else {                                 // LDM DDIM: a_recip = sqrt(1-a_t), a_recipm1 = sqrt(a_t)
      const float x0 = (x - p.a_recip * o) / p.a_recipm1;
      xn = p.sqrt_aprev * x0 + p.dir_coef * o;
    }
    if (p.noise != nullptr && p.sigma != 0.f) xn += p.sigma * p.noise[idx];
    if constexpr (sizeof...(BLEND) != 0) {     // img_known = q_sample(x0, t'); img = img_known * mask + (1 - mask) * img
      const DdimBlend& b = (blend, ...);
      float known = b.sqrt_ac * b.x0[idx];
      if (b.qnoise != nullptr && b.sqrt_1mac != 0.f) known += b.sqrt_1mac * b.qnoise[idx];
      const float m = b.mask[idx];
      xn = known * m + (1.f - m) * xn;
    }
    out[idx] = (TX)xn;
  }
}

// ---- the strict forms of a record: restrict, threshold, measure, invert (t2v_ddim_classify) ---------------------------------------------
// Kernels of their own, so that the plain step above stays the code it was.  Everything below rounds every operation separately
// (no contraction), like the reference's tensor arithmetic: the x0 that the measure pass ranks IS the x0 that the apply pass thresholds.

// A record on the device: x_t [S,Cs,inner] fp32 with C = S*Cs rows, the eps pair [2,S,Cs,inner] (ec conditional, eu unconditional), out fp32
template <typename TE>
struct DdimView {
  const float* xt; const TE* ec; const TE* eu; float* out;
  long total, per_sample, guided_n;            // elements in all, per sample, and in a sample's first i[2] (guided) channels
  __device__ explicit DdimView(const DdimParams& p)
      : xt(reinterpret_cast<const float*>(p.xt)), ec(reinterpret_cast<const TE*>(p.eps)), eu(ec + (size_t)p.C * p.inner),
        out(reinterpret_cast<float*>(p.out)), total((long)p.C * p.inner), per_sample((long)p.cps * p.inner), guided_n((long)p.guided * p.inner) {}
  __device__ long sample(long idx) const { return idx / per_sample; }
  __device__ bool guided(long within) const { return within < guided_n; }      // within: the element's index inside its sample
};

// The guidance combine e = e_u + g (e_c - e_u) of a guided element: the difference, the product, the sum
__device__ __forceinline__ float ddim_combine(float gscale, float e_c, float e_u) {
#pragma clang fp contract(off)
  const float diff = e_c - e_u;
  const float d = gscale * diff;
  return e_u + d;
}

// FORM: which record's x0 the measure pass ranks and the apply pass thresholds.  0 the DDIM_Gaussian step (mode 0): x0 = f0 x - f1 e,
// *ax_out = f0 x.  1 UniPC's data prediction (mode 2; uni_pc/uni_pc.py:351-364 behind model_wrapper's guidance combine, :304-307):
// x0 = (x - f0 e) / f1 with f0 = sigma_t, f1 = alpha_t.  The unconditional eps is read only where guided.
template <int FORM, typename TE>
__device__ __forceinline__ float ddim_x0_of(const DdimParams& p, const DdimView<TE>& v, long idx, bool guided, float* ax_out) {
#pragma clang fp contract(off)
  const float x = v.xt[idx];
  float e = (float)v.ec[idx];
  if (guided) e = ddim_combine(p.gscale, e, (float)v.eu[idx]);
  if constexpr (FORM == 0) {
    const float ax = p.a_recip * x;
    const float be = p.a_recipm1 * e;
    *ax_out = ax;
    return ax - be;
  } else {
    const float se = p.a_recip * e;
    const float num = x - se;
    return num / p.a_recipm1;
  }
}

// torch.min / torch.max: a NaN in either operand is the result
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }

// The restricted mode-0 step (FORM 0; gaussian_sampler.py:110-120, 199-211) — RESTRICT: 0 none, 1 clamp to [-bound, bound], 2 dynamic
// threshold by table[sample][0]; COND: the classifier-guidance term — and the apply pass of mode 2 (FORM 1, RESTRICT 2): out is the
// thresholded x0 itself, clamp(x0, -s, s) / s.  A NaN in x0 or s is the result; each form keeps torch's operand order of its clamp.
struct DdimRestrict {
  const float* table;   // i[8] = 2: [samples, 4] fp32, s in column 0 (p[7])
  const float* grad;    // i[9] = 1: condition_fn's result, fp32, dense like x (p[8])
  float bound;          // i[8] = 1: clamp bound (f[6])
  float sqrt_1mat;      // i[9] = 1: sqrt(1 - a_t) (f[7])
};

template <typename TE, int FORM, int RESTRICT, bool COND>
__global__ __launch_bounds__(256) void ddim_restrict_kernel(const DdimParams p, const DdimRestrict r) {
#pragma clang fp contract(off)
  const DdimView<TE> v(p);
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < v.total; idx += (long)gridDim.x * 256) {
    const long smp = v.sample(idx);
    float ax = 0.f;
    float x0 = ddim_x0_of<FORM>(p, v, idx, v.guided(idx - smp * v.per_sample), &ax);
    if constexpr (RESTRICT == 1) {
      x0 = nan_min(nan_max(x0, -r.bound), r.bound);                    // torch.clamp: a NaN stays a NaN
    } else if constexpr (RESTRICT == 2) {
      const float s = r.table[smp * 4];
      x0 = (FORM == 0 ? nan_min(s, nan_max(-s, x0)) : nan_min(nan_max(x0, -s), s)) / s;
    }
    if constexpr (FORM == 1) {
      v.out[idx] = x0;
    } else {
      float eps = (ax - x0) / p.a_recipm1;
      if constexpr (COND) {
        const float g = r.sqrt_1mat * r.grad[idx];
        eps = eps - g;
        const float be = p.a_recipm1 * eps;
        x0 = ax - be;
      }
      const float m0 = p.sqrt_aprev * x0, m1 = p.dir_coef * eps;
      float xn = m0 + m1;
      if (p.noise != nullptr && p.sigma != 0.f) {
        const float m2 = p.sigma * p.noise[idx];
        xn = xn + m2;
      }
      v.out[idx] = xn;
    }
  }
}

// ---- mode 3: the DDIM inversion step, DDIMSampler.encode (samplers/ddim/sampler.py:242-254) ---------------------------------------------
// The record is guided as a whole (all channels or none), so no element needs its channel.  out = f0 x + f1 e: both products first,
// then their sum, every operation rounded by itself.
__device__ __forceinline__ float ddim_invert_of(const DdimParams& p, float x, float y, float u, bool guided) {
#pragma clang fp contract(off)
  const float e = guided ? ddim_combine(p.gscale, y, u) : y;
  const float m0 = p.a_recip * x, m1 = p.a_recipm1 * e;
  return m0 + m1;
}

// keep: optional second destination (a kept intermediate), same values.  VEC: four elements per thread with one 128-bit access per fp32
// tensor (64-bit for fp16 eps) — the launcher found every pointer 16-byte aligned; the total % 4 last elements are the scalar work of
// workgroup 0.  !VEC: one element per thread.
template <typename TE, bool GUIDED, bool VEC>
__global__ __launch_bounds__(256) void ddim_invert_kernel(const DdimParams p, float* keep) {
  const DdimView<TE> v(p);                     // v.eu is read only when GUIDED
  const long stride = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
  auto one = [&](long idx) {
    const float u = GUIDED ? (float)v.eu[idx] : 0.f;
    const float o = ddim_invert_of(p, v.xt[idx], (float)v.ec[idx], u, GUIDED);
    v.out[idx] = o;
    if (keep != nullptr) keep[idx] = o;
  };
  if constexpr (VEC) {
    using TE4 = TE __attribute__((ext_vector_type(4)));
    const long nvec = v.total >> 2;
    for (long q = first; q < nvec; q += stride) {
      const f32x4 x = reinterpret_cast<const f32x4*>(v.xt)[q];
      const TE4 y = reinterpret_cast<const TE4*>(v.ec)[q];
      TE4 u = y;
      if constexpr (GUIDED) u = reinterpret_cast<const TE4*>(v.eu)[q];
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = ddim_invert_of(p, x[k], (float)y[k], (float)u[k], GUIDED);
      reinterpret_cast<f32x4*>(v.out)[q] = o;
      if (keep != nullptr) reinterpret_cast<f32x4*>(keep)[q] = o;
    }
    const long tail = (nvec << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4 && tail < v.total) one(tail);
  } else {
    for (long idx = first; idx < v.total; idx += stride) one(idx);
  }
}

// ---- mode 4: the DDIM_Gaussian step with the keyframe blend of the legacy img2vid loop (modelscope/t2v_model.py:1555-1562) -------------
// After the update, elements whose mask weight is <= v are reset to the re-noised original latent: bin = mask <= v ? 0 : 1 (a NaN
// weight compares false: free), known = f6 orig + f7 n, out = known (1 - bin) + x1 bin.
struct DdimKeyframe {
  const float* orig; const float* mask; const float* qnoise;     // p[4..6], fp32 and dense like x; qnoise may be null (f7 == 0)
  float sqrt_ac, sqrt_1mac, v;                                   // f[6], f[7], the fp32 threshold (the bits of i[10])
};

// The update of the plain mode-0 step, so that a free element carries the plain record's bits.  ddim_step_kernel leaves contraction to
// the compiler, and what the compiler fuses depends on the code around an expression (the four-element loop below fused other products
// than the plain kernel): here the operations are pinned — the fused multiply-adds of the plain kernel's mode-0 code written as such
// (the guidance combine, x0, the eta noise), every other operation rounded by itself.  tests/test_gpu_keyframe.py holds the two
// kernels together, bit for bit.  u is read only where guided, n only where the step has eta noise.
__device__ __forceinline__ float ddim_gaussian_of(const DdimParams& p, float x, float y, float u, bool guided, float n, bool noisy) {
#pragma clang fp contract(off)
  float o = y;
  if (guided) o = __builtin_fmaf(p.gscale, y - u, u);
  const float bo = p.a_recipm1 * o, ax = p.a_recip * x;
  const float x0 = __builtin_fmaf(p.a_recip, x, -bo);
  const float eps = (ax - x0) / p.a_recipm1;
  const float m0 = p.sqrt_aprev * x0, m1 = p.dir_coef * eps;
  float xn = m0 + m1;
  if (noisy) xn = __builtin_fmaf(p.sigma, n, xn);
  return xn;
}

// The blend: arithmetic, not a select (a non-finite value on either side propagates as in torch), every operation rounded by itself
__device__ __forceinline__ float ddim_keyframe_of(const DdimKeyframe& k, float x1, float orig, float m, float n, bool has_q) {
#pragma clang fp contract(off)
  const float bin = m <= k.v ? 0.f : 1.f;
  float known = k.sqrt_ac * orig;
  if (has_q) {
    const float qn = k.sqrt_1mac * n;
    known = known + qn;
  }
  const float held = known * (1.f - bin), kept = x1 * bin;
  return held + kept;
}

// VEC: four elements per thread with one 128-bit access per fp32 tensor (64-bit for fp16 eps) — the launcher found every pointer that
// is read 16-byte aligned; the total % 4 last elements are the scalar work of workgroup 0.  !VEC: one element per thread.
template <typename TE, bool VEC>
__global__ __launch_bounds__(256) void ddim_keyframe_kernel(const DdimParams p, const DdimKeyframe k) {
  const DdimView<TE> v(p);
  const bool noisy = p.noise != nullptr && p.sigma != 0.f, has_q = k.qnoise != nullptr, any_guided = p.guided != 0;
  const long stride = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
  auto one = [&](long idx) {
    const bool guided = v.guided(idx % v.per_sample);
    const float y = (float)v.ec[idx];
    const float x1 = ddim_gaussian_of(p, v.xt[idx], y, guided ? (float)v.eu[idx] : y, guided, noisy ? p.noise[idx] : 0.f, noisy);
    v.out[idx] = ddim_keyframe_of(k, x1, k.orig[idx], k.mask[idx], has_q ? k.qnoise[idx] : 0.f, has_q);
  };
  if constexpr (VEC) {
    using TE4 = TE __attribute__((ext_vector_type(4)));
    const long nvec = v.total >> 2;
    for (long q = first; q < nvec; q += stride) {
      const long within = (q << 2) % v.per_sample;     // (a vector may straddle the guided channels' end or a sample's: per element below)
      const f32x4 x = reinterpret_cast<const f32x4*>(v.xt)[q];
      const TE4 y = reinterpret_cast<const TE4*>(v.ec)[q];
      TE4 u = y;
      if (any_guided) u = reinterpret_cast<const TE4*>(v.eu)[q];
      f32x4 n = {0.f, 0.f, 0.f, 0.f}, qn = n;
      if (noisy) n = reinterpret_cast<const f32x4*>(p.noise)[q];
      if (has_q) qn = reinterpret_cast<const f32x4*>(k.qnoise)[q];
      const f32x4 og = reinterpret_cast<const f32x4*>(k.orig)[q];
      const f32x4 m = reinterpret_cast<const f32x4*>(k.mask)[q];
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        long w = within + e;
        if (w >= v.per_sample) w -= v.per_sample;
        const float x1 = ddim_gaussian_of(p, x[e], (float)y[e], (float)u[e], v.guided(w), n[e], noisy);
        o[e] = ddim_keyframe_of(k, x1, og[e], m[e], qn[e], has_q);
      }
      reinterpret_cast<f32x4*>(v.out)[q] = o;
    }
    const long tail = (nvec << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4 && tail < v.total) one(tail);
  } else {
    for (long idx = first; idx < v.total; idx += stride) one(idx);
  }
}

// i[8] = 3, the measure pass: per sample the order statistics lo and hi of |x0| by an exact radix select over the keys' bit patterns
// (|x0| as an unsigned integer orders like the float; a NaN is any key above +inf's), then torch.quantile's interpolation of the two.
// One workgroup of 1024 threads per sample.  Integer counting only: per-wave LDS histograms, summed in a fixed order.
constexpr int QT_THREADS = 1024, QT_WAVES = QT_THREADS / 64, QT_UNROLL = 8;     // keys per thread and trip: their loads are in flight together
struct DdimMeasure {
  float* table;         // [samples, 4]: max(q, 1), q, v_lo, v_hi
  unsigned lo, hi;      // floor / ceil of the fp32 rank f[6] * (float)(n - 1)
  float w;              // rank - lo
};

template <typename TE, int FORM = 0>
__global__ __launch_bounds__(QT_THREADS) void ddim_measure_kernel(const DdimParams p, const DdimMeasure m) {
  __shared__ unsigned hist[QT_WAVES][256];
  __shared__ unsigned total[256];
  __shared__ unsigned sel[4];           // 0 digit, 1 rank inside the digit's bin, 2 count of the bin, 3 smallest key above key_lo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned n = (unsigned)p.cps * (unsigned)p.inner;              // <= 2^24 (validated)
  const long base = (long)blockIdx.x * n;
  const DdimView<TE> v(p);
  const unsigned guided_n = (unsigned)v.guided_n;                      // (below n: the key loops compare in 32 bits)
  auto key_at = [&](unsigned i) -> unsigned {
    float ax;
    return __float_as_uint(ddim_x0_of<FORM>(p, v, base + i, i < guided_n, &ax)) & 0x7fffffffu;     // |x0|: -0.0 is 0
  };

  unsigned prefix = 0, k = m.lo, n_eq = 0;
  bool any_nan = false;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    for (int b = tid; b < QT_WAVES * 256; b += QT_THREADS) (&hist[0][0])[b] = 0;
    __syncthreads();
    for (unsigned i0 = 0; i0 < n; i0 += QT_THREADS * QT_UNROLL) {     // every lane of a wave makes every trip (ballots below)
      unsigned keys[QT_UNROLL];
#pragma unroll
      for (int u = 0; u < QT_UNROLL; ++u) {                            // the loads of one trip are in flight together
        const unsigned i = i0 + u * QT_THREADS + tid;
        keys[u] = i < n ? key_at(i) : 0xffffffffu;                     // (no key is all ones: the sign bit is cleared)
      }
#pragma unroll
      for (int u = 0; u < QT_UNROLL; ++u) {
        const unsigned key = keys[u];
        const bool valid = key != 0xffffffffu;
        if (pass == 0) any_nan |= valid && key > 0x7f800000u;
        bool pending = valid && (key & himask) == prefix;
        const unsigned digit = (key >> shift) & 255u;
        // keys crowd into a few bins (one exponent, a run of ties): the first two distinct digits of a wave are counted by ballot,
        // one add each; what is left goes bin by bin
        for (int round = 0; round < 2; ++round) {
          const unsigned long long live = __ballot(pending);
          if (live == 0) break;
          const int leader = __ffsll((long long)live) - 1;                       // wave-uniform: the lane is read without a trip through LDS
          const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)digit, __builtin_amdgcn_readfirstlane(leader));
          const unsigned long long same = __ballot(pending && digit == d0);
          if (lane == leader) atomicAdd(&hist[wave][d0], (unsigned)__popcll(same));
          pending = pending && digit != d0;
        }
        if (pending) atomicAdd(&hist[wave][digit], 1u);
      }
    }
    __syncthreads();
    if (tid < 256) {
      unsigned t = 0;
      for (int wv = 0; wv < QT_WAVES; ++wv) t += hist[wv][tid];
      total[tid] = t;
    }
    __syncthreads();
    if (tid < 256) {                                                   // the bin that holds rank k: below[tid] <= k < below[tid] + total[tid]
      unsigned below = 0;
      for (int j = 0; j < tid; ++j) below += total[j];
      const unsigned mine = total[tid];
      if (k >= below && k - below < mine) { sel[0] = (unsigned)tid; sel[1] = k - below; sel[2] = mine; }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    k = sel[1];
    n_eq = sel[2];
    __syncthreads();
  }
  // prefix = the key of rank lo; n_eq keys equal it, and lo is the k-th of them (0-based)
  const unsigned key_lo = prefix;
  unsigned key_hi = key_lo;
  const bool need_above = m.hi > m.lo && k + 1 >= n_eq;                // rank hi = lo + 1 lies past the ties at key_lo
  if (tid == 0) sel[3] = 0xffffffffu;
  __syncthreads();
  if (need_above) {                                                    // uniform over the workgroup
    unsigned best = 0xffffffffu;
    for (unsigned i0 = 0; i0 < n; i0 += QT_THREADS * QT_UNROLL) {
      unsigned keys[QT_UNROLL];
#pragma unroll
      for (int u = 0; u < QT_UNROLL; ++u) {
        const unsigned i = i0 + u * QT_THREADS + tid;
        keys[u] = i < n ? key_at(i) : 0xffffffffu;
      }
#pragma unroll
      for (int u = 0; u < QT_UNROLL; ++u)
        if (keys[u] > key_lo && keys[u] < best) best = keys[u];
    }
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)best, off);
      best = o < best ? o : best;
    }
    if (lane == 0) atomicMin(&sel[3], best);
  }
  __syncthreads();
  if (need_above) key_hi = sel[3];
  const int nan_seen = __syncthreads_or(any_nan ? 1 : 0);
  if (tid == 0) {
    const float a = __uint_as_float(key_lo), b = __uint_as_float(key_hi);
    // torch.lerp: w < 0.5 ? a + w (b - a) : b - (b - a)(1 - w), the product and the sum in one rounding as torch's CPU kernel has them
    const float d = b - a;
    float q = m.w < 0.5f ? __fmaf_rn(m.w, d, a) : __fmaf_rn(m.w - 1.f, d, b);
    if (nan_seen) q = __uint_as_float(0x7fc00000u);                    // a NaN anywhere in the sample: torch.quantile gives NaN
    float* row = m.table + (size_t)blockIdx.x * 4;
    row[0] = q != q ? q : fmaxf(q, 1.f);                               // s.clamp_(1.0)
    row[1] = q;
    row[2] = a;
    row[3] = b;
  }
}

struct LinParams {
  const void* t[6];
  void* out;
  float c[6];
  int f32[6];
  int n_terms, out_f32;
  long n;
};

__global__ __launch_bounds__(256) void lincomb_kernel(const LinParams p) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < p.n; idx += (long)gridDim.x * 256) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if (k < p.n_terms) {
        const float v = p.f32[k] ? reinterpret_cast<const float*>(p.t[k])[idx] : (float)reinterpret_cast<const f16*>(p.t[k])[idx];
        acc = k == 0 ? p.c[0] * v : acc + p.c[k] * v;
      }
    }
    if (p.out_f32) reinterpret_cast<float*>(p.out)[idx] = acc;
    else reinterpret_cast<f16*>(p.out)[idx] = (f16)acc;
  }
}

// ---- context windows (T2V_OP_LINCOMB forms i[9] = 2 and 1, include/t2v_hip.h) --------------------------------------------------------------
// Batch row `row` of a windowed forward is window w = row % nW of video v = row / nW: frames starts[w] .. starts[w] + length - 1.  A start is
// clamped into [0, F - length] where it is read, so that no table sends an access outside the clip; a table from ContextWindows.starts is
// never changed by that.
struct WindowGeom {
  const int* starts;     // [nW] int32, ascending
  int V, C, F, HW, length, nW;
};

__device__ __forceinline__ int window_start(const WindowGeom& g, int w) {
  const int s = g.starts[w];
  return min(max(s, 0), g.F - g.length);
}

// Gather: xw[r, c, j, :] = x[v, c, starts[w] + j, :] for the `rows` batch rows from `row0` on, a bit-exact copy.  U is the unit one thread
// moves: uint4 (hw_units = HW * sizeof / 16) on the vector path, the element type (hw_units = HW) on the scalar path.
template <typename U>
__global__ __launch_bounds__(256) void window_gather_kernel(const U* __restrict__ x, U* __restrict__ xw, const WindowGeom g, int row0, int rows,
                                                            int hw_units) {
  const long per_frame = hw_units, per_chan = (long)g.length * per_frame, per_row = (long)g.C * per_chan;
  const long total = (long)rows * per_row;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / per_row, in_row = idx - r * per_row;
    const int c = (int)(in_row / per_chan);
    const long in_chan = in_row - (long)c * per_chan;
    const int j = (int)(in_chan / per_frame), u = (int)(in_chan - (long)j * per_frame);
    const int row = row0 + (int)r, v = row / g.nW, w = row - v * g.nW;
    const int f = window_start(g, w) + j;
    xw[idx] = x[(((long)v * g.C + c) * g.F + f) * per_frame + u];
  }
}

// Blend: out[role, v, c, f, :] = sum_w wgt[f - starts[w]] * e[role, v * nW + w, c, f - starts[w], :] / sum_w wgt[f - starts[w]] over the
// windows that hold frame f, in ascending window order: acc = fma(wgt, e, acc), wsum += wgt, one division.  One thread per output element
// (VEC = 1) or per four neighbours of a frame (VEC = 4, 16-byte stores); no thread shares an output, so nothing depends on the grid.
template <typename TE, int VEC>
__global__ __launch_bounds__(256) void window_blend_kernel(const TE* __restrict__ e, const float* __restrict__ wgt, float* __restrict__ out,
                                                           const WindowGeom g, int roles) {
  const int hw_units = g.HW / VEC;
  const long total = (long)roles * g.V * g.C * g.F * hw_units;
  const long rows_per_role = (long)g.V * g.nW;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int u = (int)(idx % hw_units);
    long rest = idx / hw_units;
    const int f = (int)(rest % g.F); rest /= g.F;
    const int c = (int)(rest % g.C); rest /= g.C;
    const int v = (int)(rest % g.V);
    const int role = (int)(rest / g.V);
    float acc[VEC], wsum = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    for (int w = 0; w < g.nW; ++w) {
      const int j = f - window_start(g, w);
      if (j < 0 || j >= g.length) continue;
      const float wt = wgt[j];
      const TE* src = e + ((((long)role * rows_per_role + (long)v * g.nW + w) * g.C + c) * g.length + j) * g.HW + (long)u * VEC;
      if constexpr (VEC == 4) {
        typedef TE TE4 __attribute__((ext_vector_type(4)));
        const TE4 q = *reinterpret_cast<const TE4*>(src);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = __fmaf_rn(wt, (float)q[k], acc[k]);
      } else {
        acc[0] = __fmaf_rn(wt, (float)src[0], acc[0]);
      }
      wsum += wt;
    }
    float* dst = out + idx * VEC;
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(dst) = make_float4(acc[0] / wsum, acc[1] / wsum, acc[2] / wsum, acc[3] / wsum);
    } else {
      dst[0] = acc[0] / wsum;
    }
  }
}

// Row regrouping between the two layouts of a T-sharded clip (frame-sharded [frames][hw] rows <-> pixel-sharded
// [frames][hw / R] rows): row r of the op reads source row (r / P) * S_src + r % P and writes destination row
// (r / P) * S_dst + r % P (chunks of P rows, chunk strides in rows); optional fp32 residual, indexed like the
// destination, added on the way (the TemporalTransformer's `+ x` after its output is resharded back to frames).
// Round 6: blockIdx.y = part q of `nparts` regroupings of the same shape in ONE launch (the R packs in front of a frames -> pixels
// all-to-all, the R unpacks behind the way back): part q reads src + q * ps_src and writes dst + q * ps_dst (residual + q * ps_res),
// except the rank's own part `own`, whose source (own_is_src) or destination lives elsewhere (`alt`: it does not travel).
template <typename T>
__global__ __launch_bounds__(256) void reshard_rows_kernel(const T* src, T* dst, const float* res, int rows, int cols, int P,
                                                           long s_src, long s_dst, int ld_src, int ld_dst, int ld_res,
                                                           long ps_src, long ps_dst, long ps_res, int own, int own_is_src, T* alt) {
  constexpr int V = 16 / sizeof(T);               // elements per 16-byte unit
  const int q = blockIdx.y;
  src = (q == own && own_is_src) ? alt : src + q * ps_src;
  dst = (q == own && !own_is_src) ? alt : dst + q * ps_dst;
  if (res) res += q * ps_res;
  const int cv = cols / V;
  const long total = (long)rows * cv;
  for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long)gridDim.x * 256) {
    const long r = u / cv;
    const int c = (int)(u - r * cv) * V;
    const long chunk = r / P, within = r - chunk * P;
    const long rs = chunk * s_src + within, rd = chunk * s_dst + within;
    if constexpr (sizeof(T) == 4) {
      f32x4 v = *reinterpret_cast<const f32x4*>(src + rs * ld_src + c);
      if (res) v += *reinterpret_cast<const f32x4*>(res + rd * ld_res + c);
      *reinterpret_cast<f32x4*>(dst + rd * ld_dst + c) = v;
    } else {
      *reinterpret_cast<f16x8*>(dst + rd * ld_dst + c) = *reinterpret_cast<const f16x8*>(src + rs * ld_src + c);
    }
  }
}

// Depth frames [n, 1, H, W] -> PixelUnshuffle(8) tokens [n * (H/8) * (W/8), 64] (channel = (y % 8) * 8 + x % 8), fp16.  One workgroup per
// frame.  NORM: v = 2 * (d - min) / (max - min + 1e-7) - 1 with the frame's own extremes, every operation rounded to fp32 on its own (no
// contraction: the reference evaluates the expression with separate torch ops) — a constant frame maps to exactly -1.  The extremes are
// reduced with wavefront shuffles, then across the workgroup's four waves through LDS; no atomics.  A NaN pixel makes both extremes NaN,
// as torch.amin / amax do (fminf / fmaxf alone would drop it).  A thread converts the 8 pixels of one row of a token and writes them as
// ONE 16-byte store (they are 8 consecutive channels).
template <typename TIN, bool NORM>
__global__ __launch_bounds__(256) void depth_tokens_kernel(const TIN* in, f16* out, int H, int W, int ld) {
  const int hw = H * W, w8 = W >> 3;
  const TIN* src = in + (size_t)blockIdx.x * hw;
  f16* dst = out + (size_t)blockIdx.x * (hw >> 6) * ld;
  float mn = 0.f, den = 1.f;
  if (NORM) {
    float lo = (float)src[0], hi = lo;
    int bad = 0;
    for (int idx = threadIdx.x; idx < hw; idx += 256) {
      const float d = (float)src[idx];
      bad |= d != d;
      lo = fminf(lo, d);
      hi = fmaxf(hi, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, o));
      hi = fmaxf(hi, __shfl_xor(hi, o));
      bad |= __shfl_xor(bad, o);
    }
    __shared__ float s_lo[4], s_hi[4];
    __shared__ int s_bad[4];
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; s_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
    hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
    if (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) lo = hi = __builtin_nanf("");
    mn = lo;
    den = __fadd_rn(__fsub_rn(hi, lo), 1e-7f);
  }
  for (int u = threadIdx.x; u < (hw >> 3); u += 256) {        // unit = 8 consecutive pixels of one image row
    const int y = u / w8, gx = u - y * w8;
    const TIN* s8 = src + (size_t)y * W + gx * 8;
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = (float)s8[e];
      if (NORM) v = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, __fsub_rn(v, mn)), den), 1.f);
      o[e] = (f16)v;
    }
    *reinterpret_cast<f16x8*>(dst + (size_t)((y >> 3) * w8 + gx) * ld + ((y & 7) << 3)) = o;      // ld % 8 == 0 (validated): 16-byte aligned
  }
}

// nn.AvgPool2d(2, 2) of channels-last fp32 tokens: one thread per (output token, 4 channels); the mean is formed in fp32 and only then
// rounded for the fp16 output (the operand of the convolution that follows)
__global__ __launch_bounds__(256) void avgpool2_kernel(const float* in, float* out32, f16* out16, int n, int H, int W, int C, int ld_in,
                                                       int ld32, int ld16) {
  const int Ho = H >> 1, Wo = W >> 1, cv = C >> 2;
  const long total = (long)n * Ho * Wo * cv;
  for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long)gridDim.x * 256) {
    const long tok = u / cv;
    const int c = (int)(u - tok * cv) * 4;
    const int x = (int)(tok % Wo);
    const long r = tok / Wo;
    const int y = (int)(r % Ho);
    const long f = r / Ho;
    const float* s0 = in + ((f * H + 2 * y) * W + 2 * x) * ld_in + c;
    const float* s1 = s0 + (size_t)W * ld_in;
    const f32x4 a = *reinterpret_cast<const f32x4*>(s0), b = *reinterpret_cast<const f32x4*>(s0 + ld_in);
    const f32x4 d = *reinterpret_cast<const f32x4*>(s1), e = *reinterpret_cast<const f32x4*>(s1 + ld_in);
    const f32x4 v = ((a + b) + (d + e)) * 0.25f;
    if (out32) *reinterpret_cast<f32x4*>(out32 + tok * ld32 + c) = v;
    if (out16) *reinterpret_cast<f16x4*>(out16 + tok * ld16 + c) = f16x4{(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
  }
}

// Prompt emphasis with mean restoration (clip_hardcode.py:413-420): out = (z * m[row]) * (sum z / sum (z * m[row])), both sums over the WHOLE
// tensor (the reference's z.mean() of a batch of chunks).  ONE workgroup of 1024 threads, two passes over z: every thread adds its
// elements (index = thread + k * 1024 groups of 4, ascending k) into fp64 partials, the partials meet in a fixed LDS tree — the same
// order on every run, so results repeat bit for bit; with every multiplier 1.0 the two sums are the same sequence of additions and
// the ratio is exactly 1.  A zero sum of z * m gives what IEEE gives (inf / NaN), as the reference.
template <typename TZ>
__global__ __launch_bounds__(1024) void emphasis_kernel(const TZ* z, const float* mult, float* out, int rows, int W, int ldz, int ldo) {
  __shared__ double red[2][1024];
  const int cv = W >> 2, t = threadIdx.x;
  const long total = (long)rows * cv;
  double s_z = 0.0, s_zm = 0.0;
  for (long u = t; u < total; u += 1024) {
    const long r = u / cv;
    const int c = (int)(u - r * cv) * 4;
    const TZ* s = z + r * ldz + c;
    const double m = (double)mult[r];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double v = (double)(float)s[e];
      s_z += v;
      s_zm += v * m;
    }
  }
  red[0][t] = s_z;
  red[1][t] = s_zm;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (t < w) {
      red[0][t] += red[0][t + w];
      red[1][t] += red[1][t + w];
    }
    __syncthreads();
  }
  const float ratio = (float)(red[0][0] / red[1][0]);
  for (long u = t; u < total; u += 1024) {
    const long r = u / cv;
    const int c = (int)(u - r * cv) * 4;
    const TZ* s = z + r * ldz + c;
    const float m = mult[r];
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float zm = (float)s[e] * m;
      v[e] = zm * ratio;
    }
    *reinterpret_cast<f32x4*>(out + r * ldo + c) = v;
  }
}

// Fingerprint of byte ranges (T2V_OP_FINGERPRINT): one 64-bit value per segment {address, nbytes} of a table, a function of the segment's
// bytes and of nothing else.  A segment is read as n = nbytes / 2 little-endian 16-bit words v_0 .. v_{n-1} (address and nbytes even):
//     value = sum_j v_j * (2 j + 1)  +  2^32 * sum_j v_j^2  +  (n + 1) * T2V_FINGERPRINT_LEN      (mod 2^64)
// Word j contributes f(v, j) = v * ((2 j + 1) + 2^32 v): f(a, j) - f(b, j) = (a - b) * (odd number), which is 0 mod 2^64 only for a = b, so
// ONE changed word always changes the value; two unequal words a, b swapped between j and k move it by 2 (a - b)(j - k) != 0; the last
// term separates equal bytes of different lengths (trailing zero words add nothing to the sums).  Integer wrap-around adds only: the
// order of the fold is free, the value does not depend on the grid or on the run.
// One workgroup per chunk {segment, chunk index} of the host's chunk table (T2V_FINGERPRINT_CHUNK bytes of ONE segment; every segment has
// a chunk 0, an empty one too, which adds the length term): 16-byte loads on the part of the chunk between 16-byte boundaries of the
// ADDRESS, single words in front of and behind it, so the start may sit at any even address; per 16-byte vector at word j0 the sum is
// (2 j0 + 1) * sum v_i + 2 * sum i v_i (v_dot2_u32_u16 on the packed words, no unpacking).  One 64-bit atomic add per workgroup into
// out[segment], which the launcher zeroed on the same stream.  Nothing else is written.
struct FpSeg { unsigned long long addr, nbytes; };

__global__ __launch_bounds__(256) void fingerprint_kernel(const FpSeg* segs, const uint2* chunks, unsigned long long* out, int n) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  typedef unsigned long long u64;
  __shared__ u64 red[256];
  const int t = threadIdx.x;
  const uint2 ck = chunks[blockIdx.x];
  if (ck.x >= (unsigned)n) return;
  const FpSeg sg = segs[ck.x];
  if ((sg.addr | sg.nbytes) & 1ull) return;                       // (the host refuses odd ranges; never read one)
  const u64 b0 = (u64)ck.y * T2V_FINGERPRINT_CHUNK;
  u64 lin = 0;         // sum v_j (2 j + 1)
  unsigned sq = 0;     // sum v_j^2 mod 2^32 (it enters shifted left by 32)
  if (b0 < sg.nbytes) {
    const u64 b1 = b0 + T2V_FINGERPRINT_CHUNK < sg.nbytes ? b0 + T2V_FINGERPRINT_CHUNK : sg.nbytes;
    const u64 p0 = sg.addr + b0, p1 = sg.addr + b1;
    u64 a0 = (p0 + 15) & ~15ull;                                  // the 16-byte aligned interior [a0, a1) of [p0, p1)
    if (a0 > p1) a0 = p1;
    u64 a1 = p1 & ~15ull;
    if (a1 < a0) a1 = a0;
    const int head = (int)((a0 - p0) >> 1), tail = (int)((p1 - a1) >> 1);        // <= 7 words each
    if (t < head + tail) {
      const u64 at = t < head ? p0 + 2 * (u64)t : a1 + 2 * (u64)(t - head);
      const unsigned v = *reinterpret_cast<const unsigned short*>(at);
      lin += (u64)v * (((at - sg.addr) >> 1) * 2 + 1);
      sq += v * v;
    }
    const long nvec = (long)((a1 - a0) >> 4);
    const u16x2 ones = __builtin_bit_cast(u16x2, 0x00010001u);
    for (long q = t; q < nvec; q += 256) {
      const u64 at = a0 + 16 * (u64)q;
      const uint4 w = *reinterpret_cast<const uint4*>(at);
      const u16x2 w0 = __builtin_bit_cast(u16x2, w.x), w1 = __builtin_bit_cast(u16x2, w.y);
      const u16x2 w2 = __builtin_bit_cast(u16x2, w.z), w3 = __builtin_bit_cast(u16x2, w.w);
      unsigned s = __builtin_amdgcn_udot2(w0, ones, 0u, false);                  // sum v_i        < 2^19
      s = __builtin_amdgcn_udot2(w1, ones, s, false);
      s = __builtin_amdgcn_udot2(w2, ones, s, false);
      s = __builtin_amdgcn_udot2(w3, ones, s, false);
      unsigned m = __builtin_amdgcn_udot2(w0, __builtin_bit_cast(u16x2, 0x00010000u), 0u, false);   // sum i v_i, i = 0 .. 7   < 2^21
      m = __builtin_amdgcn_udot2(w1, __builtin_bit_cast(u16x2, 0x00030002u), m, false);
      m = __builtin_amdgcn_udot2(w2, __builtin_bit_cast(u16x2, 0x00050004u), m, false);
      m = __builtin_amdgcn_udot2(w3, __builtin_bit_cast(u16x2, 0x00070006u), m, false);
      sq = __builtin_amdgcn_udot2(w0, w0, sq, false);
      sq = __builtin_amdgcn_udot2(w1, w1, sq, false);
      sq = __builtin_amdgcn_udot2(w2, w2, sq, false);
      sq = __builtin_amdgcn_udot2(w3, w3, sq, false);
      lin += (((at - sg.addr) >> 1) * 2 + 1) * (u64)s + 2 * (u64)m;
    }
  }
  u64 acc = lin + ((u64)sq << 32);
  if (ck.y == 0 && t == 0) acc += ((sg.nbytes >> 1) + 1) * T2V_FINGERPRINT_LEN;
  red[t] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) atomicAdd(out + ck.x, red[0]);
}

// Stable LoRA merge (T2V_OP_LORA_MERGE; stable_lora/stable_utils/lora_processor.py:50-101): W += alpha * (B A) for every weight of a table, in
// place, one launch.  The contract per element, every step rounded once to the weight's type T (include/t2v_hip.h):
//     d = T(sum over ascending k of B[n,k] A[k,j'])  (fp32 accumulation; fp16 products are exact in fp32, so the FMA below adds no rounding of its own)
//     temporal form (Conv3d [o, i, 3, 1, 1], A of 3 J columns):  d = T((d(3j) + d(3j+1) + d(3j+2)) / 3), fp32, that order, IEEE division
//     e = T(d * alpha);   W = T(W + e)
// which is bit for bit what the reference's `(lora_B @ lora_A).view(...)`, `torch.mean`, `* alpha` and `+=` give on fp16 tensors.  The products of
// the last two lines are written with the _rn intrinsics and fenced (lora_f32): the compiler may neither contract them into one FMA (for
// T = float nothing else would separate them) nor fold an fp32 step into the conversion to fp16 that follows it.
// One workgroup per tile {segment, tile index} of the host's tile table: T2V_LORA_TILE consecutive elements of ONE weight (flat, row-major).
// Like the fingerprint: 16-byte accesses of W between 16-byte boundaries of the ADDRESS, single elements in front of and behind them, so a
// weight may start anywhere and end anywhere; nothing outside [W + t0, W + t1) is touched.  Per vector of one row, A's row k is read as one
// 16-byte load where its address allows (lanes side by side: coalesced), B[n, k] once per vector; a vector that runs over a row end, and
// factors at odd addresses, take the element path.  The loops over k are unrolled by 4: the loads of four rows of A are in flight together;
// the sums stay in ascending k.  Measured (profiles/stable_lora.txt): 3.4 ms for the full UNet at rank 16, bound by the r rows of A that every
// element of a one-row run re-reads through the vector L1, not by HBM and not by latency (one row per wait: 3.5 ms).
struct LoraSeg { unsigned long long w, a, b; int N, J, r, form, dtype, pad; };
template <typename T> struct LoraVec;
template <> struct LoraVec<f16> { typedef f16x8 type; };
template <> struct LoraVec<float> { typedef f32x4 type; };

// An fp32 result that the contract rounds to fp32 BEFORE it is rounded to T.  Without the fence the compiler selects v_fma_mixlo_f16 for
// `(f16)(d * alpha)` (and may for the last FMA of a sum), which rounds the exact product ONCE to fp16: measured on the device, 1.9 % of the
// products with alpha = 0.7 come out one fp16 ulp away from the reference's `tensor * alpha` (fp32 product, then fp16), which shows in W where
// W + e cancels.  The empty statement keeps the value in a VGPR as an fp32 number; it costs no instruction.
__device__ __forceinline__ float lora_f32(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// d = T(s) of an fp32 sum, as an fp32 number
template <typename T>
__device__ __forceinline__ float lora_round(float s) { return (float)(T)lora_f32(s); }

template <typename T>
__device__ __forceinline__ T lora_apply(T w, float d, float alpha) {
  const float e = lora_round<T>(__fmul_rn(d, alpha));
  return (T)lora_f32(__fadd_rn((float)w, e));
}

template <typename T>
__device__ __forceinline__ float lora_mean3(float s0, float s1, float s2) {
  const float d0 = lora_round<T>(s0), d1 = lora_round<T>(s1), d2 = lora_round<T>(s2);
  return lora_round<T>(__fdiv_rn(lora_f32(__fadd_rn(lora_f32(__fadd_rn(d0, d1)), d2)), 3.0f));
}

// d of one element (n, j): b = row n of B
template <typename T>
__device__ float lora_delta(const T* A, const T* b, long Jf, int r, int form, long j) {
  if (form == T2V_LORA_DIRECT) {
    const T* a = A + j;
    float s = 0.f;
#pragma unroll 4
    for (int k = 0; k < r; ++k) s = fmaf((float)b[k], (float)a[(long)k * Jf], s);
    return lora_round<T>(s);
  }
  const T* a = A + 3 * j;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll 4
  for (int k = 0; k < r; ++k) {
    const float bk = (float)b[k];
    const T* ak = a + (long)k * Jf;
    s0 = fmaf(bk, (float)ak[0], s0);
    s1 = fmaf(bk, (float)ak[1], s1);
    s2 = fmaf(bk, (float)ak[2], s2);
  }
  return lora_mean3<T>(s0, s1, s2);
}

template <typename T>
__device__ void lora_merge_tile(const LoraSeg& sg, unsigned tile, float alpha, int t) {
  typedef unsigned long long u64;
  typedef typename LoraVec<T>::type vec;
  constexpr int V = 16 / (int)sizeof(T);
  if ((sg.w | sg.a | sg.b) % sizeof(T) != 0) return;               // (the host refuses addresses that are not element-aligned; never touch one)
  const u64 total = (u64)sg.N * (u64)sg.J;
  const u64 t0 = (u64)tile * T2V_LORA_TILE;
  if (t0 >= total) return;
  const u64 t1 = t0 + T2V_LORA_TILE < total ? t0 + T2V_LORA_TILE : total;
  T* W = reinterpret_cast<T*>(sg.w);
  const T* A = reinterpret_cast<const T*>(sg.a);
  const T* B = reinterpret_cast<const T*>(sg.b);
  const int r = sg.r, form = sg.form;
  const long J = sg.J, Jf = form == T2V_LORA_TEMPORAL ? 3 * J : J;
  const u64 p0 = sg.w + t0 * sizeof(T), p1 = sg.w + t1 * sizeof(T);
  u64 a0 = (p0 + 15) & ~15ull;                                     // the 16-byte aligned interior [a0, a1) of [p0, p1)
  if (a0 > p1) a0 = p1;
  const u64 a1 = a0 + ((p1 - a0) & ~15ull);
  const int head = (int)((a0 - p0) / sizeof(T)), tail = (int)((p1 - a1) / sizeof(T));     // < V elements each
  if (t < head + tail) {
    const u64 e = t < head ? t0 + (u64)t : t1 - (u64)tail + (u64)(t - head);
    const u64 n = e / (u64)J;
    const float d = lora_delta<T>(A, B + n * (u64)r, Jf, r, form, (long)(e - n * (u64)J));
    W[e] = lora_apply<T>(W[e], d, alpha);
  }
  const u64 e_first = t0 + (u64)head;
  const long nvec = (long)((a1 - a0) >> 4);
  const bool rows_aligned = ((u64)Jf * sizeof(T)) % 16 == 0;       // every row of A starts at the same offset from a 16-byte boundary
  for (long q = t; q < nvec; q += 256) {
    const u64 e = e_first + (u64)q * V;
    u64 n = e / (u64)J;
    long j = (long)(e - n * (u64)J);
    vec w = *reinterpret_cast<const vec*>(W + e);
    if (j + V <= J) {                                              // V elements of one row
      const T* b = B + n * (u64)r;
      if (form == T2V_LORA_DIRECT) {
        const T* a = A + j;
        float s[V];
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] = 0.f;
        if (rows_aligned && (u64)a % 16 == 0) {
#pragma unroll 4
          for (int k = 0; k < r; ++k) {
            const float bk = (float)b[k];
            const vec av = *reinterpret_cast<const vec*>(a + (long)k * Jf);
#pragma unroll
            for (int i = 0; i < V; ++i) s[i] = fmaf(bk, (float)av[i], s[i]);
          }
        } else {
#pragma unroll 4
          for (int k = 0; k < r; ++k) {
            const float bk = (float)b[k];
            const T* ak = a + (long)k * Jf;
#pragma unroll
            for (int i = 0; i < V; ++i) s[i] = fmaf(bk, (float)ak[i], s[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) w[i] = lora_apply<T>(w[i], lora_round<T>(s[i]), alpha);
      } else {
        const T* a = A + 3 * j;
        float s[3 * V];
#pragma unroll
        for (int i = 0; i < 3 * V; ++i) s[i] = 0.f;
        if (rows_aligned && (u64)a % 16 == 0) {
#pragma unroll 4
          for (int k = 0; k < r; ++k) {
            const float bk = (float)b[k];
            const vec* ak = reinterpret_cast<const vec*>(a + (long)k * Jf);
            const vec v0 = ak[0], v1 = ak[1], v2 = ak[2];
#pragma unroll
            for (int i = 0; i < V; ++i) {
              s[i] = fmaf(bk, (float)v0[i], s[i]);
              s[V + i] = fmaf(bk, (float)v1[i], s[V + i]);
              s[2 * V + i] = fmaf(bk, (float)v2[i], s[2 * V + i]);
            }
          }
        } else {
#pragma unroll 4
          for (int k = 0; k < r; ++k) {
            const float bk = (float)b[k];
            const T* ak = a + (long)k * Jf;
#pragma unroll
            for (int i = 0; i < 3 * V; ++i) s[i] = fmaf(bk, (float)ak[i], s[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) w[i] = lora_apply<T>(w[i], lora_mean3<T>(s[3 * i], s[3 * i + 1], s[3 * i + 2]), alpha);
      }
    } else {                                                       // the vector runs over a row end: element by element
#pragma unroll
      for (int i = 0; i < V; ++i) {
        w[i] = lora_apply<T>(w[i], lora_delta<T>(A, B + n * (u64)r, Jf, r, form, j), alpha);
        if (++j == J) { j = 0; ++n; }
      }
    }
    *reinterpret_cast<vec*>(W + e) = w;
  }
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraSeg* segs, const uint2* tiles, int n, float alpha) {
  const uint2 tl = tiles[blockIdx.x];
  if (tl.x >= (unsigned)n) return;
  const LoraSeg sg = segs[tl.x];
  if (sg.N <= 0 || sg.J <= 0 || sg.r <= 0 || sg.w == 0 || sg.a == 0 || sg.b == 0) return;      // (the host builds none of these)
  if (sg.form != T2V_LORA_DIRECT && sg.form != T2V_LORA_TEMPORAL) return;
  if (sg.dtype == T2V_F16) lora_merge_tile<f16>(sg, tl.y, alpha, threadIdx.x);
  else if (sg.dtype == T2V_F32) lora_merge_tile<float>(sg, tl.y, alpha, threadIdx.x);
}

// tensor2vid (t2v_pipeline.py:447-460): video[i,c,f,y,x] -> uint8 out[f, y, i*W + x, c]: v*0.5 + 0.5 (two roundings, as
// mul_ / add_), clamp to [0,1], *255, TRUNCATED like `(image.numpy()*255).astype('uint8')`.  HALF: the reference's
// 'GPU (half precision)' VAE hands tensor2vid an fp16 video, so every intermediate is rounded to fp16 (the input too
// when the tokens are fp32).  Input addressed by element strides: channels-last decoder tokens or a plain NCFHW tensor.
template <typename TIN, bool HALF>
__global__ __launch_bounds__(256) void to_uint8_kernel(const TIN* in, unsigned char* out, int NI, int C, int F, int H, int W,
                                                       long si, long sc, long sf, long sy, long sx, int bgr) {
  const long total = (long)F * H * NI * W;
  for (long px = (long)blockIdx.x * 256 + threadIdx.x; px < total; px += (long)gridDim.x * 256) {
    const int xw = (int)(px % ((long)NI * W));
    long r = px / ((long)NI * W);
    const int y = (int)(r % H);
    const int f = (int)(r / H);
    const int i = xw / W, x = xw - i * W;
    const TIN* src = in + i * si + f * sf + y * sy + x * sx;
    unsigned char* o = out + px * C;
    for (int c = 0; c < C; ++c) {
      float v = (float)src[c * sc];
      if (HALF) {
        f16 h = (f16)v;
        h = (f16)__fmul_rn((float)h, 0.5f);
        h = (f16)__fadd_rn((float)h, 0.5f);
        h = h < (f16)0.f ? (f16)0.f : (h > (f16)1.f ? (f16)1.f : h);
        v = (float)(f16)__fmul_rn((float)h, 255.f);
      } else {
        v = __fadd_rn(__fmul_rn(v, 0.5f), 0.5f);
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        v = __fmul_rn(v, 255.f);
      }
      o[bgr ? C - 1 - c : c] = (unsigned char)(int)v;
    }
  }
}

// torch_to_np (videocrafter/sample_utils.py:98-107), form 1 of T2V_OP_TO_UINT8: video[i,c,f,y,x] -> uint8 out[i, f, y, x, c] (one
// [F,H,W,C] block per video): a = x + 1, b = a * 127.5 (each rounded by itself in fp32, never an fma), clamp to [0, 255] (+-inf -> 0 | 255),
// TRUNCATED like `.to(torch.uint8)`; a NaN stores 0.  HALF: the input element is rounded to fp16 first (the fp16 model's video), the
// arithmetic stays fp32 — torch_to_np's `.float()` — unlike tensor2vid's fp16 chain above.  Same input addressing and pixel mapping.
template <typename TIN, bool HALF>
__global__ __launch_bounds__(256) void to_uint8_np_kernel(const TIN* in, unsigned char* out, int NI, int C, int F, int H, int W,
                                                          long si, long sc, long sf, long sy, long sx) {
  const long total = (long)NI * F * H * W;
  for (long px = (long)blockIdx.x * 256 + threadIdx.x; px < total; px += (long)gridDim.x * 256) {
    const int x = (int)(px % W);
    long r = px / W;
    const int y = (int)(r % H);
    r /= H;
    const int f = (int)(r % F);
    const int i = (int)(r / F);
    const TIN* src = in + i * si + f * sf + y * sy + x * sx;
    unsigned char* o = out + px * C;
    for (int c = 0; c < C; ++c) {
      float v = (float)src[c * sc];
      if (HALF) v = (float)(f16)v;
      v = __fmul_rn(__fadd_rn(v, 1.f), 127.5f);
      v = !(v > 0.f) ? 0.f : (v > 255.f ? 255.f : v);        // (a NaN fails `v > 0`)
      o[c] = (unsigned char)(int)v;
    }
  }
}

// Separable table-driven resampler for uint8 [N, H, W, 3] images (T2V_OP_RESAMPLE): ONE pass of Pillow's 8-bit resize
// (Resample.c, PRECISION_BITS = 22) — the Lanczos resize of process_modelscope.py:116-120,174-178 is a horizontal pass into a
// uint8 intermediate followed by a vertical one.  Per output index o with table row k[0..ksize) and bounds {first, count}:
//   acc = 2^21 + sum_j src[first + j] * k[j]  (int32),  result = clamp(acc >> 22, 0, 255)  (arithmetic shift).
// FORM 0 stores the byte; FORM 1 / 2 (the last pass in front of the VAE encoder) store lut[byte] as fp32 / fp16 channels-last
// tokens of `ld` channels, the channels beyond 3 zeroed — the encoder's entry buffer, so no float image ever exists.
// Bounds are clamped to the source axis before use: a malformed table gives wrong pixels, never a read outside the image.
constexpr int RS_LDS_BYTES = 32768;

__device__ __forceinline__ void rs_bounds(const int* bounds, int o, int in_size, int ksize, int& first, int& count) {
  first = bounds[2 * o];
  first = first < 0 ? 0 : (first > in_size ? in_size : first);
  const int room = in_size - first;
  count = bounds[2 * o + 1];
  count = count < 0 ? 0 : (count > ksize ? ksize : count);
  count = count > room ? room : count;
}

__device__ __forceinline__ int rs_clip8(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// one store unit: FORM 0 = 4 consecutive bytes of the output row (one dword store where the address allows; the tail of a row and
// unaligned rows go byte by byte), FORM 1 / 2 = one pixel (3 bytes -> one token row of ld floats / halfs)
template <int FORM>
__device__ __forceinline__ void rs_store(void* dst_row, int e0, int row_bytes, const int (&v)[4], const float* lut, int ld) {
  if constexpr (FORM == 0) {
    unsigned char* d = reinterpret_cast<unsigned char*>(dst_row) + e0;
    if (e0 + 4 <= row_bytes && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(d) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
      for (int q = 0; q < 4 && e0 + q < row_bytes; ++q) d[q] = (unsigned char)v[q];
    }
  } else if constexpr (FORM == 1) {
    float* d = reinterpret_cast<float*>(dst_row) + (size_t)(e0 / 3) * ld;
    for (int c = 0; c < ld; ++c) d[c] = c < 3 ? lut[v[c]] : 0.f;
  } else {
    f16* d = reinterpret_cast<f16*>(dst_row) + (size_t)(e0 / 3) * ld;
    if (ld == 8 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {          // the encoder's 8-channel token row: one 16-byte store
      f16x8 t = {(f16)lut[v[0]], (f16)lut[v[1]], (f16)lut[v[2]], (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
      *reinterpret_cast<f16x8*>(d) = t;
    } else {
      for (int c = 0; c < ld; ++c) d[c] = c < 3 ? (f16)lut[v[c]] : (f16)0.f;
    }
  }
}

// Horizontal pass: a workgroup owns 256 units of ONE source row — a unit is 4 consecutive output pixels (12 bytes, three dword
// stores) for FORM 0 and one pixel (one token row) for FORM 1 / 2; a pixel's bounds and table row are read once for its three
// channels.  The source span those outputs read is staged in LDS with 16-byte loads (LDS offset congruent to the global address
// mod 16) when it fits, else the taps come from global memory.
template <int FORM>
__global__ __launch_bounds__(256) void resample_h_kernel(const unsigned char* src, void* dst, const int* coef, const int* bounds,
                                                         const float* lut, int W, int Wout, int ksize, int ld, int tiles) {
  constexpr int PX = FORM == 0 ? 4 : 1;                 // output pixels per unit
  __shared__ __attribute__((aligned(16))) unsigned char smem[RS_LDS_BYTES];
  __shared__ int s_lo, s_hi;
  const long row = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - row * tiles);
  const int row_bytes = Wout * 3;
  const unsigned char* srow = src + row * (long)W * 3;
  const int x_first = tile * 256 * PX;
  int x_end = x_first + 256 * PX;
  x_end = x_end > Wout ? Wout : x_end;
  if (threadIdx.x == 0) { s_lo = W; s_hi = 0; }
  __syncthreads();
  for (int x = x_first + (int)threadIdx.x; x < x_end; x += 256) {
    int first, count;
    rs_bounds(bounds, x, W, ksize, first, count);
    if (count > 0) { atomicMin(&s_lo, first); atomicMax(&s_hi, first + count); }
  }
  __syncthreads();
  const int lo = s_lo, span = (s_hi - s_lo) * 3;        // bytes [lo * 3, lo * 3 + span) of the source row
  const unsigned char* g = srow + (long)lo * 3;
  const int pad = (int)(reinterpret_cast<uintptr_t>(g) & 15);
  const bool staged = span > 0 && pad + span <= RS_LDS_BYTES;
  if (staged) {
    int head = (16 - pad) & 15;
    head = head > span ? span : head;
    const int nvec = (span - head) >> 4, tail0 = head + (nvec << 4);
    for (int b = threadIdx.x; b < head; b += 256) smem[pad + b] = g[b];
    for (int q = threadIdx.x; q < nvec; q += 256)
      *reinterpret_cast<uint4*>(smem + pad + head + (q << 4)) = *reinterpret_cast<const uint4*>(g + head + (q << 4));
    for (int b = tail0 + threadIdx.x; b < span; b += 256) smem[pad + b] = g[b];
    __syncthreads();
  }
  const int x0 = x_first + (int)threadIdx.x * PX;
  if (x0 >= Wout) return;
  int v[PX * 3 + (FORM == 0 ? 0 : 1)] = {};
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    const int x = x0 + p;
    if (x < Wout) {
      int first, count;
      rs_bounds(bounds, x, W, ksize, first, count);
      const int* k = coef + (long)x * ksize;
      const unsigned char* s = staged ? smem + pad + (first - lo) * 3 : srow + (long)first * 3;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int j = 0; j < count; ++j, s += 3) {
        const int kj = k[j];
        a0 += (int)s[0] * kj; a1 += (int)s[1] * kj; a2 += (int)s[2] * kj;
      }
      v[p * 3] = rs_clip8(a0); v[p * 3 + 1] = rs_clip8(a1); v[p * 3 + 2] = rs_clip8(a2);
    }
  }
  char* drow = reinterpret_cast<char*>(dst) + row * (long)Wout * (FORM == 0 ? 3 : (FORM == 1 ? 4 : 2) * ld);
  if constexpr (FORM == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int u[4] = {v[q * 4], v[q * 4 + 1], v[q * 4 + 2], v[q * 4 + 3]};
      if (x0 * 3 + q * 4 < row_bytes) rs_store<0>(drow, x0 * 3 + q * 4, row_bytes, u, lut, ld);
    }
  } else {
    rs_store<FORM>(drow, x0 * 3, row_bytes, v, lut, ld);
  }
}

// Vertical pass: a workgroup owns 256 units of ONE output row; every tap is a coalesced read of the same bytes of a source row
// (dword loads where the address allows), the table row and bounds are uniform over the workgroup.
template <int FORM>
__global__ __launch_bounds__(256) void resample_v_kernel(const unsigned char* src, void* dst, const int* coef, const int* bounds,
                                                         const float* lut, int H, int W, int Hout, int ksize, int ld, int tiles) {
  constexpr int UB = FORM == 0 ? 4 : 3;
  const long orow = blockIdx.x / tiles;                 // image * Hout + y
  const int tile = (int)(blockIdx.x - orow * tiles);
  const long img = orow / Hout;
  const int y = (int)(orow - img * Hout);
  const int row_bytes = W * 3;
  const int e0 = (tile * 256 + (int)threadIdx.x) * UB;
  if (e0 >= row_bytes) return;
  int first, count;
  rs_bounds(bounds, y, H, ksize, first, count);
  const int* k = coef + (long)y * ksize;
  const unsigned char* s = src + (img * H + first) * (long)row_bytes + e0;
  int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
  const bool whole = e0 + UB <= row_bytes;
  for (int j = 0; j < count; ++j, s += row_bytes) {
    const int kj = k[j];
    if (FORM == 0 && whole && (reinterpret_cast<uintptr_t>(s) & 3) == 0) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(s);
      acc[0] += (int)(u & 255u) * kj; acc[1] += (int)((u >> 8) & 255u) * kj;
      acc[2] += (int)((u >> 16) & 255u) * kj; acc[3] += (int)(u >> 24) * kj;
    } else {
#pragma unroll
      for (int q = 0; q < UB; ++q)
        if (e0 + q < row_bytes) acc[q] += (int)s[q] * kj;
    }
  }
  int v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = rs_clip8(acc[q]);
  char* drow = reinterpret_cast<char*>(dst) + orow * (long)W * (FORM == 0 ? 3 : (FORM == 1 ? 4 : 2) * ld);
  rs_store<FORM>(drow, e0, row_bytes, v, lut, ld);
}

// Float bicubic resize (T2V_OP_RESAMPLE with i[9] = 1): P planar single-channel images [P, H, W] (fp16 | fp32) -> fp32 [P, Ho, Wo], both
// axes in one launch, with torch's upsample_bicubic2d semantics (align_corners = False, no antialiasing) carried by host-built tables
// (packing.bicubic_table): per output row y four weights wy / source rows iy, per output column x four weights wx / source columns ix.
//   out = sum_{a = 0..3} wy[a] * ( sum_{b = 0..3} wx[b] * fp32(src[iy[a]][ix[b]]) )
// both sums in ascending order from the first product, every multiply and add rounded to fp32 on its own (no contraction): the bits do
// not depend on the grid or the compiler, and tests/interp_bicubic.py reproduces them with numpy.  Nothing is special-cased for NaN / inf
// (0 * NaN is NaN, as in torch).  The indices are clamped to the image again before use: a malformed table gives wrong pixels, never a
// read outside the source.  A workgroup owns 256 consecutive columns of ONE output row (row weights and indices are uniform, the stores
// coalesced); the four source rows are shared by neighbouring columns and rows through the cache.
__device__ __forceinline__ int bc_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }
// hipcc contracts a * b + c into one fused multiply-add by default, and to it __fmul_rn / __fadd_rn are the plain operators (they
// only keep a product apart where no sum follows it directly): here a sum follows every product, so the two operations are written
// under `fp contract(off)`, which the compiler's default contraction mode honours.
__device__ __forceinline__ float bc_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float bc_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <typename TIN>
__global__ __launch_bounds__(256) void bicubic_kernel(const TIN* src, float* dst, const float* wgt, const int* idx, int H, int W, int Ho,
                                                      int Wo, int tiles) {
  const long orow = blockIdx.x / tiles;                 // plane * Ho + y
  const int x = (int)(blockIdx.x - orow * tiles) * 256 + (int)threadIdx.x;
  if (x >= Wo) return;
  const long plane = orow / Ho;
  const int y = (int)(orow - plane * Ho);
  const float* wy = wgt + 4 * (long)y;
  const int* iy = idx + 4 * (long)y;
  const float* wx = wgt + 4 * ((long)Ho + x);
  const int* ix = idx + 4 * ((long)Ho + x);
  const float wx0 = wx[0], wx1 = wx[1], wx2 = wx[2], wx3 = wx[3];
  const int c0 = bc_clamp(ix[0], W), c1 = bc_clamp(ix[1], W), c2 = bc_clamp(ix[2], W), c3 = bc_clamp(ix[3], W);
  const TIN* img = src + plane * (long)H * W;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const TIN* row = img + (long)bc_clamp(iy[a], H) * W;
    float h = bc_mul(wx0, (float)row[c0]);
    h = bc_add(h, bc_mul(wx1, (float)row[c1]));
    h = bc_add(h, bc_mul(wx2, (float)row[c2]));
    h = bc_add(h, bc_mul(wx3, (float)row[c3]));
    const float t = bc_mul(wy[a], h);
    acc = a == 0 ? t : bc_add(acc, t);
  }
  dst[orow * Wo + x] = acc;
}

inline int grid_for(long n) {
  const long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// A run-time dtype tag, flag or small index as a compile-time argument of a generic lambda: f gets a value of the element type
// (`using T = decltype(t)`), a std::bool_constant, or a std::integral_constant below N (the last one for anything at or beyond it)
template <typename F> void by_dtype(int dtype, F&& f) { if (dtype == T2V_F32) f(float()); else f(f16()); }
template <typename F> void by_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <int N, typename F> void by_index(int i, F&& f) {
  if constexpr (N > 1) { if (i < N - 1) return by_index<N - 1>(i, f); }
  f(std::integral_constant<int, N - 1>{});
}

}  // namespace

hipError_t t2v_launch_ncthw_to_cl(const t2v_op& op, hipStream_t s) {
  const int B = op.i[0], C = op.i[1], F = op.i[2], HW = op.i[3], ld = op.i[4];
  const long n = (long)B * F * HW;
  const int Bsrc = (op.i[6] > 0 && op.i[6] < B) ? op.i[6] : B;
  by_dtype(op.i[5], [&](auto t) {
    using TIN = decltype(t);
    hipLaunchKernelGGL(ncthw_to_cl_kernel<TIN>, dim3(grid_for(n)), dim3(256), 0, s, reinterpret_cast<const TIN*>(op.p[0]),
                       reinterpret_cast<f16*>(op.p[1]), B, C, F, HW, ld, op.f[0], Bsrc, reinterpret_cast<f16*>(op.p[2]),
                       (op.i[7] != 0 && ld >= 2 * C) ? 1 : 0);
  });
  return hipGetLastError();
}

hipError_t t2v_launch_cl_to_ncthw(const t2v_op& op, hipStream_t s) {
  const int B = op.i[0], C = op.i[1], F = op.i[2], HW = op.i[3], ld = op.i[4];
  const long n = (long)B * C * F * HW;
  by_dtype(op.i[5], [&](auto t) {
    using TOUT = decltype(t);
    hipLaunchKernelGGL(cl_to_ncthw_kernel<TOUT>, dim3(grid_for(n)), dim3(256), 0, s, reinterpret_cast<const float*>(op.p[0]),
                       reinterpret_cast<TOUT*>(op.p[1]), B, C, F, HW, ld);
  });
  return hipGetLastError();
}

hipError_t t2v_launch_to_uint8(const t2v_op& op, hipStream_t s) {
  const int NI = op.i[0], C = op.i[1], F = op.i[2], H = op.i[3], W = op.i[4];
  const int bgr = op.i[7];
  const long si = (long)(uint32_t)op.i[8] | ((long)op.i[9] << 32), sc = op.i[10], sf = (long)(uint32_t)op.i[11] | ((long)op.i[12] << 32);
  const long sy = op.i[13], sx = op.i[14];
  const dim3 g(grid_for((long)F * H * NI * W)), b(256);
  unsigned char* out = reinterpret_cast<unsigned char*>(op.p[1]);
  by_dtype(op.i[5], [&](auto t) {
    by_bool(op.i[6] != 0, [&](auto half) {
      using TIN = decltype(t);
      constexpr bool HALF = decltype(half)::value;
      const TIN* in = reinterpret_cast<const TIN*>(op.p[0]);
      if (op.i[15] == 1)                                 // torch_to_np: a kernel of its own, form 0 launches what it always launched
        hipLaunchKernelGGL((to_uint8_np_kernel<TIN, HALF>), g, b, 0, s, in, out, NI, C, F, H, W, si, sc, sf, sy, sx);
      else
        hipLaunchKernelGGL((to_uint8_kernel<TIN, HALF>), g, b, 0, s, in, out, NI, C, F, H, W, si, sc, sf, sy, sx, bgr);
    });
  });
  return hipGetLastError();
}

// Units of a row — bicubic: an output column; uint8 pass: a pixel (token forms), 4 pixels (horizontal, uint8) or 4 bytes (vertical,
// uint8) — in tiles of 256, one workgroup each, over the rows (planes x output rows | images x rows of the pass)
t2v_resample_grid t2v_resample_grid_of(const t2v_op& op) {
  const long out = op.i[4], axis = op.i[5], form = op.i[7];
  t2v_resample_grid g;
  if (op.i[9] == 1) {
    g.rows = (long)op.i[0] * out;
    g.units = op.i[10];
  } else {
    const long row_px = axis == 0 ? out : op.i[2];
    g.rows = (long)op.i[0] * (axis == 0 ? op.i[1] : out);
    g.units = form != 0 ? row_px : (axis == 0 ? (row_px + 3) / 4 : (row_px * 3 + 3) / 4);
  }
  g.tiles = (g.units + 255) / 256;
  return g;
}

hipError_t t2v_launch_resample(const t2v_op& op, hipStream_t s) {
  // (shape, pointers and the grid size were checked by the executor's validation)
  const t2v_resample_grid grid = t2v_resample_grid_of(op);
  const int tiles = (int)grid.tiles;
  const dim3 g((unsigned)(grid.rows * grid.tiles)), b(256);
  if (op.i[9] == 1) {                                    // float bicubic mode: [P, H, W] -> fp32 [P, Ho, Wo], one launch
    const int H = op.i[1], W = op.i[2], Ho = op.i[4], Wo = op.i[10];
    by_dtype(op.i[11], [&](auto t) {
      using TIN = decltype(t);
      hipLaunchKernelGGL(bicubic_kernel<TIN>, g, b, 0, s, reinterpret_cast<const TIN*>(op.p[0]), reinterpret_cast<float*>(op.p[1]),
                         reinterpret_cast<const float*>(op.p[2]), reinterpret_cast<const int*>(op.p[3]), H, W, Ho, Wo, tiles);
    });
    return hipGetLastError();
  }
  const int H = op.i[1], W = op.i[2], out = op.i[4], axis = op.i[5], ksize = op.i[6], ld = op.i[8];
  const unsigned char* src = reinterpret_cast<const unsigned char*>(op.p[0]);
  void* dst = reinterpret_cast<void*>(op.p[1]);
  const int* coef = reinterpret_cast<const int*>(op.p[2]);
  const int* bounds = reinterpret_cast<const int*>(op.p[3]);
  const float* lut = reinterpret_cast<const float*>(op.p[4]);
  by_index<3>(op.i[7], [&](auto form) {
    constexpr int FORM = decltype(form)::value;
    if (axis == 0) hipLaunchKernelGGL(resample_h_kernel<FORM>, g, b, 0, s, src, dst, coef, bounds, lut, W, out, ksize, ld, tiles);
    else hipLaunchKernelGGL(resample_v_kernel<FORM>, g, b, 0, s, src, dst, coef, bounds, lut, H, W, out, ksize, ld, tiles);
  });
  return hipGetLastError();
}

hipError_t t2v_launch_depth_tokens(const t2v_op& op, hipStream_t s) {
  // (shape and pointers were checked by the executor's validation)
  const int n = op.i[0], H = op.i[1], W = op.i[2], ld = op.i[5];
  by_dtype(op.i[3], [&](auto t) {
    by_bool(op.i[4] != 0, [&](auto norm) {
      using TIN = decltype(t);
      hipLaunchKernelGGL((depth_tokens_kernel<TIN, decltype(norm)::value>), dim3(n), dim3(256), 0, s, reinterpret_cast<const TIN*>(op.p[0]),
                         reinterpret_cast<f16*>(op.p[1]), H, W, ld);
    });
  });
  return hipGetLastError();
}

hipError_t t2v_launch_avgpool2(const t2v_op& op, hipStream_t s) {
  const int n = op.i[0], H = op.i[1], W = op.i[2], C = op.i[3];
  const int g = grid_for((long)n * (H / 2) * (W / 2) * (C / 4));
  hipLaunchKernelGGL(avgpool2_kernel, dim3(g), dim3(256), 0, s, reinterpret_cast<const float*>(op.p[0]), reinterpret_cast<float*>(op.p[1]),
                     reinterpret_cast<f16*>(op.p[2]), n, H, W, C, op.i[4], op.i[5], op.i[6]);
  return hipGetLastError();
}

hipError_t t2v_launch_reshard_rows(const t2v_op& op, hipStream_t s) {
  const int rows = op.i[0], cols = op.i[1], P = op.i[2], ld_src = op.i[5], ld_dst = op.i[6], ld_res = op.i[8];
  const long s_src = op.i[3], s_dst = op.i[4];
  const bool f32 = op.i[7] == T2V_F32;
  if (rows <= 0 || cols <= 0 || P <= 0 || cols % (f32 ? 4 : 8) != 0 || ld_src % (f32 ? 4 : 8) != 0 || ld_dst % (f32 ? 4 : 8) != 0)
    return hipErrorInvalidValue;
  if (op.p[2] != 0 && (!f32 || ld_res % 4 != 0)) return hipErrorInvalidValue;
  const int nparts = op.i[9] > 1 ? op.i[9] : 1;
  const int own = nparts > 1 ? op.i[13] : -1, own_is_src = op.i[14];
  const int v = f32 ? 4 : 8;
  if (nparts > 1 && (op.i[10] % v != 0 || op.i[11] % v != 0 || op.i[12] % 4 != 0 || own >= nparts || (own >= 0 && op.p[3] == 0) || nparts > 64))
    return hipErrorInvalidValue;
  const int g = grid_for((long)rows * (cols / v));
  by_dtype(op.i[7], [&](auto t) {                        // fp16 rows carry no residual: a null pointer, zero strides
    using T = decltype(t);
    hipLaunchKernelGGL(reshard_rows_kernel<T>, dim3(g, nparts), dim3(256), 0, s, reinterpret_cast<const T*>(op.p[0]),
                       reinterpret_cast<T*>(op.p[1]), f32 ? reinterpret_cast<const float*>(op.p[2]) : nullptr, rows, cols, P, s_src, s_dst,
                       ld_src, ld_dst, f32 ? ld_res : 0, (long)op.i[10], (long)op.i[11], f32 ? (long)op.i[12] : 0L, own, own_is_src,
                       reinterpret_cast<T*>(op.p[3]));
  });
  return hipGetLastError();
}

hipError_t t2v_launch_time_embed(const t2v_op& op, hipStream_t s) {
  const int B = op.i[0], dim = op.i[1];
  hipLaunchKernelGGL(time_embed_kernel, dim3((B * (dim / 2) + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const float*>(op.p[0]), reinterpret_cast<const float*>(op.p[1]),
                     reinterpret_cast<f16*>(op.p[2]), B, dim);
  return hipGetLastError();
}

hipError_t t2v_launch_copy2d(const t2v_op& op, hipStream_t s) {
  const int rows = op.i[0], cols = op.i[1], lds_ = op.i[2], ldd = op.i[3], sdt = op.i[4], ddt = op.i[5], act = op.i[6];
  if (cols % 4 != 0) return hipErrorInvalidValue;
  const int g = grid_for((long)rows * (cols / 4));
  const bool known = (sdt == T2V_F16 || sdt == T2V_F32) && (ddt == T2V_F16 || ddt == T2V_F32);      // (any other pair of tags: fp16 -> fp32)
  by_dtype(known ? sdt : T2V_F16, [&](auto ts) {
    by_dtype(known ? ddt : T2V_F32, [&](auto td) {
      using TS = decltype(ts);
      using TD = decltype(td);
      constexpr bool LO = std::is_same_v<TS, float> && std::is_same_v<TD, f16>;      // the low-order image exists for fp32 -> fp16 casts only
      hipLaunchKernelGGL((copy2d_kernel<TS, TD>), dim3(g), dim3(256), 0, s, reinterpret_cast<const TS*>(op.p[0]),
                         reinterpret_cast<TD*>(op.p[1]), rows, cols, lds_, ldd, act, LO ? reinterpret_cast<f16*>(op.p[2]) : nullptr);
    });
  });
  return hipGetLastError();
}

hipError_t t2v_launch_emphasis(const t2v_op& op, hipStream_t s) {
  const int rows = op.i[0], W = op.i[1], ldz = op.i[2], ldo = op.i[3];
  if (rows <= 0 || W <= 0 || W % 4 != 0 || ldz < W || ldo < W || ldo % 4 != 0) return hipErrorInvalidValue;
  by_dtype(op.i[4], [&](auto t) {
    using TZ = decltype(t);
    hipLaunchKernelGGL((emphasis_kernel<TZ>), dim3(1), dim3(1024), 0, s, reinterpret_cast<const TZ*>(op.p[0]),
                       reinterpret_cast<const float*>(op.p[1]), reinterpret_cast<float*>(op.p[2]), rows, W, ldz, ldo);
  });
  return hipGetLastError();
}

hipError_t t2v_launch_fingerprint(const t2v_op& op, hipStream_t s) {
  const int n = op.i[0], n_chunks = op.i[1];
  if (n <= 0 || n_chunks < n || op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0) return hipErrorInvalidValue;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(op.p[1]);
  const hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long) * (size_t)n, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fingerprint_kernel, dim3(n_chunks), dim3(256), 0, s, reinterpret_cast<const FpSeg*>(op.p[0]),
                     reinterpret_cast<const uint2*>(op.p[2]), out, n);
  return hipGetLastError();
}

hipError_t t2v_launch_lora_merge(const t2v_op& op, hipStream_t s) {
  static_assert(sizeof(LoraSeg) == 48, "the segment record of include/t2v_hip.h");
  const int n = op.i[0], n_tiles = op.i[1];
  if (n <= 0 || n_tiles < n || op.p[0] == 0 || op.p[1] == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lora_merge_kernel, dim3(n_tiles), dim3(256), 0, s, reinterpret_cast<const LoraSeg*>(op.p[0]),
                     reinterpret_cast<const uint2*>(op.p[1]), n, op.f[0]);
  return hipGetLastError();
}

hipError_t t2v_launch_embed_rows(const t2v_op& op, hipStream_t s) {
  const int rows = op.i[0], W = op.i[1], L = op.i[2], vocab = op.i[3];
  if (rows <= 0 || W <= 0 || L <= 0 || vocab <= 0) return hipErrorInvalidValue;
  by_dtype(op.i[4], [&](auto t) {
    using TT = decltype(t);
    hipLaunchKernelGGL((embed_rows_kernel<TT>), dim3(rows), dim3(256), 0, s, reinterpret_cast<const int*>(op.p[0]),
                       reinterpret_cast<const TT*>(op.p[1]), reinterpret_cast<const float*>(op.p[2]), reinterpret_cast<float*>(op.p[3]),
                       rows, W, L, vocab);
  });
  return hipGetLastError();
}

// What a DDIM_STEP record is, or why it is none: the one place that knows which combinations of i[5], i[7], i[8], i[9], i[4], p[3..8] and
// f[6] are legal (include/t2v_hip.h)
t2v_ddim_class t2v_ddim_classify(const t2v_op& op) {
  auto is = [](t2v_ddim_form form, int x0_form = 0) { return t2v_ddim_class{form, x0_form, nullptr}; };
  auto bad = [](const char* why) { return t2v_ddim_class{T2V_DDIM_MALFORMED, 0, why}; };
  const int C = op.i[0], cps = op.i[6] > 0 ? op.i[6] : C;
  if (C <= 0 || op.i[1] <= 0 || cps <= 0 || C % cps != 0) return bad("DDIM step needs C > 0, inner > 0, C % channels-per-sample == 0");
  if (op.i[2] < 0 || op.i[2] > cps || op.i[5] < 0 || op.i[5] > 4) return bad("DDIM step: guided channels / mode");
  if (op.i[5] == 3) {      // DDIM inversion (DDIMSampler.encode): out = f0 x + f1 e, nothing else
    if (op.i[7] != 0 || op.i[8] != 0 || op.i[9] != 0) return bad("DDIM step: mode 3 (inversion) has no mask blend i[7], no x0 restriction i[8] and no classifier-guidance term i[9]");
    if (op.i[4] != T2V_F32) return bad("DDIM step: mode 3 (inversion) needs an fp32 x");
    if (op.i[2] != 0 && op.i[2] != cps) return bad("DDIM step: mode 3 (inversion) combines the guidance over all channels (i[2] = channels per sample) or not at all (0)");
    if (op.p[0] == 0 || op.p[1] == 0 || op.p[3] == 0) return bad("null DDIM step pointer (mode 3 reads x p[0] and the eps pair p[1] and writes p[3])");
    return is(T2V_DDIM_INVERT);
  }
  if (op.i[5] == 4) {      // DDIM_Gaussian with the keyframe blend of the legacy img2vid loop: mode 0's update, then the blend
    if (op.i[7] != 0 || op.i[8] != 0 || op.i[9] != 0) return bad("DDIM step: mode 4 (keyframe blend) has no mask blend flag i[7], no x0 restriction i[8] and no classifier-guidance term i[9]");
    if (op.i[4] != T2V_F32) return bad("DDIM step: mode 4 (keyframe blend) needs an fp32 x");
    if (op.p[0] == 0 || op.p[1] == 0 || op.p[3] == 0) return bad("null DDIM step pointer");
    if (op.p[4] == 0 || op.p[5] == 0) return bad("DDIM step: mode 4 (keyframe blend) needs the original latent p[4] and the mask p[5]");
    if (op.p[6] == 0 && op.f[7] != 0.f) return bad("DDIM step: mode 4 (keyframe blend) needs the blend noise p[6] unless f[7] == 0");
    return is(T2V_DDIM_KEYFRAME);
  }
  if (op.i[8] < 0 || op.i[8] > 3) return bad("DDIM step: x0 restriction i[8] must be 0 (none), 1 (clamp), 2 (threshold) or 3 (measure pass)");
  if (op.i[9] != 0 && op.i[9] != 1) return bad("DDIM step: classifier-guidance flag i[9] must be 0 or 1");
  if (op.p[0] == 0 || op.p[1] == 0 || (op.p[3] == 0 && op.i[8] != 3)) return bad("null DDIM step pointer");
  if (op.i[7] != 0 && op.i[7] != 1) return bad("DDIM step: blend flag i[7] must be 0 or 1");
  if (op.i[5] == 2) {      // UniPC's thresholded data prediction: a measure record and an apply record, nothing else
    if (op.i[8] != 2 && op.i[8] != 3) return bad("DDIM step: mode 2 (thresholded data prediction) is the measure pass i[8] = 3 or the apply pass i[8] = 2; the clamp i[8] = 1 and the plain prediction (a LINCOMB) are not records of it");
    if (op.i[7] != 0 || op.i[9] != 0) return bad("DDIM step: mode 2 has no mask blend i[7] and no classifier-guidance term i[9]");
    if (op.i[4] != T2V_F32) return bad("DDIM step: mode 2 needs an fp32 x");
    if (op.i[2] != 0 && op.i[2] != cps) return bad("DDIM step: mode 2 combines the guidance over all channels (i[2] = channels per sample) or not at all (0)");
    if (op.p[7] == 0) return bad("DDIM step: mode 2 needs the threshold table p[7]");
    if ((int64_t)cps * op.i[1] > (int64_t)16777216) return bad("DDIM step: mode 2 ranks at most 16 777 216 elements per sample (torch.quantile's limit)");
    if (op.i[8] == 3 && !(op.f[6] > 0.f && op.f[6] <= 1.f)) return bad("DDIM step: the measure pass i[8] = 3 needs a quantile f[6] in (0, 1]");
    return op.i[8] == 3 ? is(T2V_DDIM_MEASURE, 1) : is(T2V_DDIM_THRESHOLD);
  }
  if (op.i[8] != 0 || op.i[9] != 0) {
    if (op.i[5] != 0) return bad("DDIM step: the x0 restriction i[8] and the classifier-guidance term i[9] exist for mode 0 (DDIM_Gaussian) only");
    if (op.i[7] != 0) return bad("DDIM step: the x0 restriction i[8] / classifier-guidance term i[9] and the mask blend i[7] exclude each other");
    if (op.i[4] != T2V_F32) return bad("DDIM step: the x0 restriction i[8] and the classifier-guidance term i[9] need an fp32 x");
    if ((op.i[8] == 2 || op.i[8] == 3) && op.p[7] == 0) return bad("DDIM step: the x0 threshold i[8] = 2 | 3 needs the threshold table p[7]");
    if (op.i[9] == 1 && op.p[8] == 0) return bad("DDIM step: the classifier-guidance term i[9] needs the gradient p[8]");
    if (op.i[8] == 1 && !(op.f[6] >= 0.f)) return bad("DDIM step: the x0 clamp i[8] = 1 needs a bound f[6] >= 0");
    if (op.i[8] != 3) return is(T2V_DDIM_RESTRICT);
    if ((int64_t)cps * op.i[1] > (int64_t)16777216) return bad("DDIM step: the measure pass i[8] = 3 ranks at most 16 777 216 elements per sample (torch.quantile's limit)");
    if (!(op.f[6] > 0.f && op.f[6] <= 1.f)) return bad("DDIM step: the measure pass i[8] = 3 needs a percentile f[6] in (0, 1]");
    return is(T2V_DDIM_MEASURE, 0);
  }
  if (op.i[7] == 0) return is(T2V_DDIM_PLAIN);
  if (op.i[5] != 1) return bad("DDIM step: the mask blend i[7] exists for mode 1 (LDM DDIM) only");
  if (op.i[4] != T2V_F32) return bad("DDIM step: the mask blend i[7] needs an fp32 x");
  if (op.p[4] == 0 || op.p[5] == 0) return bad("DDIM step: the mask blend i[7] needs the known x0 p[4] and the mask p[5]");
  if (op.p[6] == 0 && op.f[7] != 0.f) return bad("DDIM step: the mask blend i[7] needs the q-noise p[6] unless f[7] == 0");
  return is(T2V_DDIM_BLEND);
}

// Every caller has validated the record (t2v_run_ops and t2v_plan_create pass each record through validate_op, which asks
// t2v_ddim_classify): the launcher asks for the form and checks nothing again.
hipError_t t2v_launch_ddim_step(const t2v_op& op, hipStream_t s) {
  DdimParams p;
  p.xt = reinterpret_cast<const void*>(op.p[0]);
  p.eps = reinterpret_cast<const void*>(op.p[1]);
  p.noise = reinterpret_cast<const float*>(op.p[2]);
  p.out = reinterpret_cast<void*>(op.p[3]);
  p.C = op.i[0]; p.inner = op.i[1]; p.guided = op.i[2]; p.eps_f32 = op.i[3] == T2V_F32; p.x_f32 = op.i[4] == T2V_F32;
  p.mode = op.i[5];
  p.cps = op.i[6] > 0 ? op.i[6] : p.C;       // channels per sample (several videos per batch: C = samples * cps)
  p.a_recip = op.f[0]; p.a_recipm1 = op.f[1]; p.sqrt_aprev = op.f[2]; p.dir_coef = op.f[3]; p.sigma = op.f[4];
  p.gscale = op.f[5];
  const t2v_ddim_class cls = t2v_ddim_classify(op);
  const long total = (long)p.C * p.inner;
  const dim3 g(grid_for(total)), b(256);
  const DdimRestrict r = {reinterpret_cast<const float*>(op.p[7]), reinterpret_cast<const float*>(op.p[8]), op.f[6], op.f[7]};
  by_dtype(op.i[3], [&](auto te) {
    using TE = decltype(te);
    switch (cls.form) {
      case T2V_DDIM_PLAIN:
        by_dtype(op.i[4], [&](auto tx) { hipLaunchKernelGGL((ddim_step_kernel<decltype(tx), TE>), g, b, 0, s, p); });
        break;
      case T2V_DDIM_BLEND: {                   // masked step: the blend is a compile-time variant (fp32 x only)
        const DdimBlend k = {reinterpret_cast<const float*>(op.p[4]), reinterpret_cast<const float*>(op.p[5]),
                             reinterpret_cast<const float*>(op.p[6]), op.f[6], op.f[7]};
        hipLaunchKernelGGL((ddim_step_kernel<float, TE, DdimBlend>), g, b, 0, s, p, k);
        break;
      }
      case T2V_DDIM_RESTRICT:                  // mode 0 with a restricted x0 (i[8] = 1 | 2) and / or the classifier-guidance term (i[9])
        by_index<3>(op.i[8], [&](auto restrict_) {
          by_bool(op.i[9] != 0, [&](auto cond) {
            constexpr int RESTRICT = decltype(restrict_)::value;
            constexpr bool COND = decltype(cond)::value;
            if constexpr (RESTRICT != 0 || COND) hipLaunchKernelGGL((ddim_restrict_kernel<TE, 0, RESTRICT, COND>), g, b, 0, s, p, r);
          });
        });
        break;
      case T2V_DDIM_THRESHOLD:                 // mode 2's apply pass: the thresholded data prediction itself
        hipLaunchKernelGGL((ddim_restrict_kernel<TE, 1, 2, false>), g, b, 0, s, p, r);
        break;
      case T2V_DDIM_MEASURE: {                 // one workgroup per sample, writes table[sample][0..3] only
        const long n = (long)p.cps * p.inner;
        DdimMeasure m;
        m.table = reinterpret_cast<float*>(op.p[7]);
        volatile float rank = op.f[6] * (float)(n - 1);     // torch.quantile's fp32 rank (one rounded product)
        const float below = floorf(rank);
        m.lo = (unsigned)below; m.hi = (unsigned)ceilf(rank); m.w = rank - below;
        by_index<2>(cls.x0_form, [&](auto form) {
          hipLaunchKernelGGL((ddim_measure_kernel<TE, decltype(form)::value>), dim3(p.C / p.cps), dim3(QT_THREADS), 0, s, p, m);
        });
        break;
      }
      case T2V_DDIM_INVERT: {                  // fp32 x, guidance over all channels or none; p[4]: the optional kept copy
        const bool guided = p.guided != 0;
        // every 16-byte access of the vector path: x, out, keep, the conditional half and — guided — the unconditional half behind it
        const uint64_t eu = op.p[1] + (uint64_t)total * sizeof(TE);
        const bool vec = total >= 4 && ((op.p[0] | op.p[1] | op.p[3] | op.p[4] | (guided ? eu : 0)) & 15) == 0;
        const dim3 gi(grid_for(vec ? total >> 2 : total));
        by_bool(guided, [&](auto gd) {
          by_bool(vec, [&](auto vc) {
            hipLaunchKernelGGL((ddim_invert_kernel<TE, decltype(gd)::value, decltype(vc)::value>), gi, b, 0, s, p, reinterpret_cast<float*>(op.p[4]));
          });
        });
        break;
      }
      case T2V_DDIM_KEYFRAME: {                // fp32 x; p[4..6]: the original latent, the mask, the blend noise; i[10]: the threshold's bits
        float thr;
        __builtin_memcpy(&thr, &op.i[10], sizeof thr);
        const DdimKeyframe k = {reinterpret_cast<const float*>(op.p[4]), reinterpret_cast<const float*>(op.p[5]),
                                reinterpret_cast<const float*>(op.p[6]), op.f[6], op.f[7], thr};
        // every 16-byte access of the vector path: x, out, original, mask, the conditional half, and what of the unconditional half,
        // the eta noise and the blend noise the kernel reads
        const uint64_t eu = p.guided != 0 ? op.p[1] + (uint64_t)total * sizeof(TE) : 0;
        const uint64_t eta = (op.p[2] != 0 && p.sigma != 0.f) ? op.p[2] : 0;
        const bool vec = (long)p.cps * p.inner >= 4 && ((op.p[0] | op.p[1] | op.p[3] | op.p[4] | op.p[5] | op.p[6] | eu | eta) & 15) == 0;
        by_bool(vec, [&](auto vc) {
          hipLaunchKernelGGL((ddim_keyframe_kernel<TE, decltype(vc)::value>), dim3(grid_for(vec ? total >> 2 : total)), b, 0, s, p, k);
        });
        break;
      }
      case T2V_DDIM_MALFORMED: break;
    }
  });
  return cls.form == T2V_DDIM_MALFORMED ? hipErrorInvalidValue : hipGetLastError();
}

const char* t2v_window_refusal(const t2v_op& op) {
  const int32_t* I = op.i;
  const bool blend = I[9] == 1;
  const long V = I[0], C = I[1], F = I[3], HW = I[4], len = I[5], nW = I[6];
  if (V <= 0 || C <= 0 || F <= 0 || HW <= 0 || nW <= 0)
    return blend ? "window blend (lincomb i[9] = 1): videos, channels, frames, pixels per frame and windows per video must be positive"
                 : "window gather (lincomb i[9] = 2): videos, channels, frames, pixels per frame and windows per video must be positive";
  if (len < 2 || len > F)
    return blend ? "window blend (lincomb i[9] = 1): the window length i[5] must lie in 2 .. frames"
                 : "window gather (lincomb i[9] = 2): the window length i[5] must lie in 2 .. frames";
  if (I[2] != T2V_F16 && I[2] != T2V_F32)
    return blend ? "window blend (lincomb i[9] = 1): unknown eps dtype i[2] (fp16 | fp32)" : "window gather (lincomb i[9] = 2): unknown latent dtype i[2] (fp16 | fp32)";
  const long clip = V * C * F * HW, windows = V * nW * C * len * HW;
  if (blend) {
    if (I[7] != 1 && I[7] != 2) return "window blend (lincomb i[9] = 1): roles i[7] must be 1 (conditional) or 2 (cond | uncond)";
    if (I[8] != 0) return "window blend (lincomb i[9] = 1): i[8] must be 0";
    if (op.p[0] == 0 || op.p[1] == 0 || op.p[2] == 0 || op.p[6] == 0) return "null window blend pointer (lincomb i[9] = 1: windows' eps, starts, weights, out)";
    if (I[7] * clip > 0x7fffffffL || I[7] * windows > 0x7fffffffL) return "window blend (lincomb i[9] = 1): more than 2^31 - 1 elements";
  } else {
    if (I[8] <= 0 || I[7] < 0 || (long)I[7] + I[8] > V * nW) return "window gather (lincomb i[9] = 2): batch rows i[7] .. i[7] + i[8] must lie inside videos x windows";
    if (op.p[0] == 0 || op.p[1] == 0 || op.p[6] == 0) return "null window gather pointer (lincomb i[9] = 2: latent, starts, out)";
    if (clip > 0x7fffffffL || windows > 0x7fffffffL) return "window gather (lincomb i[9] = 2): more than 2^31 - 1 elements";
  }
  return nullptr;
}

static hipError_t launch_window(const t2v_op& op, hipStream_t s) {
  if (t2v_window_refusal(op) != nullptr) return hipErrorInvalidValue;
  const WindowGeom g = {reinterpret_cast<const int*>(op.p[1]), op.i[0], op.i[1], op.i[3], op.i[4], op.i[5], op.i[6]};
  const int item = op.i[2] == T2V_F32 ? 4 : 2;
  if (op.i[9] == 2) {
    const int row0 = op.i[7], rows = op.i[8];
    const long row_elems = (long)g.C * g.length * g.HW;
    // every 16-byte access of the vector path: a frame is a whole number of units, and both bases sit on one
    const bool vec = ((long)g.HW * item) % 16 == 0 && ((op.p[0] | op.p[6]) & 15) == 0;
    if (vec) {
      const int units = g.HW * item / 16;
      hipLaunchKernelGGL(window_gather_kernel<uint4>, dim3(grid_for(rows * row_elems / g.HW * units)), dim3(256), 0, s,
                         reinterpret_cast<const uint4*>(op.p[0]), reinterpret_cast<uint4*>(op.p[6]), g, row0, rows, units);
    } else {
      by_dtype(op.i[2], [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(window_gather_kernel<T>, dim3(grid_for(rows * row_elems)), dim3(256), 0, s, reinterpret_cast<const T*>(op.p[0]),
                           reinterpret_cast<T*>(op.p[6]), g, row0, rows, g.HW);
      });
    }
    return hipGetLastError();
  }
  const int roles = op.i[7];
  const long total = (long)roles * g.V * g.C * g.F * g.HW;
  // four neighbours of a frame per thread: 16-byte stores, 8- or 16-byte loads — HW % 4 keeps every run inside a frame and aligned
  const bool vec = g.HW % 4 == 0 && (op.p[6] & 15) == 0 && (op.p[0] & (uint64_t)(4 * item - 1)) == 0;
  by_dtype(op.i[2], [&](auto t) {
    using TE = decltype(t);
    by_bool(vec, [&](auto vc) {
      constexpr int VEC = decltype(vc)::value ? 4 : 1;
      hipLaunchKernelGGL((window_blend_kernel<TE, VEC>), dim3(grid_for(total / VEC)), dim3(256), 0, s, reinterpret_cast<const TE*>(op.p[0]),
                         reinterpret_cast<const float*>(op.p[2]), reinterpret_cast<float*>(op.p[6]), g, roles);
    });
  });
  return hipGetLastError();
}

hipError_t t2v_launch_lincomb(const t2v_op& op, hipStream_t s) {
  if (op.i[9] != 0) return launch_window(op, s);      // the context-window forms; every earlier record leaves i[9] at zero
  LinParams p;
  p.n = op.i[0]; p.n_terms = op.i[1]; p.out_f32 = op.i[2] == T2V_F32;
  if (p.n_terms < 1 || p.n_terms > 6 || p.n <= 0) return hipErrorInvalidValue;
  for (int k = 0; k < 6; ++k) {
    p.t[k] = reinterpret_cast<const void*>(op.p[k]);
    p.c[k] = op.f[k];
    p.f32[k] = op.i[3 + k] == T2V_F32;
  }
  p.out = reinterpret_cast<void*>(op.p[6]);
  hipLaunchKernelGGL(lincomb_kernel, dim3(grid_for(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
