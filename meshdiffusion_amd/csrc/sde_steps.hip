// Every sampler update: the DDPM ancestral step, the DDIM step and the inpainting blend / re-noise, the predictor-corrector
// updates (reference lib/diffusion/sampling.py:185-210 predictors, :259-321 correctors, sde_lib.py:83-111 reverse SDE, :198-232
// VPSDE), the probability-flow right-hand side, reconstruction guidance and the DPM-Solver++ multistep update.  All NCDHW
// [B][C][P]; the per-sample coefficients come from the host, built once per sampler with the reference's torch expressions.
// Same operation order as the reference, no FMA contraction anywhere in this file: with identical eps / z the float32 updates
// are bit-identical to the PyTorch elementwise chains.
// An export refuses, in this order: null or misaligned pointers (16 bytes where the kernel moves four floats or two doubles at
// a time, the element size elsewhere), sizes and scalars, aliasing.
#include "md_args.h"

#pragma clang fp contract(off)

typedef __attribute__((ext_vector_type(2))) double f64x2;
typedef __attribute__((ext_vector_type(4))) double f64x4;

// ---- device vocabulary ----------------------------------------------------------------------------------------------
// grid-stride loops over [0, n) of one sample (blockIdx.y picks the sample): four values or one value per thread and trip
#define MD_STREAM4(i, CP) \
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < CP; i += (int64_t)gridDim.x * blockDim.x * 4)
#define MD_STREAM1(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)

// four values at a 16-byte aligned address: one f32x4, or a pair of f64x2
static __device__ __forceinline__ f32x4 md_load4(const float* p) { return *(const f32x4*)p; }
static __device__ __forceinline__ void md_store4(float* p, f32x4 v) { *(f32x4*)p = v; }
static __device__ __forceinline__ f64x4 md_load4(const double* p) {
  const f64x2 a = *(const f64x2*)p, c = *(const f64x2*)(p + 2);
  return f64x4{a[0], a[1], c[0], c[1]};
}
static __device__ __forceinline__ void md_store4(double* p, f64x4 v) {
  *(f64x2*)p = f64x2{v[0], v[1]};
  *(f64x2*)(p + 2) = f64x2{v[2], v[3]};
}
// the optional grid mask at `pos`: ones without one
static __device__ __forceinline__ f32x4 md_mask4(const float* mask, int64_t pos) {
  f32x4 mv = {1.f, 1.f, 1.f, 1.f};
  if (mask) mv = md_load4(mask + pos);
  return mv;
}

// wave64 xor butterfly over the offsets 32, 16, ..., 1: every lane ends with the same bits
template <int N>
static __device__ __forceinline__ void md_wave_sum(double (&v)[N]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += __shfl_xor(v[k], o, 64);
  }
}

// N sums over a workgroup of 256 in a fixed order: butterfly, one LDS word per wave, (r0 + r1) + (r2 + r3).  True in
// thread 0 only, which then holds the sums in v.  The order of these additions is what makes the slabs reproducible.
template <int N>
static __device__ __forceinline__ bool md_block_sum(double (&v)[N]) {
  md_wave_sum(v);
  __shared__ double red[N][4];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
  return true;
}

// ---- host vocabulary ------------------------------------------------------------------------------------------------
// the sizes of a [batch][C][P] state; four_wide: the kernel moves four values at a time, which must not straddle two channels
static bool md_bad_dims(int32_t batch, int32_t C, int64_t P, bool four_wide) {
  return batch <= 0 || C <= 0 || P <= 0 || (four_wide && (P % 4));
}

// workgroups of 256 threads for `threads` of them, at most `cap`
static unsigned md_grid_x(int64_t threads, int64_t cap) {
  const int64_t blocks = (threads + 255) / 256;
  return (unsigned)(blocks < cap ? blocks : cap);
}
// one workgroup per 1024 values, at most 1024 workgroups in all (B*S <= 1024 keeps the slab prologue's L2 reads small)
static unsigned stream_blocks(int64_t CP, int batch) { return md_grid_x(CP / 4, batch >= 1024 ? 1 : 1024 / batch); }

struct md_span { const void* p; int64_t n; };       // n bytes at p; null: an absent operand
static bool md_overlap(const md_span& a, const md_span& b) {
  const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
  return a.p && b.p && pa < pb + (uintptr_t)b.n && pb < pa + (uintptr_t)a.n;
}
// an output shares memory with an input or with another output
template <int NO, int NI>
static bool md_any_alias(const md_span (&out)[NO], const md_span (&in)[NI]) {
  for (int o = 0; o < NO; ++o) {
    for (const md_span& i : in)
      if (md_overlap(out[o], i)) return true;
    for (int q = o + 1; q < NO; ++q)
      if (md_overlap(out[o], out[q])) return true;
  }
  return false;
}

// ---- DDPM ancestral update (reference models/utils.py:191-198, sampling.py:222-230,476-478) ----
__global__ void md_ancestral_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                         const float* __restrict__ z, const float* __restrict__ mask,
                                         const float* __restrict__ coef, float* __restrict__ x_out,
                                         float* __restrict__ xm_out, int64_t CP, int64_t P) {
  const int b = blockIdx.y;
  const float beta = coef[b * 4 + 0], sigma = coef[b * 4 + 1], sq1mb = coef[b * 4 + 2], sqb = coef[b * 4 + 3];
  const int64_t base = (int64_t)b * CP;
  MD_STREAM4(i, CP) {
    const f32x4 xv = md_load4(x + base + i), ev = md_load4(eps + base + i), zv = md_load4(z + base + i);
    const f32x4 mv = md_mask4(mask, i % P);
    f32x4 xo, xmo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float score = (-ev[e]) / sigma;
      const float xm = (xv[e] + beta * score) / sq1mb;
      const float xn = xm + sqb * zv[e];
      xo[e] = xn * mv[e];
      xmo[e] = xm * mv[e];
    }
    md_store4(x_out + base + i, xo);
    md_store4(xm_out + base + i, xmo);
  }
}

// ---- deterministic DDIM update (reference sde_lib.py:113-140 `discretize_ddim`, sampling.py:556-565) ----
// The reference keeps the state in float64 from the first update on (x.double() arithmetic, float32 only for the U-Net
// input); so does this kernel.  Same operation order:
//   x0s = x - a2*eps ; sst = x - x0s ; x0_pred = x0s / a1 ; x_new = r1*x + (r2 - r1)*sst   (r1 = a1p/a1, r2 = a2p/a2)
// then both results times the grid mask, and the optional channel-`ch` inpainting blend v*(1-pm) + partial*pm
// (sampling.py:562-564).  coef[b] = {a1, a2, r1, r2} as doubles (a1, a2 are float32 table entries widened).
// One value per thread and trip: P need not be a multiple of four.
__global__ void md_ddim_step_kernel(const double* __restrict__ x, const float* __restrict__ eps,
                                    const float* __restrict__ mask, const double* __restrict__ coef,
                                    const float* __restrict__ partial, const float* __restrict__ pmask, int ch,
                                    double* __restrict__ x_out, double* __restrict__ x0_out, float* __restrict__ x_f32,
                                    int64_t CP, int64_t P) {
  const int b = blockIdx.y;
  const double a1 = coef[b * 4 + 0], a2 = coef[b * 4 + 1], r1 = coef[b * 4 + 2], r2 = coef[b * 4 + 3];
  const double r21 = (-r1) + r2;
  const int64_t base = (int64_t)b * CP;
  MD_STREAM1(i, CP) {
    const double xv = x[base + i];
    const double x0s = xv - a2 * (double)eps[base + i];
    const double sst = xv - x0s;
    double x0p = x0s / a1;
    double xn = r1 * xv + r21 * sst;
    const int64_t pos = i % P;
    if (mask) { const double m = (double)mask[pos]; xn = xn * m; x0p = x0p * m; }
    if (partial != nullptr && i / P == ch) {
      const double pm = (double)pmask[pos], pv = (double)partial[pos];
      xn = xn * (1.0 - pm) + pv * pm;
      x0p = x0p * (1.0 - pm) + pv * pm;
    }
    x_out[base + i] = xn;
    x0_out[base + i] = x0p;
    x_f32[base + i] = (float)xn;
  }
}

// ---- inpainting blend of one channel (reference sampling.py:455-466), scalar: any P ----------------------------------
__global__ void md_inpaint_blend_kernel(float* __restrict__ x, const float* __restrict__ src,
                                        const float* __restrict__ pmask, const float* __restrict__ gmask,
                                        int C, int ch, int64_t P, int64_t src_bstride) {
  const int b = blockIdx.y;
  float* xc = x + ((int64_t)b * C + ch) * P;
  const float* sc = src + (int64_t)b * src_bstride;
  MD_STREAM1(i, P) {
    const float m = pmask[i];
    float v = xc[i] * (1.f - m) + sc[i] * m;
    if (gmask) v = v * gmask[i];
    xc[i] = v;
  }
}

// re-noise the conditioned channel to level t (reference sampling.py:460-466):
//   upd = mean_coef[b]*x + std[b]*z ;  x = (x*(1-m) + upd*m)*gm ;  x_mean[ch] = x[ch]
__global__ void md_inpaint_renoise_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                          const float* __restrict__ z, const float* __restrict__ pmask,
                                          const float* __restrict__ gmask, const float* __restrict__ coef,
                                          int C, int ch, int64_t P) {
  const int b = blockIdx.y;
  const float mc = coef[b * 2 + 0], sd = coef[b * 2 + 1];
  float* xc = x + ((int64_t)b * C + ch) * P;
  float* xm = x_mean ? x_mean + ((int64_t)b * C + ch) * P : nullptr;
  const float* zc = z + (int64_t)b * P;
  MD_STREAM1(i, P) {
    const float m = pmask[i];
    const float xv = xc[i];
    const float mean = mc * xv;
    const float upd = mean + sd * zc[i];
    float v = xv * (1.f - m) + upd * m;
    if (gmask) v = v * gmask[i];
    xc[i] = v;
    if (xm) xm[i] = v;
  }
}

// ---- Langevin corrector, launch 1: per-workgroup partial sums of eps^2 and z^2 ---------------------------------
// grid (MD_LANGEVIN_SLABS, B): workgroup (s, b) writes slabs[b][s] = {sum eps^2, sum z^2} over its strided share of
// sample b.  Fixed grid and fixed per-thread order: the partial sums do not depend on scheduling.
__global__ __launch_bounds__(256) void md_langevin_norms_kernel(const float* __restrict__ eps, const float* __restrict__ z,
                                                                double* __restrict__ slabs, int64_t CP) {
  const int b = blockIdx.y;
  const int64_t base = (int64_t)b * CP;
  double ae = 0.0, az = 0.0;
#pragma unroll 4
  MD_STREAM4(i, CP) {
    const f32x4 ev = md_load4(eps + base + i), zv = md_load4(z + base + i);
    ae += (double)(ev[0] * ev[0] + ev[1] * ev[1]) + (double)(ev[2] * ev[2] + ev[3] * ev[3]);
    az += (double)(zv[0] * zv[0] + zv[1] * zv[1]) + (double)(zv[2] * zv[2] + zv[3] * zv[3]);
  }
  double acc[2] = {ae, az};
  if (md_block_sum(acc)) *(f64x2*)(slabs + ((int64_t)b * MD_LANGEVIN_SLABS + blockIdx.x) * 2) = f64x2{acc[0], acc[1]};
}

// ---- Langevin / ALD corrector, launch 2 ---------------------------------------------------------------------------
// coef[b] = {sigma, alpha, ald_step}.  Prologue (wave 0, Langevin only): the slabs of every sample are reduced in a fixed
// order (one slab per lane, xor butterfly: every lane ends with the same bits), giving
//   grad_norm  = mean_b sqrt(sum eps_b^2) / sigma_b      (score = -eps/sigma, models/utils.py:191-198)
//   noise_norm = mean_b sqrt(sum z_b^2)
//   step_b     = (snr * noise_norm / grad_norm)^2 * 2 * alpha_b                                     (sampling.py:282-284)
// ALD takes step_b = coef[b][2] = (snr*std_b)^2 * 2 * alpha_b (sampling.py:312-315).  Then
//   x_mean = x + step_b*score ; x = x_mean + sqrt(step_b*2)*z ; both times the grid mask        (sampling.py:285-286, 450)
static_assert(MD_LANGEVIN_SLABS == 64, "the prologue reduces one slab per lane of a wave64");

__global__ __launch_bounds__(256) void md_langevin_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                               const float* __restrict__ z, const float* __restrict__ mask,
                                                               const float* __restrict__ coef, const double* __restrict__ slabs,
                                                               float snr, int mode, float* __restrict__ x_out,
                                                               float* __restrict__ xm_out, float* __restrict__ step_out,
                                                               int B, int64_t CP, int64_t P) {
  const int b = blockIdx.y;
  __shared__ float s_step;
  if (threadIdx.x < 64) {
    float step;
    if (mode == MD_CORRECTOR_LANGEVIN) {
      const int lane = threadIdx.x;
      double gsum = 0.0, nsum = 0.0;
      for (int bb = 0; bb < B; ++bb) {
        const f64x2 v = *(const f64x2*)(slabs + ((int64_t)bb * MD_LANGEVIN_SLABS + lane) * 2);
        double s[2] = {v[0], v[1]};
        md_wave_sum(s);
        gsum += sqrt(s[0]) / (double)coef[bb * 3 + 0];
        nsum += sqrt(s[1]);
      }
      const float grad_norm = (float)(gsum / (double)B), noise_norm = (float)(nsum / (double)B);
      const float r = (snr * noise_norm) / grad_norm;
      step = ((r * r) * 2.f) * coef[b * 3 + 1];
    } else {
      step = coef[b * 3 + 2];
    }
    if (threadIdx.x == 0) {
      s_step = step;
      if (blockIdx.x == 0) step_out[b] = step;
    }
  }
  __syncthreads();
  const float step = s_step;
  const float sigma = coef[b * 3 + 0];
  const float sq = sqrtf(step * 2.f);
  const int64_t base = (int64_t)b * CP;
  MD_STREAM4(i, CP) {
    const f32x4 xv = md_load4(x + base + i), ev = md_load4(eps + base + i), zv = md_load4(z + base + i);
    const f32x4 mv = md_mask4(mask, i % P);
    f32x4 xo, xmo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float score = (-ev[e]) / sigma;
      const float xm = xv[e] + step * score;
      const float xn = xm + sq * zv[e];
      xo[e] = xn * mv[e];
      xmo[e] = xm * mv[e];
    }
    md_store4(x_out + base + i, xo);
    md_store4(xm_out + base + i, xmo);
  }
}

// ---- SDE predictors, one launch ------------------------------------------------------------------------------------
// coef[b] = {sigma, c1, c2, c3, c4}; score = -eps/sigma.
//   MD_SDE_REVERSE_DIFFUSION (sde_lib.py:106-111 with VPSDE.discretize :224-232, sampling.py:204-209):
//     c1 = sqrt(alpha), c2 = G^2 = sqrt(beta)^2, c3 = h (1, or 0.5 under probability flow), c4 = G' (sqrt(beta), or 0)
//     f = c1*x - x ; rev_f = f - (c2*score)*c3 ; x_mean = x - rev_f ; x = x_mean + c4*z
//   MD_SDE_EULER_MARUYAMA (sde_lib.py:93-99 with VPSDE.sde :198-202, sampling.py:190-196):
//     c1 = -0.5*beta_t, c2 = diffusion^2 = sqrt(beta_t)^2, c3 = dt = -1/N, c4 = diffusion*sqrt(-dt)
//     drift = c1*x - c2*score ; x_mean = x + drift*c3 ; x = x_mean + c4*z
// both results times the grid mask (sampling.py:452, 478).
__global__ __launch_bounds__(256) void md_sde_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                          const float* __restrict__ z, const float* __restrict__ mask,
                                                          const float* __restrict__ coef, int kind, float* __restrict__ x_out,
                                                          float* __restrict__ xm_out, int64_t CP, int64_t P) {
  const int b = blockIdx.y;
  const float sigma = coef[b * 5 + 0], c1 = coef[b * 5 + 1], c2 = coef[b * 5 + 2], c3 = coef[b * 5 + 3], c4 = coef[b * 5 + 4];
  const int64_t base = (int64_t)b * CP;
  MD_STREAM4(i, CP) {
    const f32x4 xv = md_load4(x + base + i), ev = md_load4(eps + base + i), zv = md_load4(z + base + i);
    const f32x4 mv = md_mask4(mask, i % P);
    f32x4 xo, xmo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float score = (-ev[e]) / sigma;
      float xm;
      if (kind == MD_SDE_REVERSE_DIFFUSION) {
        const float f = c1 * xv[e] - xv[e];
        const float rev_f = f - (c2 * score) * c3;
        xm = xv[e] - rev_f;
      } else {
        const float drift = c1 * xv[e] - c2 * score;
        xm = xv[e] + drift * c3;
      }
      const float xn = xm + c4 * zv[e];
      xo[e] = xn * mv[e];
      xmo[e] = xm * mv[e];
    }
    md_store4(x_out + base + i, xo);
    md_store4(xm_out + base + i, xmo);
  }
}

// ---- probability-flow ODE right-hand side (reference lib/diffusion/likelihood.py:63-78 drift_fn / div_fn, one launch) ----
// coef[b] = {c_x = -0.5*beta(t), c_e = 0.5*beta(t)/sigma(t)} as doubles (VPSDE.sde with score = -eps_hat/sigma under
// probability flow): drift = (c_x*x + c_e*eps_hat)*mask, formed in double and rounded once.  With the vector-Jacobian product
// g = J^T probe: slabs[b][s] = sum over workgroup s's share of probe*(c_x*probe + c_e*g)*mask -- the Hutchinson estimate of the
// drift's divergence, in the manner of md_langevin_norms: fixed grid, fixed per-thread order, fp64 partial sums, no atomics.
template <bool DIV>
__global__ __launch_bounds__(256) void md_pf_ode_rhs_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                            const float* __restrict__ g, const float* __restrict__ probe,
                                                            const float* __restrict__ mask, const double* __restrict__ coef,
                                                            float* __restrict__ drift, double* __restrict__ slabs, int64_t CP,
                                                            int64_t P) {
  const int b = blockIdx.y;
  const double cx = coef[b * 2 + 0], ce = coef[b * 2 + 1];
  const int64_t base = (int64_t)b * CP;
  double acc[1] = {0.0};
  MD_STREAM4(i, CP) {
    const f32x4 xv = md_load4(x + base + i), ev = md_load4(eps + base + i);
    const f32x4 mv = md_mask4(mask, i % P);
    f32x4 dv;
#pragma unroll
    for (int e = 0; e < 4; ++e) dv[e] = (float)((cx * (double)xv[e] + ce * (double)ev[e]) * (double)mv[e]);
    md_store4(drift + base + i, dv);
    if constexpr (DIV) {
      const f32x4 gv = md_load4(g + base + i), pv = md_load4(probe + base + i);
      double t[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = ((double)pv[e] * (cx * (double)pv[e] + ce * (double)gv[e])) * (double)mv[e];
      acc[0] += (t[0] + t[1]) + (t[2] + t[3]);
    }
  }
  if constexpr (DIV) {
    if (md_block_sum(acc)) slabs[(int64_t)b * MD_LANGEVIN_SLABS + blockIdx.x] = acc[0];
  }
}

// ---- reconstruction guidance (diffusion posterior sampling, Chung et al. 2023) on one channel of the predicted clean grid ----
// launch 1: coef[b] = {alpha, sigma} as doubles.  x0_hat = (x - sigma*eps_hat)/alpha ; r = (pm*gm)*(x0_hat[ch] - y), formed in
// double and rounded once, is channel `ch` of the cotangent; every other channel is +0.  slabs[b][s] = sum over workgroup s's
// share of the squares of the ROUNDED r, so the norm is that of the cotangent the backward sees.  Grid and order as
// md_langevin_norms: two runs give the same bits.
__global__ __launch_bounds__(256) void md_guide_residual_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                                const float* __restrict__ src, int64_t src_bstride,
                                                                const float* __restrict__ pmask, const float* __restrict__ gmask,
                                                                const double* __restrict__ coef, int ch, float* __restrict__ cot,
                                                                double* __restrict__ slabs, int64_t CP, int64_t P) {
  const int b = blockIdx.y;
  const double alpha = coef[b * 2 + 0], sigma = coef[b * 2 + 1];
  const int64_t base = (int64_t)b * CP, lo = (int64_t)ch * P, hi = lo + P;
  double acc[1] = {0.0};
  MD_STREAM4(i, CP) {
    f32x4 rv = {0.f, 0.f, 0.f, 0.f};
    if (i >= lo && i < hi) {                    // P % 4 == 0: four values never straddle two channels
      const int64_t p = i - lo;
      const f32x4 xv = md_load4(x + base + i), ev = md_load4(eps + base + i);
      const f32x4 yv = md_load4(src + (int64_t)b * src_bstride + p), pv = md_load4(pmask + p);
      const f32x4 mv = md_mask4(gmask, p);
      double t[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double x0 = ((double)xv[e] - sigma * (double)ev[e]) / alpha;
        rv[e] = (float)(((double)pv[e] * (double)mv[e]) * (x0 - (double)yv[e]));
        t[e] = (double)rv[e] * (double)rv[e];
      }
      acc[0] += (t[0] + t[1]) + (t[2] + t[3]);
    }
    md_store4(cot + base + i, rv);
  }
  if (md_block_sum(acc)) slabs[(int64_t)b * MD_LANGEVIN_SLABS + blockIdx.x] = acc[0];
}

// launch 2, in place: coef[b] = {alpha, sigma, zeta} as doubles.  Prologue: n_b = sqrt(slabs[b][0] + slabs[b][1] + ...) in
// ascending order, k_b = zeta/(alpha*n_b), exactly 0 where n_b == 0 (nothing visible: no step), NaN where n_b is NaN.
//   d = (k_b*(cot - sigma*g))*gm = zeta * d||r||/dx, formed in double
// F64 false: d rounded to float once, x = fl(x - d), x_mean (may be NULL) likewise from the same d.
// F64 true (the DDIM sampler's float64 state): x64 -= d with d kept in double, aux = float(x64), the next U-Net input.
template <bool F64>
__global__ __launch_bounds__(256) void md_guide_apply_kernel(void* __restrict__ state, float* __restrict__ aux,
                                                             const float* __restrict__ cot, const float* __restrict__ g,
                                                             const float* __restrict__ gmask, const double* __restrict__ coef,
                                                             const double* __restrict__ slabs, int64_t CP, int64_t P) {
  const int b = blockIdx.y;
  __shared__ double s_slab[MD_LANGEVIN_SLABS];
  __shared__ double s_k;
  if (threadIdx.x < MD_LANGEVIN_SLABS) s_slab[threadIdx.x] = slabs[(int64_t)b * MD_LANGEVIN_SLABS + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int s = 0; s < MD_LANGEVIN_SLABS; ++s) sum += s_slab[s];
    const double n = sqrt(sum);
    s_k = (n == 0.0) ? 0.0 : coef[b * 3 + 2] / (coef[b * 3 + 0] * n);
  }
  __syncthreads();
  const double k = s_k, sigma = coef[b * 3 + 1];
  const int64_t base = (int64_t)b * CP;
  MD_STREAM4(i, CP) {
    const f32x4 cv = md_load4(cot + base + i), gv = md_load4(g + base + i);
    const f32x4 mv = md_mask4(gmask, i % P);
    double d[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = (k * ((double)cv[e] - sigma * (double)gv[e])) * (double)mv[e];
    if constexpr (F64) {
      double* x64 = (double*)state + base + i;
      f64x4 xv = md_load4(x64);
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[e] -= d[e];
      md_store4(x64, xv);
      md_store4(aux + base + i, f32x4{(float)xv[0], (float)xv[1], (float)xv[2], (float)xv[3]});
    } else {
      float* x32 = (float*)state + base + i;
      f32x4 xv = md_load4(x32);
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[e] -= (float)d[e];
      md_store4(x32, xv);
      if (aux) {
        f32x4 xm = md_load4(aux + base + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) xm[e] -= (float)d[e];
        md_store4(aux + base + i, xm);
      }
    }
  }
}

// ---- multistep exponential-integrator update (DPM-Solver++, Lu et al. 2022; ODE and SDE variants), one launch ----------------
// coef[b] = {alpha_s, sigma_s, c_x, c_0, c_1, c_2, c_z, unused} as doubles, formed by the host from the half-log-SNR of the two
// levels (sampling.dpmpp_tables).  Everything in double, in this order:
//   x0 = (x - sigma_s*eps)/alpha_s ; x_new = c_x*x + c_0*x0 [+ c_1*h1] [+ c_2*h2] [+ c_z*z]    (added left to right)
// then both times the grid mask, then on channel `ch` the replacement v*(1-pm) + partial*pm: the order of md_ddim_step.
// x0 enters x_new as formed, before the mask; x0_out is the masked and replaced one, which the caller keeps as h1 / h2.
// NH: how many earlier predictions are read; Z, MASK, REP: whether z / mask / partial+pmask are: an absent operand costs no load.
// Four values per thread and trip, 16-byte loads and stores; the row is uniform per workgroup (scalar loads).
template <int NH, bool Z, bool MASK, bool REP>
__global__ __launch_bounds__(256) void md_multistep_step_kernel(const double* __restrict__ x, const float* __restrict__ eps,
                                                                const double* __restrict__ h1, const double* __restrict__ h2,
                                                                const float* __restrict__ z, const float* __restrict__ mask,
                                                                const double* __restrict__ coef, const float* __restrict__ partial,
                                                                const float* __restrict__ pmask, int ch, double* __restrict__ x_out,
                                                                double* __restrict__ x0_out, float* __restrict__ x_f32, int64_t CP,
                                                                int64_t P) {
  const int b = blockIdx.y;
  const double* row = coef + (int64_t)b * 8;
  const double alpha = row[0], sigma = row[1], cx = row[2], c0 = row[3], c1 = row[4], c2 = row[5], cz = row[6];
  const int64_t base = (int64_t)b * CP, lo = (int64_t)ch * P, hi = lo + P;
  MD_STREAM4(i, CP) {
    const f64x4 xv = md_load4(x + base + i);
    const f32x4 ev = md_load4(eps + base + i);
    f64x4 xn, x0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x0[e] = (xv[e] - sigma * (double)ev[e]) / alpha;
      xn[e] = cx * xv[e] + c0 * x0[e];
    }
    if constexpr (NH >= 1) {
      const f64x4 hv = md_load4(h1 + base + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) xn[e] = xn[e] + c1 * hv[e];
    }
    if constexpr (NH >= 2) {
      const f64x4 hv = md_load4(h2 + base + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) xn[e] = xn[e] + c2 * hv[e];
    }
    if constexpr (Z) {
      const f32x4 zv = md_load4(z + base + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) xn[e] = xn[e] + cz * (double)zv[e];
    }
    const int64_t pos = i % P;                  // P % 4 == 0: four values never straddle two channels
    if constexpr (MASK) {
      const f32x4 mv = md_load4(mask + pos);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xn[e] = xn[e] * (double)mv[e];
        x0[e] = x0[e] * (double)mv[e];
      }
    }
    if constexpr (REP) {
      if (i >= lo && i < hi) {
        const f32x4 pm = md_load4(pmask + pos), pv = md_load4(partial + pos);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double m = (double)pm[e], v = (double)pv[e];
          xn[e] = xn[e] * (1.0 - m) + v * m;
          x0[e] = x0[e] * (1.0 - m) + v * m;
        }
      }
    }
    md_store4(x_out + base + i, xn);
    md_store4(x0_out + base + i, x0);
    md_store4(x_f32 + base + i, f32x4{(float)xn[0], (float)xn[1], (float)xn[2], (float)xn[3]});
  }
}

// ---- spherical interpolation between latents (reference lib/diffusion/evaler.py:63-71 `slerp`), launch 1 -------------------------
// grid (MD_LANGEVIN_SLABS, pairs): workgroup (s, p) writes slabs[p][s] = {sum a*b, sum a*a, sum b*b, 0} over its strided share of
// pair p, of the masked values.  A product of two floats is exact in double; fixed grid and fixed per-thread order as in
// md_langevin_norms: the partial sums do not depend on scheduling.
__global__ __launch_bounds__(256) void md_slerp_dots_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ mask, double* __restrict__ slabs, int64_t CP,
                                                            int64_t P) {
  const int p = blockIdx.y;
  const int64_t base = (int64_t)p * CP;
  double acc[3] = {0.0, 0.0, 0.0};
  MD_STREAM4(i, CP) {
    const f32x4 av = md_load4(a + base + i), bv = md_load4(b + base + i);
    const f32x4 mv = md_mask4(mask, i % P);
    double ab[4], aa[4], bb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double x = (double)av[e] * (double)mv[e], y = (double)bv[e] * (double)mv[e];
      ab[e] = x * y;
      aa[e] = x * x;
      bb[e] = y * y;
    }
    acc[0] += (ab[0] + ab[1]) + (ab[2] + ab[3]);
    acc[1] += (aa[0] + aa[1]) + (aa[2] + aa[3]);
    acc[2] += (bb[0] + bb[1]) + (bb[2] + bb[3]);
  }
  if (md_block_sum(acc)) {
    double* row = slabs + ((int64_t)p * MD_LANGEVIN_SLABS + blockIdx.x) * 4;      // 8-byte aligned: one double at a time
    row[0] = acc[0];
    row[1] = acc[1];
    row[2] = acc[2];
    row[3] = 0.0;
  }
}

// launch 2.  Prologue, in double: the pair's slabs added in ascending order (thread 0), c = sum ab / (sqrt(sum aa)*sqrt(sum bb))
// clamped to [-1, 1] by comparisons (a NaN stays a NaN), theta = acos(c); thread k < K then forms
//   w1_k = sin((1-alpha_k) theta)/sin(theta), w2_k = sin(alpha_k theta)/sin(theta)      (evaler.py:67-70)
// or, where (1-c)(1+c) = sin^2(theta) < 2^-40 (parallel or antiparallel endpoints, where the reference divides 0 by 0),
//   w1_k = 1-alpha_k, w2_k = alpha_k.
// alpha = 0 gives w = (1, 0) and alpha = 1 gives (0, 1) exactly, because sin(theta)/sin(theta) is 1 and sin(0) is 0: the endpoints
// need no branch.  Then out[p][k] = float((w1_k*a + w2_k*b)*mask), formed in double and rounded once: a and b are read once for all K.
static_assert(MD_SLERP_MAX_K <= 256, "the prologue forms one weight pair per thread of a workgroup");

__global__ __launch_bounds__(256) void md_slerp_mix_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ mask, const double* __restrict__ slabs,
                                                           const double* __restrict__ alpha, int K, float* __restrict__ out,
                                                           double* __restrict__ theta_out, int64_t CP, int64_t P) {
  const int p = blockIdx.y;
  __shared__ double s_slab[MD_LANGEVIN_SLABS][3];
  __shared__ double s_theta;
  __shared__ int s_linear;
  __shared__ double s_w[MD_SLERP_MAX_K][2];
  if (threadIdx.x < MD_LANGEVIN_SLABS) {
    const double* row = slabs + ((int64_t)p * MD_LANGEVIN_SLABS + threadIdx.x) * 4;
    s_slab[threadIdx.x][0] = row[0];
    s_slab[threadIdx.x][1] = row[1];
    s_slab[threadIdx.x][2] = row[2];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int s = 0; s < MD_LANGEVIN_SLABS; ++s) {
      ab += s_slab[s][0];
      aa += s_slab[s][1];
      bb += s_slab[s][2];
    }
    double c = ab / (sqrt(aa) * sqrt(bb));
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double theta = acos(c);
    s_theta = theta;
    s_linear = ((1.0 - c) * (1.0 + c) < 0x1p-40) ? 1 : 0;
    if (blockIdx.x == 0 && theta_out) theta_out[p] = theta;
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    const double al = alpha[threadIdx.x], theta = s_theta;
    double w1 = 1.0 - al, w2 = al;
    if (!s_linear) {
      const double st = sin(theta);
      w1 = sin((1.0 - al) * theta) / st;
      w2 = sin(al * theta) / st;
    }
    s_w[threadIdx.x][0] = w1;
    s_w[threadIdx.x][1] = w2;
  }
  __syncthreads();
  const int64_t base = (int64_t)p * CP;
  float* po = out + (int64_t)p * K * CP;
  MD_STREAM4(i, CP) {
    const f32x4 av = md_load4(a + base + i), bv = md_load4(b + base + i);
    const f32x4 mv = md_mask4(mask, i % P);
    for (int k = 0; k < K; ++k) {
      const double w1 = s_w[k][0], w2 = s_w[k][1];
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (float)((w1 * (double)av[e] + w2 * (double)bv[e]) * (double)mv[e]);
      md_store4(po + (int64_t)k * CP + i, v);
    }
  }
}

// ---- classifier-free guidance: combine the two halves of a doubled evaluation, optional guidance rescale ------------------------
// up to four values of a row of n at i: one vector load where the rows are 16-byte aligned (n % 4 == 0), else one value at a time;
// a slot past the end reads as zero and is neither stored nor summed
static __device__ __forceinline__ f32x4 md_load4_of(const float* row, int64_t i, int64_t n, bool vec) {
  if (vec) return md_load4(row + i);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < n) v[e] = row[i + e];
  return v;
}
static __device__ __forceinline__ void md_store4_of(float* row, int64_t i, int64_t n, bool vec, f32x4 v) {
  if (vec) {
    md_store4(row + i, v);
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < n) row[i + e] = v[e];
}

// grid (S, B): workgroup (s, b) combines its strided share of sample b, out = fmaf(w_b, ec - eu, eu) (an explicit fma: this file
// contracts nothing by itself), and with slabs (then S = MD_LANGEVIN_SLABS) writes slabs[b][s] = {sum ec, sum ec^2, sum out,
// sum out^2}: terms and sums in double, four values as (t0 + t1) + (t2 + t3), then md_block_sum -- a fixed order.
__global__ __launch_bounds__(256) void md_cfg_combine_kernel(const float* __restrict__ eps2, const float* __restrict__ w,
                                                             float* __restrict__ out, double* __restrict__ slabs, int B, int64_t n,
                                                             int vec) {
  const int b = blockIdx.y;
  const float wb = w[b];
  const float* ec = eps2 + (int64_t)b * n;
  const float* eu = eps2 + ((int64_t)B + b) * n;
  float* po = out + (int64_t)b * n;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  MD_STREAM4(i, n) {
    const f32x4 cv = md_load4_of(ec, i, n, vec), uv = md_load4_of(eu, i, n, vec);
    f32x4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = fmaf(wb, cv[e] - uv[e], uv[e]);
    md_store4_of(po, i, n, vec, ov);
    if (slabs) {
      double c[4], o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = i + e < n;
        c[e] = in ? (double)cv[e] : 0.0;
        o[e] = in ? (double)ov[e] : 0.0;
      }
      acc[0] += (c[0] + c[1]) + (c[2] + c[3]);
      acc[1] += (c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3]);
      acc[2] += (o[0] + o[1]) + (o[2] + o[3]);
      acc[3] += (o[0] * o[0] + o[1] * o[1]) + (o[2] * o[2] + o[3] * o[3]);
    }
  }
  if (slabs && md_block_sum(acc)) {
    double* row = slabs + ((int64_t)b * MD_LANGEVIN_SLABS + blockIdx.x) * 4;      // 8-byte aligned: one double at a time
    row[0] = acc[0];
    row[1] = acc[1];
    row[2] = acc[2];
    row[3] = acc[3];
  }
}

// guidance rescale.  Prologue: the sample's slabs added in ascending order (thread 0), mean = sum/n, var = sum2/n - mean^2 for ec and
// out, f = phi*sqrt(var_ec/var_out) + (1 - phi) in double.  A var_out at or below 2^-40 of out's mean square counts as zero: below
// that the double sums cannot tell a spread from their own rounding (a constant sample comes out there, not at exactly 0).  Such a
// sample, and one whose f is not finite, keeps its values and reports f = 1.  Then out *= (float)f.
__global__ __launch_bounds__(256) void md_cfg_rescale_kernel(float* __restrict__ out, const double* __restrict__ slabs, double phi,
                                                             double* __restrict__ factor_out, int64_t n, int vec) {
  const int b = blockIdx.y;
  __shared__ double s_slab[MD_LANGEVIN_SLABS][4];
  __shared__ float s_f;
  __shared__ int s_keep;
  if (threadIdx.x < MD_LANGEVIN_SLABS) {
    const double* row = slabs + ((int64_t)b * MD_LANGEVIN_SLABS + threadIdx.x) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) s_slab[threadIdx.x][k] = row[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < MD_LANGEVIN_SLABS; ++j) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += s_slab[j][k];
    }
    const double dn = (double)n;
    const double mc = s[0] / dn, mo = s[2] / dn, msc = s[1] / dn, mso = s[3] / dn;
    const double vc = msc - mc * mc, vo = mso - mo * mo;
    double f = phi * sqrt(vc / vo) + (1.0 - phi);
    const bool keep = !(vo > 0x1p-40 * mso) || !(f == f) || f - f != 0.0;      // zero spread, NaN, inf
    if (keep) f = 1.0;
    s_f = (float)f;
    s_keep = keep ? 1 : 0;
    if (blockIdx.x == 0 && factor_out) factor_out[b] = f;
  }
  __syncthreads();
  if (s_keep) return;
  const float f = s_f;
  float* po = out + (int64_t)b * n;
  MD_STREAM4(i, n) {
    f32x4 v = md_load4_of(po, i, n, vec);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] * f;
    md_store4_of(po, i, n, vec, v);
  }
}

// ---- exports ------------------------------------------------------------------------------------------------------------
// The tail of an export: one launch of 256-thread workgroups on `stream`, the export's last parameter.
#define MD_LAUNCH_STEP(kernel, grid, ...)                                                       \
  do {                                                                                          \
    MD_HIP_CLEAR_ERROR();                                                                       \
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);           \
    MD_HIP_CHECK_LAUNCH();                                                                      \
    return MD_OK;                                                                               \
  } while (0)

extern "C" int md_ancestral_step(const float* x, const float* eps, const float* z, const float* mask,
                                 const float* coef, float* x_out, float* x_mean_out, int32_t batch,
                                 int32_t C, int64_t P, void* stream) {
  if (md_any_bad<16>(x, eps, z, x_out, x_mean_out) || md_any_bad<4>(coef) || md_any_misaligned<16>(mask)) return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, true)) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P;
  MD_LAUNCH_STEP(md_ancestral_step_kernel, dim3(md_grid_x(CP / 4, 2048), (unsigned)batch), x, eps, z, mask, coef, x_out,
                 x_mean_out, CP, P);
}

extern "C" int md_ddim_step(const double* x, const float* eps, const float* mask, const double* coef, const float* partial,
                            const float* pmask, int32_t ch, double* x_out, double* x0_out, float* x_f32, int32_t batch,
                            int32_t C, int64_t P, void* stream) {
  if (md_any_bad<8>(x, coef, x_out, x0_out) || md_any_bad<4>(eps, x_f32) || md_any_misaligned<4>(mask, partial, pmask))
    return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, false)) return MD_ERR_BAD_ARG;
  if ((partial != nullptr) != (pmask != nullptr) || (partial != nullptr && (ch < 0 || ch >= C))) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P;
  MD_LAUNCH_STEP(md_ddim_step_kernel, dim3(md_grid_x(CP, 4096), (unsigned)batch), x, eps, mask, coef, partial, pmask, ch, x_out,
                 x0_out, x_f32, CP, P);
}

extern "C" int md_inpaint_blend(float* x, const float* src, const float* pmask, const float* gmask,
                                int32_t batch, int32_t C, int32_t ch, int64_t P, int64_t src_bstride,
                                void* stream) {
  if (md_any_bad<4>(x, src, pmask) || md_any_misaligned<4>(gmask)) return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, false) || ch < 0 || ch >= C) return MD_ERR_BAD_ARG;
  MD_LAUNCH_STEP(md_inpaint_blend_kernel, dim3(md_grid_x(P, 1024), (unsigned)batch), x, src, pmask, gmask, C, ch, P, src_bstride);
}

extern "C" int md_inpaint_renoise(float* x, float* x_mean, const float* z, const float* pmask,
                                  const float* gmask, const float* coef, int32_t batch, int32_t C,
                                  int32_t ch, int64_t P, void* stream) {
  if (md_any_bad<4>(x, z, pmask, coef) || md_any_misaligned<4>(x_mean, gmask)) return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, false) || ch < 0 || ch >= C) return MD_ERR_BAD_ARG;
  MD_LAUNCH_STEP(md_inpaint_renoise_kernel, dim3(md_grid_x(P, 1024), (unsigned)batch), x, x_mean, z, pmask, gmask, coef, C, ch, P);
}

extern "C" int md_langevin_norms(const float* eps, const float* z, int32_t batch, int32_t C, int64_t P, double* slabs,
                                 void* stream) {
  if (md_any_bad<16>(eps, z, slabs)) return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, true)) return MD_ERR_BAD_ARG;
  MD_LAUNCH_STEP(md_langevin_norms_kernel, dim3(MD_LANGEVIN_SLABS, (unsigned)batch), eps, z, slabs, (int64_t)C * P);
}

extern "C" int md_langevin_step(const float* x, const float* eps, const float* z, const float* mask, const float* coef,
                                const double* slabs, float snr, int32_t mode, float* x_out, float* x_mean_out,
                                float* step_out, int32_t batch, int32_t C, int64_t P, void* stream) {
  if (md_any_bad<16>(x, eps, z, x_out, x_mean_out) || md_any_bad<4>(coef, step_out) || md_any_misaligned<16>(mask, slabs))
    return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, true)) return MD_ERR_BAD_ARG;
  if (mode != MD_CORRECTOR_LANGEVIN && mode != MD_CORRECTOR_ALD) return MD_ERR_BAD_ARG;
  if (mode == MD_CORRECTOR_LANGEVIN && !slabs) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P;
  MD_LAUNCH_STEP(md_langevin_step_kernel, dim3(stream_blocks(CP, batch), (unsigned)batch), x, eps, z, mask, coef, slabs, snr,
                 (int)mode, x_out, x_mean_out, step_out, (int)batch, CP, P);
}

extern "C" int md_sde_step(const float* x, const float* eps, const float* z, const float* mask, const float* coef,
                           int32_t kind, float* x_out, float* x_mean_out, int32_t batch, int32_t C, int64_t P, void* stream) {
  if (md_any_bad<16>(x, eps, z, x_out, x_mean_out) || md_any_bad<4>(coef) || md_any_misaligned<16>(mask)) return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, true)) return MD_ERR_BAD_ARG;
  if (kind != MD_SDE_REVERSE_DIFFUSION && kind != MD_SDE_EULER_MARUYAMA) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P;
  MD_LAUNCH_STEP(md_sde_step_kernel, dim3(stream_blocks(CP, batch), (unsigned)batch), x, eps, z, mask, coef, (int)kind, x_out,
                 x_mean_out, CP, P);
}

extern "C" int md_pf_ode_rhs(const float* x, const float* eps_hat, const float* g, const float* probe, const float* mask,
                             const double* coef, float* drift, double* slabs, int32_t batch, int32_t C, int64_t P, void* stream) {
  if (md_any_bad<16>(x, eps_hat, drift) || md_any_bad<8>(coef) || md_any_misaligned<16>(g, probe, mask) ||
      md_any_misaligned<8>(slabs))
    return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, true)) return MD_ERR_BAD_ARG;
  if ((g == nullptr) != (probe == nullptr) || (g && !slabs)) return MD_ERR_BAD_ARG;     // the divergence needs both, and its slabs
  const int64_t CP = (int64_t)C * P;
  if (g)
    MD_LAUNCH_STEP(md_pf_ode_rhs_kernel<true>, dim3(MD_LANGEVIN_SLABS, (unsigned)batch), x, eps_hat, g, probe, mask, coef, drift,
                   slabs, CP, P);
  MD_LAUNCH_STEP(md_pf_ode_rhs_kernel<false>, dim3(stream_blocks(CP, batch), (unsigned)batch), x, eps_hat, g, probe, mask, coef,
                 drift, slabs, CP, P);
}

extern "C" int md_guide_residual(const float* x, const float* eps_hat, const float* src, int64_t src_bstride, const float* pmask,
                                 const float* gmask, const double* coef, int32_t ch, float* cot, double* slabs, int32_t batch,
                                 int32_t C, int64_t P, void* stream) {
  if (md_any_bad<16>(x, eps_hat, src, pmask, cot) || md_any_bad<8>(coef, slabs) || md_any_misaligned<16>(gmask))
    return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, true)) return MD_ERR_BAD_ARG;
  if (ch < 0 || ch >= C || (src_bstride != 0 && src_bstride != P)) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P, n = 4 * CP * batch, np = 4 * P, ns = src_bstride ? np * batch : np;
  const md_span out[] = {{cot, n}, {slabs, 8LL * MD_LANGEVIN_SLABS * batch}};
  const md_span in[] = {{x, n}, {eps_hat, n}, {src, ns}, {pmask, np}, {gmask, np}, {coef, 16LL * batch}};
  if (md_any_alias(out, in)) return MD_ERR_BAD_ARG;
  MD_LAUNCH_STEP(md_guide_residual_kernel, dim3(MD_LANGEVIN_SLABS, (unsigned)batch), x, eps_hat, src, src_bstride, pmask, gmask,
                 coef, (int)ch, cot, slabs, CP, P);
}

// the checks and the launch of both md_guide_apply exports: the state is float with x_mean as `aux`, or double with x_f32
template <bool F64>
static int md_guide_apply(void* state, float* aux, const float* cot, const float* g, const float* gmask, const double* coef,
                          const double* slabs, int32_t batch, int32_t C, int64_t P, void* stream) {
  if (md_any_bad<16>(state, cot, g) || md_any_bad<8>(coef, slabs) || md_any_misaligned<16>(aux, gmask)) return MD_ERR_BAD_ARG;
  if (F64 && !aux) return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, true)) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P, n = 4 * CP * batch;
  const md_span out[] = {{state, (F64 ? 8 : 4) * CP * batch}, {aux, n}};
  const md_span in[] = {{cot, n}, {g, n}, {gmask, 4 * P}, {coef, 24LL * batch}, {slabs, 8LL * MD_LANGEVIN_SLABS * batch}};
  if (md_any_alias(out, in)) return MD_ERR_BAD_ARG;
  MD_LAUNCH_STEP(md_guide_apply_kernel<F64>, dim3(stream_blocks(CP, batch), (unsigned)batch), state, aux, cot, g, gmask, coef,
                 slabs, CP, P);
}

extern "C" int md_guide_apply_f32(float* x, float* x_mean, const float* cot, const float* g, const float* gmask, const double* coef,
                                  const double* slabs, int32_t batch, int32_t C, int64_t P, void* stream) {
  return md_guide_apply<false>(x, x_mean, cot, g, gmask, coef, slabs, batch, C, P, stream);
}

extern "C" int md_guide_apply_f64(double* x64, float* x_f32, const float* cot, const float* g, const float* gmask,
                                  const double* coef, const double* slabs, int32_t batch, int32_t C, int64_t P, void* stream) {
  return md_guide_apply<true>(x64, x_f32, cot, g, gmask, coef, slabs, batch, C, P, stream);
}

template <int NH, bool Z>
static void md_multistep_launch(bool has_mask, bool rep, dim3 grid, hipStream_t s, const double* x, const float* eps, const double* h1,
                                const double* h2, const float* z, const float* mask, const double* coef, const float* partial,
                                const float* pmask, int ch, double* x_out, double* x0_out, float* x_f32, int64_t CP, int64_t P) {
#define MD_MULTISTEP_GO(M, R)                                                                                                \
  hipLaunchKernelGGL((md_multistep_step_kernel<NH, Z, M, R>), grid, dim3(256), 0, s, x, eps, h1, h2, z, mask, coef, partial, \
                     pmask, ch, x_out, x0_out, x_f32, CP, P)
  if (has_mask && rep) MD_MULTISTEP_GO(true, true);
  else if (has_mask) MD_MULTISTEP_GO(true, false);
  else if (rep) MD_MULTISTEP_GO(false, true);
  else MD_MULTISTEP_GO(false, false);
#undef MD_MULTISTEP_GO
}

extern "C" int md_multistep_step(const double* x, const float* eps, const double* h1, const double* h2, const float* z,
                                 const float* mask, const double* coef, const float* partial, const float* pmask, int32_t ch,
                                 double* x_out, double* x0_out, float* x_f32, int32_t batch, int32_t C, int64_t P, void* stream) {
  if (md_any_bad<16>(x, eps, x_out, x0_out, x_f32) || md_any_bad<8>(coef) || md_any_misaligned<16>(h1, h2, z, mask, partial, pmask))
    return MD_ERR_BAD_ARG;
  if (md_bad_dims(batch, C, P, true)) return MD_ERR_BAD_ARG;
  if (ch < 0 || ch >= C || (partial == nullptr) != (pmask == nullptr) || (h2 && !h1)) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P, n4 = 4 * CP * batch, n8 = 8 * CP * batch, np = 4 * P;
  const md_span out[] = {{x_out, n8}, {x0_out, n8}, {x_f32, n4}};
  const md_span in[] = {{x, n8}, {eps, n4}, {h1, n8}, {h2, n8}, {z, n4}, {mask, np}, {coef, 64LL * batch}, {partial, np}, {pmask, np}};
  if (md_any_alias(out, in)) return MD_ERR_BAD_ARG;
  const dim3 grid(stream_blocks(CP, batch), (unsigned)batch);
  const bool m = mask != nullptr, r = partial != nullptr;
  hipStream_t s = (hipStream_t)stream;
  MD_HIP_CLEAR_ERROR();
#define MD_MULTISTEP_ARGS m, r, grid, s, x, eps, h1, h2, z, mask, coef, partial, pmask, (int)ch, x_out, x0_out, x_f32, CP, P
  if (h2) z ? md_multistep_launch<2, true>(MD_MULTISTEP_ARGS) : md_multistep_launch<2, false>(MD_MULTISTEP_ARGS);
  else if (h1) z ? md_multistep_launch<1, true>(MD_MULTISTEP_ARGS) : md_multistep_launch<1, false>(MD_MULTISTEP_ARGS);
  else z ? md_multistep_launch<0, true>(MD_MULTISTEP_ARGS) : md_multistep_launch<0, false>(MD_MULTISTEP_ARGS);
#undef MD_MULTISTEP_ARGS
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_slerp_dots(const float* a, const float* b, const float* mask, int32_t pairs, int32_t C, int64_t P, double* slabs,
                             void* stream) {
  if (md_any_bad<16>(a, b) || md_any_bad<8>(slabs) || md_any_misaligned<16>(mask)) return MD_ERR_BAD_ARG;
  if (md_bad_dims(pairs, C, P, true)) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P, n = 4 * CP * pairs;
  const md_span out[] = {{slabs, 32LL * MD_LANGEVIN_SLABS * pairs}};
  const md_span in[] = {{a, n}, {b, n}, {mask, 4 * P}};
  if (md_any_alias(out, in)) return MD_ERR_BAD_ARG;
  MD_LAUNCH_STEP(md_slerp_dots_kernel, dim3(MD_LANGEVIN_SLABS, (unsigned)pairs), a, b, mask, slabs, CP, P);
}

extern "C" int md_slerp_mix(const float* a, const float* b, const float* mask, const double* slabs, const double* alpha, int32_t K,
                            float* out, double* theta_out, int32_t pairs, int32_t C, int64_t P, void* stream) {
  if (md_any_bad<16>(a, b, out) || md_any_bad<8>(slabs, alpha) || md_any_misaligned<16>(mask) || md_any_misaligned<8>(theta_out))
    return MD_ERR_BAD_ARG;
  if (md_bad_dims(pairs, C, P, true) || K < 1 || K > MD_SLERP_MAX_K) return MD_ERR_BAD_ARG;
  const int64_t CP = (int64_t)C * P, n = 4 * CP * pairs;
  const md_span outs[] = {{out, n * K}, {theta_out, 8LL * pairs}};
  const md_span in[] = {{a, n}, {b, n}, {mask, 4 * P}, {slabs, 32LL * MD_LANGEVIN_SLABS * pairs}, {alpha, 8LL * K}};
  if (md_any_alias(outs, in)) return MD_ERR_BAD_ARG;
  MD_LAUNCH_STEP(md_slerp_mix_kernel, dim3(stream_blocks(CP, pairs), (unsigned)pairs), a, b, mask, slabs, alpha, (int)K, out,
                 theta_out, CP, P);
}

extern "C" int md_cfg_combine(const float* eps2, const float* w, int32_t batch, int64_t n, float* out, double* slabs, void* stream) {
  const bool vec = n > 0 && n % 4 == 0;
  if (vec ? md_any_bad<16>(eps2, out) : md_any_bad<4>(eps2, out)) return MD_ERR_BAD_ARG;
  if (md_any_bad<4>(w) || md_any_misaligned<8>(slabs)) return MD_ERR_BAD_ARG;
  if (batch < 1 || n < 1) return MD_ERR_BAD_ARG;
  const int64_t bytes = 4 * n * batch;
  const md_span outs[] = {{out, bytes}, {slabs, 32LL * MD_LANGEVIN_SLABS * batch}};
  const md_span in[] = {{eps2, 2 * bytes}, {w, 4LL * batch}};
  if (md_any_alias(outs, in)) return MD_ERR_BAD_ARG;
  const unsigned gx = slabs ? (unsigned)MD_LANGEVIN_SLABS : stream_blocks(n + 3, batch);
  MD_LAUNCH_STEP(md_cfg_combine_kernel, dim3(gx, (unsigned)batch), eps2, w, out, slabs, (int)batch, n, vec ? 1 : 0);
}

extern "C" int md_cfg_rescale(float* out, const double* slabs, double phi, double* factor_out, int32_t batch, int64_t n,
                              void* stream) {
  const bool vec = n > 0 && n % 4 == 0;
  if (vec ? md_any_bad<16>(out) : md_any_bad<4>(out)) return MD_ERR_BAD_ARG;
  if (md_any_bad<8>(slabs) || md_any_misaligned<8>(factor_out)) return MD_ERR_BAD_ARG;
  if (batch < 1 || n < 1 || !(phi >= 0.0 && phi <= 1.0)) return MD_ERR_BAD_ARG;
  const md_span outs[] = {{out, 4 * n * batch}, {factor_out, 8LL * batch}};
  const md_span in[] = {{slabs, 32LL * MD_LANGEVIN_SLABS * batch}};
  if (md_any_alias(outs, in)) return MD_ERR_BAD_ARG;
  MD_LAUNCH_STEP(md_cfg_rescale_kernel, dim3(stream_blocks(n + 3, batch), (unsigned)batch), out, slabs, phi, factor_out, n,
                 vec ? 1 : 0);
}
