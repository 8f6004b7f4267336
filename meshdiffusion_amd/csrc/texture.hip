// Textures for meshes: the bilinear fetch with its two gradients, one dilation step of a baked atlas and the multi-view projection
// bake: what nvdiffrec/lib/render/texture.py (Texture2D.sample = dr.texture with filter_mode = 'linear', no mip levels) and
// render.py:render_uv give the reference's eval.py and fit_singleview.py when they write mesh.obj + mesh.mtl + texture_kd.png.
//
// THE TEXTURE CONTRACT (tests/texture_cases.py restates it in numpy: fp32 in this order, and float64)
//   Inputs     tex float32 [T][Ht][Wt][C], T = 1 (shared by the views) or B, 1 <= C <= 8, 1 <= Ht, Wt <= 2048; uv float32
//              [B][H][W][2]; rast float32 [B][H][W][4] one layer of the rasteriser, optional.  The limits on B, H, W are those of
//              the rasterisation contract (csrc/raster.hip); anything else is MD_ERR_UNSUPPORTED.
//   Skipped    a pixel whose rast id (channel 3) is 0 when rast is given, and a pixel whose x or y below is not finite (u or v
//              NaN or inf, or so large that u Wt overflows).  A skipped pixel outputs C zeros and contributes nothing to any gradient.
//   Texels     the centre of texel (row i, column j) is (u, v) = ((j + 0.5) / Wt, (i + 0.5) / Ht): row 0 is v = 0, the orientation
//              of a rasterisation at the clip position (2 u - 1, 2 v - 1, 0, 1), so a baked texel and a sampled texel coincide.
//   Value      fp32, every operation rounded on its own (no contraction):
//                x = u * Wt - 0.5f, x0 = floor(x), fx = x - x0; y, y0, fy likewise with v and Ht;
//                out[c] = (t00 * (1 - fx) + t10 * fx) * (1 - fy) + (t01 * (1 - fx) + t11 * fx) * fy,
//              t_ab = tex[iy_b][ix_a][c] with ix_0, ix_1 from x0, x0 + 1 and iy_0, iy_1 from y0, y0 + 1 by the boundary mode.
//   Boundary   clamp (0): each index is clamped to [0, size - 1].  wrap (1): ix_0 = x0 modulo the size, negative x0 included (-1
//              is size - 1), exact for every finite x0 (fmodf), and ix_1 = ix_0 + 1, or 0 when that is the size: (x0 + 1) modulo the
//              size wherever x0 + 1 is an fp32 number, and the definition beyond (|x0| >= 2^24, where fx = 0 anyway); y likewise.
//   Corners    corner k = 0..3 of a pixel is (t00, t10, t01, t11) with the weights w = ((1-fx)(1-fy), fx (1-fy), (1-fx) fy, fx fy),
//              each one fp32 product.  The code of a (pixel, corner) is 4 * pixel + k, pixel = (b H + i) W + j.
//   d tex      corner k of a pixel that is not skipped contributes w_k * g[pixel][c] to its texel (of texture b when T == B, of
//              the one texture otherwise).  Summed per texel in ascending code order, a compensated (Kahan) fp32 sum as
//              md_kahan_add (csrc/md_gather.h).  Two corners that clamping sends to one texel are two terms.  Every element of
//              d tex is written; a texel nobody sampled gets 0.
//   d uv       du = Wt * sum_c g[c] ((t10 - t00) (1 - fy) + (t11 - t01) fy), dv = Ht * sum_c g[c] ((t01 - t00) (1 - fx) +
//              (t11 - t10) fx), plain fp32 sums in ascending c; zero where clamping made the two texels one; (0, 0) where skipped.
//   Dilation   one step over tex float32 [Ht][Wt][C] and mask float32 [Ht][Wt] (covered: mask > 0.5): a texel that is not covered
//              and has at least one covered 8-neighbour inside the texture becomes the sum of those neighbours, taken in row-major
//              order (dy = -1, 0, 1 outside, dx = -1, 0, 1 inside), divided by their count, and its mask becomes 1; every other
//              texel and mask value is copied.  out must not alias in.
//   Projection per texel with texmask > 0.5, position p, unit normal n, over the views v = 0 .. V - 1 in ascending order, V <= 64:
//                clip = ((p.x m0 + p.y m1) + p.z m2) + m3, m_k the columns of mvp_v (the order of xfm_points); skip unless w > 0;
//                ndc = clip.xy / w; skip unless both lie in [-1, 1];
//                px = (ndc.x * 0.5f + 0.5f) * W - 0.5f, x0 = floor(px), fx = px - x0; py, y0, fy likewise with H; skip unless
//                the four pixels (x0 | x0 + 1, y0 | y0 + 1) lie inside the image and have viewmask > 0.5;
//                d = sqrt((dx dx + dy dy) + dz dz), (dx, dy, dz) = campos_v - p; skip if d - depth_v[floor(py + 0.5)][floor(px +
//                0.5)] > depth_bias;  cos = ((n.x dx + n.y dy) + n.z dz) / d; skip unless cos > cos_min;
//                w_v = powf(cos, power); c_v = the bilinear fetch of image_v at (fx, fy) in the order of Value.
//              color = (sum_v w_v c_v) / (sum_v w_v) where the sum of weights is > 0, zeros elsewhere; weight = sum_v w_v; plain
//              fp32 sums.  A texel with texmask <= 0.5 gets zeros.  No gradient.
//
// Kernels.  All streaming, one thread per pixel or texel, no LDS.  md_texture_sample: one 8-byte uv load and one 16-byte rast
// load per pixel, C unrolled at compile time, 16-byte texel loads and stores at C = 4 and C = 8.  The texture gradient is a GATHER
// in a fixed order: md_texture_codes writes the texel row of every code (row T Ht Wt for a skipped pixel), the host sorts them
// stably by row (meshdiffusion_amd/_csr.py), and md_texture_sample_bwd runs one thread per texel over its span of the CSR,
// recomputing w_k from uv inside the row loop, so no 4 C floats per pixel go through memory.  No floating-point atomics anywhere: two
// runs agree bit for bit, forward and backward.
//
// Every export checks, in this order: null or misaligned pointers (MD_ERR_BAD_ARG), sizes and scalars (MD_ERR_BAD_ARG), limits
// (MD_ERR_UNSUPPORTED), aliasing (MD_ERR_BAD_ARG).  Nothing is allocated, nothing synchronises.
#include "md_args.h"
#include "md_gather.h"
#include "md_raster_snap.h"

#pragma clang fp contract(off)

static constexpr int TX_MAX_RES = 2048, TX_MAX_VIEWS = 64;

// index of the float integer `f` (any finite value) in a row of `n` texels
__device__ __forceinline__ int tx_index(float f, int n, int wrap) {
  if (wrap) {
    int r = (int)fmodf(f, (float)n);                           // exact; |r| < n
    return r < 0 ? r + n : r;
  }
  return (int)fminf(fmaxf(f, 0.f), (float)(n - 1));
}

struct TxTap {
  int ix0, ix1, iy0, iy1;
  float fx, fy;
  bool live;
};

// the footprint of a uv under the contract; live == false: skipped
__device__ __forceinline__ TxTap tx_tap(float u, float v, int Ht, int Wt, int wrap) {
  TxTap t;
  const float x = u * (float)Wt - 0.5f, y = v * (float)Ht - 0.5f;
  t.live = __builtin_isfinite(x) && __builtin_isfinite(y);
  const float x0 = t.live ? floorf(x) : 0.f, y0 = t.live ? floorf(y) : 0.f;
  t.fx = t.live ? x - x0 : 0.f;
  t.fy = t.live ? y - y0 : 0.f;
  t.ix0 = tx_index(x0, Wt, wrap);
  t.iy0 = tx_index(y0, Ht, wrap);
  if (wrap) {
    t.ix1 = t.ix0 + 1 == Wt ? 0 : t.ix0 + 1;
    t.iy1 = t.iy0 + 1 == Ht ? 0 : t.iy0 + 1;
  } else {
    t.ix1 = tx_index(x0 + 1.f, Wt, 0);                         // a huge x0 absorbs the + 1 and clamps to the same end either way
    t.iy1 = tx_index(y0 + 1.f, Ht, 0);
  }
  return t;
}

template <int C>
__device__ __forceinline__ void tx_load(const float* __restrict__ p, float (&t)[C]) {
  if constexpr (C == 4 || C == 8) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
      const float4 v4 = *reinterpret_cast<const float4*>(p + 4 * q);
      t[4 * q] = v4.x; t[4 * q + 1] = v4.y; t[4 * q + 2] = v4.z; t[4 * q + 3] = v4.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = p[c];
  }
}

template <int C>
__device__ __forceinline__ void tx_store(float* __restrict__ p, const float (&t)[C]) {
  if constexpr (C == 4 || C == 8) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) *reinterpret_cast<float4*>(p + 4 * q) = make_float4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = t[c];
  }
}

// is pixel o (flat over the views) sampled at all: the rast id, when there is a rast
__device__ __forceinline__ bool tx_covered(const float* __restrict__ rast, int64_t o) {
  if (!rast) return true;
  return (*reinterpret_cast<const float4*>(rast + o * 4)).w != 0.f;
}

template <int C>
__global__ __launch_bounds__(256) void md_texture_sample_kernel(const float* __restrict__ tex, const float* __restrict__ uv,
                                                                const float* __restrict__ rast, int64_t tex_bstride, int Ht, int Wt,
                                                                int HW, int wrap, float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int64_t o = (int64_t)blockIdx.y * HW + p;
  float val[C];
#pragma unroll
  for (int c = 0; c < C; ++c) val[c] = 0.f;
  const float2 q = *reinterpret_cast<const float2*>(uv + o * 2);
  const TxTap t = tx_tap(q.x, q.y, Ht, Wt, wrap);
  if (t.live && tx_covered(rast, o)) {
    const float* T = tex + (int64_t)blockIdx.y * tex_bstride;
    float t00[C], t10[C], t01[C], t11[C];
    tx_load<C>(T + ((int64_t)t.iy0 * Wt + t.ix0) * C, t00);
    tx_load<C>(T + ((int64_t)t.iy0 * Wt + t.ix1) * C, t10);
    tx_load<C>(T + ((int64_t)t.iy1 * Wt + t.ix0) * C, t01);
    tx_load<C>(T + ((int64_t)t.iy1 * Wt + t.ix1) * C, t11);
    const float gx = 1.f - t.fx, gy = 1.f - t.fy;
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = (t00[c] * gx + t10[c] * t.fx) * gy + (t01[c] * gx + t11[c] * t.fx) * t.fy;
  }
  tx_store<C>(out + o * C, val);
}

// dest int32 [B H W][4]: the texel row of every code, `trash` (= T Ht Wt) for the four codes of a skipped pixel
__global__ __launch_bounds__(256) void md_texture_codes_kernel(const float* __restrict__ uv, const float* __restrict__ rast,
                                                               int64_t row_bstride, int Ht, int Wt, int HW, int wrap, int trash,
                                                               int32_t* __restrict__ dest) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int64_t o = (int64_t)blockIdx.y * HW + p;
  const float2 q = *reinterpret_cast<const float2*>(uv + o * 2);
  const TxTap t = tx_tap(q.x, q.y, Ht, Wt, wrap);
  int4 d = make_int4(trash, trash, trash, trash);
  if (t.live && tx_covered(rast, o)) {
    const int base = (int)((int64_t)blockIdx.y * row_bstride);
    d = make_int4(base + t.iy0 * Wt + t.ix0, base + t.iy0 * Wt + t.ix1, base + t.iy1 * Wt + t.ix0, base + t.iy1 * Wt + t.ix1);
  }
  *reinterpret_cast<int4*>(dest + o * 4) = d;
}

template <int C>
__global__ __launch_bounds__(256) void md_texture_duv_kernel(const float* __restrict__ tex, const float* __restrict__ uv,
                                                             const float* __restrict__ rast, const float* __restrict__ gout,
                                                             int64_t tex_bstride, int Ht, int Wt, int HW, int wrap,
                                                             float* __restrict__ duv) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int64_t o = (int64_t)blockIdx.y * HW + p;
  const float2 q = *reinterpret_cast<const float2*>(uv + o * 2);
  const TxTap t = tx_tap(q.x, q.y, Ht, Wt, wrap);
  float du = 0.f, dv = 0.f;
  if (t.live && tx_covered(rast, o)) {
    const float* T = tex + (int64_t)blockIdx.y * tex_bstride;
    float t00[C], t10[C], t01[C], t11[C], g[C];
    tx_load<C>(T + ((int64_t)t.iy0 * Wt + t.ix0) * C, t00);
    tx_load<C>(T + ((int64_t)t.iy0 * Wt + t.ix1) * C, t10);
    tx_load<C>(T + ((int64_t)t.iy1 * Wt + t.ix0) * C, t01);
    tx_load<C>(T + ((int64_t)t.iy1 * Wt + t.ix1) * C, t11);
    tx_load<C>(gout + o * C, g);
    const float gx = 1.f - t.fx, gy = 1.f - t.fy;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      du += g[c] * ((t10[c] - t00[c]) * gy + (t11[c] - t01[c]) * t.fy);
      dv += g[c] * ((t01[c] - t00[c]) * gx + (t11[c] - t10[c]) * t.fx);
    }
    du = (float)Wt * du;
    dv = (float)Ht * dv;
  }
  *reinterpret_cast<float2*>(duv + o * 2) = make_float2(du, dv);
}

// One thread per texel row: the Kahan sum of w_k g[pixel] over the row's codes in the order of the CSR.  A position outside
// [0, n_codes) ends the row and a code outside it is skipped (never with the CSR of the host): nothing outside uv and gout is read.
template <int C>
__global__ __launch_bounds__(256) void md_texture_dtex_kernel(const float* __restrict__ uv, const float* __restrict__ gout,
                                                              const int32_t* __restrict__ ptr, const int32_t* __restrict__ order,
                                                              int64_t rows, int64_t n_codes, int Ht, int Wt,
                                                              float* __restrict__ dtex) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  float acc[C], lost[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { acc[c] = 0.f; lost[c] = 0.f; }
  const int j1 = ptr[row + 1];
  for (int j = ptr[row]; j < j1; ++j) {
    if (j < 0 || j >= n_codes) break;
    const int32_t code = order[j];
    if (code < 0 || code >= n_codes) continue;
    const int64_t o = code >> 2;
    const int k = code & 3;
    const float2 q = *reinterpret_cast<const float2*>(uv + o * 2);
    const float x = q.x * (float)Wt - 0.5f, y = q.y * (float)Ht - 0.5f;      // finite: the code names a texel
    const float fx = x - floorf(x), fy = y - floorf(y);
    const float w = ((k & 1) ? fx : 1.f - fx) * ((k & 2) ? fy : 1.f - fy);
    float g[C];
    tx_load<C>(gout + o * C, g);
#pragma unroll
    for (int c = 0; c < C; ++c) md_kahan_add(acc[c], lost[c], w * g[c]);
  }
  tx_store<C>(dtex + row * C, acc);
}

template <int C>
__global__ __launch_bounds__(256) void md_texture_dilate_kernel(const float* __restrict__ tex, const float* __restrict__ mask, int Ht,
                                                                int Wt, float* __restrict__ out_tex, float* __restrict__ out_mask) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= Ht * Wt) return;
  const int i = p / Wt, j = p - i * Wt;
  const float m = mask[p];
  float val[C];
  tx_load<C>(tex + (int64_t)p * C, val);
  float m_out = m;
  if (!(m > 0.5f)) {
    float sum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = 0.f;
    int n = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int ii = i + dy, jj = j + dx;
        if ((dy == 0 && dx == 0) || ii < 0 || ii >= Ht || jj < 0 || jj >= Wt) continue;
        const int q = ii * Wt + jj;
        if (mask[q] > 0.5f) {
          float t[C];
          tx_load<C>(tex + (int64_t)q * C, t);
#pragma unroll
          for (int c = 0; c < C; ++c) sum[c] += t[c];
          ++n;
        }
      }
    if (n > 0) {
      const float fn = (float)n;
#pragma unroll
      for (int c = 0; c < C; ++c) val[c] = sum[c] / fn;
      m_out = 1.f;
    }
  }
  tx_store<C>(out_tex + (int64_t)p * C, val);
  out_mask[p] = m_out;
}

__global__ __launch_bounds__(256) void md_texture_project_kernel(const float* __restrict__ pos, const float* __restrict__ nrm,
                                                                 const float* __restrict__ texmask, const float* __restrict__ image,
                                                                 const float* __restrict__ depth, const float* __restrict__ viewmask,
                                                                 const float* __restrict__ mvp, const float* __restrict__ campos,
                                                                 int n_texels, int V, int H, int W, float depth_bias, float cos_min,
                                                                 float power, float* __restrict__ color, float* __restrict__ weight) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_texels) return;
  float acc[3] = {0.f, 0.f, 0.f}, wsum = 0.f;
  if (texmask[p] > 0.5f) {
    const float P[3] = {pos[(int64_t)p * 3], pos[(int64_t)p * 3 + 1], pos[(int64_t)p * 3 + 2]};
    const float N[3] = {nrm[(int64_t)p * 3], nrm[(int64_t)p * 3 + 1], nrm[(int64_t)p * 3 + 2]};
    for (int v = 0; v < V; ++v) {
      const float* m = mvp + v * 16;                             // row-major: clip_r = sum_k m[r][k] (p, 1)_k
      const float cx = ((P[0] * m[0] + P[1] * m[1]) + P[2] * m[2]) + m[3];
      const float cy = ((P[0] * m[4] + P[1] * m[5]) + P[2] * m[6]) + m[7];
      const float cw = ((P[0] * m[12] + P[1] * m[13]) + P[2] * m[14]) + m[15];
      if (!(cw > 0.f)) continue;
      const float nx = cx / cw, ny = cy / cw;
      if (!(nx >= -1.f && nx <= 1.f && ny >= -1.f && ny <= 1.f)) continue;
      const float px = (nx * 0.5f + 0.5f) * (float)W - 0.5f, py = (ny * 0.5f + 0.5f) * (float)H - 0.5f;
      const float x0f = floorf(px), y0f = floorf(py);
      const int x0 = (int)x0f, y0 = (int)y0f;                    // px in [-0.5, W - 0.5]: no overflow
      if (x0 < 0 || y0 < 0 || x0 + 1 >= W || y0 + 1 >= H) continue;
      const int64_t base = (int64_t)v * H * W;
      const int64_t q00 = base + (int64_t)y0 * W + x0, q10 = q00 + 1, q01 = q00 + W, q11 = q01 + 1;
      if (!(viewmask[q00] > 0.5f && viewmask[q10] > 0.5f && viewmask[q01] > 0.5f && viewmask[q11] > 0.5f)) continue;
      const float* cam = campos + v * 3;
      const float dx = cam[0] - P[0], dy = cam[1] - P[1], dz = cam[2] - P[2];
      const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
      const int xn = min(max((int)floorf(px + 0.5f), 0), W - 1), yn = min(max((int)floorf(py + 0.5f), 0), H - 1);
      if (d - depth[base + (int64_t)yn * W + xn] > depth_bias) continue;
      const float cs = ((N[0] * dx + N[1] * dy) + N[2] * dz) / d;
      if (!(cs > cos_min)) continue;
      const float w = powf(cs, power);
      if (!(w > 0.f) || !__builtin_isfinite(w)) continue;        // cos_min < 0 with a fractional power: no weight, no view
      const float fx = px - x0f, fy = py - y0f, gx = 1.f - fx, gy = 1.f - fy;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float col = (image[q00 * 3 + c] * gx + image[q10 * 3 + c] * fx) * gy + (image[q01 * 3 + c] * gx + image[q11 * 3 + c] * fx) * fy;
        acc[c] += w * col;
      }
      wsum += w;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) color[(int64_t)p * 3 + c] = wsum > 0.f ? acc[c] / wsum : 0.f;
  weight[p] = wsum;
}

// ---- exports -------------------------------------------------------------------------------------------------------------------
#define TX_DISPATCH_C(C, CALL) \
  switch (C) {                 \
    case 1: { constexpr int K = 1; CALL; } break; \
    case 2: { constexpr int K = 2; CALL; } break; \
    case 3: { constexpr int K = 3; CALL; } break; \
    case 4: { constexpr int K = 4; CALL; } break; \
    case 5: { constexpr int K = 5; CALL; } break; \
    case 6: { constexpr int K = 6; CALL; } break; \
    case 7: { constexpr int K = 7; CALL; } break; \
    default: { constexpr int K = 8; CALL; } break; \
  }

// sizes, then limits, of a fetch: T textures of Ht x Wt x C sampled by B images of H x W
static int tx_sample_args(int32_t T, int32_t Ht, int32_t Wt, int32_t C, int32_t B, int32_t H, int32_t W, int32_t boundary) {
  if (T <= 0 || Ht <= 0 || Wt <= 0 || B <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if ((T != 1 && T != B) || (boundary != MD_TEXTURE_CLAMP && boundary != MD_TEXTURE_WRAP)) return MD_ERR_BAD_ARG;
  if (C < 1 || C > RS_MAX_CHANNELS || Ht > TX_MAX_RES || Wt > TX_MAX_RES || B > RS_MAX_VIEWS || H > RS_MAX_RES || W > RS_MAX_RES)
    return MD_ERR_UNSUPPORTED;
  return MD_OK;                                                  // 4 B H W <= 2^30 codes and T Ht Wt + 1 <= 2^28 + 1 rows fit int32
}

static inline bool tx_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const char* x = (const char*)a;
  const char* y = (const char*)b;
  return x < y + nb && y < x + na;
}

extern "C" int md_texture_sample(const float* tex, const float* uv, const float* rast, int32_t T, int32_t Ht, int32_t Wt, int32_t C,
                                 int32_t B, int32_t H, int32_t W, int32_t boundary, float* out, void* stream) {
  if (md_any_bad<16>(tex, out) || md_any_bad<8>(uv) || md_any_misaligned<16>(rast)) return MD_ERR_BAD_ARG;
  const int rc = tx_sample_args(T, Ht, Wt, C, B, H, W, boundary);
  if (rc != MD_OK) return rc;
  const int64_t bstride = T == 1 ? 0 : (int64_t)Ht * Wt * C;
  MD_HIP_CLEAR_ERROR();
  TX_DISPATCH_C(C, hipLaunchKernelGGL(md_texture_sample_kernel<K>, dim3(md_blocks(H * W, 256), (unsigned)B), dim3(256), 0,
                                      (hipStream_t)stream, tex, uv, rast, bstride, (int)Ht, (int)Wt, (int)(H * W), (int)boundary, out));
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_texture_codes(const float* uv, const float* rast, int32_t T, int32_t Ht, int32_t Wt, int32_t B, int32_t H,
                                int32_t W, int32_t boundary, int32_t* dest, void* stream) {
  if (md_any_bad<8>(uv) || md_any_bad<16>(dest) || md_any_misaligned<16>(rast)) return MD_ERR_BAD_ARG;
  const int rc = tx_sample_args(T, Ht, Wt, 1, B, H, W, boundary);
  if (rc != MD_OK) return rc;
  const int64_t bstride = T == 1 ? 0 : (int64_t)Ht * Wt;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_texture_codes_kernel, dim3(md_blocks(H * W, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, uv, rast,
                     bstride, (int)Ht, (int)Wt, (int)(H * W), (int)boundary, (int)((int64_t)T * Ht * Wt), dest);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_texture_sample_bwd(const float* tex, const float* uv, const float* rast, const float* grad_out, const int32_t* ptr,
                                     const int32_t* order, int32_t T, int32_t Ht, int32_t Wt, int32_t C, int32_t B, int32_t H,
                                     int32_t W, int32_t boundary, float* dtex, float* duv, void* stream) {
  if (md_any_bad<16>(tex, grad_out) || md_any_bad<8>(uv) || md_any_misaligned<16>(rast, dtex) || md_any_misaligned<8>(duv) ||
      md_any_misaligned<4>(ptr, order))
    return MD_ERR_BAD_ARG;
  if ((!dtex && !duv) || (dtex && (!ptr || !order))) return MD_ERR_BAD_ARG;
  const int rc = tx_sample_args(T, Ht, Wt, C, B, H, W, boundary);
  if (rc != MD_OK) return rc;
  const int64_t bstride = T == 1 ? 0 : (int64_t)Ht * Wt * C;
  const int64_t rows = (int64_t)T * Ht * Wt, n_codes = (int64_t)B * H * W * 4;
  MD_HIP_CLEAR_ERROR();
  if (duv)
    TX_DISPATCH_C(C, hipLaunchKernelGGL(md_texture_duv_kernel<K>, dim3(md_blocks(H * W, 256), (unsigned)B), dim3(256), 0,
                                        (hipStream_t)stream, tex, uv, rast, grad_out, bstride, (int)Ht, (int)Wt, (int)(H * W),
                                        (int)boundary, duv));
  if (dtex)
    TX_DISPATCH_C(C, hipLaunchKernelGGL(md_texture_dtex_kernel<K>, dim3(md_blocks(rows, 256)), dim3(256), 0, (hipStream_t)stream, uv,
                                        grad_out, ptr, order, rows, n_codes, (int)Ht, (int)Wt, dtex));
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_texture_dilate(const float* tex, const float* mask, int32_t Ht, int32_t Wt, int32_t C, float* out_tex,
                                 float* out_mask, void* stream) {
  if (md_any_bad<16>(tex, out_tex) || md_any_bad<4>(mask, out_mask)) return MD_ERR_BAD_ARG;
  if (Ht <= 0 || Wt <= 0) return MD_ERR_BAD_ARG;
  if (C < 1 || C > RS_MAX_CHANNELS || Ht > TX_MAX_RES || Wt > TX_MAX_RES) return MD_ERR_UNSUPPORTED;
  const int64_t n = (int64_t)Ht * Wt * 4;
  if (tx_overlap(tex, n * C, out_tex, n * C) || tx_overlap(mask, n, out_mask, n) || tx_overlap(tex, n * C, out_mask, n) ||
      tx_overlap(mask, n, out_tex, n * C) || tx_overlap(out_tex, n * C, out_mask, n))
    return MD_ERR_BAD_ARG;
  MD_HIP_CLEAR_ERROR();
  TX_DISPATCH_C(C, hipLaunchKernelGGL(md_texture_dilate_kernel<K>, dim3(md_blocks((int64_t)Ht * Wt, 256)), dim3(256), 0,
                                      (hipStream_t)stream, tex, mask, (int)Ht, (int)Wt, out_tex, out_mask));
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_texture_project(const float* pos, const float* nrm, const float* texmask, const float* image, const float* depth,
                                  const float* viewmask, const float* mvp, const float* campos, int32_t Ht, int32_t Wt, int32_t V,
                                  int32_t H, int32_t W, float depth_bias, float cos_min, float power, float* color, float* weight,
                                  void* stream) {
  if (md_any_bad<4>(pos, nrm, texmask, image, depth, viewmask, mvp, campos, color, weight)) return MD_ERR_BAD_ARG;
  if (Ht <= 0 || Wt <= 0 || V <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (!(depth_bias == depth_bias) || !(cos_min == cos_min) || !(power == power)) return MD_ERR_BAD_ARG;
  if (Ht > TX_MAX_RES || Wt > TX_MAX_RES || V > TX_MAX_VIEWS || H > RS_MAX_RES || W > RS_MAX_RES) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_texture_project_kernel, (int64_t)Ht * Wt, 256, pos, nrm, texmask, image, depth, viewmask, mvp, campos,
               (int)(Ht * Wt), (int)V, (int)H, (int)W, depth_bias, cos_min, power, color, weight);
}
