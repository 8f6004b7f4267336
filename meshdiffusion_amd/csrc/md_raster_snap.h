// The snap of the rasterisation contract (csrc/raster.hip), shared with the antialiasing kernels (csrc/antialias.hip): both must
// reach the same integers X, Y from the same clip floats.  Also its shape limits and its barycentric backward, for every file
// that reads `rast`.
#pragma once
#include "md_common.h"

#pragma clang fp contract(off)

static constexpr int RS_SNAP_MAX = 1 << 22;

// The shape limits of the rasterisation contract, for every file that reads or writes `rast` (raster.hip, antialias.hip,
// interp.hip): at most 64 views, 2048 x 2048 pixels, fewer than 2^24 faces; images and attributes of 1 to 8 channels.
static constexpr int RS_MAX_VIEWS = 64, RS_MAX_RES = 2048, RS_MAX_FACES = 1 << 24, RS_MAX_CHANNELS = 8;
static inline bool rs_limits_ok(int32_t batch, int32_t n_faces, int32_t H, int32_t W) {
  return batch <= RS_MAX_VIEWS && H <= RS_MAX_RES && W <= RS_MAX_RES && n_faces < RS_MAX_FACES;
}

__device__ __forceinline__ bool rs_finite(float x) { return fabsf(x) < __builtin_inff(); }

// the contract's snap of one coordinate: rint(((x / w) * 0.5 + 0.5) * scale), clamped to +-2^22
__device__ __forceinline__ int rs_snap(float x, float w, float scale) {
  const float t = __fadd_rn(__fmul_rn(__fdiv_rn(x, w), 0.5f), 0.5f);
  const float r = rintf(__fmul_rn(t, scale));
  return (int)fminf(fmaxf(r, -(float)RS_SNAP_MAX), (float)RS_SNAP_MAX);
}

// The barycentric backward of the rasterisation contract, shared by md_raster_depth_bwd_pix_kernel (csrc/raster.hip) and
// md_raster_bary_bwd_pix_kernel (csrc/interp.hip): from (du, dv), the gradient of a covered pixel's (u, v), to the gradient of
// the three clip-space corners.  px, py are the shifted p_k = (x_k - fx w_k, y_k - fy w_k).  With S = a0 + a1 + a2:
//   d a_j = (du (delta_0j - u) + dv (delta_1j - v)) / S; a0 = p1 x p2 etc. give d p_k; d w_k = -fx d p_k.x - fy d p_k.y.
__device__ __forceinline__ void rs_bary_bwd(const float (&px)[3], const float (&py)[3], float u, float v, float du, float dv,
                                            float fx, float fy, float (&dpx)[3], float (&dpy)[3], float (&dw)[3]) {
  const float a0 = px[1] * py[2] - py[1] * px[2];
  const float a1 = px[2] * py[0] - py[2] * px[0];
  const float a2 = px[0] * py[1] - py[0] * px[1];
  const float S = (a0 + a1) + a2;
  const float da0 = (du * (1.f - u) - dv * v) / S;
  const float da1 = (dv * (1.f - v) - du * u) / S;
  const float da2 = (-du * u - dv * v) / S;
  dpx[0] = da2 * py[1] - da1 * py[2];
  dpy[0] = da1 * px[2] - da2 * px[1];
  dpx[1] = da0 * py[2] - da2 * py[0];
  dpy[1] = da2 * px[0] - da0 * px[2];
  dpx[2] = da1 * py[0] - da0 * py[1];
  dpy[2] = da0 * px[1] - da1 * px[0];
#pragma unroll
  for (int k = 0; k < 3; ++k) dw[k] = -fx * dpx[k] - fy * dpy[k];
}
