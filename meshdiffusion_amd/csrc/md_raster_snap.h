// The snap of the rasterisation contract (csrc/raster.hip), shared with the antialiasing kernels (csrc/antialias.hip): both must
// reach the same integers X, Y from the same clip floats.
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
