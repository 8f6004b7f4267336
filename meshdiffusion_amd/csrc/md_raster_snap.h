// The snap of the rasterisation contract (csrc/raster.hip), shared with the antialiasing kernels (csrc/antialias.hip): both must
// reach the same integers X, Y from the same clip floats.
#pragma once
#include "md_common.h"

#pragma clang fp contract(off)

static constexpr int RS_SNAP_MAX = 1 << 22;

__device__ __forceinline__ bool rs_finite(float x) { return fabsf(x) < __builtin_inff(); }

// the contract's snap of one coordinate: rint(((x / w) * 0.5 + 0.5) * scale), clamped to +-2^22
__device__ __forceinline__ int rs_snap(float x, float w, float scale) {
  const float t = __fadd_rn(__fmul_rn(__fdiv_rn(x, w), 0.5f), 0.5f);
  const float r = rintf(__fmul_rn(t, scale));
  return (int)fminf(fmaxf(r, -(float)RS_SNAP_MAX), (float)RS_SNAP_MAX);
}
