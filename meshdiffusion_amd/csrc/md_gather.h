// The one backward reduction of the DMTet fitting stack: per-code gradients are written first, then one thread per destination
// row GATHERS them in a fixed order over (ptr int32 [rows + 1], order int32 [n_codes]), the CSR of the codes sorted stably by the
// row they name (meshdiffusion_amd/_csr.py builds it).  No floating-point atomics: two runs agree bit for bit.
//
// A plain and a compensated sum give different bits, so every site keeps the kind its contract fixes:
//   depth backward        plain   the rasterisation contract, "Gradient" (csrc/raster.hip)
//   antialias backward    plain   the antialiasing contract, "Gradient" (csrc/antialias.hip)
//   interpolate d attr    Kahan   the interpolation contract, "Sums" (csrc/interp.hip)
//   barycentric backward  Kahan   the interpolation contract, "Sums"
//   normals backward      Kahan   the interpolation contract, "Sums"
// Kernels that compute a term per code (md_vertex_normals_gather_kernel, the Laplacian of csrc/fixedtopo.hip) keep their own row
// loop and share md_kahan_add only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

// One step of a compensated (Kahan) sum: the order of the terms is the contract's, `lost` carries the low bits a plain fp32 add
// drops, so a row of a thousand codes is as accurate as a row of three.  No contraction, no reassociation: still bit-reproducible.
__host__ __device__ __forceinline__ void md_kahan_add(float& sum, float& lost, float x) {
  const float y = x - lost;
  const float t = sum + y;
  lost = (t - sum) - y;
  sum = t;
}

// acc = the sum of src[code] (W floats each) over the codes of `row`, in the order of the CSR.  A position outside [0, n_codes)
// ends the row and a code outside [0, n_codes) is skipped: never with the CSR of the host, and nothing outside src is read.
template <int W, bool KAHAN>
__host__ __device__ __forceinline__ void md_gather_row(const float* __restrict__ src, const int32_t* __restrict__ ptr,
                                                       const int32_t* __restrict__ order, int64_t row, int64_t n_codes,
                                                       float (&acc)[W]) {
  float lost[W];
#pragma unroll
  for (int c = 0; c < W; ++c) { acc[c] = 0.f; lost[c] = 0.f; }
  const int j1 = ptr[row + 1];
  for (int j = ptr[row]; j < j1; ++j) {
    if (j < 0 || j >= n_codes) break;
    const int32_t code = order[j];
    if (code < 0 || code >= n_codes) continue;
    const float* s = src + (int64_t)code * W;
#pragma unroll
    for (int c = 0; c < W; ++c) {
      if constexpr (KAHAN) md_kahan_add(acc[c], lost[c], s[c]);
      else acc[c] += s[c];
    }
  }
}

// dst[row] = that sum, one thread per row.  AS_CLIP (W == 3): the row is a clip-space vertex and (a0, a1, a2) is stored as
// (x, y, 0, w), one float4 at pitch 4; otherwise W floats at pitch W.
template <int W, bool KAHAN, bool AS_CLIP>
__global__ __launch_bounds__(256) void md_csr_gather_kernel(const float* __restrict__ src, const int32_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ order, int64_t rows, int64_t n_codes,
                                                            float* __restrict__ dst) {
  static_assert(!AS_CLIP || W == 3, "the clip layout holds (x, y, w)");
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  float acc[W];
  md_gather_row<W, KAHAN>(src, ptr, order, row, n_codes, acc);
  if constexpr (AS_CLIP) {
    *reinterpret_cast<float4*>(dst + row * 4) = make_float4(acc[0], acc[1], 0.f, acc[2]);
  } else {
#pragma unroll
    for (int c = 0; c < W; ++c) dst[row * W + c] = acc[c];
  }
}

template <int W, bool KAHAN, bool AS_CLIP>
static inline void md_csr_gather(const float* src, const int32_t* ptr, const int32_t* order, int64_t rows, int64_t n_codes,
                                 float* dst, hipStream_t stream) {
  hipLaunchKernelGGL((md_csr_gather_kernel<W, KAHAN, AS_CLIP>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, src,
                     ptr, order, rows, n_codes, dst);
}
