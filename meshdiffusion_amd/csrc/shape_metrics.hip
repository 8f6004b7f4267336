// Generation metrics (MMD / COV / 1-NNA under the chamfer distance): the all-pairs matrix of sided mean squared distances
// between two SETS of point clouds,
//     out[i][j] = (1/p) * sum_a min_b |x[i][a] - y[j][b]|^2,        x [nx][p][3], y [ny][q][3], out [nx][ny].
// The chamfer distance of a pair is out_xy[i][j] + out_yx[j][i]; for the union matrix of one set the caller passes the same
// pointer twice and adds the transpose.
//
// Arithmetic: that of md_nn_partial_kernel (pointcloud.hip), for the reason written there.  Squared distances in the DIRECT
// form dz*dz + (dy*dy + dx*dx) in fp32 -- never |p|^2 + |q|^2 - 2 p.q, so no matrix-core instruction.  The per-point minima
// are summed in float64 in a fixed order (a lane's points in ascending order, then the lanes of a wave by an xor tree, then
// the four waves in ascending order), divided by p and rounded once to fp32.  No atomics; the value of out[i][j] does not
// depend on which workgroup computes it, so it does not depend on how the launch is cut up and two runs agree bit for bit.
//
// Launch: a workgroup of 256 lanes owns ONE x cloud and a contiguous RUN of y clouds.  It keeps a block of up to 2048 points
// of its x cloud in registers (8 per lane, as float2 pairs so that the subtractions and multiply-adds issue as packed fp32)
// and streams every y cloud of the run through LDS tiles of 1024 points (16 KiB); every lane reads the same float4 of the
// tile (a broadcast), so one LDS read feeds eight distances, and two candidates fold into a running minimum with one
// three-operand min.  Only `min` is kept: no index.  The workgroup writes out[i][j] itself: no workspace, one launch.  For
// p > 2048 it loops over the blocks of its cloud for every y cloud and carries the float64 sum.  The x clouds are the fast
// grid dimension, so the workgroups in flight together walk the same run of y clouds (24 KB each at 2048 points: L2).
//
// NaN / inf: out[i][j] is what torch gives for d2.min(dim=1).values.mean() on the direct-form fp32 distances.  A NaN distance
// (a NaN coordinate on either side, or inf - inf) wins a row's minimum, a NaN minimum makes the mean NaN.  The fast loop's
// min drops NaNs -- a NaN candidate and a NaN running minimum alike -- so a tile takes the CAREFUL loop whenever it, the
// resident block, or an EARLIER tile of the same y cloud holds a non-finite coordinate: once a tile of a (y cloud, x block)
// pass has been careful, the rest of that pass is, and a NaN minimum survives the tiles after it.  On finite data the careful
// loop gives the fast loop's bits.
#include "md_args.h"

typedef float sm_f2 __attribute__((ext_vector_type(2)));

static constexpr int SM_THREADS = 256;
static constexpr int SM_PPL = 8;                            // x points per lane
static constexpr int SM_BLOCK = SM_THREADS * SM_PPL;        // x points resident per workgroup
static constexpr int SM_TILE = 1024;                        // y points per LDS tile (16 KiB)
static constexpr int SM_TARGET_WGS = 2048;                  // ~8 workgroups per CU

// y clouds per workgroup: deterministic in (nx, ny) alone.  Enough runs per x cloud for ~SM_TARGET_WGS workgroups; the point
// counts do not enter (a workgroup's work per y cloud is p * q whatever the run).
static inline int64_t sm_run_len(int64_t nx, int64_t ny) {
  int64_t want = (SM_TARGET_WGS + nx - 1) / nx;
  if (want > ny) want = ny;
  if (want < 1) want = 1;
  return (ny + want - 1) / want;
}

__device__ __forceinline__ bool sm_finite(float v) { return fabsf(v) < __builtin_inff(); }    // false for NaN too

__global__ __launch_bounds__(SM_THREADS) void md_sided_mean_matrix_kernel(const float* x, const float* y, int ny, int p, int q,
                                                                          int run_len, float* __restrict__ out) {
  __shared__ float4 tile[SM_TILE];
  __shared__ int s_bad[2];
  __shared__ double s_wave[SM_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  const int64_t j_begin = (int64_t)blockIdx.y * run_len;
  int64_t j_end = j_begin + run_len;
  if (j_end > ny) j_end = ny;
  const float* xi = x + i * p * 3;
  const bool resident = p <= SM_BLOCK;                       // the whole x cloud fits the registers: loaded once

  if (tid == 0) { s_bad[0] = 0; s_bad[1] = 0; }
  __syncthreads();
  sm_f2 PX[SM_PPL / 2], PY[SM_PPL / 2], PZ[SM_PPL / 2];
  bool xbad = false;
  unsigned t = 0;                                            // tiles walked so far: s_bad alternates with its parity
  for (int64_t j = j_begin; j < j_end; ++j) {
    const float* yj = y + j * q * 3;
    double acc = 0.0;
    for (int64_t a0 = 0; a0 < p; a0 += SM_BLOCK) {
      if (!resident || j == j_begin) {
        xbad = false;
#pragma unroll
        for (int k = 0; k < SM_PPL; ++k) {
          const int64_t a = a0 + k * SM_THREADS + tid;
          const int64_t ac = a < p ? a : p - 1;              // lanes past the end repeat the last point; it is not summed
          const float vx = xi[ac * 3], vy = xi[ac * 3 + 1], vz = xi[ac * 3 + 2];
          PX[k >> 1][k & 1] = vx; PY[k >> 1][k & 1] = vy; PZ[k >> 1][k & 1] = vz;
          xbad |= !(sm_finite(vx) && sm_finite(vy) && sm_finite(vz));
        }
      }
      float best[SM_PPL];
#pragma unroll
      for (int k = 0; k < SM_PPL; ++k) best[k] = __builtin_inff();
      bool careful = false;                                  // workgroup-uniform; sticky for the rest of this (y cloud, x block)

      for (int64_t b0 = 0; b0 < q; b0 += SM_TILE, ++t) {
        const int cnt = (int)((q - b0) < SM_TILE ? (q - b0) : SM_TILE);
        const int cnt4 = (cnt + 3) & ~3;                     // padded with copies of the last point: a minimum ignores them
        bool bad = xbad;
        for (int c = tid; c < cnt4; c += SM_THREADS) {
          const float* s = yj + (b0 + (c < cnt ? c : cnt - 1)) * 3;
          const float vx = s[0], vy = s[1], vz = s[2];
          tile[c] = make_float4(vx, vy, vz, 0.f);
          bad |= !(sm_finite(vx) && sm_finite(vy) && sm_finite(vz));
        }
        if (bad) s_bad[t & 1] = 1;
        __syncthreads();
        if (tid == 0) s_bad[(t + 1) & 1] = 0;
        careful |= s_bad[t & 1] != 0;
        if (!careful) {
#pragma clang fp contract(fast)
#pragma unroll 2
          for (int c = 0; c < cnt4; c += 2) {
            const float4 u = tile[c], v = tile[c + 1];
#pragma unroll
            for (int h = 0; h < SM_PPL / 2; ++h) {
              const sm_f2 ux = PX[h] - u.x, uy = PY[h] - u.y, uz = PZ[h] - u.z;
              const sm_f2 vx = PX[h] - v.x, vy = PY[h] - v.y, vz = PZ[h] - v.z;
              const sm_f2 du = uz * uz + (uy * uy + ux * ux);
              const sm_f2 dv = vz * vz + (vy * vy + vx * vx);
#pragma unroll
              for (int e = 0; e < 2; ++e) best[2 * h + e] = __builtin_fminf(__builtin_fminf(best[2 * h + e], du[e]), dv[e]);
            }
          }
        } else {
#pragma clang fp contract(fast)
          for (int c = 0; c < cnt; ++c) {
            const float4 u = tile[c];
#pragma unroll
            for (int k = 0; k < SM_PPL; ++k) {
              const float dx = PX[k >> 1][k & 1] - u.x, dy = PY[k >> 1][k & 1] - u.y, dz = PZ[k >> 1][k & 1] - u.z;
              const float d = dz * dz + (dy * dy + dx * dx);
              // a NaN sticks (best != best from then on); otherwise a strictly smaller distance replaces
              if (best[k] == best[k] && (d != d || d < best[k])) best[k] = d;
            }
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < SM_PPL; ++k)
        if (a0 + k * SM_THREADS + tid < p) acc += (double)best[k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) s_wave[tid >> 6] = acc;
    __syncthreads();                                         // the next s_wave write follows a tile loop's barriers
    if (tid == 0) {
      double s = s_wave[0];
#pragma unroll
      for (int w = 1; w < SM_THREADS / 64; ++w) s += s_wave[w];
      out[i * ny + j] = (float)(s / (double)p);
    }
  }
}

extern "C" int md_sided_mean_matrix(const float* x, const float* y, int32_t nx, int32_t ny, int32_t p, int32_t q, float* out,
                                    void* stream) {
  if (md_any_bad<1>(x, y, out) || nx < 1 || ny < 1 || p < 1 || q < 1) return MD_ERR_BAD_ARG;
  // gridDim.y = runs <= SM_TARGET_WGS; gridDim.x = nx, and a launch's threads along x must stay below 2^32
  static_assert(SM_TARGET_WGS <= 65535, "runs per x cloud must fit gridDim.y");
  if ((int64_t)nx * SM_THREADS > 0xffffffffLL) return MD_ERR_UNSUPPORTED;
  const int64_t run = sm_run_len(nx, ny);
  const int64_t runs = (ny + run - 1) / run;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_sided_mean_matrix_kernel, dim3((unsigned)nx, (unsigned)runs), dim3(SM_THREADS), 0, (hipStream_t)stream,
                     x, y, (int)ny, (int)p, (int)q, (int)run, out);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
