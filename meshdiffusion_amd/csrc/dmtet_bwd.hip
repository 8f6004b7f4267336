// Backward of the marching-tetrahedra vertex interpolation (md_mt_verts_kernel of dmtet.hip) and the SDF sign regulariser
// of nvdiffrec/lib/geometry/dmtet.py:169-175 with its backward.
//
// Both backwards GATHER: one thread per (mesh, grid vertex) walks the static incidence list of that vertex (CSR over grid
// vertices: inc_ptr [N+1], inc [2E] = 2 * edge id + (0: the vertex is the edge's first endpoint, 1: its second), ascending
// edge id inside a vertex) and writes its outputs once.  No atomics: the sums have a fixed order, two runs agree bit for
// bit, and the launch does not depend on how many edges cross.  At most 14 incident edges per vertex on the shipped grid.
//
// Vertex interpolation, edge e = (a, b), sa = sdf[a], sb = sdf[b], den = sa - sb (the forward's expressions):
//   v = pos[a] * (-sb / den) + pos[b] * (sa / den)
//   dpos[a] += g * (-sb / den)        dpos[b] += g * (sa / den)
//   d = dot(g, pos[a] - pos[b]) / den^2
//   dsdf[a] += d * sb                 dsdf[b] -= d * sa
#include "md_args.h"

#pragma clang fp contract(off)

static constexpr int MTB_THREADS = 256;

__global__ __launch_bounds__(MTB_THREADS) void md_mt_bwd_kernel(
    const float* __restrict__ pos, const float* __restrict__ sdf, const int32_t* __restrict__ edges,
    const int32_t* __restrict__ vid, const int32_t* __restrict__ counts, const float* __restrict__ grad_verts,
    const int32_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc, int n_verts, int n_edges,
    float* __restrict__ dpos, float* __restrict__ dsdf) {
  const int m = blockIdx.y;
  const int n = blockIdx.x * MTB_THREADS + threadIdx.x;
  if (n >= n_verts) return;
  const float* mpos = pos + (int64_t)m * n_verts * 3;
  const float* msdf = sdf + (int64_t)m * n_verts;
  const int32_t* mvid = vid + (int64_t)m * n_edges;
  const float* mg = grad_verts + (int64_t)m * n_edges * 3;
  const int nv = counts[m * 4];
  const float sn = msdf[n];
  const float pn0 = mpos[n * 3], pn1 = mpos[n * 3 + 1], pn2 = mpos[n * 3 + 2];
  float dp0 = 0.f, dp1 = 0.f, dp2 = 0.f, ds = 0.f;
  const int j1 = inc_ptr[n + 1];
  for (int j = inc_ptr[n]; j < j1; ++j) {
    const int code = inc[j];
    const int e = code >> 1, side = code & 1;
    const int v = mvid[e];
    if (v < 0 || v >= nv) continue;                 // not a crossing edge of this mesh
    const int o = edges[2 * (int64_t)e + (side ^ 1)];
    const float so = msdf[o];
    const float po0 = mpos[o * 3], po1 = mpos[o * 3 + 1], po2 = mpos[o * 3 + 2];
    const float g0 = mg[(int64_t)v * 3], g1 = mg[(int64_t)v * 3 + 1], g2 = mg[(int64_t)v * 3 + 2];
    const float sa = side ? so : sn, sb = side ? sn : so;
    const float nsb = -sb;
    const float den = sa + nsb;                     // the forward's denominator, bit for bit
    const float w = (side ? sa : nsb) / den;        // the forward's weight of this endpoint
    dp0 += g0 * w; dp1 += g1 * w; dp2 += g2 * w;
    // dot(g, pos[a] - pos[b]): for the second endpoint the difference is taken the other way round and the sign folded in
    const float dot = (g0 * (pn0 - po0) + g1 * (pn1 - po1)) + g2 * (pn2 - po2);
    const float d = dot / (den * den);
    ds += d * so;                                   // side 0: +d_ab * sb ; side 1: d_ba = -d_ab, so -d_ab * sa
  }
  float* mdpos = dpos + ((int64_t)m * n_verts + n) * 3;
  mdpos[0] = dp0; mdpos[1] = dp1; mdpos[2] = dp2;
  dsdf[(int64_t)m * n_verts + n] = ds;
}

extern "C" int md_marching_tets_bwd(const float* pos, const float* sdf, const int32_t* edges, const int32_t* vid,
                                    const int32_t* counts, const float* grad_verts, const int32_t* inc_ptr,
                                    const int32_t* inc, int32_t n_meshes, int32_t n_verts, int32_t n_edges, float* dpos,
                                    float* dsdf, void* stream) {
  if (md_any_bad<1>(pos, sdf, edges, vid, counts, grad_verts, inc_ptr, inc, dpos,
      dsdf) || n_meshes <= 0 || n_verts <= 0 || n_edges <= 0)
    return MD_ERR_BAD_ARG;
  if (n_meshes > 65535) return MD_ERR_UNSUPPORTED;             // gridDim.y
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_mt_bwd_kernel, dim3(md_blocks(n_verts, MTB_THREADS), (unsigned)n_meshes), dim3(MTB_THREADS), 0,
                     (hipStream_t)stream, pos, sdf, edges, vid, counts, grad_verts, inc_ptr, inc, (int)n_verts,
                     (int)n_edges, dpos, dsdf);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

// ---- SDF sign regulariser ----------------------------------------------------------------------------------------------
// Over the edges with sign(s0) != sign(s1) (torch.sign: a zero endpoint counts, a NaN endpoint differs from everything):
//   loss = mean bce_with_logits(s0, [s1 > 0]) + mean bce_with_logits(s1, [s0 > 0]),
//   bce_with_logits(x, t) = max(x, 0) - x * t + log1p(exp(-|x|))                              (the stable form torch uses)
// Launch 1: workgroup s writes {sum of the first term, sum of the second term} in fp64 and its masked-edge count at slab s
// of the workspace (fixed grid, fixed per-thread order).  Launch 2: one wave adds the slabs in a fixed order and writes
// loss (float) and the count; an empty mask gives 0 / 0 = nan, the reference's mean of an empty tensor.
static_assert(MD_SDF_REG_SLABS == 64, "the final reduction takes one slab per lane of a wave64");

__device__ __forceinline__ bool sdf_reg_mask(float s0, float s1) {
  const int g0 = (s0 > 0.f) - (s0 < 0.f), g1 = (s1 > 0.f) - (s1 < 0.f);
  return g0 != g1 || s0 != s0 || s1 != s1;
}

__device__ __forceinline__ float sdf_reg_bce(float x, float t) {
  return (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x)));
}

__global__ __launch_bounds__(256) void md_sdf_reg_partial_kernel(const float* __restrict__ sdf, const int32_t* __restrict__ edges,
                                                                 int n_edges, double* __restrict__ sums,
                                                                 int64_t* __restrict__ cnts) {
  double a0 = 0.0, a1 = 0.0;
  int c = 0;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += gridDim.x * blockDim.x) {
    const int2 ab = *(const int2*)(edges + 2 * (int64_t)e);
    const float s0 = sdf[ab.x], s1 = sdf[ab.y];
    if (sdf_reg_mask(s0, s1)) {
      a0 += (double)sdf_reg_bce(s0, s1 > 0.f ? 1.f : 0.f);
      a1 += (double)sdf_reg_bce(s1, s0 > 0.f ? 1.f : 0.f);
      ++c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o, 64);
    a1 += __shfl_xor(a1, o, 64);
    c += __shfl_xor(c, o, 64);
  }
  __shared__ double red[2][4];
  __shared__ int redc[4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a0;
    red[1][threadIdx.x >> 6] = a1;
    redc[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sums[blockIdx.x * 2] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    sums[blockIdx.x * 2 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    cnts[blockIdx.x] = (int64_t)((redc[0] + redc[1]) + (redc[2] + redc[3]));
  }
}

__global__ __launch_bounds__(64) void md_sdf_reg_final_kernel(const double* __restrict__ sums, const int64_t* __restrict__ cnts,
                                                              float* __restrict__ loss, int32_t* __restrict__ count) {
  double a0 = sums[threadIdx.x * 2], a1 = sums[threadIdx.x * 2 + 1];
  int c = (int)cnts[threadIdx.x];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o, 64);
    a1 += __shfl_xor(a1, o, 64);
    c += __shfl_xor(c, o, 64);
  }
  if (threadIdx.x == 0) {
    const double n = (double)c;
    *loss = (float)(a0 / n) + (float)(a1 / n);     // the reference adds two float32 means
    *count = c;
  }
}

// Backward: dsdf[n] = (grad_out / count) * sum over the masked incident edges of (sigmoid(s_n) - [s_other > 0]); the target
// is a constant of the graph, as in the reference.  count and grad_out are read from device memory.  A vertex with no masked
// edge gets exactly 0 (also when count == 0, where the reference's gradient is all zeros).
__global__ __launch_bounds__(MTB_THREADS) void md_sdf_reg_bwd_kernel(const float* __restrict__ sdf, const int32_t* __restrict__ edges,
                                                                     const int32_t* __restrict__ inc_ptr,
                                                                     const int32_t* __restrict__ inc,
                                                                     const int32_t* __restrict__ count,
                                                                     const float* __restrict__ grad_out, int n_verts,
                                                                     float* __restrict__ dsdf) {
  const int n = blockIdx.x * MTB_THREADS + threadIdx.x;
  if (n >= n_verts) return;
  const float sn = sdf[n];
  const float sig = 1.f / (1.f + expf(-sn));
  float acc = 0.f;
  bool any = false;
  const int j1 = inc_ptr[n + 1];
  for (int j = inc_ptr[n]; j < j1; ++j) {
    const int code = inc[j];
    const int o = edges[2 * (int64_t)(code >> 1) + ((code & 1) ^ 1)];
    const float so = sdf[o];
    if (sdf_reg_mask(sn, so)) {
      acc += sig - (so > 0.f ? 1.f : 0.f);
      any = true;
    }
  }
  dsdf[n] = any ? acc * (*grad_out / (float)(*count)) : 0.f;
}

extern "C" int md_sdf_reg_loss(const float* sdf, const int32_t* edges, int32_t n_verts, int32_t n_edges, void* workspace,
                               float* loss, int32_t* count, void* stream) {
  if (md_any_bad<1>(sdf, loss, count) || md_any_bad<8>(edges, workspace)) return MD_ERR_BAD_ARG;  // int2 rows, fp64 slabs
  if (n_verts <= 0 || n_edges <= 0) return MD_ERR_BAD_ARG;
  double* sums = (double*)workspace;
  int64_t* cnts = (int64_t*)(sums + 2 * MD_SDF_REG_SLABS);
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_sdf_reg_partial_kernel, dim3(MD_SDF_REG_SLABS), dim3(256), 0, (hipStream_t)stream, sdf, edges,
                     (int)n_edges, sums, cnts);
  hipLaunchKernelGGL(md_sdf_reg_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)sums,
                     (const int64_t*)cnts, loss, count);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_sdf_reg_loss_bwd(const float* sdf, const int32_t* edges, const int32_t* inc_ptr, const int32_t* inc,
                                   const int32_t* count, const float* grad_out, int32_t n_verts, int32_t n_edges,
                                   float* dsdf, void* stream) {
  if (md_any_bad<1>(sdf, edges, inc_ptr, inc, count, grad_out, dsdf) || n_verts <= 0 || n_edges <= 0)
    return MD_ERR_BAD_ARG;
  MD_LAUNCH_1D(md_sdf_reg_bwd_kernel, n_verts, MTB_THREADS, sdf, edges, inc_ptr, inc, count, grad_out, (int)n_verts,
               dsdf);
}
