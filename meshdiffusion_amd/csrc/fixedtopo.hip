// The fixed-topology second pass of the DMTet fit (nvdiffrec/fit_dmtets.py:758-793, DMTetGeometryFixedTopo of
// nvdiffrec/lib/geometry/dmtet_fixedtopo.py:176-288 and laplace_regularizer_const of nvdiffrec/lib/render/regularizer.py:41-60):
// with the sign of the SDF frozen the mesh's topology never changes, so the crossing edges, the faces and every CSR keyed on
// them are a PLAN built once (meshdiffusion_amd/dmtet.py FixedTopoPlan), and an iteration only moves the vertices.
//
// THE FIXED-TOPOLOGY CONTRACT (tests/fixedtopo_cases.py restates it in torch)
//   Plan       edge int32 [Vm][2] (8-byte aligned): the grid endpoints (a, b), a < b, of mesh vertex i, i.e. the crossing edges of
//              the static sorted edge table in ascending edge id -- the numbering of md_marching_tets.  Grid-vertex CSR:
//              ptr int32 [N+1], inc int32 [2 Vm] with the codes 2 * mesh vertex + (0: the grid vertex is edge[i][0], 1: it is
//              edge[i][1]), ascending inside a grid vertex.  Face-corner CSR: ptr int32 [V+1], order int32 [3 F] with the codes
//              3 f + k sorted stably by the vertex faces[f][k] (the CSR of md_vertex_normals_det).  The host builds the tables and
//              checks their ranges once; the kernels skip (treat as absent) any index outside its table and never read there.
//   Vertices   fp32, every operation rounded on its own (no contraction), the expressions of md_mt_verts_kernel in its order:
//              sa = sdf[a], sb = sdf[b], nsb = -sb, den = sa + nsb, w0 = nsb / den, w1 = sa / den,
//              verts[i][c] = pos[a][c] * w0 + pos[b][c] * w1.  Bit-equal to md_marching_tets on the same inputs; for
//              sdf = +-1 the weights are exactly 0.5.
//   d pos      dpos[n] = the sum over the codes of grid vertex n, in ascending code order, of g[i] * w, w the forward's weight of
//              that endpoint ((side ? sa : nsb) / den); a plain fp32 sum, the association of md_marching_tets_bwd, whose dpos it
//              equals bit for bit.  A grid vertex with no codes gets zeros.  The SDF gets no gradient: it is frozen in pass 2.
//   Laplacian  y = x - base (base NULL: y = x).  For vertex v with corners (f, k) in ascending code order:
//                c_(f,k) = (y[f[(k+1)%3]] - y_v) + (y[f[(k+2)%3]] - y_v)           per component, each operation rounded
//                s_v = the compensated sum of c (below), term_v = s_v / max(2 * corners_v, 1)
//              loss = mean of term^2 over the 3 V components: fp64 partial sums (each square formed in fp64 from the fp32 term)
//              of MD_LAPLACE_SLABS workgroups at fixed slabs of the workspace, each thread striding the 3 V components in
//              order, one wave adds the slabs in a fixed order, loss = (float)(sum / (3 V)) stays on the device.
//              A vertex no face names has term = 0.
//   d x        q_v = ((2 / (3 V)) * g) * term_v / max(2 * corners_v, 1), g = the incoming gradient read from device memory;
//              d x_v = the compensated sum over the corners (f, k) of v, ascending, of (q[f[(k+1)%3]] + q[f[(k+2)%3]]) - 2 q_v.
//              base gets no gradient.  A vertex no face names gets exactly 0.
//   Sums       compensated (Kahan) fp32 in ascending code order, as in the interpolation contract (csrc/interp.hip): sum = 0,
//              lost = 0; per term x: y = x - lost, t = sum + y, lost = (t - sum) - y, sum = t.
//   Limits     sizes are int64 at the boundary: non-positive MD_ERR_BAD_ARG; N, V, 2 Vm, 3 F beyond int32 or F >= 2^24
//              MD_ERR_UNSUPPORTED; null or misaligned pointers MD_ERR_BAD_ARG.
//
// Kernels.  Latency- and HBM-bound gathers over short rows (valence ~6 on a marching-tets mesh, at most 14 codes per grid vertex):
// one thread per row, 256-thread workgroups, coalesced ptr reads, no LDS, no floating-point atomics, plain stores: two runs
// agree bit for bit.  Every row computes a term per code, so the row loops stay here; the compensated step is md_kahan_add of
// csrc/md_gather.h.
#include "md_args.h"
#include "md_gather.h"

#pragma clang fp contract(off)

static constexpr int FT_THREADS = 256;
static_assert(MD_LAPLACE_SLABS == 64, "the final reduction takes one slab per lane of a wave64");

// ---- vertices ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FT_THREADS) void md_ft_verts_kernel(const float* __restrict__ pos, const float* __restrict__ sdf,
                                                                 const int32_t* __restrict__ edge, int N, int Vm,
                                                                 float* __restrict__ verts) {
  const int i = blockIdx.x * FT_THREADS + threadIdx.x;
  if (i >= Vm) return;
  const int2 ab = *(const int2*)(edge + 2 * (int64_t)i);
  float out[3] = {0.f, 0.f, 0.f};
  if ((unsigned)ab.x < (unsigned)N && (unsigned)ab.y < (unsigned)N) {
    const float sa = sdf[ab.x], sb = sdf[ab.y];
    const float nsb = -sb;
    const float den = sa + nsb;
    const float w0 = nsb / den, w1 = sa / den;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float t0 = pos[(int64_t)ab.x * 3 + k] * w0;
      const float t1 = pos[(int64_t)ab.y * 3 + k] * w1;
      out[k] = t0 + t1;
    }
  }
  float* dst = verts + (int64_t)i * 3;
  dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
}

__global__ __launch_bounds__(FT_THREADS) void md_ft_verts_bwd_kernel(const float* __restrict__ g, const float* __restrict__ sdf,
                                                                     const int32_t* __restrict__ edge,
                                                                     const int32_t* __restrict__ ptr, const int32_t* __restrict__ inc,
                                                                     int N, int Vm, float* __restrict__ dpos) {
  const int n = blockIdx.x * FT_THREADS + threadIdx.x;
  if (n >= N) return;
  float dp0 = 0.f, dp1 = 0.f, dp2 = 0.f;
  const int j0 = max(ptr[n], 0), j1 = min(ptr[n + 1], 2 * Vm);
  for (int j = j0; j < j1; ++j) {
    const int code = inc[j];
    const int i = code >> 1, side = code & 1;
    if ((unsigned)i >= (unsigned)Vm) continue;
    const int2 ab = *(const int2*)(edge + 2 * (int64_t)i);
    if ((unsigned)ab.x >= (unsigned)N || (unsigned)ab.y >= (unsigned)N) continue;
    const float sa = sdf[ab.x], sb = sdf[ab.y];
    const float nsb = -sb;
    const float den = sa + nsb;                     // the forward's denominator, bit for bit
    const float w = (side ? sa : nsb) / den;        // the forward's weight of this endpoint
    const float* gi = g + (int64_t)i * 3;
    dp0 += gi[0] * w; dp1 += gi[1] * w; dp2 += gi[2] * w;
  }
  float* dst = dpos + (int64_t)n * 3;
  dst[0] = dp0; dst[1] = dp1; dst[2] = dp2;
}

// ---- umbrella Laplacian --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ft_load_y(const float* __restrict__ x, const float* __restrict__ base, int64_t v, float* y) {
  y[0] = x[v * 3]; y[1] = x[v * 3 + 1]; y[2] = x[v * 3 + 2];
  if (base) { y[0] -= base[v * 3]; y[1] -= base[v * 3 + 1]; y[2] -= base[v * 3 + 2]; }
}

// the two other corners of code = 3 f + k, or false when the code or a vertex lies outside its table
__device__ __forceinline__ bool ft_others(const int64_t* __restrict__ faces, int code, int V, int F, int64_t& i1, int64_t& i2) {
  const int f = code / 3, k = code - 3 * f;
  if ((unsigned)f >= (unsigned)F) return false;
  i1 = faces[(int64_t)f * 3 + (k + 1) % 3];
  i2 = faces[(int64_t)f * 3 + (k + 2) % 3];
  return i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
}

__global__ __launch_bounds__(FT_THREADS) void md_ft_laplace_term_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                                        const int64_t* __restrict__ faces,
                                                                        const int32_t* __restrict__ ptr,
                                                                        const int32_t* __restrict__ order, int V, int F,
                                                                        float* __restrict__ term) {
  const int v = blockIdx.x * FT_THREADS + threadIdx.x;
  if (v >= V) return;
  float yv[3], s[3] = {0.f, 0.f, 0.f}, lost[3] = {0.f, 0.f, 0.f};
  ft_load_y(x, base, v, yv);
  const int j0 = max(ptr[v], 0), j1 = min(ptr[v + 1], 3 * F);
  for (int j = j0; j < j1; ++j) {
    int64_t i1, i2;
    if (!ft_others(faces, order[j], V, F, i1, i2)) continue;
    float y1[3], y2[3];
    ft_load_y(x, base, i1, y1);
    ft_load_y(x, base, i2, y2);
#pragma unroll
    for (int c = 0; c < 3; ++c) md_kahan_add(s[c], lost[c], (y1[c] - yv[c]) + (y2[c] - yv[c]));
  }
  const float n = fmaxf(2.f * (float)max(j1 - j0, 0), 1.f);
  float* dst = term + (int64_t)v * 3;
  dst[0] = s[0] / n; dst[1] = s[1] / n; dst[2] = s[2] / n;
}

__global__ __launch_bounds__(FT_THREADS) void md_ft_sq_partial_kernel(const float* __restrict__ term, int64_t n,
                                                                      double* __restrict__ sums) {
  double a = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FT_THREADS) {
    const double t = (double)term[i];
    a += t * t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  __shared__ double red[FT_THREADS / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void md_ft_sq_final_kernel(const double* __restrict__ sums, int64_t n, float* __restrict__ loss) {
  double a = sums[threadIdx.x];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (threadIdx.x == 0) *loss = (float)(a / (double)n);
}

__global__ __launch_bounds__(FT_THREADS) void md_ft_laplace_q_kernel(const float* __restrict__ term, const int32_t* __restrict__ ptr,
                                                                     const float* __restrict__ grad_out, int V, int F,
                                                                     float* __restrict__ q) {
  const int v = blockIdx.x * FT_THREADS + threadIdx.x;
  if (v >= V) return;
  const int j0 = max(ptr[v], 0), j1 = min(ptr[v + 1], 3 * F);
  const float n = fmaxf(2.f * (float)max(j1 - j0, 0), 1.f);
  const float s = (2.f / (float)(3 * (int64_t)V)) * (*grad_out);
#pragma unroll
  for (int c = 0; c < 3; ++c) q[(int64_t)v * 3 + c] = (s * term[(int64_t)v * 3 + c]) / n;
}

__global__ __launch_bounds__(FT_THREADS) void md_ft_laplace_bwd_kernel(const float* __restrict__ q, const int64_t* __restrict__ faces,
                                                                       const int32_t* __restrict__ ptr,
                                                                       const int32_t* __restrict__ order, int V, int F,
                                                                       float* __restrict__ dx) {
  const int v = blockIdx.x * FT_THREADS + threadIdx.x;
  if (v >= V) return;
  float s[3] = {0.f, 0.f, 0.f}, lost[3] = {0.f, 0.f, 0.f};
  const float qv2[3] = {2.f * q[(int64_t)v * 3], 2.f * q[(int64_t)v * 3 + 1], 2.f * q[(int64_t)v * 3 + 2]};
  const int j0 = max(ptr[v], 0), j1 = min(ptr[v + 1], 3 * F);
  for (int j = j0; j < j1; ++j) {
    int64_t i1, i2;
    if (!ft_others(faces, order[j], V, F, i1, i2)) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) md_kahan_add(s[c], lost[c], (q[i1 * 3 + c] + q[i2 * 3 + c]) - qv2[c]);
  }
  float* dst = dx + (int64_t)v * 3;
  dst[0] = s[0]; dst[1] = s[1]; dst[2] = s[2];
}

// ---- exports -------------------------------------------------------------------------------------------------------------------
static int ft_plan_sizes(int64_t n_verts, int64_t n_mesh_verts) {
  if (n_verts <= 0 || n_mesh_verts <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_mesh_verts)) return MD_ERR_UNSUPPORTED;                         // int32 indices and codes
  return MD_OK;
}

static int ft_mesh_sizes(int64_t n_verts, int64_t n_faces) {
  if (n_verts <= 0 || n_faces <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts) || n_faces >= (1LL << 24)) return MD_ERR_UNSUPPORTED;                // 3 F corner codes fit int32
  return MD_OK;
}

extern "C" int md_fixedtopo_verts(const float* pos, const float* sdf, const int32_t* edge, int64_t n_verts, int64_t n_mesh_verts,
                                  float* verts, void* stream) {
  if (md_any_bad<4>(pos, sdf, verts) || md_any_bad<8>(edge)) return MD_ERR_BAD_ARG;
  const int rc = ft_plan_sizes(n_verts, n_mesh_verts);
  if (rc != MD_OK) return rc;
  MD_LAUNCH_1D(md_ft_verts_kernel, n_mesh_verts, FT_THREADS, pos, sdf, edge, (int)n_verts, (int)n_mesh_verts, verts);
}

extern "C" int md_fixedtopo_verts_bwd(const float* grad_verts, const float* sdf, const int32_t* edge, const int32_t* ptr,
                                      const int32_t* inc, int64_t n_verts, int64_t n_mesh_verts, float* dpos, void* stream) {
  if (md_any_bad<4>(grad_verts, sdf, ptr, inc, dpos) || md_any_bad<8>(edge)) return MD_ERR_BAD_ARG;
  const int rc = ft_plan_sizes(n_verts, n_mesh_verts);
  if (rc != MD_OK) return rc;
  MD_LAUNCH_1D(md_ft_verts_bwd_kernel, n_verts, FT_THREADS, grad_verts, sdf, edge, ptr, inc, (int)n_verts, (int)n_mesh_verts, dpos);
}

extern "C" int md_laplace_umbrella(const float* x, const float* base, const int64_t* faces, const int32_t* ptr, const int32_t* order,
                                   int64_t n_verts, int64_t n_faces, float* term, void* workspace, float* loss, void* stream) {
  if (md_any_bad<4>(x, ptr, order, term, loss) || md_any_bad<8>(faces, workspace) || md_any_misaligned<4>(base)) return MD_ERR_BAD_ARG;
  const int rc = ft_mesh_sizes(n_verts, n_faces);
  if (rc != MD_OK) return rc;
  const hipStream_t st = (hipStream_t)stream;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_ft_laplace_term_kernel, dim3(md_blocks(n_verts, FT_THREADS)), dim3(FT_THREADS), 0, st, x, base, faces, ptr, order,
                     (int)n_verts, (int)n_faces, term);
  hipLaunchKernelGGL(md_ft_sq_partial_kernel, dim3(MD_LAPLACE_SLABS), dim3(FT_THREADS), 0, st, (const float*)term, 3 * n_verts,
                     (double*)workspace);
  hipLaunchKernelGGL(md_ft_sq_final_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, 3 * n_verts, loss);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_laplace_umbrella_bwd(const float* term, const int64_t* faces, const int32_t* ptr, const int32_t* order,
                                       const float* grad_out, int64_t n_verts, int64_t n_faces, float* q, float* dx, void* stream) {
  if (md_any_bad<4>(term, ptr, order, grad_out, q, dx) || md_any_bad<8>(faces)) return MD_ERR_BAD_ARG;
  const int rc = ft_mesh_sizes(n_verts, n_faces);
  if (rc != MD_OK) return rc;
  const hipStream_t st = (hipStream_t)stream;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_ft_laplace_q_kernel, dim3(md_blocks(n_verts, FT_THREADS)), dim3(FT_THREADS), 0, st, term, ptr, grad_out,
                     (int)n_verts, (int)n_faces, q);
  hipLaunchKernelGGL(md_ft_laplace_bwd_kernel, dim3(md_blocks(n_verts, FT_THREADS)), dim3(FT_THREADS), 0, st, (const float*)q, faces, ptr,
                     order, (int)n_verts, (int)n_faces, dx);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
