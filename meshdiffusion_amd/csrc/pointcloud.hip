// Point-cloud supervision of the fitting loop (nvdiffrec/lib/geometry/dmtet.py:454-459): nearest neighbours between two
// clouds, the chamfer gradient, and area-weighted surface sampling of a triangle mesh (geometry/utils.py:3-127).
//
// md_nn_sided -- brute force, N x M squared distances in the DIRECT form (px-qx)^2 + (py-qy)^2 + (pz-qz)^2 in fp32.  The
// expanded form |p|^2 + |q|^2 - 2 p.q (cdist, any matrix-core formulation) cancels catastrophically for near neighbours
// and is used neither for the value nor for the choice.  A workgroup of 256 lanes keeps NN_QPL = 4 queries per lane in
// registers (1024 queries) and walks ONE CHUNK of q in LDS tiles of 1024 points; every lane reads the same float4 of the
// tile (a broadcast), so one LDS read feeds four queries.  The pairs of queries are float2 so that the subtractions and
// the multiply-adds can issue as packed fp32 instructions.  q is split into chunks across blockIdx.y so that 50 000
// queries (49 workgroups' worth) still fill 256 CUs; each (chunk, query) writes one 64-bit key
//     key = (nan ? 0 : float bits + 1) << 32 | index
// to the workspace and a second launch takes the minimum over the chunks.  Squared distances are non-negative, so the
// unsigned order of the key is the lexicographic (distance, index) order: ties go to the lowest index, the combination
// does not depend on any execution order, and two runs agree bit for bit.  No atomics.
//
// NaN / inf: the result is what torch.min over the row of direct-form distances gives.  A NaN distance (a NaN coordinate
// on either side, or inf - inf) wins over every number and the first one keeps the index.  The fast loop's `d < best`
// would drop a NaN, so a tile takes the CAREFUL loop whenever it, or a query of the workgroup, holds a non-finite
// coordinate -- and whenever skip_same_index applies to it (the tile overlaps the workgroup's own index range).
#include "md_args.h"

typedef float nn_f2 __attribute__((ext_vector_type(2)));

static constexpr int NN_THREADS = 256;
static constexpr int NN_QPL = 4;                            // queries per lane
static constexpr int NN_QUERIES = NN_THREADS * NN_QPL;      // queries per workgroup
static constexpr int NN_TILE = 1024;                        // q points per LDS tile (16 KiB)
static constexpr int NN_TARGET_WGS = 2048;                  // ~8 workgroups per CU
static constexpr uint64_t NN_NO_CANDIDATE = ~0ull;

// chunks of q (each a whole number of tiles) for a launch: deterministic in (B, N, M) alone
static inline void nn_chunks(int64_t B, int64_t N, int64_t M, int64_t* n_chunks, int64_t* tiles_per_chunk) {
  const int64_t qblocks = (N + NN_QUERIES - 1) / NN_QUERIES * B;
  const int64_t tiles = (M + NN_TILE - 1) / NN_TILE;
  int64_t want = (NN_TARGET_WGS + qblocks - 1) / qblocks;
  if (want > tiles) want = tiles;
  if (want > 65535) want = 65535;
  if (want < 1) want = 1;
  int64_t tpc = (tiles + want - 1) / want;
  if ((tiles + tpc - 1) / tpc > 65535) tpc = (tiles + 65534) / 65535;
  *tiles_per_chunk = tpc;
  *n_chunks = (tiles + tpc - 1) / tpc;
}

__device__ __forceinline__ bool nn_finite(float x) { return fabsf(x) < __builtin_inff(); }    // false for NaN too

__global__ __launch_bounds__(NN_THREADS) void md_nn_partial_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                                   int N, int M, int tiles_per_chunk, int skip_same,
                                                                   uint64_t* __restrict__ keys) {
  __shared__ float4 tile[NN_TILE];
  __shared__ int s_tile_bad[2], s_query_bad;
  const int tid = threadIdx.x;
  const int b = blockIdx.z, chunk = blockIdx.y, n_chunks = gridDim.y;
  const int64_t q0 = (int64_t)blockIdx.x * NN_QUERIES;
  const float* pb = p + (int64_t)b * N * 3;
  const float* qb = q + (int64_t)b * M * 3;
  const int64_t c_begin = (int64_t)chunk * tiles_per_chunk * NN_TILE;
  int64_t c_end = c_begin + (int64_t)tiles_per_chunk * NN_TILE;
  if (c_end > M) c_end = M;

  if (tid == 0) { s_tile_bad[0] = 0; s_tile_bad[1] = 0; s_query_bad = 0; }
  __syncthreads();
  nn_f2 PX[2], PY[2], PZ[2];
  float best[NN_QPL];
  int bidx[NN_QPL], gi[NN_QPL];
  bool qbad = false;
#pragma unroll
  for (int k = 0; k < NN_QPL; ++k) {
    const int64_t i = q0 + k * NN_THREADS + tid;
    const int64_t ic = i < N ? i : N - 1;                    // lanes past the end repeat the last query; nothing is written
    const float x = pb[ic * 3], y = pb[ic * 3 + 1], z = pb[ic * 3 + 2];
    PX[k >> 1][k & 1] = x; PY[k >> 1][k & 1] = y; PZ[k >> 1][k & 1] = z;
    qbad |= !(nn_finite(x) && nn_finite(y) && nn_finite(z));
    best[k] = __builtin_inff();
    bidx[k] = -1;
    gi[k] = (int)ic;
  }
  if (qbad) s_query_bad = 1;
  // skip_same_index concerns the tiles that overlap [q0, q0 + NN_QUERIES)
  const int64_t own_lo = q0, own_hi = q0 + NN_QUERIES;

  int t = 0;
  for (int64_t j0 = c_begin; j0 < c_end; j0 += NN_TILE, ++t) {
    const int cnt = (int)((c_end - j0) < NN_TILE ? (c_end - j0) : NN_TILE);
    bool bad = false;
    for (int i = tid; i < cnt; i += NN_THREADS) {
      const float* s = qb + (j0 + i) * 3;
      const float x = s[0], y = s[1], z = s[2];
      tile[i] = make_float4(x, y, z, 0.f);
      bad |= !(nn_finite(x) && nn_finite(y) && nn_finite(z));
    }
    if (bad) s_tile_bad[t & 1] = 1;
    __syncthreads();
    if (tid == 0) s_tile_bad[(t + 1) & 1] = 0;
    const bool careful = s_tile_bad[t & 1] || s_query_bad || (skip_same && j0 < own_hi && j0 + cnt > own_lo);
    if (!careful) {
#pragma clang fp contract(fast)
#pragma unroll 4
      for (int j = 0; j < cnt; ++j) {
        const float4 c = tile[j];
        const int gj = (int)j0 + j;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const nn_f2 dx = PX[h] - c.x, dy = PY[h] - c.y, dz = PZ[h] - c.z;
          const nn_f2 d = dz * dz + (dy * dy + dx * dx);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const bool lt = d[e] < best[2 * h + e];
            best[2 * h + e] = lt ? d[e] : best[2 * h + e];
            bidx[2 * h + e] = lt ? gj : bidx[2 * h + e];
          }
        }
      }
    } else {
#pragma clang fp contract(fast)
      for (int j = 0; j < cnt; ++j) {
        const float4 c = tile[j];
        const int gj = (int)j0 + j;
#pragma unroll
        for (int k = 0; k < NN_QPL; ++k) {
          const float dx = PX[k >> 1][k & 1] - c.x, dy = PY[k >> 1][k & 1] - c.y, dz = PZ[k >> 1][k & 1] - c.z;
          const float d = dz * dz + (dy * dy + dx * dx);
          const bool cand = !(skip_same && gj == gi[k]);
          // the first NaN sticks (best != best from then on); otherwise a strictly smaller distance replaces
          if (cand && best[k] == best[k] && (d != d || d < best[k])) { best[k] = d; bidx[k] = gj; }
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < NN_QPL; ++k) {
    const int64_t i = q0 + k * NN_THREADS + tid;
    if (i >= N) continue;
    int64_t first = c_begin;                                 // the chunk's first candidate of this query
    if (skip_same && first == i) ++first;
    uint64_t key = NN_NO_CANDIDATE;
    if (first < c_end) {
      const bool isnan = best[k] != best[k];
      const uint32_t hi = isnan ? 0u : __float_as_uint(best[k]) + 1u;
      const uint32_t lo = (uint32_t)(bidx[k] < 0 ? (int)first : bidx[k]);      // every candidate at +inf: the first one
      key = ((uint64_t)hi << 32) | lo;
    }
    keys[((int64_t)b * n_chunks + chunk) * N + i] = key;
  }
}

__global__ __launch_bounds__(256) void md_nn_final_kernel(const uint64_t* __restrict__ keys, int N, int n_chunks,
                                                          float* __restrict__ dist, int64_t* __restrict__ idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= N) return;
  const uint64_t* k = keys + (int64_t)b * n_chunks * N + i;
  uint64_t m = NN_NO_CANDIDATE;
  for (int c = 0; c < n_chunks; ++c) {
    const uint64_t v = k[(int64_t)c * N];
    m = v < m ? v : m;
  }
  const uint32_t hi = (uint32_t)(m >> 32);
  float d;
  int64_t j;
  if (m == NN_NO_CANDIDATE) { d = __builtin_inff(); j = -1; }
  else { d = hi == 0u ? __builtin_nanf("") : __uint_as_float(hi - 1u); j = (int64_t)(uint32_t)m; }
  dist[(int64_t)b * N + i] = d;
  idx[(int64_t)b * N + i] = j;
}

extern "C" int64_t md_nn_sided_workspace_bytes(int32_t batch, int32_t n, int32_t m) {
  if (batch <= 0 || n <= 0 || m <= 0) return MD_ERR_BAD_ARG;
  int64_t nc, tpc;
  nn_chunks(batch, n, m, &nc, &tpc);
  return (int64_t)batch * nc * n * 8;
}

extern "C" int md_nn_sided(const float* p, const float* q, int32_t batch, int32_t n, int32_t m, int32_t skip_same_index,
                           float* dist, int64_t* idx, void* workspace, int64_t workspace_bytes, void* stream) {
  if (md_any_bad<1>(p, q, dist) || md_any_bad<8>(idx, workspace) || batch <= 0 || n <= 0 || m <= 0) return MD_ERR_BAD_ARG;
  if (batch > 65535) return MD_ERR_UNSUPPORTED;              // gridDim.z / gridDim.y
  int64_t nc, tpc;
  nn_chunks(batch, n, m, &nc, &tpc);
  if (workspace_bytes < (int64_t)batch * nc * n * 8) return MD_ERR_BAD_ARG;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_nn_partial_kernel, dim3(md_blocks(n, NN_QUERIES), (unsigned)nc, (unsigned)batch),
                     dim3(NN_THREADS), 0, (hipStream_t)stream, p, q, (int)n, (int)m, (int)tpc, (int)(skip_same_index != 0),
                     (uint64_t*)workspace);
  hipLaunchKernelGGL(md_nn_final_kernel, dim3(md_blocks(n, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                     (const uint64_t*)workspace, (int)n, (int)nc, dist, idx);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

// ---- chamfer backward --------------------------------------------------------------------------------------------------
// L[b] = w1 * mean_i |p_i - q_nn(i)|^2 + w2 * mean_j |q_j - p_nn(j)|^2, neighbours held fixed.  For a point a_i of one side
// (count Na, weight wa; the other side: Nb, wb):
//   dL/da_i = g * ( 2 wa / Na * (a_i - b_nn(i))  +  2 wb / Nb * sum_{j : nn_ba(j) = i} (a_i - b_j) )
// The second sum is a GATHER over a CSR of the other direction's neighbour indices (ptr [B][Na+1], order [B][Nb] = the j
// sorted stably by nn_ba(j)): fixed order, no float atomics, bit-reproducible.  The same kernel serves both sides.
#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void md_chamfer_bwd_kernel(const float* __restrict__ a, const float* __restrict__ bpts,
                                                             const int64_t* __restrict__ nn_ab, const int32_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ order, int Na, int Nb, float wa,
                                                             float wb, const float* __restrict__ grad_out,
                                                             float* __restrict__ da) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int bt = blockIdx.y;
  if (i >= Na) return;
  const float* ab = a + (int64_t)bt * Na * 3;
  const float* bb = bpts + (int64_t)bt * Nb * 3;
  const float g = grad_out[bt];
  const float ca = (2.f * wa / (float)Na) * g, cb = (2.f * wb / (float)Nb) * g;
  const float x = ab[(int64_t)i * 3], y = ab[(int64_t)i * 3 + 1], z = ab[(int64_t)i * 3 + 2];
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  const int64_t nn = nn_ab[(int64_t)bt * Na + i];
  if (nn >= 0) {
    d0 = (x - bb[nn * 3]) * ca; d1 = (y - bb[nn * 3 + 1]) * ca; d2 = (z - bb[nn * 3 + 2]) * ca;
  }
  const int32_t* pr = ptr + (int64_t)bt * (Na + 1);
  const int32_t* od = order + (int64_t)bt * Nb;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  const int j1 = pr[i + 1];
  for (int j = pr[i]; j < j1; ++j) {
    const int64_t o = od[j];
    s0 += x - bb[o * 3]; s1 += y - bb[o * 3 + 1]; s2 += z - bb[o * 3 + 2];
  }
  float* out = da + ((int64_t)bt * Na + i) * 3;
  out[0] = d0 + s0 * cb; out[1] = d1 + s1 * cb; out[2] = d2 + s2 * cb;
}

extern "C" int md_chamfer_bwd(const float* p, const float* q, const int64_t* idx_pq, const int64_t* idx_qp,
                              const int32_t* ptr_p, const int32_t* order_p, const int32_t* ptr_q, const int32_t* order_q,
                              int32_t batch, int32_t n, int32_t m, float w1, float w2, const float* grad_out, float* dp,
                              float* dq, void* stream) {
  if (md_any_bad<1>(p, q, ptr_p, order_p, grad_out, dp) || md_any_bad<8>(idx_pq, idx_qp) || batch <= 0 || n <= 0 || m <= 0)
    return MD_ERR_BAD_ARG;
  if (dq && (!ptr_q || !order_q)) return MD_ERR_BAD_ARG;
  if (batch > 65535) return MD_ERR_UNSUPPORTED;              // gridDim.y
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_chamfer_bwd_kernel, dim3(md_blocks(n, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, p, q, idx_pq, ptr_p, order_p, (int)n, (int)m, w1, w2, grad_out, dp);
  if (dq)
    hipLaunchKernelGGL(md_chamfer_bwd_kernel, dim3(md_blocks(m, 256), (unsigned)batch), dim3(256), 0,
                       (hipStream_t)stream, q, p, idx_qp, ptr_q, order_q, (int)m, (int)n, w2, w1, grad_out, dq);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

// ---- surface sampling --------------------------------------------------------------------------------------------------
// areas[b][f] = 0.5 * |(v1 - v0) x (v2 - v0)|.  faces are shared by the batch (geometry/utils.py:97-100).
__global__ __launch_bounds__(256) void md_face_areas_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                            int V, int F, float* __restrict__ areas) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const float* vb = verts + (int64_t)blockIdx.y * V * 3;
  const int64_t i0 = faces[(int64_t)f * 3], i1 = faces[(int64_t)f * 3 + 1], i2 = faces[(int64_t)f * 3 + 2];
  const float ax = vb[i1 * 3] - vb[i0 * 3], ay = vb[i1 * 3 + 1] - vb[i0 * 3 + 1], az = vb[i1 * 3 + 2] - vb[i0 * 3 + 2];
  const float bx = vb[i2 * 3] - vb[i0 * 3], by = vb[i2 * 3 + 1] - vb[i0 * 3 + 1], bz = vb[i2 * 3 + 2] - vb[i0 * 3 + 2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  areas[(int64_t)blockIdx.y * F + f] = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
}

// One thread per (mesh, sample).  Face: the given one, or the first f with cdf[f] > r_face * cdf[F-1] by bisection over the
// inclusive prefix sum (non-decreasing: a zero-area face has cdf[f] == cdf[f-1] and is never the first to exceed).  Point:
// u = sqrt(r_u), w0 = 1 - u, w1 = u (1 - r_v), w2 = u r_v, (w0 v0 + w1 v1) + w2 v2 without contraction: the reference's
// expressions and order (geometry/utils.py:34-45).
__global__ __launch_bounds__(256) void md_sample_points_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                               const float* __restrict__ cdf, const float* __restrict__ r_face,
                                                               const float* __restrict__ r_u, const float* __restrict__ r_v,
                                                               const int64_t* __restrict__ choices_in, int V, int F, int S,
                                                               float* __restrict__ points, int64_t* __restrict__ choices,
                                                               float* __restrict__ weights) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const int64_t bs = (int64_t)blockIdx.y * S + s;
  const float* vb = verts + (int64_t)blockIdx.y * V * 3;
  int64_t f;
  if (choices_in) {
    f = choices_in[bs];
  } else {
    const float* c = cdf + (int64_t)blockIdx.y * F;
    const float tgt = r_face[bs] * c[F - 1];
    int lo = -1, hi = F - 1;                                 // invariant: cdf[lo] <= tgt (or lo = -1); the answer is in (lo, hi]
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if (c[mid] > tgt) hi = mid; else lo = mid;
    }
    // tgt rounded up to the total (r_face within 2^-24 of 1): fall back to the last face of positive area
    while (hi > 0 && c[hi] == c[hi - 1]) --hi;
    f = hi;
  }
  const int64_t i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  const float u = sqrtf(r_u[bs]), v = r_v[bs];
  const float w0 = 1.f - u, w1 = u * (1.f - v), w2 = u * v;
#pragma unroll
  for (int k = 0; k < 3; ++k) points[bs * 3 + k] = (w0 * vb[i0 * 3 + k] + w1 * vb[i1 * 3 + k]) + w2 * vb[i2 * 3 + k];
  choices[bs] = f;
  if (weights) { weights[bs * 3] = w0; weights[bs * 3 + 1] = w1; weights[bs * 3 + 2] = w2; }
}

// dverts[b][v] = sum over the (sample, corner) pairs that name v of weight * grad_points[sample]: a gather over a CSR of the
// 3S corner entries (ptr [B][V+1], order [B][3S] = 3 * sample + corner sorted stably by vertex).  No atomics.
__global__ __launch_bounds__(256) void md_sample_points_bwd_kernel(const float* __restrict__ grad_points,
                                                                   const float* __restrict__ weights,
                                                                   const int32_t* __restrict__ ptr,
                                                                   const int32_t* __restrict__ order, int V, int S,
                                                                   float* __restrict__ dverts) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const int bt = blockIdx.y;
  const float* g = grad_points + (int64_t)bt * S * 3;
  const float* w = weights + (int64_t)bt * S * 3;
  const int32_t* pr = ptr + (int64_t)bt * (V + 1);
  const int32_t* od = order + (int64_t)bt * S * 3;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  const int j1 = pr[v + 1];
  for (int j = pr[v]; j < j1; ++j) {
    const int e = od[j];
    const int s = e / 3;
    const float wk = w[e];
    a0 += wk * g[(int64_t)s * 3]; a1 += wk * g[(int64_t)s * 3 + 1]; a2 += wk * g[(int64_t)s * 3 + 2];
  }
  float* out = dverts + ((int64_t)bt * V + v) * 3;
  out[0] = a0; out[1] = a1; out[2] = a2;
}

extern "C" int md_face_areas(const float* verts, const int64_t* faces, int32_t batch, int32_t n_verts, int32_t n_faces,
                             float* areas, void* stream) {
  if (md_any_bad<1>(verts, areas) || md_any_bad<8>(faces) || batch <= 0 || n_verts <= 0 || n_faces <= 0) return MD_ERR_BAD_ARG;
  if (batch > 65535) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_face_areas_kernel, dim3(md_blocks(n_faces, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, verts, faces, (int)n_verts, (int)n_faces, areas);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_sample_points(const float* verts, const int64_t* faces, const float* cdf, const float* r_face,
                                const float* r_u, const float* r_v, const int64_t* face_choices_in, int32_t batch,
                                int32_t n_verts, int32_t n_faces, int32_t n_samples, float* points, int64_t* face_choices,
                                float* weights, void* stream) {
  if (md_any_bad<1>(verts, r_u, r_v, points) || md_any_bad<8>(faces, face_choices) || md_any_misaligned<8>(face_choices_in))
    return MD_ERR_BAD_ARG;
  if (batch <= 0 || n_verts <= 0 || n_faces <= 0 || n_samples <= 0) return MD_ERR_BAD_ARG;
  if (!face_choices_in && (!cdf || !r_face)) return MD_ERR_BAD_ARG;
  if (batch > 65535) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_sample_points_kernel, dim3(md_blocks(n_samples, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, verts, faces, cdf, r_face, r_u, r_v, face_choices_in, (int)n_verts, (int)n_faces,
                     (int)n_samples, points, face_choices, weights);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_sample_points_bwd(const float* grad_points, const float* weights, const int32_t* ptr, const int32_t* order,
                                    int32_t batch, int32_t n_verts, int32_t n_samples, float* dverts, void* stream) {
  if (md_any_bad<1>(grad_points, weights, ptr, order, dverts) || batch <= 0 || n_verts <= 0 || n_samples <= 0)
    return MD_ERR_BAD_ARG;
  if (batch > 65535 || !md_fits_i32((int64_t)n_samples * 3)) return MD_ERR_UNSUPPORTED;    // gridDim.y; int32 corner codes
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_sample_points_bwd_kernel, dim3(md_blocks(n_verts, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, grad_points, weights, ptr, order, (int)n_verts, (int)n_samples, dverts);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
