// Distance from points to triangle meshes: for a batch of query points, the closest point on the triangles of the query's own mesh
// and the generalised winding number of that mesh at the query (Jacobson et al. 2013), by brute force over (queries x triangles).
// Two consumers: the warm start of the DMTet fit (the signed distance of the target at the tet grid's vertices, meshdist.py
// init_sdf) and the re-projection step of the isotropic remeshing (postprocess.py remesh(project=True)).  The reference has no
// counterpart (it fits by rendering alone and remeshes with MeshLab), so this is built under a contract of its own.  No gradient.
//
// THE MESH DISTANCE CONTRACT (tests/meshdist_cases.py restates it in float32 numpy, operation for operation)
//   Inputs      tri fp32 [T][3][3]: the gathered corners (a, b, c) of every triangle, grouped by mesh; tri_ptr int32 [M+1]: ascending
//               CSR of the triangles of each mesh; query fp32 [Q][3], grouped by mesh; query_ptr int32 [M+1]: ascending CSR of the
//               queries of each mesh.  A query of mesh m sees the triangles tri_ptr[m] .. tri_ptr[m+1]-1 only.  The host gathers
//               verts[faces]: no kernel reads an index.  Both CSRs are clamped to their tables: nothing outside them is read.
//   Outputs     each may be null, one at least is not: dist2 fp32 [Q], face int32 [Q] (an index into tri), closest fp32 [Q][3],
//               winding fp32 [Q].
//   Arithmetic  fp32, every operation rounded on its own (fp contract off in the whole file), no atomics.  sub and add are per
//               component; dot(u, v) = u2 v2 + (u1 v1 + u0 v0); divisions and square roots are the correctly rounded fp32 ones.
//   Per triangle  ab = b - a and ac = c - a are formed once (when the tile is loaded); every query then uses a, ab, ac only.
//   Closest     the region classification of Ericson's ClosestPtPointTriangle (Real-Time Collision Detection, 5.1.5):
//                 ap = p - a;   d1 = dot(ab, ap);  d2 = dot(ac, ap)
//                 bp = ap - ab; d3 = dot(ab, bp);  d4 = dot(ac, bp)
//                 cp = ap - ac; d5 = dot(ab, cp);  d6 = dot(ac, cp)
//                 vc = d1 d4 - d3 d2;  vb = d5 d2 - d1 d6;  va = d3 d6 - d5 d4;  e43 = d4 - d3;  e56 = d5 - d6
//               The first test that holds, in this order, names the region and the fractions (nv / dv, nw / dw):
//                 A   d1 <= 0 and d2 <= 0                      (0 / 1, 0 / 1)
//                 B   d3 >= 0 and d4 <= d3                     (1 / 1, 0 / 1)
//                 C   d6 >= 0 and d5 <= d6                     (0 / 1, 1 / 1)
//                 AB  vc <= 0 and d1 >= 0 and d3 <= 0          (d1 / (d1 - d3), 0 / 1)
//                 AC  vb <= 0 and d2 >= 0 and d6 <= 0          (0 / 1, d2 / (d2 - d6))
//                 BC  va <= 0 and e43 >= 0 and e56 >= 0        w = e43 / (e43 + e56), then v = 1 - w
//                 interior (none holds, also on NaN)           (vb / den, vc / den), den = (va + vb) + vc
//               v = nv / dv and w = nw / dw are two fp32 divisions (on BC only w is divided); the closest point is
//               c = a + (ab v + ac w) per component, and d2 = dot(p - c, p - c).  Written with selects: no divergent branch.
//               Triangles are visited in ascending index order and a candidate replaces the best only when d2 < best (best starts
//               at +inf): ties keep the lowest index and a NaN candidate is never taken.  A query that takes no triangle (an empty
//               mesh, every candidate NaN or +inf) gets dist2 = +inf, face = -1, closest = the query.  Nothing else is
//               special-cased: a zero-area triangle is whatever these rules make of it (three equal corners fall in region A and
//               give the distance to the corner; a needle whose fractions become 0 / 0 gives NaN and is never taken).
//   Winding     per triangle, with the corners minus the query A = a - p, B = A + ab, C = A + ac, la = sqrt(dot(A, A)) (lb, lc alike):
//                 det = dot(A, cross(B, C)),  cross(u, v) = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0)
//                 den = ((la lb) lc + dot(A, B) lc) + dot(B, C) la) + dot(C, A) lb
//                 omega = 2 atan2f(det, den)
//               in fp32; the terms are summed in float64 in ascending triangle order by the lane that owns the query, the sum is
//               divided by 4 pi in float64 and rounded once to fp32.  An empty mesh gives 0.  A non-finite query or corner gives what
//               this arithmetic gives: NaN (a NaN term makes the sum NaN; no term is skipped).  atan2f is the device library's: the
//               winding number is held to float64 by a tolerance, not bit for bit to the restatement; two runs agree bit for bit.
//   Determinism a query's outputs depend on its coordinates and on its mesh's triangles in order, not on how the launch is cut up.
//   Limits      in this order: a null or misaligned (4-byte) tri_ptr, query or query_ptr, a misaligned tri or output, no output
//               requested: MD_ERR_BAD_ARG; a negative count, a null tri with T > 0: MD_ERR_BAD_ARG; T or Q beyond int32, M >
//               MD_MESHDIST_MAX_MESHES (gridDim.y): MD_ERR_UNSUPPORTED; an output that is an input: MD_ERR_BAD_ARG.  Nothing is
//               launched before the last check; Q == 0 or M == 0 then returns MD_OK without a launch.  The CSRs live on the device
//               and are not read by the export: the host that builds them answers for them (the kernel clamps them, so a wrong
//               CSR reads nothing outside tri and query).  Nothing is allocated, nothing synchronises.
//   Not built   an acceleration structure (BVH, grid), Barnes-Hut winding numbers, gradients, and splitting one mesh's triangles
//               over workgroups: a launch with few queries and very many triangles runs on few workgroups.  That case is not ours
//               (a tet grid has 10^4 .. 10^5 vertices, a remeshed batch as many).
//
// Launch.  256 lanes per workgroup; blockIdx.y = mesh, blockIdx.x = block of MDQ_QPL * 256 of that mesh's queries, blocks past the
// mesh's count return before the first barrier.  A lane keeps MDQ_QPL = 1 query in registers: a tet grid has 3 * 10^4 vertices, 120
// workgroups of 256, which already leaves half of the 256 CUs idle; two queries per lane (measured: DESIGN.md) halve the
// workgroups again and were slower at every size we run.  Triangles stream through an LDS tile of 256 (one per lane per load, 12
// KiB) as three float4 (a, ab, ac); every lane reads the same address (a broadcast, as in md_sided_mean_matrix_kernel), so the loop
// is bound by the vector ALU, not by LDS.  The kernel is instantiated on (want closest, want winding): a caller that wants one
// pays for one.
#include "md_args.h"

#pragma clang fp contract(off)

static constexpr int MDQ_THREADS = 256;
static constexpr int MDQ_QPL = 1;                             // queries per lane
static constexpr int MDQ_TILE = MDQ_THREADS;                  // triangles per LDS tile: one per lane per load
static constexpr int MDQ_MAX_MESHES = 65535;                  // gridDim.y; MD_MESHDIST_MAX_MESHES of the header

struct mq_v3 { float x, y, z; };
__device__ __forceinline__ mq_v3 mq_sub(mq_v3 a, mq_v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ mq_v3 mq_add(mq_v3 a, mq_v3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ float mq_dot(mq_v3 u, mq_v3 v) { return u.z * v.z + (u.y * v.y + u.x * v.x); }
__device__ __forceinline__ mq_v3 mq_cross(mq_v3 u, mq_v3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }

// the closest point of triangle (a, ab, ac) to p by the contract, and its squared distance
__device__ __forceinline__ float mq_closest(mq_v3 p, mq_v3 a, mq_v3 ab, mq_v3 ac, mq_v3& c) {
  const mq_v3 ap = mq_sub(p, a);
  const float d1 = mq_dot(ab, ap), d2 = mq_dot(ac, ap);
  const mq_v3 bp = mq_sub(ap, ab);
  const float d3 = mq_dot(ab, bp), d4 = mq_dot(ac, bp);
  const mq_v3 cp = mq_sub(ap, ac);
  const float d5 = mq_dot(ab, cp), d6 = mq_dot(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  const bool inA = d1 <= 0.f && d2 <= 0.f;
  const bool inB = d3 >= 0.f && d4 <= d3;
  const bool inC = d6 >= 0.f && d5 <= d6;
  const bool inAB = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
  const bool inAC = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
  const bool inBC = va <= 0.f && e43 >= 0.f && e56 >= 0.f;
  const float den = (va + vb) + vc;
  // the interior first, then every region from the last to the first: the first that holds wins
  float nv = vb, dv = den, nw = vc, dw = den;
  bool bc = false;
  if (inBC) { nw = e43; dw = e43 + e56; bc = true; }
  if (inAC) { nv = 0.f; dv = 1.f; nw = d2; dw = d2 - d6; bc = false; }
  if (inAB) { nv = d1; dv = d1 - d3; nw = 0.f; dw = 1.f; bc = false; }
  if (inC) { nv = 0.f; dv = 1.f; nw = 1.f; dw = 1.f; bc = false; }
  if (inB) { nv = 1.f; dv = 1.f; nw = 0.f; dw = 1.f; bc = false; }
  if (inA) { nv = 0.f; dv = 1.f; nw = 0.f; dw = 1.f; bc = false; }
  const float w = nw / dw;
  const float v = bc ? 1.f - w : nv / dv;
  c = {a.x + (ab.x * v + ac.x * w), a.y + (ab.y * v + ac.y * w), a.z + (ab.z * v + ac.z * w)};
  const mq_v3 d = mq_sub(p, c);
  return mq_dot(d, d);
}

// the solid angle of triangle (a, ab, ac) seen from p by the contract
__device__ __forceinline__ float mq_omega(mq_v3 p, mq_v3 a, mq_v3 ab, mq_v3 ac) {
  const mq_v3 A = mq_sub(a, p), B = mq_add(A, ab), C = mq_add(A, ac);
  const float la = sqrtf(mq_dot(A, A)), lb = sqrtf(mq_dot(B, B)), lc = sqrtf(mq_dot(C, C));
  const float det = mq_dot(A, mq_cross(B, C));
  const float den = (((la * lb) * lc + mq_dot(A, B) * lc) + mq_dot(B, C) * la) + mq_dot(C, A) * lb;
  return 2.f * atan2f(det, den);
}

template <bool CLOSEST, bool WINDING>
__global__ __launch_bounds__(MDQ_THREADS) void md_mesh_query_kernel(const float* __restrict__ tri, const int32_t* __restrict__ tri_ptr,
                                                                    const float* __restrict__ query,
                                                                    const int32_t* __restrict__ query_ptr, int T, int Q,
                                                                    float* __restrict__ dist2, int32_t* __restrict__ face,
                                                                    float* __restrict__ closest, float* __restrict__ winding) {
  __shared__ float4 tile[MDQ_TILE * 3];
  const int tid = threadIdx.x, m = blockIdx.y;
  const int q_lo = min(max(query_ptr[m], 0), Q), q_hi = min(max(query_ptr[m + 1], q_lo), Q);
  const int t_lo = min(max(tri_ptr[m], 0), T), t_hi = min(max(tri_ptr[m + 1], t_lo), T);
  const int64_t q0 = (int64_t)q_lo + (int64_t)blockIdx.x * (MDQ_THREADS * MDQ_QPL);
  if (q0 >= q_hi) return;                                     // workgroup-uniform, before the first barrier

  mq_v3 p[MDQ_QPL], best_c[MDQ_QPL];
  float best[MDQ_QPL];
  int best_f[MDQ_QPL];
  double wsum[MDQ_QPL];
  bool live[MDQ_QPL];
#pragma unroll
  for (int k = 0; k < MDQ_QPL; ++k) {
    const int64_t q = q0 + k * MDQ_THREADS + tid;
    live[k] = q < q_hi;
    const int64_t qc = live[k] ? q : (int64_t)q_hi - 1;       // lanes past the end repeat the last query; nothing is written for them
    p[k] = {query[qc * 3], query[qc * 3 + 1], query[qc * 3 + 2]};
    best_c[k] = p[k];
    best[k] = __builtin_inff();
    best_f[k] = -1;
    wsum[k] = 0.0;
  }

  for (int t0 = t_lo; t0 < t_hi; t0 += MDQ_TILE) {
    const int cnt = min(t_hi - t0, MDQ_TILE);
    if (tid < cnt) {
      const float* s = tri + (int64_t)(t0 + tid) * 9;
      const mq_v3 a = {s[0], s[1], s[2]}, b = {s[3], s[4], s[5]}, c = {s[6], s[7], s[8]};
      const mq_v3 ab = mq_sub(b, a), ac = mq_sub(c, a);
      tile[tid * 3] = make_float4(a.x, a.y, a.z, 0.f);
      tile[tid * 3 + 1] = make_float4(ab.x, ab.y, ab.z, 0.f);
      tile[tid * 3 + 2] = make_float4(ac.x, ac.y, ac.z, 0.f);
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float4 ta = tile[j * 3], tb = tile[j * 3 + 1], tc = tile[j * 3 + 2];
      const mq_v3 a = {ta.x, ta.y, ta.z}, ab = {tb.x, tb.y, tb.z}, ac = {tc.x, tc.y, tc.z};
#pragma unroll
      for (int k = 0; k < MDQ_QPL; ++k) {
        if (CLOSEST) {
          mq_v3 c;
          const float d = mq_closest(p[k], a, ab, ac, c);
          const bool take = d < best[k];                      // false on NaN and on a tie
          best[k] = take ? d : best[k];
          best_f[k] = take ? t0 + j : best_f[k];
          best_c[k].x = take ? c.x : best_c[k].x;
          best_c[k].y = take ? c.y : best_c[k].y;
          best_c[k].z = take ? c.z : best_c[k].z;
        }
        if (WINDING) wsum[k] += (double)mq_omega(p[k], a, ab, ac);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < MDQ_QPL; ++k) {
    if (!live[k]) continue;
    const int64_t q = q0 + k * MDQ_THREADS + tid;
    if (CLOSEST) {
      if (dist2) dist2[q] = best[k];
      if (face) face[q] = best_f[k];
      if (closest) { closest[q * 3] = best_c[k].x; closest[q * 3 + 1] = best_c[k].y; closest[q * 3 + 2] = best_c[k].z; }
    }
    if (WINDING) winding[q] = (float)(wsum[k] / 12.566370614359172);      // 4 pi
  }
}

template <bool CLOSEST, bool WINDING>
static int mq_launch(const float* tri, const int32_t* tri_ptr, const float* query, const int32_t* query_ptr, int64_t T, int64_t Q,
                     int64_t M, float* dist2, int32_t* face, float* closest, float* winding, void* stream) {
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL((md_mesh_query_kernel<CLOSEST, WINDING>), dim3(md_blocks(Q, MDQ_THREADS * MDQ_QPL), (unsigned)M), dim3(MDQ_THREADS),
                     0, (hipStream_t)stream, tri, tri_ptr, query, query_ptr, (int)T, (int)Q, dist2, face, closest, winding);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_mesh_query(const float* tri, const int32_t* tri_ptr, const float* query, const int32_t* query_ptr, int64_t n_tris,
                             int64_t n_queries, int64_t n_meshes, float* dist2, int32_t* face, float* closest, float* winding,
                             void* stream) {
  // 1 pointers: tri may be null only when there is no triangle to read
  if (md_any_bad<4>(tri_ptr, query, query_ptr) || md_any_misaligned<4>(tri, dist2, face, closest, winding)) return MD_ERR_BAD_ARG;
  if (!dist2 && !face && !closest && !winding) return MD_ERR_BAD_ARG;
  // 2 counts
  if (n_tris < 0 || n_queries < 0 || n_meshes < 0 || (!tri && n_tris > 0)) return MD_ERR_BAD_ARG;
  // 3 limits: the kernel counts triangles and queries in int (and addresses them in int64); gridDim.y = M
  static_assert(MDQ_MAX_MESHES == MD_MESHDIST_MAX_MESHES, "the header states the cap");
  if (!md_fits_i32(n_tris, n_queries) || n_meshes > MDQ_MAX_MESHES) return MD_ERR_UNSUPPORTED;
  // 4 aliasing: an output is none of the inputs
  const void* in[4] = {tri, tri_ptr, query, query_ptr};
  const void* out[4] = {dist2, face, closest, winding};
  for (const void* o : out)
    for (const void* i : in)
      if (o && o == i) return MD_ERR_BAD_ARG;
  if (n_queries == 0 || n_meshes == 0) return MD_OK;
  const bool want_closest = dist2 || face || closest;
  if (want_closest && winding) return mq_launch<true, true>(tri, tri_ptr, query, query_ptr, n_tris, n_queries, n_meshes, dist2, face, closest, winding, stream);
  if (want_closest) return mq_launch<true, false>(tri, tri_ptr, query, query_ptr, n_tris, n_queries, n_meshes, dist2, face, closest, winding, stream);
  return mq_launch<false, true>(tri, tri_ptr, query, query_ptr, n_tris, n_queries, n_meshes, dist2, face, closest, winding, stream);
}
