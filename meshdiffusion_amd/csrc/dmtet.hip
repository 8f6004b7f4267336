// Marching tetrahedra on a static tet grid: chunks of 1024 edges / tets per workgroup, M meshes per call, four launches
// (count -> per-mesh scan of the chunk totals -> vertices -> faces) so that 32 meshes of the 64-resolution grid are
// ~11 000 workgroups instead of 32 (one workgroup per mesh ran on 32 of the 256 CUs at ~95 GB/s, latency-bound).
//
// Reference: nvdiffrec/lib/geometry/dmtet.py:105-163 (DMTet.__call__), LUTs :34-54.
// The reference sorts+uniques the edges of the valid tets at run time (torch.unique(dim=0));
// because the tet grid is static we precompute ONCE the lexicographically sorted unique edge
// list of all tets and the tet->edge-id table.  A crossing edge (exactly one endpoint with
// sdf > 0) always belongs to a valid tet, so numbering the crossing edges by an exclusive
// prefix sum over that static sorted order reproduces the reference's vertex ids exactly;
// faces are emitted 1-triangle tets first (tet order), then 2-triangle tets, like the
// reference's torch.cat.  Prefix sums: wave-level ballots + popcounts (wave64) inside a chunk, the chunk offsets from the
// scan kernel -- every number is an integer, so the result does not depend on how the work is cut.
#include "md_args.h"

#pragma clang fp contract(off)

static constexpr int MT_THREADS = 1024;          // = items (edges or tets) per chunk
static constexpr int MT_WAVES = MT_THREADS / 64;

__device__ __constant__ int8_t c_tri_table[16][6] = {
    {-1, -1, -1, -1, -1, -1}, {1, 0, 2, -1, -1, -1}, {4, 0, 3, -1, -1, -1}, {1, 4, 2, 1, 3, 4},
    {3, 1, 5, -1, -1, -1},    {2, 3, 0, 2, 5, 3},    {1, 4, 0, 1, 5, 4},    {4, 2, 5, -1, -1, -1},
    {4, 5, 2, -1, -1, -1},    {4, 1, 0, 4, 5, 1},    {3, 2, 0, 3, 5, 2},    {1, 3, 5, -1, -1, -1},
    {4, 1, 2, 4, 3, 1},       {3, 0, 4, -1, -1, -1}, {2, 0, 1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1}};
__device__ __constant__ int8_t c_num_tri[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};

// exclusive prefix of a 0/1 flag over the 1024-thread block; returns block total via `total`.
__device__ __forceinline__ int block_excl_scan_flag(bool flag, int* lds_wave, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  const int wprefix = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) lds_wave[wid] = __popcll(bal);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < MT_WAVES; ++w) {
    const int c = lds_wave[w];
    if (w < wid) base += c;
    tot += c;
  }
  __syncthreads();
  total = tot;
  return base + wprefix;
}

// exclusive prefix of an int over the block
__device__ __forceinline__ int block_excl_scan_int(int v, int* lds_wave, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) lds_wave[wid] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < MT_WAVES; ++w) {
    const int c = lds_wave[w];
    if (w < wid) base += c;
    tot += c;
  }
  __syncthreads();
  total = tot;
  return base + inc - v;
}

struct MtArgs {
  const float* pos; const float* sdf; const int32_t* tets; const int32_t* edges; const int32_t* tet_edges;
  int n_verts, n_edges, n_tets, ce, ct;           // ce / ct: edge / tet chunks per mesh
  float* verts; int64_t* faces; int64_t* face_tet; int32_t* counts;
  int32_t* vid;                                   // [M][E]  edge -> vertex id or -1
  int32_t* chunk;                                 // [M][ce + 2 ct]: crossing edges per edge chunk | 1-triangle | 2-triangle tets per tet chunk
};

__device__ __forceinline__ int mt_tet_case(const float* msdf, const int32_t* tets, int t) {
  const int4 tv = *(const int4*)(tets + 4 * (int64_t)t);
  return ((msdf[tv.x] > 0.f) ? 1 : 0) | ((msdf[tv.y] > 0.f) ? 2 : 0) | ((msdf[tv.z] > 0.f) ? 4 : 0) | ((msdf[tv.w] > 0.f) ? 8 : 0);
}

// ---- launch 1: per-chunk totals.  blockIdx.x < ce: an edge chunk, else a tet chunk; blockIdx.y = mesh ----
__global__ __launch_bounds__(MT_THREADS) void md_mt_count_kernel(const MtArgs g) {
  __shared__ int lds_red[2][MT_WAVES];
  const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* msdf = g.sdf + (int64_t)m * g.n_verts;
  int32_t* mchunk = g.chunk + (int64_t)m * (g.ce + 2 * g.ct);
  bool f1 = false, f2 = false;
  const bool is_edge = (int)blockIdx.x < g.ce;
  if (is_edge) {
    const int e = blockIdx.x * MT_THREADS + tid;
    if (e < g.n_edges) {
      const int2 ab = *(const int2*)(g.edges + 2 * (int64_t)e);
      f1 = (msdf[ab.x] > 0.f) != (msdf[ab.y] > 0.f);
    }
  } else {
    const int t = (blockIdx.x - g.ce) * MT_THREADS + tid;
    if (t < g.n_tets) {
      const int nt = c_num_tri[mt_tet_case(msdf, g.tets, t)];
      f1 = nt == 1; f2 = nt == 2;
    }
  }
  const int w1 = __popcll(__ballot(f1)), w2 = __popcll(__ballot(f2));
  if (lane == 0) { lds_red[0][wid] = w1; lds_red[1][wid] = w2; }
  __syncthreads();
  if (tid == 0) {
    int s1 = 0, s2 = 0;
#pragma unroll
    for (int w = 0; w < MT_WAVES; ++w) { s1 += lds_red[0][w]; s2 += lds_red[1][w]; }
    if (is_edge) mchunk[blockIdx.x] = s1;
    else { mchunk[blockIdx.x] = s1; mchunk[blockIdx.x + g.ct] = s2; }
  }
}

// ---- launch 2: one workgroup per mesh turns the chunk totals into exclusive offsets (in place) and writes counts ----
__global__ __launch_bounds__(MT_THREADS) void md_mt_scan_kernel(const MtArgs g) {
  __shared__ int lds_wave[MT_WAVES];
  const int m = blockIdx.x, tid = threadIdx.x;
  int32_t* mchunk = g.chunk + (int64_t)m * (g.ce + 2 * g.ct);
  int tot3[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int32_t* arr = mchunk + (a == 0 ? 0 : (a == 1 ? g.ce : g.ce + g.ct));
    const int n = a == 0 ? g.ce : g.ct;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += MT_THREADS) {
      const int i = i0 + tid;
      const int v = i < n ? arr[i] : 0;
      int tot;
      const int pre = block_excl_scan_int(v, lds_wave, tot);
      if (i < n) arr[i] = base + pre;
      base += tot;
    }
    tot3[a] = base;
  }
  if (tid == 0) {
    g.counts[m * 4 + 0] = tot3[0];
    g.counts[m * 4 + 1] = tot3[1] + 2 * tot3[2];
    g.counts[m * 4 + 2] = tot3[1];
    g.counts[m * 4 + 3] = tot3[2];
  }
}

// ---- launch 3: crossing edges -> vertex ids + interpolated positions ----
__global__ __launch_bounds__(MT_THREADS) void md_mt_verts_kernel(const MtArgs g) {
  __shared__ int lds_wave[MT_WAVES];
  const int m = blockIdx.y, tid = threadIdx.x;
  const float* mpos = g.pos + (int64_t)m * g.n_verts * 3;
  const float* msdf = g.sdf + (int64_t)m * g.n_verts;
  float* mverts = g.verts + (int64_t)m * g.n_edges * 3;
  int32_t* vid = g.vid + (int64_t)m * g.n_edges;
  const int vbase = g.chunk[(int64_t)m * (g.ce + 2 * g.ct) + blockIdx.x];
  const int e = blockIdx.x * MT_THREADS + tid;
  bool cross = false;
  int a = 0, b = 0;
  float sa = 0.f, sb = 0.f;
  if (e < g.n_edges) {
    const int2 ab = *(const int2*)(g.edges + 2 * (int64_t)e);
    a = ab.x; b = ab.y;
    sa = msdf[a]; sb = msdf[b];
    cross = (sa > 0.f) != (sb > 0.f);
  }
  int tot;
  const int pre = block_excl_scan_flag(cross, lds_wave, tot);
  if (e < g.n_edges) {
    if (cross) {
      const int v = vbase + pre;
      vid[e] = v;
      // reference: sdf pair (s0, -s1); w = flip(pair)/sum(pair); vert = p0*w0 + p1*w1
      const float nsb = -sb;
      const float den = sa + nsb;
      const float w0 = nsb / den, w1 = sa / den;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float t0 = mpos[a * 3 + k] * w0;
        const float t1 = mpos[b * 3 + k] * w1;
        mverts[(int64_t)v * 3 + k] = t0 + t1;
      }
    } else {
      vid[e] = -1;
    }
  }
}

// ---- launch 4: faces (1-triangle tets first, then 2-triangle tets, both in tet order) ----
__global__ __launch_bounds__(MT_THREADS) void md_mt_faces_kernel(const MtArgs g) {
  __shared__ int lds_wave[MT_WAVES];
  const int m = blockIdx.y, tid = threadIdx.x;
  const float* msdf = g.sdf + (int64_t)m * g.n_verts;
  int64_t* mfaces = g.faces + (int64_t)m * g.n_tets * 2 * 3;
  int64_t* mftet = g.face_tet ? g.face_tet + (int64_t)m * g.n_tets * 2 : nullptr;
  const int32_t* vid = g.vid + (int64_t)m * g.n_edges;
  const int32_t* mchunk = g.chunk + (int64_t)m * (g.ce + 2 * g.ct);
  const int b1 = mchunk[g.ce + blockIdx.x], b2 = mchunk[g.ce + g.ct + blockIdx.x];
  const int N1 = g.counts[m * 4 + 2];
  const int t = blockIdx.x * MT_THREADS + tid;
  int idx = 0, nt = 0;
  if (t < g.n_tets) {
    idx = mt_tet_case(msdf, g.tets, t);
    nt = c_num_tri[idx];
  }
  int tot1, tot2;
  const int p1 = block_excl_scan_flag(nt == 1, lds_wave, tot1);
  const int p2 = block_excl_scan_flag(nt == 2, lds_wave, tot2);
  if (nt > 0) {
    int ev[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) ev[k] = vid[g.tet_edges[6 * (int64_t)t + k]];
    const int64_t f0 = (nt == 1) ? (int64_t)(b1 + p1) : (int64_t)N1 + 2 * (int64_t)(b2 + p2);
    for (int f = 0; f < nt; ++f) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int ei = c_tri_table[idx][f * 3 + k];
        int v = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) v = (ei == q) ? ev[q] : v;
        mfaces[(f0 + f) * 3 + k] = (int64_t)v;
      }
      if (mftet) mftet[f0 + f] = (int64_t)t;
    }
  }
}

static inline int mt_chunks(int32_t n) { return (n + MT_THREADS - 1) / MT_THREADS; }

extern "C" int64_t md_marching_tets_workspace_bytes(int32_t n_meshes, int32_t n_edges, int32_t n_tets) {
  if (n_meshes <= 0 || n_edges <= 0 || n_tets <= 0) return MD_ERR_BAD_ARG;
  return (int64_t)n_meshes * ((int64_t)n_edges + mt_chunks(n_edges) + 2 * mt_chunks(n_tets)) * 4;
}

extern "C" int md_marching_tets(const float* pos, const float* sdf, const int32_t* tets,
                                const int32_t* edges, const int32_t* tet_edges, int32_t n_meshes,
                                int32_t n_verts, int32_t n_edges, int32_t n_tets, float* verts,
                                int64_t* faces, int64_t* face_tet, int32_t* counts, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  if (md_any_bad<1>(pos, sdf, tets, edges, tet_edges, verts, faces, counts, workspace) ||
      n_meshes <= 0 || n_verts <= 0 || n_edges <= 0 || n_tets <= 0)
    return MD_ERR_BAD_ARG;
  if (workspace_bytes < md_marching_tets_workspace_bytes(n_meshes, n_edges, n_tets)) return MD_ERR_BAD_ARG;
  if (n_meshes > 65535) return MD_ERR_UNSUPPORTED;             // gridDim.y
  if (md_any_misaligned<16>(tets) || md_any_misaligned<8>(edges)) return MD_ERR_BAD_ARG;   // read as int4 / int2 rows
  MtArgs g;
  g.pos = pos; g.sdf = sdf; g.tets = tets; g.edges = edges; g.tet_edges = tet_edges;
  g.n_verts = n_verts; g.n_edges = n_edges; g.n_tets = n_tets; g.ce = mt_chunks(n_edges); g.ct = mt_chunks(n_tets);
  g.verts = verts; g.faces = faces; g.face_tet = face_tet; g.counts = counts;
  g.vid = (int32_t*)workspace;
  g.chunk = g.vid + (int64_t)n_meshes * n_edges;
  const hipStream_t st = (hipStream_t)stream;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_mt_count_kernel, dim3((unsigned)(g.ce + g.ct), (unsigned)n_meshes), dim3(MT_THREADS), 0, st, g);
  hipLaunchKernelGGL(md_mt_scan_kernel, dim3((unsigned)n_meshes), dim3(MT_THREADS), 0, st, g);
  hipLaunchKernelGGL(md_mt_verts_kernel, dim3((unsigned)g.ce, (unsigned)n_meshes), dim3(MT_THREADS), 0, st, g);
  hipLaunchKernelGGL(md_mt_faces_kernel, dim3((unsigned)g.ct, (unsigned)n_meshes), dim3(MT_THREADS), 0, st, g);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

// ---- smooth vertex normals of an extracted mesh (nvdiffrec/lib/render/mesh.py:200-229 `auto_normals`) ----------------
// f_nrm = cross(v1 - v0, v2 - v0) per face, splatted onto its three vertices (scatter_add in the reference: float
// atomics here, so the summation order -- not the set of terms -- differs), then v / sqrt(max(v.v, 1e-20)) with
// degenerate sums (v.v <= 1e-20) replaced by (0, 0, 1) first (util.safe_normalize, util.py:33-35).
__global__ void md_face_normals_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces, int64_t F,
                                       float* __restrict__ v_nrm, float* __restrict__ f_nrm) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int64_t i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  const float ax = verts[i1 * 3] - verts[i0 * 3], ay = verts[i1 * 3 + 1] - verts[i0 * 3 + 1], az = verts[i1 * 3 + 2] - verts[i0 * 3 + 2];
  const float bx = verts[i2 * 3] - verts[i0 * 3], by = verts[i2 * 3 + 1] - verts[i0 * 3 + 1], bz = verts[i2 * 3 + 2] - verts[i0 * 3 + 2];
  const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  if (f_nrm) { f_nrm[f * 3] = nx; f_nrm[f * 3 + 1] = ny; f_nrm[f * 3 + 2] = nz; }
  const int64_t idx[3] = {i0, i1, i2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    atomicAdd(v_nrm + idx[k] * 3, nx); atomicAdd(v_nrm + idx[k] * 3 + 1, ny); atomicAdd(v_nrm + idx[k] * 3 + 2, nz);
  }
}

__global__ void md_normalize_normals_kernel(float* __restrict__ v_nrm, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  float x = v_nrm[v * 3], y = v_nrm[v * 3 + 1], z = v_nrm[v * 3 + 2];
  float d = x * x + y * y + z * z;
  if (!(d > 1e-20f)) { x = 0.f; y = 0.f; z = 1.f; d = 1.f; }
  const float len = sqrtf(fmaxf(d, 1e-20f));
  v_nrm[v * 3] = x / len; v_nrm[v * 3 + 1] = y / len; v_nrm[v * 3 + 2] = z / len;
}

extern "C" int md_vertex_normals(const float* verts, const int64_t* faces, int64_t n_verts, int64_t n_faces, float* v_nrm,
                                 float* f_nrm, void* stream) {
  if (md_any_bad<1>(verts, faces, v_nrm) || n_verts <= 0 || n_faces < 0) return MD_ERR_BAD_ARG;
  hipError_t e = hipMemsetAsync(v_nrm, 0, (size_t)n_verts * 3 * sizeof(float), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  MD_HIP_CLEAR_ERROR();
  if (n_faces > 0)
    hipLaunchKernelGGL(md_face_normals_kernel, dim3(md_blocks(n_faces, 256)), dim3(256), 0, (hipStream_t)stream, verts,
                       faces, n_faces, v_nrm, f_nrm);
  hipLaunchKernelGGL(md_normalize_normals_kernel, dim3(md_blocks(n_verts, 256)), dim3(256), 0, (hipStream_t)stream,
                     v_nrm, n_verts);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
