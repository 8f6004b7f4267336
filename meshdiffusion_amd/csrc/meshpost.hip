// What every user of the reference runs right after sampling, the tail of nvdiffrec/eval.py:421-456: a quick-look image of the
// mesh (bsdf = 'diffuse', kd = (0.75, 0.3, 0.6), an environment light, the two-sided geometric normal of render.py:100-102 and
// light.py:120-122) and a clean-up (pymeshlab: apply_coord_laplacian_smoothing).  Built IN THE MANNER OF that tail under a contract
// of its own, not bit-equal to MeshLab or nvdiffrast: connected components with a floater filter, umbrella (Laplacian / Taubin)
// smoothing and diffuse shading from nine spherical-harmonic coefficients, batched over the meshes of one marching-tetrahedra
// launch.  It runs after generation, not inside a fit: nothing here has a gradient.
//
// THE MESH POST-PROCESSING CONTRACT (tests/meshpost_cases.py restates it in torch / numpy)
//   Mesh batch  concatenated form: verts fp32 [V][3], faces int64 [F][3] of GLOBAL vertex ids.  M meshes laid end to end share no
//               edge, so every kernel here is batched without knowing M; the host keeps vert_mesh int32 [V], the mesh of a vertex,
//               only for "the largest component of the same mesh".
//   Edge table  (host, meshdiffusion_amd/postprocess.py mesh_edges) the 3 F corner edges (faces[f][(k+1)%3], faces[f][(k+2)%3]), those
//               with a == b dropped, keyed min * V + max, sorted stably and uniqued into E undirected edges (lo, hi, mult).  An edge is
//               a BOUNDARY edge iff mult == 1; mult >= 3 counts as interior.  Neighbour CSR: ptr int32 [V+1], adj int32 [2 E] of the
//               codes 2 * neighbour + (1 if the edge is a boundary edge), ascending by neighbour inside a row.  A vertex is a
//               BOUNDARY vertex iff its row holds a boundary code.
//   Smoothing   `steps` steps; step i uses w = lam if i is even or mu is NaN (unset), else w = mu (Taubin's lambda | mu).  Per vertex
//               v with row R: a boundary vertex keeps only its boundary codes (a boundary moves along itself); n = |R|; n == 0: the
//               vertex keeps its bits.  Otherwise per component s = the compensated sum (md_kahan_add) of the neighbours' coordinates
//               in row order, m = s / (float)n, x' = x + w * (m - x).  Ping-pong buffers, one launch per step, the input is never
//               written; steps == 0 copies.
//   Components  label[v] = the smallest vertex index connected to v.  A face connects its three indices, a degenerate face too; a
//               vertex no face names is its own component.  Hook and compress: label[v] = v; a round is two kernels: one thread per
//               face chases `label` from its three indices to their roots and atomicMin's the smallest root into the other two; one
//               thread per vertex then chases its chain and stores the root.  label[v] <= v always holds, so every chase is
//               strictly decreasing and ends whatever a racing thread writes; correctness relies on visibility BETWEEN launches only
//               (the loads are relaxed atomics, which the compiler may not hoist).  A device flag records "some hook lowered a
//               label"; rounds run until a round leaves it clear, at most MD_MESHPOST_MAX_ROUNDS = 64, then MD_ERR_UNSUPPORTED.  The
//               result is the unique fixed point: it does not depend on the order the atomics land in.  comp_faces int32 [V]: at
//               index label, the number of faces whose FIRST vertex carries that label (integer atomics), 0 elsewhere.
//   Shading     forward only.  rast fp32 [B][H][W][4] one layer of the rasteriser, campos fp32 [B][3], sh fp32 [9][3] radiance
//               coefficients in the real spherical-harmonic basis of bands 0-2 ordered (0,0), (1,-1), (1,0), (1,1), (2,-2) .. (2,2),
//               kd fp32 [3].  A pixel with 1 <= id <= F, (p0, p1, p2) the face's vertices, (u, v) = rast.xy:
//                 p = (u p0 + v p1) + t p2, t = (1 - u) - v                       the order of md_interpolate
//                 g = cross(p1 - p0, p2 - p0), geo = g / sqrt(max(g . g, 1e-20))
//                 d = c - p, view = d / max(sqrt(d . d), 1e-12)
//                 n = geo if geo . view > 0 else -geo
//                 Y = (0.282095, 0.488603 y, 0.488603 z, 0.488603 x, 1.092548 x y, 1.092548 y z, 0.315392 (3 z z - 1), 1.092548 x z,
//                      0.546274 (x x - y y)) at n = (x, y, z)
//                 e_c = sum over k = 0..8, in that order, of (A_k Y_k) sh[k][c], A = (1, 2/3, 2/3, 2/3, 1/4, 1/4, 1/4, 1/4, 1/4)
//                 out = (kd_c max(e_c, 0), 1)
//               (dot products are (x x + y y) + z z.)  e is irradiance over pi: a uniform white environment of radiance 1 gives kd.
//               Every other pixel is four zeros; an id above F is never an index.
//   Arithmetic  fp32, every operation rounded on its own (no contraction); no floating-point atomics: two runs agree bit for bit.
//               Integer atomicMin / atomicAdd only.
//   Limits      sizes are int64 at the boundary: null pointers and non-positive sizes MD_ERR_BAD_ARG; V, 2 V (the codes), 2 E or 3 F
//               beyond int32, F >= 2^24 / H, W > 2048 / B > 64 for shading MD_ERR_UNSUPPORTED; lam must be finite, mu finite or NaN.
//               The host checks index ranges once; the kernels treat an index outside its table as absent and never read there.
//               The library allocates nothing: the caller passes the scratch.
//
// Kernels.  Latency- and HBM-bound gathers over short rows (valence ~6 on a marching-tets mesh) and one pass over the pixels: one
// thread per row, face or pixel, 256-thread workgroups, no LDS, plain stores.
#include "md_args.h"
#include "md_gather.h"

#pragma clang fp contract(off)

static constexpr int MP_THREADS = 256;

// ---- smoothing -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void md_mp_smooth_kernel(const float* __restrict__ src, const int32_t* __restrict__ ptr,
                                                                  const int32_t* __restrict__ adj, int V, int n_codes, float w,
                                                                  float* __restrict__ dst) {
  const int v = blockIdx.x * MP_THREADS + threadIdx.x;
  if (v >= V) return;
  const int j0 = max(ptr[v], 0), j1 = min(ptr[v + 1], n_codes);
  bool boundary = false;
  for (int j = j0; j < j1; ++j) {
    const int code = adj[j];
    if ((unsigned)(code >> 1) < (unsigned)V && (code & 1)) boundary = true;
  }
  float s[3] = {0.f, 0.f, 0.f}, lost[3] = {0.f, 0.f, 0.f};
  int n = 0;
  for (int j = j0; j < j1; ++j) {
    const int code = adj[j];
    const int u = code >> 1;
    if ((unsigned)u >= (unsigned)V) continue;                 // never with the table of the host
    if (boundary && !(code & 1)) continue;
    const float* q = src + (int64_t)u * 3;
    md_kahan_add(s[0], lost[0], q[0]);
    md_kahan_add(s[1], lost[1], q[1]);
    md_kahan_add(s[2], lost[2], q[2]);
    ++n;
  }
  const float* x = src + (int64_t)v * 3;
  float* o = dst + (int64_t)v * 3;
  if (n == 0) {
    o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
    return;
  }
  const float fn = (float)n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float m = s[c] / fn;
    o[c] = x[c] + w * (m - x[c]);
  }
}

// ---- connected components ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mp_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v: label <= index makes the chain strictly decreasing, so it ends after at most v steps whatever is written meanwhile
__device__ __forceinline__ int mp_root(const int32_t* label, int v) {
  int r = v;
  for (;;) {
    const int l = mp_load(label + r);
    if (l >= r || l < 0) return r;
    r = l;
  }
}

__global__ __launch_bounds__(MP_THREADS) void md_mp_init_kernel(int V, int32_t* __restrict__ label, int32_t* __restrict__ comp_faces) {
  const int v = blockIdx.x * MP_THREADS + threadIdx.x;
  if (v >= V) return;
  label[v] = v;
  comp_faces[v] = 0;
}

__global__ __launch_bounds__(MP_THREADS) void md_mp_hook_kernel(const int64_t* __restrict__ faces, int V, int F, int32_t* label,
                                                                int32_t* flag) {
  const int f = blockIdx.x * MP_THREADS + threadIdx.x;
  if (f >= F) return;
  int r[3], nr = 0, m = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t i = faces[(int64_t)f * 3 + k];
    if (i < 0 || i >= V) continue;                            // absent
    r[nr] = mp_root(label, (int)i);
    m = min(m, r[nr]);
    ++nr;
  }
  bool lowered = false;
  for (int k = 0; k < nr; ++k)
    if (r[k] > m && atomicMin(label + r[k], m) > m) lowered = true;
  if (lowered) atomicOr(flag, 1);
}

__global__ __launch_bounds__(MP_THREADS) void md_mp_compress_kernel(int V, int32_t* label) {
  const int v = blockIdx.x * MP_THREADS + threadIdx.x;
  if (v >= V) return;
  const int r = mp_root(label, v);
  if (r < v) __hip_atomic_store(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(MP_THREADS) void md_mp_count_kernel(const int64_t* __restrict__ faces, const int32_t* __restrict__ label,
                                                                 int V, int F, int32_t* comp_faces) {
  const int f = blockIdx.x * MP_THREADS + threadIdx.x;
  if (f >= F) return;
  const int64_t i = faces[(int64_t)f * 3];
  if (i < 0 || i >= V) return;
  const int l = label[i];
  if ((unsigned)l < (unsigned)V) atomicAdd(comp_faces + l, 1);
}

// ---- diffuse shading -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void md_mp_shade_kernel(const float* __restrict__ rast, const float* __restrict__ verts,
                                                                 const int64_t* __restrict__ faces, const float* __restrict__ campos,
                                                                 const float* __restrict__ sh, const float* __restrict__ kd, int V,
                                                                 int F, int HW, float* __restrict__ out) {
  const int pix = blockIdx.x * MP_THREADS + threadIdx.x;
  if (pix >= HW) return;
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * HW + pix;
  const float4 r = *reinterpret_cast<const float4*>(rast + o * 4);
  float4 res = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r.w >= 1.f && r.w <= (float)F) {
    const int64_t f = (int64_t)r.w - 1;
    const int64_t i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
      float p0[3], p1[3], p2[3], p[3], a[3], e[3], d[3];
      const float t = (1.f - r.x) - r.y;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p0[c] = verts[i0 * 3 + c]; p1[c] = verts[i1 * 3 + c]; p2[c] = verts[i2 * 3 + c];
        p[c] = (r.x * p0[c] + r.y * p1[c]) + t * p2[c];
        a[c] = p1[c] - p0[c];
        e[c] = p2[c] - p0[c];
        d[c] = campos[b * 3 + c] - p[c];
      }
      const float g[3] = {a[1] * e[2] - a[2] * e[1], a[2] * e[0] - a[0] * e[2], a[0] * e[1] - a[1] * e[0]};
      const float glen = sqrtf(fmaxf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2], 1e-20f));
      const float dlen = fmaxf(sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), 1e-12f);
      float n[3], view[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { n[c] = g[c] / glen; view[c] = d[c] / dlen; }
      const float gv = (n[0] * view[0] + n[1] * view[1]) + n[2] * view[2];
      if (!(gv > 0.f)) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
      const float x = n[0], y = n[1], z = n[2];
      const float third2 = 2.f / 3.f;
      const float ay[9] = {0.282095f,
                           third2 * (0.488603f * y), third2 * (0.488603f * z), third2 * (0.488603f * x),
                           0.25f * (1.092548f * (x * y)), 0.25f * (1.092548f * (y * z)), 0.25f * (0.315392f * (3.f * (z * z) - 1.f)),
                           0.25f * (1.092548f * (x * z)), 0.25f * (0.546274f * (x * x - y * y))};
      float col[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float acc = ay[0] * sh[c];
#pragma unroll
        for (int k = 1; k < 9; ++k) acc = acc + ay[k] * sh[k * 3 + c];
        col[c] = kd[c] * fmaxf(acc, 0.f);
      }
      res = make_float4(col[0], col[1], col[2], 1.f);
    }
  }
  *reinterpret_cast<float4*>(out + o * 4) = res;
}

// ---- exports -------------------------------------------------------------------------------------------------------------------
extern "C" int md_mesh_smooth(const float* verts, const int32_t* ptr, const int32_t* adj, int64_t n_verts, int64_t n_codes,
                              int32_t steps, float lam, float mu, float* out, float* scratch, void* stream) {
  if (md_any_bad<4>(verts, ptr, adj, out) || md_any_misaligned<4>(scratch) || (steps >= 2 && !scratch)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_codes <= 0 || steps < 0) return MD_ERR_BAD_ARG;
  if (!(fabsf(lam) <= 3.402823466e+38f) || !(mu != mu || fabsf(mu) <= 3.402823466e+38f)) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(2 * n_verts, n_codes)) return MD_ERR_UNSUPPORTED;          // the codes 2 * neighbour + 1 fit int32
  if (out == verts || scratch == verts || (steps >= 2 && out == scratch)) return MD_ERR_BAD_ARG;  // the input is never written
  const hipStream_t st = (hipStream_t)stream;
  MD_HIP_CLEAR_ERROR();
  if (steps == 0) {
    const hipError_t e = hipMemcpyAsync(out, verts, (size_t)n_verts * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? MD_OK : (int)e;
  }
  const float* src = verts;
  for (int i = 0; i < steps; ++i) {
    float* dst = ((steps - 1 - i) & 1) ? scratch : out;                                          // the last step lands in `out`
    const float w = ((i & 1) == 0 || mu != mu) ? lam : mu;
    hipLaunchKernelGGL(md_mp_smooth_kernel, dim3(md_blocks(n_verts, MP_THREADS)), dim3(MP_THREADS), 0, st, src, ptr, adj, (int)n_verts,
                       (int)n_codes, w, dst);
    src = dst;
  }
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_mesh_components(const int64_t* faces, int64_t n_verts, int64_t n_faces, int32_t* label, int32_t* comp_faces,
                                  void* workspace, int32_t* rounds, void* stream) {
  if (rounds) *rounds = 0;
  if (md_any_bad<8>(faces) || md_any_bad<4>(label, comp_faces, workspace)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_faces <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 3 * n_faces)) return MD_ERR_UNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  const int V = (int)n_verts, F = (int)n_faces;
  int32_t* flag = (int32_t*)workspace;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_mp_init_kernel, dim3(md_blocks(V, MP_THREADS)), dim3(MP_THREADS), 0, st, V, label, comp_faces);
  MD_HIP_CHECK_LAUNCH();
  bool settled = false;
  for (int round = 1; round <= MD_MESHPOST_MAX_ROUNDS && !settled; ++round) {
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(md_mp_hook_kernel, dim3(md_blocks(F, MP_THREADS)), dim3(MP_THREADS), 0, st, faces, V, F, label, flag);
    hipLaunchKernelGGL(md_mp_compress_kernel, dim3(md_blocks(V, MP_THREADS)), dim3(MP_THREADS), 0, st, V, label);
    MD_HIP_CHECK_LAUNCH();
    int32_t host_flag = 1;
    e = hipMemcpyAsync(&host_flag, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st);            // the one 4-byte copy of a round
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (rounds) *rounds = round;
    settled = host_flag == 0;
  }
  if (!settled) return MD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(md_mp_count_kernel, dim3(md_blocks(F, MP_THREADS)), dim3(MP_THREADS), 0, st, faces, (const int32_t*)label, V, F,
                     comp_faces);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_shade_diffuse(const float* rast, const float* verts, const int64_t* faces, const float* campos, const float* sh,
                                const float* kd, int32_t batch, int64_t n_verts, int64_t n_faces, int32_t H, int32_t W, float* out,
                                void* stream) {
  if (md_any_bad<16>(rast, out) || md_any_bad<8>(faces) || md_any_bad<4>(verts, campos, sh, kd)) return MD_ERR_BAD_ARG;
  if (batch <= 0 || n_verts <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (batch > 64 || H > 2048 || W > 2048 || !md_fits_i32(n_verts) || n_faces >= (1LL << 24)) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_mp_shade_kernel, dim3(md_blocks((int64_t)H * W, MP_THREADS), (unsigned)batch), dim3(MP_THREADS), 0,
                     (hipStream_t)stream, rast, verts, faces, campos, sh, kd, (int)n_verts, (int)n_faces, (int)(H * W), out);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
