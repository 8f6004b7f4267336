// Attribute interpolation, the gradient of the barycentrics and differentiable vertex normals of the DMTet fitting loop: what
// nvdiffrec/lib/render/render.py:20,177-210 gets from dr.interpolate, the `rast` gradient of dr.rasterize and
// nvdiffrec/lib/render/mesh.py:200-229 (auto_normals under autograd).
//
// THE INTERPOLATION CONTRACT (tests/interp_cases.py restates it in torch)
//   Inputs     rast float32 [B][H][W][4], one layer as the rasteriser writes it: (u, v, zf, face + 1), zeros where uncovered;
//              attr float32 [Ba][N][C], Ba = 1 (shared by the views) or B, 1 <= C <= 8; tri int64 [F][3] with indices into N.  It
//              need not be the position index: a face-constant attribute uses tri[f] = (f, f, f) with N = F.  The limits on B, H,
//              W, F are those of the rasterisation contract (csrc/raster.hip); anything else is MD_ERR_UNSUPPORTED.  The host
//              checks the range of tri once (meshdiffusion_amd/render.py); the kernels index unchecked.
//   Value      fp32, every operation rounded on its own (no contraction).  A pixel with id = rast.w, 1 <= id <= F:
//              out[c] = (u A0[c] + v A1[c]) + t A2[c], t = (1 - u) - v, (u, v) = rast.xy, A_k = attr[tri[id-1][k]]: the operation
//              order of md_raster_depth.  Every other pixel: all C channels 0.  An id above F is never an index.
//   d attr     corner k of a covered pixel contributes w_k g, weights (u, v, t), to attr[tri[id-1][k]].  Summed per destination
//              row in ascending order of the code 3 * entry + corner, entry = the rank of the pixel among the covered pixels in
//              flat (b, i, j) order; with Ba == 1 the sum runs over all views.
//   Sums       every sum over codes in this contract (d attr, d pos_clip, s_v, d verts) is a compensated (Kahan) fp32 sum in
//              ascending code order: sum = 0, lost = 0; per term x: y = x - lost, t = sum + y, lost = (t - sum) - y, sum = t,
//              every operation rounded on its own.  A row's accuracy then does not depend on how many codes it has.
//   d rast     du = sum_c g[c] (A0[c] - A2[c]), dv = sum_c g[c] (A1[c] - A2[c]) in channels 0 and 1 of a float32 [B][H][W][4]
//              tensor; channels 2 and 3 and uncovered pixels are zero.
//   Barycentric backward   from d rast (du, dv in channels 0 and 1) to d pos_clip [B][V][4].  Per covered pixel, with p_k, a_j
//              of the rasterisation contract and S = a0 + a1 + a2:
//                d a_j = (du (delta_0j - u) + dv (delta_1j - v)) / S; a0 = p1 x p2 etc. give d p_k;
//                d clip_k = (d p_k.x, d p_k.y, 0, -fx d p_k.x - fy d p_k.y)
//              (the formulas above md_raster_depth_bwd_pix_kernel), summed per (view, vertex) in ascending code order.  z gets no
//              gradient and zf is not differentiated.
//   Vertex normals   fn_f = cross(v1 - v0, v2 - v0); s_v = the sum of fn_f over the corners that name v in ascending order of the
//              code 3 f + k; s_v is replaced by (0, 0, 1) when s_v . s_v <= 1e-20 (a vertex no face names included);
//              n_v = s_v / sqrt(max(s_v . s_v, 1e-20)).  v_len holds sqrt(max(s_v . s_v, 1e-20)), or 0 for a replaced vertex.
//              Backward: d s_v = (g - n (n . g)) / |s_v|, zero for a replaced vertex; d fn_f = the sum of d s over the face's
//              corners k = 0, 1, 2; with a = v1 - v0, b = v2 - v0: d a = b x d fn, d b = d fn x a, d v0 = -d a - d b.
//
// Kernels.  Every reduction is a GATHER in a fixed order over a CSR of codes sorted stably by destination (csrc/md_gather.h):
// one thread per covered entry (or face) writes its per-corner gradients, one thread per destination row then sums them,
// compensated (md_kahan_add), in that order: md_csr_gather_kernel<W, true, .>.  No floating-point atomics anywhere: two runs
// agree bit for bit.  md_interpolate: one thread per pixel, one 16-byte rast load, C unrolled at compile time.
#include "md_args.h"
#include "md_gather.h"
#include "md_raster_snap.h"

#pragma clang fp contract(off)

// face index of a rast id, -1 unless 1 <= id <= F
__device__ __forceinline__ int64_t ip_face(float id, int F) { return (id >= 1.f && id <= (float)F) ? (int64_t)id - 1 : -1; }

template <int C>
__global__ __launch_bounds__(256) void md_interpolate_kernel(const float* __restrict__ rast, const float* __restrict__ attr,
                                                             const int64_t* __restrict__ tri, int64_t attr_bstride, int F, int HW,
                                                             float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * HW + p;
  const float4 r = *reinterpret_cast<const float4*>(rast + o * 4);
  float val[C];
#pragma unroll
  for (int c = 0; c < C; ++c) val[c] = 0.f;
  const int64_t f = ip_face(r.w, F);
  if (f >= 0) {
    const float* A = attr + (int64_t)b * attr_bstride;
    const float* A0 = A + tri[f * 3] * C;
    const float* A1 = A + tri[f * 3 + 1] * C;
    const float* A2 = A + tri[f * 3 + 2] * C;
    const float t = (1.f - r.x) - r.y;
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = (r.x * A0[c] + r.y * A1[c]) + t * A2[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[o * C + c] = val[c];
}

// Entry n names the covered pixel cov[n] = b H W + pixel.  corner_grad float32 [N][3][C] receives w_k g (when the attribute
// gradient is wanted), drast (when wanted; zeroed before) receives (du, dv, 0, 0) at the pixel.
template <int C>
__global__ __launch_bounds__(256) void md_interpolate_bwd_pix_kernel(const int32_t* __restrict__ cov, int N,
                                                                     const float* __restrict__ rast, const float* __restrict__ gout,
                                                                     const float* __restrict__ attr, const int64_t* __restrict__ tri,
                                                                     int64_t attr_bstride, int F, int HW, int64_t n_pix,
                                                                     float* __restrict__ corner_grad, float* __restrict__ drast) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int64_t o = cov[n];
  float w[3] = {0.f, 0.f, 0.f}, g[C], du = 0.f, dv = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = 0.f;
  const bool in_image = o >= 0 && o < n_pix;                 // always with the list of the host
  if (in_image) {
    const float4 r = *reinterpret_cast<const float4*>(rast + o * 4);
    const int64_t f = ip_face(r.w, F);
    if (f >= 0) {
      w[0] = r.x; w[1] = r.y; w[2] = (1.f - r.x) - r.y;
#pragma unroll
      for (int c = 0; c < C; ++c) g[c] = gout[o * C + c];
      if (drast) {
        const float* A = attr + (o / HW) * attr_bstride;
        const float* A0 = A + tri[f * 3] * C;
        const float* A1 = A + tri[f * 3 + 1] * C;
        const float* A2 = A + tri[f * 3 + 2] * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          du += g[c] * (A0[c] - A2[c]);
          dv += g[c] * (A1[c] - A2[c]);
        }
      }
    }
    if (drast) *reinterpret_cast<float4*>(drast + o * 4) = make_float4(du, dv, 0.f, 0.f);
  }
  if (corner_grad) {
    float* dst = corner_grad + (int64_t)n * 3 * C;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < C; ++c) dst[k * C + c] = w[k] * g[c];
  }
}

// Entry n names the covered pixel cov[n] = b H W + pixel; corner_grad float32 [N][3][3] receives (d x, d y, d w) of the three
// corners: rs_bary_bwd (csrc/md_raster_snap.h), the barycentric path of md_raster_depth_bwd_pix_kernel, fed (du, dv) from drast.
__global__ __launch_bounds__(256) void md_raster_bary_bwd_pix_kernel(const int32_t* __restrict__ cov, int N,
                                                                     const float* __restrict__ rast, const float* __restrict__ drast,
                                                                     const float* __restrict__ pos_clip,
                                                                     const int64_t* __restrict__ faces, int V, int F, int H, int W,
                                                                     int64_t n_pix, float* __restrict__ corner_grad) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float out[3][3] = {};
  const int64_t o = cov[n];
  if (o >= 0 && o < n_pix) {
    const int HW = H * W;
    const int64_t b = o / HW;
    const int p = (int)(o - b * HW);
    const int i = p / W, j = p - i * W;
    const float4 r = *reinterpret_cast<const float4*>(rast + o * 4);
    const float4 gr = *reinterpret_cast<const float4*>(drast + o * 4);
    const int64_t f = ip_face(r.w, F);
    if (f >= 0) {
      const float u = r.x, v = r.y, du = gr.x, dv = gr.y;
      const float* pc = pos_clip + b * V * 4;
      float px[3], py[3], wc[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float4 c4 = *reinterpret_cast<const float4*>(pc + faces[f * 3 + k] * 4);
        px[k] = c4.x; py[k] = c4.y; wc[k] = c4.w;
      }
      const float fx = (float)(2 * j + 1) / (float)W - 1.f, fy = (float)(2 * i + 1) / (float)H - 1.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) { px[k] = px[k] - fx * wc[k]; py[k] = py[k] - fy * wc[k]; }
      float dpx[3], dpy[3], dw[3];
      rs_bary_bwd(px, py, u, v, du, dv, fx, fy, dpx, dpy, dw);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        out[k][0] = dpx[k];
        out[k][1] = dpy[k];
        out[k][2] = dw[k];
      }
    }
  }
  float* dst = corner_grad + (int64_t)n * 9;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[k * 3 + c] = out[k][c];
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void md_face_normals_det_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                                  int F, float* __restrict__ f_nrm) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const float* v0 = verts + faces[(int64_t)f * 3] * 3;
  const float* v1 = verts + faces[(int64_t)f * 3 + 1] * 3;
  const float* v2 = verts + faces[(int64_t)f * 3 + 2] * 3;
  const float a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
  const float b[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
  f_nrm[(int64_t)f * 3] = a[1] * b[2] - a[2] * b[1];
  f_nrm[(int64_t)f * 3 + 1] = a[2] * b[0] - a[0] * b[2];
  f_nrm[(int64_t)f * 3 + 2] = a[0] * b[1] - a[1] * b[0];
}

// (ptr int32 [V + 1], order int32 [3 F]): the CSR of the corner codes 3 f + k sorted stably by vertex
__global__ __launch_bounds__(256) void md_vertex_normals_gather_kernel(const float* __restrict__ f_nrm,
                                                                       const int32_t* __restrict__ ptr,
                                                                       const int32_t* __restrict__ order, int V, int64_t n_codes,
                                                                       float* __restrict__ v_nrm, float* __restrict__ v_len) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, l0 = 0.f, l1 = 0.f, l2 = 0.f;
  const int j1 = ptr[v + 1];
  for (int j = ptr[v]; j < j1; ++j) {
    if (j < 0 || j >= n_codes) break;                        // never with the CSR of the host
    const int32_t code = order[j];
    if (code < 0 || code >= n_codes) continue;
    const float* fn = f_nrm + (int64_t)(code / 3) * 3;
    md_kahan_add(s0, l0, fn[0]); md_kahan_add(s1, l1, fn[1]); md_kahan_add(s2, l2, fn[2]);
  }
  const float d = (s0 * s0 + s1 * s1) + s2 * s2;
  float len = 0.f, n0 = 0.f, n1 = 0.f, n2 = 1.f;
  if (d > 1e-20f) {
    len = sqrtf(fmaxf(d, 1e-20f));
    n0 = s0 / len; n1 = s1 / len; n2 = s2 / len;
  }
  v_nrm[(int64_t)v * 3] = n0; v_nrm[(int64_t)v * 3 + 1] = n1; v_nrm[(int64_t)v * 3 + 2] = n2;
  v_len[v] = len;
}

// face_grad float32 [F][3][3] receives (d v0, d v1, d v2) of the face
__global__ __launch_bounds__(256) void md_vertex_normals_bwd_face_kernel(const float* __restrict__ verts,
                                                                         const int64_t* __restrict__ faces,
                                                                         const float* __restrict__ v_nrm,
                                                                         const float* __restrict__ v_len, const float* __restrict__ g,
                                                                         int F, float* __restrict__ face_grad) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int64_t vi[3];
  float dfn[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    vi[k] = faces[(int64_t)f * 3 + k];
    const float len = v_len[vi[k]];
    if (len > 0.f) {
      const float* n = v_nrm + vi[k] * 3;
      const float* gv = g + vi[k] * 3;
      const float ng = (n[0] * gv[0] + n[1] * gv[1]) + n[2] * gv[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) dfn[c] += (gv[c] - n[c] * ng) / len;
    }
  }
  const float* v0 = verts + vi[0] * 3;
  const float* v1 = verts + vi[1] * 3;
  const float* v2 = verts + vi[2] * 3;
  const float a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
  const float b[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
  const float da[3] = {b[1] * dfn[2] - b[2] * dfn[1], b[2] * dfn[0] - b[0] * dfn[2], b[0] * dfn[1] - b[1] * dfn[0]};
  const float db[3] = {dfn[1] * a[2] - dfn[2] * a[1], dfn[2] * a[0] - dfn[0] * a[2], dfn[0] * a[1] - dfn[1] * a[0]};
  float* dst = face_grad + (int64_t)f * 9;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dst[c] = -da[c] - db[c];
    dst[3 + c] = da[c];
    dst[6 + c] = db[c];
  }
}

// ---- exports -------------------------------------------------------------------------------------------------------------------
#define IP_DISPATCH_C(C, CALL) \
  switch (C) {                 \
    case 1: { constexpr int K = 1; CALL; } break; \
    case 2: { constexpr int K = 2; CALL; } break; \
    case 3: { constexpr int K = 3; CALL; } break; \
    case 4: { constexpr int K = 4; CALL; } break; \
    case 5: { constexpr int K = 5; CALL; } break; \
    case 6: { constexpr int K = 6; CALL; } break; \
    case 7: { constexpr int K = 7; CALL; } break; \
    default: { constexpr int K = 8; CALL; } break; \
  }

static int ip_attr_args(int32_t batch, int32_t attr_batch, int32_t n_rows, int32_t C, int32_t n_faces, int32_t H, int32_t W) {
  if (batch <= 0 || attr_batch <= 0 || n_rows <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (attr_batch != 1 && attr_batch != batch) return MD_ERR_BAD_ARG;
  if (C < 1 || C > RS_MAX_CHANNELS || !rs_limits_ok(batch, n_faces, H, W)) return MD_ERR_UNSUPPORTED;
  return MD_OK;
}

extern "C" int md_interpolate(const float* rast, const float* attr, const int64_t* tri, int32_t batch, int32_t attr_batch,
                              int32_t n_rows, int32_t C, int32_t n_faces, int32_t H, int32_t W, float* out, void* stream) {
  if (md_any_bad<16>(rast) || md_any_bad<8>(tri) || md_any_bad<4>(attr, out)) return MD_ERR_BAD_ARG;
  const int rc = ip_attr_args(batch, attr_batch, n_rows, C, n_faces, H, W);
  if (rc != MD_OK) return rc;
  const int64_t bstride = attr_batch == 1 ? 0 : (int64_t)n_rows * C;
  MD_HIP_CLEAR_ERROR();
  IP_DISPATCH_C(C, hipLaunchKernelGGL(md_interpolate_kernel<K>, dim3(md_blocks(H * W, 256), (unsigned)batch), dim3(256), 0,
                                      (hipStream_t)stream, rast, attr, tri, bstride, (int)n_faces, (int)(H * W), out));
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_interpolate_bwd(const int32_t* cov, int32_t n_cov, const float* rast, const float* grad_out, const float* attr,
                                  const int64_t* tri, const int32_t* ptr, const int32_t* order, int32_t batch, int32_t attr_batch,
                                  int32_t n_rows, int32_t C, int32_t n_faces, int32_t H, int32_t W, float* corner_grad, float* dattr,
                                  float* drast, void* stream) {
  if (n_cov < 0 || (!dattr && !drast)) return MD_ERR_BAD_ARG;
  if (dattr && !ptr) return MD_ERR_BAD_ARG;
  if (n_cov > 0 && (!cov || !rast || !grad_out || !attr || !tri || (dattr && (!order || !corner_grad)))) return MD_ERR_BAD_ARG;
  if (md_any_misaligned<16>(rast, drast) || md_any_misaligned<8>(tri) || md_any_misaligned<4>(cov, ptr, order)) return MD_ERR_BAD_ARG;
  const int rc = ip_attr_args(batch, attr_batch, n_rows, C, n_faces, H, W);
  if (rc != MD_OK) return rc;
  const int64_t rows = (int64_t)attr_batch * n_rows, n_pix = (int64_t)batch * H * W;
  if (!md_fits_i32((int64_t)n_cov * 3, rows + 1)) return MD_ERR_UNSUPPORTED;
  const int64_t bstride = attr_batch == 1 ? 0 : (int64_t)n_rows * C;
  if (drast) {
    hipError_t e = hipMemsetAsync(drast, 0, (size_t)n_pix * 4 * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  MD_HIP_CLEAR_ERROR();
  if (n_cov > 0)
    IP_DISPATCH_C(C, hipLaunchKernelGGL(md_interpolate_bwd_pix_kernel<K>, dim3(md_blocks(n_cov, 256)), dim3(256), 0,
                                        (hipStream_t)stream, cov, (int)n_cov, rast, grad_out, attr, tri, bstride, (int)n_faces,
                                        (int)(H * W), n_pix, dattr ? corner_grad : (float*)nullptr, drast));
  if (dattr)
    IP_DISPATCH_C(C, (md_csr_gather<K, true, false>(corner_grad, ptr, order, rows, (int64_t)n_cov * 3, dattr, (hipStream_t)stream)));
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_raster_bary_bwd(const int32_t* cov, int32_t n_cov, const float* rast, const float* drast, const float* pos_clip,
                                  const int64_t* faces, const int32_t* ptr, const int32_t* order, int32_t batch, int32_t n_verts,
                                  int32_t n_faces, int32_t H, int32_t W, float* corner_grad, float* dpos_clip, void* stream) {
  if (md_any_bad<16>(dpos_clip) || md_any_bad<4>(ptr)) return MD_ERR_BAD_ARG;
  if (batch <= 0 || n_verts <= 0 || n_faces <= 0 || H <= 0 || W <= 0 || n_cov < 0) return MD_ERR_BAD_ARG;
  if (n_cov > 0 && md_any_bad<1>(cov, rast, drast, pos_clip, faces, order, corner_grad)) return MD_ERR_BAD_ARG;
  if (md_any_misaligned<16>(rast, drast, pos_clip) || md_any_misaligned<8>(faces) || md_any_misaligned<4>(cov, order))
    return MD_ERR_BAD_ARG;
  const int64_t BV = (int64_t)batch * n_verts;
  if (!rs_limits_ok(batch, n_faces, H, W) || !md_fits_i32((int64_t)n_cov * 3, BV + 1)) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  if (n_cov > 0)
    hipLaunchKernelGGL(md_raster_bary_bwd_pix_kernel, dim3(md_blocks(n_cov, 256)), dim3(256), 0, (hipStream_t)stream, cov,
                       (int)n_cov, rast, drast, pos_clip, faces, (int)n_verts, (int)n_faces, (int)H, (int)W,
                       (int64_t)batch * H * W, corner_grad);
  md_csr_gather<3, true, true>(corner_grad, ptr, order, BV, (int64_t)n_cov * 3, dpos_clip, (hipStream_t)stream);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_vertex_normals_det(const float* verts, const int64_t* faces, const int32_t* ptr, const int32_t* order,
                                     int32_t n_verts, int32_t n_faces, float* v_nrm, float* f_nrm, float* v_len, void* stream) {
  if (md_any_bad<1>(verts, v_nrm, f_nrm, v_len) || md_any_bad<8>(faces) || md_any_bad<4>(ptr, order)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_faces <= 0) return MD_ERR_BAD_ARG;
  if (n_faces >= RS_MAX_FACES) return MD_ERR_UNSUPPORTED;                 // 3 F corner codes fit int32
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_face_normals_det_kernel, dim3(md_blocks(n_faces, 256)), dim3(256), 0, (hipStream_t)stream, verts,
                     faces, (int)n_faces, f_nrm);
  hipLaunchKernelGGL(md_vertex_normals_gather_kernel, dim3(md_blocks(n_verts, 256)), dim3(256), 0, (hipStream_t)stream,
                     f_nrm, ptr, order, (int)n_verts, (int64_t)n_faces * 3, v_nrm, v_len);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_vertex_normals_bwd(const float* verts, const int64_t* faces, const int32_t* ptr, const int32_t* order,
                                     const float* v_nrm, const float* v_len, const float* grad_v_nrm, int32_t n_verts,
                                     int32_t n_faces, float* face_grad, float* dverts, void* stream) {
  if (md_any_bad<1>(verts, v_nrm, v_len, grad_v_nrm, face_grad, dverts) || md_any_bad<8>(faces) || md_any_bad<4>(ptr, order))
    return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_faces <= 0) return MD_ERR_BAD_ARG;
  if (n_faces >= RS_MAX_FACES) return MD_ERR_UNSUPPORTED;                 // 3 F corner codes fit int32
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_vertex_normals_bwd_face_kernel, dim3(md_blocks(n_faces, 256)), dim3(256), 0, (hipStream_t)stream,
                     verts, faces, v_nrm, v_len, grad_v_nrm, (int)n_faces, face_grad);
  md_csr_gather<3, true, false>(face_grad, ptr, order, n_verts, (int64_t)n_faces * 3, dverts, (hipStream_t)stream);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
