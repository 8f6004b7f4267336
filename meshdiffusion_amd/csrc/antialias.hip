// Silhouette antialiasing of the DMTet fitting loop, in the manner of nvdiffrast's dr.antialias (nvdiffrec/lib/render/
// render.py:256-276), not equal to it: pixel pairs whose triangle ids differ, the nearer triangle's silhouette edges, linear
// blending by the edge's crossing point, with gradients for the colour and for the vertices.
//
// THE ANTIALIASING CONTRACT (tests/antialias_cases.py restates it in torch)
//   Inputs     color float32 [B][H][W][C], 1 <= C <= 8; rast float32 [B][H][W][4], one layer as the rasteriser writes it:
//              (u, v, zf, face + 1), zeros where uncovered; pos_clip float32 [B][V][4]; faces int64 [F][3]; nbr int32 [F][3].
//              The limits on B, H, W, F are those of the rasterisation contract (csrc/raster.hip); anything else is
//              MD_ERR_UNSUPPORTED.  A rast id outside [0, F] makes every pair it takes part in inactive; it is never an index.
//   Neighbours nbr[f][k] belongs to the edge opposite corner k of face f: the vertices faces[f][(k+1)%3], faces[f][(k+2)%3] as
//              an unordered pair.  If exactly two face corners of the mesh own that pair, nbr[f][k] is the other face's opposite
//              vertex, otherwise -1 (a boundary edge, or an edge of three or more faces).  nbr depends on faces only.
//   Pairs      every pixel forms a pair with its right neighbour and with the pixel below it, inside the image.  With the ids
//              t0, t1 and depths z0, z1 of the first and the second pixel the pair is a candidate iff t0 != t1.  The owning
//              pixel P is the second if t0 == 0, the first if t1 == 0, otherwise the first iff z0 < z1 (fp32 compare of the
//              stored values).  Q is the other pixel, T is P's triangle, s = +1 if Q follows P in the pair's direction, else -1.
//              A triangle T with a vertex of w <= 0 or a non-finite coordinate (never written by the rasteriser) has no edge.
//   Decisions  exact integers: the snapped X, Y of the rasterisation contract and P's centre (Px, Py) = (256 j + 128, 256 i +
//              128).  The edges of T are visited in the order k = 0, 1, 2 (edge a -> b opposite corner o, a = faces[T][(k+1)%3],
//              b = faces[T][(k+2)%3]); the first that passes all three tests is the pair's edge, and without one the pair is
//              inactive.
//                Silhouette   nbr < 0, or the neighbour vertex o' has w <= 0 or a non-finite coordinate, or
//                             sign(cross(b-a, o-a)) sign(cross(b-a, o'-a)) >= 0 (int64 cross products).
//                Orientation  |Yb-Ya| >= |Xb-Xa| for a horizontal pair, |Xb-Xa| >= |Yb-Ya| for a vertical one.
//                Crossing     with the along-pair coordinate u = s (X - Px) and the across coordinate v = Y - Py (X and Y swapped
//                             for a vertical pair): (va > 0) != (vb > 0), and with den = vb - va, n = ua den - va (ub - ua):
//                             0 <= n sign(den) <= 256 |den|.
//   Value      fp32, every operation rounded on its own (correctly rounded divide, no contraction).  From the unsnapped floats,
//              in pixels relative to P's centre: fu = s ((x / w - fx_P) W/2), fv = (y / w - fy_P) H/2 (roles swapped for a
//              vertical pair), fx, fy as in the rasterisation contract.  t = clamp(fu_a - fv_a (fu_b - fu_a) / (fv_b - fv_a),
//              0, 1); a zero denominator makes the pair inactive.  w = t - 0.5.  If w >= 0: out[Q] += w (color[P] - color[Q]),
//              otherwise out[P] += (-w) (color[Q] - color[P]).  A pixel's result is color + right pair + pair below + left pair
//              + pair above, summed in that order.
//   Gradient   color: the operator is linear in it.  pos_clip: through t, which uses x, y, w of the edge's two vertices (no z);
//              zero where the clamp is active.  rast, faces and nbr get none.
//
// Kernels.  md_mesh_edge_neighbours: the host sorts the keys min V + max of the 3 F corners stably; one thread per sorted entry
// looks at the run it sits in.  md_antialias_pairs: one thread per pixel analyses its right pair and the pair below and writes a
// 16-byte record per pair (va, vb, w, P is first); a pair with t0 == t1, which is almost every pair, writes the inactive record
// before any vertex is loaded.  md_antialias_blend / md_antialias_bwd_color: one thread per pixel gathers its four pairs.
// md_antialias_bwd_pos: one thread per active pair writes the (x, y, w) gradients of the edge's two vertices; one thread per
// (view, vertex) then GATHERS the codes 2 * entry + end, a plain fp32 sum, over a CSR sorted stably by b V + vertex
// (csrc/md_gather.h, md_csr_gather_kernel<3, false, true>).  No floating-point atomics anywhere: two runs agree bit for bit.
#include "md_args.h"
#include "md_gather.h"
#include "md_raster_snap.h"

#pragma clang fp contract(off)

static constexpr int AA_MAX_C = RS_MAX_CHANNELS;

struct alignas(16) AaPair {                                  // one pixel pair; va < 0: inactive
  int32_t va, vb;                                            // the edge's vertices
  float w;                                                   // t - 0.5: >= 0 Q receives, < 0 P receives
  int32_t p_first;                                           // P is the pair's first pixel
};
static_assert(sizeof(AaPair) == 16, "AaPair is read and written as one 16-byte word");

struct AaVertex {
  float4 c;
  int X, Y;
};

__device__ __forceinline__ bool aa_vertex(const float* __restrict__ pc, int64_t v, int H, int W, AaVertex& o) {
  o.c = *reinterpret_cast<const float4*>(pc + v * 4);
  if (!(rs_finite(o.c.x) && rs_finite(o.c.y) && rs_finite(o.c.z) && rs_finite(o.c.w) && o.c.w > 0.f)) return false;
  o.X = rs_snap(o.c.x, o.c.w, (float)(256 * W));
  o.Y = rs_snap(o.c.y, o.c.w, (float)(256 * H));
  return true;
}

__device__ __forceinline__ int aa_id(float w, int F) { return (w >= 0.f && w <= (float)F) ? (int)w : -1; }

// fu, fv of the contract for one vertex
__device__ __forceinline__ void aa_fuv(const float4& c, float fx, float fy, int H, int W, float s, bool vert, float& fu, float& fv) {
  const float px = (__fdiv_rn(c.x, c.w) - fx) * (0.5f * (float)W);
  const float py = (__fdiv_rn(c.y, c.w) - fy) * (0.5f * (float)H);
  fu = s * (vert ? py : px);
  fv = vert ? px : py;
}

// t before the clamp; false: zero denominator
__device__ __forceinline__ bool aa_t(const float4& ca, const float4& cb, int iP, int jP, int H, int W, float s, bool vert, float& fua,
                                     float& fva, float& fub, float& fvb, float& t) {
  const float fx = (float)(2 * jP + 1) / (float)W - 1.f, fy = (float)(2 * iP + 1) / (float)H - 1.f;
  aa_fuv(ca, fx, fy, H, W, s, vert, fua, fva);
  aa_fuv(cb, fx, fy, H, W, s, vert, fub, fvb);
  const float D = fvb - fva;
  if (D == 0.f) return false;
  t = fua - __fdiv_rn(fva * (fub - fua), D);
  return true;
}

__device__ __forceinline__ int aa_sign(int64_t x) { return (x > 0) - (x < 0); }

// the pair's edge: T's first edge that passes the silhouette, orientation and crossing tests
__device__ __forceinline__ AaPair aa_analyse(const float* __restrict__ pc, const int64_t* __restrict__ faces,
                                             const int32_t* __restrict__ nbr, int T, int iP, int jP, bool p_first, bool vert, int V,
                                             int H, int W) {
  AaPair out = {-1, -1, 0.f, 0};
  int64_t vid[3];
  AaVertex tv[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    vid[k] = faces[(int64_t)T * 3 + k];
    ok = aa_vertex(pc, vid[k], H, W, tv[k]) && ok;
  }
  if (!ok) return out;
  const int s = p_first ? 1 : -1;
  const int64_t Px = 256 * jP + 128, Py = 256 * iP + 128;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const int64_t dX = tv[b].X - tv[a].X, dY = tv[b].Y - tv[a].Y;
    const int64_t adX = dX < 0 ? -dX : dX, adY = dY < 0 ? -dY : dY;
    if (vert ? adX < adY : adY < adX) continue;              // orientation
    const int64_t ax = tv[a].X - Px, ay = tv[a].Y - Py, bx = tv[b].X - Px, by = tv[b].Y - Py;
    const int64_t ua = s * (vert ? ay : ax), wa = vert ? ax : ay, ub = s * (vert ? by : bx), wb = vert ? bx : by;
    if ((wa > 0) == (wb > 0)) continue;                      // crossing
    const int64_t den = wb - wa;
    const int64_t n = (ua * den - wa * (ub - ua)) * aa_sign(den);
    if (n < 0 || n > 256 * (den < 0 ? -den : den)) continue;
    const int32_t nb = nbr[(int64_t)T * 3 + k];              // silhouette
    if (nb >= 0 && nb < V) {                                 // the host checks nbr < V once
      AaVertex ov;
      if (aa_vertex(pc, nb, H, W, ov)) {
        const int64_t c1 = dX * (tv[k].Y - tv[a].Y) - dY * (tv[k].X - tv[a].X);
        const int64_t c2 = dX * (ov.Y - tv[a].Y) - dY * (ov.X - tv[a].X);
        if (aa_sign(c1) * aa_sign(c2) < 0) continue;
      }
    }
    float fua, fva, fub, fvb, t;
    if (!aa_t(tv[a].c, tv[b].c, iP, jP, H, W, (float)s, vert, fua, fva, fub, fvb, t)) return out;
    out.va = (int32_t)vid[a];
    out.vb = (int32_t)vid[b];
    out.w = fminf(fmaxf(t, 0.f), 1.f) - 0.5f;
    out.p_first = p_first ? 1 : 0;
    return out;
  }
  return out;
}

__global__ __launch_bounds__(256) void md_antialias_pairs_kernel(const float* __restrict__ rast, const float* __restrict__ pos_clip,
                                                                 const int64_t* __restrict__ faces, const int32_t* __restrict__ nbr,
                                                                 int V, int F, int H, int W, AaPair* __restrict__ pairs) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int b = blockIdx.y;
  const int i = p / W, j = p - i * W;
  const int64_t o = (int64_t)b * H * W + p;
  const float* pc = pos_clip + (int64_t)b * V * 4;
  const float2 r0 = *reinterpret_cast<const float2*>(rast + o * 4 + 2);       // (zf, id)
  const int t0 = aa_id(r0.y, F);
#pragma unroll 1
  for (int d = 0; d < 2; ++d) {                              // the right pair, the pair below
    AaPair rec = {-1, -1, 0.f, 0};
    const bool inside = d == 0 ? j + 1 < W : i + 1 < H;
    if (inside) {
      const float2 r1 = *reinterpret_cast<const float2*>(rast + (o + (d == 0 ? 1 : W)) * 4 + 2);
      const int t1 = aa_id(r1.y, F);
      if (t0 != t1 && t0 >= 0 && t1 >= 0) {
        const bool p_first = t0 == 0 ? false : (t1 == 0 ? true : r0.x < r1.x);
        const int T = (p_first ? t0 : t1) - 1;
        const int iP = i + ((d == 1 && !p_first) ? 1 : 0), jP = j + ((d == 0 && !p_first) ? 1 : 0);
        rec = aa_analyse(pc, faces, nbr, T, iP, jP, p_first, d == 1, V, H, W);
      }
    }
    pairs[o * 2 + d] = rec;
  }
}

// the four pairs of pixel (i, j) in the contract's order: for each, whether it is active and this pixel receives, |w| and the
// offset (in pixels) of the other pixel
struct AaGather {
  bool active[4], receive[4];
  float m[4];
  int other[4];
};

__device__ __forceinline__ AaGather aa_gather(const AaPair* __restrict__ pairs, int64_t o, int i, int j, int H, int W) {
  AaGather g;
  const int off[4] = {1, W, -1, -W};
  const bool inside[4] = {j + 1 < W, i + 1 < H, j > 0, i > 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    g.active[q] = false; g.receive[q] = false; g.m[q] = 0.f; g.other[q] = off[q];
    if (!inside[q]) continue;
    const bool first = q < 2;                                // this pixel is the pair's first pixel
    const AaPair r = pairs[(first ? o : o + off[q]) * 2 + (q & 1)];
    if (r.va < 0) continue;
    const bool recv_first = (r.p_first != 0) == (r.w < 0.f); // w >= 0: Q receives, w < 0: P receives
    g.active[q] = true;
    g.receive[q] = recv_first == first;
    g.m[q] = fabsf(r.w);
  }
  return g;
}

__global__ __launch_bounds__(256) void md_antialias_blend_kernel(const float* __restrict__ color, const AaPair* __restrict__ pairs,
                                                                 int H, int W, int C, float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int i = p / W, j = p - i * W;
  const int64_t o = (int64_t)blockIdx.y * H * W + p;
  const AaGather g = aa_gather(pairs, o, i, j, H, W);
  for (int c = 0; c < C; ++c) {
    const float self = color[o * C + c];
    float v = self;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (g.receive[q]) v = v + g.m[q] * (color[(o + g.other[q]) * C + c] - self);
    out[o * C + c] = v;
  }
}

// d color[x] = g[x] + sum over the pairs of x: -(|w| g[x]) where x receives, +|w| g[y] where the other pixel y receives
__global__ __launch_bounds__(256) void md_antialias_bwd_color_kernel(const float* __restrict__ gout, const AaPair* __restrict__ pairs,
                                                                     int H, int W, int C, float* __restrict__ dcolor) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int i = p / W, j = p - i * W;
  const int64_t o = (int64_t)blockIdx.y * H * W + p;
  const AaGather g = aa_gather(pairs, o, i, j, H, W);
  for (int c = 0; c < C; ++c) {
    const float self = gout[o * C + c];
    float v = self;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (g.active[q]) v = v + (g.receive[q] ? -(g.m[q] * self) : g.m[q] * gout[(o + g.other[q]) * C + c]);
    dcolor[o * C + c] = v;
  }
}

// Entry e of the active list names act[e] = ((b H + i) W + j) * 2 + direction.  With g = d L / d out at the receiving pixel:
//   d t = sum_c g_c (color[P]_c - color[Q]_c), zero where the clamp is active
//   t = fu_a - N / D, N = fv_a (fu_b - fu_a), D = fv_b - fv_a:
//     d fu_a = d t (1 + fv_a / D), d fu_b = -d t fv_a / D, d fv_a = -d t ((fu_b - fu_a) / D + N / D^2), d fv_b = d t N / D^2
//   fu, fv <- (x / w - fx) W/2, (y / w - fy) H/2: d x = d px (W/2) / w, d y = d py (H/2) / w, d w = -(d x x + d y y) / w.
// vert_grad float32 [N][2][3] receives (d x, d y, d w) of the edge's vertices a and b.
__global__ __launch_bounds__(256) void md_antialias_bwd_pair_kernel(const int64_t* __restrict__ act, int N,
                                                                    const float* __restrict__ color, const float* __restrict__ gout,
                                                                    const AaPair* __restrict__ pairs,
                                                                    const float* __restrict__ pos_clip, int V, int H, int W, int C,
                                                                    int64_t n_pairs, float* __restrict__ vert_grad) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  float out[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int64_t code = act[e];
  if (code >= 0 && code < n_pairs) {
    const AaPair r = pairs[code];
    const int d = (int)(code & 1);
    const int64_t o = code >> 1;                             // the pair's first pixel
    const int64_t b = o / ((int64_t)H * W);
    const int p = (int)(o - b * H * W);
    const int i = p / W, j = p - i * W;
    const bool inside = d == 0 ? j + 1 < W : i + 1 < H;
    if (inside && r.va >= 0 && r.va < V && r.vb >= 0 && r.vb < V) {
      const int64_t o2 = o + (d == 0 ? 1 : W);
      const bool p_first = r.p_first != 0;
      const int64_t oP = p_first ? o : o2, oQ = p_first ? o2 : o;
      const int iP = i + ((d == 1 && !p_first) ? 1 : 0), jP = j + ((d == 0 && !p_first) ? 1 : 0);
      const int64_t oR = r.w >= 0.f ? oQ : oP;
      float dt = 0.f;
      for (int c = 0; c < C; ++c) dt += gout[oR * C + c] * (color[oP * C + c] - color[oQ * C + c]);
      const float* pc = pos_clip + b * V * 4;
      const float4 ca = *reinterpret_cast<const float4*>(pc + (int64_t)r.va * 4);
      const float4 cb = *reinterpret_cast<const float4*>(pc + (int64_t)r.vb * 4);
      const float s = p_first ? 1.f : -1.f;
      const bool vert = d == 1;
      float fua, fva, fub, fvb, t;
      if (aa_t(ca, cb, iP, jP, H, W, s, vert, fua, fva, fub, fvb, t) && t >= 0.f && t <= 1.f) {
        const float D = fvb - fva, dfu = fub - fua;
        const float q = fva / D, n2 = (fva * dfu) / (D * D);
        const float g_fu[2] = {dt * (1.f + q), -dt * q};
        const float g_fv[2] = {-dt * (dfu / D + n2), dt * n2};
        const float4 cv[2] = {ca, cb};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float g_px = vert ? g_fv[k] : s * g_fu[k], g_py = vert ? s * g_fu[k] : g_fv[k];
          const float gx = g_px * (0.5f * (float)W) / cv[k].w, gy = g_py * (0.5f * (float)H) / cv[k].w;
          out[k * 3] = gx;
          out[k * 3 + 1] = gy;
          out[k * 3 + 2] = -(gx * cv[k].x + gy * cv[k].y) / cv[k].w;
        }
      }
    }
  }
  float* dst = vert_grad + (int64_t)e * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) dst[k] = out[k];
}

// sorted entry n of the 3 F corner keys: the run it sits in has exactly two entries -> the other corner's vertex
__global__ __launch_bounds__(256) void md_mesh_edge_neighbours_kernel(const int64_t* __restrict__ keys,
                                                                      const int64_t* __restrict__ order,
                                                                      const int64_t* __restrict__ faces, int64_t n,
                                                                      int32_t* __restrict__ nbr) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t k = keys[e];
  const bool prev = e > 0 && keys[e - 1] == k, next = e + 1 < n && keys[e + 1] == k;
  int64_t partner = -1;
  if (prev && !next && !(e > 1 && keys[e - 2] == k)) partner = e - 1;
  if (next && !prev && !(e + 2 < n && keys[e + 2] == k)) partner = e + 1;
  const int64_t corner = order[e];
  if (corner < 0 || corner >= n) return;                     // never with the order of a sort
  int32_t v = -1;
  if (partner >= 0) {
    const int64_t pc = order[partner];
    if (pc >= 0 && pc < n) v = (int32_t)faces[pc];           // corner f * 3 + k holds the vertex opposite edge k of face f
  }
  nbr[corner] = v;
}

static bool aa_shape_ok(int32_t batch, int32_t n_faces, int32_t H, int32_t W) {
  return rs_limits_ok(batch, n_faces, H, W);
}

extern "C" int md_mesh_edge_neighbours(const int64_t* sorted_keys, const int64_t* order, const int64_t* faces, int32_t n_faces,
                                       int32_t* nbr, void* stream) {
  if (md_any_bad<8>(sorted_keys, order, faces) || md_any_bad<4>(nbr) || n_faces <= 0) return MD_ERR_BAD_ARG;
  if (n_faces >= (1 << 24)) return MD_ERR_UNSUPPORTED;
  const int64_t n = (int64_t)n_faces * 3;
  MD_LAUNCH_1D(md_mesh_edge_neighbours_kernel, n, 256, sorted_keys, order, faces, n, nbr);
}

extern "C" int md_antialias_pairs(const float* rast, const float* pos_clip, const int64_t* faces, const int32_t* nbr,
                                  int32_t batch, int32_t n_verts, int32_t n_faces, int32_t H, int32_t W, int32_t* pairs,
                                  void* stream) {
  if (md_any_bad<16>(rast, pos_clip, pairs) || md_any_bad<8>(faces) || md_any_bad<4>(nbr)) return MD_ERR_BAD_ARG;
  if (batch <= 0 || n_verts <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (!aa_shape_ok(batch, n_faces, H, W)) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_antialias_pairs_kernel, dim3(md_blocks(H * W, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, rast, pos_clip, faces, nbr, (int)n_verts, (int)n_faces, (int)H, (int)W,
                     reinterpret_cast<AaPair*>(pairs));
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

static int aa_image_args(const void* a, const void* pairs, const void* out, int32_t batch, int32_t H, int32_t W, int32_t C) {
  if (md_any_bad<4>(a, out) || md_any_bad<16>(pairs) || batch <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (C < 1 || C > AA_MAX_C || !aa_shape_ok(batch, 0, H, W)) return MD_ERR_UNSUPPORTED;
  return MD_OK;
}

extern "C" int md_antialias_blend(const float* color, const int32_t* pairs, int32_t batch, int32_t H, int32_t W, int32_t C,
                                  float* out, void* stream) {
  const int rc = aa_image_args(color, pairs, out, batch, H, W, C);
  if (rc != MD_OK) return rc;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_antialias_blend_kernel, dim3(md_blocks(H * W, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, color, reinterpret_cast<const AaPair*>(pairs), (int)H, (int)W, (int)C, out);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_antialias_bwd_color(const float* grad_out, const int32_t* pairs, int32_t batch, int32_t H, int32_t W, int32_t C,
                                      float* dcolor, void* stream) {
  const int rc = aa_image_args(grad_out, pairs, dcolor, batch, H, W, C);
  if (rc != MD_OK) return rc;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_antialias_bwd_color_kernel, dim3(md_blocks(H * W, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, grad_out, reinterpret_cast<const AaPair*>(pairs), (int)H, (int)W, (int)C, dcolor);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_antialias_bwd_pos(const int64_t* active, int32_t n_active, const float* color, const float* grad_out,
                                    const int32_t* pairs, const float* pos_clip, const int32_t* ptr, const int32_t* order,
                                    int32_t batch, int32_t n_verts, int32_t H, int32_t W, int32_t C, float* vert_grad,
                                    float* dpos_clip, void* stream) {
  if (md_any_bad<16>(dpos_clip) || md_any_bad<1>(ptr) || batch <= 0 || n_verts <= 0 || H <= 0 || W <= 0 || n_active < 0)
    return MD_ERR_BAD_ARG;
  if (n_active > 0 && md_any_bad<1>(active, color, grad_out, pairs, pos_clip, order, vert_grad)) return MD_ERR_BAD_ARG;
  if (md_any_misaligned<16>(pos_clip, pairs) || md_any_misaligned<8>(active)) return MD_ERR_BAD_ARG;
  const int64_t BV = (int64_t)batch * n_verts;
  if (C < 1 || C > AA_MAX_C || !aa_shape_ok(batch, 0, H, W) || !md_fits_i32(BV + 1, (int64_t)n_active * 2)) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  if (n_active > 0)
    hipLaunchKernelGGL(md_antialias_bwd_pair_kernel, dim3(md_blocks(n_active, 256)), dim3(256), 0, (hipStream_t)stream,
                       active, (int)n_active, color, grad_out, reinterpret_cast<const AaPair*>(pairs), pos_clip, (int)n_verts,
                       (int)H, (int)W, (int)C, (int64_t)batch * H * W * 2, vert_grad);
  md_csr_gather<3, false, true>(vert_grad, ptr, order, BV, (int64_t)n_active * 2, dpos_clip, (hipStream_t)stream);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
