// Depth and silhouette rasteriser of the DMTet fitting loop: what nvdiffrec/lib/render/render.py:287-329 gets from
// dr.DepthPeeler + dr.interpolate (two depth-peeled layers of the clip-space mesh, the interpolated world position and its
// distance to the camera), with the gradient of both depth layers with respect to the vertices.
//
// THE RASTERISATION CONTRACT (shared by every layer and every test; tests/raster_cases.py restates it in torch)
//   Inputs     pos_clip float32 [B][V][4] = (x, y, z, w); faces int64 [F][3] shared by the views; resolution (H, W),
//              1 <= H, W <= 2048; F < 2^24; 1 <= B <= 64; anything else is MD_ERR_UNSUPPORTED.  The host checks the range of
//              the face indices once (meshdiffusion_amd/render.py); the kernels index unchecked.
//   Snap       X = rint(((x / w) * 0.5 + 0.5) * (256 W)), Y likewise with H, zw = z / w.  Every fp32 operation is rounded on
//              its own (correctly rounded divide, no contraction), so torch fp32 on the CPU reproduces X and Y exactly.  X and Y
//              are clamped to +-2^22.
//   Skipped    a triangle with a vertex of w <= 0 or a non-finite coordinate (there is no clipping), or with the integer
//              doubled area A2 = (X1-X0)(Y2-Y0) - (X2-X0)(Y1-Y0) == 0.  No back-face culling.
//   Coverage   exact integers.  Pixel (row i, column j) has the centre Q = (256 j + 128, 256 i + 128); row 0 is y = -1.  With
//              the triangle oriented so that A2 > 0, the edge a -> b, d = b - a, has e = d.x (Q.y - a.y) - d.y (Q.x - a.x).
//              Covered iff all three e >= 0, an edge with e == 0 counting only if d.y < 0 or (d.y == 0 and d.x > 0).  Of d and
//              -d exactly one passes, so two triangles sharing an edge never both own, and never both drop, a centre on it.
//   Depth      zf = sum_k (e_k / A2) zw_k in fp32, e_k the edge function opposite vertex k; a fragment with zf outside [-1, 1]
//              is dropped.
//   Layers     the fragments of a pixel are ordered by the key (zf, face index): layer 1 is the smallest, layer 2 the second
//              smallest.  Keys are unique, so the result does not depend on the order in which the triangles are visited.
//   rast       float32 [B][H][W][4] per layer: (u, v, zf, face index + 1), zeros where uncovered.  u, v are the perspective-
//              correct barycentrics from the UNSNAPPED clip floats: fx = (2j+1)/W - 1, fy = (2i+1)/H - 1,
//              p_k = (x_k - fx w_k, y_k - fy w_k), a0 = p1 x p2, a1 = p2 x p0, a2 = p0 x p1, u = a0 / (a0+a1+a2),
//              v = a1 / (a0+a1+a2), not clamped.  An attribute at the pixel is u A0 + v A1 + (1-u-v) A2.
//   Depth buffers  gb_pos = that interpolation of the world-space vertices, depth = |gb_pos - campos|; an uncovered pixel gets
//              20.0 in layer 1 and -1.0 in layer 2 (render.py:313,328); mask = 1.0 where covered.
//   Gradient   of both depth layers w.r.t. verts with the face ids held fixed, through BOTH the attribute path (weights u, v,
//              1-u-v) and the barycentric path (u, v <- pos_clip <- verts through mvp): what dr.rasterize + dr.interpolate
//              give.  mvp and campos get none.
//
// Kernels.  Binning: one thread per (view, face) snaps, tests and counts the 16x16-pixel tiles its bounding box touches; the
// host turns the counts into offsets (torch.cumsum), a second launch writes the (tile, face) pairs and a stable torch sort by
// tile gives the tile CSR.  Tile kernel: one 256-lane workgroup per (view, tile), one pixel per lane; the tile's triangles are
// set up again (one per lane) into 64-byte LDS records, 256 at a time, and every lane walks the chunk reading the same record
// (a broadcast).  Edge functions are int64 sums of 32 x 32 -> 64 bit products.  A lane keeps its two smallest 64-bit keys
//     key = sortable(zf) << 32 | face index
// and finally computes u, v of the two winners from the unsnapped floats and writes both layers with 16-byte stores.
// Backward: one thread per covered (pixel, layer) writes its three per-corner position gradients; one thread per vertex then
// GATHERS them, a plain fp32 sum, over a CSR of (covered entry, corner) codes sorted stably by vertex id (csrc/md_gather.h,
// md_csr_gather_kernel<3, false, false>): no floating-point atomics, two runs agree bit for bit.
#include "md_args.h"
#include "md_gather.h"
#include "md_raster_snap.h"

#pragma clang fp contract(off)

static constexpr int RS_TILE = 16;                           // pixels per tile side
static constexpr int RS_THREADS = RS_TILE * RS_TILE;         // one pixel per lane
static constexpr int RS_CHUNK = 256;                         // triangle records per LDS chunk (16 KiB)
static constexpr uint64_t RS_NO_KEY = ~0ull;

struct alignas(16) RsRecord {                                // one triangle, oriented so that A2 > 0; 64 bytes
  int32_t dx[3], dy[3];                                      // d of the edge OPPOSITE vertex k
  float zw[3];
  uint32_t id_flags;                                         // face index | (edge k owns e == 0) << (24 + k)
  int64_t c[3];                                              // e_k(Q) = dx[k] Q.y - dy[k] Q.x + c[k]
};
static_assert(sizeof(RsRecord) == 64, "RsRecord is read as four 16-byte LDS words");

struct RsTri {
  int X[3], Y[3];
  float zw[3];
  int64_t A2;
};

// false: the triangle is skipped
__device__ __forceinline__ bool rs_setup(const float* __restrict__ pc, const int64_t* __restrict__ faces, int64_t f, int H, int W,
                                         RsTri& t) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float4 v = *reinterpret_cast<const float4*>(pc + faces[f * 3 + k] * 4);
    ok = ok && rs_finite(v.x) && rs_finite(v.y) && rs_finite(v.z) && rs_finite(v.w) && v.w > 0.f;
    const float w = ok ? v.w : 1.f;
    t.X[k] = rs_snap(v.x, w, (float)(256 * W));
    t.Y[k] = rs_snap(v.y, w, (float)(256 * H));
    t.zw[k] = __fdiv_rn(v.z, w);
  }
  t.A2 = (int64_t)(t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (int64_t)(t.X[2] - t.X[0]) * (t.Y[1] - t.Y[0]);
  return ok && t.A2 != 0;
}

// the tiles whose pixel centres the bounding box can hold: [tx0, tx1] x [ty0, ty1], false when there is none
__device__ __forceinline__ bool rs_tile_box(const RsTri& t, int H, int W, int& tx0, int& tx1, int& ty0, int& ty1) {
  const int xmin = min(t.X[0], min(t.X[1], t.X[2])), xmax = max(t.X[0], max(t.X[1], t.X[2]));
  const int ymin = min(t.Y[0], min(t.Y[1], t.Y[2])), ymax = max(t.Y[0], max(t.Y[1], t.Y[2]));
  // centres 256 j + 128 in [xmin, xmax]: j from ceil((xmin - 128) / 256) to floor((xmax - 128) / 256) (>> floors)
  const int j0 = max((xmin - 128 + 255) >> 8, 0), j1 = min((xmax - 128) >> 8, W - 1);
  const int i0 = max((ymin - 128 + 255) >> 8, 0), i1 = min((ymax - 128) >> 8, H - 1);
  if (j0 > j1 || i0 > i1) return false;
  tx0 = j0 / RS_TILE; tx1 = j1 / RS_TILE; ty0 = i0 / RS_TILE; ty1 = i1 / RS_TILE;
  return true;
}

__global__ __launch_bounds__(256) void md_raster_bin_count_kernel(const float* __restrict__ pos_clip,
                                                                  const int64_t* __restrict__ faces, int V, int F, int H, int W,
                                                                  int32_t* __restrict__ counts) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int b = blockIdx.y;
  RsTri t;
  int n = 0, tx0, tx1, ty0, ty1;
  if (rs_setup(pos_clip + (int64_t)b * V * 4, faces, f, H, W, t) && rs_tile_box(t, H, W, tx0, tx1, ty0, ty1))
    n = (tx1 - tx0 + 1) * (ty1 - ty0 + 1);
  counts[(int64_t)b * F + f] = n;
}

__global__ __launch_bounds__(256) void md_raster_bin_emit_kernel(const float* __restrict__ pos_clip,
                                                                 const int64_t* __restrict__ faces,
                                                                 const int64_t* __restrict__ offsets, int V, int F, int H, int W,
                                                                 int64_t total, int32_t* __restrict__ pair_tile,
                                                                 int32_t* __restrict__ pair_face) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int b = blockIdx.y;
  RsTri t;
  int tx0, tx1, ty0, ty1;
  if (!rs_setup(pos_clip + (int64_t)b * V * 4, faces, f, H, W, t) || !rs_tile_box(t, H, W, tx0, tx1, ty0, ty1)) return;
  const int ntx = (W + RS_TILE - 1) / RS_TILE, nty = (H + RS_TILE - 1) / RS_TILE;
  int64_t o = offsets[(int64_t)b * F + f];
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx, ++o) {
      if (o < 0 || o >= total) return;                       // never with the offsets of md_raster_bin_count
      pair_tile[o] = (b * nty + ty) * ntx + tx;
      pair_face[o] = f;
    }
}

// zf in [-1, 1] -> a 32-bit word whose unsigned order is the numeric order (-0 was folded into +0 by the caller)
__device__ __forceinline__ uint32_t rs_sortable(float z) {
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rs_unsortable(uint32_t s) {
  return __uint_as_float((s & 0x80000000u) ? (s & 0x7fffffffu) : ~s);
}

// (u, v) of the contract at pixel (i, j) from the unsnapped clip floats of face f
__device__ __forceinline__ void rs_bary(const float* __restrict__ pc, const int64_t* __restrict__ faces, int64_t f, float fx, float fy,
                                        float& u, float& v) {
  float px[3], py[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float4 c = *reinterpret_cast<const float4*>(pc + faces[f * 3 + k] * 4);
    px[k] = c.x - fx * c.w;
    py[k] = c.y - fy * c.w;
  }
  const float a0 = px[1] * py[2] - py[1] * px[2];
  const float a1 = px[2] * py[0] - py[2] * px[0];
  const float a2 = px[0] * py[1] - py[0] * px[1];
  const float s = (a0 + a1) + a2;
  u = a0 / s;
  v = a1 / s;
}

__global__ __launch_bounds__(RS_THREADS) void md_raster_tiles_kernel(const float* __restrict__ pos_clip,
                                                                     const int64_t* __restrict__ faces,
                                                                     const int32_t* __restrict__ tile_ptr,
                                                                     const int32_t* __restrict__ tile_faces, int V, int H, int W,
                                                                     float* __restrict__ rast1, float* __restrict__ rast2) {
  __shared__ RsRecord s_rec[RS_CHUNK];
  const int ntx = (W + RS_TILE - 1) / RS_TILE, nty = (H + RS_TILE - 1) / RS_TILE;
  const int tile = blockIdx.x;
  const int b = tile / (ntx * nty);
  const int ty = (tile - b * ntx * nty) / ntx, tx = tile - (b * nty + ty) * ntx;
  const int tid = threadIdx.x;
  const int i = ty * RS_TILE + (tid >> 4), j = tx * RS_TILE + (tid & 15);
  const bool inside = i < H && j < W;
  const int32_t Qx = 256 * j + 128, Qy = 256 * i + 128;
  const float* pc = pos_clip + (int64_t)b * V * 4;

  uint64_t k1 = RS_NO_KEY, k2 = RS_NO_KEY;
  const int begin = tile_ptr[tile], end = tile_ptr[tile + 1];
  for (int c0 = begin; c0 < end; c0 += RS_CHUNK) {
    const int cnt = min(RS_CHUNK, end - c0);
    if (tid < cnt) {
      const int f = tile_faces[c0 + tid];
      RsTri t;
      RsRecord r;
      const bool ok = rs_setup(pc, faces, f, H, W, t);
      const int64_t s = t.A2 > 0 ? 1 : -1;
      uint32_t flags = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, bb = (k + 2) % 3;         // the edge opposite vertex k
        const int dx = (int)s * (t.X[bb] - t.X[a]), dy = (int)s * (t.Y[bb] - t.Y[a]);
        r.dx[k] = dx; r.dy[k] = dy;
        r.c[k] = (int64_t)dy * t.X[a] - (int64_t)dx * t.Y[a];
        r.zw[k] = t.zw[k];
        if (dy < 0 || (dy == 0 && dx > 0)) flags |= 1u << (24 + k);
      }
      if (!ok) {                                             // never listed by the binning; such a record covers nothing
#pragma unroll
        for (int k = 0; k < 3; ++k) { r.dx[k] = 0; r.dy[k] = 0; r.c[k] = -1; }
      }
      r.id_flags = (uint32_t)f | flags;
      s_rec[tid] = r;
    }
    __syncthreads();
    if (inside) {
      for (int n = 0; n < cnt; ++n) {
        const RsRecord& r = s_rec[n];
        int64_t e[3];
        bool cov = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          e[k] = (int64_t)r.dx[k] * Qy - (int64_t)r.dy[k] * Qx + r.c[k];
          cov = cov && (e[k] >= (((r.id_flags >> (24 + k)) & 1u) ? 0 : 1));
        }
        if (cov) {
          const float A2 = (float)((e[0] + e[1]) + e[2]);
          float zf = ((float)e[0] / A2) * r.zw[0] + ((float)e[1] / A2) * r.zw[1];
          zf = zf + ((float)e[2] / A2) * r.zw[2];
          if (zf >= -1.f && zf <= 1.f) {
            const uint64_t key = ((uint64_t)rs_sortable(zf + 0.f) << 32) | (r.id_flags & 0xffffffu);
            if (key < k1) { k2 = k1; k1 = key; }
            else if (key < k2) k2 = key;
          }
        }
      }
    }
    __syncthreads();
  }
  if (!inside) return;
  const float fx = (float)(2 * j + 1) / (float)W - 1.f, fy = (float)(2 * i + 1) / (float)H - 1.f;
  const int64_t o = (((int64_t)b * H + i) * W + j) * 4;
  float4 o1 = make_float4(0.f, 0.f, 0.f, 0.f), o2 = o1;
  if (k1 != RS_NO_KEY) {
    const int f = (int)(k1 & 0xffffffu);
    rs_bary(pc, faces, f, fx, fy, o1.x, o1.y);
    o1.z = rs_unsortable((uint32_t)(k1 >> 32));
    o1.w = (float)(f + 1);
  }
  if (k2 != RS_NO_KEY) {
    const int f = (int)(k2 & 0xffffffu);
    rs_bary(pc, faces, f, fx, fy, o2.x, o2.y);
    o2.z = rs_unsortable((uint32_t)(k2 >> 32));
    o2.w = (float)(f + 1);
  }
  *reinterpret_cast<float4*>(rast1 + o) = o1;
  *reinterpret_cast<float4*>(rast2 + o) = o2;
}

static bool rs_shape_ok(int32_t batch, int32_t n_verts, int32_t n_faces, int32_t H, int32_t W) {
  return rs_limits_ok(batch, n_faces, H, W) && n_verts > 0;
}

extern "C" int md_raster_bin_count(const float* pos_clip, const int64_t* faces, int32_t batch, int32_t n_verts, int32_t n_faces,
                                   int32_t H, int32_t W, int32_t* counts, void* stream) {
  if (md_any_bad<16>(pos_clip) || md_any_bad<8>(faces) || md_any_bad<1>(counts)) return MD_ERR_BAD_ARG;
  if (batch <= 0 || n_verts <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (!rs_shape_ok(batch, n_verts, n_faces, H, W)) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_raster_bin_count_kernel, dim3(md_blocks(n_faces, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, pos_clip, faces, (int)n_verts, (int)n_faces, (int)H, (int)W, counts);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_raster_bin_emit(const float* pos_clip, const int64_t* faces, const int64_t* offsets, int32_t batch,
                                  int32_t n_verts, int32_t n_faces, int32_t H, int32_t W, int64_t total, int32_t* pair_tile,
                                  int32_t* pair_face, void* stream) {
  if (md_any_bad<16>(pos_clip) || md_any_bad<8>(faces, offsets) || md_any_bad<1>(pair_tile, pair_face)) return MD_ERR_BAD_ARG;
  if (batch <= 0 || n_verts <= 0 || n_faces <= 0 || H <= 0 || W <= 0 || total <= 0) return MD_ERR_BAD_ARG;
  if (!rs_shape_ok(batch, n_verts, n_faces, H, W) || !md_fits_i32(total)) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_raster_bin_emit_kernel, dim3(md_blocks(n_faces, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, pos_clip, faces, offsets, (int)n_verts, (int)n_faces, (int)H, (int)W, total, pair_tile,
                     pair_face);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_raster_tiles(const float* pos_clip, const int64_t* faces, const int32_t* tile_ptr, const int32_t* tile_faces,
                               int32_t batch, int32_t n_verts, int32_t n_faces, int32_t H, int32_t W, float* rast1, float* rast2,
                               void* stream) {
  if (md_any_bad<16>(pos_clip, rast1, rast2) || md_any_bad<8>(faces) || md_any_bad<1>(tile_ptr, tile_faces)) return MD_ERR_BAD_ARG;
  if (batch <= 0 || n_verts <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (!rs_shape_ok(batch, n_verts, n_faces, H, W)) return MD_ERR_UNSUPPORTED;
  const int ntiles = ((W + RS_TILE - 1) / RS_TILE) * ((H + RS_TILE - 1) / RS_TILE);
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_raster_tiles_kernel, dim3((unsigned)(batch * ntiles)), dim3(RS_THREADS), 0, (hipStream_t)stream, pos_clip,
                     faces, tile_ptr, tile_faces, (int)n_verts, (int)H, (int)W, rast1, rast2);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

// ---- depth buffers ---------------------------------------------------------------------------------------------------------
// One thread per (view, layer, pixel): gb_pos = u P0 + v P1 + (1 - u - v) P2 of the WORLD vertices verts float32 [V][3] (shared
// by the views), depth = |gb_pos - campos[b]|, or the layer's background value; mask = 1 where covered.
__global__ __launch_bounds__(256) void md_raster_depth_kernel(const float* __restrict__ rast1, const float* __restrict__ rast2,
                                                              const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                              const float* __restrict__ campos, int HW, float* __restrict__ depth1,
                                                              float* __restrict__ depth2, float* __restrict__ mask1,
                                                              float* __restrict__ mask2) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int b = blockIdx.y, layer = blockIdx.z;
  const int64_t o = (int64_t)b * HW + p;
  const float4 r = *reinterpret_cast<const float4*>((layer ? rast2 : rast1) + o * 4);
  float d = layer ? -1.f : 20.f, m = 0.f;
  if (r.w > 0.f) {
    const int64_t f = (int64_t)r.w - 1;
    const float* P0 = verts + faces[f * 3] * 3;
    const float* P1 = verts + faces[f * 3 + 1] * 3;
    const float* P2 = verts + faces[f * 3 + 2] * 3;
    const float t = (1.f - r.x) - r.y;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float g = (r.x * P0[k] + r.y * P1[k]) + t * P2[k] - campos[b * 3 + k];
      s += g * g;
    }
    d = sqrtf(s);
    m = 1.f;
  }
  (layer ? depth2 : depth1)[o] = d;
  (layer ? mask2 : mask1)[o] = m;
}

extern "C" int md_raster_depth(const float* rast1, const float* rast2, const float* verts, const int64_t* faces,
                               const float* campos, int32_t batch, int32_t n_verts, int32_t n_faces, int32_t H, int32_t W,
                               float* depth1, float* depth2, float* mask1, float* mask2, void* stream) {
  if (md_any_bad<16>(rast1, rast2) || md_any_bad<8>(faces) || md_any_bad<1>(verts, campos, depth1, depth2, mask1, mask2))
    return MD_ERR_BAD_ARG;
  if (batch <= 0 || n_verts <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (!rs_shape_ok(batch, n_verts, n_faces, H, W)) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_raster_depth_kernel, dim3(md_blocks(H * W, 256), (unsigned)batch, 2u), dim3(256), 0,
                     (hipStream_t)stream, rast1, rast2, verts, faces, campos, (int)(H * W), depth1, depth2, mask1, mask2);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// Entry n of the covered list names cov[n] = (b * 2 + layer) * H W + pixel.  With g = d L / d depth at that entry:
//   d gb = g (gb - campos) / depth
//   attribute path:    d P0 += u d gb, d P1 += v d gb, d P2 += (1 - u - v) d gb
//   barycentric path:  du = d gb . (P0 - P2), dv = d gb . (P1 - P2); with S = a0 + a1 + a2,
//                      d a_j = (du (delta_0j - u) + dv (delta_1j - v)) / S; a0 = p1 x p2 etc. give d p_k;
//                      p_k = (x_k - fx w_k, y_k - fy w_k) gives d clip_k = (d p_k.x, d p_k.y, 0, -fx d p_k.x - fy d p_k.y);
//                      clip_k = mvp[b] (P_k, 1) gives d P_k += mvp[b]^T d clip_k.
// corner_grad float32 [N][3][3] receives d P_k of the entry.
__global__ __launch_bounds__(256) void md_raster_depth_bwd_pix_kernel(
    const int32_t* __restrict__ cov, int N, const float* __restrict__ rast1, const float* __restrict__ rast2,
    const float* __restrict__ gd1, const float* __restrict__ gd2, const float* __restrict__ pos_clip,
    const float* __restrict__ verts, const int64_t* __restrict__ faces, const float* __restrict__ mvp,
    const float* __restrict__ campos, int V, int H, int W, float* __restrict__ corner_grad) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int HW = H * W;
  const int code = cov[n];
  const int bl = code / HW, p = code - bl * HW;
  const int b = bl >> 1, layer = bl & 1;
  const int i = p / W, j = p - i * W;
  const int64_t o = (int64_t)b * HW + p;
  const float4 r = *reinterpret_cast<const float4*>((layer ? rast2 : rast1) + o * 4);
  const float g = (layer ? gd2 : gd1)[o];
  const int64_t f = (int64_t)r.w - 1;
  float out[3][3] = {};
  if (f >= 0) {
    const float u = r.x, v = r.y, t = (1.f - u) - v;
    const float* pc = pos_clip + (int64_t)b * V * 4;
    const float* M = mvp + b * 16;
    float P[3][3], px[3], py[3], wc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t vi = faces[f * 3 + k];
#pragma unroll
      for (int c = 0; c < 3; ++c) P[k][c] = verts[vi * 3 + c];
      const float4 c4 = *reinterpret_cast<const float4*>(pc + vi * 4);
      px[k] = c4.x; py[k] = c4.y; wc[k] = c4.w;
    }
    const float fx = (float)(2 * j + 1) / (float)W - 1.f, fy = (float)(2 * i + 1) / (float)H - 1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { px[k] = px[k] - fx * wc[k]; py[k] = py[k] - fy * wc[k]; }
    float D[3], dgb[3], s = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      D[c] = (u * P[0][c] + v * P[1][c]) + t * P[2][c] - campos[b * 3 + c];
      s += D[c] * D[c];
    }
    const float depth = sqrtf(s);
    const float gs = depth > 0.f ? g / depth : 0.f;
    float du = 0.f, dv = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      dgb[c] = gs * D[c];
      du += dgb[c] * (P[0][c] - P[2][c]);
      dv += dgb[c] * (P[1][c] - P[2][c]);
    }
    float dpx[3], dpy[3], dw[3];
    rs_bary_bwd(px, py, u, v, du, dv, fx, fy, dpx, dpy, dw);
    const float wk[3] = {u, v, t};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) out[k][c] = wk[k] * dgb[c] + ((M[c] * dpx[k] + M[4 + c] * dpy[k]) + M[12 + c] * dw[k]);
  }
  float* dst = corner_grad + (int64_t)n * 9;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[k * 3 + c] = out[k][c];
}

extern "C" int md_raster_depth_bwd(const int32_t* cov, int32_t n_cov, const float* rast1, const float* rast2, const float* gd1,
                                   const float* gd2, const float* pos_clip, const float* verts, const int64_t* faces,
                                   const float* mvp, const float* campos, const int32_t* ptr, const int32_t* order, int32_t batch,
                                   int32_t n_verts, int32_t n_faces, int32_t H, int32_t W, float* corner_grad, float* dverts,
                                   void* stream) {
  if (md_any_bad<1>(dverts, ptr) || batch <= 0 || n_verts <= 0 || n_faces <= 0 || H <= 0 || W <= 0 || n_cov < 0) return MD_ERR_BAD_ARG;
  if (n_cov > 0 && md_any_bad<1>(cov, rast1, rast2, gd1, gd2, pos_clip, verts, faces, mvp, campos, order, corner_grad))
    return MD_ERR_BAD_ARG;
  if (md_any_misaligned<16>(pos_clip, rast1, rast2) || md_any_misaligned<8>(faces)) return MD_ERR_BAD_ARG;
  if (!rs_shape_ok(batch, n_verts, n_faces, H, W) || !md_fits_i32((int64_t)n_cov * 3)) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  if (n_cov > 0)
    hipLaunchKernelGGL(md_raster_depth_bwd_pix_kernel, dim3(md_blocks(n_cov, 256)), dim3(256), 0, (hipStream_t)stream,
                       cov, (int)n_cov, rast1, rast2, gd1, gd2, pos_clip, verts, faces, mvp, campos, (int)n_verts, (int)H, (int)W,
                       corner_grad);
  md_csr_gather<3, false, false>(corner_grad, ptr, order, n_verts, (int64_t)n_cov * 3, dverts, (hipStream_t)stream);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
