// Visible-tet labelling of the single-view fit: what nvdiffrec/lib/render/render.py:346-407 (`get_visible_tets=True`) and
// nvdiffrec/fit_singleview.py:795-820 compute from the first rasterised layer of one view -- which tetrahedra of the grid the
// camera sees (their centres lie in front of the nearest surface around their pixel), which own a rasterised face, and which
// grid vertices those tetrahedra name: the `vis` / `vis_rast` arrays of the dict that conditional generation reads.
//
// THE VISIBILITY CONTRACT (tests/visibility_cases.py restates it in torch)
//   Inputs     rast float32 [B][H][W][4] (16-byte aligned): layer 1 of the rasterisation contract (csrc/raster.hip), (u, v, zf,
//              face index + 1); zf is finite and in [-1, 1] where the id is not 0.  centres float32 [T][3], the tet centres in
//              world space (computed by torch, not here); mvp float32 [B][4][4] row-major; radius r, 0 <= r <= 15 (the
//              reference's depth_search_range = 7).  1 <= H, W <= 2048, 1 <= B <= 64; anything else is MD_ERR_UNSUPPORTED.
//   Depth      D[b][i][j] = zf where rast[b][i][j][3] != 0, else 100.0.
//   Window     Dmin[b][i][j] = min of D[b][i'][j'] over |i' - i| <= r, |j' - j| <= r INSIDE the image: the reference's
//              -max_pool2d(-D, 2 r + 1, stride 1, padding r), whose padding is -inf and never wins.
//   Centre     c = mvp (p, 1), c_k = ((p.x m[k][0] + p.y m[k][1]) + p.z m[k][2]) + m[k][3] (render.xfm_points);
//              n = (c.x / c.w, c.y / c.w, c.z / c.w); q_k = rint((n_k / 2 + 0.5) * S_k) with S = (W - 1, H - 1, H - 1) for
//              (x, y, z).  Every fp32 operation is rounded on its own (correctly rounded divide, no contraction, rint = ties to
//              even), so torch fp32 on the CPU reproduces every decision exactly.  The reference asserts a square image and
//              scales all three with full_res[0] - 1; its test on q_z is kept as it is.
//   Valid      all three q_k lie in [0, S_k], compared in float before any conversion to an integer; NaN is not valid.
//   Visible    visible[b][t] = valid && (Dmin[b][q_y][q_x] >= n.z || Dmin[b][q_y][q_x] == 100): the depth test or the emptiness
//              test of the reference (row q_y, column q_x: its "transpose").  For a valid centre n.z <= 1 < 100, so the
//              emptiness test is implied by the depth test and one image serves both.
//   Deviation  a centre with c.w <= 0 or a non-finite clip coordinate is NOT visible.  The reference projects it through the
//              camera (a point behind the eye lands on a pixel, mirrored).
//   Labels     rast_tet[t] = 1 iff a pixel of layer 1 of any view has 1 <= id <= F and face_tet[id - 1] == t;
//              vis[v] = 1.0 iff a tet with visible[b][t] in any view names v; vis_rast[v] = 1 iff a tet with
//              visible[b][t] (any view) or rast_tet[t] names v.  The host zeroes the three arrays.  A face id above F, a tet
//              index outside [0, T) and a vertex index outside [0, N) are skipped, never read or written.
//   Determinism  every store of a label writes the same value (1) wherever it lands: plain vector stores, no atomics, and two
//              runs agree bit for bit.
//
// Kernels.  md_window_min: one 256-lane workgroup per (view, 32 x 32 output tile).  The tile and its r-pixel apron of D are staged
// in LDS ((32 + 2 r)^2 floats, at most 15 KiB; +inf outside the image); a row-minimum pass writes (32 + 2 r) x 32 floats (at most
// 8 KiB more), a column-minimum pass reads them: about 2 (2 r + 1) LDS reads per pixel instead of (2 r + 1)^2.  In both passes a wave reads 32
// consecutive floats per row (no bank conflict) and the stores are 128-byte rows.  md_tet_visibility: one lane per (view, tet):
// twelve multiply-adds, three divides, one gather from Dmin.  md_rast_mark_tets: one lane per pixel.  md_tets_mark_verts: one
// lane per tet, up to eight stores.  All three are latency-bound gathers and scatters with nothing to reuse: no LDS.
#include "md_args.h"

#pragma clang fp contract(off)

static constexpr int VS_THREADS = 256;
static constexpr int VS_TILE = 32;                            // output pixels per tile side
static constexpr int VS_MAX_RADIUS = 15;
static constexpr int VS_SPAN = VS_TILE + 2 * VS_MAX_RADIUS;   // 62: the staged side at the largest radius
static constexpr float VS_EMPTY = 100.0f;                     // the depth of a pixel no triangle covers
static constexpr int VS_MAX_RES = 2048, VS_MAX_VIEWS = 64;
static_assert(VS_TILE == 32, "the passes split an item into (row, column) with >> 5 and & 31");

// ---- window minimum ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VS_THREADS) void md_vs_window_min_kernel(const float* __restrict__ rast, int H, int W, int r,
                                                                      float* __restrict__ dmin) {
  __shared__ float s_d[VS_SPAN * VS_SPAN];                    // D of the tile and its apron, row stride `span`
  __shared__ float s_row[VS_SPAN * VS_TILE];                  // the row minima of every staged row at the 32 output columns
  const int b = blockIdx.z, i0 = blockIdx.y * VS_TILE, j0 = blockIdx.x * VS_TILE;
  const int span = VS_TILE + 2 * r, taps = 2 * r;
  const float* img = rast + (int64_t)b * H * W * 4;
  for (int k = threadIdx.x; k < span * span; k += VS_THREADS) {
    const int ly = k / span, lx = k - ly * span;
    const int gi = i0 - r + ly, gj = j0 - r + lx;
    float d = INFINITY;                                       // outside the image: takes no part
    if (gi >= 0 && gi < H && gj >= 0 && gj < W) {
      const float2 zi = *(const float2*)(img + ((int64_t)gi * W + gj) * 4 + 2);       // (zf, id)
      d = zi.y != 0.f ? zi.x : VS_EMPTY;
    }
    s_d[k] = d;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < span * VS_TILE; k += VS_THREADS) {
    const int ly = k >> 5, x = k & 31;
    const float* row = s_d + ly * span + x;
    float m = row[0];
    for (int t = 1; t <= taps; ++t) m = fminf(m, row[t]);
    s_row[k] = m;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < VS_TILE * VS_TILE; k += VS_THREADS) {
    const int y = k >> 5, x = k & 31;
    const int gi = i0 + y, gj = j0 + x;
    float m = s_row[k];
    for (int t = 1; t <= taps; ++t) m = fminf(m, s_row[k + t * VS_TILE]);
    if (gi < H && gj < W) dmin[((int64_t)b * H + gi) * W + gj] = m;
  }
}

// ---- centres ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VS_THREADS) void md_vs_tet_visibility_kernel(const float* __restrict__ dmin,
                                                                          const float* __restrict__ centres,
                                                                          const float* __restrict__ mvp, int64_t T, int H, int W,
                                                                          uint8_t* __restrict__ visible) {
  const int64_t t = (int64_t)blockIdx.x * VS_THREADS + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= T) return;
  const float* m = mvp + b * 16;
  const float x = centres[t * 3], y = centres[t * 3 + 1], z = centres[t * 3 + 2];
  float c[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = ((x * m[4 * k] + y * m[4 * k + 1]) + z * m[4 * k + 2]) + m[4 * k + 3];
  bool ok = __builtin_isfinite(c[0]) && __builtin_isfinite(c[1]) && __builtin_isfinite(c[2]) && __builtin_isfinite(c[3]) &&
            c[3] > 0.f;
  const float S[3] = {(float)(W - 1), (float)(H - 1), (float)(H - 1)};
  float n[3], q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    n[k] = __fdiv_rn(c[k], c[3]);
    const float half = __fdiv_rn(n[k], 2.0f);
    const float unit = half + 0.5f;
    q[k] = rintf(unit * S[k]);
    ok = ok && q[k] >= 0.f && q[k] <= S[k];                   // in float: NaN and anything beyond int32 fail here
  }
  uint8_t vis = 0;
  if (ok) {
    const float d = dmin[((int64_t)b * H + (int)q[1]) * W + (int)q[0]];
    vis = (d >= n[2] || d == VS_EMPTY) ? 1 : 0;
  }
  visible[(int64_t)b * T + t] = vis;
}

// ---- labels ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VS_THREADS) void md_vs_rast_mark_tets_kernel(const float* __restrict__ rast,
                                                                          const int64_t* __restrict__ face_tet, int64_t n_pixels,
                                                                          int64_t F, int64_t T, uint8_t* __restrict__ rast_tet) {
  const int64_t p = (int64_t)blockIdx.x * VS_THREADS + threadIdx.x;
  if (p >= n_pixels) return;
  const float id = rast[p * 4 + 3];
  if (!(id >= 1.f && id <= (float)F)) return;                 // uncovered, NaN, or a face the table does not have
  const int64_t f = (int64_t)id - 1;
  if (f >= F) return;
  const int64_t t = face_tet[f];
  if (t >= 0 && t < T) rast_tet[t] = 1;
}

__global__ __launch_bounds__(VS_THREADS) void md_vs_tets_mark_verts_kernel(const uint8_t* __restrict__ visible,
                                                                           const uint8_t* __restrict__ rast_tet,
                                                                           const int64_t* __restrict__ indices, int B, int64_t T,
                                                                           int64_t N, float* __restrict__ vis,
                                                                           uint8_t* __restrict__ vis_rast) {
  const int64_t t = (int64_t)blockIdx.x * VS_THREADS + threadIdx.x;
  if (t >= T) return;
  bool seen = false;
  for (int b = 0; b < B; ++b) seen = seen || visible[(int64_t)b * T + t] != 0;
  const bool either = seen || (rast_tet != nullptr && rast_tet[t] != 0);
  if (!either) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t v = indices[t * 4 + k];
    if (v < 0 || v >= N) continue;
    if (seen) vis[v] = 1.0f;
    vis_rast[v] = 1;
  }
}

// ---- exports -------------------------------------------------------------------------------------------------------------------
static int vs_image_sizes(int32_t batch, int32_t H, int32_t W) {
  if (batch <= 0 || H <= 0 || W <= 0) return MD_ERR_BAD_ARG;
  if (batch > VS_MAX_VIEWS || H > VS_MAX_RES || W > VS_MAX_RES) return MD_ERR_UNSUPPORTED;
  return MD_OK;
}

// counts of tets, faces and vertices: positive, and small enough that a launch of one lane each fits the grid
static int vs_count(int64_t n) {
  if (n <= 0) return MD_ERR_BAD_ARG;
  return md_fits_i32(n) ? MD_OK : MD_ERR_UNSUPPORTED;
}

extern "C" int md_window_min(const float* rast, int32_t batch, int32_t H, int32_t W, int32_t radius, float* dmin, void* stream) {
  if (md_any_bad<16>(rast) || md_any_bad<4>(dmin)) return MD_ERR_BAD_ARG;
  if (radius < 0) return MD_ERR_BAD_ARG;
  const int rc = vs_image_sizes(batch, H, W);
  if (rc != MD_OK) return rc;
  if (radius > VS_MAX_RADIUS) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  const dim3 grid((W + VS_TILE - 1) / VS_TILE, (H + VS_TILE - 1) / VS_TILE, batch);
  hipLaunchKernelGGL(md_vs_window_min_kernel, grid, dim3(VS_THREADS), 0, (hipStream_t)stream, rast, (int)H, (int)W, (int)radius, dmin);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_tet_visibility(const float* dmin, const float* centres, const float* mvp, int32_t batch, int64_t n_tets, int32_t H,
                                 int32_t W, uint8_t* visible, void* stream) {
  if (md_any_bad<4>(dmin, centres, mvp) || md_any_bad<1>(visible)) return MD_ERR_BAD_ARG;
  int rc = vs_image_sizes(batch, H, W);
  if (rc == MD_OK) rc = vs_count(n_tets);
  if (rc != MD_OK) return rc;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_vs_tet_visibility_kernel, dim3(md_blocks(n_tets, VS_THREADS), batch), dim3(VS_THREADS), 0, (hipStream_t)stream,
                     dmin, centres, mvp, n_tets, (int)H, (int)W, visible);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

extern "C" int md_rast_mark_tets(const float* rast, const int64_t* face_tet, int32_t batch, int32_t H, int32_t W, int64_t n_faces,
                                 int64_t n_tets, uint8_t* rast_tet, void* stream) {
  if (md_any_bad<16>(rast) || md_any_bad<8>(face_tet) || md_any_bad<1>(rast_tet)) return MD_ERR_BAD_ARG;
  int rc = vs_image_sizes(batch, H, W);
  if (rc == MD_OK) rc = vs_count(n_faces);
  if (rc == MD_OK) rc = vs_count(n_tets);
  if (rc != MD_OK) return rc;
  if (n_faces >= (1LL << 24)) return MD_ERR_UNSUPPORTED;      // a float32 id holds face + 1 exactly below 2^24 only
  const int64_t n_pixels = (int64_t)batch * H * W;
  MD_LAUNCH_1D(md_vs_rast_mark_tets_kernel, n_pixels, VS_THREADS, rast, face_tet, n_pixels, n_faces, n_tets, rast_tet);
}

extern "C" int md_tets_mark_verts(const uint8_t* visible, const uint8_t* rast_tet, const int64_t* indices, int32_t batch,
                                  int64_t n_tets, int64_t n_verts, float* vis, uint8_t* vis_rast, void* stream) {
  if (md_any_bad<1>(visible, vis_rast) || md_any_bad<8>(indices) || md_any_bad<4>(vis)) return MD_ERR_BAD_ARG;
  if (batch <= 0) return MD_ERR_BAD_ARG;
  if (batch > VS_MAX_VIEWS) return MD_ERR_UNSUPPORTED;
  int rc = vs_count(n_tets);
  if (rc == MD_OK) rc = vs_count(n_verts);
  if (rc != MD_OK) return rc;
  MD_LAUNCH_1D(md_vs_tets_mark_verts_kernel, n_tets, VS_THREADS, visible, rast_tet, indices, (int)batch, n_tets, n_verts, vis, vis_rast);
}
