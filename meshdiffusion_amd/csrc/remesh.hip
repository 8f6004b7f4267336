// Isotropic remeshing of generated meshes: the `meshing_isotropic_explicit_remeshing` the reference runs before and after its
// smoothing at the tail of nvdiffrec/eval.py:449-456.  Built IN THE MANNER OF MeshLab's filter under a contract of its own, not
// bit-equal to MeshLab: a parallel form of Botsch-Kobbelt remeshing (split long edges, collapse short ones, flip towards valence
// six, relax tangentially) in which every decision is a pure function of the state before the launch, so the result depends
// neither on the order of the threads nor on where the atomics land.  It runs after generation: nothing here has a gradient.
//
// THE REMESHING CONTRACT (tests/remesh_cases.py restates it in float32 numpy, decision for decision)
//   Inputs      the concatenated batch of the mesh post-processing contract (csrc/meshpost.hip): verts fp32 [V][3], faces int64 [F][3]
//               of global ids, vert_mesh int32 [V] (vertices grouped by ascending mesh), and a target length per mesh, target fp32
//               [M] (default: the mesh's own mean edge length times target_scale).  hi2 = fl((4/3 L)^2) and lo2 = fl((4/5 L)^2)
//               are computed once on the host (in float64, rounded once to fp32).  The mesh of an edge is that of its lower endpoint.
//   Tables      rebuilt by the host (torch plumbing) before every launch group from the faces of that moment: the edge table
//               (lo, hi, mult int64 [E]) and the neighbour CSR (ptr int32 [V+1], adj int32 [2 E], nbr = code >> 1) of `mesh_edges`;
//               the corner CSR (cptr int32 [V+1], corner int32 [3 F]) of `csr_by_row` over faces.reshape(-1): the codes 3 f + k of
//               the corners that name a vertex, ascending; and vflag int32 [V]: bit 0 = the vertex is on an edge of mult == 1 (a
//               BOUNDARY vertex), bit 1 = it is on an edge of mult >= 3 or named by a face that names a vertex twice.  A vertex with
//               vflag != 0 is FIXED.  The valence of a vertex is the length of its neighbour row.
//   Arithmetic  fp32, every operation rounded on its own (fp contract off), no floating-point atomics.  sub(a, b) = a - b per
//               component; dot(u, v) = (u0 v0 + u1 v1) + u2 v2; len2(a, b) = dot(d, d) with d = sub(a, b); cross(u, v) = (u1 v2 - u2 v1,
//               u2 v0 - u0 v2, u0 v1 - u1 v0); nrm(p0, p1, p2) = cross(sub(p1, p0), sub(p2, p0)); mid(a, b) = 0.5f * (a + b).  The
//               predicates use squared lengths and unnormalised cross and dot products only: no sqrt, no division.  A predicate
//               written `x > y` fails on NaN.  Only the relax pass takes a square root and divides.
//   Iteration   split, then collapse rounds, then flip rounds, then relax; `iters` <= MD_REMESH_MAX_ITERS of them.
//   1 Split     mark: edge e is marked iff len2(lo, hi) > hi2[mesh]; mid[e] = mid(lo, hi) is written for every edge.  Marked edge
//               number r in table order (host: exclusive cumsum) becomes vertex V + r, of the mesh of the edge; the host then
//               re-sorts the vertices stably by mesh.  count / emit, one thread per face (v0, v1, v2) with corner edges
//               e_k = (v_{k+1}, v_{k+2}) looked up by binary search of (lo, hi), midpoints m_k: a face that names a vertex twice
//               or whose edges are not all found counts 1 and passes through unchanged (its edges stay in the table and may be
//               marked: its neighbours across them are split, the face keeps the long edge and no area, and a marked edge that only
//               such faces hold still yields its midpoint vertex, which no face then names); otherwise k marked edges
//               give k + 1 children, consecutive, in face order (host cumsum of the counts), each keeping the orientation:
//                 k = 1, e_j marked:  (v_j, v_j+1, m_j), (v_j, m_j, v_j+2)
//                 k = 3:              (v0, m2, m1), (v1, m0, m2), (v2, m1, m0), (m0, m1, m2)
//                 k = 2, e_j unmarked: (v_j, m_j+2, m_j+1), then the quadrilateral (m_j+2, v_j+1, v_j+2, m_j+1) cut from the midpoint
//                                     of the longer marked edge (len2; tie: the lower edge index): from m_j+2:
//                                     (m_j+2, v_j+1, v_j+2), (m_j+2, v_j+2, m_j+1); from m_j+1: (m_j+1, m_j+2, v_j+1), (m_j+1, v_j+1, v_j+2)
//               All faces of an edge see the same mark, so the result is conforming on boundary and non-manifold edges too.
//   2 Collapse  at most MD_REMESH_COLLAPSE_ROUNDS rounds of three launches.  candidates, one thread per edge (a, b) = (lo, hi), p =
//               mid(a, b); all of: mult == 2; a and b not FIXED; len2(a, b) < lo2[mesh]; exactly two faces in the corner row of a
//               name b, with different third vertices c, d; the sorted neighbour rows of a and b share exactly two vertices and
//               they are c and d (the link condition); val(c) > 3 and val(d) > 3; val(a) + val(b) - 4 >= 3 (the merged vertex
//               keeps a fan); every x of N(a) u N(b) other than a, b has len2(x, p) <= hi2[mesh]; every face in the corner rows of a
//               and b that does not name both has dot(nrm(old), nrm(with that vertex at p)) > 0.  claim: a candidate does an
//               integer atomicMin of its priority = (float bits of len2) << 32 | edge index (unsigned 64-bit) into the word of every
//               vertex of N(a) u N(b) (which holds a and b); the host sets the words to all ones.  apply: a candidate wins iff every
//               word it claimed holds its priority; winners have disjoint, non-adjacent rings, so no winner reads what another
//               writes.  A winner writes verts[a] = p, remap[b] = a (the host sets remap[v] = v) and adds one to the counter.  The
//               host reads the 4-byte counter (0 ends the rounds), remaps the faces, drops those that BECAME degenerate, drops the
//               vertices b, and compacts both in order.  Vertices that no face names are kept.
//   3 Flip      at most MD_REMESH_FLIP_ROUNDS rounds of the same shape.  candidates, one thread per edge (a, b) = (lo, hi): mult ==
//               2; a and b not FIXED; the corner row of a holds exactly one face (a, b, c) (b follows a) and one (b, a, d) (a follows
//               b), c != d; val(a) > 3, val(b) > 3; (min(c, d), max(c, d)) is not in the edge table; gain = sum over a, b, c, d of
//               |val - t| before minus after (a, b lose one, c, d gain one; t = 4 on a boundary vertex, else 6) > 0; n1 = nrm(a, b, c),
//               n2 = nrm(b, a, d), q = dot(n1, n2): q > 0 and q q >= (cos2 dot(n1, n1)) dot(n2, n2), cos2 = fl(cos^2 flip_angle); with
//               s = n1 + n2: dot(nrm(a, d, c), s) > 0 and dot(nrm(d, b, c), s) > 0; and the flip does not lower the smallest of the six angles:
//               with c(corner) = d |d| / (dot(u, u) dot(w, w)), d = dot(u, w), u and w the corner's two edge vectors (the signed
//               cos^2, kept as the fraction num / den), worst(faces) = the largest c over their corners in order (a later corner
//               replaces the kept one iff num den_kept > num_kept den), the flip is refused iff num_new den_old > num_old den_new
//               for worst((a,b,c), (b,a,d)) and worst((a,d,c), (d,b,c)) -- no division; the products leave the fp32 range only for
//               edges below about 1e-5, where the comparison degrades to "not refused".  Priority (16 - gain) << 32 | edge index, claimed on
//               a, b, c, d.  A winner rewrites the slot of (a, b, c) with (a, d, c) and that of (b, a, d) with (d, b, c) and adds one to the
//               counter; nothing is compacted.
//   4 Relax     one thread per vertex v, from a copy to `out`: a FIXED vertex or one without a row keeps its bits.  Otherwise m = the
//               compensated sum (md_kahan_add) of the neighbours in row order / (float)n, d = m - x; g = the plain sum, in the order of
//               the corner row, of nrm(face) over the faces whose three indices are in range; n = g / sqrt(max(dot(g, g), 1e-20));
//               t = dot(n, d); x' = x + lam * (d - n * t) per component.  lam == 0 skips the pass on the host.
//   Projection  not a kernel of this file: with remesh(project=True) the host ends every iteration, after the relax, by replacing every
//               vertex with its closest point on the input surface of its mesh (md_mesh_query, the mesh distance contract of
//               csrc/meshdist.hip).  Without it each collapse to a midpoint moves inward by about L^2 / 8 R.
//   Not built   feature-edge preservation, adaptive sizing, cotangent weights, collapses or flips that touch a boundary vertex at a
//               or b.
//   Safety      every loop is bounded by a row length or a constant; no kernel waits on another thread; within a launch two
//               threads write the same word only through integer atomicMin / atomicAdd; rounds stop on the host at their cap,
//               which is not an error.  The library allocates nothing.
//   Limits      null or misaligned pointers and non-positive sizes MD_ERR_BAD_ARG; V, 2 E or 3 F (3 F_out) beyond int32, a non-finite
//               lam or cos2 MD_ERR_UNSUPPORTED / BAD_ARG as in meshpost.hip; iters > MD_REMESH_MAX_ITERS, a non-finite target or a
//               target <= 0 are refused by the host (ValueError).  An index outside its table is absent and never read.
//
// Kernels.  Latency-bound gathers over short rows (valence ~6): one thread per edge, face or vertex, 256-thread workgroups, no LDS.
#include "md_args.h"
#include "md_gather.h"

#pragma clang fp contract(off)

static constexpr int RM_THREADS = 256;

struct rm_v3 { float x, y, z; };
__device__ __forceinline__ rm_v3 rm_load(const float* verts, int64_t v) { return {verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2]}; }
__device__ __forceinline__ rm_v3 rm_sub(rm_v3 a, rm_v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ rm_v3 rm_add(rm_v3 a, rm_v3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ float rm_dot(rm_v3 u, rm_v3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ float rm_len2(rm_v3 a, rm_v3 b) { const rm_v3 d = rm_sub(a, b); return rm_dot(d, d); }
__device__ __forceinline__ rm_v3 rm_cross(rm_v3 u, rm_v3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ __forceinline__ rm_v3 rm_nrm(rm_v3 p0, rm_v3 p1, rm_v3 p2) { return rm_cross(rm_sub(p1, p0), rm_sub(p2, p0)); }
__device__ __forceinline__ rm_v3 rm_mid(rm_v3 a, rm_v3 b) { return {0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z)}; }

// the edge (lo[e], hi[e]) of thread e, in range and ordered, else false
__device__ __forceinline__ bool rm_edge(const int64_t* lo, const int64_t* hi, int e, int V, int& a, int& b) {
  const int64_t l = lo[e], h = hi[e];
  if (l < 0 || h <= l || h >= V) return false;
  a = (int)l; b = (int)h;
  return true;
}

// the index of the edge {u, v} in the table sorted by (lo, hi), or -1
__device__ __forceinline__ int rm_find_edge(const int64_t* lo, const int64_t* hi, int E, int64_t u, int64_t v) {
  const int64_t a = u < v ? u : v, b = u < v ? v : u;
  int l = 0, r = E;                                            // at most 32 halvings
  while (l < r) {
    const int m = l + ((r - l) >> 1);
    const int64_t ml = lo[m], mh = hi[m];
    if (ml < a || (ml == a && mh < b)) l = m + 1; else r = m;
  }
  return (l < E && lo[l] == a && hi[l] == b) ? l : -1;
}

// a row of a CSR clamped to its table
__device__ __forceinline__ void rm_row(const int32_t* ptr, int v, int n, int& j0, int& j1) {
  j0 = max(ptr[v], 0);
  j1 = min(ptr[v + 1], n);
}

// corner code -> (f, the three indices rotated so that i0 sits at the corner); false if absent
__device__ __forceinline__ bool rm_corner(const int64_t* faces, int code, int V, int F, int& f, int& i0, int& i1, int& i2) {
  if (code < 0 || code >= 3 * F) return false;
  f = code / 3;
  const int k = code - 3 * f;
  const int64_t x0 = faces[(int64_t)f * 3 + k], x1 = faces[(int64_t)f * 3 + (k + 1) % 3], x2 = faces[(int64_t)f * 3 + (k + 2) % 3];
  if (x0 < 0 || x0 >= V || x1 < 0 || x1 >= V || x2 < 0 || x2 >= V) return false;
  i0 = (int)x0; i1 = (int)x1; i2 = (int)x2;
  return true;
}

// ---- split ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RM_THREADS) void md_rm_split_mark_kernel(const float* __restrict__ verts, const int64_t* __restrict__ lo,
                                                                      const int64_t* __restrict__ hi, const int32_t* __restrict__ vert_mesh,
                                                                      const float* __restrict__ hi2, int V, int E, int M,
                                                                      int32_t* __restrict__ mark, float* __restrict__ mid) {
  const int e = blockIdx.x * RM_THREADS + threadIdx.x;
  if (e >= E) return;
  int a, b, marked = 0;
  rm_v3 p = {0.f, 0.f, 0.f};
  if (rm_edge(lo, hi, e, V, a, b)) {
    const rm_v3 A = rm_load(verts, a), B = rm_load(verts, b);
    p = rm_mid(A, B);
    const int m = vert_mesh[a];
    if ((unsigned)m < (unsigned)M && rm_len2(A, B) > hi2[m]) marked = 1;
  }
  mark[e] = marked;
  mid[(int64_t)e * 3] = p.x; mid[(int64_t)e * 3 + 1] = p.y; mid[(int64_t)e * 3 + 2] = p.z;
}

// the three corner edges of face f and their marks; false = the face passes through unchanged
__device__ __forceinline__ bool rm_face_marks(const int64_t* faces, const int64_t* lo, const int64_t* hi, const int32_t* mark, int V,
                                              int E, int f, int64_t v[3], int e[3], int mk[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = faces[(int64_t)f * 3 + k];
    if (v[k] < 0 || v[k] >= V) ok = false;
  }
  if (!ok || v[0] == v[1] || v[1] == v[2] || v[2] == v[0]) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e[k] = rm_find_edge(lo, hi, E, v[(k + 1) % 3], v[(k + 2) % 3]);
    if (e[k] < 0) return false;
    mk[k] = mark[e[k]] != 0;
  }
  return true;
}

__global__ __launch_bounds__(RM_THREADS) void md_rm_split_count_kernel(const int64_t* __restrict__ faces, const int64_t* __restrict__ lo,
                                                                       const int64_t* __restrict__ hi, const int32_t* __restrict__ mark,
                                                                       int V, int E, int F, int32_t* __restrict__ count) {
  const int f = blockIdx.x * RM_THREADS + threadIdx.x;
  if (f >= F) return;
  int64_t v[3];
  int e[3], mk[3];
  count[f] = rm_face_marks(faces, lo, hi, mark, V, E, f, v, e, mk) ? 1 + mk[0] + mk[1] + mk[2] : 1;
}

__device__ __forceinline__ void rm_put(int64_t* out, int64_t slot, int64_t F_out, int64_t a, int64_t b, int64_t c) {
  if (slot < 0 || slot >= F_out) return;                       // never with the offsets of the host
  out[slot * 3] = a; out[slot * 3 + 1] = b; out[slot * 3 + 2] = c;
}

__global__ __launch_bounds__(RM_THREADS) void md_rm_split_emit_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                                      const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                                      const int32_t* __restrict__ mark, const int32_t* __restrict__ rank,
                                                                      const int32_t* __restrict__ offset, int V, int E, int F, int64_t F_out,
                                                                      int64_t* __restrict__ out) {
  const int f = blockIdx.x * RM_THREADS + threadIdx.x;
  if (f >= F) return;
  int64_t v[3], m[3] = {0, 0, 0};
  int e[3], mk[3];
  const int64_t o = offset[f];
  if (!rm_face_marks(faces, lo, hi, mark, V, E, f, v, e, mk) || mk[0] + mk[1] + mk[2] == 0) {
    rm_put(out, o, F_out, faces[(int64_t)f * 3], faces[(int64_t)f * 3 + 1], faces[(int64_t)f * 3 + 2]);
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (mk[k]) m[k] = (int64_t)V + rank[e[k]];
  const int n = mk[0] + mk[1] + mk[2];
  if (n == 3) {
    rm_put(out, o, F_out, v[0], m[2], m[1]);
    rm_put(out, o + 1, F_out, v[1], m[0], m[2]);
    rm_put(out, o + 2, F_out, v[2], m[1], m[0]);
    rm_put(out, o + 3, F_out, m[0], m[1], m[2]);
  } else if (n == 1) {
    const int j = mk[0] ? 0 : (mk[1] ? 1 : 2);
    rm_put(out, o, F_out, v[j], v[(j + 1) % 3], m[j]);
    rm_put(out, o + 1, F_out, v[j], m[j], v[(j + 2) % 3]);
  } else {
    const int j = !mk[0] ? 0 : (!mk[1] ? 1 : 2);
    const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    rm_put(out, o, F_out, v[j], m[j2], m[j1]);
    // e[j2] = (v_j, v_j1) carries m_j2, e[j1] = (v_j2, v_j) carries m_j1
    const float l2 = rm_len2(rm_load(verts, v[j]), rm_load(verts, v[j1]));
    const float l1 = rm_len2(rm_load(verts, v[j2]), rm_load(verts, v[j]));
    const bool from2 = l2 > l1 || (l2 == l1 && e[j2] < e[j1]);
    if (from2) {
      rm_put(out, o + 1, F_out, m[j2], v[j1], v[j2]);
      rm_put(out, o + 2, F_out, m[j2], v[j2], m[j1]);
    } else {
      rm_put(out, o + 1, F_out, m[j1], m[j2], v[j1]);
      rm_put(out, o + 2, F_out, m[j1], v[j1], v[j2]);
    }
  }
}

// ---- collapse ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool rm_collapse_ok(const float* verts, const int64_t* faces, const int64_t* mult, const int32_t* ptr,
                                               const int32_t* adj, const int32_t* cptr, const int32_t* corner, const int32_t* vflag,
                                               const int32_t* vert_mesh, const float* lo2, const float* hi2, int V, int E, int F, int M,
                                               int e, int a, int b, float& len2) {
  if (mult[e] != 2 || vflag[a] != 0 || vflag[b] != 0) return false;
  const int mesh = vert_mesh[a];
  if ((unsigned)mesh >= (unsigned)M) return false;
  const rm_v3 A = rm_load(verts, a), B = rm_load(verts, b);
  len2 = rm_len2(A, B);
  if (!(len2 < lo2[mesh])) return false;
  const float h2 = hi2[mesh];
  // the two faces of the edge and their third vertices
  int c0, c1, nopp = 0, opp[2] = {-1, -1};
  rm_row(cptr, a, 3 * F, c0, c1);
  for (int j = c0; j < c1; ++j) {
    int f, i0, i1, i2;
    if (!rm_corner(faces, corner[j], V, F, f, i0, i1, i2) || i0 != a) continue;
    if (i1 != b && i2 != b) continue;
    if (nopp < 2) opp[nopp] = i1 == b ? i2 : i1;
    ++nopp;
  }
  if (nopp != 2 || opp[0] == opp[1]) return false;
  // the link condition: a merge of the two ascending rows
  int a0, a1, b0, b1;
  rm_row(ptr, a, 2 * E, a0, a1);
  rm_row(ptr, b, 2 * E, b0, b1);
  int common = 0;
  for (int i = a0, j = b0; i < a1 && j < b1;) {
    const int x = adj[i] >> 1, y = adj[j] >> 1;
    if (x < y) ++i;
    else if (y < x) ++j;
    else {
      if (x != opp[0] && x != opp[1]) return false;
      ++common; ++i; ++j;
    }
  }
  if (common != 2) return false;
  for (int k = 0; k < 2; ++k) {
    if ((unsigned)opp[k] >= (unsigned)V) return false;
    if (ptr[opp[k] + 1] - ptr[opp[k]] <= 3) return false;
  }
  if ((a1 - a0) + (b1 - b0) - 4 < 3) return false;
  const rm_v3 p = rm_mid(A, B);
  for (int side = 0; side < 2; ++side) {
    const int r0 = side ? b0 : a0, r1 = side ? b1 : a1;
    for (int j = r0; j < r1; ++j) {
      const int x = adj[j] >> 1;
      if ((unsigned)x >= (unsigned)V || x == a || x == b) continue;
      if (!(rm_len2(rm_load(verts, x), p) <= h2)) return false;
    }
  }
  for (int side = 0; side < 2; ++side) {
    const int v = side ? b : a, w = side ? a : b;
    rm_row(cptr, v, 3 * F, c0, c1);
    for (int j = c0; j < c1; ++j) {
      int f, i0, i1, i2;
      if (!rm_corner(faces, corner[j], V, F, f, i0, i1, i2) || i0 != v) continue;
      if (i1 == w || i2 == w) continue;                       // one of the two faces that vanish
      const rm_v3 P0 = rm_load(verts, i0), P1 = rm_load(verts, i1), P2 = rm_load(verts, i2);
      if (!(rm_dot(rm_nrm(P0, P1, P2), rm_nrm(p, P1, P2)) > 0.f)) return false;
    }
  }
  return true;
}

__global__ __launch_bounds__(RM_THREADS) void md_rm_collapse_cand_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                                         const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                                         const int64_t* __restrict__ mult, const int32_t* __restrict__ ptr,
                                                                         const int32_t* __restrict__ adj, const int32_t* __restrict__ cptr,
                                                                         const int32_t* __restrict__ corner, const int32_t* __restrict__ vflag,
                                                                         const int32_t* __restrict__ vert_mesh, const float* __restrict__ lo2,
                                                                         const float* __restrict__ hi2, int V, int E, int F, int M,
                                                                         int32_t* __restrict__ cand, unsigned long long* __restrict__ prio) {
  const int e = blockIdx.x * RM_THREADS + threadIdx.x;
  if (e >= E) return;
  int a, b;
  float len2 = 0.f;
  const bool ok = rm_edge(lo, hi, e, V, a, b) &&
                  rm_collapse_ok(verts, faces, mult, ptr, adj, cptr, corner, vflag, vert_mesh, lo2, hi2, V, E, F, M, e, a, b, len2);
  cand[e] = ok ? 1 : 0;
  prio[e] = ok ? (((unsigned long long)__float_as_uint(len2) << 32) | (unsigned)e) : ~0ull;
}

// the vertices of N(a) u N(b): the row of a (it holds b), then the row of b (it holds a)
template <bool CLAIM>
__device__ __forceinline__ bool rm_ring_words(const int32_t* ptr, const int32_t* adj, int V, int E, int a, int b, unsigned long long p,
                                              unsigned long long* word) {
  for (int side = 0; side < 2; ++side) {
    int j0, j1;
    rm_row(ptr, side ? b : a, 2 * E, j0, j1);
    for (int j = j0; j < j1; ++j) {
      const int x = adj[j] >> 1;
      if ((unsigned)x >= (unsigned)V) continue;
      if (CLAIM) atomicMin(word + x, p);
      else if (word[x] != p) return false;
    }
  }
  return true;
}

__global__ __launch_bounds__(RM_THREADS) void md_rm_collapse_claim_kernel(const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                                          const int32_t* __restrict__ ptr, const int32_t* __restrict__ adj,
                                                                          const int32_t* __restrict__ cand,
                                                                          const unsigned long long* __restrict__ prio, int V, int E,
                                                                          unsigned long long* word) {
  const int e = blockIdx.x * RM_THREADS + threadIdx.x;
  int a, b;
  if (e >= E || !cand[e] || !rm_edge(lo, hi, e, V, a, b)) return;
  rm_ring_words<true>(ptr, adj, V, E, a, b, prio[e], word);
}

__global__ __launch_bounds__(RM_THREADS) void md_rm_collapse_apply_kernel(const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                                          const int32_t* __restrict__ ptr, const int32_t* __restrict__ adj,
                                                                          const int32_t* __restrict__ cand,
                                                                          const unsigned long long* __restrict__ prio,
                                                                          unsigned long long* word, int V, int E, float* verts,
                                                                          int32_t* __restrict__ remap, int32_t* counter) {
  const int e = blockIdx.x * RM_THREADS + threadIdx.x;
  int a, b;
  if (e >= E || !cand[e] || !rm_edge(lo, hi, e, V, a, b)) return;
  if (!rm_ring_words<false>(ptr, adj, V, E, a, b, prio[e], word)) return;
  // a winner: nobody else reads or writes verts[a], verts[b] or remap[b] in this launch
  const rm_v3 p = rm_mid(rm_load(verts, a), rm_load(verts, b));
  verts[(int64_t)a * 3] = p.x; verts[(int64_t)a * 3 + 1] = p.y; verts[(int64_t)a * 3 + 2] = p.z;
  remap[b] = a;
  atomicAdd(counter, 1);
}

// ---- flip ----------------------------------------------------------------------------------------------------------------------
// the largest signed cos^2 = d |d| / ((u . u)(w . w)) over the corners seen so far, kept as a fraction and compared by cross-multiplying
__device__ __forceinline__ void rm_worst(rm_v3 P0, rm_v3 P1, rm_v3 P2, float& num, float& den, bool& has) {
  const rm_v3 p[3] = {P0, P1, P2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const rm_v3 u = rm_sub(p[(k + 1) % 3], p[k]), w = rm_sub(p[(k + 2) % 3], p[k]);
    const float d = rm_dot(u, w);
    const float n = d * fabsf(d), q = rm_dot(u, u) * rm_dot(w, w);
    if (!has || n * den > num * q) { num = n; den = q; has = true; }
  }
}

__device__ __forceinline__ int rm_dev(int val, int flag) { const int t = (flag & 1) ? 4 : 6; return val > t ? val - t : t - val; }

__device__ __forceinline__ bool rm_flip_ok(const float* verts, const int64_t* faces, const int64_t* lo, const int64_t* hi,
                                           const int64_t* mult, const int32_t* ptr, const int32_t* cptr, const int32_t* corner,
                                           const int32_t* vflag, float cos2, int V, int E, int F, int e, int a, int b, int info[4],
                                           int& gain) {
  if (mult[e] != 2 || vflag[a] != 0 || vflag[b] != 0) return false;
  int c0, c1, n1 = 0, n2 = 0, f1 = -1, f2 = -1, c = -1, d = -1;
  rm_row(cptr, a, 3 * F, c0, c1);
  for (int j = c0; j < c1; ++j) {
    int f, i0, i1, i2;
    if (!rm_corner(faces, corner[j], V, F, f, i0, i1, i2) || i0 != a) continue;
    if (i1 == b) { f1 = f; c = i2; ++n1; }                   // (a, b, c): b follows a
    else if (i2 == b) { f2 = f; d = i1; ++n2; }              // (a, d, b) = (b, a, d): a follows b
  }
  if (n1 != 1 || n2 != 1 || c == d || c == a || c == b || d == a || d == b) return false;
  const int va = ptr[a + 1] - ptr[a], vb = ptr[b + 1] - ptr[b], vc = ptr[c + 1] - ptr[c], vd = ptr[d + 1] - ptr[d];
  if (va <= 3 || vb <= 3) return false;
  if (rm_find_edge(lo, hi, E, c, d) >= 0) return false;
  const int fa = vflag[a], fb = vflag[b], fc = vflag[c], fd = vflag[d];
  gain = (rm_dev(va, fa) + rm_dev(vb, fb) + rm_dev(vc, fc) + rm_dev(vd, fd)) -
         (rm_dev(va - 1, fa) + rm_dev(vb - 1, fb) + rm_dev(vc + 1, fc) + rm_dev(vd + 1, fd));
  if (gain <= 0 || gain > 15) return false;
  const rm_v3 A = rm_load(verts, a), B = rm_load(verts, b), C = rm_load(verts, c), D = rm_load(verts, d);
  const rm_v3 na = rm_nrm(A, B, C), nb = rm_nrm(B, A, D);
  const float q = rm_dot(na, nb);
  if (!(q > 0.f)) return false;
  if (!(q * q >= (cos2 * rm_dot(na, na)) * rm_dot(nb, nb))) return false;
  const rm_v3 s = rm_add(na, nb);
  if (!(rm_dot(rm_nrm(A, D, C), s) > 0.f) || !(rm_dot(rm_nrm(D, B, C), s) > 0.f)) return false;
  float on = 0.f, od = 0.f, nn = 0.f, nd = 0.f;
  bool oh = false, nh = false;
  rm_worst(A, B, C, on, od, oh); rm_worst(B, A, D, on, od, oh);
  rm_worst(A, D, C, nn, nd, nh); rm_worst(D, B, C, nn, nd, nh);
  if (nn * od > on * nd) return false;                         // the flip would lower the smallest of the six angles
  info[0] = f1; info[1] = f2; info[2] = c; info[3] = d;
  return true;
}

__global__ __launch_bounds__(RM_THREADS) void md_rm_flip_cand_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                                     const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                                     const int64_t* __restrict__ mult, const int32_t* __restrict__ ptr,
                                                                     const int32_t* __restrict__ cptr, const int32_t* __restrict__ corner,
                                                                     const int32_t* __restrict__ vflag, float cos2, int V, int E, int F,
                                                                     int32_t* __restrict__ cand, unsigned long long* __restrict__ prio,
                                                                     int32_t* __restrict__ info) {
  const int e = blockIdx.x * RM_THREADS + threadIdx.x;
  if (e >= E) return;
  int a, b, gain = 0, q[4] = {-1, -1, -1, -1};
  const bool ok = rm_edge(lo, hi, e, V, a, b) &&
                  rm_flip_ok(verts, faces, lo, hi, mult, ptr, cptr, corner, vflag, cos2, V, E, F, e, a, b, q, gain);
  cand[e] = ok ? 1 : 0;
  prio[e] = ok ? (((unsigned long long)(unsigned)(16 - gain) << 32) | (unsigned)e) : ~0ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) info[(int64_t)e * 4 + k] = ok ? q[k] : -1;
}

__global__ __launch_bounds__(RM_THREADS) void md_rm_flip_claim_kernel(const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                                      const int32_t* __restrict__ cand,
                                                                      const unsigned long long* __restrict__ prio,
                                                                      const int32_t* __restrict__ info, int V, int E, unsigned long long* word) {
  const int e = blockIdx.x * RM_THREADS + threadIdx.x;
  int a, b;
  if (e >= E || !cand[e] || !rm_edge(lo, hi, e, V, a, b)) return;
  const int c = info[(int64_t)e * 4 + 2], d = info[(int64_t)e * 4 + 3];
  if ((unsigned)c >= (unsigned)V || (unsigned)d >= (unsigned)V) return;
  const unsigned long long p = prio[e];
  atomicMin(word + a, p); atomicMin(word + b, p); atomicMin(word + c, p); atomicMin(word + d, p);
}

__global__ __launch_bounds__(RM_THREADS) void md_rm_flip_apply_kernel(const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                                      const int32_t* __restrict__ cand,
                                                                      const unsigned long long* __restrict__ prio,
                                                                      const int32_t* __restrict__ info, const unsigned long long* word, int V,
                                                                      int E, int F, int64_t* faces, int32_t* counter) {
  const int e = blockIdx.x * RM_THREADS + threadIdx.x;
  int a, b;
  if (e >= E || !cand[e] || !rm_edge(lo, hi, e, V, a, b)) return;
  const int f1 = info[(int64_t)e * 4], f2 = info[(int64_t)e * 4 + 1], c = info[(int64_t)e * 4 + 2], d = info[(int64_t)e * 4 + 3];
  if ((unsigned)c >= (unsigned)V || (unsigned)d >= (unsigned)V || (unsigned)f1 >= (unsigned)F || (unsigned)f2 >= (unsigned)F) return;
  const unsigned long long p = prio[e];
  if (word[a] != p || word[b] != p || word[c] != p || word[d] != p) return;
  // a winner: its two faces hold only a, b, c, d, which no other winner holds
  faces[(int64_t)f1 * 3] = a; faces[(int64_t)f1 * 3 + 1] = d; faces[(int64_t)f1 * 3 + 2] = c;
  faces[(int64_t)f2 * 3] = d; faces[(int64_t)f2 * 3 + 1] = b; faces[(int64_t)f2 * 3 + 2] = c;
  atomicAdd(counter, 1);
}

// ---- relax ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RM_THREADS) void md_rm_relax_kernel(const float* __restrict__ src, const int64_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ ptr, const int32_t* __restrict__ adj,
                                                                 const int32_t* __restrict__ cptr, const int32_t* __restrict__ corner,
                                                                 const int32_t* __restrict__ vflag, int V, int E, int F, float lam,
                                                                 float* __restrict__ dst) {
  const int v = blockIdx.x * RM_THREADS + threadIdx.x;
  if (v >= V) return;
  const rm_v3 x = rm_load(src, v);
  float* o = dst + (int64_t)v * 3;
  o[0] = x.x; o[1] = x.y; o[2] = x.z;
  if (vflag[v] != 0) return;
  int j0, j1, n = 0;
  rm_row(ptr, v, 2 * E, j0, j1);
  float s[3] = {0.f, 0.f, 0.f}, lost[3] = {0.f, 0.f, 0.f};
  for (int j = j0; j < j1; ++j) {
    const int u = adj[j] >> 1;
    if ((unsigned)u >= (unsigned)V) continue;
    const rm_v3 q = rm_load(src, u);
    md_kahan_add(s[0], lost[0], q.x);
    md_kahan_add(s[1], lost[1], q.y);
    md_kahan_add(s[2], lost[2], q.z);
    ++n;
  }
  if (n == 0) return;
  const float fn = (float)n;
  const rm_v3 d = {s[0] / fn - x.x, s[1] / fn - x.y, s[2] / fn - x.z};
  rm_v3 g = {0.f, 0.f, 0.f};
  rm_row(cptr, v, 3 * F, j0, j1);
  for (int j = j0; j < j1; ++j) {
    int f, i0, i1, i2;
    if (!rm_corner(faces, corner[j], V, F, f, i0, i1, i2)) continue;
    const int64_t* t = faces + (int64_t)f * 3;                // the face's own order, not the corner's rotation
    g = rm_add(g, rm_nrm(rm_load(src, t[0]), rm_load(src, t[1]), rm_load(src, t[2])));
  }
  const float len = sqrtf(fmaxf(rm_dot(g, g), 1e-20f));
  const rm_v3 nn = {g.x / len, g.y / len, g.z / len};
  const float t = rm_dot(nn, d);
  o[0] = x.x + lam * (d.x - nn.x * t);
  o[1] = x.y + lam * (d.y - nn.y * t);
  o[2] = x.z + lam * (d.z - nn.z * t);
}

// ---- exports -------------------------------------------------------------------------------------------------------------------
extern "C" int md_remesh_split_mark(const float* verts, const int64_t* lo, const int64_t* hi, const int32_t* vert_mesh, const float* hi2,
                                    int64_t n_verts, int64_t n_edges, int64_t n_meshes, int32_t* mark, float* mid, void* stream) {
  if (md_any_bad<4>(verts, vert_mesh, hi2, mark, mid) || md_any_bad<8>(lo, hi)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0 || n_meshes <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges, n_meshes)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_split_mark_kernel, n_edges, RM_THREADS, verts, lo, hi, vert_mesh, hi2, (int)n_verts, (int)n_edges, (int)n_meshes, mark,
               mid);
}

extern "C" int md_remesh_split_count(const int64_t* faces, const int64_t* lo, const int64_t* hi, const int32_t* mark, int64_t n_verts,
                                     int64_t n_edges, int64_t n_faces, int32_t* count, void* stream) {
  if (md_any_bad<8>(faces, lo, hi) || md_any_bad<4>(mark, count)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0 || n_faces <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges, 3 * n_faces)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_split_count_kernel, n_faces, RM_THREADS, faces, lo, hi, mark, (int)n_verts, (int)n_edges, (int)n_faces, count);
}

extern "C" int md_remesh_split_emit(const float* verts, const int64_t* faces, const int64_t* lo, const int64_t* hi, const int32_t* mark,
                                    const int32_t* rank, const int32_t* offset, int64_t n_verts, int64_t n_edges, int64_t n_faces,
                                    int64_t n_faces_out, int64_t* out_faces, void* stream) {
  if (md_any_bad<4>(verts, mark, rank, offset) || md_any_bad<8>(faces, lo, hi, out_faces)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0 || n_faces <= 0 || n_faces_out < n_faces || out_faces == faces) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts + n_edges, 2 * n_edges, 3 * n_faces_out)) return MD_ERR_UNSUPPORTED;      // the new ids V + rank fit int32 too
  MD_LAUNCH_1D(md_rm_split_emit_kernel, n_faces, RM_THREADS, verts, faces, lo, hi, mark, rank, offset, (int)n_verts, (int)n_edges,
               (int)n_faces, n_faces_out, out_faces);
}

extern "C" int md_remesh_collapse_candidates(const float* verts, const int64_t* faces, const int64_t* lo, const int64_t* hi,
                                             const int64_t* mult, const int32_t* ptr, const int32_t* adj, const int32_t* cptr,
                                             const int32_t* corner, const int32_t* vflag, const int32_t* vert_mesh, const float* lo2,
                                             const float* hi2, int64_t n_verts, int64_t n_edges, int64_t n_faces, int64_t n_meshes,
                                             int32_t* cand, uint64_t* prio, void* stream) {
  if (md_any_bad<4>(verts, ptr, adj, cptr, corner, vflag, vert_mesh, lo2, hi2, cand) || md_any_bad<8>(faces, lo, hi, mult, prio))
    return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0 || n_faces <= 0 || n_meshes <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges, 3 * n_faces, n_meshes)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_collapse_cand_kernel, n_edges, RM_THREADS, verts, faces, lo, hi, mult, ptr, adj, cptr, corner, vflag, vert_mesh, lo2,
               hi2, (int)n_verts, (int)n_edges, (int)n_faces, (int)n_meshes, cand, (unsigned long long*)prio);
}

extern "C" int md_remesh_collapse_claim(const int64_t* lo, const int64_t* hi, const int32_t* ptr, const int32_t* adj, const int32_t* cand,
                                        const uint64_t* prio, int64_t n_verts, int64_t n_edges, uint64_t* word, void* stream) {
  if (md_any_bad<8>(lo, hi, prio, word) || md_any_bad<4>(ptr, adj, cand)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_collapse_claim_kernel, n_edges, RM_THREADS, lo, hi, ptr, adj, cand, (const unsigned long long*)prio, (int)n_verts,
               (int)n_edges, (unsigned long long*)word);
}

extern "C" int md_remesh_collapse_apply(const int64_t* lo, const int64_t* hi, const int32_t* ptr, const int32_t* adj, const int32_t* cand,
                                        const uint64_t* prio, uint64_t* word, int64_t n_verts, int64_t n_edges, float* verts,
                                        int32_t* remap, int32_t* counter, void* stream) {
  if (md_any_bad<8>(lo, hi, prio, word) || md_any_bad<4>(ptr, adj, cand, verts, remap, counter)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_collapse_apply_kernel, n_edges, RM_THREADS, lo, hi, ptr, adj, cand, (const unsigned long long*)prio,
               (unsigned long long*)word, (int)n_verts, (int)n_edges, verts, remap, counter);
}

extern "C" int md_remesh_flip_candidates(const float* verts, const int64_t* faces, const int64_t* lo, const int64_t* hi,
                                         const int64_t* mult, const int32_t* ptr, const int32_t* cptr, const int32_t* corner,
                                         const int32_t* vflag, float cos2, int64_t n_verts, int64_t n_edges, int64_t n_faces, int32_t* cand,
                                         uint64_t* prio, int32_t* info, void* stream) {
  if (md_any_bad<4>(verts, ptr, cptr, corner, vflag, cand, info) || md_any_bad<8>(faces, lo, hi, mult, prio)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0 || n_faces <= 0 || !(cos2 >= 0.f && cos2 <= 1.f)) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges, 3 * n_faces)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_flip_cand_kernel, n_edges, RM_THREADS, verts, faces, lo, hi, mult, ptr, cptr, corner, vflag, cos2, (int)n_verts,
               (int)n_edges, (int)n_faces, cand, (unsigned long long*)prio, info);
}

extern "C" int md_remesh_flip_claim(const int64_t* lo, const int64_t* hi, const int32_t* cand, const uint64_t* prio, const int32_t* info,
                                    int64_t n_verts, int64_t n_edges, uint64_t* word, void* stream) {
  if (md_any_bad<8>(lo, hi, prio, word) || md_any_bad<4>(cand, info)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_flip_claim_kernel, n_edges, RM_THREADS, lo, hi, cand, (const unsigned long long*)prio, info, (int)n_verts,
               (int)n_edges, (unsigned long long*)word);
}

extern "C" int md_remesh_flip_apply(const int64_t* lo, const int64_t* hi, const int32_t* cand, const uint64_t* prio, const int32_t* info,
                                    const uint64_t* word, int64_t n_verts, int64_t n_edges, int64_t n_faces, int64_t* faces,
                                    int32_t* counter, void* stream) {
  if (md_any_bad<8>(lo, hi, prio, word, faces) || md_any_bad<4>(cand, info, counter)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0 || n_faces <= 0) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges, 3 * n_faces)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_flip_apply_kernel, n_edges, RM_THREADS, lo, hi, cand, (const unsigned long long*)prio, info,
               (const unsigned long long*)word, (int)n_verts, (int)n_edges, (int)n_faces, faces, counter);
}

extern "C" int md_remesh_relax(const float* verts, const int64_t* faces, const int32_t* ptr, const int32_t* adj, const int32_t* cptr,
                               const int32_t* corner, const int32_t* vflag, int64_t n_verts, int64_t n_edges, int64_t n_faces, float lam,
                               float* out, void* stream) {
  if (md_any_bad<4>(verts, ptr, adj, cptr, corner, vflag, out) || md_any_bad<8>(faces)) return MD_ERR_BAD_ARG;
  if (n_verts <= 0 || n_edges <= 0 || n_faces <= 0 || out == verts || !(fabsf(lam) <= 3.402823466e+38f)) return MD_ERR_BAD_ARG;
  if (!md_fits_i32(n_verts, 2 * n_edges, 3 * n_faces)) return MD_ERR_UNSUPPORTED;
  MD_LAUNCH_1D(md_rm_relax_kernel, n_verts, RM_THREADS, verts, faces, ptr, adj, cptr, corner, vflag, (int)n_verts, (int)n_edges,
               (int)n_faces, lam, out);
}
