"""Cases and the numpy restatement of the mesh distance contract (the header comment of csrc/meshdist.hip): the closest point of a
query on the triangles of its mesh and the generalised winding number, written as elementwise numpy over (queries x triangles), one
operation at a time in `dtype` -- float32: the contract's arithmetic, decision for decision; float64: the same code path as the
yardstick, whose distance from the float32 form is the unit of the GPU tests' bars.  `remesh_with_projection_restated` composes the
passes of remesh_cases with the projection.  Shared by tools/gen_golden_meshdist.py, the CPU tests, the GPU tests and
tools/bench_meshdist.py.  Everything runs on the CPU.
"""
import functools

import numpy as np

import meshpost_cases as mc
import remesh_cases as rm

CASES = rm.CASES                                             # tetra, octa, uvsphere, ptorus, fan40, quad, degen, pair
CLOSED = rm.CLOSED
BIG = "uvsphere48"                                           # 9024 faces: more than one LDS tile
TILE = 256                                                   # MDQ_TILE of csrc/meshdist.hip
QUERY_SETS = ("lattice", "surface")
PROJECT_CASES = ("uvsphere", "ptorus", "pair")
PROJECT_ITERS = 2                                            # the second iteration starts from projected vertices
CHUNK = 512                                                  # triangles per numpy block
FOUR_PI = 4.0 * np.pi


# ---- queries and triangles -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice():
    """float32 [729,3]: the 9^3 lattice over [-1.25, 1.25]^3 shifted by 0.013 (1, 2, 3); 729 is no multiple of 256."""
    g = -1.25 + 2.5 * np.arange(9) / 8
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 0.013 * np.array([1.0, 2.0, 3.0])
    return p.astype(np.float32)


def n_meshes(name):
    return int(rm.vert_mesh(name).max()) + 1


@functools.lru_cache(maxsize=None)
def queries(name, which):
    """(points float32 [Q,3], point_mesh int32 [Q]) of a case: the lattice once per mesh, or the mesh's own vertices and the
    float32 midpoints 0.5 (a + b) of its edges (on the surface, where triangles tie), grouped by mesh."""
    M = n_meshes(name)
    if which == "lattice":
        return np.concatenate([lattice()] * M), np.repeat(np.arange(M, dtype=np.int32), lattice().shape[0])
    v, f = rm.mesh(name)
    v, vm = v.numpy(), rm.vert_mesh(name).numpy()
    lo, hi, _, _, _ = mc.edges_restated(f.numpy(), v.shape[0])
    mid = np.float32(0.5) * (v[lo] + v[hi])
    p, pm = np.concatenate([v, mid]), np.concatenate([vm, vm[lo]])
    order = np.argsort(pm, kind="stable")
    return p[order].astype(np.float32), pm[order].astype(np.int32)


def gather(verts, faces, vert_mesh=None):
    """(tri float32 [F,3,3] grouped by mesh, tri_ptr int64 [M+1], face_of int64 [F]): what meshdist.mesh_triangles builds.  A face
    belongs to the mesh of its first vertex; faces are sorted stably by mesh; tri[k] = verts[faces[face_of[k]]]."""
    v, f = np.asarray(verts, dtype=np.float32), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vm = np.zeros(v.shape[0], np.int64) if vert_mesh is None else np.asarray(vert_mesh, dtype=np.int64)
    M = int(vm.max()) + 1 if vm.size else 1
    fm = vm[f[:, 0]] if f.shape[0] else np.zeros(0, np.int64)
    face_of = np.argsort(fm, kind="stable")
    return v[f[face_of]], np.searchsorted(fm[face_of], np.arange(M + 1)), face_of


def ptr_of(ids, M):
    return np.searchsorted(np.asarray(ids, dtype=np.int64), np.arange(M + 1))


@functools.lru_cache(maxsize=None)
def case_triangles(name):
    v, f = rm.mesh(name)
    return gather(v.numpy(), f.numpy(), rm.vert_mesh(name).numpy())


# ---- arithmetic of the contract --------------------------------------------------------------------------------------------------
def _dot(u, v):
    return u[2] * v[2] + (u[1] * v[1] + u[0] * v[0])


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _form(points, tri, dtype):
    """p [Q,1] per component and (a, ab, ac) [1,T] per component, in dtype; ab and ac are formed once per triangle."""
    p = np.asarray(points, dtype=np.float32).astype(dtype)
    t = np.asarray(tri, dtype=np.float32).astype(dtype)
    comp = lambda x, axis: tuple(np.expand_dims(x[:, c], axis) for c in range(3))
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    return comp(p, 1), comp(a, 0), comp(b - a, 0), comp(c - a, 0)


def closest_block(points, tri, dtype=np.float32):
    """(d2 [Q,T], c [3][Q,T]) of every (query, triangle) pair by the contract in `dtype`."""
    ty = np.dtype(dtype).type
    p, a, ab, ac = _form(points, tri, dtype)
    zero, one = ty(0), ty(1)
    with np.errstate(all="ignore"):
        ap = tuple(p[k] - a[k] for k in range(3))
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = tuple(ap[k] - ab[k] for k in range(3))
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = tuple(ap[k] - ac[k] for k in range(3))
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        in_a = (d1 <= zero) & (d2 <= zero)
        in_b = (d3 >= zero) & (d4 <= d3)
        in_c = (d6 >= zero) & (d5 <= d6)
        in_ab = (vc <= zero) & (d1 >= zero) & (d3 <= zero)
        in_ac = (vb <= zero) & (d2 >= zero) & (d6 <= zero)
        in_bc = (va <= zero) & (e43 >= zero) & (e56 >= zero)
        den = (va + vb) + vc
        full = lambda x: np.broadcast_to(np.asarray(x, dtype=dtype), den.shape)
        nv, dv, nw, dw, bc = vb, den, vc, den, np.zeros(den.shape, bool)
        # the interior first, then every region from the last to the first: the first that holds wins
        for flag, (rnv, rdv, rnw, rdw, rbc) in ((in_bc, (nv, dv, e43, e43 + e56, True)), (in_ac, (zero, one, d2, d2 - d6, False)),
                                                (in_ab, (d1, d1 - d3, zero, one, False)), (in_c, (zero, one, one, one, False)),
                                                (in_b, (one, one, zero, one, False)), (in_a, (zero, one, zero, one, False))):
            nv, dv, nw, dw = (np.where(flag, full(r), cur) for r, cur in ((rnv, nv), (rdv, dv), (rnw, nw), (rdw, dw)))
            bc = np.where(flag, rbc, bc)
        w = nw / dw
        v = np.where(bc, one - w, nv / dv)
        c = tuple(a[k] + (ab[k] * v + ac[k] * w) for k in range(3))
        d = tuple(p[k] - c[k] for k in range(3))
        return _dot(d, d), c


def omega_block(points, tri, dtype=np.float32):
    """[Q,T]: the solid angle 2 atan2(det, den) of every (query, triangle) pair by the contract in `dtype`."""
    p, a, ab, ac = _form(points, tri, dtype)
    with np.errstate(all="ignore"):
        A = tuple(a[k] - p[k] for k in range(3))
        B = tuple(A[k] + ab[k] for k in range(3))
        C = tuple(A[k] + ac[k] for k in range(3))
        la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
        det = _dot(A, _cross(B, C))
        den = (((la * lb) * lc + _dot(A, B) * lc) + _dot(B, C) * la) + _dot(C, A) * lb
        return np.dtype(dtype).type(2) * np.arctan2(det, den)


def _spans(tri_ptr, query_ptr, T, Q):
    if tri_ptr is None:
        return [(0, T, 0, Q)]
    return [(int(tri_ptr[m]), int(tri_ptr[m + 1]), int(query_ptr[m]), int(query_ptr[m + 1])) for m in range(len(tri_ptr) - 1)]


def closest_restated(points, tri, tri_ptr=None, query_ptr=None, dtype=np.float32):
    """(dist2 [Q], face int64 [Q] into tri, closest [Q,3]) in `dtype`: triangles in ascending order, a candidate replaces the best
    only when d2 < best; no triangle taken: +inf, -1, the query."""
    p = np.asarray(points, dtype=np.float32)
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    Q = p.shape[0]
    best = np.full(Q, np.inf, dtype)
    face = np.full(Q, -1, np.int64)
    close = p.astype(dtype).copy()
    for t_lo, t_hi, q_lo, q_hi in _spans(tri_ptr, query_ptr, tri.shape[0], Q):
        if q_hi <= q_lo:
            continue
        rows = np.arange(q_hi - q_lo)
        for t0 in range(t_lo, t_hi, CHUNK):
            d2, c = closest_block(p[q_lo:q_hi], tri[t0:min(t0 + CHUNK, t_hi)], dtype)
            cand = np.where(np.isnan(d2), np.inf, d2)
            j = np.argmin(cand, axis=1)                      # the first of the smallest: what ascending strict "<" keeps
            dj = cand[rows, j]
            take = dj < best[q_lo:q_hi]
            sel = np.nonzero(take)[0] + q_lo
            best[sel], face[sel] = dj[take], t0 + j[take]
            for k in range(3):
                close[sel, k] = np.broadcast_to(c[k], d2.shape)[rows, j][take]
    return best, face, close


def dist2_matrix(points, tri, dtype=np.float64):
    """[Q,T]: the squared distance of every pair (one mesh), NaN where the contract's arithmetic gives NaN."""
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    return np.concatenate([closest_block(points, tri[t0:t0 + CHUNK], dtype)[0] for t0 in range(0, tri.shape[0], CHUNK)], axis=1)


def winding_restated(points, tri, tri_ptr=None, query_ptr=None, dtype=np.float32):
    """[Q]: float32 terms summed in float64 in ascending order, over 4 pi, rounded once to float32 (dtype float32); or everything
    in float64, not rounded (dtype float64)."""
    p = np.asarray(points, dtype=np.float32)
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    total = np.zeros(p.shape[0], np.float64)
    for t_lo, t_hi, q_lo, q_hi in _spans(tri_ptr, query_ptr, tri.shape[0], p.shape[0]):
        if q_hi <= q_lo:
            continue
        for t0 in range(t_lo, t_hi, CHUNK):
            om = omega_block(p[q_lo:q_hi], tri[t0:min(t0 + CHUNK, t_hi)], dtype).astype(np.float64)
            total[q_lo:q_hi] = np.cumsum(np.concatenate([total[q_lo:q_hi, None], om], axis=1), axis=1)[:, -1]      # sequential
    w = total / FOUR_PI
    return w.astype(np.float32) if np.dtype(dtype) == np.float32 else w


# ---- figures -------------------------------------------------------------------------------------------------------------------
def rel_l2(x, ref):
    """|x - ref| / |ref| over the entries finite on both sides."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = np.isfinite(x) & np.isfinite(ref)
    return float(np.sqrt(((x[ok] - ref[ok]) ** 2).sum() / max((ref[ok] ** 2).sum(), 1e-300)))


def max_abs(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = np.isfinite(x) & np.isfinite(ref)
    return float(np.abs(x[ok] - ref[ok]).max()) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def case_closest(name, which, dtype):
    """The restatement on a case (the CSRs of the batch included), computed once: (dist2, face, closest)."""
    tri, tri_ptr, _ = case_triangles(name)
    p, pm = queries(name, which)
    return closest_restated(p, tri, tri_ptr, ptr_of(pm, n_meshes(name)), dtype)


@functools.lru_cache(maxsize=None)
def case_winding(name, dtype):
    tri, tri_ptr, _ = case_triangles(name)
    p, pm = queries(name, "lattice")
    return winding_restated(p, tri, tri_ptr, ptr_of(pm, n_meshes(name)), dtype)


def closest_units(name, which):
    """(rel-L2 of closest, rel-L2 of sqrt(dist2)) of the float32 restatement from the float64 one."""
    d32, _, c32 = case_closest(name, which, np.float32)
    d64, _, c64 = case_closest(name, which, np.float64)
    return rel_l2(c32, c64), rel_l2(np.sqrt(d32.astype(np.float64)), np.sqrt(d64))


def winding_unit(name):
    return max_abs(case_winding(name, np.float32), case_winding(name, np.float64))


def surface_distance64(points, name):
    """float64 [Q]: the distance of each point (of mesh point_mesh, grouped) to the surface of a case."""
    tri, tri_ptr, _ = case_triangles(name)
    p, pm = points
    return np.sqrt(closest_restated(p, tri, tri_ptr, ptr_of(pm, n_meshes(name)), np.float64)[0])


# ---- remeshing with re-projection --------------------------------------------------------------------------------------------------
def remesh_with_projection_restated(verts, faces, *, iters=3, target_len=None, target_scale=1.0, relax=0.5, flip_angle=30.0,
                                    vert_mesh=None, project=True):
    """`postprocess.remesh(project=...)` by the two contracts: the passes of remesh_cases in the order of `remesh_restated`, and at
    the end of every iteration, after the relax, every vertex replaced by its closest point on the input surface of its mesh."""
    x, f = np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int64)
    vm = np.zeros(x.shape[0], np.int32) if vert_mesh is None else np.asarray(vert_mesh, dtype=np.int32)
    M = int(vm.max()) + 1 if vm.size else 1
    base = rm.default_target(x, f, vm, M) if target_len is None else np.broadcast_to(np.asarray(target_len, dtype=np.float32), (M,))
    target = (base.astype(np.float64) * float(target_scale)).astype(np.float32)
    lo2, hi2 = rm.bands(target)
    cos2 = rm.cos2_of(flip_angle)
    ref_tri, ref_ptr, _ = gather(x, f, vm)
    info = []
    for _ in range(int(iters)):
        rec = dict(splits=0, collapses=0, flips=0, collapse_rounds=0, flip_rounds=0)
        x, f, vm, rec["splits"] = rm.split_restated(x, f, vm, hi2)
        for _r in range(rm.COLLAPSE_ROUNDS):
            x, f, vm, n = rm.collapse_round_restated(x, f, vm, lo2, hi2)
            rec["collapse_rounds"] += 1
            rec["collapses"] += n
            if n == 0:
                break
        for _r in range(rm.FLIP_ROUNDS):
            f, n = rm.flip_round_restated(x, f, cos2)
            rec["flip_rounds"] += 1
            rec["flips"] += n
            if n == 0:
                break
        if relax != 0:
            x = rm.relax_restated(x, f, relax, np.float32)
        if project:
            d2, _, x = closest_restated(x, ref_tri, ref_ptr, ptr_of(vm, M), np.float32)
            rec["max_project_dist2"] = float(d2.max()) if d2.size else 0.0
        info.append(rec)
    return x, f, vm, dict(target=target, iterations=info)


@functools.lru_cache(maxsize=None)
def project_restated(name, project):
    v, f = rm.mesh(name)
    return remesh_with_projection_restated(v.numpy(), f.numpy(), iters=PROJECT_ITERS, relax=0.5, vert_mesh=rm.vert_mesh(name).numpy(),
                                           project=project)


def project_figures(name, x, f, vm, target):
    """(share of edges in the band, minimum angle, mean and maximum float64 distance of the vertices to the input surface); the
    quality figures are those of the first mesh of a batch against its own target."""
    first = np.asarray(vm) == 0
    nf = first[np.asarray(f)[:, 0]]
    share, angle = rm.quality(np.asarray(x)[first], np.asarray(f)[nf], float(target[0]))
    d = surface_distance64((np.asarray(x, dtype=np.float32), np.asarray(vm, dtype=np.int32)), name)
    return share, angle, float(d.mean()), float(d.max())
