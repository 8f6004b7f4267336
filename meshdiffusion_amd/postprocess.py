"""Clean-up of generated meshes on MI355X -- host side of csrc/meshpost.hip: connected components with a floater filter and
umbrella (Laplacian / Taubin) smoothing, batched over the meshes of one marching-tetrahedra launch.

The reference cleans each sampled mesh with pymeshlab at the end of nvdiffrec/eval.py (:449-456: isotropic remeshing and
`apply_coord_laplacian_smoothing(stepsmoothnum=--num_smooth_steps)`).  This module is built in the manner of that step under the
mesh post-processing contract in the header comment of csrc/meshpost.hip, not bit-equal to MeshLab: uniform (umbrella) weights, a
filter for the small disconnected shells that the sign noise of a sampled SDF leaves behind, and `remesh`, the isotropic remeshing
(split, collapse, flip, relax) of the remeshing contract in the header comment of csrc/remesh.hip -- with re-projection onto the
input surface on request (`project=True`, the closest point of csrc/meshdist.hip), without feature edges, adaptive sizing or
cotangent weights.  The kernels run on the GPU only: a CPU tensor is an error, not a fallback.  The edge table, the compaction and
the split / concat of a batch are torch plumbing.  Nothing here has a gradient: it runs after generation, not inside a fit.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, meshdist
from ._csr import INT32_MAX, check_faces, csr_by_row
from .hip_ops import _gpu_only, call


def _check_faces(faces, n_verts, what):
    """faces [F,3] -> int64 contiguous, every index in [0, n_verts): checked once, the kernels treat anything else as absent."""
    def limits(F):
        if n_verts < 0:
            raise ValueError(f"{what}: n_verts must not be negative, got {n_verts}")
        if n_verts > INT32_MAX or 3 * F > INT32_MAX:
            raise _lib.MeshDiffusionHipError(f"{what}: V and 3 F must fit int32 (MD_ERR_UNSUPPORTED)")
    return check_faces(faces, n_verts, what, limits)


def mesh_edges(faces, n_verts):
    """The edge table of the contract: (lo int64 [E], hi int64 [E], mult int64 [E], ptr int32 [V+1], adj int32 [2 E]).  The 3 F
    corner edges (faces[f][(k+1)%3], faces[f][(k+2)%3]) without those of a == b, keyed min * V + max, sorted stably and uniqued;
    mult = the number of corner edges of a key, 1 on a boundary edge.  (ptr, adj) is the neighbour CSR with the codes
    2 * neighbour + (1 if mult == 1), ascending by neighbour inside a row.  Torch plumbing."""
    _gpu_only(faces, "mesh_edges")
    V = int(n_verts)
    f = _check_faces(faces, V, "mesh_edges")
    if 2 * V > INT32_MAX:
        raise _lib.MeshDiffusionHipError("mesh_edges: the codes 2 * neighbour + 1 must fit int32 (MD_ERR_UNSUPPORTED)")
    a, b = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    keep = a != b
    keys = (torch.minimum(a, b) * V + torch.maximum(a, b))[keep]
    keys = torch.sort(keys, stable=True).values
    keys, mult = torch.unique_consecutive(keys, return_counts=True)
    E = keys.shape[0]
    if 2 * E > INT32_MAX:
        raise _lib.MeshDiffusionHipError("mesh_edges: 2 E must fit int32 (MD_ERR_UNSUPPORTED)")
    lo, hi = torch.div(keys, max(V, 1), rounding_mode="floor"), keys % max(V, 1)
    bnd = (mult == 1).to(torch.int64)
    # row hi first: its neighbour lo is below it, so a stable sort by row leaves every row ascending by neighbour
    ptr, order = csr_by_row(torch.cat([hi, lo]), V)
    adj = (2 * torch.cat([lo, hi]) + torch.cat([bnd, bnd]))[order.to(torch.int64)].to(torch.int32).contiguous()
    return lo, hi, mult, ptr, adj


def smooth(verts, faces, steps=3, lam=0.5, mu=None, edges=None):
    """`steps` umbrella steps of the contract on verts float32 [V,3], faces [F,3]: a new tensor, `verts` is never written.
    Step i moves every vertex by w (mean of its neighbours - itself), w = lam for even i or without mu, else mu (Taubin's
    lambda | mu, e.g. 0.5 / -0.53, which does not shrink); a boundary vertex averages its boundary neighbours only, a vertex
    without neighbours keeps its bits.  edges: the prebuilt `mesh_edges(faces, V)`.  One C call issues every step; two runs agree
    bit for bit."""
    _gpu_only(verts, "smooth")
    if verts.dim() != 2 or verts.shape[-1] != 3:
        raise ValueError(f"smooth: expected verts [V,3], got {tuple(verts.shape)}")
    steps = int(steps)
    if steps < 0:
        raise ValueError(f"smooth: steps must not be negative, got {steps}")
    lam = float(lam)
    mu = float("nan") if mu is None else float(mu)
    if not math.isfinite(lam) or math.isinf(mu):
        raise ValueError("smooth: lam must be finite, mu finite or None")
    x = verts.detach().to(torch.float32).contiguous()
    V = x.shape[0]
    if edges is None:
        edges = mesh_edges(faces.to(x.device), V)
    ptr, adj = edges[3], edges[4]
    if tuple(ptr.shape) != (V + 1,) or ptr.dtype != torch.int32 or adj.dtype != torch.int32:
        raise ValueError(f"smooth: expected the edge table of a mesh of {V} vertices")
    out = torch.empty_like(x)
    if V == 0:
        return out
    if adj.numel() == 0:                                                        # no edge: every vertex keeps its bits
        out.copy_(x)
        return out
    scratch = torch.empty_like(x) if steps >= 2 else None
    call("md_mesh_smooth", x, ptr, adj, V, adj.numel(), steps, lam, mu, out, scratch)
    return out


def components(faces, n_verts):
    """(label int32 [V], comp_faces int32 [V], rounds): label[v] = the smallest vertex index connected to v through faces (a vertex
    no face names is its own component), comp_faces[label] = the number of faces of that component, 0 at every other index, rounds =
    the hook-and-compress rounds the kernel ran (it reads one flag per round, so the call synchronises)."""
    _gpu_only(faces, "components")
    V = int(n_verts)
    f = _check_faces(faces, V, "components")
    dev = f.device
    if V == 0 or f.shape[0] == 0:
        return torch.arange(V, dtype=torch.int32, device=dev), torch.zeros(V, dtype=torch.int32, device=dev), 0
    label = torch.empty(V, dtype=torch.int32, device=dev)
    comp_faces = torch.empty(V, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.MESH_COMPONENTS_WORKSPACE_BYTES // 4, dtype=torch.int32, device=dev)
    rounds = ctypes.c_int32(0)
    call("md_mesh_components", f, V, f.shape[0], label, comp_faces, ws, ctypes.byref(rounds))
    return label, comp_faces, int(rounds.value)


def drop_floaters(verts, faces, *, min_faces=1, min_fraction=0.0, keep_largest=False, vert_mesh=None):
    """Drop the small components of a (concatenated) mesh: (verts', faces', vert_map int64 [V] (-1 = dropped), face_keep bool [F]).
    A component survives iff comp_faces >= max(min_faces, 1, ceil(min_fraction * the largest comp_faces of the same mesh)), and with
    keep_largest only if it is also the largest of its mesh (a tie goes to the smaller label).  vert_mesh int [V] names the mesh of a
    vertex (None: one mesh).  Surviving vertices and faces keep their relative order; an unreferenced vertex, a component of 0
    faces, is always dropped.  The labelling is the kernel's, the compaction torch."""
    _gpu_only(verts, "drop_floaters")
    if verts.dim() != 2 or verts.shape[-1] != 3:
        raise ValueError(f"drop_floaters: expected verts [V,3], got {tuple(verts.shape)}")
    V, dev = verts.shape[0], verts.device
    f = _check_faces(faces.to(dev), V, "drop_floaters")
    if vert_mesh is None:
        vm = torch.zeros(V, dtype=torch.int64, device=dev)
    else:
        vm = vert_mesh.to(device=dev, dtype=torch.int64)
        if tuple(vm.shape) != (V,) or (V > 0 and int(vm.min()) < 0):
            raise ValueError(f"drop_floaters: expected vert_mesh [{V}] of mesh numbers >= 0")
    if V == 0:
        return verts.clone(), f.clone(), torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(f.shape[0], dtype=torch.bool, device=dev)
    label, comp_faces, _ = components(f, V)
    cf = comp_faces.to(torch.int64)
    M = int(vm.max()) + 1
    largest = torch.zeros(M, dtype=torch.int64, device=dev).scatter_reduce(0, vm, cf, "amax", include_self=True)
    need = torch.ceil(float(min_fraction) * largest.to(torch.float64)).to(torch.int64).clamp_min(max(int(min_faces), 1))
    root_ok = cf >= need[vm]
    if keep_largest:
        idx = torch.arange(V, dtype=torch.int64, device=dev)
        cand = torch.where((cf == largest[vm]) & (cf >= 1), idx, torch.full_like(idx, V))
        winner = torch.full((M,), V, dtype=torch.int64, device=dev).scatter_reduce(0, vm, cand, "amin", include_self=True)
        root_ok = root_ok & (idx == winner[vm])
    vert_keep = root_ok[label.to(torch.int64)]
    face_keep = vert_keep[f[:, 0]] if f.shape[0] > 0 else torch.zeros(0, dtype=torch.bool, device=dev)
    vert_map = torch.where(vert_keep, torch.cumsum(vert_keep.to(torch.int64), 0) - 1, torch.full((V,), -1, dtype=torch.int64, device=dev))
    return verts[vert_keep], vert_map[f[face_keep]], vert_map, face_keep


def concat_meshes(meshes):
    """A list of (verts [V_m,3], faces [F_m,3], ...) or a `dmtet.MeshBatch` (each mesh at its trimmed counts) -> the concatenated
    form (verts float32 [V,3], faces int64 [F,3] of global ids, vert_mesh int32 [V])."""
    items = [(m[0], m[1]) for m in meshes]
    if not items:
        raise ValueError("concat_meshes: no meshes")
    dev = items[0][0].device
    vs, fs, vm, base = [], [], [], 0
    for k, (v, f) in enumerate(items):
        vs.append(v.detach().to(torch.float32).reshape(-1, 3))
        fs.append(f.to(torch.int64).reshape(-1, 3) + base)
        vm.append(torch.full((v.shape[0],), k, dtype=torch.int32, device=dev))
        base += v.shape[0]
    return torch.cat(vs).contiguous(), torch.cat(fs).contiguous(), torch.cat(vm)


def split_meshes(verts, faces, vert_mesh, n_meshes):
    """The inverse of `concat_meshes` for a concatenated mesh whose vertices are still grouped by ascending mesh (`drop_floaters`
    keeps the order): a list of `n_meshes` (verts [V_m,3], faces int64 [F_m,3] of local ids).  A face belongs to the mesh of its
    first vertex."""
    vm = vert_mesh.to(torch.int64)
    nv = torch.bincount(vm, minlength=n_meshes)
    fm = vm[faces[:, 0]] if faces.shape[0] > 0 else vm[:0]
    nf = torch.bincount(fm, minlength=n_meshes)
    nv, nf = nv.tolist(), nf.tolist()
    out, v0, f0 = [], 0, 0
    for m in range(n_meshes):
        out.append((verts[v0:v0 + nv[m]], faces[f0:f0 + nf[m]] - v0))
        v0, f0 = v0 + nv[m], f0 + nf[m]
    return out


def _repeated(f):
    return (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])


def _remesh_tables(f, V):
    """The tables of the remeshing contract from the faces of the moment: (lo, hi, mult int64 [E], ptr int32 [V+1], adj int32 [2 E],
    cptr int32 [V+1], corner int32 [3 F], vflag int32 [V]).  Torch plumbing."""
    lo, hi, mult, ptr, adj = mesh_edges(f, V)
    cptr, corner = csr_by_row(f.reshape(-1), V)
    vflag = torch.zeros(V, dtype=torch.int32, device=f.device)
    for sel, bit in ((mult == 1, 1), (mult >= 3, 2)):
        vflag[lo[sel]] |= bit
        vflag[hi[sel]] |= bit
    vflag[f[_repeated(f)].reshape(-1)] |= 2
    return lo.contiguous(), hi.contiguous(), mult.contiguous(), ptr, adj, cptr, corner, vflag


def remesh_default_target(verts, faces, vert_mesh, n_meshes):
    """float32 numpy [M]: the mean edge length of each mesh (1 for a mesh without edges) -- float64 lengths from the fp32
    coordinates on the device, then on the host the sequential float64 sum in table order, so that two runs agree bit for bit."""
    V = verts.shape[0]
    lo, hi, _, _, _ = mesh_edges(faces, V)
    x = verts.to(torch.float64)
    d = x[hi] - x[lo]
    ln = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).cpu().numpy()
    em = vert_mesh.to(torch.int64)[lo].cpu().numpy()
    s = np.bincount(em, weights=ln, minlength=n_meshes)
    n = np.bincount(em, minlength=n_meshes)
    return np.where(n > 0, s / np.maximum(n, 1), 1.0).astype(np.float32)


def remesh_split(x, f, vm, hi2):
    """One split pass of the remeshing contract on checked device tensors: (verts', faces', vert_mesh', marked edges)."""
    V, F, M, dev = x.shape[0], f.shape[0], hi2.shape[0], x.device
    lo, hi, mult, ptr, adj, cptr, corner, vflag = _remesh_tables(f, V)
    E = lo.shape[0]
    if E == 0:
        return x, f, vm, 0
    mark = torch.empty(E, dtype=torch.int32, device=dev)
    mid = torch.empty(E, 3, dtype=torch.float32, device=dev)
    call("md_remesh_split_mark", x, lo, hi, vm, hi2, V, E, M, mark, mid)
    n = int(mark.sum())
    if n == 0:
        return x, f, vm, 0
    if V + n > INT32_MAX:
        raise _lib.MeshDiffusionHipError("remesh: V must fit int32 after the split (MD_ERR_UNSUPPORTED)")
    rank = (torch.cumsum(mark, 0) - mark).to(torch.int32)
    count = torch.empty(F, dtype=torch.int32, device=dev)
    call("md_remesh_split_count", f, lo, hi, mark, V, E, F, count)
    total = torch.cumsum(count.to(torch.int64), 0)
    F_out = int(total[-1])
    if 3 * F_out > INT32_MAX:
        raise _lib.MeshDiffusionHipError("remesh: 3 F must fit int32 after the split (MD_ERR_UNSUPPORTED)")
    offset = (total - count).to(torch.int32)
    out = torch.empty(F_out, 3, dtype=torch.int64, device=dev)
    call("md_remesh_split_emit", x, f, lo, hi, mark, rank, offset, V, E, F, F_out, out)
    sel = mark.bool()
    x2, vm2 = torch.cat([x, mid[sel]]), torch.cat([vm, vm[lo[sel]]])
    if M > 1:                                                                    # vertices stay grouped by mesh
        order = torch.sort(vm2, stable=True).indices
        inv = torch.empty_like(order)
        inv[order] = torch.arange(order.shape[0], device=dev)
        x2, vm2, out = x2[order], vm2[order], inv[out]
    return x2.contiguous(), out.contiguous(), vm2.contiguous(), n


def remesh_collapse_round(x, f, vm, lo2, hi2):
    """One collapse round of the remeshing contract: (verts', faces', vert_mesh', winners).  `x` is not written."""
    V, F, M, dev = x.shape[0], f.shape[0], hi2.shape[0], x.device
    lo, hi, mult, ptr, adj, cptr, corner, vflag = _remesh_tables(f, V)
    E = lo.shape[0]
    if E == 0:
        return x, f, vm, 0
    cand = torch.empty(E, dtype=torch.int32, device=dev)
    prio = torch.empty(E, dtype=torch.int64, device=dev)
    word = torch.full((V,), -1, dtype=torch.int64, device=dev)                  # all ones
    remap = torch.arange(V, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    new = x.clone()
    call("md_remesh_collapse_candidates", x, f, lo, hi, mult, ptr, adj, cptr, corner, vflag, vm, lo2, hi2, V, E, F, M, cand, prio)
    call("md_remesh_collapse_claim", lo, hi, ptr, adj, cand, prio, V, E, word)
    call("md_remesh_collapse_apply", lo, hi, ptr, adj, cand, prio, word, V, E, new, remap, counter)
    n = int(counter)                                                            # the one 4-byte copy of a round
    if n == 0:
        return x, f, vm, 0
    remap = remap.to(torch.int64)
    f2 = remap[f]
    f2 = f2[~_repeated(f2) | _repeated(f)]
    keep = remap == torch.arange(V, device=dev)
    newid = torch.cumsum(keep.to(torch.int64), 0) - 1
    return new[keep].contiguous(), newid[f2].contiguous(), vm[keep].contiguous(), n


def remesh_flip_round(x, f, cos2):
    """One flip round of the remeshing contract: (faces', winners).  `f` is not written."""
    V, F, dev = x.shape[0], f.shape[0], x.device
    lo, hi, mult, ptr, adj, cptr, corner, vflag = _remesh_tables(f, V)
    E = lo.shape[0]
    if E == 0:
        return f, 0
    cand = torch.empty(E, dtype=torch.int32, device=dev)
    prio = torch.empty(E, dtype=torch.int64, device=dev)
    info = torch.empty(E, 4, dtype=torch.int32, device=dev)
    word = torch.full((V,), -1, dtype=torch.int64, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    out = f.clone()
    call("md_remesh_flip_candidates", x, f, lo, hi, mult, ptr, cptr, corner, vflag, float(cos2), V, E, F, cand, prio, info)
    call("md_remesh_flip_claim", lo, hi, cand, prio, info, V, E, word)
    call("md_remesh_flip_apply", lo, hi, cand, prio, info, word, V, E, F, out, counter)
    n = int(counter)
    return (out if n else f), n


def remesh_relax(x, f, lam=0.5):
    """The relax pass of the remeshing contract: a new tensor."""
    V, F = x.shape[0], f.shape[0]
    lo, hi, mult, ptr, adj, cptr, corner, vflag = _remesh_tables(f, V)
    E = lo.shape[0]
    if E == 0:
        return x.clone()
    out = torch.empty_like(x)
    call("md_remesh_relax", x, f, ptr, adj, cptr, corner, vflag, V, E, F, float(lam), out)
    return out


def remesh_bands(target):
    """(lo2, hi2) float32 numpy [M] of float32 targets: (4/5 L)^2 and (4/3 L)^2 in float64, rounded once."""
    t = np.asarray(target, dtype=np.float32).astype(np.float64)
    return ((0.8 * t) ** 2).astype(np.float32), ((4.0 / 3.0 * t) ** 2).astype(np.float32)


def remesh(verts, faces, *, iters=3, target_len=None, target_scale=1.0, relax=0.5, flip_angle=30.0, vert_mesh=None, project=False):
    """Isotropic remeshing of a (concatenated) mesh by the remeshing contract (csrc/remesh.hip): `iters` iterations of split (edges
    longer than 4/3 L), collapse (shorter than 4/5 L), flip (towards valence six) and tangential relaxation (weight `relax`, 0 = off).
    L per mesh = (target_len float or [M], default the mesh's own mean edge length) * target_scale.  vert_mesh int [V] names the mesh
    of a vertex (None: one mesh), ascending.  Returns (verts' float32 [V',3], faces' int64 [F',3], vert_mesh' int32 [V'], info) with
    info = dict(target float32 numpy [M], iterations = [dict(splits, collapses, flips, collapse_rounds, flip_rounds), ...]).  GPU
    only; the inputs are never written; two runs agree bit for bit.  Reaching a round cap is not an error.
    project=True keeps the checked input of this call as the reference surface and ends every iteration, after the relax, by
    replacing every vertex with the closest point on the reference surface of its own mesh (the mesh distance contract of
    csrc/meshdist.hip; a vertex whose mesh has no face stays); each iteration's record gains max_project_dist2, the largest squared
    distance a vertex was moved by.  Without it the result is what it was before the flag existed, bit for bit."""
    _gpu_only(verts, "remesh")
    if verts.dim() != 2 or verts.shape[-1] != 3:
        raise ValueError(f"remesh: expected verts [V,3], got {tuple(verts.shape)}")
    iters = int(iters)
    if iters < 0 or iters > _lib.REMESH_MAX_ITERS:
        raise ValueError(f"remesh: iters must be in [0, {_lib.REMESH_MAX_ITERS}], got {iters}")
    relax, flip_angle, target_scale = float(relax), float(flip_angle), float(target_scale)
    if not math.isfinite(relax) or not 0.0 <= flip_angle <= 90.0 or not (math.isfinite(target_scale) and target_scale > 0):
        raise ValueError("remesh: relax must be finite, flip_angle in [0, 90] degrees, target_scale finite and > 0")
    dev = verts.device
    x = verts.detach().to(torch.float32).contiguous().clone()
    V = x.shape[0]
    f = _check_faces(faces.to(dev), V, "remesh").clone()
    if vert_mesh is None:
        vm = torch.zeros(V, dtype=torch.int32, device=dev)
    else:
        vm = vert_mesh.to(device=dev, dtype=torch.int32).contiguous().clone()
        if tuple(vm.shape) != (V,) or (V > 1 and (int(vm.min()) < 0 or bool((vm[1:] < vm[:-1]).any()))):
            raise ValueError(f"remesh: expected vert_mesh [{V}] of ascending mesh numbers >= 0")
    M = int(vm.max()) + 1 if V > 0 else 1
    if target_len is None:
        base = remesh_default_target(x, f, vm, M) if V > 0 and f.shape[0] > 0 else np.ones(M, np.float32)
    else:
        t = target_len.detach().cpu().numpy() if torch.is_tensor(target_len) else np.asarray(target_len)
        if t.ndim > 1 or (t.ndim == 1 and t.shape[0] != M):
            raise ValueError(f"remesh: expected one target length or [{M}], got {t.shape}")
        base = np.broadcast_to(t.astype(np.float32), (M,))
    target = (base.astype(np.float64) * target_scale).astype(np.float32)
    if not (np.isfinite(target).all() and (target > 0).all()):
        raise ValueError("remesh: every target length must be finite and > 0")
    lo2, hi2 = (torch.as_tensor(a, device=dev) for a in remesh_bands(target))
    cos2 = float(np.float32(math.cos(math.radians(flip_angle)) ** 2))
    if project:
        ref_tri, ref_ptr, _, _ = meshdist.mesh_triangles(x, f, vm, "remesh")
    info = []
    for _ in range(iters if V > 0 and f.shape[0] > 0 else 0):
        rec = dict(splits=0, collapses=0, flips=0, collapse_rounds=0, flip_rounds=0)
        x, f, vm, rec["splits"] = remesh_split(x, f, vm, hi2)
        for _r in range(_lib.REMESH_COLLAPSE_ROUNDS):
            x, f, vm, n = remesh_collapse_round(x, f, vm, lo2, hi2)
            rec["collapse_rounds"] += 1
            rec["collapses"] += n
            if n == 0:
                break
        for _r in range(_lib.REMESH_FLIP_ROUNDS):
            f, n = remesh_flip_round(x, f, cos2)
            rec["flip_rounds"] += 1
            rec["flips"] += n
            if n == 0:
                break
        if relax != 0.0:
            x = remesh_relax(x, f, relax)
        if project:
            d2, _, x, _ = meshdist.mesh_query(x, ref_tri, ref_ptr, None, M, vm, "remesh", True, False)
            rec["max_project_dist2"] = float(d2.max()) if d2.numel() > 0 else 0.0
        info.append(rec)
    return x, f, vm, dict(target=target, iterations=info)


def postprocess(meshes, *, smooth_steps=0, lam=0.5, mu=None, min_component_faces=0, min_component_fraction=0.0, keep_largest=False,
                remesh_iters=0, remesh_target_scale=1.0, remesh_project=False):
    """The clean-up of a whole batch (a list of (verts, faces, ...) or a `dmtet.MeshBatch`) in one set of launches, in the
    reference's order: the floater filter first (when min_component_faces > 0, min_component_fraction > 0 or keep_largest), then,
    with remesh_iters > 0, `remesh`, then `smooth_steps` smoothing steps, then `remesh` again (remesh_project: each of the two
    with project=True, onto its own input).
    Returns a list of (verts float32 [V_m,3], faces int64 [F_m,3]).  With every keyword at its default the meshes come back as they
    are."""
    verts, faces, vert_mesh = concat_meshes(meshes)
    _gpu_only(verts, "postprocess")
    n = int(vert_mesh[-1]) + 1 if vert_mesh.numel() > 0 else 0
    n = max(n, len(meshes))
    if min_component_faces > 0 or min_component_fraction > 0 or keep_largest:
        verts, faces, vert_map, _ = drop_floaters(verts, faces, min_faces=min_component_faces, min_fraction=min_component_fraction,
                                                  keep_largest=keep_largest, vert_mesh=vert_mesh)
        vert_mesh = vert_mesh[vert_map >= 0]
    if remesh_iters > 0 and verts.shape[0] > 0:
        verts, faces, vert_mesh, _ = remesh(verts, faces, iters=remesh_iters, target_scale=remesh_target_scale, vert_mesh=vert_mesh,
                                            project=remesh_project)
    if smooth_steps > 0 and verts.shape[0] > 0:
        verts = smooth(verts, faces, smooth_steps, lam, mu)
    if remesh_iters > 0 and verts.shape[0] > 0:
        verts, faces, vert_mesh, _ = remesh(verts, faces, iters=remesh_iters, target_scale=remesh_target_scale, vert_mesh=vert_mesh,
                                            project=remesh_project)
    return split_meshes(verts, faces, vert_mesh, n)
