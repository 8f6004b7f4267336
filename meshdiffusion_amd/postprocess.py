"""Clean-up of generated meshes on MI355X -- host side of csrc/meshpost.hip: connected components with a floater filter and
umbrella (Laplacian / Taubin) smoothing, batched over the meshes of one marching-tetrahedra launch.

The reference cleans each sampled mesh with pymeshlab at the end of nvdiffrec/eval.py (:449-456: isotropic remeshing and
`apply_coord_laplacian_smoothing(stepsmoothnum=--num_smooth_steps)`).  This module is built in the manner of that step under the
mesh post-processing contract in the header comment of csrc/meshpost.hip, not bit-equal to MeshLab: no remeshing, uniform
(umbrella) weights, and a filter for the small disconnected shells that the sign noise of a sampled SDF leaves behind.  The
kernels run on the GPU only: a CPU tensor is an error, not a fallback.  The edge table, the compaction and the split / concat of a
batch are torch plumbing.  Nothing here has a gradient: it runs after generation, not inside a fit.
"""
import ctypes
import math

import torch

from . import _lib
from ._csr import INT32_MAX, csr_by_row
from .hip_ops import _ptr, _stream


def _gpu_only(t, what):
    if not t.is_cuda:
        raise _lib.MeshDiffusionHipError(f"{what} runs on the GPU only (no CPU fallback)")


def _check_faces(faces, n_verts, what):
    """faces [F,3] -> int64 contiguous, every index in [0, n_verts): checked once, the kernels treat anything else as absent."""
    if faces.dim() != 2 or faces.shape[-1] != 3:
        raise ValueError(f"{what}: expected faces [F,3], got {tuple(faces.shape)}")
    n_verts = int(n_verts)
    if n_verts < 0:
        raise ValueError(f"{what}: n_verts must not be negative, got {n_verts}")
    if n_verts > INT32_MAX or 3 * faces.shape[0] > INT32_MAX:
        raise _lib.MeshDiffusionHipError(f"{what}: V and 3 F must fit int32 (MD_ERR_UNSUPPORTED)")
    f = faces.to(torch.int64).contiguous()
    if f.shape[0] > 0:
        lo, hi = torch.aminmax(f)
        if int(lo) < 0 or int(hi) >= n_verts:
            raise ValueError(f"{what}: faces name vertices outside [0, {n_verts})")
    return f


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
    _lib.check(_lib.load().md_mesh_smooth(_ptr(x), _ptr(ptr), _ptr(adj), V, adj.numel(), steps, lam, mu, _ptr(out), _ptr(scratch),
                                          _stream()), "md_mesh_smooth")
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
    _lib.check(_lib.load().md_mesh_components(_ptr(f), V, f.shape[0], _ptr(label), _ptr(comp_faces), _ptr(ws), ctypes.byref(rounds),
                                              _stream()), "md_mesh_components")
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


def postprocess(meshes, *, smooth_steps=0, lam=0.5, mu=None, min_component_faces=0, min_component_fraction=0.0, keep_largest=False):
    """The clean-up of a whole batch (a list of (verts, faces, ...) or a `dmtet.MeshBatch`) in one set of launches: the floater
    filter first (when min_component_faces > 0, min_component_fraction > 0 or keep_largest), then `smooth_steps` smoothing steps.
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
    if smooth_steps > 0 and verts.shape[0] > 0:
        verts = smooth(verts, faces, smooth_steps, lam, mu)
    return split_meshes(verts, faces, vert_mesh, n)
