"""Distance from points to triangle meshes on MI355X -- host side of csrc/meshdist.hip: closest point, generalised winding number
and the signed distance made of the two, batched over the meshes of `postprocess.concat_meshes`.

Meshes: verts float32 [V,3], faces int64 [F,3] of global ids, optional ascending vert_mesh int [V] (None: one mesh).  Queries:
points float32 [Q,3] with an optional ascending point_mesh int [Q] (None: one mesh, which then must be the only one).  A query looks
at the faces of its own mesh only; a face belongs to the mesh of its first vertex.  The arithmetic is the mesh distance contract in
the header comment of csrc/meshdist.hip; this module gathers verts[faces], builds the two CSRs the kernel reads and maps the face
index back.  GPU only: a CPU tensor is an error, not a fallback.  Everything runs under no_grad and writes none of its inputs.
Nothing here has a gradient: the results are detached.
"""
import torch

from . import _lib
from ._csr import INT32_MAX, check_faces
from .hip_ops import _gpu_only, call


def _mesh_ids(ids, n, dev, what, name):
    if ids is None:
        return torch.zeros(n, dtype=torch.int64, device=dev)
    ids = ids.to(device=dev, dtype=torch.int64)
    if tuple(ids.shape) != (n,) or (n > 0 and (int(ids.min()) < 0 or bool((ids[1:] < ids[:-1]).any()))):
        raise ValueError(f"{what}: expected {name} [{n}] of ascending mesh numbers >= 0")
    return ids


def _ptr(ids, M):
    return torch.searchsorted(ids, torch.arange(M + 1, dtype=torch.int64, device=ids.device)).to(torch.int32).contiguous()


def mesh_triangles(verts, faces, vert_mesh=None, what="mesh_triangles"):
    """The reference surface the kernel reads: (tri float32 [F,3,3] grouped by mesh, tri_ptr int32 [M+1], face_of int64 [F] or
    None, M).  tri[k] = verts[faces[face_of[k]]]; face_of is None when the faces were already grouped by ascending mesh, else the
    stable sort by mesh.  Checks shapes, dtypes, index range and ordering on the host."""
    _gpu_only(verts, what)
    if verts.dim() != 2 or verts.shape[-1] != 3 or not verts.is_floating_point():
        raise ValueError(f"{what}: expected floating-point verts [V,3], got {verts.dtype} {tuple(verts.shape)}")
    x = verts.detach().to(torch.float32).contiguous()
    V, dev = x.shape[0], x.device

    def limits(F):
        if V > INT32_MAX or F > INT32_MAX:
            raise _lib.MeshDiffusionHipError(f"{what}: V and F must fit int32 (MD_ERR_UNSUPPORTED)")
    f = check_faces(faces.to(dev), V, what, limits)
    vm = _mesh_ids(vert_mesh, V, dev, what, "vert_mesh")
    M = int(vm[-1]) + 1 if V > 0 else 1
    if M > _lib.MESHDIST_MAX_MESHES:
        raise _lib.MeshDiffusionHipError(f"{what}: at most {_lib.MESHDIST_MAX_MESHES} meshes (MD_ERR_UNSUPPORTED)")
    fm = vm[f[:, 0]] if f.shape[0] > 0 else vm[:0]
    face_of = None
    if f.shape[0] > 1 and bool((fm[1:] < fm[:-1]).any()):
        fm, face_of = torch.sort(fm, stable=True)
        f = f[face_of]
    return x[f].contiguous(), _ptr(fm, M), face_of, M


def mesh_query(points, tri, tri_ptr, face_of, M, point_mesh, what, want_closest, want_winding):
    """One launch of md_mesh_query against the surface `mesh_triangles` built: (dist2, face int64, closest, winding), the ones not
    asked for None.  What `closest_point`, `winding_number` and `signed_distance` are made of, and what `postprocess.remesh` calls
    once per iteration against the surface it kept."""
    _gpu_only(points, what)
    if points.dim() != 2 or points.shape[-1] != 3 or not points.is_floating_point():
        raise ValueError(f"{what}: expected floating-point points [Q,3], got {points.dtype} {tuple(points.shape)}")
    if points.device != tri.device:
        raise ValueError(f"{what}: points and the mesh must be on the same device")
    p = points.detach().to(torch.float32).contiguous()
    Q, dev = p.shape[0], p.device
    if Q > INT32_MAX:
        raise _lib.MeshDiffusionHipError(f"{what}: Q must fit int32 (MD_ERR_UNSUPPORTED)")
    pm = _mesh_ids(point_mesh, Q, dev, what, "point_mesh")
    if Q > 0 and int(pm[-1]) >= M:
        raise ValueError(f"{what}: point_mesh names mesh {int(pm[-1])} of {M}")
    dist2 = face = closest = winding = None
    if want_closest:
        dist2 = torch.empty(Q, dtype=torch.float32, device=dev)
        face = torch.empty(Q, dtype=torch.int32, device=dev)
        closest = torch.empty(Q, 3, dtype=torch.float32, device=dev)
    if want_winding:
        winding = torch.empty(Q, dtype=torch.float32, device=dev)
    if Q > 0:
        call("md_mesh_query", tri if tri.shape[0] > 0 else None, tri_ptr, p, _ptr(pm, M), tri.shape[0], Q, M, dist2, face, closest, winding)
    if want_closest:
        face = face.to(torch.int64)
        if face_of is not None:
            face = torch.where(face >= 0, face_of[face.clamp_min(0)], face)
    return dist2, face, closest, winding


@torch.no_grad()
def closest_point(points, verts, faces, *, point_mesh=None, vert_mesh=None):
    """(dist2 float32 [Q], face int64 [Q], closest float32 [Q,3]): for every point the closest point on the faces of its mesh, the
    squared distance to it and the index of the face in the caller's `faces` (ties: the lowest index in mesh order).  A point whose
    mesh has no face, or whose every candidate is NaN, gets (+inf, -1, the point).  Faces that are not grouped by mesh are sorted
    stably by mesh first and the index is mapped back."""
    tri, tri_ptr, face_of, M = mesh_triangles(verts, faces, vert_mesh, "closest_point")
    return mesh_query(points, tri, tri_ptr, face_of, M, point_mesh, "closest_point", True, False)[:3]


@torch.no_grad()
def winding_number(points, verts, faces, *, point_mesh=None, vert_mesh=None):
    """float32 [Q]: the generalised winding number of every point's mesh at the point: +1 inside a closed mesh whose faces wind
    outward (counter-clockwise seen from outside), -1 inside one that winds inward, 0 outside, fractions near an open boundary."""
    tri, tri_ptr, face_of, M = mesh_triangles(verts, faces, vert_mesh, "winding_number")
    return mesh_query(points, tri, tri_ptr, face_of, M, point_mesh, "winding_number", False, True)[3]


@torch.no_grad()
def signed_distance(points, verts, faces, *, threshold=0.5, point_mesh=None, vert_mesh=None):
    """(sdf float32 [Q], face int64 [Q], closest float32 [Q,3]) in one launch: sdf = sqrt(dist2), positive where |winding| >=
    threshold (inside: the sign convention of the DMTet grids) and negative elsewhere.  |winding|, not winding: a mesh whose faces
    all wind inward gives the same field.  A NaN winding number counts as outside."""
    threshold = float(threshold)
    if not 0.0 < threshold < 1.0:
        raise ValueError(f"signed_distance: threshold must be in (0, 1), got {threshold}")
    tri, tri_ptr, face_of, M = mesh_triangles(verts, faces, vert_mesh, "signed_distance")
    dist2, face, closest, winding = mesh_query(points, tri, tri_ptr, face_of, M, point_mesh, "signed_distance", True, True)
    dist = torch.sqrt(dist2.to(torch.float64)).to(torch.float32)                # the correctly rounded fp32 root
    return torch.where(winding.abs() >= threshold, dist, -dist), face, closest


@torch.no_grad()
def init_sdf(geo, verts, faces):
    """The warm start of a DMTet fit: geo.sdf <- the signed distance of the mesh (verts, faces) at geo.verts, clamped to [-1, 1]
    (the range `--sphere_init` uses).  `geo` is a dmtet.DMTetGeometry; returns the tensor written."""
    sdf = signed_distance(geo.verts, verts, faces)[0].clamp(-1.0, 1.0)
    geo.sdf.copy_(sdf.to(geo.sdf.dtype))
    return sdf
