"""Point-cloud supervision on MI355X -- host side of csrc/pointcloud.hip.

The reference's fitting step adds one loss that needs no renderer (nvdiffrec/lib/geometry/dmtet.py:454-459):

    pred_points = kaolin.ops.mesh.sample_points(imesh.v_pos[None], imesh.t_pos_idx, 50000)[0][0]
    chamfer     = kaolin.metrics.pointcloud.chamfer_distance(pred_points[None], target['spts'][None]).mean()

`sample_points` has the signature and return shapes of the reference's pure-torch copy (geometry/utils.py:55),
`chamfer_distance` / `sided_distance` those of kaolin.metrics.pointcloud.  The loop around them, `fit_to_points` (the geometry
part of `DMTetGeometry.tick`: chamfer + the SDF regulariser with its schedule, `sdf_regularizer_weight`), lives with the other
fits in fit.py and is still found here by name.  Everything runs on the GPU only: a CPU tensor is an
error, not a fallback.  Gradients are gathers over a CSR built with torch ops on the device (stable sort of the dynamic
indices); the summation is the kernel, so two backward passes agree bit for bit.
"""
import torch

from . import _lib
from ._csr import check_faces, csr_by_row
from .hip_ops import _gpu_only, call


def _cloud(t, what):
    _gpu_only(t, what)
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: expected a [B,N,3] point cloud with B, N >= 1, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _nn(p, q, skip_same_index=False):
    """p [B,N,3], q [B,M,3] float32 contiguous on the GPU -> (dist2 float32 [B,N], idx int64 [B,N]): md_nn_sided."""
    lib = _lib.load()
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    if q.shape[0] != B or q.device != p.device:
        raise ValueError("sided distance: both clouds need the same batch size and device")
    ws_bytes = lib.md_nn_sided_workspace_bytes(B, N, M)
    if ws_bytes < 0:
        raise _lib.MeshDiffusionHipError(f"md_nn_sided_workspace_bytes failed with code {ws_bytes}")
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=p.device)
    dist = torch.empty((B, N), dtype=torch.float32, device=p.device)
    idx = torch.empty((B, N), dtype=torch.int64, device=p.device)
    call("md_nn_sided", p, q, B, N, M, int(bool(skip_same_index)), dist, idx, ws, ws_bytes)
    return dist, idx


def sided_distance(p1, p2, skip_same_index=False):
    """kaolin.metrics.pointcloud.sided_distance: for every point of p1 [B,N,3] the SQUARED distance to, and the index of, its
    nearest point in p2 [B,M,3] -> (dist2 float32 [B,N], idx int64 [B,N]).  Direct-form fp32 distances, ties to the lowest
    index, NaN coordinates give NaN.  `skip_same_index=True` leaves p2[i] out for query i (p1 is p2: the nearest OTHER
    point, pytorch3d's knn_points(K=2).dists[..., -1]).  Not differentiable; `chamfer_distance` is."""
    return _nn(_cloud(p1, "sided_distance"), _cloud(p2, "sided_distance"), skip_same_index)


def _csr(idx, n_targets):
    """CSR of a dynamic index table idx int64 [B,K] with values in [0, n_targets): (ptr int32 [B,n_targets+1], order int32
    [B,K] = the positions sorted stably by their value)."""
    return csr_by_row(idx, n_targets)


class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, q, w1, w2):
        d12, i12 = _nn(p, q)
        d21, i21 = _nn(q, p)
        ctx.save_for_backward(p, q, i12, i21)
        ctx.w = (float(w1), float(w2))
        # the two means of 50 000 float32 terms are accumulated in float64 (a [B,N] reduction: torch plumbing, not a hot path)
        val = d12.mean(dim=1, dtype=torch.float64) * w1 + d21.mean(dim=1, dtype=torch.float64) * w2
        return val.to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        p, q, i12, i21 = ctx.saved_tensors
        B, N, M = p.shape[0], p.shape[1], q.shape[1]
        need_q = ctx.needs_input_grad[1]
        g = grad_out.to(torch.float32).contiguous()
        ptr_p, order_p = _csr(i21, N)
        ptr_q, order_q = _csr(i12, M) if need_q else (None, None)
        dp = torch.empty_like(p)
        dq = torch.empty_like(q) if need_q else None
        call("md_chamfer_bwd", p, q, i12, i21, ptr_p, order_p, ptr_q, order_q, B, N, M, ctx.w[0], ctx.w[1], g, dp, dq)
        return (dp if ctx.needs_input_grad[0] else None), dq, None, None


def chamfer_distance(p1, p2, w1=1.0, w2=1.0, squared=True):
    """mean_i dist2(p1_i -> p2) * w1 + mean_j dist2(p2_j -> p1) * w2 per batch element: float32 [B], differentiable w.r.t.
    both clouds (neighbours held fixed; the gradient of p2 is skipped when it does not require one).

    This is kaolin.metrics.pointcloud.chamfer_distance as its documentation defines it.  kaolin was not available where
    this was written, so nothing here was compared with kaolin's code: the oracle of the tests is a float64 restatement of
    the formula above (tests/pointcloud_cases.py).  Only `squared=True`, the reference's call, is implemented."""
    if not squared:
        raise NotImplementedError("chamfer_distance: only squared=True (the reference's call) is implemented")
    _gpu_only(p1, "chamfer_distance")
    _gpu_only(p2, "chamfer_distance")
    for t in (p1, p2):
        if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"chamfer_distance: expected [B,N,3] point clouds with B, N >= 1, got {tuple(t.shape)}")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("chamfer_distance: both clouds need the same batch size")
    return _ChamferFn.apply(p1.to(torch.float32).contiguous(), p2.to(torch.float32).contiguous(), float(w1), float(w2))


# ---- surface sampling ----------------------------------------------------------------------------------------------------
def _check_faces(faces, n_verts):
    """faces int64 [F,3] contiguous on the GPU with every index in [0, n_verts): checked once here, the kernels index unchecked."""
    def limits(F):
        if F < 1 or n_verts < 1:
            raise ValueError("sample_points: the mesh has no faces or no vertices")
    return check_faces(faces, n_verts, "sample_points (triangle meshes only)", limits, NotImplementedError)


def face_areas(vertices, faces):
    """Triangle areas float32 [B,F] of vertices [B,V,3], faces [F,3]: md_face_areas."""
    _gpu_only(vertices, "face_areas")
    v = vertices.detach().to(torch.float32).contiguous()
    f = _check_faces(faces, v.shape[1])
    areas = torch.empty((v.shape[0], f.shape[0]), dtype=torch.float32, device=v.device)
    call("md_face_areas", v, f, v.shape[0], v.shape[1], f.shape[0], areas)
    return areas


def area_cdf(areas):
    """The inclusive prefix sum md_sample_points bisects: accumulated in float64 and rounded to float32, so it is
    non-decreasing whatever order the device scan adds in (a zero-area face repeats its predecessor's value)."""
    return torch.cumsum(areas.to(torch.float64), dim=1).to(torch.float32).contiguous()


class _SamplePointsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, faces, cdf, r_face, r_u, r_v, choices_in):
        B, V, _ = vertices.shape
        F, S = faces.shape[0], r_u.shape[1]
        dev = vertices.device
        points = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
        choices = torch.empty((B, S), dtype=torch.int64, device=dev)
        weights = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
        call("md_sample_points", vertices, faces, cdf, r_face, r_u, r_v, choices_in, B, V, F, S, points, choices, weights)
        ctx.save_for_backward(faces, choices, weights)
        ctx.n_verts = V
        ctx.mark_non_differentiable(choices, weights)
        return points, choices, weights

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_points, _gc, _gw):
        faces, choices, weights = ctx.saved_tensors
        B, S = choices.shape
        V = ctx.n_verts
        if 3 * S >= 2 ** 31:
            raise _lib.MeshDiffusionHipError("sample_points backward: 3 * num_samples must fit int32")
        g = grad_points.to(torch.float32).contiguous()
        ptr, order = _csr(faces[choices].reshape(B, S * 3), V)     # entry 3 * sample + corner names vertex faces[choice][corner]
        dverts = torch.empty((B, V, 3), dtype=torch.float32, device=g.device)
        call("md_sample_points_bwd", g, weights, ptr, order, B, V, S, dverts)
        return dverts, None, None, None, None, None, None


def sample_points(vertices, faces, num_samples, areas=None, face_features=None, *, uniforms=None, face_choices=None,
                  generator=None):
    """The reference's `sample_points` (geometry/utils.py:55, kaolin.ops.mesh.sample_points): `num_samples` points per mesh,
    faces drawn in proportion to their area, then uniform on the face.  vertices [B,V,3], faces [F,3] (shared) ->
    (points float32 [B,S,3], face_choices int64 [B,S]) and, with face_features [B,F,3,D], the interpolated features [B,S,D].
    Differentiable w.r.t. `vertices` (the face choice is not differentiated, as in the reference).

    The face of a sample is the first one whose cumulative area exceeds r_face * total (inverse CDF; the reference draws with
    `multinomial`, so its random stream is not reproduced), the point w0 v0 + w1 v1 + w2 v2 with u = sqrt(r_u), w0 = 1 - u,
    w1 = u (1 - r_v), w2 = u r_v.  `uniforms`: (r_face, r_u, r_v), each [B,S] in [0, 1) (or one [3,B,S] tensor); drawn with
    torch.rand on the device (`generator`) when not given.  `face_choices` [B,S] fixes the faces (r_face may then be None)."""
    _gpu_only(vertices, "sample_points")
    if vertices.dim() != 3 or vertices.shape[-1] != 3:
        raise ValueError(f"sample_points: expected vertices [B,V,3], got {tuple(vertices.shape)}")
    if num_samples < 1:
        raise ValueError("sample_points: num_samples must be positive")
    v = vertices.to(torch.float32).contiguous()
    B, V, dev = v.shape[0], v.shape[1], v.device
    f = _check_faces(faces, V)
    F, S = f.shape[0], int(num_samples)
    if uniforms is None:
        uniforms = torch.rand((3, B, S), dtype=torch.float32, device=dev, generator=generator)
    r_face, r_u, r_v = uniforms
    prep = lambda t: t.detach().to(device=dev, dtype=torch.float32).reshape(B, S).contiguous()      # noqa: E731
    r_u, r_v = prep(r_u), prep(r_v)
    cdf = choices_in = None
    if face_choices is not None:
        choices_in = face_choices.to(device=dev, dtype=torch.int64).reshape(B, S).contiguous()
        lo, hi = torch.aminmax(choices_in)
        if int(lo) < 0 or int(hi) >= F:
            raise ValueError(f"face_choices name faces outside [0, {F})")
        r_face = None
    else:
        r_face = prep(r_face)
        if areas is None:
            areas = face_areas(v, f)
        areas = areas.detach().to(device=dev, dtype=torch.float32).reshape(B, F)
        cdf = area_cdf(areas)
        if not bool((cdf[:, -1] > 0).all()) or not bool(torch.isfinite(cdf[:, -1]).all()):
            raise ValueError("sample_points: the total face area must be positive and finite")
    points, choices, weights = _SamplePointsFn.apply(v, f, cdf, r_face, r_u, r_v, choices_in)
    if face_features is None:
        return points, choices
    ff = face_features.to(dev)
    if ff.dim() != 4 or ff.shape[:3] != (B, F, 3):
        raise ValueError(f"sample_points: expected face_features [B,F,3,D], got {tuple(ff.shape)}")
    sel = torch.gather(ff, 1, choices[:, :, None, None].expand(B, S, 3, ff.shape[-1]))               # [B,S,3,D]
    w = weights.to(ff.dtype)
    feats = w[:, :, 0:1] * sel[:, :, 0] + w[:, :, 1:2] * sel[:, :, 1] + w[:, :, 2:3] * sel[:, :, 2]
    return points, choices, feats


_IN_FIT = ("sdf_regularizer_weight", "fit_to_points")


def __getattr__(name):
    """The fitting loop is in fit.py, which imports this module: its names are handed out from there on first use."""
    if name in _IN_FIT:
        from . import fit
        return getattr(fit, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
