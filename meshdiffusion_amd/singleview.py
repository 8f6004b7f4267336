"""The single-view fit and its visible-tet labelling on MI355X -- host side of csrc/visibility.hip.

The reference's second generation mode, `cond_gen`, reads a dict `{'sdf', 'deform', 'vis', 'vis_rast'}`: the last thing
nvdiffrec/fit_singleview.py writes (:783-827) after a single-view RGBD fit (`dmtet_singleview.DMTetGeometry.tick`), the
fixed-topology pass and a labelling of every tetrahedron as seen or occluded from that view (lib/render/render.py:346-407 with
`get_visible_tets=True`), spread to the grid vertices.  This module is that path:

  window_min_depth, visible_tets, label_vertices   the visibility contract in the header comment of csrc/visibility.hip; the
                                kernels run on the GPU only: a CPU tensor is an error, not a fallback
  single_view_partial           geometry + one view (or several: their union) -> the dict, on the CPU
  init_with_gt_surface          dmtet_singleview.py:421-435, the nearest visible face through `pointcloud._nn` (md_nn_sided)

The rest of the single-view tick is plain torch and lives with the other fits in fit.py: `carve_single_view` (:447-458),
`depth_loss_single_view` (:474-490) and `fit_single_view`, the reference's loop (fit_singleview.py:489-502) around that tick
(:438-516); they are still found here by name.  tools/fit_singleview.py is the command line around them.
"""
import torch

from . import _lib
from .hip_ops import call
from .render import MAX_RES, MAX_VIEWS, _gpu_only, rasterize, xfm_points

MAX_RADIUS = 15                          # VS_MAX_RADIUS of csrc/visibility.hip
EMPTY_DEPTH = 100.0                      # VS_EMPTY


# ---- the visibility contract -------------------------------------------------------------------------------------------------------
def _check_rast(rast, what):
    """rast float32 [B,H,W,4] within the rasteriser's limits -> (contiguous float32 rast, B, H, W)."""
    if not torch.is_tensor(rast) or rast.dim() != 4 or rast.shape[-1] != 4 or min(rast.shape[:3]) < 1:
        raise ValueError(f"{what}: expected rast [B,H,W,4], got {tuple(rast.shape) if torch.is_tensor(rast) else type(rast)}")
    _gpu_only(rast, what)
    B, H, W, _ = rast.shape
    if B > MAX_VIEWS or H > MAX_RES or W > MAX_RES:
        raise _lib.MeshDiffusionHipError(f"{what}: at most {MAX_VIEWS} views of {MAX_RES} x {MAX_RES} pixels (MD_ERR_UNSUPPORTED)")
    return rast.detach().to(torch.float32).contiguous(), B, H, W


def _check_radius(radius, what):
    r = int(radius)
    if r != radius or r < 0:
        raise ValueError(f"{what}: radius must be a non-negative integer, got {radius!r}")
    if r > MAX_RADIUS:
        raise _lib.MeshDiffusionHipError(f"{what}: radius {r} exceeds {MAX_RADIUS} (MD_ERR_UNSUPPORTED)")
    return r


def _window_min(rast, B, H, W, r):
    dmin = torch.empty((B, H, W), dtype=torch.float32, device=rast.device)
    call("md_window_min", rast, B, H, W, r, dmin)
    return dmin


def window_min_depth(rast, radius=7):
    """Dmin of the visibility contract: rast float32 [B,H,W,4], layer 1 of `rasterize` -> float32 [B,H,W], the minimum over the
    (2 radius + 1)^2 window, clipped to the image, of zf where a triangle covers the pixel and 100.0 where none does: the
    reference's -max_pool2d(-corrected_rast_depth, 2 r + 1, 1, r).  0 <= radius <= 15 (the reference's depth_search_range is 7)."""
    r = _check_radius(radius, "window_min_depth")
    rast, B, H, W = _check_rast(rast, "window_min_depth")
    return _window_min(rast, B, H, W, r)


def visible_tets(rast, centres, mvp, radius=7):
    """visible bool [B,T] of the visibility contract: tet t is visible in view b iff its centre (centres float32 [T,3], world
    space: `geometry.getTetCenters()`), projected with mvp [B,4,4] and rounded to a pixel and a depth step, lies inside the clip
    cube and not behind the window minimum of `rast` (layer 1 of `rasterize`) at that pixel.  A centre with w <= 0 or a non-finite
    clip coordinate is not visible (the reference projects it through the camera)."""
    r = _check_radius(radius, "visible_tets")
    rast, B, H, W = _check_rast(rast, "visible_tets")
    if not torch.is_tensor(centres) or centres.dim() != 2 or centres.shape[-1] != 3 or centres.shape[0] < 1:
        raise ValueError(f"visible_tets: expected centres [T,3] with T >= 1, got {tuple(centres.shape)}")
    if not torch.is_tensor(mvp) or tuple(mvp.shape) != (B, 4, 4):
        raise ValueError(f"visible_tets: expected mvp [{B},4,4], got {tuple(mvp.shape)}")
    _gpu_only(centres, "visible_tets")
    dev, T = rast.device, centres.shape[0]
    c = centres.detach().to(device=dev, dtype=torch.float32).contiguous()
    m = mvp.detach().to(device=dev, dtype=torch.float32).contiguous()
    dmin = _window_min(rast, B, H, W, r)
    visible = torch.empty((B, T), dtype=torch.uint8, device=dev)
    call("md_tet_visibility", dmin, c, m, B, T, H, W, visible)
    return visible.view(torch.bool)


def _check_index_table(t, shape_tail, hi, what, name):
    """An int64 index table with every entry in [0, hi): checked once here, the kernels skip what lies outside."""
    if not torch.is_tensor(t) or t.dim() != len(shape_tail) + 1 or tuple(t.shape[1:]) != shape_tail:
        raise ValueError(f"{what}: expected {name} [n{''.join(',' + str(s) for s in shape_tail)}], got {tuple(t.shape)}")
    t = t.to(torch.int64).contiguous()
    if t.numel() > 0:
        lo, top = torch.aminmax(t)
        if int(lo) < 0 or int(top) >= hi:
            raise ValueError(f"{what}: {name} names entries outside [0, {hi})")
    return t


def label_vertices(visible, rast, face_tet, indices, n_verts):
    """The labels of the visibility contract: visible bool [B,T] (`visible_tets`), rast float32 [B,H,W,4] the layer it came from,
    face_tet int64 [F] the tet of each face of the rasterised mesh (`geometry.getValidTetIdx()`), indices int64 [T,4] the grid's
    tets, n_verts = N -> (vis float32 [N] of 0 / 1, vis_rast bool [N]): the grid vertices of the tets visible in any view, and of
    those or the tets that own a pixel of layer 1.  These are the dtypes of the reference's dict (fit_singleview.py:812-820)."""
    what = "label_vertices"
    rast, B, H, W = _check_rast(rast, what)
    if not torch.is_tensor(visible) or visible.dim() != 2 or visible.shape[0] != B or visible.shape[1] < 1:
        raise ValueError(f"{what}: expected visible [{B},T] with T >= 1, got {tuple(visible.shape)}")
    _gpu_only(visible, what)
    N, T, dev = int(n_verts), visible.shape[1], rast.device
    if N < 1:
        raise ValueError(f"{what}: n_verts must be positive, got {n_verts}")
    if N > 2 ** 31 - 1 or T > 2 ** 31 - 1:
        raise _lib.MeshDiffusionHipError(f"{what}: the counts of tets and vertices must fit int32 (MD_ERR_UNSUPPORTED)")
    idx = _check_index_table(indices.to(dev), (4,), N, what, "indices")
    if idx.shape[0] != T:
        raise ValueError(f"{what}: visible has {T} tets, indices {idx.shape[0]}")
    ft = _check_index_table(face_tet.to(dev), (), T, what, "face_tet")
    F = ft.shape[0]
    if F >= 2 ** 24:
        raise _lib.MeshDiffusionHipError(f"{what}: the rasteriser takes fewer than 2^24 faces (MD_ERR_UNSUPPORTED)")
    vis_u8 = visible.to(torch.uint8).contiguous() if visible.dtype != torch.bool else visible.contiguous().view(torch.uint8)
    rast_tet = None
    if F > 0:
        rast_tet = torch.zeros(T, dtype=torch.uint8, device=dev)
        call("md_rast_mark_tets", rast, ft, B, H, W, F, T, rast_tet)
    vis = torch.zeros(N, dtype=torch.float32, device=dev)
    vis_rast = torch.zeros(N, dtype=torch.uint8, device=dev)
    call("md_tets_mark_verts", vis_u8, rast_tet, idx, B, T, N, vis, vis_rast)
    return vis, vis_rast.view(torch.bool)


@torch.no_grad()
def single_view_partial(geometry, target, radius=7):
    """The dict `evaler.cond_gen` reads (`config.eval.partial_dmtet_path`), as fit_singleview.py:795-827 makes it, from a
    `DMTetGeometry` or a `DMTetGeometryFixedTopo` and a target of `make_targets` (its `mvp` and `resolution`):
        getMesh -> rasterize (layer 1) -> getTetCenters -> visible_tets -> label_vertices with getValidTetIdx() as face_tet.
    Returns CPU tensors {'sdf' float32 [N] (`sdf_sign` for the fixed-topology geometry, as the reference saves it), 'deform'
    float32 [N,3], 'vis' float32 [N] of 0 / 1, 'vis_rast' bool [N]}.  More than one view in `target` gives the union over them."""
    _gpu_only(geometry.deform, "single_view_partial")
    mesh = geometry.getMesh()
    mvp = target["mvp"].detach().to(device=mesh.v_pos.device, dtype=torch.float32)
    if mesh.t_pos_idx.shape[0] == 0:
        raise _lib.MeshDiffusionHipError("single_view_partial: the mesh has no faces")
    clip = xfm_points(mesh.v_pos.detach()[None], mvp).contiguous()
    rast = rasterize(clip, mesh.t_pos_idx, target["resolution"], num_layers=1)[0]
    visible = visible_tets(rast, geometry.getTetCenters().detach(), mvp, radius)
    vis, vis_rast = label_vertices(visible, rast, geometry.getValidTetIdx(), geometry.indices, geometry.verts.shape[0])
    sdf = geometry.sdf_sign if hasattr(geometry, "sdf_sign") else geometry.sdf
    return {"sdf": sdf.detach().float().cpu(), "deform": geometry.deform.detach().cpu(), "vis": vis.cpu(), "vis_rast": vis_rast.cpu()}


# ---- the single-view tick ----------------------------------------------------------------------------------------------------------
@torch.no_grad()
def init_with_gt_surface(geometry, gt_verts, surface_faces, campos):
    """dmtet_singleview.py:421-435: every grid vertex that lies on the camera's side of its nearest visible face of the
    ground-truth mesh gets sdf = 1.0.  gt_verts [V,3], surface_faces int64 [Fs,3] the faces the view sees (the `rast_triangle_id`
    faces of `render_depth`), campos [3].  Nearest = the nearest face CENTRE, through md_nn_sided (direct-form fp32 distances, ties
    to the lowest index); the face normal (v0 - v1) x (v0 - v2) is flipped towards the camera (kept where normal . (campos -
    centre) >= 0); a vertex is outside where (vertex - centre) . normal > 0.  No gradient.  Returns the number of vertices set."""
    from .pointcloud import _nn
    _gpu_only(geometry.sdf, "init_with_gt_surface")
    dev = geometry.sdf.device
    if surface_faces.dim() != 2 or surface_faces.shape[-1] != 3 or surface_faces.shape[0] < 1:
        raise ValueError(f"init_with_gt_surface: expected surface_faces [Fs,3] with Fs >= 1, got {tuple(surface_faces.shape)}")
    gv = gt_verts.detach().to(device=dev, dtype=torch.float32)
    fv = gv[surface_faces.to(dev).long()]                                      # [Fs,3,3]
    centres = fv.mean(dim=1)
    v_pos = geometry.get_deformed().detach().to(torch.float32)
    idx = _nn(v_pos[None].contiguous(), centres[None].contiguous())[1][0]
    displacement = v_pos - centres[idx]
    view_dirs = campos.detach().to(device=dev, dtype=torch.float32).reshape(1, 3) - centres
    normals = torch.linalg.cross(fv[:, 0] - fv[:, 1], fv[:, 0] - fv[:, 2])
    mask = ((normals * view_dirs).sum(dim=-1, keepdim=True) >= 0).float()
    normals = normals * mask - normals * (1 - mask)
    outside = (displacement * normals[idx]).sum(dim=-1) > 0
    geometry.sdf.data[outside] = 1.0
    return int(outside.sum())


_IN_FIT = ("carve_single_view", "depth_loss_single_view", "fit_single_view")


def __getattr__(name):
    """The carve, the depth term and the loop of the tick are in fit.py, which imports this module: handed out from there on first use."""
    if name in _IN_FIT:
        from . import fit
        return getattr(fit, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
