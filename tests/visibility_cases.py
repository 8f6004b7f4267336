"""Cases and torch restatements of the visibility contract (the header comment of csrc/visibility.hip) and of the single-view
tick's two helpers, so that a machine without the reference can evaluate them on any input.  Shared by
tools/gen_golden_visibility.py, the CPU tests, the GPU tests and tools/bench_visibility.py.

  window_min_restated / visible_tets_restated / label_vertices_restated   the contract as the reference writes it: `max_pool2d`
                              of the negated images, both filters literally, `unique` and indexed stores.  Every fp32 operation of
                              the contract is rounded on its own, so these reproduce the kernels' decisions exactly on the CPU.
  init_with_gt_surface_restated   dmtet_singleview.py:421-435 by brute force in `dtype`, with the figures that tell where the
                              decision is ill-conditioned in fp32.
  carve_single_view_restated  the carve of the single-view tick.
Every restatement runs on the device of its inputs.
"""
import torch

import raster_cases as rc

EMPTY = 100.0
RADII = (0, 7, 15)
GRID_CASES = (("sphere", 64, 64), ("sphere", 40, 72), ("torus", 64, 64), ("torus", 40, 72), ("sphere", 5, 9))
INIT_CASES = ("sphere", "torus")
INIT_RES = 64
INIT_ANGLE = rc.ANGLES[0]
DEFORM_SEED = 21
# init_with_gt_surface in fp32 against float64.  The inputs are the same fp32 numbers; the fp32 path rounds the face centres (a sum
# of three coordinates and a division: about 2 units of 6e-8 on coordinates below 1.1), the displacement, the cross product and
# the dot products, a handful of roundings each on magnitudes below 4 (the camera is 3 away): absolute errors below 1e-6.  The
# gaps are ten times that.  A vertex is left out when, for the nearest centre or a centre within NN_GAP of it (in distance),
#   * its decision differs from the nearest's (a tie in fp32 may pick it), or
#   * its signed distance to the face's plane is below DOT_GAP * max(|displacement|, 1), or
#   * the flip of its normal is undecided: |normal . view| <= DOT_GAP * |normal| |view|.
NN_GAP = 1e-5
DOT_GAP = 1e-5
NN_CANDIDATES = 4


def case_id(case):
    return rc.case_id(case)


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def _pool_min(img, radius):
    """-max_pool2d(-img) over the (2 r + 1)^2 window, stride 1, padding r (-inf: it never wins), img [B,H,W]."""
    return -torch.nn.functional.max_pool2d(-img, kernel_size=2 * radius + 1, stride=1, padding=radius)


def corrected_depth(rast):
    d = rast[..., 2].clone()
    d[rast[..., 3] == 0] = EMPTY
    return d


def window_min_restated(rast, radius):
    """rast float32 [B,H,W,4] -> Dmin float32 [B,H,W], as render.py:372-392 writes it."""
    return _pool_min(corrected_depth(rast), radius)


def project_restated(centres, mvp, H, W):
    """(n [B,T,3], q [B,T,3] float32, valid bool [B,T]) of the contract, fp32."""
    c = rc.xfm_points_restated(centres, mvp)                                   # [B,T,4]
    n = c[..., :3] / c[..., 3:4]
    S = torch.tensor([W - 1, H - 1, H - 1], dtype=torch.float32, device=c.device)
    q = torch.round((n / 2.0 + 0.5) * S)
    valid = (torch.logical_and(q <= S, q >= 0).float().prod(dim=-1) == 1)
    valid = valid & torch.isfinite(c).all(-1) & (c[..., 3] > 0)                # the contract's deviation
    return n, q, valid


def visible_tets_restated(rast, centres, mvp, radius):
    """visible bool [B,T]: the depth filter or the emptiness filter of render.py:394-407, for the valid centres."""
    B, H, W, _ = rast.shape
    n, q, valid = project_restated(centres, mvp, H, W)
    qi = torch.where(valid[..., None], q, torch.zeros_like(q)).long()
    b = torch.arange(B, device=rast.device)[:, None]
    reference_depth = window_min_restated(rast, radius)[b, qi[..., 1], qi[..., 0]]             # row q_y, column q_x
    depth_filter = reference_depth >= n[..., 2]
    empty = _pool_min((rast[..., 3] == 0).float(), radius).bool()              # every pixel of the window is empty
    empty_filter = empty[b, qi[..., 1], qi[..., 0]]
    return valid & torch.logical_or(empty_filter, depth_filter)


def label_vertices_restated(visible, rast, face_tet, indices, n_verts):
    """(vis float32 [N], vis_rast bool [N]) as fit_singleview.py:800-820 writes them, the union over the views."""
    T, F, dev = indices.shape[0], face_tet.shape[0], indices.device
    visible_tets = visible.any(0)
    ids = rast[..., 3].unique()
    ids = ids[(ids >= 1) & (ids <= F)].long() - 1
    both = visible_tets.clone()
    if ids.numel() > 0:
        both[face_tet[ids].unique()] = True
    vis = torch.zeros(n_verts, dtype=torch.float32, device=dev)
    vis[indices[visible_tets].unique()] = 1
    vis_rast = vis.clone()
    vis_rast[indices[both].unique()] = 1
    return vis, vis_rast.bool()


# ---- the single-view tick's helpers -------------------------------------------------------------------------------------------------
def init_with_gt_surface_restated(v_pos, gt_verts, surface_faces, campos, dtype=torch.float64, chunk=2048):
    """dmtet_singleview.py:421-435 by brute force in `dtype`: dict of `outside` bool [N] (the vertices set to 1.0) and `unsure`
    bool [N] (the decision is ill-conditioned in fp32, by the gaps above)."""
    fv = gt_verts.to(dtype)[surface_faces]
    centres = fv.mean(dim=1)
    view = campos.to(dtype).reshape(1, 3) - centres
    normals = torch.linalg.cross(fv[:, 0] - fv[:, 1], fv[:, 0] - fv[:, 2])
    facing = (normals * view).sum(-1)
    flip_unsure = facing.abs() <= DOT_GAP * normals.norm(dim=-1) * view.norm(dim=-1)
    mask = (facing >= 0).to(dtype)[:, None]
    normals = normals * mask - normals * (1 - mask)
    p = v_pos.to(dtype)
    k = min(NN_CANDIDATES, centres.shape[0])
    outside, unsure = [], []
    for s in range(0, p.shape[0], chunk):
        x = p[s:s + chunk]
        d2 = ((x[:, None, :] - centres[None]) ** 2).sum(-1)
        dist2, idx = torch.topk(d2, k, dim=1, largest=False, sorted=True)       # [n,k]
        disp = x[:, None, :] - centres[idx]
        nrm = normals[idx]
        dot = (disp * nrm).sum(-1)
        out = dot > 0
        dist = dist2.sqrt()
        near = (dist - dist[:, :1]) <= NN_GAP                                  # column 0 is the nearest itself
        weak = dot.abs() <= DOT_GAP * nrm.norm(dim=-1) * disp.norm(dim=-1).clamp_min(1.0)
        bad = near & ((out != out[:, :1]) | weak | flip_unsure[idx])
        outside.append(out[:, 0])
        unsure.append(bad.any(1))
    return {"outside": torch.cat(outside), "unsure": torch.cat(unsure)}


def carve_single_view_restated(v_pos, sdf, mvp, mask_cont, H, W):
    """The carve of dmtet_singleview.py:447-458 on v_pos [N,3], sdf [N], mask_cont [B,H,W,1]: the new sdf."""
    clip = rc.xfm_points_restated(v_pos, mvp)
    cam = clip[:, :, :2] / clip[:, :, -1:]
    px = ((cam[..., 0] * 0.5 + 0.5).clip(0, 1) * (W - 1)).long()
    py = ((cam[..., 1] * 0.5 + 0.5).clip(0, 1) * (H - 1)).long()
    target_mask = mask_cont[:, :, :, 0] == 0
    sdf = sdf.clone()
    for k in range(target_mask.size(0)):
        v_mask = target_mask[k, py[k], px[k]].view(v_pos.size(0))
        sdf[v_mask] = sdf[v_mask].abs().clamp(0.0, 1.0)
    return sdf


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def grid():
    """The shipped 64 grid x 2.1: (pos float32 [N,3], tets int64 [T,4]) CPU tensors."""
    verts, idx = rc.tet_grid()
    return torch.as_tensor(verts, dtype=torch.float32) * rc.MESH_SCALE, torch.as_tensor(idx, dtype=torch.long)


def case_deform(n_verts):
    """A seeded deformation in [-0.5, 0.5]^3: moves every vertex off the grid's symmetry planes."""
    return torch.rand(n_verts, 3, generator=torch.Generator().manual_seed(DEFORM_SEED)) - 0.5


def deformed(pos, deform, grid_res=64, deform_scale=2.0):
    return pos + 2 / (grid_res * 2) * deform * deform_scale


def init_case(name):
    """The inputs of init_with_gt_surface for a case, on the CPU and by the restatements alone: (v_pos [N,3] the deformed grid,
    gt_verts, surface_faces [Fs,3] the faces layer 1 of the restated rasteriser shows, campos [3])."""
    pos, _ = grid()
    gt_verts, gt_faces = rc.mesh(name)
    mvp, campos = rc.cameras((INIT_ANGLE,), INIT_RES, INIT_RES)
    ids = rc.rasterize_restated(rc.xfm_points_restated(gt_verts, mvp), gt_faces, INIT_RES, INIT_RES)["ids"][:, 0]
    seen = ids.unique()
    seen = seen[seen > 0] - 1
    return deformed(pos, case_deform(pos.shape[0])), gt_verts, gt_faces[seen], campos[0]


def hand_rast():
    """A 6 x 6 layer with two covered patches and exact values: rast float32 [1,6,6,4]."""
    rast = torch.zeros(1, 6, 6, 4)
    for (i, j, z, f) in ((1, 1, 0.25, 1), (1, 2, 0.5, 1), (2, 1, -0.125, 2), (2, 2, 0.75, 2), (4, 4, -0.5, 3), (4, 5, 0.0, 3),
                         (0, 5, 0.875, 4)):
        rast[0, i, j] = torch.tensor([0.25, 0.5, z, float(f)])
    return rast
