"""Depth and silhouette rendering for DMTet fitting on MI355X -- host side of csrc/raster.hip and csrc/antialias.hip.

The reference gets its depth buffers from nvdiffrast (nvdiffrec/lib/render/render.py:287-329): `xfm_points` -> two depth-peeled
layers -> `interpolate(v_pos)` -> |gb_pos - campos|, and supervises the geometry with the depth terms of `DMTetGeometry.tick`
(nvdiffrec/lib/geometry/dmtet.py:402-434) and the silhouette carve (:366-378).  This module is that path: `rasterize` and
`render_depth` follow the rasterisation contract in the header comment of csrc/raster.hip and `make_targets` renders what a fit
is supervised with; the losses, the carve and the loops around them (`depth_loss`, `carve_outside_silhouette`, `fit_to_views`, ...)
are plain torch and live in fit.py, still found here by name.  `edge_neighbours` and `antialias` follow the antialiasing
contract in the header comment of csrc/antialias.hip: silhouette antialiasing in the manner of dr.antialias (render.py:256-276),
not equal to it, with gradients for the colour and the clip-space vertices.  `render_depth(antialias=True)` adds the antialiased
coverage of both layers, the one path from a silhouette to the vertices (the coverage term of tick, dmtet.py:394,399, is
`fit.silhouette_loss`).  `interpolate`, `rasterize(grad=True)` and `dmtet.vertex_normals` follow the interpolation contract in the header
comment of csrc/interp.hip: dr.interpolate, the `rast` gradient of dr.rasterize and auto_normals under autograd.  On top of them
`render_buffers` is the reference's `bsdf == 'normal'` renderer (render.py:105-106, 177-264), which the colour term of tick
(dmtet.py:391-400: `fit.image_loss` / `fit.color_loss`) reads.  `laplace_regularizer_const` is the regulariser of pass 2 of the
reference's fit (fit_dmtets.py:758-793: `fit.fit_fixed_topology`), by the fixed-topology contract in the header comment of
csrc/fixedtopo.hip.  `shade_diffuse` and `render_preview` are the quick-look image the reference renders of every sampled
mesh (nvdiffrec/eval.py:421-438: `bsdf == 'diffuse'`, kd = (0.75, 0.3, 0.6), an environment light, the two-sided geometric normal)
by the shading part of the mesh post-processing contract in the header comment of csrc/meshpost.hip: in the manner of that image,
not equal to it -- the environment comes in as nine spherical-harmonic coefficients (`sh9_from_latlong`, `default_light`), which
stand in for the reference's cosine-convolved cube map, and `preview_camera` is its `rotate_scene`.  `render_textured` is the same
image with a `kd` texture in place of the one colour (the reference's `Texture2D.sample` inside render.py:shade): `rasterize` ->
`interpolate` of the texture coordinates -> `texture.sample` (the texture contract, csrc/texture.hip) -> times the irradiance of
`shade_diffuse` -> `antialias`, differentiable in the texture (`fit.fit_texture`).  The kernels run on the GPU
only: a CPU tensor is an error, not a fallback.  The camera helpers, `xfm_points` and `shading_normal` are plain torch and run
anywhere; `sh9_from_latlong` and `default_light` are numpy on the host.

Not built: materials beyond a diffuse colour or `kd` texture (`ks`, normal maps), specular / PBR shading,
cube maps and `.hdr` loading, mip maps and trilinear filtering (no uv screen derivatives leave the rasteriser), MLP textures,
camera-space lights, gradients of the preview and of the textured render w.r.t. the geometry, spp > 1 / MSAA, clipping of triangles
that cross w = 0, more than two layers, gradients for mvp / campos and zf, a silhouette search beyond the covering triangle.
"""
import numpy as np
import torch

from . import _lib
from ._csr import check_faces, csr_by_row
from .hip_ops import _gpu_only, call

TILE = 16                                # RS_TILE of csrc/raster.hip
MAX_RES, MAX_VIEWS, MAX_FACES = 2048, 64, 2 ** 24 - 1
MAX_CHANNELS = 8                         # AA_MAX_C of csrc/antialias.hip


# ---- camera matrices (nvdiffrec/lib/render/util.py:193-277: float32 tensors of numpy-double entries) ---------------------------
def _mat(rows, device):
    return torch.tensor(rows, dtype=torch.float32, device=device)


def perspective(fovy=0.7854, aspect=1.0, n=0.1, f=1000.0, device=None):
    """gluPerspective with y flipped (row 0 of the image is y = -1)."""
    y = np.tan(fovy / 2)
    return _mat([[1 / (y * aspect), 0, 0, 0], [0, 1 / -y, 0, 0], [0, 0, -(f + n) / (f - n), -(2 * f * n) / (f - n)],
                 [0, 0, -1, 0]], device)


def translate(x, y, z, device=None):
    return _mat([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z], [0, 0, 0, 1]], device)


def rotate_x(a, device=None):
    s, c = np.sin(a), np.cos(a)
    return _mat([[1, 0, 0, 0], [0, c, s, 0], [0, -s, c, 0], [0, 0, 0, 1]], device)


def rotate_y(a, device=None):
    s, c = np.sin(a), np.cos(a)
    return _mat([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], device)


@torch.no_grad()
def random_rotation_translation(t, device=None):
    """A random frame and a translation in [-t, t]^3, drawn from numpy's global stream in the reference's order (nine
    normals, then three uniforms)."""
    m = np.random.normal(size=[3, 3])
    m[1] = np.cross(m[0], m[2])
    m[2] = np.cross(m[0], m[1])
    m = m / np.linalg.norm(m, axis=1, keepdims=True)
    out = np.zeros((4, 4))
    out[:3, :3] = m
    out[3, 3] = 1.0
    out[:3, 3] = np.random.uniform(-t, t, size=[3])
    return torch.tensor(out, dtype=torch.float32, device=device)


def xfm_points(points, matrix):
    """points [1|B,V,3] (or [V,3]), matrix [B,4,4] -> [B,V,4] = matrix (p, 1) (the reference's ru.xfm_points).  Differentiable;
    the four products are summed left to right elementwise, so the CPU and the GPU give the same bits."""
    p = points[None] if points.dim() == 2 else points
    if p.dim() != 3 or p.shape[-1] != 3 or matrix.dim() != 3 or matrix.shape[1:] != (4, 4):
        raise ValueError(f"xfm_points: expected points [1|B,V,3] and matrix [B,4,4], got {tuple(points.shape)} and {tuple(matrix.shape)}")
    if p.shape[0] not in (1, matrix.shape[0]):
        raise ValueError("xfm_points: points need batch size 1 or that of the matrices")
    m = matrix[:, None]
    return ((p[..., 0:1] * m[..., 0] + p[..., 1:2] * m[..., 1]) + p[..., 2:3] * m[..., 2]) + m[..., 3]


# ---- rasterisation -----------------------------------------------------------------------------------------------------------------
def _resolution(resolution):
    H, W = (int(resolution), int(resolution)) if np.isscalar(resolution) else (int(resolution[0]), int(resolution[1]))
    if H < 1 or W < 1:
        raise ValueError(f"resolution must be positive, got {(H, W)}")
    if H > MAX_RES or W > MAX_RES:
        raise _lib.MeshDiffusionHipError(f"resolution {(H, W)} exceeds {MAX_RES} (MD_ERR_UNSUPPORTED)")
    return H, W


def _check_faces(faces, n_verts):
    """faces int64 [F,3] contiguous on the device, F >= 0, every index in [0, n_verts): checked once, the kernels index unchecked."""
    def limits(F):
        if F > MAX_FACES:
            raise _lib.MeshDiffusionHipError("the rasteriser takes fewer than 2^24 faces (MD_ERR_UNSUPPORTED)")
    return check_faces(faces, n_verts, "rasterize", limits)


def _check_clip(pos_clip):
    if pos_clip.dim() != 3 or pos_clip.shape[-1] != 4 or pos_clip.shape[0] < 1 or pos_clip.shape[1] < 1:
        raise ValueError(f"expected pos_clip [B,V,4] with B, V >= 1, got {tuple(pos_clip.shape)}")
    if pos_clip.shape[0] > MAX_VIEWS:
        raise _lib.MeshDiffusionHipError(f"the rasteriser takes at most {MAX_VIEWS} views per call (MD_ERR_UNSUPPORTED)")


def _bin(pc, f, H, W):
    """The tile CSR of the triangles: (tile_ptr int32 [B * tiles + 1], tile_faces int32 [pairs]), or None when no triangle
    touches a tile.  Two kernels with a torch.cumsum between them, then a stable torch sort by tile."""
    B, V, F, dev = pc.shape[0], pc.shape[1], f.shape[0], pc.device
    if F == 0:
        return None
    counts = torch.empty(B * F, dtype=torch.int32, device=dev)
    call("md_raster_bin_count", pc, f, B, V, F, H, W, counts)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(ends[-1])
    if total > 2 ** 31 - 1:
        raise _lib.MeshDiffusionHipError(f"{total} (tile, triangle) pairs exceed 2^31 - 1 (MD_ERR_UNSUPPORTED)")
    if total == 0:
        return None
    offsets = (ends - counts).contiguous()
    pair_tile = torch.empty(total, dtype=torch.int32, device=dev)
    pair_face = torch.empty(total, dtype=torch.int32, device=dev)
    call("md_raster_bin_emit", pc, f, offsets, B, V, F, H, W, total, pair_tile, pair_face)
    n_tiles = B * ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
    tile_ptr, order = csr_by_row(pair_tile, n_tiles)
    return tile_ptr, pair_face[order].contiguous()


def _rasterize(pc, f, H, W):
    """pc float32 [B,V,4] contiguous, f checked faces -> (rast1, rast2) float32 [B,H,W,4]."""
    B, V, F, dev = pc.shape[0], pc.shape[1], f.shape[0], pc.device
    csr = _bin(pc, f, H, W)
    if csr is None:
        return torch.zeros((B, H, W, 4), dtype=torch.float32, device=dev), torch.zeros((B, H, W, 4), dtype=torch.float32, device=dev)
    rast1 = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
    rast2 = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
    call("md_raster_tiles", pc, f, csr[0], csr[1], B, V, F, H, W, rast1, rast2)
    return rast1, rast2


class _LayerPlan:
    """What the backward passes over one `rast` layer share: the covered list and the CSRs of the gathers, each built at the
    first backward that needs it (`nonzero`, a stable sort, `searchsorted`)."""

    def __init__(self, rast, n_faces):
        self.rast, self.F = rast, n_faces                                      # rast detached, float32, contiguous
        self._cov, self._csr = None, {}

    def cov(self):
        """(int64, int32) flat indices (b H + i) W + j of the pixels with 1 <= id <= F, ascending."""
        if self._cov is None:
            ids = self.rast[..., 3].reshape(-1)
            cov = torch.nonzero((ids >= 1) & (ids <= self.F))[:, 0]
            if 3 * cov.numel() >= 2 ** 31:
                raise _lib.MeshDiffusionHipError("3 x the covered pixels of a layer must fit int32 (MD_ERR_UNSUPPORTED)")
            self._cov = (cov, cov.to(torch.int32).contiguous())
        return self._cov

    def csr(self, tri, n_rows, per_view):
        """(ptr int32 [rows + 1], order int32 [3 n_cov]) of the codes 3 * entry + corner sorted stably by the row they name:
        tri[id - 1][corner], plus view * n_rows when every view has rows of its own."""
        key = (tri.data_ptr(), n_rows, per_view)                               # the entry holds `tri`, so the address stays its own
        if key not in self._csr or self._csr[key][2]._version != tri._version:
            B, H, W, _ = self.rast.shape
            cov = self.cov()[0]
            dest = tri[self.rast[..., 3].reshape(-1)[cov].to(torch.int64) - 1]
            if per_view:
                dest = dest + (torch.div(cov, H * W, rounding_mode="floor") * n_rows)[:, None]
            self._csr[key] = csr_by_row(dest.reshape(-1), n_rows * (B if per_view else 1)) + (tri,)
        return self._csr[key][:2]


class _RasterizeFn(torch.autograd.Function):
    """The two layers of `plans` (rasterised from pos_clip already) with md_raster_bary_bwd as the backward of their (u, v)
    w.r.t. pos_clip."""

    @staticmethod
    def forward(ctx, pos_clip, faces, plans):
        ctx.plans = plans
        ctx.save_for_backward(pos_clip, faces, plans[0].rast, plans[1].rast)
        ctx.set_materialize_grads(False)
        return plans[0].rast.view_as(plans[0].rast), plans[1].rast.view_as(plans[1].rast)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g1, g2):
        pos_clip, faces, rast1, rast2 = ctx.saved_tensors
        B, V, F = pos_clip.shape[0], pos_clip.shape[1], faces.shape[0]
        total = None
        for plan, rast, g in zip(ctx.plans, (rast1, rast2), (g1, g2)):
            if g is None or F == 0:
                continue
            _, H, W, _ = rast.shape
            cov = plan.cov()[1]
            N = cov.numel()
            if N == 0:
                continue
            ptr, order = plan.csr(faces, V, True)
            g = g.to(torch.float32).contiguous()
            corner_grad = torch.empty((N, 3, 3), dtype=torch.float32, device=g.device)
            dpos = torch.empty((B, V, 4), dtype=torch.float32, device=g.device)
            call("md_raster_bary_bwd", cov, N, rast, g, pos_clip, faces, ptr, order, B, V, F, H, W, corner_grad, dpos)
            total = dpos if total is None else total + dpos
        return (torch.zeros_like(pos_clip) if total is None else total), None, None


def _rasterize_grad(pc, f, H, W):
    """(layers, plans): the two rast layers of pc float32 [B,V,4] with a grad_fn to it, and the `_LayerPlan` of each."""
    plans = [_LayerPlan(r, f.shape[0]) for r in _rasterize(pc.detach(), f, H, W)]
    return _RasterizeFn.apply(pc, f, plans), plans


def rasterize(pos_clip, faces, resolution, num_layers=2, grad=False):
    """The contract's `rast` layers of pos_clip float32 [B,V,4], faces [F,3] at resolution (H, W) (or one int): a list of
    `num_layers` (1 or 2) float32 [B,H,W,4] tensors (u, v, zf, face index + 1), zeros where uncovered.  No gradient, unless
    grad=True: then the layers (the same bits) carry a grad_fn to `pos_clip` for u and v (ids held fixed; zf and the id get
    none, and neither does z), by the barycentric backward of the interpolation contract (csrc/interp.hip)."""
    _gpu_only(pos_clip, "rasterize")
    if num_layers not in (1, 2):
        raise NotImplementedError("rasterize: one or two layers")
    _check_clip(pos_clip)
    H, W = _resolution(resolution)
    if grad:
        pc = pos_clip.to(torch.float32).contiguous()
        f = _check_faces(faces.to(pc.device), pc.shape[1])
        return list(_rasterize_grad(pc, f, H, W)[0][:num_layers])
    pc = pos_clip.detach().to(torch.float32).contiguous()
    f = _check_faces(faces.to(pc.device), pc.shape[1])
    return list(_rasterize(pc, f, H, W)[:num_layers])


class _InterpolateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri, plan, rast_grad):
        B, H, W, _ = rast.shape
        Ba, N, C = attr.shape
        F = tri.shape[0]
        if F == 0:
            out = torch.zeros((B, H, W, C), dtype=torch.float32, device=rast.device)
        else:
            out = torch.empty((B, H, W, C), dtype=torch.float32, device=rast.device)
            call("md_interpolate", rast, attr, tri, B, Ba, N, C, F, H, W, out)
        ctx.plan, ctx.rast_grad = plan, rast_grad
        ctx.save_for_backward(attr, tri, rast)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        attr, tri, rast = ctx.saved_tensors
        plan = ctx.plan                                                        # the covered list and the CSRs of rast's layer
        B, H, W, _ = rast.shape
        Ba, N, C = attr.shape
        F = tri.shape[0]
        need_attr, need_rast = ctx.needs_input_grad[0], ctx.rast_grad and ctx.needs_input_grad[1]
        dattr = torch.empty_like(attr) if need_attr else None
        drast = torch.empty_like(rast) if need_rast else None
        n_cov = plan.cov()[1].numel() if F > 0 and (need_attr or need_rast) else 0
        if n_cov == 0:
            return (None if dattr is None else dattr.zero_()), (None if drast is None else drast.zero_()), None, None, None
        cov = plan.cov()[1]
        g = g.to(torch.float32).contiguous()
        ptr = order = corner_grad = None
        if need_attr:
            ptr, order = plan.csr(tri, N, Ba != 1)
            corner_grad = torch.empty((n_cov, 3, C), dtype=torch.float32, device=g.device)
        call("md_interpolate_bwd", cov, n_cov, rast, g, attr, tri, ptr, order, B, Ba, N, C, F, H, W, corner_grad, dattr, drast)
        return dattr, drast, None, None, None


def _check_tri(tri, n_rows):
    try:
        return _check_faces(tri, n_rows)
    except ValueError as e:
        raise ValueError(str(e).replace("faces", "tri").replace("vertices", "attribute rows")) from None


def interpolate(attr, rast, tri, rast_grad=False, _plan=None):
    """dr.interpolate by the interpolation contract in the header comment of csrc/interp.hip: attr float32 [N,C], [1,N,C] (shared
    by the views) or [B,N,C], 1 <= C <= 8; rast float32 [B,H,W,4] one layer of `rasterize`; tri [F,3] with indices into N (for a
    face-constant attribute tri[f] = (f, f, f) and N = F).  Returns float32 [B,H,W,C]: (u A0 + v A1) + (1 - u - v) A2 where
    1 <= id <= F, zeros elsewhere, with a gradient for `attr`, and with rast_grad=True and a `rast` that requires one
    (`rasterize(grad=True)`) for u and v of `rast` too.  Shapes, C and the range of tri are checked once here; the kernels
    index unchecked.  Deterministic: two runs agree bit for bit, backward included."""
    _gpu_only(rast, "interpolate")
    _gpu_only(attr, "interpolate")
    a = attr[None] if attr.dim() == 2 else attr
    if rast.dim() != 4 or rast.shape[-1] != 4 or rast.shape[0] < 1 or rast.shape[1] < 1 or rast.shape[2] < 1:
        raise ValueError(f"interpolate: expected rast [B,H,W,4], got {tuple(rast.shape)}")
    B, H, W, _ = rast.shape
    if a.dim() != 3 or a.shape[0] not in (1, B) or a.shape[1] < 1:
        raise ValueError(f"interpolate: expected attr [N,C], [1,N,C] or [{B},N,C], got {tuple(attr.shape)}")
    C = a.shape[2]
    if C < 1 or C > MAX_CHANNELS:
        raise _lib.MeshDiffusionHipError(f"interpolate takes 1 to {MAX_CHANNELS} channels, got {C} (MD_ERR_UNSUPPORTED)")
    if B > MAX_VIEWS:
        raise _lib.MeshDiffusionHipError(f"interpolate takes at most {MAX_VIEWS} views per call (MD_ERR_UNSUPPORTED)")
    _resolution((H, W))
    dev = rast.device
    a = a.to(device=dev, dtype=torch.float32).contiguous()
    t = _check_tri(tri.to(dev), a.shape[1])
    r = rast.to(torch.float32).contiguous()
    if not rast_grad:
        r = r.detach()
    if _plan is None:
        _plan = _LayerPlan(r.detach(), t.shape[0])
    elif _plan.F != t.shape[0] or _plan.rast.shape != r.shape:
        raise ValueError("interpolate: the plan belongs to another layer")
    return _InterpolateFn.apply(a, r, t, _plan, bool(rast_grad))


class _RenderDepthFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, pos_clip, faces, mvp, campos, H, W, layers=None):
        B, V, F, dev = pos_clip.shape[0], verts.shape[0], faces.shape[0], verts.device
        rast1, rast2 = _rasterize(pos_clip, faces, H, W) if layers is None else layers     # layers: these, rasterised already
        depth1 = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev)
        depth2, mask1, mask2 = torch.empty_like(depth1), torch.empty_like(depth1), torch.empty_like(depth1)
        if F == 0:
            depth1.fill_(20.0), depth2.fill_(-1.0), mask1.zero_(), mask2.zero_()
        else:
            call("md_raster_depth", rast1, rast2, verts, faces, campos, B, V, F, H, W, depth1, depth2, mask1, mask2)
        ctx.save_for_backward(verts, pos_clip, faces, mvp, campos, rast1, rast2)
        ctx.res = (H, W)
        ctx.mark_non_differentiable(mask1, mask2, rast1, rast2)
        return depth1, depth2, mask1, mask2, rast1, rast2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g1, g2, *_unused):
        verts, pos_clip, faces, mvp, campos, rast1, rast2 = ctx.saved_tensors
        H, W = ctx.res
        B, V, F, dev = pos_clip.shape[0], verts.shape[0], faces.shape[0], verts.device
        g1 = torch.zeros((B, H, W), dtype=torch.float32, device=dev) if g1 is None else g1.to(torch.float32).reshape(B, H, W).contiguous()
        g2 = torch.zeros((B, H, W), dtype=torch.float32, device=dev) if g2 is None else g2.to(torch.float32).reshape(B, H, W).contiguous()
        ids = torch.stack([rast1[..., 3], rast2[..., 3]], 1).reshape(-1)        # [B,2,H,W]: the code of an entry is its flat index
        cov = torch.nonzero(ids > 0)[:, 0]
        N = cov.numel()
        dverts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        if N == 0 or F == 0:
            return dverts.zero_(), None, None, None, None, None, None, None
        ptr, order = csr_by_row(faces[ids[cov].to(torch.int64) - 1].reshape(-1), V)     # entry 3 n + corner names this vertex
        cov = cov.to(torch.int32).contiguous()
        corner_grad = torch.empty((N, 3, 3), dtype=torch.float32, device=dev)
        call("md_raster_depth_bwd", cov, N, rast1, rast2, g1, g2, pos_clip, verts, faces, mvp, campos, ptr, order, B, V, F, H, W,
             corner_grad, dverts)
        return dverts, None, None, None, None, None, None, None


# ---- antialiasing ------------------------------------------------------------------------------------------------------------------
def edge_neighbours(faces, n_verts):
    """nbr int32 [F,3] of the antialiasing contract: nbr[f][k] is the vertex opposite the edge (faces[f][(k+1)%3],
    faces[f][(k+2)%3]) in the one other face that owns it, or -1 (boundary, or an edge of three or more faces).  A stable torch
    sort of the 3 F edge keys, then one kernel."""
    _gpu_only(faces, "edge_neighbours")
    n_verts = int(n_verts)
    if n_verts < 1:
        raise ValueError(f"edge_neighbours: n_verts must be positive, got {n_verts}")
    f = _check_faces(faces, n_verts)
    F = f.shape[0]
    nbr = torch.empty((F, 3), dtype=torch.int32, device=f.device)
    if F == 0:
        return nbr
    a, b = f[:, [1, 2, 0]], f[:, [2, 0, 1]]
    keys = (torch.minimum(a, b) * n_verts + torch.maximum(a, b)).reshape(-1)
    keys, order = torch.sort(keys, stable=True)
    call("md_mesh_edge_neighbours", keys, order, f, F, nbr)
    return nbr


class _AntialiasFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, pos_clip, rast, faces, nbr):
        B, H, W, C = color.shape
        V, F = pos_clip.shape[1], faces.shape[0]
        pairs = torch.empty((B, H, W, 2, 4), dtype=torch.int32, device=color.device)
        if F == 0:                                                             # every id is above F: no pair is active
            pairs[..., :2] = -1
            pairs[..., 2:] = 0
            out = color.clone()
        else:
            out = torch.empty_like(color)
            call("md_antialias_pairs", rast, pos_clip, faces, nbr, B, V, F, H, W, pairs)
            call("md_antialias_blend", color, pairs, B, H, W, C, out)
        ctx.save_for_backward(color, pos_clip, pairs)
        ctx.mark_non_differentiable(pairs)
        return out, pairs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _unused):
        color, pos_clip, pairs = ctx.saved_tensors
        B, H, W, C = color.shape
        V, dev = pos_clip.shape[1], color.device
        g = g.to(torch.float32).contiguous()
        dcolor = dpos = None
        if ctx.needs_input_grad[0]:
            dcolor = torch.empty_like(color)
            call("md_antialias_bwd_color", g, pairs, B, H, W, C, dcolor)
        if ctx.needs_input_grad[1]:
            rec = pairs.view(-1, 4)
            act = torch.nonzero(rec[:, 0] >= 0)[:, 0]                          # the flat index of a pair is its code
            N = act.numel()
            dpos = torch.empty((B, V, 4), dtype=torch.float32, device=dev)
            if N == 0:
                dpos.zero_()
            else:
                view = torch.div(act, 2 * H * W, rounding_mode="floor")
                end_vert = (view[:, None] * V + rec[act, :2].to(torch.int64)).reshape(-1)     # entry 2 n + end names this vertex
                ptr, order = csr_by_row(end_vert, B * V)
                vert_grad = torch.empty((N, 2, 3), dtype=torch.float32, device=dev)
                call("md_antialias_bwd_pos", act, N, color, g, pairs, pos_clip, ptr, order, B, V, H, W, C, vert_grad, dpos)
        return dcolor, dpos, None, None, None


def antialias(color, rast, pos_clip, faces, neighbours=None, return_pairs=False):
    """Silhouette antialiasing of `color` float32 [B,H,W,C] (1 <= C <= 8) by the contract in the header comment of
    csrc/antialias.hip, in the manner of dr.antialias: rast float32 [B,H,W,4] one layer of `rasterize`, pos_clip float32 [B,V,4],
    faces [F,3], neighbours = `edge_neighbours(faces, V)` (built when None).  Returns float32 [B,H,W,C] with gradients for
    `color` and `pos_clip` (x, y, w of the silhouette edges' vertices); rast, faces and neighbours get none.
    return_pairs=True also returns the pair records int32 [B,H,W,2,4]: per pixel, for the pair with its right neighbour and the
    pair with the pixel below, (va, vb, the bits of the float32 weight w, P is the pair's first pixel); va = vb = -1: inactive."""
    _gpu_only(color, "antialias")
    if color.dim() != 4 or color.shape[0] < 1 or color.shape[1] < 1 or color.shape[2] < 1:
        raise ValueError(f"antialias: expected color [B,H,W,C], got {tuple(color.shape)}")
    B, H, W, C = color.shape
    if C < 1 or C > MAX_CHANNELS:
        raise _lib.MeshDiffusionHipError(f"antialias takes 1 to {MAX_CHANNELS} channels, got {C} (MD_ERR_UNSUPPORTED)")
    _resolution((H, W))
    _check_clip(pos_clip)
    if tuple(rast.shape) != (B, H, W, 4) or pos_clip.shape[0] != B:
        raise ValueError(f"antialias: expected rast [{B},{H},{W},4] and pos_clip [{B},V,4], got {tuple(rast.shape)} and {tuple(pos_clip.shape)}")
    dev, V = color.device, pos_clip.shape[1]
    col = color.to(torch.float32).contiguous()
    pc = pos_clip.to(device=dev, dtype=torch.float32).contiguous()
    r = rast.detach().to(device=dev, dtype=torch.float32).contiguous()
    f = _check_faces(faces.to(dev), V)
    if neighbours is None:
        nbr = edge_neighbours(f, V)
    else:
        nbr = neighbours.to(device=dev, dtype=torch.int32).contiguous()
        if tuple(nbr.shape) != (f.shape[0], 3):
            raise ValueError(f"antialias: expected neighbours [{f.shape[0]},3], got {tuple(nbr.shape)}")
        if nbr.numel() > 0 and int(nbr.max()) >= V:
            raise ValueError(f"antialias: neighbours name vertices outside [0, {V})")
    out, pairs = _AntialiasFn.apply(col, pc, r, f, nbr)
    return (out, pairs) if return_pairs else out


_antialias = antialias                   # render_depth and make_targets have a flag of that name


def _render_args(what, verts, mvp, campos, resolution):
    """What render_depth and render_buffers check and convert alike: (v float32 [V,3] contiguous, mvp and campos
    detached float32 on v's device, H, W)."""
    _gpu_only(verts, what)
    v = verts[0] if verts.dim() == 3 and verts.shape[0] == 1 else verts
    if v.dim() != 2 or v.shape[-1] != 3 or v.shape[0] < 1:
        raise ValueError(f"{what}: expected verts [V,3] or [1,V,3], got {tuple(verts.shape)}")
    if mvp.dim() != 3 or mvp.shape[1:] != (4, 4) or campos.shape != (mvp.shape[0], 3):
        raise ValueError(f"{what}: expected mvp [B,4,4] and campos [B,3], got {tuple(mvp.shape)} and {tuple(campos.shape)}")
    H, W = _resolution(resolution)
    v = v.to(torch.float32).contiguous()
    mvp = mvp.detach().to(device=v.device, dtype=torch.float32).contiguous()
    campos = campos.detach().to(device=v.device, dtype=torch.float32).contiguous()
    return v, mvp, campos, H, W


def _depth_buffers(rendered, clip=None, f=None, nbr=None):
    """The dict both renderers share, from the six outputs of _RenderDepthFn: depth, mask and rast of both layers and
    rast_triangle_id; with `clip` (pos_clip with the way back to verts) also alpha and alpha_second."""
    depth, depth2, mask, mask2, rast, rast2 = rendered
    tri = torch.unique(rast[..., 3])
    tri = tri[tri > 0].to(torch.int64) - 1
    out = {"depth": depth, "depth_second": depth2, "mask": mask, "mask_second": mask2, "rast": rast, "rast_second": rast2,
           "rast_triangle_id": tri if tri.numel() > 0 else None}
    if clip is not None:
        out["alpha"] = _antialias(mask, rast, clip, f, nbr)
        out["alpha_second"] = _antialias(mask2, rast2, clip, f, nbr)
    return out


def render_depth(verts, faces, mvp, campos, resolution, antialias=False, neighbours=None):
    """The depth part of the reference's render_mesh: world-space verts [V,3] (or [1,V,3]) shared by the B views mvp [B,4,4]
    with camera centres campos [B,3] -> dict of
      depth, depth_second   float32 [B,H,W,1]: |gb_pos - campos| of layer 1 / 2, 20.0 / -1.0 where uncovered; they carry a
                            grad_fn when `verts` requires a gradient (ids held fixed; attribute and barycentric path)
      mask, mask_second     float32 [B,H,W,1]: 1.0 where covered
      rast, rast_second     float32 [B,H,W,4]: (u, v, zf, face index + 1)
      rast_triangle_id      the sorted unique visible face ids of layer 1 (int64), or None when nothing is visible.
    antialias=True adds
      alpha, alpha_second   float32 [B,H,W,1]: `antialias(mask_k, rast_k, xfm_points(verts[None], mvp), faces)`, each layer with
                            its own rast; they carry a grad_fn to `verts` through xfm_points.  neighbours: the prebuilt
                            `edge_neighbours(faces, V)` of a mesh whose faces do not change (`FixedTopoPlan.neighbours`); None
                            builds them, as before the keyword existed.  The bits are the same either way.
    The rasterised tensor is exactly `xfm_points(verts[None], mvp)`."""
    v, mvp, campos, H, W = _render_args("render_depth", verts, mvp, campos, resolution)
    pos_clip = xfm_points(v.detach()[None], mvp).contiguous()
    _check_clip(pos_clip)
    f = _check_faces(faces.to(v.device), v.shape[0])
    rendered = _RenderDepthFn.apply(v, pos_clip, f, mvp, campos, H, W)
    if not antialias:
        return _depth_buffers(rendered)
    clip = xfm_points(v[None], mvp)                                            # the bits of pos_clip, with the way back to verts
    return _depth_buffers(rendered, clip, f, edge_neighbours(f, v.shape[0]) if neighbours is None else neighbours)


# ---- the bsdf == 'normal' renderer -------------------------------------------------------------------------------------------------
NORMAL_THRESHOLD = 0.1                   # renderutils/bsdf.py:13


def _dot(a, b):
    return torch.sum(a * b, -1, keepdim=True)


def _shading_normal(gb_pos, campos, gb_normal, gb_geo_normal):
    """(shading normal, flipped geometric normal)."""
    if campos.dim() == 2:
        campos = campos[:, None, None, :]
    smooth = torch.nn.functional.normalize(gb_normal, dim=-1)
    view = torch.nn.functional.normalize(campos - gb_pos, dim=-1)
    front = _dot(gb_geo_normal, view) > 0
    smooth = torch.where(front, smooth, -smooth)
    geo = torch.where(front, gb_geo_normal, -gb_geo_normal)
    t = torch.clamp(_dot(view, smooth) / NORMAL_THRESHOLD, min=0, max=1)
    return torch.lerp(geo, smooth, t), geo


def shading_normal(gb_pos, campos, gb_normal, gb_geo_normal):
    """The reference's prepare_shading_normal with no tangent, two_sided_shading=True, use_python=True (renderutils/bsdf.py:
    28-54): normalise the smooth normal and the view vector campos - gb_pos, flip both normals where geo . view <= 0, then bend
    with t = clamp(view . smooth / 0.1, 0, 1): lerp(geo, smooth, t).  gb_* [B,H,W,3], campos [B,3] or broadcastable.  Plain torch."""
    return _shading_normal(gb_pos, campos, gb_normal, gb_geo_normal)[0]


def render_buffers(verts, faces, mvp, campos, resolution, v_nrm=None, neighbours=None, corner_csr=None):
    """The reference's render_mesh with `bsdf == 'normal'` on a zero background (render.py:105-106, 177-329): everything
    `render_depth(verts, faces, mvp, campos, resolution, antialias=True)` returns, with equal bits, plus for layer 1 and, under
    names ending in `_second`, for layer 2
      pos          float32 [B,H,W,3]: the interpolated world position; uncovered pixels hold 20.0 (layer 2: -1.0)
      geo_normal   float32 [B,H,W,3]: the interpolation of safe_normalize(f_nrm) with tri = (f, f, f), flipped towards the
                   camera as `shading_normal` flips it; zeros where uncovered
      normal       float32 [B,H,W,3]: `shading_normal` of the interpolated vertex normals, not antialiased; zeros where uncovered
      shaded       float32 [B,H,W,4]: `antialias(cat(((normal + 1) / 2) * mask, mask))` with the layer's own rast; channel 3
                   equals `alpha`.
    `shaded_second` is layer 2's own image; the reference's `shaded_second` repeats layer 1 (render.py:325).
    v_nrm [V,3]: the vertex normals to shade with (`DMTetGeometry.getMesh(normals_grad=True).v_nrm`); None: `dmtet.vertex_normals
    (verts, faces)`.  Gradients reach `verts` through the attribute path, the barycentric path (`rasterize(grad=True)` on
    `xfm_points(verts)`), the vertex normals and the antialiasing.  The rast, tri and CSRs of a layer are built once and shared
    by its interpolations.  neighbours / corner_csr: the prebuilt `edge_neighbours(faces, V)` and `dmtet.face_corner_csr(faces, V)`
    of a mesh whose faces do not change (`FixedTopoPlan`); None builds them, as before the keywords existed, with the same bits."""
    from .dmtet import vertex_normals
    v, mvp, campos, H, W = _render_args("render_buffers", verts, mvp, campos, resolution)
    dev, V = v.device, v.shape[0]
    clip = xfm_points(v[None], mvp).contiguous()                               # the rasterised bits, with the way back to verts
    _check_clip(clip)
    f = _check_faces(faces.to(dev), V)
    F = f.shape[0]
    if v_nrm is None:
        v_nrm, f_nrm = vertex_normals(v, f, csr=corner_csr)
    else:
        if tuple(v_nrm.shape) != (V, 3):
            raise ValueError(f"render_buffers: expected v_nrm [{V},3], got {tuple(v_nrm.shape)}")
        v_nrm = v_nrm.to(device=dev, dtype=torch.float32)
        f_nrm = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    layers, plans = _rasterize_grad(clip, f, H, W)
    rendered = _RenderDepthFn.apply(v, clip.detach(), f, mvp, campos, H, W, (plans[0].rast, plans[1].rast))
    nbr = edge_neighbours(f, V) if neighbours is None else neighbours
    out = _depth_buffers(rendered, clip, f, nbr)
    mask, mask2 = out["mask"], out["mask_second"]
    vert_attr = torch.cat([v, v_nrm], -1)                                      # position and smooth normal in one pass
    geo_attr = f_nrm / torch.sqrt(torch.clamp(_dot(f_nrm, f_nrm), min=1e-20))  # the reference's safe_normalize
    fff = torch.arange(F, dtype=torch.int64, device=dev)[:, None].expand(F, 3).contiguous()
    for k, (r_grad, plan, m, bg, tail) in enumerate(((layers[0], plans[0], mask, 20.0, ""), (layers[1], plans[1], mask2, -1.0, "_second"))):
        gb = interpolate(vert_attr, r_grad, f, rast_grad=True, _plan=plan)
        if F > 0:
            gb_geo = interpolate(geo_attr, plan.rast, fff, _plan=plan)         # face-constant: du = dv = 0
        else:
            gb_geo = torch.zeros_like(gb[..., :3])
        covered = m > 0
        normal, geo = _shading_normal(gb[..., :3], campos, gb[..., 3:], gb_geo)
        zero = torch.zeros_like(normal)
        normal, geo = torch.where(covered, normal, zero), torch.where(covered, geo, zero)
        out["pos" + tail] = torch.where(covered, gb[..., :3], torch.full_like(zero, bg))
        out["geo_normal" + tail], out["normal" + tail] = geo, normal
        out["shaded" + tail] = _antialias(torch.cat([((normal + 1) / 2) * m, m], -1), plan.rast, clip, f, nbr)
    return out


# ---- the targets of a fit (the losses and the loops are in fit.py) ------------------------------------------------------------------
_IN_FIT = ("depth_loss", "depth_loss_fixedtopo", "silhouette_loss", "color_loss", "image_loss", "IMAGE_LOSSES", "lr_schedule_fixedtopo",
           "_select_views", "carve_outside_silhouette", "fit_to_views", "fit_fixed_topology")


def __getattr__(name):
    """The fitting stack moved to fit.py, which imports this module: its names are handed out from there on first use."""
    if name in _IN_FIT:
        from . import fit
        return getattr(fit, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _tonemap_srgb(f):
    return torch.where(f > 0.0031308, torch.pow(torch.clamp(f, min=0.0031308), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * f)


@torch.no_grad()
def make_targets(verts, faces, mvp, campos, resolution, antialias=False, shaded=False):
    """Render the ground-truth mesh with the same rasteriser (the role of dataset_mesh.py:120): `depth`, `depth_second`,
    `mask_cont` [B,H,W,1], and the cameras `mvp`, `campos`, `resolution`; antialias=True adds `alpha`, `alpha_second`;
    shaded=True implies it and adds `img`, `img_second` [B,H,W,4], the `shaded` buffers of `render_buffers`."""
    antialias = antialias or shaded
    if shaded:
        out = render_buffers(verts.detach(), faces, mvp, campos, resolution)
    else:
        out = render_depth(verts.detach(), faces, mvp, campos, resolution, antialias=antialias)
    H, W = _resolution(resolution)
    tgt = {"depth": out["depth"], "depth_second": out["depth_second"], "mask_cont": out["mask"],
           "mvp": mvp.detach().to(device=verts.device, dtype=torch.float32), "campos": campos.detach().to(device=verts.device, dtype=torch.float32),
           "resolution": [H, W]}
    if antialias:
        tgt["alpha"], tgt["alpha_second"] = out["alpha"], out["alpha_second"]
    if shaded:
        tgt["img"], tgt["img_second"] = out["shaded"], out["shaded_second"]
    return tgt


# ---- the fixed-topology second pass (fit_dmtets.py:758-793) --------------------------------------------------------------------------
class _LaplaceUmbrellaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, base, faces, ptr, order):
        V, F, dev = x.shape[0], faces.shape[0], x.device
        term = torch.empty((V, 3), dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.LAPLACE_WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        call("md_laplace_umbrella", x, base, faces, ptr, order, V, F, term, ws, loss)
        ctx.save_for_backward(term, faces, ptr, order)
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        term, faces, ptr, order = ctx.saved_tensors
        V, F = term.shape[0], faces.shape[0]
        g = g.to(torch.float32).reshape(1).contiguous()
        q, dx = torch.empty_like(term), torch.empty_like(term)
        call("md_laplace_umbrella_bwd", term, faces, ptr, order, g, V, F, q, dx)
        return dx, None, None, None, None


def laplace_regularizer_const(v_pos, t_pos_idx, base=None, corner_csr=None):
    """The reference's umbrella Laplacian (regularizer.py:41-60) of y = v_pos - base by the fixed-topology contract in the header
    comment of csrc/fixedtopo.hip: mean over the 3 V components of (sum over the corners naming v of (y_next - y_v) + (y_prev - y_v)
    / max(2 corners, 1))^2, a float32 scalar on the device, differentiable w.r.t. v_pos (`base` gets no gradient).  The reference
    passes the difference v_pos - initial_guess_v_pos; here it is formed inside the kernel.  Gathers in a fixed order instead of
    six scatter_add_: two runs agree bit for bit.  corner_csr: the prebuilt `dmtet.face_corner_csr(t_pos_idx, V)`
    (`FixedTopoPlan.corner_csr`); None builds it and checks the range of the faces."""
    from .dmtet import _check_corner_csr, face_corner_csr
    _gpu_only(v_pos, "laplace_regularizer_const")
    if v_pos.dim() != 2 or v_pos.shape[-1] != 3 or v_pos.shape[0] < 1:
        raise ValueError(f"laplace_regularizer_const: expected v_pos [V,3], got {tuple(v_pos.shape)}")
    if base is not None and tuple(base.shape) != tuple(v_pos.shape):
        raise ValueError(f"laplace_regularizer_const: expected base {tuple(v_pos.shape)}, got {tuple(base.shape)}")
    if t_pos_idx.dim() != 2 or t_pos_idx.shape[-1] != 3 or t_pos_idx.shape[0] < 1:
        raise ValueError(f"laplace_regularizer_const: expected t_pos_idx [F,3] with F >= 1, got {tuple(t_pos_idx.shape)}")
    x = v_pos.to(torch.float32).contiguous()
    V, dev = x.shape[0], x.device
    b = None if base is None else base.detach().to(device=dev, dtype=torch.float32).contiguous()
    if corner_csr is None:
        f = _check_faces(t_pos_idx.to(dev), V)
        ptr, order = face_corner_csr(f, V)
    else:
        if t_pos_idx.shape[0] > MAX_FACES:
            raise _lib.MeshDiffusionHipError("laplace_regularizer_const takes fewer than 2^24 faces (MD_ERR_UNSUPPORTED)")
        f = t_pos_idx.to(device=dev, dtype=torch.int64).contiguous()
        ptr, order = _check_corner_csr(corner_csr, V, f.shape[0], dev, "laplace_regularizer_const")
    return _LaplaceUmbrellaFn.apply(x, b, f, ptr, order)


# ---- the diffuse preview (nvdiffrec/eval.py:421-438) ---------------------------------------------------------------------------------
SH_BAND_WEIGHTS = (1.0, 2 / 3, 2 / 3, 2 / 3, 0.25, 0.25, 0.25, 0.25, 0.25)     # A_l / pi of the cosine lobe, bands 0, 1, 2
PREVIEW_KD = (0.75, 0.3, 0.6)                                                   # eval.py:426
LIGHT_RES = (64, 128)


def sh_basis(d):
    """The nine real spherical harmonics of bands 0-2 at unit directions d [...,3] (numpy float64) -> [...,9], ordered (0,0),
    (1,-1), (1,0), (1,1), (2,-2) .. (2,2), with the six-digit constants of the contract (csrc/meshpost.hip)."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                     0.315392 * (3 * z * z - 1), 1.092548 * x * z, 0.546274 * (x * x - y * y)], -1)


def latlong_directions(h, w):
    """(directions float64 [h,w,3], solid angles float64 [h,w]) of the texel centres of a lat-long map in the reference's
    convention (nvdiffrec/lib/render/util.py:116-117: tu = atan2(x, -z) / 2 pi + 1/2, tv = acos(y) / pi)."""
    theta = (np.arange(h, dtype=np.float64) + 0.5) / h * np.pi
    phi = ((np.arange(w, dtype=np.float64) + 0.5) / w - 0.5) * 2 * np.pi
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    d = np.stack([st * np.sin(phi)[None], np.broadcast_to(ct, (h, w)), -st * np.cos(phi)[None]], -1)
    return d, np.broadcast_to(st * (np.pi / h) * (2 * np.pi / w), (h, w))


def sh9_from_latlong(env):
    """env [h,w,3] (array or tensor), a lat-long radiance map -> float32 numpy [9,3]: L_k = the integral of env * Y_k over the sphere
    by a midpoint quadrature over the texel centres with sin(theta) weights, in float64 on the host.  `shade_diffuse` turns these
    into irradiance over pi, sum_k A_k L_k Y_k(n): a white map gives 1 (to the quadrature's error, 2e-4 at 64 x 128)."""
    e = np.asarray(env.detach().cpu() if torch.is_tensor(env) else env, dtype=np.float64)
    if e.ndim != 3 or e.shape[2] != 3 or e.shape[0] < 1 or e.shape[1] < 1:
        raise ValueError(f"sh9_from_latlong: expected env [h,w,3], got {e.shape}")
    d, dw = latlong_directions(e.shape[0], e.shape[1])
    return np.einsum("hwk,hwc,hw->kc", sh_basis(d), e, dw).astype(np.float32)


def default_sky(d):
    """The analytic sky of `default_light` at unit directions d [...,3] (numpy) -> radiance [...,3]:
        L(d) = ground + (sky - ground) * (0.5 + 0.5 d.y) + sun * max(0, d . s)^2,
    ground = (0.30, 0.28, 0.26), sky = (0.95, 1.00, 1.10), sun = (0.90, 0.85, 0.75), s = (1, 2, 1) / sqrt(6)."""
    ground, sky, sun = np.array([0.30, 0.28, 0.26]), np.array([0.95, 1.00, 1.10]), np.array([0.90, 0.85, 0.75])
    s = np.array([1.0, 2.0, 1.0]) / np.sqrt(6.0)
    up = (0.5 + 0.5 * d[..., 1])[..., None]
    return ground + (sky - ground) * up + sun * (np.maximum(d @ s, 0.0) ** 2)[..., None]


_CONSTANTS = {}


def default_light():
    """The light of `render_preview`: `sh9_from_latlong` of `default_sky` (a ground-to-sky gradient along y plus a soft key light
    from the upper front right) sampled on a 64 x 128 lat-long map.  float32 numpy [9,3], deterministic (computed once, a copy per
    call).  The reference's `.hdr` probe is not shipped; any lat-long `.npy` goes through `sh9_from_latlong` instead."""
    if "light" not in _CONSTANTS:
        _CONSTANTS["light"] = sh9_from_latlong(default_sky(latlong_directions(*LIGHT_RES)[0]))
    return _CONSTANTS["light"].copy()


def _device_constant(values, device):
    """A float32 device tensor of a small host array (kd, the background, a light) or of the default light (values None),
    uploaded once per device and value: a preview per mesh of a batch should not pay a host-to-device copy for each."""
    host = _CONSTANTS["light"] if values is None and "light" in _CONSTANTS else None
    if host is None:
        host = default_light() if values is None else np.ascontiguousarray(values, dtype=np.float32)
    key = (host.tobytes(), host.shape, str(device))
    if key not in _CONSTANTS:
        if len(_CONSTANTS) > 64:                                               # colours come and go; the table stays small
            _CONSTANTS.clear()
        _CONSTANTS[key] = torch.from_numpy(host.copy()).to(device)
    return _CONSTANTS[key]


def preview_camera(angle_ind, resolution, radius=3.0, fovy=np.deg2rad(45.0), near=0.1, far=1000.0, device=None):
    """The reference's rotate_scene (eval.py:182-201): mv = translate(0, 0, -radius) @ (rotate_x(-0.4) @ rotate_y(angle_ind / 50 *
    2 pi)), mvp = perspective(fovy, W / H, near, far) @ mv, campos = inv(mv)[:3, 3].  Returns (mvp [1,4,4], campos [1,3]) float32."""
    H, W = _resolution(resolution)
    mv = translate(0, 0, -radius) @ (rotate_x(-0.4) @ rotate_y((angle_ind / 50) * np.pi * 2))
    mvp = perspective(fovy, W / H, near, far) @ mv
    campos = torch.linalg.inv(mv)[:3, 3]
    return mvp[None].to(device).contiguous(), campos[None].to(device).contiguous()


def shade_diffuse(rast, verts, faces, campos, sh, kd):
    """The shading kernel of the mesh post-processing contract (csrc/meshpost.hip): rast float32 [B,H,W,4] one layer of `rasterize`,
    verts [V,3], faces [F,3], campos [B,3], sh [9,3] (`sh9_from_latlong`), kd [3] -> float32 [B,H,W,4]: kd * max(irradiance / pi, 0)
    at the geometric normal turned towards the camera and alpha 1 where 1 <= id <= F, four zeros elsewhere.  Forward only."""
    _gpu_only(rast, "shade_diffuse")
    _gpu_only(verts, "shade_diffuse")
    if rast.dim() != 4 or rast.shape[-1] != 4 or min(rast.shape[:3]) < 1:
        raise ValueError(f"shade_diffuse: expected rast [B,H,W,4], got {tuple(rast.shape)}")
    B, H, W, _ = rast.shape
    if B > MAX_VIEWS:
        raise _lib.MeshDiffusionHipError(f"shade_diffuse takes at most {MAX_VIEWS} views per call (MD_ERR_UNSUPPORTED)")
    _resolution((H, W))
    if verts.dim() != 2 or verts.shape[-1] != 3:
        raise ValueError(f"shade_diffuse: expected verts [V,3], got {tuple(verts.shape)}")
    dev = rast.device
    v = verts.detach().to(device=dev, dtype=torch.float32).contiguous()
    f = _check_faces(faces.to(dev), v.shape[0])
    cam = torch.as_tensor(campos).detach().to(device=dev, dtype=torch.float32).contiguous()
    s = torch.as_tensor(sh).detach().to(device=dev, dtype=torch.float32).contiguous()
    k = torch.as_tensor(kd).detach().to(device=dev, dtype=torch.float32).contiguous()
    if tuple(cam.shape) != (B, 3) or tuple(s.shape) != (9, 3) or tuple(k.shape) != (3,):
        raise ValueError(f"shade_diffuse: expected campos [{B},3], sh [9,3] and kd [3], got {tuple(cam.shape)}, {tuple(s.shape)} and {tuple(k.shape)}")
    return _shade_diffuse(rast.detach().to(torch.float32).contiguous(), v, f, cam, s, k)


def _shade_diffuse(r, v, f, cam, s, k):
    """shade_diffuse on checked, contiguous float32 / int64 device tensors."""
    B, H, W, _ = r.shape
    if f.shape[0] == 0 or v.shape[0] == 0:                                      # every id is above F
        return torch.zeros((B, H, W, 4), dtype=torch.float32, device=r.device)
    out = torch.empty((B, H, W, 4), dtype=torch.float32, device=r.device)
    call("md_shade_diffuse", r, v, f, cam, s, k, B, v.shape[0], f.shape[0], H, W, out)
    return out


@torch.no_grad()
def render_preview(verts, faces, mvp, campos, resolution, *, kd=PREVIEW_KD, light=None, background=(1.0, 1.0, 1.0), antialias=True):
    """The quick-look image of eval.py:435-438: float32 [B,H,W,3] in [0, 1].  `rasterize` layer 1 of xfm_points(verts, mvp) ->
    `shade_diffuse` (light: sh [9,3], None = `default_light()`) -> the existing `antialias` on the four channels -> rgb + (1 - alpha)
    * background -> the reference's rgb_to_srgb -> clamp.  An empty mesh gives the background."""
    _gpu_only(verts, "render_preview")
    H, W = _resolution(resolution)
    dev = verts.device
    if mvp.dim() != 3 or mvp.shape[1:] != (4, 4) or tuple(campos.shape) != (mvp.shape[0], 3):
        raise ValueError(f"render_preview: expected mvp [B,4,4] and campos [B,3], got {tuple(mvp.shape)} and {tuple(campos.shape)}")
    B = mvp.shape[0]
    if B > MAX_VIEWS:
        raise _lib.MeshDiffusionHipError(f"render_preview takes at most {MAX_VIEWS} views per call (MD_ERR_UNSUPPORTED)")

    def constant(x, shape):
        if torch.is_tensor(x):
            t = x.detach().to(device=dev, dtype=torch.float32).contiguous()
        else:
            t = _device_constant(x, dev)
        if tuple(t.shape) != shape:
            raise ValueError(f"render_preview: expected a constant of shape {shape}, got {tuple(t.shape)}")
        return t

    bg = constant(background, (3,))
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        rgb = bg.expand(B, H, W, 3)
    else:
        v = verts.detach().to(torch.float32).contiguous()
        f = _check_faces(faces.to(dev), v.shape[0])                            # once for the rasteriser and the shading
        m = mvp.detach().to(device=dev, dtype=torch.float32).contiguous()
        cam = campos.detach().to(device=dev, dtype=torch.float32).contiguous()
        clip = xfm_points(v[None], m).contiguous()
        _check_clip(clip)
        rast = _rasterize(clip, f, H, W)[0]
        col = _shade_diffuse(rast, v, f, cam, constant(light, (9, 3)), constant(kd, (3,)))
        if antialias:
            col = _AntialiasFn.apply(col, clip, rast, f, edge_neighbours(f, v.shape[0]))[0]
        rgb = col[..., 0:3] + (1 - col[..., 3:4]) * bg
    return torch.clamp(_tonemap_srgb(rgb), 0.0, 1.0).contiguous()


# ---- the textured render (Texture2D.sample inside the reference's shade, render.py:57-80) ---------------------------------------------
@torch.no_grad()
def textured_fixed(verts, faces, uvs, uv_idx, tex_shape, mvp, campos, resolution, light=None, shade=True):
    """Everything of `render_textured` that does not depend on the texture, for its `_fixed=`: a dict of `rast` (layer 1), `uv`
    float32 [B,H,W,2] (`interpolate(uvs, rast, uv_idx)`), `irradiance` float32 [B,H,W,4] (`shade_diffuse` with kd = 1: rgb and the
    coverage; with shade=False rgb is 1 where covered), `plan` (the `texture.SamplePlan` of uv, rast and tex_shape), and `clip`,
    `faces`, `neighbours` for the antialiasing.  A fit on a fixed mesh and fixed cameras builds it once."""
    from . import texture
    _gpu_only(verts, "render_textured")
    H, W = _resolution(resolution)
    dev = verts.device
    if mvp.dim() != 3 or mvp.shape[1:] != (4, 4) or tuple(campos.shape) != (mvp.shape[0], 3):
        raise ValueError(f"render_textured: expected mvp [B,4,4] and campos [B,3], got {tuple(mvp.shape)} and {tuple(campos.shape)}")
    if verts.dim() != 2 or verts.shape[-1] != 3 or verts.shape[0] < 1 or uvs.dim() != 2 or uvs.shape[-1] != 2 or uvs.shape[0] < 1:
        raise ValueError(f"render_textured: expected verts [V,3] and uvs [N,2], got {tuple(verts.shape)} and {tuple(uvs.shape)}")
    if tuple(uv_idx.shape) != tuple(faces.shape):
        raise ValueError(f"render_textured: uv_idx {tuple(uv_idx.shape)} and faces {tuple(faces.shape)} must have one shape")
    v = verts.detach().to(torch.float32).contiguous()
    f = _check_faces(faces.to(dev), v.shape[0])
    uv_attr = uvs.detach().to(device=dev, dtype=torch.float32).contiguous()
    ui = _check_tri(uv_idx.to(dev), uv_attr.shape[0])
    m = mvp.detach().to(device=dev, dtype=torch.float32).contiguous()
    cam = campos.detach().to(device=dev, dtype=torch.float32).contiguous()
    clip = xfm_points(v[None], m).contiguous()
    _check_clip(clip)
    rast = _rasterize(clip, f, H, W)[0]
    uv = interpolate(uv_attr, rast, ui).contiguous()
    sh = _device_constant(None, dev) if light is None else torch.as_tensor(light).detach().to(device=dev, dtype=torch.float32).contiguous()
    if tuple(sh.shape) != (9, 3):
        raise ValueError(f"render_textured: expected light [9,3], got {tuple(sh.shape)}")
    irr = _shade_diffuse(rast, v, f, cam, sh, torch.ones(3, dtype=torch.float32, device=dev))
    if not shade:
        irr = irr[..., 3:4].expand(-1, -1, -1, 4).contiguous()
    return {"rast": rast, "uv": uv, "irradiance": irr, "plan": texture.SamplePlan(uv, rast, tex_shape), "clip": clip, "faces": f,
            "neighbours": edge_neighbours(f, v.shape[0])}


def render_textured(verts, faces, uvs, uv_idx, tex, mvp, campos, resolution, light=None, shade=True, antialias=True, _fixed=None):
    """The diffuse image of a textured mesh, float32 [B,H,W,4] (rgb, coverage): `rasterize` layer 1 of xfm_points(verts, mvp) ->
    `interpolate(uvs, rast, uv_idx)` -> `texture.sample(tex, uv, rast)` (tex float32 [Ht,Wt,3], boundary clamp) -> times the
    irradiance of `shade_diffuse(kd = 1)` under `light` (sh [9,3], None = `default_light()`; shade=False: the raw kd) -> the existing
    `antialias` on the four channels.  Linear colour, zero background, no tone mapping.  uvs [N,2] and uv_idx [F,3] are any atlas:
    the per-tet one of `DMTet()` or `texture.face_atlas`.  Differentiable in `tex`; the geometry and the irradiance are constants.
    An empty mesh gives zeros.  _fixed: the dict of `textured_fixed` for these arguments, computed once for a fit."""
    from . import texture
    _gpu_only(verts, "render_textured")
    H, W = _resolution(resolution)
    t = tex[0] if tex.dim() == 4 and tex.shape[0] == 1 else tex
    if t.dim() != 3 or t.shape[-1] != 3:
        raise ValueError(f"render_textured: expected tex [Ht,Wt,3], got {tuple(tex.shape)}")
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return torch.zeros((mvp.shape[0], H, W, 4), dtype=torch.float32, device=verts.device)
    fx = _fixed if _fixed is not None else textured_fixed(verts, faces, uvs, uv_idx, t.shape, mvp, campos, (H, W), light, shade)
    if tuple(fx["rast"].shape[1:3]) != (H, W) or fx["rast"].shape[0] != mvp.shape[0]:
        raise ValueError("render_textured: _fixed belongs to other views")
    kd = texture.sample(t, fx["uv"], fx["rast"], plan=fx["plan"])
    irr = fx["irradiance"]
    col = torch.cat([kd * irr[..., :3], irr[..., 3:4]], -1)
    if antialias:
        col = _AntialiasFn.apply(col, fx["clip"], fx["rast"], fx["faces"], fx["neighbours"])[0]
    return col
