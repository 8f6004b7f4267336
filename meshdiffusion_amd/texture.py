"""Textures for meshes on MI355X -- host side of csrc/texture.hip.

The reference bakes `kd` maps with `render_uv`, wraps them in `Texture2D` (nvdiffrec/lib/render/texture.py: `dr.texture` with
filter_mode = 'linear') and writes mesh.obj + mesh.mtl + texture_kd.png (eval.py, fit_singleview.py).  This module is that path
by the texture contract in the header comment of csrc/texture.hip:

  sample            the bilinear fetch, with gradients for the texture and the uv (`SamplePlan` holds the CSR of the texture gradient)
  face_atlas        a compact two-faces-per-tile atlas over the faces of one mesh, tiles a whole number of texels, corners inset
  render_uv         the reference's render_uv without the MLP: position and normals of every texel (`rasterize` + `interpolate`)
  dilate            gutter dilation of a baked atlas
  project_views     the multi-view projection bake of posed images onto the texels
  bake_from_views   face_atlas -> render_uv -> render_depth -> project_views -> fill -> dilate
  save_textured_obj mesh.obj with vt lines + mesh.mtl + the PNG

Orientation.  Texel (row i, column j) has its centre at (u, v) = ((j + 0.5) / Wt, (i + 0.5) / Ht): row 0 is v = 0, which is what a
rasterisation at the clip position (2 u - 1, 2 v - 1, 0, 1) gives, so a baked texel and a sampled texel coincide.  The kernels run
on the GPU only: a CPU tensor is an error, not a fallback.  `face_atlas` and `save_textured_obj` are host code and run anywhere.

Not built: mip maps and trilinear filtering, cube maps, ks / normal maps, MLP textures, chart-based
unwrapping and seam-aware filtering, gradients of the projection, inpainting of texels no view saw.
"""
import math
import os

import numpy as np
import torch

from . import _lib
from ._csr import csr_by_row
from .hip_ops import _gpu_only, call

MAX_RES, MAX_VIEWS, MAX_CHANNELS = 2048, 64, 8       # MD_TEXTURE_MAX_RES, MD_TEXTURE_MAX_VIEWS, RS_MAX_CHANNELS
BOUNDARY = {"clamp": 0, "wrap": 1}                   # MD_TEXTURE_CLAMP, MD_TEXTURE_WRAP


def _f32(t, device=None):
    """float32, contiguous, 16-byte aligned (a contiguous view into a larger storage may start anywhere)."""
    t = t.to(device=device, dtype=torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _boundary(boundary):
    if boundary not in BOUNDARY:
        raise ValueError(f"texture: boundary must be 'clamp' or 'wrap', got {boundary!r}")
    return BOUNDARY[boundary]


def _check_sample_shapes(what, tex_shape, uv_shape, rast_shape):
    if len(uv_shape) != 4 or uv_shape[-1] != 2 or min(uv_shape[:3]) < 1:
        raise ValueError(f"{what}: expected uv [B,H,W,2], got {tuple(uv_shape)}")
    B, H, W, _ = uv_shape
    if len(tex_shape) != 4 or tex_shape[0] not in (1, B) or tex_shape[1] < 1 or tex_shape[2] < 1:
        raise ValueError(f"{what}: expected tex [Ht,Wt,C], [1,Ht,Wt,C] or [{B},Ht,Wt,C], got {tuple(tex_shape)}")
    if rast_shape is not None and tuple(rast_shape) != (B, H, W, 4):
        raise ValueError(f"{what}: expected rast [{B},{H},{W},4], got {tuple(rast_shape)}")
    T, Ht, Wt, C = tex_shape
    if C < 1 or C > MAX_CHANNELS:
        raise _lib.MeshDiffusionHipError(f"{what} takes 1 to {MAX_CHANNELS} channels, got {C} (MD_ERR_UNSUPPORTED)")
    if Ht > MAX_RES or Wt > MAX_RES or H > MAX_RES or W > MAX_RES:
        raise _lib.MeshDiffusionHipError(f"{what}: texture {(Ht, Wt)} or image {(H, W)} exceeds {MAX_RES} (MD_ERR_UNSUPPORTED)")
    if B > MAX_VIEWS:
        raise _lib.MeshDiffusionHipError(f"{what} takes at most {MAX_VIEWS} views per call (MD_ERR_UNSUPPORTED)")


def _stamp(uv, rast):
    return (tuple(uv.shape), uv.data_ptr(), uv._version) + ((None,) if rast is None else (rast.data_ptr(), rast._version))


class SamplePlan:
    """The CSR of the texture gradient of one (uv, rast, texture shape, boundary): the (pixel, corner) codes sorted stably by the
    texel they name.  It depends on nothing else, so a fit on a fixed mesh and fixed cameras builds it once and passes it to
    `sample` every iteration.  `sample` takes a plan only with the very tensors it was built from (the same storage, not written
    since: `data_ptr` and `_version` of the contiguous float32 uv and rast), so a plan of other values cannot give a wrong gradient
    silently.  Built at the first backward that needs it (one kernel, a stable torch sort, a searchsorted)."""

    def __init__(self, uv, rast, tex_shape, boundary="clamp"):
        _gpu_only(uv, "SamplePlan")
        tex_shape = tuple(int(s) for s in tex_shape)
        if len(tex_shape) == 3:
            tex_shape = (1,) + tex_shape
        _check_sample_shapes("SamplePlan", tex_shape, tuple(uv.shape), None if rast is None else tuple(rast.shape))
        self.boundary = boundary
        self.mode = _boundary(boundary)
        self.uv = _f32(uv.detach())
        self.rast = None if rast is None else _f32(rast.detach(), self.uv.device)
        self.tex_shape = tex_shape
        self._csr = None
        self._stamp = _stamp(self.uv, self.rast)

    def belongs_to(self, uv, rast, tex_shape, mode):
        """uv, rast: contiguous float32 device tensors (rast or None)."""
        return (tuple(tex_shape[:3]), mode, _stamp(uv, rast)) == (self.tex_shape[:3], self.mode, self._stamp)

    def csr(self):
        """(ptr int32 [T Ht Wt + 2], order int32 [4 B H W]); the last row collects the codes of the skipped pixels."""
        if self._csr is None:
            B, H, W, _ = self.uv.shape
            T, Ht, Wt = self.tex_shape[:3]
            dest = torch.empty(B * H * W * 4, dtype=torch.int32, device=self.uv.device)
            call("md_texture_codes", self.uv, self.rast, T, Ht, Wt, B, H, W, self.mode, dest)
            self._csr = csr_by_row(dest, T * Ht * Wt + 1)
        return self._csr


class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, rast, plan):
        T, Ht, Wt, C = tex.shape
        B, H, W, _ = uv.shape
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=uv.device)
        call("md_texture_sample", tex, uv, rast, T, Ht, Wt, C, B, H, W, plan.mode, out)
        ctx.plan = plan
        ctx.save_for_backward(tex, uv, rast)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        tex, uv, rast = ctx.saved_tensors
        T, Ht, Wt, C = tex.shape
        B, H, W, _ = uv.shape
        need_tex, need_uv = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_tex or need_uv):
            return None, None, None, None
        g = _f32(g)
        dtex = torch.empty_like(tex) if need_tex else None
        duv = torch.empty_like(uv) if need_uv else None
        ptr, order = ctx.plan.csr() if need_tex else (None, None)
        call("md_texture_sample_bwd", tex, uv, rast, g, ptr, order, T, Ht, Wt, C, B, H, W, ctx.plan.mode, dtex, duv)
        return dtex, duv, None, None


def sample(tex, uv, rast=None, boundary="clamp", plan=None):
    """dr.texture with filter_mode = 'linear' by the texture contract in the header comment of csrc/texture.hip: tex float32
    [Ht,Wt,C], [1,Ht,Wt,C] (shared by the views) or [B,Ht,Wt,C], 1 <= C <= 8, Ht, Wt <= 2048; uv float32 [B,H,W,2]; rast [B,H,W,4]
    one layer of `rasterize`, or None.  Returns float32 [B,H,W,C]: the bilinear fetch, zeros where the rast id is 0 or the uv is not
    finite, with gradients for `tex` and `uv` (rast gets none).  boundary: 'clamp' or 'wrap'.  plan: the `SamplePlan` built from these
    very uv and rast tensors, this texture shape and boundary (anything else raises); None builds one for this call.  Deterministic: two runs agree bit for bit, backward
    included, and a reused plan gives the same bits as none."""
    _gpu_only(uv, "texture.sample")
    _gpu_only(tex, "texture.sample")
    t = tex[None] if tex.dim() == 3 else tex
    _check_sample_shapes("texture.sample", tuple(t.shape), tuple(uv.shape), None if rast is None else tuple(rast.shape))
    dev = uv.device
    t, u = _f32(t, dev), _f32(uv)
    if plan is None:
        plan = SamplePlan(u, rast, t.shape, boundary)
    elif not plan.belongs_to(u, None if rast is None else _f32(rast.detach(), dev), tuple(t.shape), _boundary(boundary)):
        raise ValueError("texture.sample: the plan was built from another uv or rast (or they were written since), another texture "
                         "shape or another boundary; pass the contiguous float32 tensors the plan was built from")
    return _SampleFn.apply(t, u, plan.rast, plan)


# ---- the atlas -----------------------------------------------------------------------------------------------------------------------
def atlas_layout(n_faces, resolution):
    """(tiles per side, tile side in texels) of `face_atlas`: ceil(sqrt(ceil(F / 2))) tiles per side, each floor(resolution / that)
    texels wide."""
    n_tiles = (int(n_faces) + 1) // 2
    per_side = max(1, int(math.ceil(math.sqrt(n_tiles))))
    while per_side * per_side < n_tiles:                                       # the float sqrt of a large count may round down
        per_side += 1
    return per_side, int(resolution) // per_side


def face_atlas(n_faces, resolution, gutter=1):
    """A compact atlas over the faces of one mesh: (uvs float32 [4 * ceil(F / 2), 2], uv_idx int64 [F, 3]) on the CPU.

    Faces 2 k and 2 k + 1 share the square tile k, in the layout and the corner order of `dmtet._map_uv`: the tile's four uvs are
    (x0, y0), (x1, y0), (x1, y1), (x0, y1), the even face takes corners (0, 1, 2), the odd one (0, 2, 3).  Unlike the per-tet atlas of
    `DMTet()`, the tiles run over the faces of this mesh only, a tile is a whole number s = floor(resolution / n) of texels wide (n =
    ceil(sqrt(ceil(F / 2))) tiles per side, tile k at texel column (k mod n) s, row (k div n) s), and the corners sit `gutter`
    texels inside it: x0 = (col s + gutter) / resolution, x1 = (col s + s - gutter) / resolution.  A covered texel (centre inside
    the square) then has at least `gutter` texels between it and the tile's border, and the bilinear footprint of any uv inside the
    square stays inside the tile.  Raises when s < 2 gutter + 2, the smallest tile in which both faces own a texel centre."""
    F, R, g = int(n_faces), int(resolution), int(gutter)
    if F < 1 or R < 1 or g < 0:
        raise ValueError(f"face_atlas: expected n_faces >= 1, resolution >= 1 and gutter >= 0, got {(F, R, g)}")
    if R > MAX_RES:
        raise _lib.MeshDiffusionHipError(f"face_atlas: resolution {R} exceeds {MAX_RES} (MD_ERR_UNSUPPORTED)")
    n, s = atlas_layout(F, R)
    if s < 2 * g + 2:
        raise ValueError(f"face_atlas: {F} faces at resolution {R} give tiles of {s} texels, below the {2 * g + 2} that a gutter of "
                         f"{g} needs; raise the resolution or lower the gutter")
    n_tiles = (F + 1) // 2
    k = np.arange(n_tiles, dtype=np.int64)
    col, row = (k % n) * s, (k // n) * s
    x0, x1 = (col + g).astype(np.float64) / R, (col + s - g).astype(np.float64) / R
    y0, y1 = (row + g).astype(np.float64) / R, (row + s - g).astype(np.float64) / R
    uvs = np.stack([x0, y0, x1, y0, x1, y1, x0, y1], -1).reshape(-1, 2).astype(np.float32)
    f = np.arange(F, dtype=np.int64)
    tile, odd = f // 2, f % 2
    uv_idx = np.stack([tile * 4, tile * 4 + odd + 1, tile * 4 + odd + 2], -1)
    return torch.from_numpy(uvs), torch.from_numpy(uv_idx)


def render_uv(verts, faces, uvs, uv_idx, resolution, v_nrm=None):
    """The reference's render_uv (render.py:338-360) without the MLP: rasterise the mesh in uv space, at the clip position (2 uv - 1,
    0, 1) with `uv_idx`, and interpolate the world-space attributes with `faces`.  Returns a dict of
      mask        float32 [Ht,Wt]: 1.0 where a face covers the texel's centre
      pos         float32 [Ht,Wt,3]: the surface point of the texel; zeros where uncovered
      normal      float32 [Ht,Wt,3]: the interpolated vertex normals (v_nrm [V,3], None: `dmtet.vertex_normals`), unit length
      geo_normal  float32 [Ht,Wt,3]: the unit face normal
      face_id     int64 [Ht,Wt]: the face, -1 where uncovered
      rast        float32 [1,Ht,Wt,4]: the layer itself."""
    from .dmtet import vertex_normals
    from .render import _check_faces, _resolution, interpolate, rasterize
    _gpu_only(verts, "render_uv")
    if verts.dim() != 2 or verts.shape[-1] != 3 or verts.shape[0] < 1:
        raise ValueError(f"render_uv: expected verts [V,3], got {tuple(verts.shape)}")
    if uvs.dim() != 2 or uvs.shape[-1] != 2 or uvs.shape[0] < 1:
        raise ValueError(f"render_uv: expected uvs [N,2], got {tuple(uvs.shape)}")
    if tuple(uv_idx.shape) != tuple(faces.shape):
        raise ValueError(f"render_uv: uv_idx {tuple(uv_idx.shape)} and faces {tuple(faces.shape)} must have one shape")
    Ht, Wt = _resolution(resolution)
    dev = verts.device
    v = verts.detach().to(torch.float32).contiguous()
    f = _check_faces(faces.to(dev), v.shape[0])
    uv = uvs.detach().to(device=dev, dtype=torch.float32)
    ui = _check_faces(uv_idx.to(dev), uv.shape[0])
    F = f.shape[0]
    if F == 0:
        z3 = torch.zeros((Ht, Wt, 3), dtype=torch.float32, device=dev)
        return {"mask": z3[..., 0].clone(), "pos": z3, "normal": z3.clone(), "geo_normal": z3.clone(),
                "face_id": torch.full((Ht, Wt), -1, dtype=torch.int64, device=dev),
                "rast": torch.zeros((1, Ht, Wt, 4), dtype=torch.float32, device=dev)}
    if v_nrm is None:
        v_nrm, f_nrm = vertex_normals(v, f)
    else:
        v_nrm = v_nrm.detach().to(device=dev, dtype=torch.float32)
        f_nrm = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    clip = torch.cat([uv * 2 - 1, torch.zeros_like(uv[:, :1]), torch.ones_like(uv[:, :1])], -1)[None].contiguous()
    rast = rasterize(clip, ui, (Ht, Wt), num_layers=1)[0]
    gb = interpolate(torch.cat([v, v_nrm.detach()], -1), rast, f)[0]
    geo_attr = f_nrm.detach() / torch.sqrt(torch.clamp((f_nrm.detach() ** 2).sum(-1, keepdim=True), min=1e-20))
    fff = torch.arange(F, dtype=torch.int64, device=dev)[:, None].expand(F, 3).contiguous()
    geo = interpolate(geo_attr, rast, fff)[0]
    ids = rast[0, ..., 3]
    covered = (ids >= 1) & (ids <= F)
    nrm = gb[..., 3:] / torch.sqrt(torch.clamp((gb[..., 3:] ** 2).sum(-1, keepdim=True), min=1e-20))
    zero = torch.zeros_like(nrm)
    return {"mask": covered.to(torch.float32), "pos": torch.where(covered[..., None], gb[..., :3], zero).contiguous(),
            "normal": torch.where(covered[..., None], nrm, zero).contiguous(),
            "geo_normal": torch.where(covered[..., None], geo, zero).contiguous(),
            "face_id": torch.where(covered, ids.to(torch.int64) - 1, torch.full_like(ids, -1, dtype=torch.int64)), "rast": rast}


# ---- baking ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def dilate(tex, mask, steps):
    """`steps` dilation steps of the contract: tex float32 [Ht,Wt,C], mask [Ht,Wt] (covered: > 0.5).  In each step an uncovered texel
    with a covered 8-neighbour becomes the mean of those neighbours and covered.  Returns (tex, mask float32); steps = 0 returns
    float32 copies."""
    _gpu_only(tex, "texture.dilate")
    if tex.dim() != 3 or min(tex.shape) < 1 or tuple(mask.shape) != tuple(tex.shape[:2]):
        raise ValueError(f"texture.dilate: expected tex [Ht,Wt,C] and mask [Ht,Wt], got {tuple(tex.shape)} and {tuple(mask.shape)}")
    Ht, Wt, C = tex.shape
    if C > MAX_CHANNELS or Ht > MAX_RES or Wt > MAX_RES:
        raise _lib.MeshDiffusionHipError(f"texture.dilate takes up to {MAX_CHANNELS} channels and {MAX_RES} texels a side (MD_ERR_UNSUPPORTED)")
    t, m = _f32(tex.detach()).clone(), _f32(mask.detach(), tex.device).clone()
    for _ in range(int(steps)):
        t2, m2 = torch.empty_like(t), torch.empty_like(m)
        call("md_texture_dilate", t, m, Ht, Wt, C, t2, m2)
        t, m = t2, m2
    return t, m


@torch.no_grad()
def project_views(bake, images, depth, viewmask, mvp, campos, depth_bias=0.01, cos_min=0.1, power=2.0):
    """The projection bake of the contract.  bake: the dict of `render_uv` (`pos`, `normal`, `mask`); images float32 [V,H,W,3];
    depth [V,H,W] or [V,H,W,1], the layer-1 `depth` of `render_depth` for the same cameras (the distance to the camera); viewmask
    [V,H,W] or [V,H,W,1]; mvp [V,4,4]; campos [V,3]; V <= 64.  A view colours a texel when the texel projects inside it onto four
    foreground pixels, is no further than depth_bias behind the view's depth and faces the camera with cos > cos_min; its weight is
    cos ** power.  Returns (color float32 [Ht,Wt,3], weight float32 [Ht,Wt]), zeros where no view counts.  No gradient."""
    pos, nrm, tmask = bake["pos"], bake["normal"], bake["mask"]
    _gpu_only(pos, "texture.project_views")
    dev = pos.device
    if pos.dim() != 3 or pos.shape[-1] != 3 or tuple(nrm.shape) != tuple(pos.shape) or tuple(tmask.shape) != tuple(pos.shape[:2]):
        raise ValueError("texture.project_views: expected the pos [Ht,Wt,3], normal [Ht,Wt,3] and mask [Ht,Wt] of render_uv")
    Ht, Wt, _ = pos.shape
    if images.dim() != 4 or images.shape[-1] != 3 or min(images.shape[:3]) < 1:
        raise ValueError(f"texture.project_views: expected images [V,H,W,3], got {tuple(images.shape)}")
    V, H, W, _ = images.shape
    d = depth[..., 0] if depth.dim() == 4 else depth
    vm = viewmask[..., 0] if viewmask.dim() == 4 else viewmask
    if tuple(d.shape) != (V, H, W) or tuple(vm.shape) != (V, H, W) or tuple(mvp.shape) != (V, 4, 4) or tuple(campos.shape) != (V, 3):
        raise ValueError(f"texture.project_views: expected depth and viewmask [{V},{H},{W}], mvp [{V},4,4] and campos [{V},3], got "
                         f"{tuple(depth.shape)}, {tuple(viewmask.shape)}, {tuple(mvp.shape)} and {tuple(campos.shape)}")
    if V > MAX_VIEWS or max(Ht, Wt, H, W) > MAX_RES:
        raise _lib.MeshDiffusionHipError(f"texture.project_views takes at most {MAX_VIEWS} views and {MAX_RES} pixels a side (MD_ERR_UNSUPPORTED)")
    color = torch.empty((Ht, Wt, 3), dtype=torch.float32, device=dev)
    weight = torch.empty((Ht, Wt), dtype=torch.float32, device=dev)
    call("md_texture_project", _f32(pos.detach()), _f32(nrm.detach()), _f32(tmask.detach()), _f32(images.detach(), dev),
         _f32(d.detach(), dev), _f32(vm.detach(), dev), _f32(mvp.detach(), dev), _f32(campos.detach(), dev), Ht, Wt, V, H, W,
         float(depth_bias), float(cos_min), float(power), color, weight)
    return color, weight


@torch.no_grad()
def bake_from_views(verts, faces, images, viewmask, mvp, campos, resolution, gutter=1, fill=(0.5, 0.5, 0.5)):
    """Posed images -> a texture for the mesh: `face_atlas(F, resolution, gutter)`, `render_uv`, `render_depth` at the images' size for
    the visibility depth, `project_views`; covered texels no view saw get `fill`; then `gutter` steps of `dilate`.  Square atlas.
    Returns a dict of `uvs` float32 [4 ceil(F / 2), 2], `uv_idx` int64 [F,3], `tex` float32 [R,R,3] and `weight` float32 [R,R] (the
    projection weights before the fill), all on the device of `verts`."""
    from .render import render_depth
    _gpu_only(verts, "texture.bake_from_views")
    dev = verts.device
    R = int(resolution)
    uvs, uv_idx = face_atlas(faces.shape[0], R, gutter)
    uvs, uv_idx = uvs.to(dev), uv_idx.to(dev)
    bake = render_uv(verts, faces, uvs, uv_idx, R)
    H, W = images.shape[1], images.shape[2]
    depth = render_depth(verts.detach(), faces, mvp, campos, (H, W))["depth"]
    color, weight = project_views(bake, images, depth, viewmask, mvp, campos)
    unseen = (bake["mask"] > 0.5) & ~(weight > 0)
    color = torch.where(unseen[..., None], torch.tensor(fill, dtype=torch.float32, device=dev).expand_as(color), color)
    tex, _ = dilate(color, bake["mask"], gutter)
    return {"uvs": uvs, "uv_idx": uv_idx, "tex": tex, "weight": weight}


# ---- export ----------------------------------------------------------------------------------------------------------------------
def save_textured_obj(path, verts, faces, uvs, uv_idx, tex, decimal_places=None):
    """Write `path` (mesh.obj) with `v`, `vt` and `f v/vt` lines, `<stem>.mtl` next to it with one material whose `map_Kd` names
    `<stem>_kd.png`, and that PNG (`mesh_export.save_png`: 8 bits, rint(clip(x, 0, 1) * 255)).  Returns the three paths.

    Convention.  Row 0 of `tex` is v = 0 (the texture contract) and `save_png` writes row 0 as the top line of the image, unflipped.
    A Wavefront `vt` puts v = 0 at the BOTTOM line of the image, so the file holds `vt u (1 - v)`: a viewer then finds the texel
    this module samples at (u, v).  The `v` lines and the vertex indices of the `f` lines equal those of `mesh_export.save_obj` for
    the same mesh."""
    from .mesh_export import save_png
    v = torch.as_tensor(verts).detach().cpu().numpy().astype(np.float64)
    f = torch.as_tensor(faces).detach().cpu().numpy().astype(np.int64) + 1
    uv = torch.as_tensor(uvs).detach().cpu().numpy().astype(np.float64)
    ui = torch.as_tensor(uv_idx).detach().cpu().numpy().astype(np.int64) + 1
    t = torch.as_tensor(tex).detach().cpu()
    if f.ndim != 2 or f.shape[1] != 3 or ui.shape != f.shape or uv.ndim != 2 or uv.shape[1] != 2:
        raise ValueError(f"save_textured_obj: expected faces and uv_idx [F,3] and uvs [N,2], got {f.shape}, {ui.shape} and {uv.shape}")
    if f.shape[0] > 0 and (ui.min() < 1 or ui.max() > uv.shape[0]):
        raise ValueError(f"save_textured_obj: uv_idx names uvs outside [0, {uv.shape[0]})")
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or t.shape[-1] != 3:
        raise ValueError(f"save_textured_obj: expected tex [Ht,Wt,3], got {tuple(t.shape)}")
    stem = os.path.splitext(path)[0]
    mtl, png = stem + ".mtl", stem + "_kd.png"
    fmt = "%f" if decimal_places is None else f"%.{int(decimal_places)}f"
    with open(path, "w") as fh:
        fh.write("mtllib %s\n" % os.path.basename(mtl))
        for row in v:
            fh.write("v " + " ".join(fmt % c for c in row) + "\n")
        for row in uv:
            fh.write("vt " + fmt % row[0] + " " + fmt % (1.0 - row[1]) + "\n")
        fh.write("usemtl material_0\n")
        for a, b in zip(f, ui):
            fh.write("f %d/%d %d/%d %d/%d\n" % (a[0], b[0], a[1], b[1], a[2], b[2]))
    with open(mtl, "w") as fh:
        fh.write("newmtl material_0\nKa 0.000000 0.000000 0.000000\nKd 1.000000 1.000000 1.000000\nKs 0.000000 0.000000 0.000000\n"
                 "illum 1\nmap_Kd %s\n" % os.path.basename(png))
    save_png(png, t)
    return path, mtl, png
