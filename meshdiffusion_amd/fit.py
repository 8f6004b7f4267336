"""The DMTet fitting stack: the loss terms, the carves, the four fitting loops and the setup their command lines share.

Plain torch around the kernels of `render`, `pointcloud`, `dmtet` and `singleview`; nothing here launches a kernel of its own.
The four loops supervise a `DMTetGeometry` (or, `fit_fixed_topology`, a `DMTetGeometryFixedTopo`) the way the reference's ticks do:

  fit_to_points        chamfer + SDF regulariser, no renderer (nvdiffrec/lib/geometry/dmtet.py:441-459)
  fit_to_views         the depth terms, the carve and the image terms of DMTetGeometry.tick (dmtet.py:366-434)
  fit_fixed_topology   pass 2 of the fit (fit_dmtets.py:758-793, dmtet_fixedtopo.py:318-337)
  fit_single_view      the single-view loop (fit_singleview.py:489-502 around dmtet_singleview.py:438-516)

Each is a step function handed to `_optimise`, which owns what they share: zero_grad -> step(it) -> backward -> opt.step [->
sched.step] -> clamp_deform -> the history of the detached terms -> callback(it, headline term, mesh) -> the stacked history.  The
pieces of a step that more than one loop needs are written once: `_masked_sdf_reg`, `_chamfer_term`, `_pre_step`, `_huber_depth`,
`_vertex_pixels`, `_layer1_image_terms`, `_need_targets`, `_get_mesh`.  `fit_texture` runs the same driver on a `kd` texture of a fixed mesh (`render.render_textured`).  `render`, `pointcloud` and `singleview` hand out the
public names below under their old addresses.  tools/fit_views.py, fit_singleview.py and fit_pointcloud.py build their command
lines from `add_fit_arguments`, `load_normalised_obj`, `look_at_cameras`, `make_geometry`, `progress` and `second_pass`.
"""
import math
import os

import numpy as np
import torch

from . import _lib
from .dmtet import DMTetGeometry, DMTetGeometryFixedTopo, sdf_reg_loss
from .hip_ops import _gpu_only
from .pointcloud import chamfer_distance, sample_points
from .render import (_tonemap_srgb, laplace_regularizer_const, perspective, render_buffers, render_depth, rotate_x, rotate_y,
                     translate, xfm_points)
from .singleview import init_with_gt_surface


# ---- the loss terms ----------------------------------------------------------------------------------------------------------------
def _huber(d):
    """Huber at 1 for d >= 0: d below 1, d^2 from there."""
    return torch.where(d < 1.0, d, d * d)


def _huber_depth(buffers, target, layers, exact_mask, scale):
    """scale * the sum over layers = ((key, second_layer_gate, factor), ...) of mean(huber(d)),
        d = |buffers[key] - target[key]| * mask * [target depth_second >= 0] [* [|target depth_second - target depth| >= 5e-3]] [* factor],
    mask = [mask_cont == 1] (exact_mask) or `mask_cont` as it is.  The gates are 0 / 1, so their grouping does not change a bit."""
    mask = target["mask_cont"][..., 0]
    mask = ((mask == 1.0).float() if exact_mask else mask).unsqueeze(-1)
    valid = (target["depth_second"] >= 0).float()
    both = valid * ((target["depth_second"] - target["depth"]).abs() >= 5e-3).float()
    total = None
    for key, second_layer_gate, factor in layers:
        d = (buffers[key][..., :1] - target[key][..., :1]).abs() * mask * (both if second_layer_gate else valid)
        term = _huber(d if factor is None else d * factor).mean()
        total = term if total is None else total + term
    return total * scale


def depth_loss(buffers, target, iteration):
    """The depth terms of DMTetGeometry.tick (dmtet.py:402-434) with no_depth_thin: elementwise torch.
    buffers: `depth`, `depth_second`; target: `depth`, `depth_second`, `mask_cont`, all [B,H,W,1]."""
    return _huber_depth(buffers, target, (("depth", False, None), ("depth_second", True, 0.1)), True, 100.0 if iteration < 10000 else 1.0)


def depth_loss_fixedtopo(buffers, target):
    """The depth term of DMTetGeometryFixedTopo.tick (dmtet_fixedtopo.py:326-337) as written there: the line that forms the
    layer-1 difference (:333) is overwritten by the next one (:334), so the term is the SECOND layer only,
        d = |depth_second - target depth_second| * mask * [target depth_second >= 0] * [|target depth_second - target depth| >= 5e-3] * 0.1,
    Huber at 1 (d below 1, d^2 from there), mean, times 100; `buffers['depth']` does not enter.  Kept, not fixed.  The mask is
    `target['mask_cont'][..., 0]` (the reference's `target['mask']`) as it is.  Elementwise torch."""
    return _huber_depth(buffers, target, (("depth_second", True, 1e-1),), False, 100.0)


def depth_loss_single_view(buffers, target):
    """The depth term of the single-view tick (dmtet_singleview.py:474-490): layer 1 only,
        d = |depth - target depth| * [mask_cont == 1] * [target depth_second >= 0] * [|target depth_second - target depth| >= 5e-3],
    Huber at 1 (d below 1, d^2 from there), mean, times 100.  Elementwise torch."""
    return _huber_depth(buffers, target, (("depth", True, None),), True, 100.0)


def silhouette_loss(buffers, target):
    """The coverage term of DMTetGeometry.tick (dmtet.py:394,399): mse(alpha) + 0.1 mse(alpha_second), all [B,H,W,1]."""
    mse = torch.nn.functional.mse_loss
    return mse(buffers["alpha"], target["alpha"]) + 0.1 * mse(buffers["alpha_second"], target["alpha_second"])


IMAGE_LOSSES = ("smape", "mse", "logl1", "logl2", "relmse")


def image_loss(img, ref, kind):
    """The reference's createLoss(kind)(img, ref) (fit_dmtets.py:65-77, renderutils/loss.py): `smape`, `mse`, `relmse` on the
    images as they are, `logl1` / `logl2` the L1 / MSE of tonemap_srgb(log(clamp(x, 0, 65535) + 1)).  Plain torch."""
    if kind not in IMAGE_LOSSES:
        raise ValueError(f"image_loss: kind must be one of {IMAGE_LOSSES}, got {kind!r}")
    if kind in ("logl1", "logl2"):
        img = _tonemap_srgb(torch.log(torch.clamp(img, min=0, max=65535) + 1))
        ref = _tonemap_srgb(torch.log(torch.clamp(ref, min=0, max=65535) + 1))
    if kind in ("mse", "logl2"):
        return torch.nn.functional.mse_loss(img, ref)
    if kind == "smape":
        return torch.mean(torch.abs(img - ref) / (torch.abs(img) + torch.abs(ref) + 0.01))
    if kind == "relmse":
        return torch.mean((img - ref) * (img - ref) / (img * img + ref * ref + 0.1))
    return torch.nn.functional.l1_loss(img, ref)


def _masked_color(shaded, ref, kind):
    return image_loss(shaded[..., 0:3] * ref[..., 3:], ref[..., 0:3] * ref[..., 3:], kind)


def color_loss(buffers, target, kind="logl1"):
    """The colour term of DMTetGeometry.tick (dmtet.py:395,400): image_loss(shaded rgb x ref alpha, ref rgb x ref alpha) of layer
    1 plus 0.1 times that of `shaded_second` / `img_second`.  The alpha terms of those lines are `silhouette_loss`."""
    return (_masked_color(buffers["shaded"], target["img"], kind)
            + 0.1 * _masked_color(buffers["shaded_second"], target["img_second"], kind))


def _layer1_image_terms(coverage, ref_coverage, shaded, ref, kind):
    """(alpha, colour) of layer 1 alone, as the fixed-topology and single-view ticks take them (dmtet_fixedtopo.py:318-322):
    mse(coverage, ref_coverage) and image_loss(shaded rgb x ref alpha, ref rgb x ref alpha); a term whose reference is None is None."""
    alpha = None if ref_coverage is None else torch.nn.functional.mse_loss(coverage, ref_coverage)
    return alpha, None if ref is None else _masked_color(shaded, ref, kind)


def sdf_regularizer_weight(iteration, iters, sdf_regularizer):
    """dmtet.py:440-441: falls linearly from `sdf_regularizer` to 0.01 over the first quarter of the run."""
    return sdf_regularizer - (sdf_regularizer - 0.01) * min(1.0, 4.0 * (iteration / iters))


def lr_schedule_fixedtopo(it, warmup_iter=100):
    """fit_dmtets.py:396-399: it / warmup below warmup_iter, then 10^(-0.0002 (it - warmup))."""
    if it < warmup_iter:
        return it / warmup_iter
    return max(0.0, 10 ** (-(it - warmup_iter) * 0.0002))


def _masked_sdf_reg(geometry, mesh, weight):
    """mean(sdf_reg_loss) * weight with the reference's detach mask (dmtet.py:441-446): the SDF of the vertices that own a
    crossing edge of `mesh` (`valid_vert_idx`) is held fixed."""
    sdf_mask = torch.zeros_like(geometry.sdf)
    sdf_mask[mesh.valid_vert_idx] = 1.0
    sdf_masked = geometry.sdf.detach() * sdf_mask + geometry.sdf * (1 - sdf_mask)
    return sdf_reg_loss(sdf_masked, geometry.all_edges).mean() * weight


def _chamfer_term(target_points, dev, num_samples, generator):
    """None without target points, else term(mesh, uniforms=None) = chamfer(sample_points(mesh, num_samples), target_points).mean()
    (dmtet.py:454-459)."""
    if target_points is None:
        return None
    pts = target_points.detach().to(device=dev, dtype=torch.float32).reshape(1, -1, 3).contiguous()

    def term(mesh, uniforms=None):
        pred = sample_points(mesh.v_pos[None], mesh.t_pos_idx, num_samples, uniforms=uniforms, generator=generator)[0]
        return chamfer_distance(pred, pts).mean()
    return term


# ---- the carves and the schedules of tick -------------------------------------------------------------------------------------------
def _vertex_pixels(geometry, target, rounded):
    """(px, py) int64 [B,N]: the deformed grid vertices projected with target['mvp'], their unit coordinates clipped to [0, 1],
    scaled (x with the width, y with the height) and rounded to the nearest pixel, or truncated (`.long()`)."""
    H, W = target["resolution"]
    clip = xfm_points(geometry.get_deformed().detach()[None], target["mvp"])
    ndc = clip[..., :2] / clip[..., 3:4]
    px, py = ((ndc[..., k] * 0.5 + 0.5).clip(0, 1) * (size - 1) for k, size in ((0, W), (1, H)))
    return (torch.round(px).long(), torch.round(py).long()) if rounded else (px.long(), py.long())


@torch.no_grad()
def carve_outside_silhouette(geometry, target, kernel_size=11):
    """The carve of tick (dmtet.py:366-378): project the deformed grid vertices, round to pixels, dilate `mask_cont` with a
    `kernel_size` box; where a vertex lands on a pixel whose dilated mask is 0 in ANY view, sdf = 1e-2 and deform = 0.
    x is scaled with the width and y with the height.  Returns the number of vertices carved."""
    px, py = _vertex_pixels(geometry, target, rounded=True)
    m = target["mask_cont"][..., 0].unsqueeze(1)
    box = torch.ones((1, 1, kernel_size, kernel_size), dtype=m.dtype, device=m.device) / (kernel_size * kernel_size)
    dilated = torch.nn.functional.conv2d(m, box, stride=1, padding=kernel_size // 2)[:, 0]
    outside = dilated == 0
    carved = torch.zeros(px.shape[1], dtype=torch.bool, device=px.device)
    for k in range(outside.shape[0]):
        carved |= outside[k, py[k], px[k]]
    geometry.sdf.data[carved] = 1e-2
    geometry.deform.data[carved] = 0.0
    return int(carved.sum())


@torch.no_grad()
def carve_single_view(geometry, target):
    """The carve of the single-view tick (dmtet_singleview.py:447-458): project the deformed grid vertices, clip the unit
    coordinates to [0, 1], scale and TRUNCATE them to pixels (`.long()`: no rounding, no dilation); where a vertex lands on a
    pixel whose `mask_cont` is 0 in a view, sdf = |sdf|.clamp(0, 1), view after view.  x is scaled with the width and y with
    the height (the reference asserts a square image).  Plain torch.  Returns the number of vertices carved."""
    px, py = _vertex_pixels(geometry, target, rounded=False)
    empty = target["mask_cont"][..., 0] == 0
    carved = torch.zeros(px.shape[1], dtype=torch.bool, device=px.device)
    for k in range(empty.shape[0]):
        m = empty[k, py[k], px[k]]
        geometry.sdf.data[m] = geometry.sdf.data[m].abs().clamp(0.0, 1.0)
        carved |= m
    return int(carved.sum())


def _pre_step(geometry, it, carve):
    """Before the step of iteration `it`, as both ticks have it: carve() for 200 < it < 2000 and it % 20 == 0 (carve None: never),
    then deform *= 0.4 for it % 300 == 0 and it < 1790."""
    if carve is not None and 200 < it < 2000 and it % 20 == 0:
        carve()
    if it % 300 == 0 and it < 1790:
        with torch.no_grad():
            geometry.deform.data[:] *= 0.4


# ---- what the loops share -----------------------------------------------------------------------------------------------------------
def _select_views(targets, n_views, views_per_iter, generator, dev):
    """The targets of one iteration: all of them, or `views_per_iter` views drawn without replacement (one torch.randperm)."""
    if views_per_iter is None or views_per_iter >= n_views:
        return targets
    sel = torch.randperm(n_views, generator=generator, device=generator.device if generator is not None else "cpu")
    sel = sel[:views_per_iter].to(dev)
    return {key: (val[sel] if torch.is_tensor(val) and val.shape[0] == n_views else val) for key, val in targets.items()}


def _need_targets(who, targets, keys, term, flag):
    for key in keys:
        if key not in targets:
            raise ValueError(f"{who}: the {term} term needs targets made with make_targets(..., {flag}=True): no {key!r}")


def _get_mesh(geometry, who, it, **kwargs):
    mesh = geometry.getMesh(**kwargs)
    if mesh.t_pos_idx.shape[0] == 0:
        raise _lib.MeshDiffusionHipError(f"{who}: the mesh of iteration {it} has no faces")
    return mesh


def _optimise(geometry, opt, iters, step, names, callback, dev, start_iteration=0, sched=None):
    """The loop of every fit.  For it = start_iteration .. start_iteration + iters - 1:
        opt.zero_grad -> step(it) = (total, {name: term}, mesh) -> total.backward -> opt.step [-> sched.step] -> clamp_deform
        -> the terms of `names` detached into the history -> callback(it, the term of names[0], mesh).
    Returns {name: float32 [iters] on `dev`} (length 0 for iters = 0)."""
    history = {name: [] for name in names}
    for it in range(start_iteration, start_iteration + iters):
        opt.zero_grad(set_to_none=True)
        total, terms, mesh = step(it)
        total.backward()
        opt.step()
        if sched is not None:
            sched.step()
        geometry.clamp_deform()
        for name in names:
            history[name].append(terms[name].detach())
        if callback is not None:
            callback(it, history[names[0]][-1], mesh)
    return {name: (torch.stack(xs) if xs else torch.empty(0, device=dev)) for name, xs in history.items()}


class _TextureParam:
    """What `_optimise` asks of a geometry, for a texture: nothing to clamp."""

    def clamp_deform(self):
        pass


def fit_texture(verts, faces, uvs, uv_idx, targets, resolution_tex, iters, lr=0.01, init=None, light=None, shade=True, callback=None):
    """Adam on a `kd` texture float32 [Ht,Wt,3] of a fixed mesh under the masked L1 between `render.render_textured` and posed images
    (the colour term of the reference's fit with the geometry frozen).  targets: dict of `images` [B,H,W,3], `viewmask` [B,H,W] or
    [B,H,W,1], `mvp` [B,4,4], `campos` [B,3].  loss = sum(|render.rgb - images| * viewmask) / (3 sum(viewmask)).  init: the starting
    texture (e.g. `texture.bake_from_views(...)["tex"]`), None: 0.5 everywhere.  Everything that does not depend on the texture (the
    layer, the texture coordinates, the irradiance, the antialiasing pairs' inputs, the `SamplePlan`) is computed once
    (`render.textured_fixed`).  Returns (texture, {"loss": float32 [iters]})."""
    from .render import _resolution, render_textured, textured_fixed
    _gpu_only(verts, "fit_texture")
    dev = verts.device
    Ht, Wt = _resolution(resolution_tex)
    images = targets["images"].detach().to(device=dev, dtype=torch.float32)
    vm = targets["viewmask"].detach().to(device=dev, dtype=torch.float32)
    vm = vm[..., None] if vm.dim() == 3 else vm
    if images.dim() != 4 or images.shape[-1] != 3 or tuple(vm.shape) != tuple(images.shape[:3]) + (1,):
        raise ValueError(f"fit_texture: expected images [B,H,W,3] and viewmask [B,H,W], got {tuple(images.shape)} and {tuple(targets['viewmask'].shape)}")
    H, W = images.shape[1], images.shape[2]
    if init is None:
        tex = torch.full((Ht, Wt, 3), 0.5, dtype=torch.float32, device=dev)
    else:
        if tuple(init.shape) != (Ht, Wt, 3):
            raise ValueError(f"fit_texture: expected init [{Ht},{Wt},3], got {tuple(init.shape)}")
        tex = init.detach().to(device=dev, dtype=torch.float32).clone()
    tex.requires_grad_(True)
    fixed = textured_fixed(verts, faces, uvs, uv_idx, (Ht, Wt, 3), targets["mvp"], targets["campos"], (H, W), light, shade)
    norm = 3.0 * vm.sum().clamp_min(1.0)
    opt = torch.optim.Adam([tex], lr=lr)

    def step(it):
        img = render_textured(verts, faces, uvs, uv_idx, tex, targets["mvp"], targets["campos"], (H, W), light, shade, _fixed=fixed)
        loss = ((img[..., :3] - images).abs() * vm).sum() / norm
        return loss, {"loss": loss}, None

    history = _optimise(_TextureParam(), opt, iters, step, ("loss",), callback, dev)
    return tex.detach(), history


# ---- the four fits ------------------------------------------------------------------------------------------------------------------
def fit_to_points(geometry, target_points, iters, *, num_samples=50000, lr=0.01, sdf_regularizer=0.2, generator=None,
                  callback=None, uniforms=None):
    """Fit a `DMTetGeometry` to target points [P,3] without a renderer: per iteration
        getMesh -> sample_points(num_samples) -> chamfer_distance(pred, target) + sdf_reg_loss(masked sdf) * weight * 0.1
        -> Adam step on (sdf, deform) -> clamp_deform,
    with the reference's regulariser schedule and `valid_vert_idx` detach mask (dmtet.py:441-446, 454-459).
    `uniforms(it)` may supply the iteration's (r_face, r_u, r_v), each [1,num_samples]; else torch.rand(generator=generator).
    `callback(it, chamfer, mesh)` is called after each step.  Returns the chamfer values, float32 [iters] on the device."""
    _gpu_only(target_points, "fit_to_points")
    dev = target_points.device
    chamfer_term = _chamfer_term(target_points, dev, num_samples, generator)

    def step(it):
        mesh = _get_mesh(geometry, "fit_to_points", it)
        chamfer = chamfer_term(mesh, uniforms(it) if uniforms is not None else None)
        reg = _masked_sdf_reg(geometry, mesh, sdf_regularizer_weight(it, iters, sdf_regularizer)) * 0.1
        return chamfer + reg, {"chamfer": chamfer}, mesh
    opt = torch.optim.Adam([geometry.sdf, geometry.deform], lr=lr)
    return _optimise(geometry, opt, iters, step, ("chamfer",), callback, dev)["chamfer"]


def fit_to_views(geometry, targets, iters, *, lr=0.01, sdf_regularizer=0.2, views_per_iter=None, generator=None,
                 target_points=None, num_samples=50000, carve=True, callback=None, start_iteration=0, alpha_weight=0.0,
                 return_terms=False, color_weight=0.0, color_loss_kind="logl1"):
    """Fit a `DMTetGeometry` to rendered targets (`make_targets`) the way the reference's tick supervises geometry: per
    iteration
        [carve, for 200 < it < 2000 and it % 20 == 0] -> [deform *= 0.4, for it % 300 == 0 and it < 1790]
        -> getMesh -> render_depth on `views_per_iter` views -> depth_loss + sdf_reg_loss(masked sdf) * weight * 0.1
        [+ alpha_weight * silhouette_loss, for alpha_weight > 0; the reference's weight is 1.0]
        [+ color_weight * color_loss(color_loss_kind), for color_weight > 0: the mesh then comes from getMesh(normals_grad=True)
           and is rendered with render_buffers; the reference's weight is 1.0 and its loss logl1]
        [+ chamfer(sample_points(num_samples), target_points)] -> Adam step on (sdf, deform) -> clamp_deform.
    views_per_iter: None = every view each iteration, else that many drawn without replacement (torch.randperm, `generator`).
    `callback(it, loss, mesh)` after each step.  Returns the depth-loss values, float32 [iters] on the device; with
    return_terms=True the dict {"depth": [iters], "alpha": [iters]} of both terms.  alpha_weight > 0 and return_terms need
    targets made with `make_targets(..., antialias=True)`; color_weight > 0 needs `make_targets(..., shaded=True)` and adds
    "color": [iters] to the dict of return_terms."""
    dev = geometry.sdf.device
    _gpu_only(geometry.sdf, "fit_to_views")
    n_views = targets["mvp"].shape[0]
    with_alpha, with_color = alpha_weight > 0 or return_terms, color_weight > 0
    if with_alpha:
        _need_targets("fit_to_views", targets, ("alpha", "alpha_second"), "alpha", "antialias")
    if with_color:
        _need_targets("fit_to_views", targets, ("img", "img_second"), "colour", "shaded")
    chamfer_term = _chamfer_term(target_points, dev, num_samples, generator)

    def step(it):
        tgt = _select_views(targets, n_views, views_per_iter, generator, dev)
        _pre_step(geometry, it, (lambda: carve_outside_silhouette(geometry, tgt)) if carve else None)
        mesh = _get_mesh(geometry, "fit_to_views", it, **({"normals_grad": True} if with_color else {}))
        if with_color:
            buffers = render_buffers(mesh.v_pos, mesh.t_pos_idx, tgt["mvp"], tgt["campos"], tgt["resolution"], v_nrm=mesh.v_nrm)
        else:
            buffers = render_depth(mesh.v_pos, mesh.t_pos_idx, tgt["mvp"], tgt["campos"], tgt["resolution"], antialias=with_alpha)
        terms = {"depth": depth_loss(buffers, tgt, it)}
        total = terms["depth"] + _masked_sdf_reg(geometry, mesh, sdf_regularizer_weight(it, start_iteration + iters, sdf_regularizer)) * 0.1
        if with_alpha:
            terms["alpha"] = silhouette_loss(buffers, tgt)
            if alpha_weight > 0:
                total = total + terms["alpha"] * alpha_weight
        if with_color:
            terms["color"] = color_loss(buffers, tgt, color_loss_kind)
            total = total + terms["color"] * color_weight
        if chamfer_term is not None:
            total = total + chamfer_term(mesh)
        return total, terms, mesh
    opt = torch.optim.Adam([geometry.sdf, geometry.deform], lr=lr)
    names = ("depth",) + ("alpha",) * with_alpha + ("color",) * with_color
    terms = _optimise(geometry, opt, iters, step, names, callback, dev, start_iteration)
    return terms if return_terms else terms["depth"]


def fit_fixed_topology(geometry, targets, iters, *, lr=0.01, laplace_scale=10000.0, warmup_iter=100, views_per_iter=None,
                       generator=None, target_points=None, num_samples=50000, callback=None, alpha_weight=0.0,
                       return_terms=False, color_weight=0.0, color_loss_kind="logl1"):
    """Pass 2 of the reference's fit (fit_dmtets.py:758-793, DMTetGeometryFixedTopo.tick): fine-tune the `deform` of a
    `dmtet.DMTetGeometryFixedTopo` on its frozen topology.  Per iteration
        getMesh (through the plan) -> render_depth, or render_buffers when color_weight > 0, on `views_per_iter` views, with the
        plan's neighbours and corner CSR -> depth_loss_fixedtopo
        [+ laplace_regularizer_const(v_pos, faces, base=initial_guess_v_pos) * laplace_scale * (1 - it / iters) * 1e-2, for laplace_scale > 0]
        [+ alpha_weight * mse(alpha), layer 1 only (:318)] [+ color_weight * image_loss(color_loss_kind), layer 1 only (:319-322)]
        [+ chamfer(sample_points(num_samples), target_points)]
        -> Adam step on deform, LambdaLR(lr_schedule_fixedtopo) step -> clamp_deform.
    `callback(it, loss, mesh)` after each step.  Returns the depth terms, float32 [iters] on the device; with return_terms=True
    the dict {"depth", "laplace", "alpha"[, "color"]} of the unweighted terms per iteration (device tensors; the Laplacian and
    alpha terms are then computed even at weight 0, and added to the loss only above it).  The alpha term needs targets made
    with `make_targets(..., antialias=True)`, the colour term `make_targets(..., shaded=True)`."""
    _gpu_only(geometry.deform, "fit_fixed_topology")
    dev = geometry.deform.device
    n_views = targets["mvp"].shape[0]
    with_alpha, with_color, with_laplace = alpha_weight > 0 or return_terms, color_weight > 0, laplace_scale > 0 or return_terms
    if with_alpha:
        _need_targets("fit_fixed_topology", targets, ("alpha",), "alpha", "antialias")
    if with_color:
        _need_targets("fit_fixed_topology", targets, ("img",), "colour", "shaded")
    chamfer_term = _chamfer_term(target_points, dev, num_samples, generator)

    def step(it):
        tgt = _select_views(targets, n_views, views_per_iter, generator, dev)
        plan = geometry.plan
        mesh = geometry.getMesh(normals_grad=True) if with_color else geometry.getMesh()
        if with_color:
            buffers = render_buffers(mesh.v_pos, mesh.t_pos_idx, tgt["mvp"], tgt["campos"], tgt["resolution"], v_nrm=mesh.v_nrm,
                                     neighbours=plan.neighbours, corner_csr=plan.corner_csr)
        else:
            buffers = render_depth(mesh.v_pos, mesh.t_pos_idx, tgt["mvp"], tgt["campos"], tgt["resolution"], antialias=with_alpha,
                                   neighbours=plan.neighbours)
        terms = {"depth": depth_loss_fixedtopo(buffers, tgt)}
        total = terms["depth"]
        if with_laplace:
            terms["laplace"] = laplace_regularizer_const(mesh.v_pos, mesh.t_pos_idx, base=geometry.initial_guess_v_pos, corner_csr=plan.corner_csr)
            if laplace_scale > 0:
                total = total + terms["laplace"] * (laplace_scale * (1 - it / iters) * 1e-2)
        terms["alpha"], terms["color"] = _layer1_image_terms(buffers.get("alpha"), tgt["alpha"] if with_alpha else None,
                                                             buffers.get("shaded"), tgt["img"] if with_color else None, color_loss_kind)
        if alpha_weight > 0:
            total = total + terms["alpha"] * alpha_weight
        if with_color:
            total = total + terms["color"] * color_weight
        if chamfer_term is not None:
            total = total + chamfer_term(mesh)
        return total, terms, mesh
    opt = torch.optim.Adam([geometry.deform], lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda it: lr_schedule_fixedtopo(it, warmup_iter))
    names = ("depth",) + ("laplace",) * with_laplace + ("alpha",) * with_alpha + ("color",) * with_color
    terms = _optimise(geometry, opt, iters, step, names, callback, dev, sched=sched)
    return terms if return_terms else terms["depth"]


def fit_single_view(geometry, target, iters, *, lr=0.01, sdf_regularizer=0.2, target_points=None, gt_mesh=None, num_samples=50000,
                    generator=None, color_loss_kind="logl1", callback=None, start_iteration=0, total_iters=None):
    """Fit a `DMTetGeometry` to ONE view the way the reference's single-view loop does (fit_singleview.py:489-502 around
    dmtet_singleview.DMTetGeometry.tick, :438-516).  target: `make_targets(..., shaded=True)` of the view.  Per iteration `it`
        [init_with_gt_surface, for it < 300 and it % 10 == 0, with the faces of gt_mesh = (verts, faces) that the view sees: the
         `rast_triangle_id` of `render_depth` on it, found once]
        -> deform.requires_grad = (it >= 100) -> [carve_single_view, for 200 < it < 2000 and it % 20 == 0]
        -> [deform *= 0.4, for it % 300 == 0 and it < 1790] -> getMesh(normals_grad=True) -> render_buffers
        -> mse(alpha) + image_loss(shaded rgb x ref alpha, ref rgb x ref alpha) of layer 1 + depth_loss_single_view
           + sdf_reg_loss(masked sdf) * weight * 2.5 [+ chamfer(sample_points(num_samples), target_points)]
        -> Adam step on (sdf, deform) -> clamp_deform.
    The regulariser's weight falls from `sdf_regularizer` to 0.01 over the first quarter of `total_iters` (default:
    start_iteration + iters).  `callback(it, depth term, mesh)` after each step.  Returns the per-iteration terms as
    `fit_to_views(return_terms=True)` does: {"depth", "alpha", "color"}, float32 [iters] each on the device.
    Not built: the reference's `kd_grad` and `occlusion` regularisers (they need materials), `msaa`, and its random background
    (the targets and the prediction are rendered on a zero background)."""
    _gpu_only(geometry.sdf, "fit_single_view")
    dev = geometry.sdf.device
    _need_targets("fit_single_view", target, ("img", "alpha", "depth", "depth_second", "mask_cont", "mvp", "campos", "resolution"),
                  "single-view", "shaded")
    total_iters = start_iteration + iters if total_iters is None else total_iters
    chamfer_term = _chamfer_term(target_points, dev, num_samples, generator)
    surface_faces = gt_verts = None
    if gt_mesh is not None:
        gt_verts = gt_mesh[0].detach().to(device=dev, dtype=torch.float32)
        gt_faces = gt_mesh[1].to(dev).long()
        with torch.no_grad():
            seen = render_depth(gt_verts, gt_faces, target["mvp"], target["campos"], target["resolution"])["rast_triangle_id"]
        surface_faces = None if seen is None else gt_faces[seen]
    ref = target["img"]

    def step(it):
        if surface_faces is not None and it < 300 and it % 10 == 0:
            init_with_gt_surface(geometry, gt_verts, surface_faces, target["campos"][0])
        geometry.deform.requires_grad_(it >= 100)
        _pre_step(geometry, it, lambda: carve_single_view(geometry, target))
        mesh = _get_mesh(geometry, "fit_single_view", it, normals_grad=True)
        buffers = render_buffers(mesh.v_pos, mesh.t_pos_idx, target["mvp"], target["campos"], target["resolution"], v_nrm=mesh.v_nrm)
        alpha, color = _layer1_image_terms(buffers["shaded"][..., 3:], ref[..., 3:], buffers["shaded"], ref, color_loss_kind)
        depth = depth_loss_single_view(buffers, target)
        reg = _masked_sdf_reg(geometry, mesh, sdf_regularizer_weight(it, total_iters, sdf_regularizer)) * 2.5
        total = alpha + color + depth + reg
        if chamfer_term is not None:
            total = total + chamfer_term(mesh)
        return total, {"depth": depth, "alpha": alpha, "color": color}, mesh
    opt = torch.optim.Adam([geometry.sdf, geometry.deform], lr=lr)
    try:
        return _optimise(geometry, opt, iters, step, ("depth", "alpha", "color"), callback, dev, start_iteration)
    finally:
        geometry.deform.requires_grad_(True)


# ---- what the command lines tools/fit_*.py share ------------------------------------------------------------------------------------
def add_fit_arguments(ap, *, iters, out_example, points=0, points_help="> 0: add the chamfer term with this many target points and samples",
                      pass2_help=None):
    """The arguments every fitting tool takes (the defaults of --iters and --points are the tool's) and, with pass2_help, those
    of the tools that render: the image size, the camera and the second pass."""
    ap.add_argument("--obj", required=True, help="triangle mesh to fit")
    ap.add_argument("--tet_path", required=True, help="<R>_tets_cropped.npz (vertices, indices)")
    ap.add_argument("--out", required=True, help=f"path of the dict to write, e.g. {out_example}")
    ap.add_argument("--resolution", type=int, default=64, help="resolution of the tet grid")
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--sdf_regularizer", type=float, default=0.2)
    ap.add_argument("--points", type=int, default=points, help=points_help)
    ap.add_argument("--mesh_scale", type=float, default=2.1)
    ap.add_argument("--deform_scale", type=float, default=2.0)
    ap.add_argument("--fit_scale", type=float, default=0.8, help="largest half-extent of the normalised target")
    ap.add_argument("--seed", type=int, default=0)
    if pass2_help is not None:
        ap.add_argument("--res", type=int, default=256)
        ap.add_argument("--cam_radius", type=float, default=3.0)
        ap.add_argument("--fovy", type=float, default=math.radians(45.0))
        ap.add_argument("--pass2_iters", type=int, default=0, help=pass2_help)
        ap.add_argument("--pass2_lr", type=float, default=0.01)
        ap.add_argument("--laplace_scale", type=float, default=10000.0)


def load_normalised_obj(path, fit_scale):
    """(verts float32 [V,3], faces int64 [F,3]) of an `.obj` on the GPU, centred on its bounding box and scaled so that its
    largest half-extent is `fit_scale`."""
    from .mesh_export import load_obj
    verts, faces = load_obj(path)
    v = torch.as_tensor(verts, dtype=torch.float32).cuda()
    lo, hi = v.min(0).values, v.max(0).values
    return (v - (lo + hi) / 2) * (fit_scale / float((hi - lo).max() / 2)), torch.as_tensor(faces).cuda()


def look_at_cameras(n, radius, fovy, device, angle=None, elevation=None):
    """(mvp [n,4,4], campos [n,3]) of n cameras that look at the origin from distance `radius`: perspective(fovy, 1, 0.1, 1000) @
    translate(0, 0, -radius) @ rotate_x(elevation) @ rotate_y(angle).  By default camera k of n stands at angle 2 pi k / n around
    the y axis, the elevations alternating between -0.4 and +0.4; `angle` / `elevation` fix them (the one camera of n = 1)."""
    proj = perspective(fovy, 1.0, 0.1, 1000.0)
    mvps, cams = [], []
    for k in range(n):
        el = (-0.4 if k % 2 == 0 else 0.4) if elevation is None else elevation
        mv = translate(0, 0, -radius) @ rotate_x(el) @ rotate_y(2 * math.pi * k / n if angle is None else angle)
        mvps.append(proj @ mv)
        cams.append(torch.linalg.inv(mv)[:3, 3])
    return torch.stack(mvps).to(device), torch.stack(cams).to(device)


def make_geometry(args):
    """The `DMTetGeometry` of --tet_path, --resolution, --mesh_scale and --deform_scale; with --sphere_init r > 0 its SDF starts
    as the sphere of radius r."""
    tet = np.load(args.tet_path)
    geo = DMTetGeometry(args.resolution, args.mesh_scale, None, tets=(tet["vertices"], tet["indices"]), deform_scale=args.deform_scale)
    if getattr(args, "sphere_init", 0.0) > 0:
        with torch.no_grad():
            geo.sdf.copy_((args.sphere_init - geo.verts.norm(dim=1)).clamp(-1.0, 1.0))
    return geo


def progress(label, iters, prefix=""):
    """A fit's callback: prints every 100th and the last iteration's term, as `<prefix>iter <it>: <label> <term>  V <n> F <n>`."""
    def report(it, term, mesh):
        if it % 100 == 0 or it == iters - 1:
            print(f"{prefix}iter {it}: {label} {float(term):.6f}  V {mesh.v_pos.shape[0]} F {mesh.t_pos_idx.shape[0]}", flush=True)
    return report


def second_pass(geo, args, targets, label, *, pre_dict=None, second_deform_scale=None, **fit_kwargs):
    """The fixed-topology pass of a tool (fit_dmtets.py:758-793): `fit_fixed_topology` for --pass2_iters iterations at --pass2_lr
    and --laplace_scale on the frozen topology of `geo`; returns the `DMTetGeometryFixedTopo`.  pre_dict: where the pass-1 dict
    goes first.  second_deform_scale: the deform_scale of this pass, deform being rescaled by deform_scale / it (:770); None
    keeps --deform_scale and deform as they are."""
    if pre_dict is not None:
        os.makedirs(os.path.dirname(pre_dict), exist_ok=True)
        torch.save(geo.state_to_dict(), pre_dict)
        print(f"wrote {pre_dict}")
    rescale = second_deform_scale is not None
    fixed = DMTetGeometryFixedTopo(geo, args.resolution, args.mesh_scale, deform_scale=second_deform_scale if rescale else args.deform_scale)
    if rescale:
        with torch.no_grad():
            fixed.deform.data[:] = fixed.deform * args.deform_scale / second_deform_scale
    fixed.set_init_v_pos()
    fit_fixed_topology(fixed, targets, args.pass2_iters, lr=args.pass2_lr, laplace_scale=args.laplace_scale,
                       callback=progress(label, args.pass2_iters, "pass 2 "), **fit_kwargs)
    return fixed
