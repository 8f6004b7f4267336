"""Cases and torch restatements of the interpolation contract (the header comment of csrc/interp.hip): attribute interpolation,
the gradient of the barycentrics, deterministic vertex normals, the `bsdf == 'normal'` buffers and the colour term of the fit.
Shared by tools/gen_golden_interp.py, the CPU tests, the GPU tests and tools/bench_raster.py.  Everything runs in fp32 or float64
under torch autograd on the device of its inputs; discrete decisions (ids, the pairs of the antialiasing, the flip) can be passed
in, so that one set of decisions serves both precisions.
"""
import functools

import torch

import antialias_cases as ac
import raster_cases as rc

# (mesh, H, W), each seen from rc.ANGLES (B = 2)
CASES = (("ptorus", 40, 72), ("ptorus", 64, 64), ("sphere", 64, 64), ("quad", 16, 16), ("fan40", 16, 16), ("degen", 16, 16))
BUFFER_CASES = CASES[:3]
CHANNELS = (1, 3, 8)
TRI_KINDS = ("faces", "fff")
FAN = 40
KINK = 1e-4                            # |view . smooth / 0.1 - {0, 1}| under which a pixel sits on the kink of the bend
FLIP_MARGIN = 1e-3                     # no covered pixel of a fixture case may have |geo . view| under this
FIT_RES, FIT_ITERS, FIT_STEPS = 64, 21, (0, 10, 20)
FIT_COLOR_WEIGHT = FIT_ALPHA_WEIGHT = 1.0
FIT_KIND = "logl1"
LOSS_KINDS = ("smape", "mse", "logl1", "logl2", "relmse")


def case_id(case):
    return f"{case[0]}-{case[1]}x{case[2]}"


# ---- meshes (world space) -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts float32 [V,3], faces int64 [F,3]) on the CPU."""
    if name == "ptorus":
        return ac.param_torus()
    if name == "sphere":
        return rc.mesh("sphere")
    quad = [(-0.7, -0.5, 0.1), (0.6, -0.55, 0.0), (0.65, 0.5, -0.1), (-0.6, 0.45, 0.05)]
    if name == "quad":
        return torch.tensor(quad, dtype=torch.float32), torch.tensor([[0, 1, 2], [0, 2, 3]])
    if name == "fan40":             # 40 triangles around vertex 0: its CSR row has 40 entries
        k = torch.arange(FAN, dtype=torch.float64) * (2 * torch.pi / FAN)
        ring = torch.stack([0.8 * torch.cos(k), 0.8 * torch.sin(k), torch.zeros_like(k)], 1)
        v = torch.cat([torch.tensor([[0.0, 0.0, 0.3]], dtype=torch.float64), ring]).to(torch.float32)
        i = torch.arange(FAN)
        return v, torch.stack([torch.zeros_like(i), 1 + i, 1 + (i + 1) % FAN], 1)
    if name == "degen":             # vertex 4 is named by no face; 5, 6, 7 (one point) only by a face of zero area; face 3 names 1 twice
        v = quad + [(0.3, 0.2, 0.4), (0.3, 0.7, 0.0), (0.3, 0.7, 0.0), (0.3, 0.7, 0.0)]
        return torch.tensor(v, dtype=torch.float32), torch.tensor([[0, 1, 2], [0, 2, 3], [5, 6, 7], [1, 1, 2]])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(verts [V,3], faces [F,3], mvp [B,4,4], campos [B,3], pos_clip float32 [B,V,4], H, W) on the CPU."""
    name, H, W = case
    verts, faces = mesh(name)
    mvp, campos = rc.cameras(rc.ANGLES, H, W)
    return verts, faces, mvp, campos, rc.xfm_points_restated(verts, mvp).contiguous(), H, W


def fff(n_faces):
    return torch.arange(n_faces, dtype=torch.int64)[:, None].expand(n_faces, 3).contiguous()


def case_attr(n_rows, C, Ba, seed):
    return torch.randn(Ba, n_rows, C, generator=torch.Generator().manual_seed(int(seed) + 17 * C + Ba))


def case_G(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def attr_cases(n_verts, n_faces, faces, B):
    """(name, tri, N, C, Ba) of every attribute case of a mesh."""
    out = []
    for kind in TRI_KINDS:
        tri, N = (faces, n_verts) if kind == "faces" else (fff(n_faces), n_faces)
        for C in CHANNELS:
            for Ba in (1, B):
                out.append((f"{kind}/C{C}/Ba{1 if Ba == 1 else 'B'}", tri, N, C, Ba))
    return out


# ---- interpolation -------------------------------------------------------------------------------------------------------------------
def covered(rast, n_faces):
    return (rast[..., 3] >= 1) & (rast[..., 3] <= n_faces)


def interpolate_restated(attr, rast, tri, dtype=torch.float64, uv=None):
    """The contract's value [B,H,W,C] in `dtype`: attr [N,C] or [Ba,N,C], rast float32 [B,H,W,4], tri int64 [F,3]; `uv` = (u, v)
    [B,H,W] in `dtype` replaces rast's own (the barycentric path under autograd).  Differentiable w.r.t. attr and uv."""
    a = attr.to(dtype)
    a = a[None] if a.dim() == 2 else a
    B, H, W, _ = rast.shape
    F = tri.shape[0]
    if F == 0:
        return torch.zeros(B, H, W, a.shape[-1], dtype=dtype, device=rast.device)
    cov = covered(rast, F)
    t3 = tri[(rast[..., 3].to(torch.int64) - 1).clamp(0, F - 1)]                # [B,H,W,3]; an id above F is masked below
    bi = torch.arange(B, device=rast.device)[:, None, None] if a.shape[0] > 1 else torch.zeros(1, 1, 1, dtype=torch.int64, device=rast.device)
    A0, A1, A2 = a[bi, t3[..., 0]], a[bi, t3[..., 1]], a[bi, t3[..., 2]]
    u, v = (rast[..., 0].to(dtype), rast[..., 1].to(dtype)) if uv is None else uv
    out = (u[..., None] * A0 + v[..., None] * A1) + ((1 - u) - v)[..., None] * A2
    return torch.where(cov[..., None], out, torch.zeros_like(out))


def interpolate_grads_restated(attr, rast, tri, G, dtype=torch.float64):
    """(value, d attr, d rast [B,H,W,4]) of sum(G * interpolate) in `dtype`."""
    a = attr.detach().to(dtype).requires_grad_(True)
    u = rast[..., 0].detach().to(dtype).requires_grad_(True)
    v = rast[..., 1].detach().to(dtype).requires_grad_(True)
    out = interpolate_restated(a, rast, tri, dtype, (u, v))
    (out * G.to(dtype)).sum().backward()
    zero = torch.zeros_like(u)
    du, dv = (zero if u.grad is None else u.grad), (zero if v.grad is None else v.grad)
    return out.detach(), (torch.zeros_like(a) if a.grad is None else a.grad), torch.stack([du, dv, zero, zero], -1)


def layer_uv(pos_clip, faces, rast, dtype=torch.float64):
    """(u, v) [B,H,W] of one rast layer recomputed from pos_clip in `dtype`, as rc.bary_restated does: differentiable w.r.t.
    pos_clip, which is the barycentric path."""
    ids = rast[..., 3].to(torch.int64)[:, None]
    ids = torch.where((ids >= 1) & (ids <= faces.shape[0]), ids, torch.zeros_like(ids))
    u, v = rc.bary_restated(pos_clip, faces, ids, dtype)
    return u[:, 0], v[:, 0]


def bary_grad_restated(pos_clip, faces, rast, G, dtype=torch.float64):
    """d sum(G[..., 0] u + G[..., 1] v) / d pos_clip [B,V,4] in `dtype`, G [B,H,W,4] (channels 2, 3 unused)."""
    p = pos_clip.detach().to(dtype).requires_grad_(True)
    if faces.shape[0] == 0:
        return torch.zeros_like(p)
    u, v = layer_uv(p, faces, rast, dtype)
    (u * G[..., 0].to(dtype) + v * G[..., 1].to(dtype)).sum().backward()
    return p.grad


def chain_depth_restated(verts, faces, mvp, campos, rast, dtype=torch.float64):
    """|interpolate(verts) - campos| [B,H,W] of one layer with u, v recomputed from xfm_points(verts): the chain
    rasterize(grad=True) -> interpolate(rast_grad=True) -> distance.  Zero where uncovered."""
    v = verts.to(dtype)
    pc = rc.xfm_points_restated(v, mvp, dtype)
    pos = interpolate_restated(v, rast, faces, dtype, layer_uv(pc, faces, rast, dtype))
    cov = covered(rast, faces.shape[0])
    d = torch.where(cov[..., None], pos - campos.to(dtype)[:, None, None, :], torch.ones_like(pos))
    return torch.where(cov, torch.sqrt((d * d).sum(-1)), torch.zeros_like(d[..., 0]))


# ---- vertex normals -------------------------------------------------------------------------------------------------------------------
def vertex_normals_restated(verts, faces, dtype=torch.float64):
    """(v_nrm [V,3], f_nrm [F,3] unnormalised, replaced bool [V]) in `dtype`, differentiable w.r.t. verts."""
    v = verts.to(dtype)
    V = v.shape[0]
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    fn = torch.linalg.cross(v1 - v0, v2 - v0)
    s = torch.zeros(V, 3, dtype=dtype, device=v.device).index_add(0, faces.reshape(-1), fn.repeat_interleave(3, 0))
    replaced = (s * s).sum(-1) <= 1e-20
    up = torch.tensor([0.0, 0.0, 1.0], dtype=dtype, device=v.device).expand(V, 3)
    s = torch.where(replaced[:, None], up, s)
    return s / torch.sqrt(torch.clamp((s * s).sum(-1, keepdim=True), min=1e-20)), fn, replaced


def vertex_normals_grads_restated(verts, faces, G, dtype=torch.float64):
    v = verts.detach().to(dtype).requires_grad_(True)
    n, _, _ = vertex_normals_restated(v, faces, dtype)
    (n * G.to(dtype)).sum().backward()
    return n.detach(), v.grad


# ---- shading normal, buffers, losses ---------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _normalize(x):
    return x / torch.clamp(torch.sqrt(_dot(x, x)), min=1e-12)


def shading_normal_restated(pos, campos, nrm, geo, dtype=torch.float64, front=None):
    """(shading normal, flipped geo, geo . view, view . smooth / 0.1) in `dtype`; `front` bool [...,1] fixes the flip decision."""
    pos, nrm, geo = pos.to(dtype), nrm.to(dtype), geo.to(dtype)
    cam = campos.to(dtype)
    cam = cam[:, None, None, :] if cam.dim() == 2 else cam
    smooth, view = _normalize(nrm), _normalize(cam - pos)
    gv = _dot(geo, view)
    front = gv > 0 if front is None else front
    smooth = torch.where(front, smooth, -smooth)
    geo = torch.where(front, geo, -geo)
    t_raw = _dot(view, smooth) / 0.1
    t = t_raw.clamp(0, 1)
    return geo + t * (smooth - geo), geo, gv, t_raw


def buffers_restated(verts, faces, mvp, campos, rast, dtype=torch.float64, v_nrm=None, dec=None):
    """The buffers of render.render_buffers for the two given `rast` layers (float32 [B,H,W,4] each) in `dtype`, differentiable
    w.r.t. verts (and v_nrm when given) through the attribute path, the barycentric path, the vertex normals and the
    antialiasing: dict of pos, geo_normal, normal, shaded, alpha, mask (+ `_second`), and per layer the diagnostics
    `geo_view` (geo . view before the flip) and `kink` (bool [B,H,W], the pixels on the kink of the bend).  dec: the pair
    decisions of both layers (built when None)."""
    v = verts.to(dtype)
    V, F = v.shape[0], faces.shape[0]
    pc = rc.xfm_points_restated(v, mvp, dtype)
    pc32 = pc.detach().to(torch.float32)
    if v_nrm is None:
        n, fn, _ = vertex_normals_restated(v, faces, dtype)
    else:
        n = v_nrm.to(dtype)
        fn = torch.linalg.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    geo_attr = fn / torch.sqrt(torch.clamp(_dot(fn, fn), min=1e-20))
    nbr = torch.as_tensor(ac.edge_neighbours_restated(faces.cpu().numpy(), V), device=faces.device)
    out = {}
    for k, (r, bg, tail) in enumerate(((rast[0], 20.0, ""), (rast[1], -1.0, "_second"))):
        cov = covered(r, F)[..., None]
        mask = cov.to(dtype)
        uv = layer_uv(pc, faces, r, dtype)
        pos = interpolate_restated(v, r, faces, dtype, uv)
        gb_n = interpolate_restated(n, r, faces, dtype, uv)
        gb_geo = interpolate_restated(geo_attr, r, fff(F).to(faces.device), dtype)
        normal, geo, gv, t_raw = shading_normal_restated(pos, campos, gb_n, gb_geo, dtype)
        zero = torch.zeros_like(normal)
        normal, geo = torch.where(cov, normal, zero), torch.where(cov, geo, zero)
        d = ac.pair_decisions(r, pc32, faces, nbr) if dec is None else dec[k]
        col = torch.cat([((normal + 1) / 2) * mask, mask], -1)
        shaded = ac.antialias_restated(col, r, pc, faces, nbr, dtype, d)
        out["pos" + tail] = torch.where(cov, pos, torch.full_like(pos, bg))
        out["geo_normal" + tail], out["normal" + tail], out["shaded" + tail] = geo, normal, shaded
        out["alpha" + tail], out["mask" + tail] = shaded[..., 3:], mask
        out["geo_view" + tail] = torch.where(cov, gv, torch.ones_like(gv))[..., 0].detach()
        tr = t_raw[..., 0].detach()
        out["kink" + tail] = cov[..., 0] & ((tr.abs() < KINK) | ((tr - 1).abs() < KINK))
    return out


GRAD_KEYS = ("normal", "pos", "shaded", "normal_second", "pos_second", "shaded_second")


def dilate(m):
    """bool [B,H,W] -> the pixels and their four neighbours."""
    out = m.clone()
    out[:, 1:] |= m[:, :-1]
    out[:, :-1] |= m[:, 1:]
    out[:, :, 1:] |= m[:, :, :-1]
    out[:, :, :-1] |= m[:, :, 1:]
    return out


def buffer_G(buf, seed):
    """The seeded G of every key of GRAD_KEYS, zero on the kink pixels of its layer (for `shaded`, which blends neighbours, on
    their four neighbours as well) and on the uncovered pixels of `pos` (a constant)."""
    G = {}
    for i, key in enumerate(GRAD_KEYS):
        tail = "_second" if key.endswith("_second") else ""
        g = case_G(buf[key].shape, int(seed) + i)
        kink = buf["kink" + tail]
        kink = dilate(kink) if key.startswith("shaded") else kink
        g = torch.where(kink[..., None], torch.zeros_like(g), g)
        if key.startswith("pos"):
            g = g * buf["mask" + tail].to(g.dtype)
        G[key] = g
    return G


def buffers_dverts_restated(verts, faces, mvp, campos, rast, G, dtype=torch.float64, dec=None):
    v = verts.detach().to(dtype).requires_grad_(True)
    buf = buffers_restated(v, faces, mvp, campos, rast, dtype, dec=dec)
    sum((buf[k] * G[k].to(dtype)).sum() for k in GRAD_KEYS).backward()
    return v.grad


def _tonemap_srgb(f):
    return torch.where(f > 0.0031308, torch.clamp(f, min=0.0031308) ** (1.0 / 2.4) * 1.055 - 0.055, 12.92 * f)


def image_loss_restated(img, ref, kind):
    """createLoss(kind) of the reference, literally (fit_dmtets.py:65-77, renderutils/loss.py)."""
    if kind in ("logl1", "logl2"):
        img, ref = (_tonemap_srgb(torch.log(x.clamp(0, 65535) + 1)) for x in (img, ref))
    if kind in ("mse", "logl2"):
        return ((img - ref) ** 2).mean()
    if kind == "smape":
        return ((img - ref).abs() / (img.abs() + ref.abs() + 0.01)).mean()
    if kind == "relmse":
        return ((img - ref) * (img - ref) / (img * img + ref * ref + 0.1)).mean()
    if kind == "logl1":
        return (img - ref).abs().mean()
    raise KeyError(kind)


def color_loss_restated(shaded, shaded_second, img, img_second, kind="logl1"):
    return (image_loss_restated(shaded[..., 0:3] * img[..., 3:], img[..., 0:3] * img[..., 3:], kind)
            + 0.1 * image_loss_restated(shaded_second[..., 0:3] * img_second[..., 3:], img_second[..., 0:3] * img_second[..., 3:], kind))


# ---- the fitting run with the colour term ----------------------------------------------------------------------------------------------
def fit_restated(geo, sdf_reg_loss, dtype, iters=FIT_ITERS):
    """The loop of render.fit_to_views(color_weight=1, alpha_weight=1, every view each iteration, no chamfer, no carve) on the
    CPU in `dtype` with the restated rasteriser, buffers and losses: `geo` is a DMTetGeometry-like object (verts, sdf, deform,
    indices, all_edges, marching_tets, get_deformed, clamp_deform) already on the sphere start, `sdf_reg_loss` its regulariser.
    Returns {"depth", "alpha", "color"}: float lists per iteration."""
    H = W = FIT_RES
    mvp, campos = rc.cameras(rc.FIT_ANGLES, H, W)
    tv, tf = rc.mesh("torus")
    tgt = rc.targets_restated(tv, tf, mvp, campos, H, W, dtype)
    with torch.no_grad():
        tb = buffers_restated(tv, tf, mvp, campos, ac.rast_restated(rc.xfm_points_restated(tv, mvp), tf, H, W), dtype)
    opt = torch.optim.Adam([geo.sdf, geo.deform], lr=rc.FIT_LR)
    terms = {"depth": [], "alpha": [], "color": []}
    for it in range(iters):
        if it % 300 == 0 and it < 1790:
            geo.deform.data[:] *= 0.4
        opt.zero_grad()
        verts, faces, _, _, _, valid_vert_idx = geo.marching_tets(geo.get_deformed(), geo.sdf, geo.indices)
        pc = rc.xfm_points_restated(verts.detach(), mvp, dtype).to(torch.float32)
        ids = rc.rasterize_restated(pc, faces, H, W)["ids"]
        d = rc.depth_restated(verts, faces, mvp, campos, ids, dtype)
        depth = rc.depth_loss_restated(d[:, 0, :, :, None], d[:, 1, :, :, None], tgt["depth"], tgt["depth_second"], tgt["mask_cont"], it)
        buf = buffers_restated(verts, faces, mvp, campos, ac.rast_restated(pc, faces, H, W, ids), dtype)
        alpha = ac.silhouette_loss_restated(buf["alpha"], buf["alpha_second"], tb["alpha"], tb["alpha_second"])
        color = color_loss_restated(buf["shaded"], buf["shaded_second"], tb["shaded"], tb["shaded_second"], FIT_KIND)
        sdf_weight = rc.FIT_SDF_REGULARIZER - (rc.FIT_SDF_REGULARIZER - 0.01) * min(1.0, 4.0 * (it / iters))
        sdf_mask = torch.zeros_like(geo.sdf)
        sdf_mask[valid_vert_idx] = 1.0
        sdf_masked = geo.sdf.detach() * sdf_mask + geo.sdf * (1 - sdf_mask)
        reg = sdf_reg_loss(sdf_masked, geo.all_edges).mean() * sdf_weight * 0.1
        (depth + reg + alpha * FIT_ALPHA_WEIGHT + color * FIT_COLOR_WEIGHT).backward()
        opt.step()
        geo.clamp_deform()
        for k, x in (("depth", depth), ("alpha", alpha), ("color", color)):
            terms[k].append(float(x))
    return terms
