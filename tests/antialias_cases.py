"""Cases and torch / numpy restatements of the antialiasing contract (the header comment of csrc/antialias.hip), in the manner
of nvdiffrast's dr.antialias, not equal to it.  Shared by tools/gen_golden_antialias.py, the CPU tests, the GPU tests and
tools/bench_raster.py.

  edge_neighbours_restated   nbr of the contract, by a dictionary over the unordered vertex pairs (numpy).
  pair_decisions             every discrete decision of the contract for the pairs of a `rast` layer: int64 arithmetic on the
                             fp32 snap of raster_cases.snap, fp32 compares of the depths stored in rast, and the fp32 test of the
                             value's denominator.  Independent of the dtype the values are then computed in.
  antialias_restated         the value in fp32 or float64 under torch autograd (color and pos_clip), decisions given.
Every restatement runs on the device of its inputs.
"""
import functools

import numpy as np
import torch

import raster_cases as rc

TORUS_NU, TORUS_NV = 16, 8
COLOURS = ("mask", "c3", "c8")
# (mesh, H, W): the cases of the GPU tests and of the fixture's units
CASES = (("ptorus", 40, 72), ("ptorus", 64, 64), ("quad", 16, 16), ("fan3", 16, 16), ("wneg", 16, 16), ("sphere", 128, 128))
RECT = (2.3, 11.7, 3.6, 12.2)          # x0, x1, y0, y1 of the rectangle case in pixels, at 16 x 16
FIT_RES = 256
FIT_ITERS = 21
FIT_STEPS = (0, 10, 20)
FIT_ALPHA_WEIGHT = 1.0
FIT_SMALL_RADIUS = 0.5                 # a start that does not cover the torus's silhouette


def case_id(case):
    return f"{case[0]}-{case[1]}x{case[2]}"


# ---- meshes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def param_torus(nu=TORUS_NU, nv=TORUS_NV, R=0.6, r=0.25):
    """A closed nu x nv parametric torus around y: (verts float32 [nu nv,3], faces int64 [2 nu nv,3])."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    u, v = 2 * np.pi * i / nu, 2 * np.pi * j / nv
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), r * np.sin(v), (R + r * np.cos(v)) * np.sin(u)], -1).reshape(-1, 3)
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    f = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3)
    return torch.tensor(p, dtype=torch.float32), torch.tensor(f, dtype=torch.int64)


def _pix(x, y, z, H, W, w=1.0):
    """A clip-space vertex at the pixel position (x, y) (pixel (i, j) has its centre at (j + 0.5, i + 0.5))."""
    return ((2.0 * x / W - 1.0) * w, (2.0 * y / H - 1.0) * w, z * w, w)


def small_mesh(name):
    """(pos_clip float32 [1,V,4], faces int64 [F,3]) of the hand-made cases at 16 x 16."""
    H = W = 16
    if name == "quad":              # an open rectangle with edges at fractional pixel positions: 4 boundary edges, one diagonal
        x0, x1, y0, y1 = RECT
        v = [_pix(x0, y0, 0.3, H, W), _pix(x1, y0, 0.3, H, W), _pix(x1, y1, 0.3, H, W), _pix(x0, y1, 0.3, H, W)]
        f = [[0, 1, 2], [0, 2, 3]]
    elif name == "fan3":            # three triangles sharing the edge 0-1: that edge has no neighbour in any of them
        v = [_pix(7.7, 1.4, 0.2, H, W), _pix(8.4, 14.3, 0.2, H, W), _pix(1.6, 6.2, 0.25, H, W, 1.5), _pix(14.1, 9.3, 0.3, H, W),
             _pix(12.2, 2.7, 0.5, H, W, 0.8)]
        f = [[0, 1, 2], [1, 0, 3], [0, 1, 4]]
    elif name == "wneg":            # the neighbour across the edge 1-2 has its opposite vertex behind the camera
        v = [_pix(2.2, 2.6, 0.3, H, W), _pix(12.7, 3.4, 0.3, H, W), _pix(4.3, 13.1, 0.3, H, W), (0.4, 0.5, 0.1, -1.0)]
        f = [[0, 1, 2], [2, 1, 3]]                # face 1 is skipped by the rasteriser; nbr of the edge 1-2 in face 0 is vertex 3
    else:
        raise KeyError(name)
    return torch.tensor(v, dtype=torch.float32)[None], torch.tensor(f, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(pos_clip float32 [B,V,4], faces int64 [F,3], H, W) on the CPU; the meshes are seen from rc.ANGLES (B = 2)."""
    name, H, W = case
    if name in ("quad", "fan3", "wneg"):
        pc, f = small_mesh(name)
        return pc, f, H, W
    verts, f = param_torus() if name == "ptorus" else rc.mesh(name)
    mvp, _ = rc.cameras(rc.ANGLES, H, W)
    return rc.xfm_points_restated(verts, mvp).contiguous(), f, H, W


def case_colour(kind, mask, seed):
    """The colour image of a case: the coverage mask [B,H,W,1], or a seeded random image with 3 or 8 channels."""
    if kind == "mask":
        return mask.to(torch.float32)[..., None].contiguous()
    C = {"c3": 3, "c8": 8}[kind]
    return torch.rand(*mask.shape, C, generator=torch.Generator().manual_seed(int(seed) + C))


def case_G(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def rast_restated(pos_clip, faces, H, W, ids=None):
    """The two `rast` layers of the rasterisation contract by its restatement, float32 [B,H,W,4] each; `ids` [B,2,H,W] when
    the caller has rasterised already."""
    ids = rc.rasterize_restated(pos_clip, faces, H, W)["ids"] if ids is None else ids
    if faces.shape[0] == 0:
        z = torch.zeros(ids.shape + (4,), dtype=torch.float32)
        return z[:, 0].contiguous(), z[:, 1].contiguous()
    u, v = rc.bary_restated(pos_clip, faces, ids, torch.float32)
    zf = rc.zf_restated(pos_clip, faces, ids, torch.float32)
    rast = torch.stack([u, v, zf, ids.to(torch.float32)], -1)
    return rast[:, 0].contiguous(), rast[:, 1].contiguous()


# ---- edge neighbours ---------------------------------------------------------------------------------------------------------------
def edge_neighbours_restated(faces, n_verts):
    """nbr int32 [F,3] (numpy) of faces [F,3]: the opposite vertex of the one other corner that owns the edge, else -1."""
    f = np.asarray(faces).reshape(-1, 3)
    owners = {}
    for fi in range(f.shape[0]):
        for k in range(3):
            a, b = int(f[fi, (k + 1) % 3]), int(f[fi, (k + 2) % 3])
            owners.setdefault((min(a, b), max(a, b)), []).append((fi, k))
    nbr = np.full(f.shape, -1, np.int32)
    for own in owners.values():
        if len(own) == 2:
            (f0, k0), (f1, k1) = own
            nbr[f0, k0], nbr[f1, k1] = f[f1, k1], f[f0, k0]
    return nbr


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def _pair_value_terms(pc, b, va, vb, pi, pj, s, d, H, W, dtype):
    """fu_a, fv_a, fu_b, fv_b of the contract for flat pair lists (direction d: 0 horizontal, 1 vertical)."""
    fx = ((2 * pj.to(dtype) + 1) / W - 1)
    fy = ((2 * pi.to(dtype) + 1) / H - 1)
    out = []
    for v in (va, vb):
        c = pc[b, v]
        px = (c[:, 0] / c[:, 3] - fx) * (W / 2)
        py = (c[:, 1] / c[:, 3] - fy) * (H / 2)
        out += [s.to(dtype) * px, py] if d == 0 else [s.to(dtype) * py, px]
    return out


def pair_decisions(rast, pos_clip, faces, nbr):
    """Every discrete decision of the contract.  rast float32 [B,H,W,4], pos_clip float32 [B,V,4], faces int64 [F,3], nbr
    int32 [F,3] -> dict of dense tensors [B,H,W,2] (last axis: the pair with the right neighbour, the pair with the pixel below;
    pairs that leave the image are inactive):
      active bool, va, vb int64 (the edge's vertices, -1 where inactive), p_first bool (P is the pair's first pixel),
      n_pass int64 (how many of T's edges pass all tests), edge int64 (the k of the chosen edge, -1)."""
    dev = rast.device
    B, H, W, _ = rast.shape
    F = faces.shape[0]
    ids, z = rast[..., 3].to(torch.int64), rast[..., 2].to(torch.float32)
    X, Y, ok = rc.snap(pos_clip, H, W)
    pc32 = pos_clip.to(torch.float32)
    res = dict(active=torch.zeros(B, H, W, 2, dtype=torch.bool, device=dev),
               va=torch.full((B, H, W, 2), -1, dtype=torch.int64, device=dev),
               vb=torch.full((B, H, W, 2), -1, dtype=torch.int64, device=dev),
               p_first=torch.zeros(B, H, W, 2, dtype=torch.bool, device=dev),
               n_pass=torch.zeros(B, H, W, 2, dtype=torch.int64, device=dev),
               edge=torch.full((B, H, W, 2), -1, dtype=torch.int64, device=dev))
    for d in (0, 1):
        first = (slice(None), slice(None), slice(0, W - 1)) if d == 0 else (slice(None), slice(0, H - 1), slice(None))
        second = (slice(None), slice(None), slice(1, W)) if d == 0 else (slice(None), slice(1, H), slice(None))
        t0, t1 = ids[first], ids[second]
        cand = (t0 != t1) & (t0 >= 0) & (t0 <= F) & (t1 >= 0) & (t1 <= F)
        b, i, j = torch.nonzero(cand, as_tuple=True)
        if b.numel() == 0:
            continue
        t0, t1, z0, z1 = t0[b, i, j], t1[b, i, j], z[first][b, i, j], z[second][b, i, j]
        p_first = torch.where(t0 == 0, torch.zeros_like(t0, dtype=torch.bool),
                              torch.where(t1 == 0, torch.ones_like(t0, dtype=torch.bool), z0 < z1))
        T = torch.where(p_first, t0, t1) - 1
        s = torch.where(p_first, 1, -1).to(torch.int64)
        pi = i + (0 if d == 0 else 1) * (~p_first).long()
        pj = j + (1 if d == 0 else 0) * (~p_first).long()
        Px, Py = 256 * pj + 128, 256 * pi + 128
        tri = faces[T]
        tri_ok = ok[b[:, None], tri].all(1)
        n_pass = torch.zeros_like(T)
        edge = torch.full_like(T, -1)
        for k in range(3):
            a, c, o = tri[:, (k + 1) % 3], tri[:, (k + 2) % 3], tri[:, k]
            Xa, Ya, Xb, Yb, Xo, Yo = X[b, a], Y[b, a], X[b, c], Y[b, c], X[b, o], Y[b, o]
            nb = nbr[T, k].to(torch.int64)
            nbc = nb.clamp_min(0)
            Xn, Yn, okn = X[b, nbc], Y[b, nbc], ok[b, nbc]
            dX, dY = Xb - Xa, Yb - Ya
            c1 = dX * (Yo - Ya) - dY * (Xo - Xa)
            c2 = dX * (Yn - Ya) - dY * (Xn - Xa)
            sil = (nb < 0) | ~okn | (torch.sign(c1) * torch.sign(c2) >= 0)
            if d == 0:
                orient = dY.abs() >= dX.abs()
                ua, wa, ub, wb = s * (Xa - Px), Ya - Py, s * (Xb - Px), Yb - Py
            else:
                orient = dX.abs() >= dY.abs()
                ua, wa, ub, wb = s * (Ya - Py), Xa - Px, s * (Yb - Py), Xb - Px
            den = wb - wa
            n = (ua * den - wa * (ub - ua)) * torch.sign(den)
            crossing = ((wa > 0) != (wb > 0)) & (n >= 0) & (n <= 256 * den.abs())
            passes = tri_ok & sil & orient & crossing
            n_pass += passes.long()
            edge = torch.where((edge < 0) & passes, torch.full_like(edge, k), edge)
        act = edge >= 0
        ek = edge.clamp_min(0)
        va = tri.gather(1, ((ek + 1) % 3)[:, None])[:, 0]
        vb = tri.gather(1, ((ek + 2) % 3)[:, None])[:, 0]
        _, fva, _, fvb = _pair_value_terms(pc32, b, va, vb, pi, pj, s, d, H, W, torch.float32)
        act = act & ((fvb - fva) != 0)                                          # the fp32 denominator of the value
        m1 = torch.full_like(va, -1)
        res["active"][b, i, j, d] = act
        res["va"][b, i, j, d] = torch.where(act, va, m1)
        res["vb"][b, i, j, d] = torch.where(act, vb, m1)
        res["p_first"][b, i, j, d] = p_first & act
        res["n_pass"][b, i, j, d] = n_pass
        res["edge"][b, i, j, d] = torch.where(act, edge, m1)
    return res


def pair_weights(pos_clip, dec, dtype=torch.float64):
    """The signed weight w = t - 0.5 of every active pair, [B,H,W,2] in `dtype`, 0 where inactive; differentiable w.r.t.
    pos_clip."""
    B, H, W, _ = dec["active"].shape
    pc = pos_clip.to(dtype)
    w = torch.zeros(B, H, W, 2, dtype=dtype, device=pc.device)
    for d in (0, 1):
        b, i, j = torch.nonzero(dec["active"][..., d], as_tuple=True)
        if b.numel() == 0:
            continue
        p_first = dec["p_first"][b, i, j, d]
        s = torch.where(p_first, 1, -1)
        pi = i + (0 if d == 0 else 1) * (~p_first).long()
        pj = j + (1 if d == 0 else 0) * (~p_first).long()
        fua, fva, fub, fvb = _pair_value_terms(pc, b, dec["va"][b, i, j, d], dec["vb"][b, i, j, d], pi, pj, s, d, H, W, dtype)
        t = (fua - fva * (fub - fua) / (fvb - fva)).clamp(0, 1)
        w = w.index_put((b, i, j, torch.full_like(b, d)), t - 0.5)
    return w


def antialias_restated(color, rast, pos_clip, faces, nbr, dtype=torch.float64, dec=None):
    """The contract's value [B,H,W,C] in `dtype`, differentiable w.r.t. color and pos_clip."""
    dec = pair_decisions(rast, pos_clip.detach(), faces, nbr) if dec is None else dec
    col = color.to(dtype)
    w = pair_weights(pos_clip, dec, dtype)
    act, p_first = dec["active"], dec["p_first"]
    recv_first = act & (p_first == (w < 0))                                     # w >= 0: Q receives; w < 0: P receives
    recv_second = act & ~recv_first
    mag = w.abs()[..., None]
    out = col
    zero = torch.zeros_like(col)
    # right pair, pair below, left pair, pair above, in that order
    term = zero.clone()
    term[:, :, :-1] = mag[:, :, :-1, 0] * (col[:, :, 1:] - col[:, :, :-1])
    out = torch.where(recv_first[..., 0:1], out + term, out)
    term = zero.clone()
    term[:, :-1] = mag[:, :-1, :, 1] * (col[:, 1:] - col[:, :-1])
    out = torch.where(recv_first[..., 1:2], out + term, out)
    term, m = zero.clone(), torch.zeros_like(recv_first[..., 0:1])
    term[:, :, 1:] = mag[:, :, :-1, 0] * (col[:, :, :-1] - col[:, :, 1:])
    m[:, :, 1:] = recv_second[:, :, :-1, 0:1]
    out = torch.where(m, out + term, out)
    term, m = zero.clone(), torch.zeros_like(recv_first[..., 0:1])
    term[:, 1:] = mag[:, :-1, :, 1] * (col[:, :-1] - col[:, 1:])
    m[:, 1:] = recv_second[:, :-1, :, 1:2]
    out = torch.where(m, out + term, out)
    return out


def grads_restated(color, rast, pos_clip, faces, nbr, G, dtype=torch.float64, dec=None):
    """(value, d color, d pos_clip) of sum(G * antialias) in `dtype`."""
    c = color.detach().to(dtype).requires_grad_(True)
    p = pos_clip.detach().to(dtype).requires_grad_(True)
    out = antialias_restated(c, rast, p, faces, nbr, dtype, dec)
    (out * G.to(dtype)).sum().backward()
    dp = p.grad if p.grad is not None else torch.zeros_like(p)
    return out.detach(), c.grad, dp


def silhouette_loss_restated(alpha, alpha_second, t_alpha, t_alpha_second):
    return ((alpha - t_alpha) ** 2).mean() + 0.1 * ((alpha_second - t_alpha_second) ** 2).mean()


def alpha_restated(verts, faces, mvp, H, W, dtype, rast=None):
    """(alpha, alpha_second, mask, mask_second) [B,H,W,1] in `dtype`: the antialiased coverage of both layers, differentiable
    w.r.t. verts through xfm_points; `rast` = the two layers, or None for the restated rasterisation of the fp32 clip positions."""
    pc = rc.xfm_points_restated(verts, mvp, dtype)
    pc32 = pc.detach().to(torch.float32)
    rast = rast_restated(pc32, faces, H, W) if rast is None else rast
    nbr = torch.as_tensor(edge_neighbours_restated(faces.cpu().numpy(), verts.shape[0]), device=faces.device)
    out = []
    for r in rast:
        mask = (r[..., 3:4] > 0).to(dtype)
        out.append((antialias_restated(mask, r, pc, faces, nbr, dtype, pair_decisions(r, pc32, faces, nbr)), mask))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def iou(a, b):
    a, b = a > 0.5, b > 0.5
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)
