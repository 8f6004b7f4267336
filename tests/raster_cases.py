"""Cases and torch restatements of the rasterisation contract (the header comment of csrc/raster.hip), so that a machine
without the reference can evaluate it on any input.  Shared by tools/gen_golden_raster.py, the CPU tests, the GPU tests and
tools/bench_raster.py.

  snap / rasterize_restated   the contract by brute force: fp32 snap (as the contract demands, torch reproduces X and Y
                              exactly), int64 coverage over the (pixel, triangle) pairs expanded from the bounding boxes,
                              fragment depth and key order in float64.
  bary_restated / depth_restated   u, v and the depth buffers with the face ids GIVEN, under torch autograd, in fp32 or
                              float64: the oracle of the value and gradient tests and of the fitting loop.
Every restatement runs on the device of its inputs.
"""
import functools
import math
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZF_GAP = 1e-6                          # float64 key gap under which an fp32 evaluation may order two fragments either way
SLIVER = 1000.0                        # max edge^2 / |A2| (snapped units) above which the winner's numbers are ill-conditioned
EXCLUDE_CAP = 0.005                    # each exclusion may take at most 0.5 % of the covered pixels of its case
MESH_SCALE = 2.1
ANGLES = (0.7, 2.1)
MESH_CASES = (("sphere", 64, 64), ("sphere", 40, 72), ("torus", 64, 64), ("torus", 40, 72), ("noise", 32, 32))
GRAD_CASES = MESH_CASES[:4]            # the cases of 1(e)
FIT_STEPS = (0, 10, 20, 40)
FIT_ITERS = 41
FIT_LR = 0.03
FIT_SDF_REGULARIZER = 0.2
FIT_RES = 64
FIT_ANGLES = (0.0, math.pi / 2, math.pi, 3 * math.pi / 2)
FIT_START_RADIUS = 0.9


def case_id(case):
    return f"{case[0]}-{case[1]}x{case[2]}"


# ---- camera (float64 numpy, rounded to float32 at the end: the reference builds float32 tensors from numpy doubles) --------
def perspective64(fovy, aspect, n, f):
    y = np.tan(fovy / 2)
    return np.array([[1 / (y * aspect), 0, 0, 0], [0, -1 / y, 0, 0], [0, 0, -(f + n) / (f - n), -(2 * f * n) / (f - n)],
                     [0, 0, -1, 0]], np.float64)


def camera(angle, H, W):
    """perspective(45 deg, W/H, 0.1, 1000) @ translate(0, 0, -3) @ rotate_x(-0.4) @ rotate_y(angle): (mvp [4,4], campos [3]),
    both float32; campos = the camera centre, inv(modelview)[:3, 3]."""
    def f32(m):
        return torch.tensor(m, dtype=torch.float32)
    s, c = np.sin(-0.4), np.cos(-0.4)
    rx = f32([[1, 0, 0, 0], [0, c, s, 0], [0, -s, c, 0], [0, 0, 0, 1]])
    s, c = np.sin(angle), np.cos(angle)
    ry = f32([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    tr = f32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -3], [0, 0, 0, 1]])
    mv = tr @ rx @ ry
    mvp = f32(perspective64(np.deg2rad(45.0), W / H, 0.1, 1000.0)) @ tr @ rx @ ry      # left to right, as the expression reads
    return mvp, torch.linalg.inv(mv)[:3, 3].contiguous()


def cameras(angles, H, W):
    ms, cs = zip(*(camera(a, H, W) for a in angles))
    return torch.stack(ms), torch.stack(cs)


# ---- meshes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tet_grid():
    t = np.load(os.path.join(GOLD, "64_tets_cropped.npz"))
    return t["vertices"], t["indices"]


def case_sdf(name, p):
    """The analytic SDFs of the cases at the points p [N,3] (float32 torch)."""
    if name == "sphere":
        return p.norm(dim=1) - 0.7
    if name == "torus":                                                        # R = 0.6, r = 0.25, around y
        return torch.sqrt((torch.sqrt(p[:, 0] ** 2 + p[:, 2] ** 2) - 0.6) ** 2 + p[:, 1] ** 2) - 0.25
    if name == "noise":
        return torch.rand(p.shape[0], generator=torch.Generator().manual_seed(0)) * 2 - 1
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """Marching tetrahedra (oracle/dmtet_oracle.py, numpy, CPU) of the case's SDF on the shipped grid x 2.1:
    (verts float32 [V,3], faces int64 [F,3]) CPU tensors."""
    from oracle import dmtet_oracle
    verts, idx = tet_grid()
    p = torch.as_tensor(verts, dtype=torch.float32) * MESH_SCALE
    v, f, _ = dmtet_oracle.marching_tets(p.numpy(), case_sdf(name, p).numpy(), idx)
    return torch.as_tensor(v), torch.as_tensor(f)


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def xfm_points_restated(points, matrix, dtype=torch.float32):
    """[V,3] or [1|B,V,3] points, [B,4,4] matrices -> [B,V,4] = matrix (p, 1), the four products summed left to right."""
    p = points.to(dtype)
    p = p[None] if p.dim() == 2 else p
    m = matrix.to(dtype)[:, None]                                              # [B,1,4,4]
    return ((p[..., 0:1] * m[..., 0] + p[..., 1:2] * m[..., 1]) + p[..., 2:3] * m[..., 2]) + m[..., 3]


def snap(pos_clip, H, W):
    """fp32 torch: (X int64 [B,V], Y int64 [B,V], vertex_ok bool [B,V])."""
    pc = pos_clip.to(torch.float32)
    w = pc[..., 3]
    ok = torch.isfinite(pc).all(-1) & (w > 0)
    ws = torch.where(ok, w, torch.ones_like(w))
    lim = float(2 ** 22)
    X = torch.round(((pc[..., 0] / ws) * 0.5 + 0.5) * float(256 * W)).clamp(-lim, lim)
    Y = torch.round(((pc[..., 1] / ws) * 0.5 + 0.5) * float(256 * H)).clamp(-lim, lim)
    X = torch.where(ok, X, torch.zeros_like(X))
    Y = torch.where(ok, Y, torch.zeros_like(Y))
    return X.to(torch.int64), Y.to(torch.int64), ok


def _owns_zero(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def rasterize_restated(pos_clip, faces, H, W):
    """The contract by brute force.  pos_clip float32 [B,V,4], faces int64 [F,3] -> dict of
      ids [B,2,H,W] int64 (face + 1, 0 = uncovered), zf [B,2,H,W] float64 (0 where uncovered),
      gap12, gap23 [B,H,W] float64: zf gap between keys 1-2 and 2-3 (inf when the later key does not exist),
      sliver [B,2,H,W] float64: max edge^2 / |A2| of the winner in snapped units (0 where uncovered),
      on_edge: the number of (pixel, triangle) pairs with a centre exactly on an edge of a non-skipped triangle,
      max_frags: the largest number of fragments of a pixel."""
    dev = pos_clip.device
    B = pos_clip.shape[0]
    F = faces.shape[0]
    ids = torch.zeros(B, 2, H * W, dtype=torch.int64, device=dev)
    zf_out = torch.zeros(B, 2, H * W, dtype=torch.float64, device=dev)
    sliver = torch.zeros(B, 2, H * W, dtype=torch.float64, device=dev)
    gaps = torch.full((B, 2, H * W), float("inf"), dtype=torch.float64, device=dev)
    on_edge, max_frags = 0, 0
    if F == 0:
        return dict(ids=ids.view(B, 2, H, W), zf=zf_out.view(B, 2, H, W), gap12=gaps[:, 0].view(B, H, W),
                    gap23=gaps[:, 1].view(B, H, W), sliver=sliver.view(B, 2, H, W), on_edge=0, max_frags=0)
    Xa, Ya, oka = snap(pos_clip, H, W)
    for b in range(B):
        X, Y = Xa[b][faces], Ya[b][faces]                                      # [F,3]
        ok = oka[b][faces].all(1)
        A2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
        ok = ok & (A2 != 0)
        # pixel centres 256 j + 128 inside the bounding box
        j0 = torch.div(X.min(1).values - 128 + 255, 256, rounding_mode="floor").clamp_min(0)
        j1 = torch.div(X.max(1).values - 128, 256, rounding_mode="floor").clamp_max(W - 1)
        i0 = torch.div(Y.min(1).values - 128 + 255, 256, rounding_mode="floor").clamp_min(0)
        i1 = torch.div(Y.max(1).values - 128, 256, rounding_mode="floor").clamp_max(H - 1)
        nj, ni = (j1 - j0 + 1).clamp_min(0), (i1 - i0 + 1).clamp_min(0)
        cnt = torch.where(ok, nj * ni, torch.zeros_like(nj))
        tri = torch.repeat_interleave(torch.arange(F, device=dev), cnt)
        if tri.numel() == 0:
            continue
        start = torch.cumsum(cnt, 0) - cnt
        local = torch.arange(tri.numel(), device=dev) - start[tri]
        pj = j0[tri] + local % nj[tri]
        pi = i0[tri] + torch.div(local, nj[tri], rounding_mode="floor")
        Qx, Qy = 256 * pj + 128, 256 * pi + 128
        s = torch.sign(A2)[tri]
        cov = torch.ones_like(tri, dtype=torch.bool)
        touch = torch.zeros_like(cov)
        e = []
        for k in range(3):                                                      # the edge opposite vertex k
            a, c = (k + 1) % 3, (k + 2) % 3
            dx, dy = s * (X[tri, c] - X[tri, a]), s * (Y[tri, c] - Y[tri, a])
            ek = dx * (Qy - Y[tri, a]) - dy * (Qx - X[tri, a])
            cov &= (ek > 0) | ((ek == 0) & _owns_zero(dx, dy))
            touch |= ek == 0
            e.append(ek)
        inside_closed = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
        on_edge += int((touch & inside_closed).sum())
        pc64 = pos_clip[b].to(torch.float64)
        zw = (pc64[:, 2] / pc64[:, 3])[faces]                                   # [F,3]
        A2o = (s * A2[tri]).to(torch.float64)
        zf = sum((e[k].to(torch.float64) / A2o) * zw[tri, k] for k in range(3))
        keep = cov & (zf >= -1) & (zf <= 1)
        tri, zf, pix = tri[keep], zf[keep] + 0.0, (pi * W + pj)[keep]
        if tri.numel() == 0:
            continue
        # order by (pixel, zf, face): three stable sorts, least significant first
        o = torch.sort(tri, stable=True).indices
        o = o[torch.sort(zf[o], stable=True).indices]
        o = o[torch.sort(pix[o], stable=True).indices]
        tri, zf, pix = tri[o], zf[o], pix[o]
        first = torch.ones_like(pix, dtype=torch.bool)
        first[1:] = pix[1:] != pix[:-1]
        seg_start = torch.nonzero(first)[:, 0]
        seg_id = torch.cumsum(first, 0) - 1
        rank = torch.arange(pix.numel(), device=dev) - seg_start[seg_id]
        max_frags = max(max_frags, int(rank.max()) + 1)
        E2 = torch.stack([(X[:, (k + 2) % 3] - X[:, (k + 1) % 3]) ** 2 + (Y[:, (k + 2) % 3] - Y[:, (k + 1) % 3]) ** 2
                          for k in range(3)], 1).max(1).values.to(torch.float64)
        sl = E2 / A2.abs().clamp_min(1).to(torch.float64)
        for layer in range(2):
            m = rank == layer
            ids[b, layer, pix[m]] = tri[m] + 1
            zf_out[b, layer, pix[m]] = zf[m]
            sliver[b, layer, pix[m]] = sl[tri[m]]
        for g in range(2):                                                      # gap between rank g and rank g + 1
            m = torch.zeros_like(first)
            m[1:] = (rank[1:] == g + 1)
            idx = torch.nonzero(m)[:, 0]
            gaps[b, g, pix[idx]] = zf[idx] - zf[idx - 1]
    return dict(ids=ids.view(B, 2, H, W), zf=zf_out.view(B, 2, H, W), gap12=gaps[:, 0].view(B, H, W),
                gap23=gaps[:, 1].view(B, H, W), sliver=sliver.view(B, 2, H, W), on_edge=on_edge, max_frags=max_frags)


def left_out(r):
    """(order [B,2,H,W], numeric [B,2,H,W]) bool: the pixels a comparison may leave out.  order: the float64 keys the layer
    depends on are closer than ZF_GAP (keys 1-2 for layer 1, keys 2-3 as well for layer 2).  numeric: the winner is a sliver."""
    near12, near23 = r["gap12"] < ZF_GAP, r["gap23"] < ZF_GAP
    order = torch.stack([near12, near12 | near23], 1)
    return order, r["sliver"] > SLIVER


def check_caps(r, name):
    """The 0.5 % caps of both exclusions; returns (order, numeric, covered) with the counts printed."""
    order, numeric = left_out(r)
    covered = r["ids"] > 0
    n = int(covered[:, 0].sum())
    n_order, n_num = int((order[:, 1] & covered[:, 0]).sum()), int((numeric & covered).any(1).sum())
    print(f"[raster] {name}: covered {n} second layer {int(covered[:, 1].sum())} max fragments {r['max_frags']} centres on "
          f"edges {r['on_edge']} smallest gaps {float(r['gap12'].min()):.2e} / {float(r['gap23'].min()):.2e} largest sliver "
          f"ratio {float(r['sliver'].max()):.0f} left out: order {n_order} numeric {n_num}")
    assert n_order <= EXCLUDE_CAP * n and n_num <= EXCLUDE_CAP * n, (name, n_order, n_num, n)
    return order, numeric, covered


def pixel_ndc(H, W, device, dtype):
    fy = (2 * torch.arange(H, device=device, dtype=dtype) + 1) / H - 1
    fx = (2 * torch.arange(W, device=device, dtype=dtype) + 1) / W - 1
    return fx[None, None, None, :], fy[None, None, :, None]                    # broadcast over [B,2,H,W]


def bary_restated(pos_clip, faces, ids, dtype=torch.float64):
    """u, v [B,2,H,W] in `dtype` from the unsnapped clip floats, ids given (0 where uncovered, as rast holds)."""
    B, _, H, W = ids.shape
    pc = pos_clip.to(dtype)
    fx, fy = pixel_ndc(H, W, pc.device, dtype)
    tri = faces[(ids - 1).clamp_min(0)]                                         # [B,2,H,W,3]
    bi = torch.arange(B, device=pc.device)[:, None, None, None]
    px, py = [], []
    for k in range(3):
        c = pc[bi, tri[..., k]]                                                # [B,2,H,W,4]
        px.append(c[..., 0] - fx * c[..., 3])
        py.append(c[..., 1] - fy * c[..., 3])
    a0 = px[1] * py[2] - py[1] * px[2]
    a1 = px[2] * py[0] - py[2] * px[0]
    a2 = px[0] * py[1] - py[0] * px[1]
    s = (a0 + a1) + a2
    cov = ids > 0
    s = torch.where(cov, s, torch.ones_like(s))
    zero = torch.zeros_like(s)
    return torch.where(cov, a0 / s, zero), torch.where(cov, a1 / s, zero)


def zf_restated(pos_clip, faces, ids, dtype=torch.float64):
    """zf [B,2,H,W] of the contract in `dtype` for the given ids (0 where uncovered): exact integer edge functions of the
    fp32 snap, then sum_k (e_k / A2) zw_k with zw = z / w, all in `dtype`."""
    B, _, H, W = ids.shape
    dev = pos_clip.device
    X, Y, _ = snap(pos_clip, H, W)
    tri = faces[(ids - 1).clamp_min(0)]
    bi = torch.arange(B, device=dev)[:, None, None, None]
    Xt, Yt = X[bi[..., None], tri], Y[bi[..., None], tri]                       # [B,2,H,W,3]
    Qx = (256 * torch.arange(W, device=dev) + 128)[None, None, None, :]
    Qy = (256 * torch.arange(H, device=dev) + 128)[None, None, :, None]
    pc = pos_clip.to(dtype)
    zw = (pc[..., 2] / pc[..., 3])[bi[..., None], tri]
    e = []
    for k in range(3):
        a, c = (k + 1) % 3, (k + 2) % 3
        e.append((Xt[..., c] - Xt[..., a]) * (Qy - Yt[..., a]) - (Yt[..., c] - Yt[..., a]) * (Qx - Xt[..., a]))
    A2 = ((e[0] + e[1]) + e[2]).to(dtype)
    cov = ids > 0
    A2 = torch.where(cov, A2, torch.ones_like(A2))
    zf = ((e[0].to(dtype) / A2) * zw[..., 0] + (e[1].to(dtype) / A2) * zw[..., 1]) + (e[2].to(dtype) / A2) * zw[..., 2]
    return torch.where(cov, zf, torch.zeros_like(zf))


def depth_restated(verts, faces, mvp, campos, ids, dtype=torch.float64):
    """depth [B,2,H,W] in `dtype` (20 / -1 where uncovered) of world verts [V,3] through pos_clip = mvp (P, 1), ids given.
    Differentiable w.r.t. `verts` when it requires a gradient (both the attribute and the barycentric path)."""
    v = verts.to(dtype)
    pc = xfm_points_restated(v, mvp, dtype)
    u, w = bary_restated(pc, faces, ids, dtype)
    tri = faces[(ids - 1).clamp_min(0)]
    P0, P1, P2 = v[tri[..., 0]], v[tri[..., 1]], v[tri[..., 2]]
    gb = (u[..., None] * P0 + w[..., None] * P1) + ((1 - u) - w)[..., None] * P2
    d = gb - campos.to(dtype)[:, None, None, None, :]
    cov = ids > 0
    d = torch.where(cov[..., None], d, torch.ones_like(d))                      # keeps sqrt away from 0 on the background
    depth = torch.sqrt((d * d).sum(-1))
    bg = torch.tensor([20.0, -1.0], dtype=dtype, device=depth.device)[None, :, None, None].expand_as(depth)
    return torch.where(cov, depth, bg)


def grad_restated(verts, faces, mvp, campos, ids, G, dtype=torch.float64):
    """d sum(G * depth) / d verts, G [B,2,H,W], by autograd over depth_restated in `dtype`."""
    v = verts.detach().to(dtype).requires_grad_(True)
    (depth_restated(v, faces, mvp, campos, ids, dtype) * G.to(dtype)).sum().backward()
    return v.grad


def case_G(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- small hand-made cases (face ids only) ---------------------------------------------------------------------------------------
def _ndc_of_fixed(X, Y, H, W):
    """An NDC position that snaps exactly to the 1/256-pixel position (X, Y)."""
    return X / (128.0 * W) - 1.0, Y / (128.0 * H) - 1.0


def small_case(name):
    """(pos_clip float32 [1,V,4], faces int64 [F,3], H, W)"""
    H = W = 8
    if name == "quad":              # corners on pixel centres: the diagonal and the outer edges pass through centres
        c = [(1, 1), (6, 1), (6, 6), (1, 6)]
        v = [(*_ndc_of_fixed(256 * x + 128, 256 * y + 128, H, W), 0.25 + 0.05 * k, 1.0) for k, (x, y) in enumerate(c)]
        return torch.tensor(v, dtype=torch.float32)[None], torch.tensor([[0, 1, 2], [0, 2, 3]]), H, W
    if name == "huge":              # larger than the viewport, vertices far off screen: the +-2^22 clamp
        v = [(-5e4, -4e4, 0.1, 1.0), (7e4, -3e4, 0.2, 1.0), (1e3, 9e4, 0.3, 1.0)]
        return torch.tensor(v, dtype=torch.float32)[None], torch.tensor([[0, 1, 2]]), H, W
    if name == "skipped":           # one w < 0, and a zero-area triangle: both skipped; a third triangle stays
        v = [(-0.9, -0.9, 0.1, 1.0), (0.9, -0.9, 0.1, 1.0), (0.0, 0.9, 0.1, -1.0), (0.5, 0.5, 0.2, 1.0), (-0.5, -0.5, 0.2, 1.0),
             (0.0, 0.0, 0.2, 1.0), (-0.7, 0.8, 0.3, 2.0), (0.8, 0.7, 0.3, 1.5), (0.1, -0.8, 0.3, 1.0)]
        return torch.tensor(v, dtype=torch.float32)[None], torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8]]), H, W
    if name == "empty":
        v = [(-0.5, -0.5, 0.1, 1.0), (0.5, -0.5, 0.1, 1.0), (0.0, 0.5, 0.1, 1.0)]
        return torch.tensor(v, dtype=torch.float32)[None], torch.zeros(0, 3, dtype=torch.int64), H, W
    if name == "coincident":        # two copies of one triangle: layer 1 the lower index, layer 2 the higher
        v = [(-0.8, -0.7, 0.1, 1.0), (0.9, -0.6, 0.4, 1.3), (-0.1, 0.8, 0.2, 0.9)]
        return torch.tensor(v, dtype=torch.float32)[None], torch.tensor([[0, 1, 2], [0, 1, 2]]), H, W
    if name == "fan":               # 8 triangles around the centre of pixel (4, 4): every edge through it is shared
        cx, cy = 256 * 4 + 128, 256 * 4 + 128
        ring = [(900, 0), (900, 900), (0, 900), (-900, 900), (-900, 0), (-900, -900), (0, -900), (900, -900)]
        v = [(*_ndc_of_fixed(cx, cy, H, W), 0.5, 1.0)] + [(*_ndc_of_fixed(cx + x, cy + y, H, W), 0.5, 1.0) for x, y in ring]
        f = [[0, 1 + k, 1 + (k + 1) % 8] if k % 2 == 0 else [0, 1 + (k + 1) % 8, 1 + k] for k in range(8)]   # mixed orientation
        return torch.tensor(v, dtype=torch.float32)[None], torch.tensor(f), H, W
    raise KeyError(name)


SMALL_CASES = ("quad", "huge", "skipped", "empty", "coincident")


# ---- the depth loss, literally ------------------------------------------------------------------------------------------------------
def depth_loss_restated(depth, depth_second, t_depth, t_depth_second, mask_cont, iteration):
    """The depth terms of DMTetGeometry.tick (dmtet.py:402-434), all [B,H,W,1]."""
    mask = (mask_cont[..., 0] == 1.0).to(depth.dtype)[..., None]
    valid = (t_depth_second >= 0).to(depth.dtype)
    prox = ((t_depth_second - t_depth).abs() >= 5e-3).to(depth.dtype)
    d1 = (depth - t_depth).abs() * mask * valid
    d2 = (depth_second - t_depth_second).abs() * mask * valid * prox * 0.1
    scale = 100.0 if iteration < 10000 else 1.0
    out = 0.0
    for d in (d1, d2):
        l1 = (d < 1.0).to(d.dtype)
        out = out + (l1 * d + (1 - l1) * (d.pow(2) + 1.0 - 1.0 ** 2)).mean() * scale
    return out


# ---- the fitting run ---------------------------------------------------------------------------------------------------------------
def fit_initial_sdf(verts_scaled):
    """The fit starts from a sphere of radius FIT_START_RADIUS (positive outside, as the targets are written): wide enough to
    cover the torus's silhouette (outer radius 0.85) in every view.  A target pixel the prediction does not cover holds the
    constant 20.0, a term of (20 - d)^2 x 100 without a gradient, so a start that leaves such pixels cannot be judged by its loss."""
    return (verts_scaled.norm(dim=1) - FIT_START_RADIUS).clamp(-1.0, 1.0)


def fit_cameras():
    return cameras(FIT_ANGLES, FIT_RES, FIT_RES)


def targets_restated(verts, faces, mvp, campos, H, W, dtype):
    """make_targets by the restatement: the buffers of the ground-truth mesh, [B,H,W,1] each, in `dtype`."""
    pc = xfm_points_restated(verts, mvp, dtype).to(torch.float32)
    ids = rasterize_restated(pc, faces, H, W)["ids"]
    d = depth_restated(verts, faces, mvp, campos, ids, dtype)
    return dict(depth=d[:, 0, :, :, None], depth_second=d[:, 1, :, :, None], mask_cont=(ids[:, 0] > 0).to(dtype)[..., None])
