"""The texture contract (header comment of meshdiffusion_amd/csrc/texture.hip) restated in numpy, for tests/test_cpu_texture.py,
tests/test_gpu_texture.py and tools/gen_golden_texture.py: the fetch in fp32 in the contract's own order (it reproduces the kernel
bit for bit) and in float64, the analytic gradients, one dilation step, the projection bake with its margins, the inputs of every
case, and a CPU pipeline (uv-space bake, textured render) over the restatements of raster_cases.py and interp_cases.py."""
import numpy as np
import torch

import raster_cases as rc

BAR_MARGIN = 4.0                       # a bar is BAR_MARGIN x the distance of the fp32 restatement from float64; where that is 0 so is the bar
KINK = 1e-4                            # d uv is discontinuous where x or y is an integer: such pixels are left out of its comparison
MARGIN = 1e-4                          # float64 distance to a threshold of the projection under which a texel may be left out
MAX_LEFT_OUT = 0.01                    # share of the masked texels


def bar(ref_err):
    return BAR_MARGIN * float(ref_err)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---- the fetch ------------------------------------------------------------------------------------------------------------------
def _index(f, n, wrap):
    if wrap:
        r = np.fmod(f, f.dtype.type(n))
        return np.where(r < 0, r + n, r).astype(np.int64)
    return np.clip(f, 0, n - 1).astype(np.int64)


def tap(uv, rast, Ht, Wt, boundary, dtype):
    """(live bool [B,H,W], ix0, ix1, iy0, iy1 int64, fx, fy in `dtype`) of uv float32 [B,H,W,2] by the contract."""
    wrap = boundary == "wrap"
    with np.errstate(all="ignore"):
        x = uv[..., 0].astype(dtype) * dtype(Wt) - dtype(0.5)
        y = uv[..., 1].astype(dtype) * dtype(Ht) - dtype(0.5)
        live = np.isfinite(uv[..., 0].astype(np.float32) * np.float32(Wt) - np.float32(0.5))     # skipped is decided in fp32
        live &= np.isfinite(uv[..., 1].astype(np.float32) * np.float32(Ht) - np.float32(0.5))
    x, y = np.where(live, x, dtype(0)), np.where(live, y, dtype(0))
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    ix0, iy0 = _index(x0, Wt, wrap), _index(y0, Ht, wrap)
    if wrap:
        ix1, iy1 = np.where(ix0 + 1 == Wt, 0, ix0 + 1), np.where(iy0 + 1 == Ht, 0, iy0 + 1)
    else:
        ix1, iy1 = _index(x0 + dtype(1), Wt, False), _index(y0 + dtype(1), Ht, False)
    if rast is not None:
        live = live & (rast[..., 3] != 0)
    return live, ix0, ix1, iy0, iy1, fx, fy, x, y


def _texels(tex, B, ix, iy):
    t = tex if tex.shape[0] > 1 else np.broadcast_to(tex, (B,) + tex.shape[1:])
    return t[np.arange(B)[:, None, None], iy, ix]                              # [B,H,W,C]


def sample_restated(tex, uv, rast=None, boundary="clamp", dtype=np.float32):
    """The contract's value [B,H,W,C] in `dtype`, each operation rounded on its own: tex float32 [T,Ht,Wt,C], uv float32 [B,H,W,2]."""
    tex = np.asarray(tex, np.float32).astype(dtype)
    T, Ht, Wt, C = tex.shape
    B = uv.shape[0]
    live, ix0, ix1, iy0, iy1, fx, fy, _, _ = tap(uv, rast, Ht, Wt, boundary, dtype)
    t00, t10 = _texels(tex, B, ix0, iy0), _texels(tex, B, ix1, iy0)
    t01, t11 = _texels(tex, B, ix0, iy1), _texels(tex, B, ix1, iy1)
    fx, fy = fx[..., None], fy[..., None]
    gx, gy = dtype(1) - fx, dtype(1) - fy
    with np.errstate(all="ignore"):
        out = (t00 * gx + t10 * fx) * gy + (t01 * gx + t11 * fx) * fy
    return np.where(live[..., None], out, dtype(0)).astype(dtype)


def sample_grads_restated(tex, uv, G, rast=None, boundary="clamp", dtype=np.float64):
    """(d tex [T,Ht,Wt,C], d uv [B,H,W,2], kink bool [B,H,W]) of sum(G * sample) by the contract's formulas in `dtype`; the sums
    over codes are numpy's (np.add.at, in code order, uncompensated).  kink: x or y closer than KINK to an integer."""
    tex = np.asarray(tex, np.float32).astype(dtype)
    G = np.asarray(G, np.float32).astype(dtype)
    T, Ht, Wt, C = tex.shape
    B = uv.shape[0]
    live, ix0, ix1, iy0, iy1, fx, fy, x, y = tap(uv, rast, Ht, Wt, boundary, dtype)
    t00, t10 = _texels(tex, B, ix0, iy0), _texels(tex, B, ix1, iy0)
    t01, t11 = _texels(tex, B, ix0, iy1), _texels(tex, B, ix1, iy1)
    gx, gy = dtype(1) - fx, dtype(1) - fy
    du = ((G * ((t10 - t00) * gy[..., None] + (t11 - t01) * fy[..., None])).sum(-1)) * dtype(Wt)
    dv = ((G * ((t01 - t00) * gx[..., None] + (t11 - t10) * fx[..., None])).sum(-1)) * dtype(Ht)
    duv = np.where(live[..., None], np.stack([du, dv], -1), dtype(0)).astype(dtype)
    dtex = np.zeros((T * Ht * Wt, C), dtype)
    base = (np.arange(B) * Ht * Wt if T > 1 else np.zeros(B, np.int64))[:, None, None]
    rows = np.stack([base + iy0 * Wt + ix0, base + iy0 * Wt + ix1, base + iy1 * Wt + ix0, base + iy1 * Wt + ix1], -1)    # [B,H,W,4]
    w = np.stack([gx * gy, fx * gy, gx * fy, fx * fy], -1)
    terms = w[..., None] * G[..., None, :]                                      # [B,H,W,4,C]
    keep = np.broadcast_to(live[..., None], rows.shape)
    np.add.at(dtex, rows[keep], terms[keep])
    kink = (np.abs(x - np.rint(x)) < KINK) | (np.abs(y - np.rint(y)) < KINK)
    return dtex.reshape(T, Ht, Wt, C), duv, kink


# ---- inputs of the fetch cases --------------------------------------------------------------------------------------------------
# (texture (Ht, Wt), C, T, B, image (H, W), boundary, with a rast): every texture, channel count, (T, B), image and boundary of
# the issue at least once, the 16-byte paths (C = 4, 8) with and without a rast
SAMPLE_CASES = (
    ((1, 1), 1, 1, 3, (1, 1), "clamp", False), ((1, 1), 3, 2, 2, (7, 5), "wrap", True),
    ((1, 5), 3, 1, 3, (7, 5), "clamp", True), ((1, 5), 4, 2, 2, (17, 33), "wrap", False),
    ((2, 2), 1, 2, 2, (7, 5), "clamp", False), ((2, 2), 8, 1, 3, (17, 33), "wrap", True),
    ((5, 3), 3, 1, 3, (17, 33), "clamp", True), ((5, 3), 4, 1, 3, (7, 5), "wrap", True), ((5, 3), 8, 2, 2, (1, 1), "clamp", False),
    ((64, 64), 1, 1, 3, (17, 33), "wrap", False), ((64, 64), 3, 2, 2, (17, 33), "clamp", True),
    ((64, 64), 4, 1, 3, (17, 33), "clamp", False), ((64, 64), 8, 2, 2, (7, 5), "wrap", True),
    # the remaining channel counts of the compile-time dispatch
    ((5, 3), 2, 1, 3, (7, 5), "clamp", True), ((2, 2), 5, 2, 2, (7, 5), "wrap", False),
    ((1, 5), 6, 1, 3, (7, 5), "wrap", True), ((64, 64), 7, 2, 2, (7, 5), "clamp", False),
)
# backward only: a 64 x 64 image onto a 2 x 2 texture (rows of about 4096 codes), a 3 x 3 image onto a 64 x 64 texture
EXTRA_BWD_CASES = (((2, 2), 3, 1, 1, (64, 64), "clamp", False), ((64, 64), 3, 1, 1, (3, 3), "clamp", False))
BWD_CASES = SAMPLE_CASES + EXTRA_BWD_CASES


def sample_case_id(case):
    (Ht, Wt), C, T, B, (H, W), boundary, with_rast = case
    return f"tex{Ht}x{Wt}c{C}-T{T}B{B}-img{H}x{W}-{boundary}" + ("-rast" if with_rast else "")


def sample_case_inputs(case):
    """(tex float32 [T,Ht,Wt,C], uv float32 [B,H,W,2], rast float32 [B,H,W,4] or None, G float32 [B,H,W,C]) numpy.  uv by pixel:
    exact texel centres, exact texel borders, 0 and 1, values in [-1.5, 2.5] (twice), values in [0, 1]; three pixels NaN / inf."""
    (Ht, Wt), C, T, B, (H, W), boundary, with_rast = case
    rng = np.random.default_rng(1000 + BWD_CASES.index(case))
    tex = rng.standard_normal((T, Ht, Wt, C)).astype(np.float32)
    n = B * H * W
    kind = np.arange(n) % 6
    size = np.array([Wt, Ht])
    cell = rng.integers(0, size, (n, 2))
    uv = rng.uniform(-1.5, 2.5, (n, 2))
    uv = np.where((kind == 0)[:, None], (cell + 0.5) / size, uv)
    uv = np.where((kind == 1)[:, None], cell / size, uv)
    uv = np.where((kind == 2)[:, None], rng.integers(0, 2, (n, 2)).astype(np.float64), uv)
    uv = np.where((kind == 5)[:, None], rng.uniform(0, 1, (n, 2)), uv).astype(np.float32)
    if case in EXTRA_BWD_CASES:
        uv = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    elif n >= 8:
        uv[3, 0], uv[5, 1], uv[7, 0] = np.nan, np.inf, -np.inf
    rast = None
    if with_rast:
        rast = rng.standard_normal((B, H, W, 4)).astype(np.float32)
        rast[..., 3] = np.where(rng.uniform(size=(B, H, W)) < 0.25, 0.0, rng.integers(1, 50, (B, H, W))).astype(np.float32)
    G = rng.standard_normal((B, H, W, C)).astype(np.float32)
    return tex, uv.reshape(B, H, W, 2), rast, G


# ---- dilation -------------------------------------------------------------------------------------------------------------------
def dilate_restated(tex, mask, dtype=np.float64):
    """One step of the contract: tex [Ht,Wt,C], mask [Ht,Wt] -> (tex, mask) in `dtype`; the neighbours are added in row-major order."""
    tex, m = np.asarray(tex, np.float32).astype(dtype), np.asarray(mask) > 0.5
    Ht, Wt, C = tex.shape
    tp, mp = np.zeros((Ht + 2, Wt + 2, C), dtype), np.zeros((Ht + 2, Wt + 2), bool)
    tp[1:-1, 1:-1], mp[1:-1, 1:-1] = tex, m
    total, count = np.zeros((Ht, Wt, C), dtype), np.zeros((Ht, Wt), np.int64)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                nm = mp[dy:dy + Ht, dx:dx + Wt]
                total = total + np.where(nm[..., None], tp[dy:dy + Ht, dx:dx + Wt], dtype(0))
                count += nm
    grow = ~m & (count > 0)
    out = np.where(grow[..., None], total / np.maximum(count, 1)[..., None].astype(dtype), tex)
    return out.astype(dtype), np.where(grow, 1.0, np.asarray(mask, np.float64)).astype(np.float32)


def dilate_cases():
    """name -> (tex float32 [Ht,Wt,C], mask float32 [Ht,Wt])."""
    rng = np.random.default_rng(77)
    one = np.zeros((5, 5), np.float32)
    one[2, 1] = 1
    ii, jj = np.meshgrid(np.arange(6), np.arange(7), indexing="ij")
    cases = {"one-texel": (rng.standard_normal((5, 5, 3)), one), "checkerboard": (rng.standard_normal((6, 7, 4)), ((ii + jj) % 2)),
             "empty": (rng.standard_normal((4, 6, 1)), np.zeros((4, 6))), "full": (rng.standard_normal((4, 6, 8)), np.ones((4, 6))),
             "c3-33x17": (rng.standard_normal((33, 17, 3)), rng.uniform(size=(33, 17)) < 0.15)}
    for c in (2, 5, 6, 7):                                                      # the remaining channel counts of the dispatch
        cases[f"c{c}-9x6"] = (rng.standard_normal((9, 6, c)), rng.uniform(size=(9, 6)) < 0.2)
    return {k: (t.astype(np.float32), np.asarray(m, np.float32)) for k, (t, m) in cases.items()}


# ---- the projection bake --------------------------------------------------------------------------------------------------------
def project_restated(pos, nrm, texmask, image, depth, viewmask, mvp, campos, depth_bias=0.01, cos_min=0.1, power=2.0, dtype=np.float64):
    """(color [Ht,Wt,3], weight [Ht,Wt], unsafe bool [Ht,Wt]) of the contract in `dtype`.  unsafe: a test that a view reached came
    closer than MARGIN to its threshold (w, the frustum, the pixel lattice of the footprint and of the nearest pixel, depth_bias,
    cos_min), so an fp32 evaluation may decide it the other way."""
    f = lambda a: np.asarray(a, np.float32).astype(dtype)
    pos, nrm, image, depth, mvp, campos = f(pos), f(nrm), f(image), f(depth), f(mvp), f(campos)
    vm = np.asarray(viewmask, np.float32) > 0.5
    V, H, W, _ = image.shape
    P, N = pos.reshape(-1, 3), nrm.reshape(-1, 3)
    on = (np.asarray(texmask, np.float32) > 0.5).reshape(-1)
    acc, wsum, unsafe = np.zeros((P.shape[0], 3), dtype), np.zeros(P.shape[0], dtype), np.zeros(P.shape[0], bool)
    one, half = dtype(1), dtype(0.5)
    with np.errstate(all="ignore"):
        for v in range(V):
            m = mvp[v]
            cx = ((P[:, 0] * m[0, 0] + P[:, 1] * m[0, 1]) + P[:, 2] * m[0, 2]) + m[0, 3]
            cy = ((P[:, 0] * m[1, 0] + P[:, 1] * m[1, 1]) + P[:, 2] * m[1, 2]) + m[1, 3]
            cw = ((P[:, 0] * m[3, 0] + P[:, 1] * m[3, 1]) + P[:, 2] * m[3, 2]) + m[3, 3]
            alive = on.copy()
            unsafe |= alive & (np.abs(cw) < MARGIN)
            alive &= cw > 0
            cws = np.where(alive, cw, one)
            nx, ny = cx / cws, cy / cws
            unsafe |= alive & ((np.abs(np.abs(nx) - 1) < MARGIN) | (np.abs(np.abs(ny) - 1) < MARGIN))
            alive &= (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1)
            nx, ny = np.where(alive, nx, 0), np.where(alive, ny, 0)
            px, py = (nx * half + half) * dtype(W) - half, (ny * half + half) * dtype(H) - half
            d3 = campos[v][None] - P
            d = np.sqrt((d3[:, 0] * d3[:, 0] + d3[:, 1] * d3[:, 1]) + d3[:, 2] * d3[:, 2])

            def decide(qx, qy):
                """(the footprint lies inside the image on foreground pixels, d - depth at the nearest pixel) at (qx, qy)"""
                ax, ay = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
                inside = (ax >= 0) & (ay >= 0) & (ax + 1 < W) & (ay + 1 < H)
                ax, ay = np.where(inside, ax, 0), np.where(inside, ay, 0)
                fg = inside & vm[v, ay, ax] & vm[v, ay, ax + 1] & vm[v, ay + 1, ax] & vm[v, ay + 1, ax + 1]
                bx = np.clip(np.floor(qx + half).astype(np.int64), 0, W - 1)
                by = np.clip(np.floor(qy + half).astype(np.int64), 0, H - 1)
                return fg, d - depth[v, by, bx]

            fg, behind = decide(px, py)
            for ox, oy in ((MARGIN, 0), (-MARGIN, 0), (0, MARGIN), (0, -MARGIN)):       # the pixel lattice: would a neighbour decide otherwise?
                fg2, behind2 = decide(px + dtype(ox), py + dtype(oy))
                unsafe |= alive & ((fg2 != fg) | (fg & ((behind2 > dtype(depth_bias)) != (behind > dtype(depth_bias)))))
            x0f, y0f = np.floor(px), np.floor(py)
            alive &= fg
            x0, y0 = np.where(alive, x0f.astype(np.int64), 0), np.where(alive, y0f.astype(np.int64), 0)
            unsafe |= alive & (np.abs(behind - dtype(depth_bias)) < MARGIN)
            alive &= ~(behind > dtype(depth_bias))
            cs = ((N[:, 0] * d3[:, 0] + N[:, 1] * d3[:, 1]) + N[:, 2] * d3[:, 2]) / np.where(d > 0, d, one)
            unsafe |= alive & (np.abs(cs - dtype(cos_min)) < MARGIN)
            alive &= cs > dtype(cos_min)
            w = np.where(alive, np.power(np.where(alive, cs, one), dtype(power)), dtype(0))
            fx, fy = (px - x0f)[:, None], (py - y0f)[:, None]
            gx, gy = one - fx, one - fy
            img = image[v]
            col = (img[y0, x0] * gx + img[y0, x0 + 1] * fx) * gy + (img[y0 + 1, x0] * gx + img[y0 + 1, x0 + 1] * fx) * fy
            acc = acc + np.where(alive[:, None], w[:, None] * col, dtype(0))
            wsum = wsum + w
        color = np.where((wsum > 0)[:, None], acc / np.where(wsum > 0, wsum, one)[:, None], dtype(0))
    Ht, Wt = pos.shape[:2]
    return color.reshape(Ht, Wt, 3).astype(dtype), wsum.reshape(Ht, Wt).astype(dtype), unsafe.reshape(Ht, Wt)


# ---- meshes, cameras and the smooth colour of the baking cases --------------------------------------------------------------------
def cube_mesh(n=8, half=0.55):
    """A cube of side 2 half with n x n quads a face, 12 n^2 faces, outward normals: (verts float32 [V,3], faces int64 [F,3])."""
    lin = np.linspace(-half, half, n + 1)
    a, b = np.meshgrid(lin, lin, indexing="ij")
    verts, faces = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            p = np.zeros((n + 1, n + 1, 3))
            p[..., axis], p[..., (axis + 1) % 3], p[..., (axis + 2) % 3] = sign * half, a, b
            idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1) + len(verts) * (n + 1) ** 2
            q = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 4)
            tri = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
            faces.append(tri if sign > 0 else tri[:, ::-1])
            verts.append(p.reshape(-1, 3))
    return torch.tensor(np.concatenate(verts), dtype=torch.float32), torch.tensor(np.concatenate(faces).copy(), dtype=torch.int64)


def sphere_mesh(n_lat=16, n_lon=32, radius=0.7):
    """A latitude-longitude sphere, 2 n_lon (n_lat - 1) faces (960), outward normals, shared vertices."""
    verts = [[0.0, radius, 0.0]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            verts.append([radius * np.sin(th) * np.cos(ph), radius * np.cos(th), radius * np.sin(th) * np.sin(ph)])
    verts.append([0.0, -radius, 0.0])
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    faces = []
    for j in range(n_lon):
        faces.append([0, ring(1, j + 1), ring(1, j)])
        faces.append([len(verts) - 1, ring(n_lat - 1, j), ring(n_lat - 1, j + 1)])
        for i in range(1, n_lat - 1):
            faces.append([ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)])
            faces.append([ring(i, j), ring(i + 1, j + 1), ring(i + 1, j)])
    return torch.tensor(verts, dtype=torch.float32), torch.tensor(faces, dtype=torch.int64)


MESHES = {"cube": cube_mesh, "sphere": sphere_mesh}
# (mesh, views, image side, atlas side)
# eight views go to the sphere: about 0.13 % of a cube's texels per view lie within MARGIN of a threshold (its flat sides cross
# depth_bias along whole lines), which eight views would carry past MAX_LEFT_OUT; the sphere's 960 faces get the 256 atlas, whose
# 39k masked texels make the share a steadier number than the 4k of the 128 atlas
PROJECT_CASES = (("cube", 4, 64, 128), ("cube", 4, 96, 128), ("sphere", 8, 64, 256), ("sphere", 8, 96, 256))
ROUND_TRIP = ("sphere", 8, 96, 256)    # the end-to-end scene


def project_case_id(case):
    return f"{case[0]}-{case[1]}views-{case[2]}px-atlas{case[3]}"


def view_cameras(n_views, side):
    """n_views cameras of raster_cases.camera around the object, alternately from above and below: (mvp [V,4,4], campos [V,3])."""
    ms, cs = [], []
    for k in range(n_views):
        mvp, campos = rc.camera(2 * np.pi * k / n_views + 0.3, side, side)
        if k % 2:                                                               # mirror the camera through y = 0
            flip = torch.diag(torch.tensor([1.0, -1.0, 1.0, 1.0]))
            mvp, campos = mvp @ flip, campos * torch.tensor([1.0, -1.0, 1.0])
        ms.append(mvp), cs.append(campos)
    return torch.stack(ms).contiguous(), torch.stack(cs).contiguous()


def smooth_color(p):
    """A smooth colour in [0.1, 0.9] of the position p [...,3] (numpy or torch)."""
    s, c = (torch.sin, torch.cos) if torch.is_tensor(p) else (np.sin, np.cos)
    stack = torch.stack if torch.is_tensor(p) else np.stack
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return stack([0.5 + 0.4 * s(2.0 * x + 0.5 * y), 0.5 + 0.4 * c(1.5 * y - z), 0.5 + 0.4 * s(1.7 * z + x * y)], -1)


# ---- a CPU pipeline over the restatements of raster_cases.py (the generator; no GPU) ------------------------------------------------
def _interp(attr, faces, ids, u, v):
    tri = faces[(ids - 1).clamp_min(0)]
    a = attr.to(torch.float64)
    out = (u[..., None] * a[tri[..., 0]] + v[..., None] * a[tri[..., 1]]) + ((1 - u) - v)[..., None] * a[tri[..., 2]]
    return torch.where((ids > 0)[..., None], out, torch.zeros_like(out))


def vertex_normals64(verts, faces):
    v = verts.to(torch.float64)
    fn = torch.linalg.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    vn = torch.zeros_like(v)
    for k in range(3):
        vn.index_add_(0, faces[:, k], fn)
    return vn / vn.norm(dim=1, keepdim=True).clamp_min(1e-10), fn


def atlas_clip(uvs):
    uv = uvs.to(torch.float32)
    return torch.cat([uv * 2 - 1, torch.zeros_like(uv[:, :1]), torch.ones_like(uv[:, :1])], -1)[None].contiguous()


def render_uv_cpu(verts, faces, uvs, uv_idx, R):
    """`texture.render_uv` from the restatements: dict of numpy mask [R,R], pos, normal [R,R,3] (float64), face_id, uv [R,R,2]."""
    clip = atlas_clip(uvs)
    ids = rc.rasterize_restated(clip, uv_idx, R, R)["ids"][:, :1]
    u, v = rc.bary_restated(clip, uv_idx, ids)
    vn, _ = vertex_normals64(verts, faces)
    pos, nrm = _interp(verts, faces, ids, u, v)[0, 0], _interp(vn, faces, ids, u, v)[0, 0]
    nrm = nrm / nrm.norm(dim=-1, keepdim=True).clamp_min(1e-10)
    tuv = _interp(uvs, uv_idx, ids, u, v)[0, 0]
    cov = ids[0, 0] > 0
    return {"mask": cov.numpy().astype(np.float32), "pos": pos.numpy(), "normal": (nrm * cov[..., None]).numpy(),
            "face_id": (ids[0, 0] - 1).numpy(), "uv": tuv.numpy()}


def views_cpu(verts, faces, uvs, uv_idx, mvp, campos, side):
    """Layer 1 of every view from the restatements: dict of numpy depth [V,H,W] (20 where uncovered), mask [V,H,W], pos [V,H,W,3],
    uv [V,H,W,2] (the interpolated texture coordinates), all float64."""
    pc = rc.xfm_points_restated(verts, mvp)
    ids = rc.rasterize_restated(pc, faces, side, side)["ids"][:, :1]
    u, v = rc.bary_restated(pc, faces, ids)
    depth = rc.depth_restated(verts, faces, mvp, campos, torch.cat([ids, torch.zeros_like(ids)], 1))[:, 0]
    pos = _interp(verts, faces, ids, u, v)[:, 0]
    tuv = torch.zeros(ids.shape[0], side, side, 2, dtype=torch.float64) if uvs is None else _interp(uvs, uv_idx, ids, u, v)[:, 0]
    return {"depth": depth.numpy(), "mask": (ids[:, 0] > 0).numpy().astype(np.float32), "pos": pos.numpy(), "uv": tuv.numpy()}
