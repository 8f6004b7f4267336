"""Cases and numpy / torch restatements of the mesh post-processing contract (the header comment of csrc/meshpost.hip): the edge
table, umbrella smoothing, connected components, the floater filter, diffuse shading from nine spherical-harmonic coefficients and
their projection from a lat-long map.  Shared by tools/gen_golden_meshpost.py, the CPU tests, the GPU tests and
tools/bench_meshpost.py.  Everything runs on the CPU; the smoothing and the shading take a dtype, so that the fp32 restatement's
own distance from float64 is the unit of the GPU tests' bars.
"""
import functools
import math

import numpy as np
import torch

import antialias_cases as ac
import interp_cases as ic
import raster_cases as rc

CASES = ("quad", "fan40", "degen", "ptorus", "noise", "pair", "strip4096")
STRIP = 4096
STRIP_SEED = 5
DEGEN_LABELS = [0, 0, 0, 0, 4, 5, 5, 5]
MAX_ROUNDS = 64
# (name, steps, lam, mu) of the smoothing settings
SMOOTH_SETTINGS = (("lap1", 1, 0.5, None), ("lap3", 3, 0.5, None), ("lap10", 10, 0.5, None), ("taubin10", 10, 0.5, -0.53))
SHADE_CASES = ic.BUFFER_CASES + (("quad", 16, 16), ("fan40", 16, 16))
LIGHTS = ("random", "default")
SH_SEED = 23
A_HAT = (1.0, 2 / 3, 2 / 3, 2 / 3, 0.25, 0.25, 0.25, 0.25, 0.25)
ENV_RES = (64, 128)


# ---- meshes ----------------------------------------------------------------------------------------------------------------------
def concat(parts):
    """[(verts, faces), ...] -> (verts, faces of global ids, vert_mesh int32 [V])."""
    vs, fs, vm, base = [], [], [], 0
    for k, (v, f) in enumerate(parts):
        vs.append(v)
        fs.append(f + base)
        vm.append(torch.full((v.shape[0],), k, dtype=torch.int32))
        base += v.shape[0]
    return torch.cat(vs), torch.cat(fs), torch.cat(vm)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts float32 [V,3], faces int64 [F,3]) on the CPU, left unchanged by every user."""
    if name in ("quad", "fan40", "degen", "ptorus"):
        return ic.mesh(name)
    if name == "noise":
        return rc.mesh("noise")
    if name == "pair":
        return concat([mesh("ptorus"), mesh("fan40")])[:2]
    if name == "strip4096":         # triangle i = (i, i+1, i+2), then every vertex renumbered by a seeded permutation
        i = torch.arange(STRIP)
        f = torch.stack([i, i + 1 + i % 2, i + 2 - i % 2], 1)
        k = torch.arange(STRIP + 2, dtype=torch.float64)
        v = torch.stack([0.01 * torch.div(k, 2, rounding_mode="floor"), 0.02 * (k % 2), 0.003 * torch.sin(0.37 * k)], 1).to(torch.float32)
        perm = torch.randperm(STRIP + 2, generator=torch.Generator().manual_seed(STRIP_SEED))
        out = torch.empty_like(v)
        out[perm] = v
        return out, perm[f]
    raise KeyError(name)


def vert_mesh(name):
    if name == "pair":
        return concat([mesh("ptorus"), mesh("fan40")])[2]
    return torch.zeros(mesh(name)[0].shape[0], dtype=torch.int32)


# ---- the edge table ----------------------------------------------------------------------------------------------------------------
def edges_restated(faces, n_verts):
    """(lo, hi, mult int64 [E], ptr int32 [V+1], adj int32 [2 E]) numpy, by the contract: a dictionary of the undirected corner
    edges, then every row listed in ascending order of the neighbour."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = int(n_verts)
    a, b = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    keep = a != b
    key = np.minimum(a, b)[keep] * V + np.maximum(a, b)[keep]
    key, mult = np.unique(key, return_counts=True)
    lo, hi = key // max(V, 1), key % max(V, 1)
    bnd = (mult == 1).astype(np.int64)
    row = np.concatenate([lo, hi])
    nbr = np.concatenate([hi, lo])
    code = 2 * nbr + np.concatenate([bnd, bnd])
    order = np.lexsort((nbr, row))
    ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=V), out=ptr[1:])
    return lo, hi, mult.astype(np.int64), ptr.astype(np.int32), code[order].astype(np.int32)


def smoothing_rows(faces, n_verts):
    """(nb int64 [V,D] padded with -1, n int64 [V]): the codes each vertex averages, in row order -- all of them, or only the
    boundary codes on a boundary vertex."""
    _, _, _, ptr, adj = edges_restated(faces, n_verts)
    V = int(n_verts)
    ptr, adj = ptr.astype(np.int64), adj.astype(np.int64)
    row = np.repeat(np.arange(V), ptr[1:] - ptr[:-1])
    is_b = np.zeros(V, bool)
    is_b[row[(adj & 1) == 1]] = True
    use = ~is_b[row] | ((adj & 1) == 1)
    row, nbr = row[use], adj[use] >> 1
    n = np.bincount(row, minlength=V)
    start = np.cumsum(n) - n
    D = int(n.max()) if n.size and n.max() > 0 else 1
    nb = np.full((V, D), -1, np.int64)
    nb[row, np.arange(row.size) - start[row]] = nbr
    return nb, n


def smooth_restated(verts, faces, steps=3, lam=0.5, mu=None, dtype=torch.float64, rows=None):
    """The contract's smoothing in `dtype`: per step and vertex the compensated (Kahan) sum of the row in row order, every
    operation rounded on its own (elementwise torch), m = s / n, x' = x + w (m - x); n == 0 keeps the vertex."""
    x = verts.to(dtype).clone()
    nb, n = smoothing_rows(faces, x.shape[0]) if rows is None else rows
    nb_t, n_t = torch.as_tensor(nb), torch.as_tensor(n)
    has = (n_t > 0)[:, None]
    cnt = n_t.clamp_min(1).to(dtype)[:, None]
    for i in range(int(steps)):
        w = lam if (i % 2 == 0 or mu is None or math.isnan(mu)) else mu
        s, lost = torch.zeros_like(x), torch.zeros_like(x)
        for j in range(nb_t.shape[1]):
            on = (nb_t[:, j] >= 0)[:, None]
            q = x[nb_t[:, j].clamp_min(0)]
            y = q - lost
            t = s + y
            lost = torch.where(on, (t - s) - y, lost)
            s = torch.where(on, t, s)
        m = s / cnt
        x = torch.where(has, x + torch.tensor(w, dtype=dtype) * (m - x), x)
    return x


# ---- connected components ----------------------------------------------------------------------------------------------------------
def components_restated(faces, n_verts):
    """(label int32 [V], comp_faces int32 [V]) numpy: scipy's connected components of the graph of the face corners,
    canonicalised to the smallest vertex index; comp_faces[label] = the faces whose first vertex carries the label."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = int(n_verts)
    a, b = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    _, comp = connected_components(coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(V, V)), directed=False)
    smallest = np.full(comp.max() + 1 if V else 0, V, np.int64)
    np.minimum.at(smallest, comp, np.arange(V))
    label = smallest[comp]
    return label.astype(np.int32), np.bincount(label[f[:, 0]], minlength=V).astype(np.int32)


def rounds_simulated(faces, n_verts, max_rounds=MAX_ROUNDS):
    """The hook-and-compress rounds of the contract with every kernel run synchronously (all faces read the labels of the round's
    start): (label int32 [V], rounds), rounds counting the last one, which lowers nothing."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = np.arange(int(n_verts), dtype=np.int64)
    for r in range(1, max_rounds + 1):
        roots = label[f]                                                        # compressed: the label of a vertex is its root
        m = roots.min(1)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, roots[:, k], m)
        lowered = bool((new < label).any())
        label = new
        while True:                                                             # compress
            nxt = label[label]
            if (nxt == label).all():
                break
            label = nxt
        if not lowered:
            return label.astype(np.int32), r
    raise RuntimeError(f"no fixed point in {max_rounds} rounds")


def drop_floaters_restated(verts, faces, *, min_faces=1, min_fraction=0.0, keep_largest=False, vert_mesh=None):
    """(verts', faces', vert_map int64 [V], face_keep bool [F]) numpy, by the contract's rule on the restated components."""
    v, f = np.asarray(verts), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = v.shape[0]
    vm = np.zeros(V, np.int64) if vert_mesh is None else np.asarray(vert_mesh, dtype=np.int64)
    label, cf = components_restated(f, V)
    cf = cf.astype(np.int64)
    M = int(vm.max()) + 1
    largest = np.zeros(M, np.int64)
    np.maximum.at(largest, vm, cf)
    need = np.maximum(np.ceil(float(min_fraction) * largest.astype(np.float64)).astype(np.int64), max(int(min_faces), 1))
    ok = cf >= need[vm]
    if keep_largest:
        winner = np.full(M, V, np.int64)
        for r in np.nonzero(cf >= 1)[0]:                                        # ascending: the first of the largest wins a tie
            if cf[r] == largest[vm[r]] and winner[vm[r]] == V:
                winner[vm[r]] = r
        ok &= np.arange(V) == winner[vm]
    vert_keep = ok[label]
    face_keep = vert_keep[f[:, 0]]
    vert_map = np.where(vert_keep, np.cumsum(vert_keep) - 1, -1).astype(np.int64)
    return v[vert_keep], vert_map[f[face_keep]], vert_map, face_keep


# ---- shading -----------------------------------------------------------------------------------------------------------------------
def sh_basis_restated(n):
    """[...,3] unit vectors -> [...,9] in the dtype of n, the constants of the contract."""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    return torch.stack([torch.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * (x * y), 1.092548 * (y * z),
                        0.315392 * (3 * (z * z) - 1), 1.092548 * (x * z), 0.546274 * (x * x - y * y)], -1)


def _dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])[..., None]


def shade_restated(rast, verts, faces, campos, sh, kd, dtype=torch.float64, front=None):
    """(out [B,H,W,4], geo . view [B,H,W] (1 where uncovered), covered bool [B,H,W]) of the contract's shading in `dtype`; `front`
    bool [B,H,W] fixes the flip decision."""
    B, H, W, _ = rast.shape
    F = faces.shape[0]
    cov = ic.covered(rast, F) if F > 0 else torch.zeros(B, H, W, dtype=torch.bool)
    v = verts.to(dtype)
    t3 = faces[(rast[..., 3].to(torch.int64) - 1).clamp(0, max(F - 1, 0))] if F > 0 else torch.zeros(B, H, W, 3, dtype=torch.int64)
    p0, p1, p2 = v[t3[..., 0]], v[t3[..., 1]], v[t3[..., 2]]
    u, w = rast[..., 0:1].to(dtype), rast[..., 1:2].to(dtype)
    p = (u * p0 + w * p1) + ((1 - u) - w) * p2
    g = torch.linalg.cross(p1 - p0, p2 - p0)
    geo = g / torch.sqrt(torch.clamp(_dot(g, g), min=1e-20))
    d = campos.to(dtype)[:, None, None, :] - p
    view = d / torch.clamp(torch.sqrt(_dot(d, d)), min=1e-12)
    gv = _dot(geo, view)
    fr = gv > 0 if front is None else front[..., None]
    n = torch.where(fr, geo, -geo)
    ay = sh_basis_restated(n) * torch.tensor(A_HAT, dtype=dtype)
    s = sh.to(dtype)
    e = ay[..., 0:1] * s[0]
    for k in range(1, 9):
        e = e + ay[..., k:k + 1] * s[k]
    rgb = kd.to(dtype) * torch.clamp(e, min=0)
    out = torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1)
    out = torch.where(cov[..., None], out, torch.zeros_like(out))
    return out, torch.where(cov, gv[..., 0], torch.ones_like(gv[..., 0])), cov


def case_light(kind):
    """(sh float32 [9,3], kd float32 [3]) of a shading case: a seeded random light and colour, or the library's default light
    with the reference's kd."""
    if kind == "random":
        gen = torch.Generator().manual_seed(SH_SEED)
        sh = torch.randn(9, 3, generator=gen) * 0.3
        sh[0] += 1.5
        return sh, torch.rand(3, generator=gen) * 0.8 + 0.1
    from meshdiffusion_amd import render
    return torch.as_tensor(render.default_light()), torch.tensor(render.PREVIEW_KD, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def shade_inputs(case):
    """(verts, faces, mvp, campos, pos_clip, H, W, rast float32 [B,H,W,4] by the CPU restatement of the rasteriser)."""
    verts, faces, mvp, campos, pc, H, W = ic.case_inputs(case)
    return verts, faces, mvp, campos, pc, H, W, ac.rast_restated(pc, faces, H, W)[0]


def rgb_rel_l2(a, b, cov):
    """rel-L2 of the rgb channels over the covered pixels."""
    return rc.rel_l2(a[..., :3][cov], b[..., :3][cov])


# ---- the light ---------------------------------------------------------------------------------------------------------------------
def latlong_restated(h, w):
    """(directions [h,w,3], solid angles [h,w]) float64 of the texel centres: the direction whose lat-long coordinates
    tu = atan2(x, -z) / 2 pi + 1/2, tv = acos(y) / pi are the centre's."""
    tv, tu = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    theta, phi = tv * np.pi, (tu - 0.5) * 2 * np.pi
    d = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], -1)
    assert np.allclose(np.arctan2(d[..., 0], -d[..., 2]) / (2 * np.pi) + 0.5, tu) and np.allclose(np.arccos(d[..., 1]) / np.pi, tv)
    return d, np.sin(theta) * (np.pi / h) * (2 * np.pi / w)


def sh9_restated(env):
    """float64 [9,3]: sum over the texels of env Y_k sin(theta) d theta d phi."""
    env = np.asarray(env, dtype=np.float64)
    d, dw = latlong_restated(env.shape[0], env.shape[1])
    Y = sh_basis_restated(torch.as_tensor(d)).numpy()
    return np.stack([[(env[..., c] * Y[..., k] * dw).sum() for c in range(3)] for k in range(9)])


def irradiance_brute(env, normals):
    """The cosine integral by brute force: (1 / pi) sum over the texels of env max(0, n . d) d omega, float64 [N,3]."""
    env = np.asarray(env, dtype=np.float64)
    d, dw = latlong_restated(env.shape[0], env.shape[1])
    cosine = np.maximum(np.einsum("nk,hwk->nhw", np.asarray(normals, dtype=np.float64), d), 0.0)
    return np.einsum("nhw,hwc,hw->nc", cosine, env, dw) / np.pi


def irradiance_sh(sh, normals):
    """sum_k A_k sh[k] Y_k(n) in float64, [N,3]."""
    Y = sh_basis_restated(torch.as_tensor(np.asarray(normals, dtype=np.float64))).numpy()
    return np.einsum("nk,kc->nc", Y * np.asarray(A_HAT), np.asarray(sh, dtype=np.float64))


def smooth_env(h=ENV_RES[0], w=ENV_RES[1]):
    """A smooth analytic environment, a polynomial of degree two in the direction (so band-limited to the nine coefficients):
    float64 [h,w,3]."""
    d, _ = latlong_restated(h, w)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([0.50 + 0.15 * y + 0.10 * x * z - 0.05 * x,
                     0.45 + 0.10 * y - 0.08 * y * z + 0.05 * z + 0.04 * (x * x - y * y),
                     0.55 + 0.12 * y + 0.06 * x * y + 0.05 * (3 * z * z - 1)], -1)


def seeded_normals(n=200, seed=3):
    v = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy()
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def srgb(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 0.0031308, np.maximum(x, 0.0031308) ** (1 / 2.4) * 1.055 - 0.055, 12.92 * x)


# ---- synthetic samples of the command-line test -------------------------------------------------------------------------------------
def sphere_and_blob_samples(R=64, M=2):
    """[M,4,R,R,R] float32: channel 0 the sign of a sphere plus a small far-away blob (a floater), no deformation."""
    k = (torch.arange(R, dtype=torch.float32) + 0.5) / R - 0.5
    z, y, x = torch.meshgrid(k, k, k, indexing="ij")
    out = torch.zeros(M, 4, R, R, R)
    for m in range(M):
        ball = torch.sqrt(x * x + y * y + z * z) - (0.25 + 0.04 * m)
        blob = torch.sqrt((x - 0.38) ** 2 + (y - 0.38) ** 2 + (z + 0.38) ** 2) - 0.05
        out[m, 0] = torch.sign(torch.minimum(ball, blob))
    return out.numpy()
