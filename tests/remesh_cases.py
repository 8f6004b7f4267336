"""Cases and the numpy restatement of the remeshing contract (the header comment of csrc/remesh.hip): split, collapse, flip and
relax written as plain loops over edges, faces and vertices in float32 scalars, one operation at a time, so that every decision of
the kernels is reproduced exactly; the relax pass also takes float64, whose distance from the float32 form is the unit of the GPU
test's bar.  A validity checker (closed orientable manifold per mesh) and the quality figures are here too.  Shared by
tools/gen_golden_remesh.py, the CPU tests, the GPU tests and tools/bench_remesh.py.  Everything runs on the CPU.
"""
import functools
import math

import numpy as np
import torch

import meshpost_cases as mc

CASES = ("tetra", "octa", "uvsphere", "ptorus", "fan40", "quad", "degen", "pair")
CLOSED = ("tetra", "octa", "uvsphere", "ptorus")
EXACT_CASES = ("uvsphere", "ptorus", "fan40", "pair")
PIPELINE_CASES = ("uvsphere", "ptorus", "pair")
QUALITY_CASES = (("uvsphere", 1.0), ("uvsphere", 0.6), ("ptorus", 1.0), ("ptorus", 0.6))
COLLAPSE_ROUNDS, FLIP_ROUNDS, MAX_ITERS = 8, 4, 32
PIPELINE_ITERS = 5
F32 = np.float32
ONES64 = (1 << 64) - 1


# ---- meshes ----------------------------------------------------------------------------------------------------------------------
def uv_sphere(stacks, slices):
    """The unit sphere cut into `stacks` bands and `slices` sectors: two poles of valence `slices`, slivers next to them."""
    th = np.pi * np.arange(1, stacks) / stacks
    ph = 2 * np.pi * np.arange(slices) / slices
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(slices))], -1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    idx = lambda i, j: 1 + i * slices + j % slices
    south = 1 + (stacks - 1) * slices
    f = []
    for j in range(slices):
        f.append((0, idx(0, j), idx(0, j + 1)))
        for i in range(stacks - 2):
            f.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            f.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
        f.append((south, idx(stacks - 2, j + 1), idx(stacks - 2, j)))
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts float32 [V,3], faces int64 [F,3]) on the CPU, left unchanged by every user."""
    if name == "tetra":
        v = torch.tensor([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], dtype=torch.float32) * 0.5
        return v, torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    if name == "octa":
        v = torch.tensor([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=torch.float32)
        return v, torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    if name == "uvsphere":
        return uv_sphere(12, 24)
    if name == "uvsphere48":
        return uv_sphere(48, 96)
    return mc.mesh(name)


def vert_mesh(name):
    return mc.vert_mesh(name) if name == "pair" else torch.zeros(mesh(name)[0].shape[0], dtype=torch.int32)


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def repeated(f):
    return (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])


def tables(faces, V):
    """The tables of the contract from the faces of the moment, numpy: dict(lo, hi, mult, ptr, adj, cptr, corner, vflag, index)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lo, hi, mult, ptr, adj = mc.edges_restated(f, V)
    flat = f.reshape(-1)
    corner = np.argsort(flat, kind="stable").astype(np.int32)
    cptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=V), out=cptr[1:])
    vflag = np.zeros(V, np.int32)
    for sel, bit in ((mult == 1, 1), (mult >= 3, 2)):
        vflag[lo[sel]] |= bit
        vflag[hi[sel]] |= bit
    vflag[f[repeated(f)].reshape(-1)] |= 2
    index = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(lo, hi))}
    return dict(lo=lo, hi=hi, mult=mult, ptr=ptr.astype(np.int64), adj=adj.astype(np.int64), cptr=cptr, corner=corner.astype(np.int64),
                vflag=vflag, index=index)


def edge_lengths64(verts, lo, hi):
    """float64 lengths of the table's edges from the float32 coordinates, every operation on its own."""
    x = np.asarray(verts, dtype=np.float64)
    d = x[hi] - x[lo]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def default_target(verts, faces, vm, M):
    """float32 [M]: per mesh the sequential float64 sum, in table order, of the edge lengths over their number (1 without edges)."""
    lo, hi, _, _, _ = mc.edges_restated(faces, np.asarray(verts).shape[0])
    em = np.asarray(vm, dtype=np.int64)[lo]
    s = np.bincount(em, weights=edge_lengths64(verts, lo, hi), minlength=M)
    n = np.bincount(em, minlength=M)
    return np.where(n > 0, s / np.maximum(n, 1), 1.0).astype(np.float32)


def bands(target):
    """(lo2, hi2) float32 [M] of float32 targets: computed in float64, rounded once."""
    t = np.asarray(target, dtype=np.float32).astype(np.float64)
    return ((0.8 * t) ** 2).astype(np.float32), ((4.0 / 3.0 * t) ** 2).astype(np.float32)


# ---- arithmetic of the contract --------------------------------------------------------------------------------------------------
def _pt(x, v):
    return (x[v, 0], x[v, 1], x[v, 2])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _len2(a, b):
    d = _sub(a, b)
    return _dot(d, d)


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _nrm(p0, p1, p2):
    return _cross(_sub(p1, p0), _sub(p2, p0))


def _mid(a, b):
    h = type(a[0])(0.5)
    return (h * (a[0] + b[0]), h * (a[1] + b[1]), h * (a[2] + b[2]))


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def _corners(T, f, v):
    """The corner row of v: (face, i0, i1, i2) rotated so that i0 sits at the corner."""
    for j in range(T["cptr"][v], T["cptr"][v + 1]):
        code = int(T["corner"][j])
        t, k = code // 3, code % 3
        yield t, int(f[t, k]), int(f[t, (k + 1) % 3]), int(f[t, (k + 2) % 3])


def _row(T, v):
    return [int(c) >> 1 for c in T["adj"][T["ptr"][v]:T["ptr"][v + 1]]]


# ---- split -----------------------------------------------------------------------------------------------------------------------
def split_restated(verts, faces, vm, hi2):
    """One split pass: (verts', faces', vert_mesh', number of marked edges)."""
    x, f, vm = np.asarray(verts, dtype=np.float32), np.asarray(faces, dtype=np.int64), np.asarray(vm, dtype=np.int32)
    V = x.shape[0]
    T = tables(f, V)
    lo, hi = T["lo"], T["hi"]
    E = lo.shape[0]
    with np.errstate(all="ignore"):
        mark = np.array([_len2(_pt(x, lo[e]), _pt(x, hi[e])) > hi2[vm[lo[e]]] for e in range(E)], dtype=bool)
        mids = np.array([_mid(_pt(x, lo[e]), _pt(x, hi[e])) for e in range(E)], dtype=np.float32).reshape(E, 3)
    n = int(mark.sum())
    if n == 0:
        return x.copy(), f.copy(), vm.copy(), 0
    rank = np.cumsum(mark) - mark
    out = []
    for t in range(f.shape[0]):
        v = [int(i) for i in f[t]]
        if v[0] == v[1] or v[1] == v[2] or v[2] == v[0]:
            out.append(tuple(v))
            continue
        e = [T["index"][(min(v[(k + 1) % 3], v[(k + 2) % 3]), max(v[(k + 1) % 3], v[(k + 2) % 3]))] for k in range(3)]
        mk = [bool(mark[e[k]]) for k in range(3)]
        m = [V + int(rank[e[k]]) if mk[k] else None for k in range(3)]
        k = sum(mk)
        if k == 0:
            out.append(tuple(v))
        elif k == 3:
            out += [(v[0], m[2], m[1]), (v[1], m[0], m[2]), (v[2], m[1], m[0]), (m[0], m[1], m[2])]
        elif k == 1:
            j = mk.index(True)
            out += [(v[j], v[(j + 1) % 3], m[j]), (v[j], m[j], v[(j + 2) % 3])]
        else:
            j = mk.index(False)
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            out.append((v[j], m[j2], m[j1]))
            l2 = _len2(_pt(x, v[j]), _pt(x, v[j1]))
            l1 = _len2(_pt(x, v[j2]), _pt(x, v[j]))
            if l2 > l1 or (l2 == l1 and e[j2] < e[j1]):
                out += [(m[j2], v[j1], v[j2]), (m[j2], v[j2], m[j1])]
            else:
                out += [(m[j1], m[j2], v[j1]), (m[j1], v[j1], v[j2])]
    f2 = np.array(out, dtype=np.int64).reshape(-1, 3)
    x2 = np.concatenate([x, mids[mark]])
    vm2 = np.concatenate([vm, vm[lo[mark]]])
    order = np.argsort(vm2, kind="stable")
    inv = np.empty_like(order)
    inv[order] = np.arange(order.shape[0])
    return x2[order], inv[f2], vm2[order], n


# ---- collapse --------------------------------------------------------------------------------------------------------------------
def _collapse_ok(x, f, T, vm, lo2, hi2, e):
    a, b = int(T["lo"][e]), int(T["hi"][e])
    if T["mult"][e] != 2 or T["vflag"][a] != 0 or T["vflag"][b] != 0:
        return None
    A, B = _pt(x, a), _pt(x, b)
    l2 = _len2(A, B)
    if not l2 < lo2[vm[a]]:
        return None
    h2 = hi2[vm[a]]
    opp = [(i2 if i1 == b else i1) for _, i0, i1, i2 in _corners(T, f, a) if i1 == b or i2 == b]
    if len(opp) != 2 or opp[0] == opp[1]:
        return None
    ra, rb = _row(T, a), _row(T, b)
    common = sorted(set(ra) & set(rb))
    if common != sorted(opp):
        return None
    if any(T["ptr"][c + 1] - T["ptr"][c] <= 3 for c in opp) or len(ra) + len(rb) - 4 < 3:
        return None
    p = _mid(A, B)
    for xv in ra + rb:
        if xv != a and xv != b and not _len2(_pt(x, xv), p) <= h2:
            return None
    for v, w in ((a, b), (b, a)):
        for _, i0, i1, i2 in _corners(T, f, v):
            if i1 == w or i2 == w:
                continue
            P0, P1, P2 = _pt(x, i0), _pt(x, i1), _pt(x, i2)
            if not _dot(_nrm(P0, P1, P2), _nrm(p, P1, P2)) > 0:
                return None
    return (_bits(l2) << 32) | e


def collapse_round_restated(verts, faces, vm, lo2, hi2):
    """One collapse round: (verts', faces', vert_mesh', winners)."""
    x, f, vm = np.array(verts, dtype=np.float32), np.asarray(faces, dtype=np.int64), np.asarray(vm, dtype=np.int32)
    V = x.shape[0]
    T = tables(f, V)
    E = T["lo"].shape[0]
    with np.errstate(all="ignore"):
        short = [e for e in range(E) if T["mult"][e] == 2]
        prio = {e: p for e in short for p in [_collapse_ok(x, f, T, vm, lo2, hi2, e)] if p is not None}
    word = [ONES64] * V
    rings = {e: set(_row(T, int(T["lo"][e])) + _row(T, int(T["hi"][e]))) for e in prio}
    for e, p in prio.items():
        for v in rings[e]:
            word[v] = min(word[v], p)
    winners = [e for e, p in prio.items() if all(word[v] == p for v in rings[e])]
    if not winners:
        return x, f.copy(), vm.copy(), 0
    remap = np.arange(V)
    new = x.copy()
    for e in winners:
        a, b = int(T["lo"][e]), int(T["hi"][e])
        new[a] = _mid(_pt(x, a), _pt(x, b))
        remap[b] = a
    f2 = remap[f]
    f2 = f2[~repeated(f2) | repeated(f)]
    keep = remap == np.arange(V)
    newid = np.cumsum(keep) - 1
    return new[keep], newid[f2], vm[keep], len(winners)


# ---- flip ------------------------------------------------------------------------------------------------------------------------
def _dev(val, flag):
    return abs(val - (4 if flag & 1 else 6))


def _worst(tris):
    """The largest signed cos^2 = d |d| / ((u . u)(w . w)) over the corners of `tris`, in order, as the fraction (num, den)."""
    best = None
    for p in tris:
        for k in range(3):
            u, w = _sub(p[(k + 1) % 3], p[k]), _sub(p[(k + 2) % 3], p[k])
            d = _dot(u, w)
            num, den = d * abs(d), _dot(u, u) * _dot(w, w)
            if best is None or num * best[1] > best[0] * den:
                best = (num, den)
    return best


def _flip_ok(x, f, T, cos2, e):
    a, b = int(T["lo"][e]), int(T["hi"][e])
    vflag, ptr = T["vflag"], T["ptr"]
    if T["mult"][e] != 2 or vflag[a] != 0 or vflag[b] != 0:
        return None
    one = [(t, i2) for t, i0, i1, i2 in _corners(T, f, a) if i1 == b]
    two = [(t, i1) for t, i0, i1, i2 in _corners(T, f, a) if i1 != b and i2 == b]
    if len(one) != 1 or len(two) != 1:
        return None
    (f1, c), (f2, d) = one[0], two[0]
    if c == d or c in (a, b) or d in (a, b):
        return None
    val = {v: int(ptr[v + 1] - ptr[v]) for v in (a, b, c, d)}
    if val[a] <= 3 or val[b] <= 3 or (min(c, d), max(c, d)) in T["index"]:
        return None
    gain = sum(_dev(val[v], vflag[v]) for v in (a, b, c, d)) - sum(_dev(val[v] + s, vflag[v]) for v, s in ((a, -1), (b, -1), (c, 1), (d, 1)))
    if gain <= 0 or gain > 15:
        return None
    A, B, C, D = _pt(x, a), _pt(x, b), _pt(x, c), _pt(x, d)
    na, nb = _nrm(A, B, C), _nrm(B, A, D)
    q = _dot(na, nb)
    if not q > 0 or not q * q >= (cos2 * _dot(na, na)) * _dot(nb, nb):
        return None
    s = _add(na, nb)
    if not _dot(_nrm(A, D, C), s) > 0 or not _dot(_nrm(D, B, C), s) > 0:
        return None
    old, new = _worst([(A, B, C), (B, A, D)]), _worst([(A, D, C), (D, B, C)])
    if new[0] * old[1] > old[0] * new[1]:                                       # the flip would lower the smallest of the six angles
        return None
    return ((16 - gain) << 32) | e, (f1, f2, c, d)


def cos2_of(flip_angle):
    return np.float32(math.cos(math.radians(float(flip_angle))) ** 2)


def flip_round_restated(verts, faces, cos2):
    """One flip round: (faces', winners)."""
    x, f = np.asarray(verts, dtype=np.float32), np.array(faces, dtype=np.int64)
    V = x.shape[0]
    T = tables(f, V)
    with np.errstate(all="ignore"):
        got = {e: r for e in range(T["lo"].shape[0]) for r in [_flip_ok(x, f, T, F32(cos2), e)] if r is not None}
    word = [ONES64] * V
    own = {e: (int(T["lo"][e]), int(T["hi"][e]), r[1][2], r[1][3]) for e, r in got.items()}
    for e, (p, _) in got.items():
        for v in own[e]:
            word[v] = min(word[v], p)
    winners = [e for e, (p, _) in got.items() if all(word[v] == p for v in own[e])]
    out = f.copy()
    for e in winners:
        a, b, c, d = own[e]
        f1, f2 = got[e][1][:2]
        out[f1] = (a, d, c)
        out[f2] = (d, b, c)
    return out, len(winners)


# ---- relax -----------------------------------------------------------------------------------------------------------------------
def relax_restated(verts, faces, lam=0.5, dtype=np.float32):
    """The relax pass in `dtype` (float32: the contract's arithmetic; float64: the reference of the bar)."""
    x = np.asarray(verts, dtype=np.float32).astype(dtype)
    f = np.asarray(faces, dtype=np.int64)
    ty = x.dtype.type
    V = x.shape[0]
    T = tables(f, V)
    out = x.copy()
    lam, tiny = ty(lam), ty(np.float32(1e-20))
    with np.errstate(all="ignore"):
        for v in range(V):
            row = _row(T, v)
            if T["vflag"][v] != 0 or not row:
                continue
            s, lost = [ty(0)] * 3, [ty(0)] * 3
            for u in row:
                for c in range(3):
                    y = x[u, c] - lost[c]
                    t = s[c] + y
                    lost[c] = (t - s[c]) - y
                    s[c] = t
            fn = ty(len(row))
            d = tuple(s[c] / fn - x[v, c] for c in range(3))
            g = (ty(0), ty(0), ty(0))
            for t, _, _, _ in _corners(T, f, v):
                g = _add(g, _nrm(_pt(x, f[t, 0]), _pt(x, f[t, 1]), _pt(x, f[t, 2])))
            ln = np.sqrt(max(_dot(g, g), tiny))
            nn = (g[0] / ln, g[1] / ln, g[2] / ln)
            t = _dot(nn, d)
            for c in range(3):
                out[v, c] = x[v, c] + lam * (d[c] - nn[c] * t)
    return out


# ---- the whole pipeline ----------------------------------------------------------------------------------------------------------
def remesh_restated(verts, faces, *, iters=3, target_len=None, target_scale=1.0, relax=0.5, flip_angle=30.0, vert_mesh=None):
    """`postprocess.remesh` by the contract: (verts', faces', vert_mesh', info)."""
    x, f = np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int64)
    vm = np.zeros(x.shape[0], np.int32) if vert_mesh is None else np.asarray(vert_mesh, dtype=np.int32)
    M = int(vm.max()) + 1 if vm.size else 1
    base = default_target(x, f, vm, M) if target_len is None else np.broadcast_to(np.asarray(target_len, dtype=np.float32), (M,))
    target = (base.astype(np.float64) * float(target_scale)).astype(np.float32)
    lo2, hi2 = bands(target)
    cos2 = cos2_of(flip_angle)
    info = []
    for _ in range(int(iters)):
        rec = dict(splits=0, collapses=0, flips=0, collapse_rounds=0, flip_rounds=0)
        x, f, vm, rec["splits"] = split_restated(x, f, vm, hi2)
        for _r in range(COLLAPSE_ROUNDS):
            x, f, vm, n = collapse_round_restated(x, f, vm, lo2, hi2)
            rec["collapse_rounds"] += 1
            rec["collapses"] += n
            if n == 0:
                break
        for _r in range(FLIP_ROUNDS):
            f, n = flip_round_restated(x, f, cos2)
            rec["flip_rounds"] += 1
            rec["flips"] += n
            if n == 0:
                break
        if relax != 0:
            x = relax_restated(x, f, relax, np.float32)
        info.append(rec)
    return x, f, vm, dict(target=target, iterations=info)


# ---- validity and quality --------------------------------------------------------------------------------------------------------
def problems(faces, V, closed=True):
    """A list of what keeps (faces, V) from being a valid orientable manifold (closed: without boundary): empty when valid."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = []
    if f.size and (f.min() < 0 or f.max() >= V):
        return ["index out of range"]
    if repeated(f).any():
        bad.append(f"{int(repeated(f).sum())} degenerate faces")
    lo, hi, mult, _, _ = mc.edges_restated(f, V)
    if closed and (mult != 2).any():
        bad.append(f"{int((mult != 2).sum())} edges of mult != 2")
    if not closed and (mult > 2).any():
        bad.append(f"{int((mult > 2).sum())} edges of mult > 2")
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if np.unique(d[:, 0] * V + d[:, 1]).shape[0] != d.shape[0]:
        bad.append("duplicate directed edge")
    if np.bincount(f.reshape(-1), minlength=V).min(initial=1) == 0:
        bad.append("unreferenced vertex")
    nxt = [dict() for _ in range(V)]
    for t in f[~repeated(f)]:
        for k in range(3):
            nxt[t[k]][int(t[(k + 1) % 3])] = int(t[(k + 2) % 3])           # a duplicate directed edge is reported above
    for v in range(V):
        link = nxt[v]
        if not link:
            continue
        starts = [u for u in link if u not in link.values()]
        if len(starts) > 1 or (closed and starts):
            bad.append(f"vertex {v}: fan of {len(starts)} open pieces")
            continue
        u, seen = (starts[0] if starts else next(iter(link))), set()
        while u in link and u not in seen:
            seen.add(u)
            u = link[u]
        if len(seen) != len(link):
            bad.append(f"vertex {v}: fan is not a single cycle or path")
    return bad


def euler(faces, vm, M):
    """chi = V - E + F per mesh over the referenced vertices."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vm = np.asarray(vm, dtype=np.int64)
    lo, _, _, _, _ = mc.edges_restated(f, vm.shape[0])
    used = np.zeros(vm.shape[0], bool)
    used[f.reshape(-1)] = True
    return (np.bincount(vm[used], minlength=M) - np.bincount(vm[lo], minlength=M) + np.bincount(vm[f[:, 0]], minlength=M)).tolist()


def quality(verts, faces, target):
    """(share of edges with 4/5 L <= length <= 4/3 L, minimum angle in degrees) in float64; target: one length."""
    x, f = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    lo, hi, _, _, _ = mc.edges_restated(f, x.shape[0])
    ln = np.linalg.norm(x[hi] - x[lo], axis=1)
    share = float(((ln >= 0.8 * target) & (ln <= 4.0 / 3.0 * target)).mean())
    ang = []
    for k in range(3):
        u, w = x[f[:, (k + 1) % 3]] - x[f[:, k]], x[f[:, (k + 2) % 3]] - x[f[:, k]]
        ang.append(np.arctan2(np.linalg.norm(np.cross(u, w), axis=1), (u * w).sum(1)))
    return share, float(np.degrees(np.min(ang)))


def boundary_vertices(faces, V):
    lo, hi, mult, _, _ = mc.edges_restated(faces, V)
    return np.unique(np.concatenate([lo[mult == 1], hi[mult == 1]]))


# ---- shared, computed once ---------------------------------------------------------------------------------------------------------
def case_bands(name, scale=1.0):
    """(target, lo2, hi2) float32 [M] of a case at its default target times `scale`."""
    v, f = mesh(name)
    vm = vert_mesh(name).numpy()
    base = default_target(v.numpy(), f.numpy(), vm, int(vm.max()) + 1)
    target = (base.astype(np.float64) * float(scale)).astype(np.float32)
    return (target,) + bands(target)


@functools.lru_cache(maxsize=None)
def pass_states(name):
    """The restatement's chain input -> split -> one collapse round -> one flip round of a case, each (verts, faces, vert_mesh,
    count): the state every pass of the exactness test starts from, and what it must return."""
    v, f = mesh(name)
    _, lo2, hi2 = case_bands(name)
    s0 = (v.numpy(), f.numpy(), vert_mesh(name).numpy(), 0)
    s1 = split_restated(s0[0], s0[1], s0[2], hi2)
    s2 = collapse_round_restated(s1[0], s1[1], s1[2], lo2, hi2)
    f3, n3 = flip_round_restated(s2[0], s2[1], cos2_of(30.0))
    return s0, s1, s2, (s2[0], f3, s2[2], n3)


@functools.lru_cache(maxsize=None)
def pipeline_restated(name, scale=1.0, relax=0.0, iters=PIPELINE_ITERS):
    v, f = mesh(name)
    return remesh_restated(v.numpy(), f.numpy(), iters=iters, target_scale=scale, relax=relax, vert_mesh=vert_mesh(name).numpy())


def flip_patch():
    """A flat 6 x 6 grid of vertices, every cell cut along the same diagonal (inner valence six), except the middle cell, cut the
    other way: its diagonal joins two vertices of valence seven and faces two of valence five.  (verts, faces, the grid's own faces)."""
    n = 6
    k = np.arange(n, dtype=np.float32)
    v = np.stack([np.repeat(k, n), np.tile(k, n), np.zeros(n * n, np.float32)], 1)          # vertex (i, j) = i * n + j at (i, j, 0)
    idx = lambda i, j: i * n + j
    even, odd = [], []
    for i in range(n - 1):
        for j in range(n - 1):
            p00, p10, p01, p11 = idx(i, j), idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)
            even += [(p00, p10, p11), (p00, p11, p01)]
            odd += [(p00, p10, p01), (p10, p11, p01)] if (i, j) == (2, 2) else [(p00, p10, p11), (p00, p11, p01)]
    return v, np.array(odd, dtype=np.int64), np.array(even, dtype=np.int64)
