"""Synthetic tet grids for the kernels that walk one (csrc/dmtet.hip, csrc/dmtet_bwd.hip, the vertex kernels of csrc/fixedtopo.hip)
and the host tables of meshdiffusion_amd/dmtet.py, so that they are tested at their chunk and block edges, on the second pass of
the chunk scan, on long and empty incidence rows and on tet lists in an order the host has never seen -- none of which the
shipped 64 grid reaches.  torch and numpy only; tests/test_cpu_tetgrid_cases.py proves what each case claims to own and
tests/test_gpu_tetgrid.py runs them on the GPU.

Also here: a numpy emulation of the KERNEL's formulation of marching tetrahedra (static sorted edge table, per-chunk totals of
1024, a scan in passes of 1024 with a carry, vertex ids by exclusive prefix, one-triangle faces before two-triangle faces) with
the one-line mistakes such a kernel makes, to be held against oracle/dmtet_oracle.py, which follows the reference's run-time
sort-and-unique algorithm.
"""
import functools
import itertools
import types

import numpy as np
import torch

CHUNK = 1024                       # MT_THREADS of csrc/dmtet.hip: edges or tets per workgroup, and chunk totals per scan pass
BLOCK = 256                        # MTB_THREADS / FT_THREADS: grid vertices per workgroup of the gather kernels
SECOND_PASS = CHUNK * CHUNK        # the first edge / tet id whose chunk offset comes from the second pass of the scan
BASE_TET_EDGES = (0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3)
# c_tri_table / c_num_tri of csrc/dmtet.hip
TRI_TABLE = np.array([
    [-1, -1, -1, -1, -1, -1], [1, 0, 2, -1, -1, -1], [4, 0, 3, -1, -1, -1], [1, 4, 2, 1, 3, 4],
    [3, 1, 5, -1, -1, -1], [2, 3, 0, 2, 5, 3], [1, 4, 0, 1, 5, 4], [4, 2, 5, -1, -1, -1],
    [4, 5, 2, -1, -1, -1], [4, 1, 0, 4, 5, 1], [3, 2, 0, 3, 5, 2], [1, 3, 5, -1, -1, -1],
    [4, 1, 2, 4, 3, 1], [3, 0, 4, -1, -1, -1], [2, 0, 1, -1, -1, -1], [-1, -1, -1, -1, -1, -1]], dtype=np.int64)
NUM_TRI = np.array([0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0], dtype=np.int64)

FLT_MAX = float(np.finfo(np.float32).max)
SUBNORMAL = float(np.float32(2.0 ** -149))          # the smallest positive subnormal


# ---------------------------------------------------------------------------------------------------------------
# grid builders
# ---------------------------------------------------------------------------------------------------------------
_AXIS_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
_ODD = (False, True, True, False, False, True)


def kuhn(nx, ny, nz):
    """The six-tet (Freudenthal) split of every cell of an integer lattice: vertices float32 [(nx+1)(ny+1)(nz+1), 3] at integer
    coordinates with id (i (ny+1) + j)(nz+1) + k, tets int32 [6 nx ny nz, 4], cell-major.  A tet walks from a cell's corner
    (i, j, k) to (i+1, j+1, k+1) along one of the six orders of the axes; the last two corners of the odd orders are swapped so
    that all tets have the same orientation.  Any subset or reordering of the tets is a valid grid for the kernels."""
    i, j, k = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), np.arange(nz + 1), indexing="ij")
    verts = np.stack([i, j, k], -1).reshape(-1, 3).astype(np.float32)
    cell = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")).reshape(3, -1).astype(np.int64)
    vid = lambda c: (c[0] * (ny + 1) + c[1]) * (nz + 1) + c[2]
    tets = np.empty((cell.shape[1], 6, 4), dtype=np.int64)
    for p, order in enumerate(_AXIS_ORDERS):
        c = cell.copy()
        ids = [vid(c)]
        for ax in order:
            c[ax] += 1
            ids.append(vid(c))
        if _ODD[p]:
            ids[2], ids[3] = ids[3], ids[2]
        tets[:, p] = np.stack(ids, -1)
    return verts, tets.reshape(-1, 4).astype(np.int32)


def truncated(grid, seed, T):
    """The first T tets of a seeded permutation of the grid's tets."""
    verts, tets = grid
    return verts, tets[np.random.default_rng(seed).permutation(tets.shape[0])[:T]]


EVEN_PERMS = np.array([p for p in itertools.permutations(range(4))
                       if sum(p[a] > p[b] for a in range(4) for b in range(a + 1, 4)) % 2 == 0], dtype=np.int64)     # A4: 12


def rotated(tets, seed):
    """An even permutation of the four indices of every tet, seeded per tet: every sign case meets every corner order, and the
    orientation of every tet is kept."""
    pick = np.random.default_rng(seed).integers(0, len(EVEN_PERMS), tets.shape[0])
    return np.take_along_axis(tets, EVEN_PERMS[pick], axis=1)


def with_unnamed(verts, k):
    """k more vertices that no tet names, behind the grid's."""
    extra = np.stack([-2.0 - np.arange(k), np.full(k, -2.0), np.full(k, -2.0)], -1).astype(np.float32)
    return np.concatenate([verts, extra], 0)


def star(n):
    """n tets (0, t+1, t+2, t+3) that all name vertex 0: vertex 0 has n + 2 incident edges.  The other named vertices wind
    around it on a spiral; the last vertex, n + 3, is named by no tet."""
    i = np.arange(1, n + 3, dtype=np.float64)
    ring = np.stack([(2 + 0.001 * i) * np.cos(0.37 * i), (2 + 0.001 * i) * np.sin(0.37 * i), 0.002 * i - 3], -1)
    verts = np.concatenate([np.zeros((1, 3)), ring, [[-5.0, -5.0, -5.0]]], 0).astype(np.float32)
    t = np.arange(n)
    return verts, np.stack([np.zeros(n, np.int64), t + 1, t + 2, t + 3], -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
SMALL_CASES = ("one-tet", "T1023", "T1024", "T1025", "E1023", "E1024", "E1025", "N255", "N256", "N257", "star")
CASES = SMALL_CASES + ("two-pass",)
STAR_N = 3000
# (seed, T) of truncated(kuhn(6, 6, 6)) with exactly E unique edges, found by edge_count_search below on the CPU
E_CASES = {1023: (1, 242), 1024: (3, 244), 1025: (0, 238)}
T_SEED = 5                        # the permutation of the T-cases
TWO_PASS_R = 56
# the seed of each small case's randn SDF (0 where not listed): the first one from 0 at which the last edge of the table is a
# crossing edge and the last tet is cut, so that the item next to a chunk edge does something a test can see (chosen with
# the sign tests alone on the CPU, asserted by tests/test_cpu_tetgrid_cases.py)
SDF_SEED = {"T1024": 1, "E1023": 1, "E1024": 3, "star": 1}


def edge_count_search(target, seeds=range(8)):
    """(seed, T) pairs for which truncated(kuhn(6, 6, 6), seed, T) has exactly `target` unique edges."""
    grid = kuhn(6, 6, 6)
    hits = []
    for seed in seeds:
        tets = truncated(grid, seed, grid[1].shape[0])[1]
        first = np.unique(_edge_keys(tets, grid[0].shape[0]), return_index=True)[1] // 6     # the tet that brings each edge
        count = np.cumsum(np.bincount(first, minlength=tets.shape[0]))                       # E of the first T + 1 tets
        hits += [(seed, int(T) + 1) for T in np.nonzero(count == target)[0]]
    return hits


def _grid_of(name):
    """(lattice vertices float32 [N,3], tets int32 [T,4], number of trailing unnamed vertices appended)."""
    if name == "one-tet":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.array([[0, 1, 2, 3]], np.int32), 0
    if name[0] == "T":
        v, t = truncated(kuhn(6, 6, 6), T_SEED, int(name[1:]))
        return v, rotated(t, 11), 0
    if name[0] == "E":
        v, t = truncated(kuhn(6, 6, 6), *E_CASES[int(name[1:])])
        return v, rotated(t, 12), 0
    if name[0] == "N":
        v, t = kuhn(5, 5, 6)                                                          # 6 * 6 * 7 = 252 vertices
        k = int(name[1:]) - v.shape[0]
        return with_unnamed(v, k), rotated(t, 13), k
    if name == "star":
        v, t = star(STAR_N)
        return v, t, 1
    if name == "two-pass":
        v, t = kuhn(TWO_PASS_R, TWO_PASS_R, TWO_PASS_R)
        return v, rotated(t, 14), 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """name, lattice float32 [N,3] (numpy), pos float32 [N,3] (torch: the lattice plus seeded jitter of +-0.3), tets int32 [T,4]
    (numpy), N, T, appended (how many vertices were added behind the grid's), unnamed (ids of the vertices that no tet names:
    the appended ones, and the lattice vertices that a truncated tet list leaves out)."""
    lattice, tets, k = _grid_of(name)
    N = lattice.shape[0]
    g = torch.Generator().manual_seed(1000 + CASES.index(name))
    pos = torch.from_numpy(lattice) + (torch.rand(N, 3, generator=g) * 2 - 1) * 0.3
    return types.SimpleNamespace(name=name, lattice=lattice, pos=pos.contiguous(), tets=np.ascontiguousarray(tets), N=N,
                                 T=tets.shape[0], appended=k, unnamed=np.setdiff1d(np.arange(N), tets.reshape(-1)))


def sdf_randn(c, seed=None):
    """The case's ordinary SDF: a seeded randn on the small cases, and on `two-pass` a noisy surface z = 27.6 + 0.7 sin(1.3 x)
    that cuts the last tets and the last edges of the lattice (27.6 - z + 0.7 sin(1.3 x) + 1.5 randn)."""
    seed = SDF_SEED.get(c.name, 0) if seed is None else seed
    r = torch.randn(c.N, generator=torch.Generator().manual_seed(2000 + 97 * CASES.index(c.name) + seed))
    if c.name != "two-pass":
        return r
    x, z = torch.from_numpy(c.lattice[:, 0]), torch.from_numpy(c.lattice[:, 2])
    return (27.6 - z + 0.7 * torch.sin(1.3 * x) + 1.5 * r).contiguous()


def sign_patterns():
    """The 16 sign cases of one tet as 16 SDFs [16,4]: bit k of the row number set <=> vertex k is inside (> 0)."""
    mag = torch.tensor([0.3, 1.1, 0.7, 2.5])
    bits = (torch.arange(16)[:, None] >> torch.arange(4)[None]) & 1
    return (mag[None] * (bits * 2 - 1)).float().contiguous()


# kind -> (value at the edge's first endpoint, value at its second; None: the vertex's own |randn| with this sign)
SPECIAL_KINDS = {
    "+0": (0.0, +1), "-0": (-0.0, +1), "+sub": (SUBNORMAL, -1), "-sub": (-SUBNORMAL, +1), "sub-pair": (SUBNORMAL, -SUBNORMAL),
    "flt-max": (FLT_MAX, -FLT_MAX), "tiny-huge": (1e-30, -1e30)}
ZERO_KINDS = ("+0", "-0")


def special_field(c, kinds, seed=0, copies=1):
    """(sdf float32 [N], placed): the case's randn SDF with every kind of `kinds` written `copies` times onto the two endpoints of
    seeded edges that share no vertex, next to the ordinary values of all other vertices.  placed: [(kind, a, b)].  An int in
    SPECIAL_KINDS stands for the vertex's own |randn| with that sign, so that every special value lies on a crossing edge."""
    sdf = sdf_randn(c).clone()
    edges = edge_table(c.tets, c.N)[0]
    order = np.random.default_rng(300 + seed).permutation(edges.shape[0])
    used, placed, todo = set(), [], [k for k in kinds for _ in range(copies)]
    for e in order:
        if not todo:
            break
        a, b = int(edges[e, 0]), int(edges[e, 1])
        if a in used or b in used:
            continue
        if len(placed) % 2:                                     # special values on first and on second endpoints
            a, b = b, a
        kind = todo.pop(0)
        va, vb = SPECIAL_KINDS[kind]
        sdf[a] = va
        sdf[b] = vb * (abs(float(sdf[b])) + 1e-3) if isinstance(vb, int) else vb
        used.update((a, b))
        placed.append((kind, a, b))
    assert not todo, f"{c.name}: no room for {todo}"
    return sdf.contiguous(), placed


def forward_fields(c):
    """Ordered {field name: sdf float32 [N]} the forward is tested on.  Small cases: `randn` and the special values (all on one
    field where the grid has room for them, one field per kind on the one-tet grid, which has two disjoint edges); one-tet also
    the 16 sign patterns; `two-pass`: its surface."""
    if c.name == "two-pass":
        return {"surface": sdf_randn(c)}
    out = {}
    if c.name == "one-tet":
        out.update({f"sign{p}": s for p, s in enumerate(sign_patterns())})
    out["randn"] = sdf_randn(c)
    if c.name == "one-tet":
        out.update({f"special:{k}": special_field(c, (k,))[0] for k in SPECIAL_KINDS})
    else:
        out["special"] = special_field(c, tuple(SPECIAL_KINDS))[0]
    return out


def special_placements(c):
    """{field name: placed} of the special fields of forward_fields(c)."""
    if c.name == "two-pass":
        return {}
    if c.name == "one-tet":
        return {f"special:{k}": special_field(c, (k,))[1] for k in SPECIAL_KINDS}
    return {"special": special_field(c, tuple(SPECIAL_KINDS))[1]}


def zeros_field(c):
    """The +-0.0 field of the regulariser: four +0.0 and four -0.0 (one each on the one-tet grid) among the randn values."""
    return special_field(c, ZERO_KINDS, seed=1, copies=1 if c.name == "one-tet" else 4)


GRID_MESHER_KINDS = ("lattice", "unit-cube")


def grid_mesher_inputs(kind, M=3, R=7, seed=5):
    """(tet vertices float32 [343,3], tets, grids float32 [M,4,R,R,R]) of the GridMesher test at R = 7: kuhn(6, 6, 6) at its
    integer coordinates (`lattice`) or scaled into the unit cube (`unit-cube`, the shipped grid's range), channel 0 a signed field,
    channels 1-3 0.7 randn, so that part of the deformation is clipped."""
    v, t = kuhn(6, 6, 6)
    if kind == "unit-cube":
        v = (v / np.float32(6) - np.float32(0.5)).astype(np.float32)
    g = torch.Generator().manual_seed(seed)
    ax = torch.linspace(-1, 1, R)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    grids = torch.empty(M, 4, R, R, R)
    for m in range(M):
        grids[m, 0] = 0.6 + 0.1 * m - (X ** 2 + Y ** 2 + Z ** 2).sqrt() + 0.2 * torch.sin(3 * X + m)
        grids[m, 1:] = torch.randn(3, R, R, R, generator=g) * 0.7
    return v, rotated(t, 15), grids


# ---------------------------------------------------------------------------------------------------------------
# plain numpy restatements of the host's outputs
# ---------------------------------------------------------------------------------------------------------------
def _edge_keys(tets, N):
    e = np.asarray(tets, np.int64)[:, list(BASE_TET_EDGES)].reshape(-1, 2)
    return e.min(1) * N + e.max(1)


def edge_table(tets, N):
    """(edges int64 [E,2] sorted lexicographically, tet_edges int64 [T,6]) of ALL tets: the static tables of the kernel."""
    keys, inv = np.unique(_edge_keys(tets, N), return_inverse=True)
    return np.stack([keys // N, keys % N], -1), inv.reshape(-1, 6)


def tet_sign_cases(sdf, tets):
    """The sign case 0..15 of every tet (bit k: vertex k has sdf > 0)."""
    occ = np.asarray(sdf, np.float32) > 0
    return (occ[np.asarray(tets, np.int64)] * (1 << np.arange(4))[None]).sum(-1)


def uv_idx_of(face_tet, n1, num_tets):
    """The reference's map_uv (nvdiffrec/lib/geometry/dmtet.py:70-99) on the face ids of :149-152, in numpy: face_gidx = 2 tet
    for a one-triangle tet and (2 tet, 2 tet + 1) for the two triangles of a two-triangle tet."""
    ft = np.asarray(face_tet, np.int64)
    gidx = 2 * ft
    gidx[n1:] += np.arange(ft.shape[0] - n1) % 2
    Nn = int(np.ceil(np.sqrt((num_tets * 2 + 1) // 2)))
    t = gidx // 2
    tet_idx = (t // Nn) * Nn + t % Nn
    tri = gidx % 2
    return np.stack([tet_idx * 4, tet_idx * 4 + tri + 1, tet_idx * 4 + tri + 2], -1).reshape(-1, 3)


def valid_vert_idx_of(face_tet, tets):
    """dmtet.py:161: the sorted unique vertices of the tets that emit a face."""
    return np.unique(np.asarray(tets, np.int64)[np.unique(np.asarray(face_tet, np.int64))])


def incidence_brute_force(edges, N):
    """(inc_ptr [N+1], inc [2E]) of `build_incidence` by a loop over the edges in ascending id."""
    rows = [[] for _ in range(N)]
    for e, (a, b) in enumerate(np.asarray(edges).tolist()):
        rows[a].append(2 * e)
        rows[b].append(2 * e + 1)
    ptr = np.zeros(N + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([x for r in rows for x in r], np.int64)


# ---------------------------------------------------------------------------------------------------------------
# the kernel's formulation, emulated
# ---------------------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_carry", "ge_zero", "two_tri_stride", "tet_chunk_base")


def _chunk_totals(flag):
    n = -(-flag.shape[0] // CHUNK)
    pad = np.zeros(n * CHUNK, np.int64)
    pad[:flag.shape[0]] = flag
    return pad.reshape(n, CHUNK).sum(1)


def _scan_in_passes(totals, carry=True):
    """md_mt_scan_kernel: exclusive offsets of the chunk totals, 1024 of them per pass, `base` carried from pass to pass."""
    out, base = np.empty_like(totals), 0
    for i0 in range(0, totals.shape[0], CHUNK):
        seg = totals[i0:i0 + CHUNK]
        out[i0:i0 + CHUNK] = (base if carry else 0) + np.cumsum(seg) - seg
        base += int(seg.sum())
    return out, base


def _prefix_in_chunk(flag):
    """Exclusive prefix of a 0/1 flag inside its chunk of 1024."""
    f = flag.astype(np.int64)
    excl = np.cumsum(f) - f
    start = (np.arange(f.shape[0]) // CHUNK) * CHUNK
    return excl - excl[start]


@functools.lru_cache(maxsize=None)
def case_tables(name):
    """edge_table of a case, computed once."""
    c = case(name)
    return edge_table(c.tets, c.N)


def emulate_kernel(pos, sdf, tets, mut=None, tables=None):
    """md_marching_tets in numpy, launch by launch: (verts float32 [V,3], faces int64 [F,3], face_tet int64 [F], counts (V, F, n1,
    n2)).  mut: one of MUTATIONS --
      drop_carry       the scan's second pass starts from 0 again
      ge_zero          inside is sdf >= 0
      two_tri_stride   a two-triangle tet's first face is N1 + (b2 + p2), not N1 + 2 (b2 + p2)
      tet_chunk_base   face_tet gets the tet's number inside its chunk
    Rows that a mutated run never writes stay -1 (faces, face_tet) or 0 (verts).  tables: the grid's edge_table, if at hand."""
    assert mut is None or mut in MUTATIONS
    pos, sdf, tets = np.asarray(pos, np.float32), np.asarray(sdf, np.float32), np.asarray(tets, np.int64)
    carry = mut != "drop_carry"
    edges, tet_edges = tables if tables is not None else edge_table(tets, pos.shape[0])
    occ = (sdf >= 0) if mut == "ge_zero" else (sdf > 0)
    cross = occ[edges[:, 0]] != occ[edges[:, 1]]
    idx = (occ[tets] * (1 << np.arange(4))[None]).sum(-1)
    nt = NUM_TRI[idx]
    # launches 1 and 2
    voff, V = _scan_in_passes(_chunk_totals(cross), carry)
    off1, N1 = _scan_in_passes(_chunk_totals(nt == 1), carry)
    off2, N2 = _scan_in_passes(_chunk_totals(nt == 2), carry)
    # launch 3
    e = np.nonzero(cross)[0]
    vid = -np.ones(edges.shape[0], np.int64)
    vid[e] = voff[e // CHUNK] + _prefix_in_chunk(cross)[e]
    a, b = edges[e, 0], edges[e, 1]
    with np.errstate(all="ignore"):
        nsb = -sdf[b]
        den = sdf[a] + nsb
        w0, w1 = nsb / den, sdf[a] / den
        val = (pos[a] * w0[:, None]).astype(np.float32) + (pos[b] * w1[:, None]).astype(np.float32)
    verts = np.zeros((V, 3), np.float32)
    verts[vid[e]] = val
    # launch 4
    F = N1 + 2 * N2
    faces, face_tet = -np.ones((F, 3), np.int64), -np.ones(F, np.int64)
    ev = vid[tet_edges]                                                                       # [T,6]
    t1, t2 = np.nonzero(nt == 1)[0], np.nonzero(nt == 2)[0]
    f1 = off1[t1 // CHUNK] + _prefix_in_chunk(nt == 1)[t1]
    f2 = N1 + (1 if mut == "two_tri_stride" else 2) * (off2[t2 // CHUNK] + _prefix_in_chunk(nt == 2)[t2])
    tet_id = (lambda t: t % CHUNK) if mut == "tet_chunk_base" else (lambda t: t)
    for t, f0, n in ((t1, f1, 1), (t2, f2, 2)):
        for f in range(n):                                                                    # in tet order: a later write wins
            faces[f0 + f] = np.take_along_axis(ev[t], TRI_TABLE[idx[t]][:, 3 * f:3 * f + 3], axis=1)
            face_tet[f0 + f] = tet_id(t)
    return verts, faces, face_tet, (V, F, N1, N2)


def same_mesh(a, b):
    """Two (verts, faces, face_tet, ...) results agree: faces and face_tet equal, vertices bit-equal apart from a common NaN mask."""
    va, vb = np.asarray(a[0], np.float32), np.asarray(b[0], np.float32)
    if va.shape != vb.shape or not np.array_equal(a[1], b[1]) or not np.array_equal(a[2], b[2]):
        return False
    na, nb = np.isnan(va), np.isnan(vb)
    return bool(np.array_equal(na, nb) and np.array_equal(va.view(np.int32)[~na], vb.view(np.int32)[~nb]))
