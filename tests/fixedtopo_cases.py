"""Cases and torch restatements of the fixed-topology contract (the header comment of csrc/fixedtopo.hip): the vertex formula of
the plan, the umbrella Laplacian, the depth term of pass 2 and its learning-rate schedule.  Shared by tools/gen_golden_fixedtopo.py,
the CPU tests, the GPU tests and tools/bench_fixedtopo.py.  Everything runs in fp32 or float64 under torch autograd on the device
of its inputs.
"""
import functools

import torch

import interp_cases as ic
import raster_cases as rc

LAPLACE_MESHES = ("ptorus", "sphere", "quad", "fan40", "degen")      # 256-face torus, marching-tets sphere, open quad, 40-corner row, unreferenced vertex + zero-area face
SMALL_MESHES = LAPLACE_MESHES[2:]
BASES = ("nobase", "base")
X_SEED, NOISE = 9800, 0.02
GRAD_OUT = 1.75                         # the incoming gradient of the Laplacian's backward
HALF_ULP = 2.0 ** -24                   # a float32 scalar cannot be expected nearer to its float64 value than this, relatively
SDF_CASES = ("sphere", "deformed", "random_sign")
LOOP_RES, LOOP_ITERS, LOOP_LR, LOOP_STEPS = 64, 12, 0.01, (0, 5, 11)
SECOND_LAYER_WEIGHT, DEPTH_SCALE, PROXIMITY = 0.1, 100.0, 5e-3


# ---- the vertex formula -----------------------------------------------------------------------------------------------------------------
def sorted_edges(tets):
    """The lexicographically sorted unique edge table int64 [E,2] of tets int64 [T,4] (that of `TetTables`)."""
    be = torch.tensor((0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3), dtype=torch.int64, device=tets.device)
    e = tets[:, be].reshape(-1, 2)
    e = torch.stack([e.min(dim=1).values, e.max(dim=1).values], dim=-1)
    return torch.unique(e, dim=0)


def crossing_edges(sdf, edges):
    """The plan's `edge` [Vm,2]: the rows of the sorted table with exactly one endpoint above zero, in table order."""
    above = sdf > 0
    return edges[above[edges[:, 0]] != above[edges[:, 1]]]


def verts_restated(pos, sdf, edge, dtype=torch.float64):
    """verts [Vm,3] in `dtype`: pos[a] (-sb / den) + pos[b] (sa / den), den = sa - sb.  Differentiable w.r.t. pos."""
    p, s = pos.to(dtype), sdf.to(dtype)
    sa, sb = s[edge[:, 0]], s[edge[:, 1]]
    den = sa - sb
    return p[edge[:, 0]] * (-sb / den)[:, None] + p[edge[:, 1]] * (sa / den)[:, None]


def two_tet_grid():
    """(pos float64 [5,3], tets int64 [2,4]): two tets sharing the face (1, 2, 3)."""
    pos = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.1, 1.0, 0.2], [0.2, 0.1, 1.0], [1.1, 1.2, 0.9]], dtype=torch.float64)
    return pos, torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])


@functools.lru_cache(maxsize=None)
def sdf_case(name):
    """(sdf float32 [N], deform float32 [N,3]) on the shipped 64 grid x rc.MESH_SCALE, CPU: a sphere's sign, the same with a
    random deform in (-0.99, 0.99), and a +-1 field of random signs."""
    p = torch.as_tensor(rc.tet_grid()[0], dtype=torch.float32) * rc.MESH_SCALE
    gen = torch.Generator().manual_seed(X_SEED + 1)
    sphere = torch.sign(p.norm(dim=1) - 0.7 + 1e-8)
    if name == "sphere":
        return sphere, torch.zeros_like(p)
    if name == "deformed":
        return sphere, (torch.rand(p.shape, generator=gen) * 2 - 1) * 0.99
    if name == "random_sign":
        return torch.where(torch.rand(p.shape[0], generator=gen) < 0.5, -1.0, 1.0), torch.zeros_like(p)
    raise KeyError(name)


# ---- the umbrella Laplacian -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def laplace_case(name):
    """(x float32 [V,3], base float32 [V,3], faces int64 [F,3]) on the CPU: the mesh's vertices displaced by seeded noise, and
    the undisplaced vertices.  The three coincident vertices of `degen` stay coincident, so their face keeps its zero area."""
    verts, faces = ic.mesh(name)
    gen = torch.Generator().manual_seed(X_SEED + LAPLACE_MESHES.index(name))
    x = verts + NOISE * torch.randn(verts.shape, generator=gen)
    if name == "degen":
        x[6:] = x[5]
    return x, verts.clone(), faces


def laplace_restated(x, faces, base=None, dtype=torch.float64):
    """(mean(term^2), term [V,3]) in `dtype`: per corner (f, k) of v the contribution (y[f[(k+1)%3]] - y_v) + (y[f[(k+2)%3]] -
    y_v) of y = x - base, added by index_add in corner order, divided by max(2 corners, 1).  Differentiable w.r.t. x."""
    y = x.to(dtype) if base is None else x.to(dtype) - base.to(dtype)
    V = y.shape[0]
    c = y[faces]                                                                # [F,3,3]: corner k of face f
    contrib = (c[:, [1, 2, 0]] - c) + (c[:, [2, 0, 1]] - c)
    flat = faces.reshape(-1)
    term = torch.zeros(V, 3, dtype=dtype, device=y.device).index_add(0, flat, contrib.reshape(-1, 3))
    corners = torch.zeros(V, dtype=dtype, device=y.device).index_add(0, flat, torch.ones(flat.shape[0], dtype=dtype, device=y.device))
    term = term / torch.clamp(2 * corners, min=1.0)[:, None]
    return (term * term).mean(), term


def laplace_grads_restated(x, faces, base=None, dtype=torch.float64, grad_out=GRAD_OUT):
    """(value, d x [V,3]) of grad_out * laplace in `dtype`."""
    xx = x.detach().to(dtype).requires_grad_(True)
    loss, _ = laplace_restated(xx, faces, base, dtype)
    (loss * grad_out).backward()
    return loss.detach(), xx.grad


def laplace_reference(x, faces):
    """regularizer.py:41-60 as a user writes it in fp32 torch (scatter_add_): what the parent commit's path has to run."""
    term, norm = torch.zeros_like(x), torch.zeros_like(x[..., 0:1])
    v0, v1, v2 = x[faces[:, 0], :], x[faces[:, 1], :], x[faces[:, 2], :]
    term.scatter_add_(0, faces[:, 0:1].repeat(1, 3), (v1 - v0) + (v2 - v0))
    term.scatter_add_(0, faces[:, 1:2].repeat(1, 3), (v0 - v1) + (v2 - v1))
    term.scatter_add_(0, faces[:, 2:3].repeat(1, 3), (v0 - v2) + (v1 - v2))
    two = torch.ones_like(v0[..., 0:1]) * 2.0
    for k in range(3):
        norm.scatter_add_(0, faces[:, k:k + 1], two)
    term = term / torch.clamp(norm, min=1.0)
    return torch.mean(term ** 2)


def flat_patch(n=5):
    """A flat regular n x n patch, every cell cut along the same diagonal: (verts float64 [n n,3], faces [2 (n-1)^2,3], interior bool)."""
    i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    verts = torch.stack([j * 0.25, i * 0.25, torch.zeros_like(i) * 1.0], -1).reshape(-1, 3).double()
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    faces = torch.cat([torch.stack([a, a + 1, a + n + 1], 1), torch.stack([a, a + n + 1, a + n], 1)])
    interior = ((i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)).reshape(-1)
    return verts, faces, interior


# ---- the depth term and the schedule ------------------------------------------------------------------------------------------------------
def depth_loss_fixedtopo_restated(depth_second, t_depth, t_depth_second, mask):
    """dmtet_fixedtopo.py:326-337 as it evaluates: the second layer only.  All [B,H,W,1]; mask [B,H,W]."""
    valid = (t_depth_second >= 0).to(depth_second.dtype) * ((t_depth_second - t_depth).abs() >= PROXIMITY).to(depth_second.dtype)
    d = (depth_second - t_depth_second).abs() * mask[..., None].to(depth_second.dtype) * valid * SECOND_LAYER_WEIGHT
    return torch.where(d < 1.0, d, d * d).mean() * DEPTH_SCALE


def lr_schedule_restated(it, warmup_iter=100):
    """fit_dmtets.py:396-399."""
    return it / warmup_iter if it < warmup_iter else max(0.0, 10.0 ** (-0.0002 * (it - warmup_iter)))


def within(err, unit, bar=4.0):
    return err <= bar * unit if unit > 0 else err == 0.0


def ratio(err, unit):
    return err / unit if unit > 0 else float(err > 0)
