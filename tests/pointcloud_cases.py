"""Case definitions and float64 restatements for the point-cloud kernels (csrc/pointcloud.hip): nearest neighbours, the
chamfer distance of kaolin's documentation, the reference's surface sampling (nvdiffrec/lib/geometry/utils.py:3-127) and the
renderer-free fitting loop of dmtet.py:441-459, so that a machine without the reference can evaluate its expressions on any
input.  tools/gen_golden_pointcloud.py asserts the sampling restatement against the UNMODIFIED reference before it writes
tests/golden/pointcloud.npz; tests/test_cpu_pointcloud_host.py re-checks that on the fixture and proves the input
conditions the GPU tests rely on.  Shared by the CPU tests, the GPU tests and tools/bench_pointcloud.py.

Every restatement runs on the device of its inputs (float64 on the GPU in the GPU tests, on the CPU on the build host).
"""
import math

import torch

NEAR_TIE = 2.0 ** -20                  # relative gap under which nearest / second nearest, or r_face * total / a CDF boundary, are "near"
NN_VALUE_BAR = 2.0 ** -20              # |d2_gpu - d2_64| <= 2^-20 d2_64: 5 * 2^-24 direct-form evaluation + 10 * 2^-24 for a neighbour
                                       # that is nearest in fp32 but not in float64, rounded up to 16 * 2^-24
FIT_STEPS = (0, 10, 20, 40)
FIT_ITERS = 41
FIT_SAMPLES = 20000
FIT_TARGET_POINTS = 20000
FIT_LR = 0.01
FIT_SDF_REGULARIZER = 0.2
FIT_RADIUS = 0.6
FIT_SEED = 9100


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def sphere_cloud(n, radius, centre, seed):
    """n float32 points on a sphere (normalised normal deviates, CPU generator)."""
    x = torch.randn(n, 3, generator=_gen(seed), dtype=torch.float64)
    x = x / x.norm(dim=1, keepdim=True) * radius + torch.tensor(centre, dtype=torch.float64)
    return x.to(torch.float32)


def _lattice():
    """Exact ties: p at the odd points (2i+1, 2j+1, 2k+1), q at the even points of a small integer lattice in a shuffled
    order.  Every p has eight q at squared distance 3; every coordinate, difference, square and sum is a small integer."""
    r = torch.arange(6)
    odd = torch.stack(torch.meshgrid(2 * r + 1, 2 * r + 1, 2 * r + 1, indexing="ij"), -1).reshape(-1, 3)
    r = torch.arange(7)
    even = torch.stack(torch.meshgrid(2 * r, 2 * r, 2 * r, indexing="ij"), -1).reshape(-1, 3)
    even = even[torch.randperm(even.shape[0], generator=_gen(5107))]
    return odd.to(torch.float32)[None], even.to(torch.float32)[None]


def _dups():
    """2000 random points followed by copies of the first 500: with skip_same_index the copies are at distance 0."""
    x = torch.rand(2000, 3, generator=_gen(5108))
    return torch.cat([x, x[:500]])[None]


# name -> (p [B,N,3], q [B,M,3] or None for q = p, skip_same_index, exact_ties)
NN_CASES = ("spheres", "unequal", "n1", "m1", "batch3", "lattice", "self", "dups")
EXACT_TIE_CASES = ("lattice", "dups")


def nn_case(name):
    if name == "spheres":                                   # the real size: 50 000 x 50 000
        return sphere_cloud(50000, 0.8, (0.0, 0.0, 0.0), 5101)[None], sphere_cloud(50000, 0.75, (0.03, -0.02, 0.01), 5102)[None], False
    if name == "unequal":                                   # N != M, multiples of no tile
        return sphere_cloud(1237, 0.5, (0.1, 0.0, 0.0), 5103)[None], torch.rand(1, 3001, 3, generator=_gen(5104)) - 0.5, False
    if name == "n1":
        return torch.rand(1, 1, 3, generator=_gen(5105)), torch.rand(1, 2777, 3, generator=_gen(5106)), False
    if name == "m1":
        return torch.rand(1, 513, 3, generator=_gen(5109)), torch.rand(1, 1, 3, generator=_gen(5110)), False
    if name == "batch3":
        return torch.randn(3, 700, 3, generator=_gen(5111)), torch.randn(3, 1900, 3, generator=_gen(5112)), False
    if name == "lattice":
        p, q = _lattice()
        return p, q, False
    if name == "self":
        p = torch.randn(1, 5000, 3, generator=_gen(5113))
        return p, None, True
    if name == "dups":
        return _dups(), None, True
    raise KeyError(name)


def nn_float64(p, q=None, skip_same_index=False, chunk=1024):
    """Brute force in float64, direct form: (d1 [B,N], i1 int64 [B,N], d2 [B,N]) = nearest squared distance, its LOWEST index,
    and the second-nearest squared distance (inf when there is none).  With skip_same_index candidate i is left out for
    query i."""
    p = p.to(torch.float64)
    q = p if q is None else q.to(torch.float64)
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    d1 = torch.empty(B, N, dtype=torch.float64, device=p.device)
    d2 = torch.empty_like(d1)
    i1 = torch.empty(B, N, dtype=torch.int64, device=p.device)
    ar = torch.arange(M, device=p.device)
    for b in range(B):
        for s in range(0, N, chunk):
            a = p[b, s:s + chunk]
            d = (a[:, None, 0] - q[b, None, :, 0]) ** 2
            d += (a[:, None, 1] - q[b, None, :, 1]) ** 2
            d += (a[:, None, 2] - q[b, None, :, 2]) ** 2
            if skip_same_index:
                rows = torch.arange(a.shape[0], device=p.device)
                keep = rows + s < M
                d[rows[keep], rows[keep] + s] = float("inf")
            m = d.min(dim=1).values
            first = torch.where(d == m[:, None], ar[None], M).min(dim=1).values
            d1[b, s:s + chunk], i1[b, s:s + chunk] = m, first
            if M > 1:
                d.scatter_(1, first[:, None], float("inf"))
                d2[b, s:s + chunk] = d.min(dim=1).values
            else:
                d2[b, s:s + chunk] = float("inf")
    return d1, i1, d2


def near_tie(d1, d2):
    """Queries whose nearest and second-nearest squared distances differ by less than 2^-20 relative: an fp32 evaluation may
    order them either way."""
    return (d2 - d1) < NEAR_TIE * d2


# ---- chamfer ----------------------------------------------------------------------------------------------------------------
CHAMFER_CASES = ("spheres4", "weighted")


def chamfer_case(name):
    """(p1 [B,N,3], p2 [B,M,3], w1, w2)"""
    if name == "spheres4":
        p = torch.stack([sphere_cloud(3000, 0.8, (0.0, 0.0, 0.0), 5201 + b) for b in range(4)])
        q = torch.stack([sphere_cloud(2500, 0.7 + 0.02 * b, (0.05, 0.0, -0.03), 5211 + b) for b in range(4)])
        return p, q, 1.0, 1.0
    if name == "weighted":
        return torch.randn(2, 1100, 3, generator=_gen(5221)), torch.randn(2, 1700, 3, generator=_gen(5222)) * 1.2, 0.7, 1.9
    raise KeyError(name)


def chamfer_restated(p1, p2, w1, w2, i12, i21, dtype=torch.float64, g=None):
    """mean_i |p1_i - p2_i12(i)|^2 w1 + mean_j |p2_j - p1_i21(j)|^2 w2 in `dtype` with the given (float64) neighbours, and its
    gradients under the cotangent g [B] (ones when None): (value [B], dp1, dp2)."""
    a = p1.detach().to(dtype).requires_grad_(True)
    b = p2.detach().to(dtype).requires_grad_(True)
    B = a.shape[0]
    bi = torch.arange(B, device=a.device)[:, None]
    d12 = ((a - b[bi, i12]) ** 2).sum(-1)
    d21 = ((b - a[bi, i21]) ** 2).sum(-1)
    val = d12.mean(dim=1) * w1 + d21.mean(dim=1) * w2
    g = torch.ones_like(val) if g is None else g.to(device=val.device, dtype=dtype)
    (val * g).sum().backward()
    return val.detach(), a.grad, b.grad


def chamfer_cotangent(B):
    return torch.linspace(0.5, 1.5, B)


# ---- meshes and sampling ----------------------------------------------------------------------------------------------------
def uv_sphere(n_lat, n_lon, radius=0.7, squash=(1.0, 0.6, 1.3)):
    """A closed UV ellipsoid: triangles shrink towards the poles (very unequal areas).  (verts float32 [V,3], faces int64 [F,3])"""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * math.pi * j / n_lon
            v.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    v.append((0.0, 0.0, -1.0))
    f = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon          # noqa: E731
    for j in range(n_lon):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    verts = torch.tensor(v, dtype=torch.float64) * radius * torch.tensor(squash, dtype=torch.float64)
    return verts.to(torch.float32), torch.tensor(f, dtype=torch.int64)


SAMPLE_CASES = ("ellipsoid", "batch2", "degenerate")
SAMPLE_SIZES = {"ellipsoid": 2048, "batch2": 768, "degenerate": 1024}
SAMPLE_SEEDS = {"ellipsoid": 5301, "batch2": 5302, "degenerate": 5303}


def sample_case(name):
    """(vertices float32 [B,V,3], faces int64 [F,3])"""
    if name == "ellipsoid":                                 # F = 352: 2 F 2^-20 of the samples fall near a CDF boundary, under 0.1 %
        v, f = uv_sphere(12, 16)
        return v[None], f
    if name == "batch2":                                    # two meshes over one face table
        v, f = uv_sphere(10, 12)
        v2 = v * torch.tensor([1.3, 0.8, 0.5]) + 0.05 * torch.randn(v.shape, generator=_gen(5304))
        return torch.stack([v, v2]), f
    if name == "degenerate":                                # zero-area faces between the others: never to be chosen
        v, f = uv_sphere(8, 10)
        zero = torch.stack([f[::3, 0], f[::3, 0], f[::3, 1]], dim=1)          # two corners coincide: area exactly 0
        rows = torch.cat([zero[:5], f[:40], zero[5:], f[40:], zero[:3]])
        return v[None], rows
    raise KeyError(name)


def unequal_mesh():
    """The mesh of the 10^6-sample count test: 14 faces whose areas span five orders of magnitude, one of them zero."""
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 2], [1, 0, 2], [1, 1, 2], [0, 1, 2],
                      [2, 0, 0], [2.01, 0, 0], [2, 0.01, 0], [3, 0, 0], [3.1, 0, 0], [3, 0.1, 0], [4, 0, 0]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 5, 1], [0, 4, 5], [1, 6, 2], [1, 5, 6], [2, 7, 3], [2, 6, 7],
                      [8, 9, 10], [11, 11, 14], [11, 12, 13], [3, 4, 0]], dtype=torch.int64)
    return v[None], f


def face_areas_restated(vertices, faces, dtype=torch.float64):
    """0.5 |(v1 - v0) x (v2 - v0)|: [B,F] in `dtype`."""
    v = vertices.to(dtype)
    v0, v1, v2 = v[:, faces[:, 0]], v[:, faces[:, 1]], v[:, faces[:, 2]]
    return 0.5 * torch.linalg.cross(v1 - v0, v2 - v0, dim=-1).norm(dim=-1)


def face_choices_restated(areas, r_face):
    """Inverse CDF in float64: the first face whose inclusive cumulative area exceeds r_face * total.  areas [B,F], r_face
    [B,S] -> (choices int64 [B,S], near bool [B,S]: r_face * total within 2^-20 * total of a CDF boundary)."""
    a = areas.to(torch.float64)
    cdf = torch.cumsum(a, dim=1)
    total = cdf[:, -1:]
    t = r_face.to(torch.float64) * total
    c = torch.searchsorted(cdf.contiguous(), t.contiguous(), right=True).clamp_max(a.shape[1] - 1)
    lo = torch.gather(cdf, 1, (c - 1).clamp_min(0))
    hi = torch.gather(cdf, 1, c)
    near = ((t - lo).abs() < NEAR_TIE * total) | ((hi - t).abs() < NEAR_TIE * total)
    return c, near


def sample_points_restated(vertices, faces, choices, r_u, r_v, dtype=torch.float64):
    """geometry/utils.py:34-45 in `dtype` for given faces and uniforms: (points [B,S,3], weights [B,S,3])."""
    v = vertices.to(dtype)
    B = v.shape[0]
    bi = torch.arange(B, device=v.device)[:, None]
    tri = faces.to(v.device)[choices]                                   # [B,S,3]
    u = torch.sqrt(r_u.to(dtype))[..., None]
    vv = r_v.to(dtype)[..., None]
    w0, w1, w2 = 1 - u, u * (1 - vv), u * vv
    pts = w0 * v[bi, tri[..., 0]] + w1 * v[bi, tri[..., 1]] + w2 * v[bi, tri[..., 2]]
    return pts, torch.cat([w0, w1, w2], dim=-1)


def sample_points_grad_restated(vertices, faces, choices, r_u, r_v, G, dtype=torch.float64):
    """d sum(points * G) / d vertices by autograd over sample_points_restated, in `dtype`."""
    v = vertices.detach().to(dtype).requires_grad_(True)
    pts, _ = sample_points_restated(v, faces, choices, r_u, r_v, dtype)
    (pts * G.to(device=v.device, dtype=dtype)).sum().backward()
    return v.grad


def case_G(shape, seed):
    return torch.randn(*shape, generator=_gen(seed))


def case_uniforms(B, S, seed):
    """(r_face, r_u, r_v), each float32 [B,S] in [0, 1), CPU generator."""
    return tuple(torch.rand(3, B, S, generator=_gen(seed)))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the fitting run ----------------------------------------------------------------------------------------------------------
def fit_target():
    """Target of the end-to-end fit: FIT_TARGET_POINTS points on a sphere of radius FIT_RADIUS."""
    return sphere_cloud(FIT_TARGET_POINTS, FIT_RADIUS, (0.0, 0.0, 0.0), FIT_SEED)


def fit_initial_sdf(verts_scaled):
    """The fit starts from a sphere of radius 0.45, as the fitting run of tests/dmtet_grad_cases.py does.  From the reference's
    random start (dmtet.py:224) every grid vertex belongs to a surface tet, so the regulariser is detached everywhere and this
    renderer-free loop does not halve its chamfer value in 41 iterations at any learning rate tried (float64 reference loop,
    lr 0.01 / 0.03 / 0.1 / 0.3: 0.205 -> 0.174 / 0.155 / 0.153 / 0.147): the start is the hyper-parameter that was changed."""
    return (0.45 - verts_scaled.norm(dim=1)).clamp(-1.0, 1.0)


def fit_uniforms(it):
    """The explicit uniforms of iteration `it`: (r_face, r_u, r_v), each float32 [1, FIT_SAMPLES]."""
    return case_uniforms(1, FIT_SAMPLES, FIT_SEED + 1 + it)
