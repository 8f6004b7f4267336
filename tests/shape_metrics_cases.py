"""Case definitions and float64 restatements for the generation metrics (csrc/shape_metrics.hip, meshdiffusion_amd/metrics.py):
the all-pairs matrix of sided mean squared distances, the chamfer matrix, MMD / COV / 1-NNA.  No implementation of the metrics
was available where this was written: the restatements are the formulas of metrics.py's docstrings, written a second time in
float64 with plain loops.  Shared by tests/test_cpu_shape_metrics_host.py, tests/test_gpu_shape_metrics.py and tools/bench_shape_metrics.py.

Every restatement works on the fp32 inputs converted to float64, on the device of its inputs.

VALUE_BAR = 1.125 * 2^-20, relative, elementwise on the sided matrix.  Derivation: every per-point minimum is within
NN_VALUE_BAR = 2^-20 of its float64 value (tests/pointcloud_cases.py: 5 * 2^-24 for the direct-form evaluation plus 10 * 2^-24
for a neighbour that is nearest in fp32 but not in float64, rounded up to 16 * 2^-24); the minima are non-negative, so their
float64 sum and mean carry the same relative bound (the float64 additions add < 2^-40); one rounding to fp32 adds 2^-24;
(16 + 1) * 2^-24 rounded up to 18 * 2^-24.  No case is exempt.

ARGMIN_GAP = 2^-18.  An fp32 chamfer matrix whose sided halves are within VALUE_BAR of float64 is itself within VALUE_BAR + 2^-24
< 1.2 * 2^-20 (relative) of the float64 chamfer matrix; two entries a < b can change order only if b - a <= 1.2 * 2^-20 (a + b)
< 2^-18 b.  tests/test_cpu_shape_metrics_host.py proves that every row minimum COV and 1-NNA use in the metric cases is
separated from its runner-up by more than that, and the GPU test re-checks it on the clouds it actually sampled.
"""
import math

import torch

import pointcloud_cases as pc

VALUE_BAR = 1.125 * 2.0 ** -20
ARGMIN_GAP = 2.0 ** -18
CONSISTENCY_BAR = 2.0 ** -23           # chamfer_matrix against pointcloud.chamfer_distance: same fp32 minima, float64 sums in another order
METRIC_POINTS = 2048

# the last three make a workgroup walk a RUN of more than one y cloud (the run length is ceil(ny / min(ny, ceil(2048 / nx))):
# 1 for the nine before them)
FINITE_CASES = ("tiny", "ones", "edges", "typical", "near", "offset", "runs", "self", "lattice", "run3", "run2_blocks", "run_tail")
LATTICE_EXPECTED = [[3.0, 12.0], [180.0, 7.5], [15.0, 9.0]]


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _spheres(n, points, radius, seed):
    return torch.stack([pc.sphere_cloud(points, radius, (0.0, 0.0, 0.0), seed + k) for k in range(n)])


def _lattice():
    r = torch.arange(8)
    odd = torch.stack(torch.meshgrid(2 * r + 1, 2 * r + 1, 2 * r + 1, indexing="ij"), -1).reshape(-1, 3).to(torch.float32)
    even = torch.stack(torch.meshgrid(2 * r, 2 * r, 2 * r, indexing="ij"), -1).reshape(-1, 3).to(torch.float32)
    return torch.stack([odd, odd * 2, odd + 4]), torch.stack([even, even * 3])


def case(name):
    """(x float32 [Nx,P,3], y float32 [Ny,Q,3]) on the CPU; for "self" y IS x."""
    if name == "tiny":
        return torch.rand(3, 7, 3, generator=_gen(7101)), torch.rand(5, 11, 3, generator=_gen(7102))
    if name == "ones":
        return torch.rand(2, 1, 3, generator=_gen(7103)), torch.rand(2, 1, 3, generator=_gen(7104))
    if name == "edges":                                     # one past the 2048-point register block and the 1024-point tile
        return _spheres(2, 2049, 0.5, 7110), _spheres(3, 1025, 0.45, 7120)
    if name == "typical":
        return _spheres(6, 2048, 0.5, 7130), _spheres(7, 2048, 0.45, 7140)
    if name == "near":                                      # distances about 1e-8
        x = _spheres(3, 2048, 0.5, 7150)
        return x, x + 1e-4 * torch.randn(x.shape, generator=_gen(7153))
    if name == "offset":                                    # coordinates large against distances
        x = _spheres(3, 2048, 0.5, 7160) + 3.0
        return x, x + 1e-3 * torch.randn(x.shape, generator=_gen(7163))
    if name == "runs":                                      # one x cloud, many y clouds
        return torch.rand(1, 64, 3, generator=_gen(7170)), torch.rand(70, 64, 3, generator=_gen(7171))
    if name == "self":
        x = _spheres(9, 2048, 0.5, 7180)
        return x, x
    if name == "lattice":
        return _lattice()
    if name == "run3":                                      # run length 3, seven runs, the last one of two clouds
        return torch.rand(300, 33, 3, generator=_gen(7190)), torch.rand(20, 17, 3, generator=_gen(7191))
    if name == "run2_blocks":                               # run length 2 with two register blocks per x cloud
        return torch.rand(1100, 2049, 3, generator=_gen(7192)), torch.rand(3, 5, 3, generator=_gen(7193))
    if name == "run_tail":                                  # run length 5 with a tile of 1024 + 3 points: the tile is re-filled per cloud
        return torch.rand(256, 9, 3, generator=_gen(7194)), torch.rand(40, 1027, 3, generator=_gen(7195))
    raise KeyError(name)


def nonfinite_case():
    """`tiny` with a NaN coordinate in x[1], the point y[2][3] at +inf, and one more cloud on either side holding +inf in the same
    coordinate (inf - inf): (x [4,7,3], y [6,11,3], clean_x_rows, clean_y_rows) -- the rows that `tiny` has unchanged."""
    x, y = case("tiny")
    inf = float("inf")
    x = torch.cat([x, torch.rand(1, 7, 3, generator=_gen(7105))])
    y = torch.cat([y, torch.rand(1, 11, 3, generator=_gen(7106))])
    x[1, 4, 1] = float("nan")
    y[2, 3, :] = inf
    x[3, 2, 0] = inf
    y[5, 6, 0] = inf
    return x, y, (0, 2), (0, 1, 3, 4)


# a non-finite point in a y cloud of more than one LDS tile, outside its last tile: the minimum carried from tile to tile must keep it
NONFINITE_TILE_CASES = ("nan_first_tile", "nan_middle_tile", "nan_blocks")


def nonfinite_tile_case(name):
    """(x, y, clean y): x finite, y[0] with non-finite points, y[1] untouched; `clean y` is y before the points were set."""
    nan = float("nan")
    if name == "nan_first_tile":                            # the shape the feature exists for: 2048 points, two tiles, NaN in the first
        x, y = _spheres(2, 2048, 0.5, 7301), _spheres(2, 2048, 0.45, 7311)
        spots = [(100, 1, nan)]
    elif name == "nan_middle_tile":                         # three tiles: a finite one, the NaN in the second, a finite one after it
        x, y = torch.rand(2, 64, 3, generator=_gen(7321)), torch.rand(2, 3000, 3, generator=_gen(7322))
        spots = [(1500, 2, nan)]
    elif name == "nan_blocks":                              # three register blocks on the x side, two tiles on the y side
        x, y = torch.rand(2, 4100, 3, generator=_gen(7331)), torch.rand(2, 1500, 3, generator=_gen(7332))
        spots = [(5, 0, nan)]
    else:
        raise KeyError(name)
    clean = y.clone()
    for point, coord, value in spots:
        y[0, point, coord] = value
    return x, y, clean


# ---- float64 restatements -------------------------------------------------------------------------------------------------
def sided_mean_float64(x, y, budget=1 << 24):
    """out[i,j] = mean_a min_b |x[i,a] - y[j,b]|^2 in float64, direct form: [Nx,Ny] float64 on the device of x."""
    x, y = x.to(torch.float64), y.to(torch.float64)
    Nx, P, Ny, Q = x.shape[0], x.shape[1], y.shape[0], y.shape[1]
    out = torch.empty(Nx, Ny, dtype=torch.float64, device=x.device)
    step = max(1, budget // (P * Q))
    for i in range(Nx):
        for j in range(0, Ny, step):
            yy = y[j:j + step]
            d = (x[i, None, :, None, 0] - yy[:, None, :, 0]) ** 2
            d += (x[i, None, :, None, 1] - yy[:, None, :, 1]) ** 2
            d += (x[i, None, :, None, 2] - yy[:, None, :, 2]) ** 2
            out[i, j:j + step] = d.min(dim=2).values.mean(dim=1)
    return out


def sided_mean_fp32(x, y):
    """What torch gives for d2.min(dim=1).values.mean() on the direct-form fp32 distances, pair by pair: [Nx,Ny] float32.
    Small cases only (the NaN / inf expectations)."""
    out = torch.empty(x.shape[0], y.shape[0], dtype=torch.float32, device=x.device)
    for i in range(x.shape[0]):
        for j in range(y.shape[0]):
            dx, dy, dz = (x[i, :, None, k] - y[j, None, :, k] for k in range(3))
            out[i, j] = (dz * dz + (dy * dy + dx * dx)).min(dim=1).values.mean()
    return out


def chamfer_float64(x, y=None):
    if y is None:
        s = sided_mean_float64(x, x)
        return s + s.t()
    return sided_mean_float64(x, y) + sided_mean_float64(y, x).t()


def within_bar(out, out64, bar=VALUE_BAR):
    """(ok, worst |out - out64| / out64 over the positive entries)"""
    err = (out.to(torch.float64) - out64).abs()
    pos = out64 > 0
    worst = float((err[pos] / out64[pos]).max()) if bool(pos.any()) else 0.0
    return bool((err <= bar * out64).all()), worst


def _first_argmin(row):
    best, where = None, -1
    for k, v in enumerate(row):
        if best is None or v < best:
            best, where = v, k
    return where


def mmd_cov_restated(d_sr):
    """(mmd, cov) of d_sr [S,R] with plain loops over a float64 copy."""
    d = d_sr.to(torch.float64).cpu().tolist()
    S, R = len(d), len(d[0])
    mmd = math.fsum(min(d[s][r] for s in range(S)) for r in range(R)) / R
    return mmd, len({_first_argmin(d[s]) for s in range(S)}) / R


def one_nna_restated(d_ss, d_sr, d_rr):
    """(overall, samples, references) 1-NN accuracy with plain loops over float64 copies."""
    ss, sr, rr = (t.to(torch.float64).cpu().tolist() for t in (d_ss, d_sr, d_rr))
    S, R = len(sr), len(sr[0])
    hit = []
    for i in range(S + R):
        row = (ss[i] + sr[i]) if i < S else ([sr[s][i - S] for s in range(S)] + rr[i - S])
        row[i] = float("inf")
        hit.append((_first_argmin(row) < S) == (i < S))
    return sum(hit) / (S + R), sum(hit[:S]) / S, sum(hit[S:]) / R


def argmin_gaps(d_ss, d_sr, d_rr):
    """Smallest relative gap (second - first) / second between the row minimum and its runner-up over the rows COV uses (d_sr by
    sample) and the rows 1-NNA uses (the union matrix without its diagonal).  A row whose two smallest entries are both 0 gives 0."""
    union = torch.cat([torch.cat([d_ss, d_sr], dim=1), torch.cat([d_sr.t(), d_rr], dim=1)], dim=0).to(torch.float64).clone()
    union.fill_diagonal_(float("inf"))
    worst = 1.0
    for m in (d_sr.to(torch.float64), union):
        two = torch.topk(m, 2, dim=1, largest=False).values
        gap = torch.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], torch.zeros_like(two[:, 0]))
        worst = min(worst, float(gap.min()))
    return worst


# ---- constructed sets for the end-to-end metrics ----------------------------------------------------------------------------
def sphere_mesh(radius):
    return pc.uv_sphere(12, 16, radius=radius, squash=(1.0, 1.0, 1.0))


def torus_mesh(major, minor, shift, n_major=16, n_minor=10):
    """(verts float32 [V,3], faces int64 [F,3]) of a torus around the z axis, translated by `shift` along x."""
    v, f = [], []
    for i in range(n_major):
        a = 2 * math.pi * i / n_major
        for j in range(n_minor):
            b = 2 * math.pi * j / n_minor
            r = major + minor * math.cos(b)
            v.append((r * math.cos(a) + shift, r * math.sin(a), minor * math.sin(b)))
    at = lambda i, j: (i % n_major) * n_minor + j % n_minor          # noqa: E731
    for i in range(n_major):
        for j in range(n_minor):
            f.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            f.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    return torch.tensor(v, dtype=torch.float64).to(torch.float32), torch.tensor(f, dtype=torch.int64)


METRIC_CASES = ("identical", "concentric", "families")


def metric_meshes(name):
    """(sample meshes, reference meshes, sample uniforms [3,6,2048], reference uniforms [3,6,2048]).  "identical" names the same
    meshes and the same uniforms on both sides."""
    ks = range(1, 7)
    if name == "identical":
        m = [sphere_mesh(0.1 * k) for k in ks]
        u = torch.stack(pc.case_uniforms(6, METRIC_POINTS, 7201))
        return m, m, u, u
    if name == "concentric":
        return ([sphere_mesh(0.1 * k + 0.01) for k in ks], [sphere_mesh(0.1 * k) for k in ks],
                torch.stack(pc.case_uniforms(6, METRIC_POINTS, 7202)), torch.stack(pc.case_uniforms(6, METRIC_POINTS, 7203)))
    if name == "families":
        return ([sphere_mesh(0.1 * k) for k in ks], [torus_mesh(0.3 + 0.05 * k, 0.1, 5.0) for k in ks],
                torch.stack(pc.case_uniforms(6, METRIC_POINTS, 7204)), torch.stack(pc.case_uniforms(6, METRIC_POINTS, 7205)))
    raise KeyError(name)


def clouds_restated(meshes, uniforms):
    """The float64 restatement of the surface sampling (pointcloud_cases) on the CPU, rounded to float32: [M,2048,3].  The GPU
    sampler's clouds differ from these in the last bits; the CPU proofs of the input conditions are about these, and the GPU test
    re-checks the same conditions on its own clouds."""
    out = []
    for k, (v, f) in enumerate(meshes):
        areas = pc.face_areas_restated(v[None], f)
        ch, _ = pc.face_choices_restated(areas, uniforms[0][k:k + 1])
        out.append(pc.sample_points_restated(v[None], f, ch, uniforms[1][k:k + 1], uniforms[2][k:k + 1])[0][0].to(torch.float32))
    return torch.stack(out)
