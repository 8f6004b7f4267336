"""Generation metrics on MI355X -- host side of csrc/shape_metrics.hip.

A shape generator is judged on three figures over point clouds sampled from its meshes and from a reference set, all under
the (squared-distance) chamfer distance CD(a, b) = mean_i min_j |a_i - b_j|^2 + mean_j min_i |a_i - b_j|^2:

    MMD    minimum matching distance   mean over the references of the distance to their nearest sample
    COV    coverage                    share of the references that are the nearest reference of some sample
    1-NNA  1-nearest-neighbour accuracy of the leave-one-out classifier "sample or reference" over the union of both sets
           (0.5: the two sets cannot be told apart; 1: they are separate)

The reference tree has none of them, and no implementation was consulted: the definitions are the formulas written in the
docstrings below, and the oracle of the tests is a float64 restatement of the same formulas (tests/shape_metrics_cases.py).

The hot path is the matrix of chamfer distances between EVERY pair of clouds (`chamfer_matrix`, one launch of
md_sided_mean_matrix for a union); everything after it is torch on an [S+R, S+R] matrix.  GPU only, like pointcloud.py: a CPU
tensor is an error, not a fallback.

The same three figures under the earth mover's distance EMD(a, b) = (1/P) min over permutations pi of sum_i |a_i - b_pi(i)|
(Euclidean distance; clouds of equal size) come from `emd_matrix` (csrc/emd.hip: one workgroup per pair solves the assignment
problem exactly on distances quantised to integers), and `jsd` is the Jensen-Shannon divergence of the two sets' occupancy of
a voxel grid.  `shape_metrics(..., emd=True, jsd=True)` adds them.
"""
import math

import torch

from . import _lib
from .hip_ops import call


def _clouds(t, what):
    if not t.is_cuda:
        raise _lib.MeshDiffusionHipError(f"{what} runs on the GPU only (no CPU fallback)")
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: expected [N,P,3] point clouds with N, P >= 1, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _sided(x, y):
    if y.device != x.device:
        raise ValueError("sided_mean_matrix: both sets of clouds need the same device")
    out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=x.device)
    call("md_sided_mean_matrix", x, y, x.shape[0], y.shape[0], x.shape[1], y.shape[1], out)
    return out


def sided_mean_matrix(x, y):
    """x [Nx,P,3], y [Ny,Q,3] -> float32 [Nx,Ny], out[i,j] = mean_a min_b |x[i,a] - y[j,b]|^2: md_sided_mean_matrix.
    Direct-form fp32 distances, float64 sums in a fixed order, one rounding; bit-identical from run to run.  Non-finite
    coordinates give what torch's `d2.min(dim=1).values.mean()` gives.  Not differentiable."""
    xc = _clouds(x, "sided_mean_matrix")
    return _sided(xc, xc if y is x else _clouds(y, "sided_mean_matrix"))


def chamfer_matrix(x, y=None):
    """Squared-distance chamfer matrix float32 [Nx,Ny]: sided[x->y][i,j] + sided[y->x][j,i], the definition of
    `pointcloud.chamfer_distance` with w1 = w2 = 1.  With y=None it is the union matrix of x from ONE kernel call (S + S^T):
    exactly symmetric, and its diagonal is exactly zero for finite clouds."""
    xc = _clouds(x, "chamfer_matrix")
    if y is None or y is x:
        s = _sided(xc, xc)
        return s + s.t()
    yc = _clouds(y, "chamfer_matrix")
    return _sided(xc, yc) + _sided(yc, xc).t()


def _argmin_first(d):
    """Row-wise minimum of d [N,M] and the LOWEST column that attains it."""
    m = d.min(dim=1).values
    cols = torch.arange(d.shape[1], device=d.device)
    return m, torch.where(d == m[:, None], cols[None], d.shape[1]).min(dim=1).values


def _matrix(d, what, shape=None):
    if d.dim() != 2 or d.shape[0] < 1 or d.shape[1] < 1 or (shape is not None and tuple(d.shape) != shape):
        want = "a non-empty matrix" if shape is None else f"{shape}"
        raise ValueError(f"{what}: expected {want}, got {tuple(d.shape)}")
    return d


def mmd_cov(d_sr):
    """d_sr [S,R], samples by references -> (mmd, cov) as Python floats:
        mmd = mean_r min_s d_sr[s,r]                      (accumulated in float64)
        cov = |{argmin_r d_sr[s,:] : s}| / R              (ties to the lowest r)."""
    d = _matrix(d_sr, "mmd_cov")
    mmd = d.min(dim=0).values.to(torch.float64).mean()
    nearest_ref = _argmin_first(d)[1]
    return float(mmd), int(torch.unique(nearest_ref).numel()) / d.shape[1]


def one_nna(d_ss, d_sr, d_rr):
    """Leave-one-out 1-nearest-neighbour accuracy over the union ordered samples first: every cloud's nearest OTHER cloud (the
    diagonal excluded, ties to the lowest index) votes its label; a cloud counts when the vote is its own label.
    d_ss [S,S], d_sr [S,R], d_rr [R,R] -> (overall, over the samples, over the references) as Python floats."""
    S, R = _matrix(d_sr, "one_nna").shape
    _matrix(d_ss, "one_nna: d_ss", (S, S))
    _matrix(d_rr, "one_nna: d_rr", (R, R))
    if S + R < 2:
        raise ValueError("one_nna needs at least two clouds")
    d = torch.cat([torch.cat([d_ss, d_sr], dim=1), torch.cat([d_sr.t(), d_rr], dim=1)], dim=0).clone()
    d.fill_diagonal_(float("inf"))
    vote_sample = _argmin_first(d)[1] < S
    is_sample = torch.arange(S + R, device=d.device) < S
    right = (vote_sample == is_sample).to(torch.float64)
    return float(right.mean()), float(right[:S].mean()), float(right[S:].mean())


EMD_MAX_POINTS = 2048                                       # EMD_MAX_P of csrc/emd.hip: both clouds of a pair live in LDS
EMD_PERM_PAIRS = 4096                                       # return_info: the matchings are returned for at most this many pairs


def emd_quantum(*clouds, bits=20):
    """The power of two 2^(ceil(log2 diag) - bits) as a Python float, diag being the diagonal of the bounding box of ALL the
    clouds passed ([...,3] tensors, any device): every distance between two of their points is then at most 2^bits quanta.  A
    zero diagonal gives 2^-bits.  Plain torch."""
    if not clouds:
        raise ValueError("emd_quantum: no clouds")
    pts = [c.detach().reshape(-1, 3).to(torch.float64) for c in clouds]
    lo = torch.stack([c.min(dim=0).values for c in pts]).min(dim=0).values
    hi = torch.stack([c.max(dim=0).values for c in pts]).max(dim=0).values
    diag = float((hi - lo).square().sum().sqrt())
    if not math.isfinite(diag):
        raise ValueError("emd_quantum: a non-finite coordinate")
    if diag == 0:
        return 2.0 ** -bits
    m, e = math.frexp(diag)                                 # diag = m 2^e with 0.5 <= m < 1
    return 2.0 ** ((e - 1 if m == 0.5 else e) - bits)


def emd_matrix(x, y=None, quantum=None, max_rounds=None, return_info=False):
    """Earth mover's distance matrix float32 [Nx,Ny] of x [Nx,P,3] against y [Ny,P,3]: md_emd_matrix, one workgroup per pair.
    Distances are fp32 in the direct form, quantised to rint(d / quantum) and the integer assignment problem is solved exactly
    (forward auction, eps-scaling, 64-bit integer prices): out = total * quantum / P, so the result does not depend on the
    launch, two runs agree bit for bit and emd_matrix(x, y) == emd_matrix(y, x).t().  `quantum` is a power of two, by default
    `emd_quantum(x, y)` (20 bits); pass one value to every call whose entries are to be compared.  `max_rounds` bounds the
    bidding rounds of a pair (default 256 P + 4096; at P = 64 that is 20480, 7.1 times the worst count in tests/emd_cases.py, 2867).

    y=None or y is x: the triangular launch -- the pairs i < j only, exactly symmetric, an exactly zero diagonal.
    A cloud with a NaN or infinite coordinate gives NaN in its pairs (status 3) and nothing else.  A pair that runs out of
    rounds (status 1) or whose distances exceed 2^21 quanta (status 2) raises MeshDiffusionHipError -- unless return_info,
    which returns (out, {"status", "total", "rounds", "perm", "quantum"}) as they are: int32 [Nx,Ny], int64 [Nx,Ny] (the optimal
    integer cost, -1 where there is none), int32 [Nx,Ny] (bidding rounds run) and int32 [Nx,Ny,P] (perm[i,j,k] = the point of
    y[j] matched to point k of x[i]; None beyond 4096 pairs).  P > 2048 and P != Q are ValueErrors.  Not differentiable."""
    tri = y is None or y is x
    # the shapes first, so that they are refused the same way wherever the tensors live
    for t in (x,) if tri else (x, y):
        if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"emd_matrix: expected [N,P,3] point clouds with N, P >= 1, got {tuple(t.shape)}")
    if not tri and y.shape[1] != x.shape[1]:
        raise ValueError(f"emd_matrix: the clouds of both sets need the same number of points, got {x.shape[1]} and {y.shape[1]}")
    if x.shape[1] > EMD_MAX_POINTS:
        raise ValueError(f"emd_matrix: at most {EMD_MAX_POINTS} points per cloud, got {x.shape[1]}")
    xc = _clouds(x, "emd_matrix")
    yc = xc if tri else _clouds(y, "emd_matrix")
    if yc.device != xc.device:
        raise ValueError("emd_matrix: both sets of clouds need the same device")
    P = xc.shape[1]
    nx, ny = xc.shape[0], yc.shape[0]
    if quantum is None:
        finite = [c[torch.isfinite(c).all(dim=2).all(dim=1)] for c in ((xc,) if tri else (xc, yc))]
        finite = [c for c in finite if c.shape[0]]
        quantum = emd_quantum(*finite) if finite else 2.0 ** -20
    quantum = float(quantum)
    if max_rounds is None:
        max_rounds = 256 * P + 4096
    dev = xc.device
    out = torch.empty((nx, ny), dtype=torch.float32, device=dev)
    status = torch.empty((nx, ny), dtype=torch.int32, device=dev)
    total = torch.empty((nx, ny), dtype=torch.int64, device=dev) if return_info else None
    rounds = torch.empty((nx, ny), dtype=torch.int32, device=dev) if return_info else None
    perm = torch.empty((nx, ny, P), dtype=torch.int32, device=dev) if return_info and nx * ny <= EMD_PERM_PAIRS else None
    call("md_emd_matrix", xc, yc, nx, ny, P, quantum, int(max_rounds), 1 if tri else 0, out, status, total, rounds, perm)
    if return_info:
        return out, {"status": status, "total": total, "rounds": rounds, "perm": perm, "quantum": quantum}
    failed = torch.nonzero((status == 1) | (status == 2))
    if failed.shape[0]:
        i, j = (int(v) for v in failed[0])
        if int(status[i, j]) == 1:
            raise _lib.MeshDiffusionHipError(f"emd_matrix: pair ({i}, {j}) was not solved within max_rounds={int(max_rounds)} bidding "
                                             f"rounds: raise max_rounds")
        raise _lib.MeshDiffusionHipError(f"emd_matrix: pair ({i}, {j}) has distances beyond 2^21 quanta of quantum={quantum!r}: pass a "
                                         f"larger quantum (emd_quantum of all the clouds)")
    return out


def jsd(sample_clouds, ref_clouds, resolution=28):
    """Jensen-Shannon divergence, in bits, between the occupancy histograms of two SETS of clouds [N,P,3] on a resolution^3 grid
    over [-0.5, 0.5]^3 (the range of `normalize_clouds(..., "bbox")`): every point of every cloud of a set is counted into the
    cell clamp(floor((c + 0.5) * resolution), 0, resolution - 1) per axis, each histogram is divided by its total, and
        JSD = H((P + Q) / 2) - (H(P) + H(Q)) / 2,      H = the entropy with base-2 logarithms,
    which lies in [0, 1]: 0 for equal histograms, 1 for disjoint ones.  Plain torch in float64 on the device of the inputs; a
    non-finite coordinate is a ValueError."""
    res = int(resolution)
    if res < 1:
        raise ValueError(f"jsd: resolution must be at least 1, got {resolution}")
    hist = []
    for name, c in (("sample_clouds", sample_clouds), ("ref_clouds", ref_clouds)):
        if c.dim() < 2 or c.shape[-1] != 3 or c.numel() == 0:
            raise ValueError(f"jsd: {name}: expected [...,P,3] point clouds, got {tuple(c.shape)}")
        pts = c.detach().reshape(-1, 3).to(torch.float64)
        if not bool(torch.isfinite(pts).all()):
            raise ValueError(f"jsd: {name} holds a non-finite coordinate")
        cell = torch.floor((pts + 0.5) * res).clamp_(0, res - 1).to(torch.int64)
        flat = (cell[:, 0] * res + cell[:, 1]) * res + cell[:, 2]
        h = torch.bincount(flat, minlength=res ** 3).to(torch.float64)
        hist.append(h / h.sum())
    if hist[0].device != hist[1].device:
        raise ValueError("jsd: both sets of clouds need the same device")

    def entropy(h):
        nz = h[h > 0]
        return -(nz * torch.log2(nz)).sum()

    return float(entropy((hist[0] + hist[1]) / 2) - (entropy(hist[0]) + entropy(hist[1])) / 2)


def shape_metrics(sample_clouds, ref_clouds, emd=False, jsd=False):
    """MMD / COV / 1-NNA under the chamfer distance of samples [S,P,3] against references [R,Q,3].  One kernel call on the
    concatenation when P == Q, three `chamfer_matrix` calls otherwise.  Returns {"mmd_cd", "cov_cd", "1nna_cd",
    "1nna_cd_sample", "1nna_cd_ref", "n_sample", "n_ref", "points"} (`points` = [P, Q]).  A cloud with a non-finite
    coordinate makes its whole row of the matrix non-finite; the first such cloud is named in a ValueError.
    emd=True (needs P == Q <= 2048) adds "mmd_emd", "cov_emd", "1nna_emd", "1nna_emd_sample", "1nna_emd_ref" from ONE triangular
    `emd_matrix` of the concatenation, and "emd_quantum", the `emd_quantum` of both sets it was computed with.  jsd=True adds
    "jsd" (`jsd` at its default resolution)."""
    s, r = _clouds(sample_clouds, "shape_metrics"), _clouds(ref_clouds, "shape_metrics")
    S, R = s.shape[0], r.shape[0]
    if emd and s.shape[1] != r.shape[1]:
        raise ValueError(f"shape_metrics: emd=True needs the same number of points on both sides, got {s.shape[1]} and {r.shape[1]}")
    if s.shape[1] == r.shape[1]:
        d = chamfer_matrix(torch.cat([s, r], dim=0))
    else:
        d_sr = chamfer_matrix(s, r)
        d = torch.cat([torch.cat([chamfer_matrix(s), d_sr], dim=1), torch.cat([d_sr.t(), chamfer_matrix(r)], dim=1)], dim=0)
    bad = ~torch.isfinite(d)
    if bool(bad.any()):
        whole = bad.all(dim=1)
        k = int(torch.nonzero(whole if bool(whole.any()) else bad.any(dim=1))[0])
        name = f"sample cloud {k}" if k < S else f"reference cloud {k - S}"
        raise ValueError(f"shape_metrics: {name} has non-finite chamfer distances (a NaN or infinite coordinate?)")
    d_ss, d_sr, d_rr = d[:S, :S], d[:S, S:], d[S:, S:]
    mmd, cov = mmd_cov(d_sr)
    acc, acc_s, acc_r = one_nna(d_ss, d_sr, d_rr)
    rec = {"mmd_cd": mmd, "cov_cd": cov, "1nna_cd": acc, "1nna_cd_sample": acc_s, "1nna_cd_ref": acc_r, "n_sample": S,
           "n_ref": R, "points": [int(s.shape[1]), int(r.shape[1])]}
    if emd:
        quantum = emd_quantum(s, r)
        e = emd_matrix(torch.cat([s, r], dim=0), quantum=quantum)
        mmd, cov = mmd_cov(e[:S, S:])
        acc, acc_s, acc_r = one_nna(e[:S, :S], e[:S, S:], e[S:, S:])
        rec.update({"mmd_emd": mmd, "cov_emd": cov, "1nna_emd": acc, "1nna_emd_sample": acc_s, "1nna_emd_ref": acc_r,
                    "emd_quantum": quantum})
    if jsd:
        rec["jsd"] = _jsd(s, r)
    return rec


_jsd = jsd                                                  # `shape_metrics` has a flag of that name


def normalize_clouds(points, mode="bbox"):
    """points [...,P,3].  mode "bbox": every cloud is centred on the centre of its bounding box and scaled so that the box's
    longest side is 1; "none": returned as it is.  Plain torch, any device."""
    if mode == "none":
        return points
    if mode != "bbox":
        raise ValueError(f"normalize_clouds: mode must be 'bbox' or 'none', got {mode!r}")
    lo, hi = points.min(dim=-2, keepdim=True).values, points.max(dim=-2, keepdim=True).values
    side = (hi - lo).max(dim=-1, keepdim=True).values
    if not bool((side > 0).all()):
        raise ValueError("normalize_clouds: a cloud has a bounding box without extent")
    return (points - (lo + hi) / 2) / side


def clouds_from_meshes(meshes, n_points=2048, generator=None, uniforms=None, skip_empty=False):
    """meshes: a list of (verts [V,3], faces [F,3]) -- tensors or arrays; anything not already on a GPU is moved to the current
    one.  Each mesh goes through `pointcloud.sample_points` (area-weighted surface sampling).  Returns (clouds float32
    [M,n_points,3], skipped): a mesh without faces raises a ValueError with its index, or with skip_empty=True is left out
    and its index listed in `skipped`.  `uniforms` [3,len(meshes),n_points] in [0, 1) fixes the draws of mesh k to
    uniforms[:, k]; otherwise torch.rand on the device with `generator`."""
    from .pointcloud import sample_points
    clouds, skipped = [], []
    for k, (verts, faces) in enumerate(meshes):
        dev = verts.device if isinstance(verts, torch.Tensor) and verts.is_cuda else torch.device("cuda")
        v = torch.as_tensor(verts, dtype=torch.float32, device=dev).reshape(-1, 3)
        f = torch.as_tensor(faces, device=dev).to(torch.int64).reshape(-1, 3)
        if f.shape[0] == 0 or v.shape[0] == 0:
            if not skip_empty:
                raise ValueError(f"clouds_from_meshes: mesh {k} has no faces")
            skipped.append(k)
            continue
        u = None if uniforms is None else torch.as_tensor(uniforms)[:, k:k + 1].to(dev)
        clouds.append(sample_points(v[None], f, n_points, uniforms=u, generator=generator)[0][0].detach())
    if not clouds:
        raise ValueError("clouds_from_meshes: no mesh with faces")
    return torch.stack(clouds), skipped
