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
"""
import torch

from . import _lib
from .hip_ops import _ptr, _stream


def _clouds(t, what):
    if not t.is_cuda:
        raise _lib.MeshDiffusionHipError(f"{what} runs on the GPU only (no CPU fallback)")
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: expected [N,P,3] point clouds with N, P >= 1, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _sided(x, y):
    lib = _lib.load()
    if y.device != x.device:
        raise ValueError("sided_mean_matrix: both sets of clouds need the same device")
    out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=x.device)
    _lib.check(lib.md_sided_mean_matrix(_ptr(x), _ptr(y), x.shape[0], y.shape[0], x.shape[1], y.shape[1], _ptr(out),
                                        _stream()), "md_sided_mean_matrix")
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


def shape_metrics(sample_clouds, ref_clouds):
    """MMD / COV / 1-NNA under the chamfer distance of samples [S,P,3] against references [R,Q,3].  One kernel call on the
    concatenation when P == Q, three `chamfer_matrix` calls otherwise.  Returns {"mmd_cd", "cov_cd", "1nna_cd",
    "1nna_cd_sample", "1nna_cd_ref", "n_sample", "n_ref", "points"} (`points` = [P, Q]).  A cloud with a non-finite
    coordinate makes its whole row of the matrix non-finite; the first such cloud is named in a ValueError."""
    s, r = _clouds(sample_clouds, "shape_metrics"), _clouds(ref_clouds, "shape_metrics")
    S, R = s.shape[0], r.shape[0]
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
    return {"mmd_cd": mmd, "cov_cd": cov, "1nna_cd": acc, "1nna_cd_sample": acc_s, "1nna_cd_ref": acc_r, "n_sample": S,
            "n_ref": R, "points": [int(s.shape[1]), int(r.shape[1])]}


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
