"""Float64 restatement of the differentiable part of the reference's marching tetrahedra (nvdiffrec/lib/geometry/dmtet.py
:125-132) and of its SDF regulariser (:169-175), over the STATIC sorted unique edge table, so that a machine without the
reference can evaluate the reference's expressions on any input.  tools/gen_golden_dmtet_grad.py asserts these against
the unmodified reference before it writes tests/golden/dmtet_grad.npz; tests/test_cpu_dmtet_grad_host.py re-checks that
on the fixture.  Shared by the CPU and GPU tests and by tools/bench_dmtet_grad.py (as the torch-autograd chain a user has
without the kernel).
"""
import numpy as np
import torch

GRAD_CASES = ("smooth", "sphere", "box_zeros", "noise")
REG_CASES = ("smooth", "noise")
NOISE_STRIDE = 16                      # the fixture keeps rows 0, 16, 32, ... of the `noise` case
FIT_STEPS = (0, 10, 20, 40)


def unique_edges(tets):
    """Lexicographically sorted unique (min, max) vertex pairs of all tets: int64 [E,2] (dmtet.py:239-244)."""
    t = torch.as_tensor(tets).long()
    be = torch.tensor([0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3], dtype=torch.int64, device=t.device)
    e = t[:, be].reshape(-1, 2)
    return torch.unique(torch.sort(e, dim=1)[0], dim=0)


def crossing_edges(sdf, edges):
    """Edges with exactly one endpoint of sdf > 0, in table order: the reference's vertex order (dmtet.py:119-124)."""
    occ = sdf > 0
    return edges[occ[edges[:, 0]] != occ[edges[:, 1]]]


def restated_verts(pos, sdf, edges, dtype=torch.float64):
    """dmtet.py:125-132 on the crossing edges, in `dtype`."""
    ce = crossing_edges(sdf, edges)
    p, s = pos.to(dtype), sdf.to(dtype)
    ep = p[ce.reshape(-1)].reshape(-1, 2, 3)
    es = s[ce.reshape(-1)].reshape(-1, 2, 1)
    es = es * torch.tensor([1.0, -1.0], dtype=dtype, device=es.device).reshape(1, 2, 1)
    den = es.sum(1, keepdim=True)
    w = torch.flip(es, [1]) / den
    return (ep * w).sum(1)


def restated_grads(pos, sdf, edges, G, dtype=torch.float64):
    """d sum(verts * G) / d(pos, sdf) by autograd over restated_verts: (dpos [N,3], dsdf [N]) in `dtype`."""
    p = pos.detach().to(dtype).requires_grad_(True)
    s = sdf.detach().to(dtype).requires_grad_(True)
    v = restated_verts(p, s, edges, dtype)
    if v.shape[0] == 0:
        return torch.zeros_like(p), torch.zeros_like(s)
    (v * G.to(dtype)).sum().backward()
    return p.grad, s.grad


def restated_sdf_reg(sdf, edges, dtype=torch.float64):
    """dmtet.py:169-175 in `dtype`: (loss, dloss/dsdf)."""
    s = sdf.detach().to(dtype).requires_grad_(True)
    se = s[edges.reshape(-1)].reshape(-1, 2)
    m = torch.sign(se[..., 0]) != torch.sign(se[..., 1])
    se = se[m]
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    loss = bce(se[..., 0], (se[..., 1] > 0).to(dtype)) + bce(se[..., 1], (se[..., 0] > 0).to(dtype))
    loss.backward()
    return loss.detach(), s.grad


def case_G(V, seed):
    """The cotangent of a case: randn [V,3] float32 under the fixture's recorded seed (CPU generator)."""
    return torch.randn(V, 3, generator=torch.Generator().manual_seed(int(seed)))


def fixture_rows(gold, case, N):
    """(rows int64 [K], dpos float32 [K,3], dsdf float32 [K]) of the reference gradients the fixture stores for `case`."""
    rows = gold[f"{case}/rows"].astype(np.int64)
    return rows, gold[f"{case}/dpos"], gold[f"{case}/dsdf"]


def fixture_zero_rows(gold, case, N):
    """(vertices whose reference dpos row is exactly zero, vertices whose reference dsdf is exactly zero)."""
    if f"{case}/zero_dpos" in gold.files:
        return gold[f"{case}/zero_dpos"].astype(np.int64), gold[f"{case}/zero_dsdf"].astype(np.int64)
    rows, dpos, dsdf = fixture_rows(gold, case, N)       # a case stored whole: every row not stored is zero in both
    zp, zs = np.ones(N, bool), np.ones(N, bool)
    zp[rows] = (dpos == 0).all(1)
    zs[rows] = dsdf == 0
    return np.nonzero(zp)[0], np.nonzero(zs)[0]


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def fit_initial_sdf(verts_scaled):
    """The fitting run's start: sdf = 0.45 - |v| on the scaled tet vertices."""
    return 0.45 - verts_scaled.norm(dim=1)


def fit_data_loss(verts):
    return ((verts.norm(dim=1) - 0.6) ** 2).mean()
