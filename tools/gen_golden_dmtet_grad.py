"""Generate tests/golden/dmtet_grad.npz by running the UNMODIFIED reference `DMTet.__call__`, `sdf_reg_loss` and
`DMTetGeometry` (nvdiffrec/lib/geometry/dmtet.py) under autograd on the CPU, imported from the reference checkout the way
oracle/gen_golden.py does (build host only: the GPU machines have no reference):
    python tools/gen_golden_dmtet_grad.py

  <case>/...   cases smooth, sphere, box_zeros, noise of oracle.gen_golden.dmtet_cases on the shipped 64 grid, loss
               sum(verts * G), G = randn(V, 3) under <case>/seed: the reference's pos.grad / sdf.grad.  The three small
               cases store every non-zero row (rows, dpos, dsdf in fp32); `noise` stores rows 0, 16, 32, ..., the fp64
               column sums and the vertices the reference leaves at exactly zero.
  <case>/ref_err_dpos, ref_err_dsdf   the reference's OWN rel-L2 distance from the float64 restatement of the same
               expressions (tests/dmtet_grad_cases.py): the unit of every bar of the GPU tests.
  reg/<case>/...   sdf_reg_loss value and gradient on smooth and noise, with the reference's own error as above.
  fit/...      the fitting run of tests/test_gpu_dmtet_grad.py: reference data loss at steps 0, 10, 20, 40 in fp32 and
               fp64, and V at step 0.

Before anything is written the float64 restatement is asserted against the reference (rel-L2 <= 5e-6: a float32
reference cannot sit closer to a wrong restatement than that, nor farther from a right one).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dmtet_grad_cases as dg  # noqa: E402
from oracle.gen_golden import GOLD, REF, _CudaToCpu, dmtet_cases, import_ref_dmtet  # noqa: E402

SEEDS = {"smooth": 4101, "sphere": 4102, "box_zeros": 4103, "noise": 4104}
RESTATEMENT_BOUND = 5e-6


def gen_grads(mod, verts, idx, out):
    pos, cases = dmtet_cases(verts)
    tets_t = torch.as_tensor(idx, dtype=torch.long)
    edges = dg.unique_edges(tets_t)
    N = pos.shape[0]
    with _CudaToCpu():
        dm = mod.DMTet()
        for name in dg.GRAD_CASES:
            sdf = cases[name]
            p = pos.clone().requires_grad_(True)
            s = sdf.clone().requires_grad_(True)
            v = dm(p, s, tets_t)[0]
            G = dg.case_G(v.shape[0], SEEDS[name])
            (v * G).sum().backward()
            dpos, dsdf = p.grad, s.grad
            v64 = dg.restated_verts(pos, sdf, edges)
            assert v64.shape == v.shape and dg.rel_l2(v, v64) < 1e-6, name
            dpos64, dsdf64 = dg.restated_grads(pos, sdf, edges, G)
            ep, es = dg.rel_l2(dpos, dpos64), dg.rel_l2(dsdf, dsdf64)
            assert ep < RESTATEMENT_BOUND and es < RESTATEMENT_BOUND, (name, ep, es)
            den = (sdf[dg.crossing_edges(sdf, edges)] * torch.tensor([1.0, -1.0])).sum(1).abs()
            nz = ((dpos != 0).any(1) | (dsdf != 0)).nonzero()[:, 0]
            print(f"[dmtet_grad] {name}: V={v.shape[0]} non-zero rows {nz.numel()}  reference vs float64: dpos {ep:.2e} "
                  f"dsdf {es:.2e}  min|den| {float(den.min()):.2e} max|dsdf| {float(dsdf.abs().max()):.3g}")
            out[f"{name}/seed"], out[f"{name}/V"] = np.int64(SEEDS[name]), np.int64(v.shape[0])
            out[f"{name}/ref_err_dpos"], out[f"{name}/ref_err_dsdf"] = np.float64(ep), np.float64(es)
            if name == "noise":
                rows = torch.arange(0, N, dg.NOISE_STRIDE)
                out[f"{name}/dpos_colsum"] = dpos.double().sum(0).numpy()
                out[f"{name}/dsdf_sum"] = np.float64(dsdf.double().sum())
                out[f"{name}/zero_dpos"] = (dpos == 0).all(1).nonzero()[:, 0].numpy().astype(np.int32)
                out[f"{name}/zero_dsdf"] = (dsdf == 0).nonzero()[:, 0].numpy().astype(np.int32)
            else:
                rows = nz
            out[f"{name}/rows"] = rows.numpy().astype(np.int32)
            out[f"{name}/dpos"] = dpos[rows].numpy().astype(np.float32)
            out[f"{name}/dsdf"] = dsdf[rows].numpy().astype(np.float32)
        for name in dg.REG_CASES:
            s = cases[name].clone().requires_grad_(True)
            loss = mod.sdf_reg_loss(s, edges)
            loss.backward()
            loss64, g64 = dg.restated_sdf_reg(cases[name], edges)
            ev, eg = abs(float(loss) - float(loss64)) / abs(float(loss64)), dg.rel_l2(s.grad, g64)
            assert ev < RESTATEMENT_BOUND and eg < RESTATEMENT_BOUND, (name, ev, eg)
            nz = (s.grad != 0).nonzero()[:, 0]
            print(f"[dmtet_grad] sdf_reg_loss {name}: {float(loss):.7f}  non-zero rows {nz.numel()}  reference vs float64: "
                  f"value {ev:.2e} grad {eg:.2e}")
            rows = torch.arange(0, N, dg.NOISE_STRIDE) if name == "noise" else nz
            out[f"reg/{name}/value"] = np.float32(float(loss))
            out[f"reg/{name}/value64"] = np.float64(float(loss64))
            out[f"reg/{name}/ref_err_value"], out[f"reg/{name}/ref_err_grad"] = np.float64(ev), np.float64(eg)
            out[f"reg/{name}/rows"] = rows.numpy().astype(np.int32)
            out[f"reg/{name}/grad"] = s.grad[rows].numpy().astype(np.float32)
            out[f"reg/{name}/grad_sum"] = np.float64(s.grad.double().sum())
            out[f"reg/{name}/n_nonzero"] = np.int64(nz.numel())


def run_fit(mod, dtype):
    """fit_dmtets.py's geometry loop without the renderer: the reference's DMTetGeometry, marching tets and regulariser."""
    with _CudaToCpu():
        geo = mod.DMTetGeometry(64, 2.1, None, root=os.path.join(REF, "nvdiffrec"), deform_scale=2.0)
        geo.verts = geo.verts.to(dtype)
        with torch.no_grad():
            geo.sdf.data = dg.fit_initial_sdf(geo.verts).to(dtype)
            geo.deform.data = torch.zeros_like(geo.verts)
        opt = torch.optim.Adam([geo.sdf, geo.deform], lr=0.01)
        losses, V0 = [], None
        for step in range(41):
            opt.zero_grad()
            verts = geo.marching_tets(geo.get_deformed(), geo.sdf, geo.indices)[0]
            data = dg.fit_data_loss(verts)
            (data + 0.01 * mod.sdf_reg_loss(geo.sdf, geo.all_edges)).backward()
            opt.step()
            losses.append(float(data))
            V0 = verts.shape[0] if V0 is None else V0
    return np.array([losses[k] for k in dg.FIT_STEPS], np.float64), V0


def main():
    if not torch.cuda.is_available():
        torch.Tensor.cuda = lambda self, *a, **k: self      # DMTetGeometry.__init__ hard-codes .cuda()
    tet = np.load(os.path.join(GOLD, "64_tets_cropped.npz"))
    mod = import_ref_dmtet()
    out = {}
    gen_grads(mod, tet["vertices"], tet["indices"], out)
    l32, V32 = run_fit(mod, torch.float32)
    l64, V64 = run_fit(mod, torch.float64)
    assert V32 == V64
    print("[dmtet_grad] fit: V0", V32, " data loss fp32", l32, " fp64", l64, " rel gap", np.abs(l32 - l64) / l64)
    out["fit/steps"], out["fit/loss32"], out["fit/loss64"], out["fit/V0"] = np.array(dg.FIT_STEPS), l32, l64, np.int64(V32)
    path = os.path.join(GOLD, "dmtet_grad.npz")
    np.savez_compressed(path, **out)
    print(f"[dmtet_grad] wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
