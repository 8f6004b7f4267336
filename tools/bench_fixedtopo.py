"""What the fixed-topology plan saves per iteration of pass 2, on the shipped 64 grid, one process:
  * plan path  : DMTetGeometryFixedTopo.getMesh(normals_grad=True) (md_fixedtopo_verts, vertex_normals over the plan's CSR) +
                 render.laplace_regularizer_const(base=, corner_csr=) (md_laplace_umbrella), forward and backward;
  * parent path: what the commit before the plan has to run for the same numbers: DMTet() on sign * 1 every iteration (four
                 launches, the counts read on the host, uvs and valid vertices rebuilt), vertex_normals unplanned (range check,
                 sort, searchsorted) and the reference's Laplacian as fp32 torch ops (tests/fixedtopo_cases.py laplace_reference:
                 gathers, six scatter_add_, their autograd).
Cases: the sign of a sphere (V ~ 4k) and `noise`, random signs.  Device events after warm-up; the variants alternate round by
round and each figure is the median over rounds.
    python tools/bench_fixedtopo.py [--rounds 7] [--reps 10] [--json PATH]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pc import interleaved  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fixedtopo.py needs a GPU: the HIP path has no CPU fallback")
    import fixedtopo_cases as fc
    import raster_cases as rc
    from meshdiffusion_amd import dmtet, render

    rec = {"rounds": a.rounds, "reps": a.reps, "cases": {}}
    for case in ("sphere", "noise"):
        first = dmtet.DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
        with torch.no_grad():
            first.sdf.copy_(rc.case_sdf(case, first.verts.cpu()).cuda() if case == "noise" else first.verts.norm(dim=1) - 0.7)
            first.deform.copy_((torch.rand(first.verts.shape, generator=torch.Generator().manual_seed(1)) * 0.2 - 0.1).cuda())
        geo = dmtet.DMTetGeometryFixedTopo(first, 64, rc.MESH_SCALE, deform_scale=2.0)
        with torch.no_grad():
            geo.initial_guess_v_pos = geo.initial_guess_v_pos + 0.01        # a displacement for the Laplacian to measure
        base, sign, mt = geo.initial_guess_v_pos, geo.sdf_sign.detach().clone(), dmtet.DMTet()
        V, F = geo.plan.n_mesh_verts, geo.plan.faces.shape[0]
        Gn = torch.randn(V, 3, generator=torch.Generator().manual_seed(2)).cuda()

        def plan_path():
            geo.deform.grad = None
            mesh = geo.getMesh(normals_grad=True)
            lap = render.laplace_regularizer_const(mesh.v_pos, mesh.t_pos_idx, base=base, corner_csr=geo.plan.corner_csr)
            ((mesh.v_nrm * Gn).sum() + lap).backward()
            return lap.detach(), geo.deform.grad

        def parent_path():
            geo.deform.grad = None
            verts, faces = mt(geo.get_deformed(), sign * 1.0, geo.indices)[:2]
            v_nrm = dmtet.vertex_normals(verts, faces)[0]
            lap = fc.laplace_reference(verts - base, faces)
            ((v_nrm * Gn).sum() + lap).backward()
            return lap.detach(), geo.deform.grad

        (l1, g1), (l2, g2) = plan_path(), parent_path()
        agree = (abs(float(l1) - float(l2)) / abs(float(l2)), rc.rel_l2(g1, g2))
        for _ in range(2):
            plan_path(); parent_path()
        torch.cuda.synchronize()
        med, raw = interleaved({"plan": plan_path, "parent": parent_path}, a.rounds, a.reps)
        print(f"{case} (V {V} F {F}): getMesh + vertex_normals + Laplacian, forward+backward: plan path {med['plan']:.3f} ms | parent "
              f"path {med['parent']:.3f} ms | x{med['parent'] / med['plan']:.2f} | Laplacian values differ by {agree[0]:.1e} relative, "
              f"d deform by rel-L2 {agree[1]:.1e}", flush=True)
        rec["cases"][case] = {"V": V, "F": F, "plan_ms": round(med["plan"], 4), "parent_ms": round(med["parent"], 4), "raw": raw}
    print(json.dumps({k: ({c: {q: w for q, w in v.items() if q != "raw"} for c, v in rec["cases"].items()} if k == "cases" else v)
                      for k, v in rec.items()}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
