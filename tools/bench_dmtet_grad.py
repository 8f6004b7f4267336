"""Differentiable marching tetrahedra, forward + backward on the shipped 64 grid, one process:
  * kernel path: marching_tets_batch under autograd (md_marching_tets, four launches, + md_marching_tets_bwd, one launch);
  * torch path : the reference's differentiable expressions (dmtet.py:119-132) as float32 torch ops under autograd on the
    static edge table (tests/dmtet_grad_cases.py) -- what a user has without the kernel; its topology part (faces) is NOT
    computed, the kernel path's is.  One mesh per call, as the reference's DMTet: M meshes are M calls.
M = 1 and M = 32 on the `smooth` and `noise` inputs, cotangent fixed.  Device events after warm-up; the variants alternate
round by round and each figure is the median over rounds.  Also md_sdf_reg_loss forward + backward against its torch chain.
    python tools/bench_dmtet_grad.py [--rounds 7] [--reps 10] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np
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
        raise SystemExit("bench_dmtet_grad.py needs a GPU: the HIP path has no CPU fallback")
    import dmtet_grad_cases as dg
    from meshdiffusion_amd.dmtet import TetTables, marching_tets_batch, sdf_reg_loss
    from oracle.gen_golden import dmtet_cases

    tet = np.load(os.path.join(ROOT, "tests", "golden", "64_tets_cropped.npz"))
    pos, cases = dmtet_cases(tet["vertices"])
    pos = pos.cuda()
    tets_t = torch.as_tensor(tet["indices"], dtype=torch.long).cuda()
    tb = TetTables(tets_t, tets_t.device)
    edges = tb.all_edges
    N, E, T = pos.shape[0], tb.n_edges, tb.n_tets
    # incidence list + edge table (once per launch, shared by the meshes); per mesh: vid, pos + sdf, grad rows, outputs
    rec = {"N": N, "E": E, "rounds": a.rounds, "reps": a.reps, "cases": {}}
    for case in ("smooth", "noise"):
        for M in (1, 32):
            sdf1 = cases[case].cuda()
            posb = pos[None].expand(M, N, 3).contiguous()
            sdfb = torch.stack([sdf1 if case == "noise" else sdf1 + 0.003 * m for m in range(M)]).contiguous()
            Gfull = torch.randn(M, E, 3, generator=torch.Generator().manual_seed(5)).cuda()
            V = [int(dg.crossing_edges(sdfb[m], edges).shape[0]) for m in range(M)]

            def hip_path():
                p, s = posb.detach().requires_grad_(True), sdfb.detach().requires_grad_(True)
                meshes, _ = marching_tets_batch(p, s, tb)
                torch.autograd.backward(meshes.verts, Gfull)
                return p.grad, s.grad

            def torch_path():
                out = []
                for m in range(M):
                    p, s = posb[m].detach().requires_grad_(True), sdfb[m].detach().requires_grad_(True)
                    v = dg.restated_verts(p, s, edges, torch.float32)
                    torch.autograd.backward(v, Gfull[m, :v.shape[0]])
                    out.append((p.grad, s.grad))
                return out

            hp, hs = hip_path()
            tp, ts = torch_path()[M - 1]
            agree = (dg.rel_l2(hp[M - 1], tp), dg.rel_l2(hs[M - 1], ts))
            for _ in range(2):
                hip_path(); torch_path()
            torch.cuda.synchronize()
            med, raw = interleaved({"hip": hip_path, "torch": torch_path}, a.rounds, a.reps if M == 1 else max(2, a.reps // 5))
            # bytes the backward launch has to move: static tables once, per mesh vid + pos/sdf + outputs + touched grad rows
            nbytes = (2 * E + N + 1) * 4 + 2 * E * 4 + sum(E * 4 + N * 16 + N * 16 + 12 * v for v in V)
            print(f"{case} M={M} (V {min(V)}..{max(V)}): forward+backward kernel path {med['hip']:.3f} ms | torch autograd chain "
                  f"{med['torch']:.3f} ms | x{med['torch'] / med['hip']:.1f} | backward bytes {nbytes / 1e6:.1f} MB | "
                  f"rel-L2 between the two dpos {agree[0]:.1e} dsdf {agree[1]:.1e}", flush=True)
            rec["cases"][f"{case}_M{M}"] = {"hip_ms": round(med["hip"], 4), "torch_ms": round(med["torch"], 4),
                                            "bwd_bytes": nbytes, "V_min": min(V), "V_max": max(V), "raw": raw}

    # md_marching_tets_bwd alone (M = 32, noise: the worst case), for the bandwidth figure
    for case in ("smooth", "noise"):
        M = 32
        sdfb = torch.stack([cases[case].cuda()] * M).contiguous()
        posb = pos[None].expand(M, N, 3).contiguous()
        Gfull = torch.randn(M, E, 3, generator=torch.Generator().manual_seed(5)).cuda()
        p, s = posb.detach().requires_grad_(True), sdfb.detach().requires_grad_(True)
        meshes, cnt = marching_tets_batch(p, s, tb)
        V = int(cnt[0, 0])

        def bwd_only():
            torch.autograd.backward(meshes.verts, Gfull, retain_graph=True, inputs=[p, s])

        for _ in range(3):
            bwd_only()
        torch.cuda.synchronize()
        med, raw = interleaved({"bwd": bwd_only}, a.rounds, a.reps)
        nbytes = (2 * E + N + 1) * 4 + 2 * E * 4 + M * (E * 4 + N * 16 + N * 16 + 12 * V)
        print(f"md_marching_tets_bwd {case} M={M}: {med['bwd']:.3f} ms per backward (with torch's gradient accumulation), "
              f"{nbytes / 1e6:.1f} MB -> {nbytes / med['bwd'] / 1e6:.0f} GB/s", flush=True)
        rec["cases"][f"bwd_only_{case}_M{M}"] = {"ms": round(med["bwd"], 4), "bytes": nbytes}

    for case in ("smooth", "noise"):
        sdf1 = cases[case].cuda()

        def hip_reg():
            s = sdf1.detach().requires_grad_(True)
            sdf_reg_loss(s, edges).backward()
            return s.grad

        def torch_reg():
            return dg.restated_sdf_reg(sdf1, edges, torch.float32)[1]

        agree = dg.rel_l2(hip_reg(), torch_reg())
        for _ in range(2):
            hip_reg(); torch_reg()
        torch.cuda.synchronize()
        med, raw = interleaved({"hip": hip_reg, "torch": torch_reg}, a.rounds, a.reps)
        print(f"sdf_reg_loss {case}: forward+backward kernel path {med['hip']:.3f} ms | torch chain {med['torch']:.3f} ms | "
              f"x{med['torch'] / med['hip']:.1f} | rel-L2 between the gradients {agree:.1e}", flush=True)
        rec["cases"][f"reg_{case}"] = {"hip_ms": round(med["hip"], 4), "torch_ms": round(med["torch"], 4), "raw": raw}
    print(json.dumps({k: ({c: {q: w for q, w in v.items() if q != "raw"} for c, v in rec["cases"].items()} if k == "cases" else v)
                      for k, v in rec.items()}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
