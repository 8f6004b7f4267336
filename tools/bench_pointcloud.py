"""Point-cloud supervision cost, one process, kernel path against the best torch formulation on the same GPU:
  (a) md_nn_sided, one direction, N = M in --sizes, against a chunked `torch.cdist(...).min(1)` loop (chunk chosen so the
      distance block stays under 1 GB);
  (b) chamfer_distance forward + backward (both directions, both gradients) against that loop with index-gather autograd;
  (c) one fit_to_points iteration on the shipped 64 grid split into marching tets / sampling / chamfer / regulariser / Adam,
      with the torch formulation of the two new stages beside them.
Device events after warm-up; the variants alternate round by round and each figure is the median over rounds.  Reports pair
evaluations per second and the implied share of the fp32 vector peak (PAIR_OPS lane-operations per pair against 157.3 TF).
    python tools/bench_pointcloud.py [--sizes 10000 50000 200000] [--rounds 5] [--reps 5] [--json PATH]"""
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

PAIR_OPS = 9            # 3 subtractions, 1 multiply, 2 multiply-adds (2 flops each), 1 compare, 2 selects: lane-operations, fused ones once
PEAK_FP32 = 157.3e12
BLOCK_BYTES = 1 << 30


def torch_nn(p, q):
    """Nearest neighbour of every p [N,3] in q [M,3] with torch ops: (dist2, idx)."""
    rows = max(1, BLOCK_BYTES // (4 * q.shape[0]))
    d, i = [], []
    for s in range(0, p.shape[0], rows):
        m = torch.cdist(p[s:s + rows], q).min(dim=1)
        d.append(m.values)
        i.append(m.indices)
    return torch.cat(d) ** 2, torch.cat(i)


def torch_chamfer(p, q):
    with torch.no_grad():
        i12, i21 = torch_nn(p, q)[1], torch_nn(q, p)[1]
    return ((p - q[i12]) ** 2).sum(-1).mean() + ((q - p[i21]) ** 2).sum(-1).mean()


def torch_sample(verts, faces, uni):
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with torch.no_grad():
        areas = 0.5 * torch.linalg.cross(v1 - v0, v2 - v0, dim=-1).norm(dim=-1)
        cdf = torch.cumsum(areas.double(), 0).float()
        ch = torch.searchsorted(cdf, uni[0][0] * cdf[-1], right=True).clamp_max(faces.shape[0] - 1)
    u, v = torch.sqrt(uni[1][0])[:, None], uni[2][0][:, None]
    return (1 - u) * v0[ch] + u * (1 - v) * v1[ch] + u * v * v2[ch]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 50000, 200000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud.py needs a GPU: the HIP path has no CPU fallback")
    import pointcloud_cases as pc
    from meshdiffusion_amd.dmtet import DMTetGeometry, sdf_reg_loss
    from meshdiffusion_amd.pointcloud import chamfer_distance, sample_points, sdf_regularizer_weight, sided_distance

    rec = {"rounds": a.rounds, "reps": a.reps, "nn": {}, "chamfer": {}, "fit": {}}
    for n in a.sizes:
        p = pc.sphere_cloud(n, 0.8, (0.0, 0.0, 0.0), 1).cuda()
        q = pc.sphere_cloud(n, 0.75, (0.03, -0.02, 0.01), 2).cuda()
        hd, hi = sided_distance(p[None], q[None])
        td, ti = torch_nn(p, q)
        same = float((hi[0] == ti).double().mean())
        worst_torch = float(((td - hd[0]).abs() / hd[0]).max())
        reps = a.reps if n <= 50000 else max(1, a.reps // 3)
        for _ in range(2):
            sided_distance(p[None], q[None]); torch_nn(p, q)
        torch.cuda.synchronize()
        med, raw = interleaved({"hip": lambda: sided_distance(p[None], q[None]), "torch": lambda: torch_nn(p, q)}, a.rounds, reps)
        pairs = n * n / (med["hip"] * 1e-3)
        print(f"nn one direction N=M={n}: md_nn_sided {med['hip']:.3f} ms | chunked cdist+min {med['torch']:.3f} ms | x{med['torch'] / med['hip']:.1f} | "
              f"{pairs / 1e12:.2f} T pairs/s = {pairs * PAIR_OPS / PEAK_FP32 * 100:.1f} % of the fp32 vector peak at {PAIR_OPS} ops/pair | "
              f"same neighbour {same * 100:.2f} %, cdist's worst relative error on dist2 {worst_torch:.1e}", flush=True)
        rec["nn"][str(n)] = {"hip_ms": round(med["hip"], 4), "torch_ms": round(med["torch"], 4), "pairs_per_s": pairs,
                             "valu_fraction": pairs * PAIR_OPS / PEAK_FP32, "same_neighbour": same, "cdist_worst_rel": worst_torch, "raw": raw}

        def hip_ch():
            x, y = p[None].detach().requires_grad_(True), q[None].detach().requires_grad_(True)
            chamfer_distance(x, y).sum().backward()
            return x.grad, y.grad

        def torch_ch():
            x, y = p.detach().requires_grad_(True), q.detach().requires_grad_(True)
            torch_chamfer(x, y).backward()
            return x.grad, y.grad

        for _ in range(2):
            hip_ch(); torch_ch()
        torch.cuda.synchronize()
        med, raw = interleaved({"hip": hip_ch, "torch": torch_ch}, a.rounds, reps)
        print(f"chamfer forward+backward N=M={n}: kernel path {med['hip']:.3f} ms | torch {med['torch']:.3f} ms | x{med['torch'] / med['hip']:.1f}", flush=True)
        rec["chamfer"][str(n)] = {"hip_ms": round(med["hip"], 4), "torch_ms": round(med["torch"], 4), "raw": raw}

    # one fitting iteration on the shipped grid, stage by stage (50 000 samples, 50 000 target points)
    tet = np.load(os.path.join(ROOT, "tests", "golden", "64_tets_cropped.npz"))
    geo = DMTetGeometry(64, 2.1, None, tets=(tet["vertices"], tet["indices"]), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(pc.fit_initial_sdf(geo.verts))
    S = 50000
    target = pc.sphere_cloud(S, 0.6, (0.0, 0.0, 0.0), 3).cuda()[None]
    uni = tuple(t.cuda() for t in pc.case_uniforms(1, S, 4))
    opt = torch.optim.Adam([geo.sdf, geo.deform], lr=0.01)
    mesh = geo.getMesh()
    verts, faces = mesh.v_pos.detach(), mesh.t_pos_idx
    pred = sample_points(verts[None], faces, S, uniforms=uni)[0]

    def st_mesh():
        geo.getMesh().v_pos.sum().backward()

    def st_sample():
        v = verts.requires_grad_(True)
        v.grad = None
        sample_points(v[None], faces, S, uniforms=uni)[0].sum().backward()

    def st_sample_torch():
        v = verts.requires_grad_(True)
        v.grad = None
        torch_sample(v, faces, uni).sum().backward()

    def st_chamfer():
        x = pred.detach().requires_grad_(True)
        chamfer_distance(x, target).mean().backward()

    def st_chamfer_torch():
        x = pred[0].detach().requires_grad_(True)
        torch_chamfer(x, target[0]).backward()

    def st_reg():
        m = torch.zeros_like(geo.sdf)
        m[mesh.valid_vert_idx] = 1.0
        (sdf_reg_loss(geo.sdf.detach() * m + geo.sdf * (1 - m), geo.all_edges) * sdf_regularizer_weight(0, 100, 0.2) * 0.1).backward()

    def st_adam():
        opt.step()

    st_mesh(); st_reg()
    stages = {"marching_tets": st_mesh, "sampling": st_sample, "sampling_torch": st_sample_torch, "chamfer": st_chamfer,
              "chamfer_torch": st_chamfer_torch, "regulariser": st_reg, "adam": st_adam}
    for f in stages.values():
        f(); f()
    torch.cuda.synchronize()
    med, raw = interleaved(stages, a.rounds, a.reps)
    ours = sum(med[k] for k in ("marching_tets", "sampling", "chamfer", "regulariser", "adam"))
    print(f"fit iteration (V {verts.shape[0]} F {faces.shape[0]} S {S}): " + " | ".join(f"{k} {v:.3f} ms" for k, v in med.items()) +
          f" | kernel-path total {ours:.3f} ms", flush=True)
    rec["fit"] = {k: round(v, 4) for k, v in med.items()}
    rec["fit"]["total_ms"] = round(ours, 4)
    print(json.dumps({k: ({c: {x: y for x, y in v.items() if x != "raw"} if isinstance(v, dict) else v for c, v in w.items()}
                          if isinstance(w, dict) else w) for k, w in rec.items()}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
