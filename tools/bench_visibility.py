"""Visible-tet labelling on the shipped 64 grid at 512 x 512, r = 7, one view, one process:
  * hip path   : singleview.window_min_depth + visible_tets + label_vertices (csrc/visibility.hip; the window minimum is computed
                 twice, once by each of the first two calls, as a caller of the three functions pays for it);
  * torch path : the reference's formulation on the same GPU, the restatements of tests/visibility_cases.py: two max_pool2d calls,
                 the gathers, `unique` and indexed stores.
The sphere of radius 0.7 is meshed on the grid and rasterised once; both paths start from that `rast`.  Device events after
warm-up; the variants alternate round by round and each figure is the median over rounds.  The outputs are compared first.
    python tools/bench_visibility.py [--res 512] [--radius 7] [--rounds 7] [--reps 10] [--out profiles/visibility_bench.txt]"""
import argparse
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
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--radius", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visibility.py needs a GPU: the HIP path has no CPU fallback")
    import raster_cases as rc
    import visibility_cases as vc
    from meshdiffusion_amd import dmtet, render, singleview as sv

    geo = dmtet.DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(geo.verts.norm(dim=1) - 0.7)
        mesh = geo.getMesh()
        mvp = rc.cameras((rc.ANGLES[0],), a.res, a.res)[0].cuda()
        rast = render.rasterize(render.xfm_points(mesh.v_pos[None], mvp).contiguous(), mesh.t_pos_idx, a.res, num_layers=1)[0]
        centres = geo.getTetCenters().detach().contiguous()
        face_tet, indices, N = geo.getValidTetIdx(), geo.indices, geo.verts.shape[0]

    def hip_path():
        dmin = sv.window_min_depth(rast, a.radius)
        visible = sv.visible_tets(rast, centres, mvp, a.radius)
        return (dmin, visible) + sv.label_vertices(visible, rast, face_tet, indices, N)

    def torch_path():
        dmin = vc.window_min_restated(rast, a.radius)
        visible = vc.visible_tets_restated(rast, centres, mvp, a.radius)
        return (dmin, visible) + vc.label_vertices_restated(visible, rast, face_tet, indices, N)

    got, want = hip_path(), torch_path()
    differ = [int((g != w).sum()) for g, w in zip(got, want)]
    for _ in range(2):
        hip_path(); torch_path()
    torch.cuda.synchronize()
    med, raw = interleaved({"hip": hip_path, "torch": torch_path}, a.rounds, a.reps)
    lines = [f"visible-tet labelling, {a.res} x {a.res}, r = {a.radius}, 1 view, T {centres.shape[0]} tets, N {N} vertices, F "
             f"{face_tet.shape[0]} faces, covered pixels {int((rast[..., 3] > 0).sum())}",
             f"  hip path (window_min_depth + visible_tets + label_vertices): {med['hip']:.3f} ms per call",
             f"  torch path (the reference's formulation, same GPU, same process): {med['torch']:.3f} ms per call",
             f"  torch / hip: x{med['torch'] / med['hip']:.2f}; median of {a.rounds} interleaved rounds of {a.reps} calls",
             f"  rounds, ms: hip {[round(x, 3) for x in raw['hip']]} torch {[round(x, 3) for x in raw['torch']]}",
             f"  elements differing between the paths (Dmin, visible, vis, vis_rast): {differ}; visible tets {int(got[1].sum())}, vis "
             f"{int(got[2].sum())}, vis_rast {int(got[3].sum())}"]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
