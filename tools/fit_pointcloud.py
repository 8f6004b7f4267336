"""Fit a DMTet grid to a mesh without a renderer: `.obj` -> target points -> DMTetGeometry fitted with the chamfer distance and
the SDF regulariser -> the `{'sdf', 'deform'}` dict that `mesh_export.dicts_to_grids` turns into a training grid.

    python tools/fit_pointcloud.py --obj shape.obj --tet_path data/tets/64_tets_cropped.npz --out fitted/dmt_dict_00000.pt
and then `mesh_export.dicts_to_grids(tet_vertices, "fitted", "grids", 64, [0])` writes grids/grid_00000.pt.

The mesh is centred and scaled into the tet grid's volume (largest half-extent -> --fit_scale); the target is --points samples
of its surface (meshdiffusion_amd.pointcloud.sample_points); the loop is meshdiffusion_amd.pointcloud.fit_to_points.  GPU only."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--obj", required=True, help="triangle mesh to fit")
    ap.add_argument("--tet_path", required=True, help="<R>_tets_cropped.npz (vertices, indices)")
    ap.add_argument("--out", required=True, help="path of the dict to write, e.g. fitted/dmt_dict_00000.pt")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--points", type=int, default=50000, help="target points and samples per iteration")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--sdf_regularizer", type=float, default=0.2)
    ap.add_argument("--mesh_scale", type=float, default=2.1)
    ap.add_argument("--deform_scale", type=float, default=2.0)
    ap.add_argument("--fit_scale", type=float, default=0.8, help="largest half-extent of the normalised target")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sphere_init", type=float, default=0.0, help="start from a sphere of this radius instead of the random SDF")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fit_pointcloud.py needs a GPU: the HIP path has no CPU fallback")
    from meshdiffusion_amd import mesh_export
    from meshdiffusion_amd.dmtet import DMTetGeometry
    from meshdiffusion_amd.pointcloud import fit_to_points, sample_points

    torch.manual_seed(a.seed)
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    verts, faces = mesh_export.load_obj(a.obj)
    v = torch.as_tensor(verts).cuda()
    lo, hi = v.min(0).values, v.max(0).values
    v = (v - (lo + hi) / 2) * (a.fit_scale / float((hi - lo).max() / 2))
    target = sample_points(v[None], torch.as_tensor(faces).cuda(), a.points, generator=gen)[0][0]
    tet = np.load(a.tet_path)
    geo = DMTetGeometry(a.resolution, a.mesh_scale, None, tets=(tet["vertices"], tet["indices"]), deform_scale=a.deform_scale)
    if a.sphere_init > 0:
        with torch.no_grad():
            geo.sdf.copy_((a.sphere_init - geo.verts.norm(dim=1)).clamp(-1.0, 1.0))

    def report(it, chamfer, mesh):
        if it % 100 == 0 or it == a.iters - 1:
            print(f"iter {it}: chamfer {float(chamfer):.6f}  V {mesh.v_pos.shape[0]} F {mesh.t_pos_idx.shape[0]}", flush=True)

    fit_to_points(geo, target, a.iters, num_samples=a.points, lr=a.lr, sdf_regularizer=a.sdf_regularizer, generator=gen,
                  callback=report)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save(geo.state_to_dict(), a.out)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
