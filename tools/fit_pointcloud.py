"""Fit a DMTet grid to a mesh without a renderer: `.obj` -> target points -> DMTetGeometry fitted with the chamfer distance and
the SDF regulariser -> the `{'sdf', 'deform'}` dict that `mesh_export.dicts_to_grids` turns into a training grid.

    python tools/fit_pointcloud.py --obj shape.obj --tet_path data/tets/64_tets_cropped.npz --out fitted/dmt_dict_00000.pt
and then `mesh_export.dicts_to_grids(tet_vertices, "fitted", "grids", 64, [0])` writes grids/grid_00000.pt.

The mesh is centred and scaled into the tet grid's volume (largest half-extent -> --fit_scale); the target is --points samples
of its surface (meshdiffusion_amd.pointcloud.sample_points); the loop is meshdiffusion_amd.fit.fit_to_points.  GPU only."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from meshdiffusion_amd import fit
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    fit.add_fit_arguments(ap, iters=2000, out_example="fitted/dmt_dict_00000.pt", points=50000, points_help="target points and samples per iteration")
    ap.add_argument("--sphere_init", type=float, default=0.0, help="start from a sphere of this radius instead of the random SDF")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fit_pointcloud.py needs a GPU: the HIP path has no CPU fallback")
    from meshdiffusion_amd.pointcloud import sample_points

    torch.manual_seed(a.seed)
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    v, f = fit.load_normalised_obj(a.obj, a.fit_scale)
    target = sample_points(v[None], f, a.points, generator=gen)[0][0]
    geo = fit.make_geometry(a)
    fit.fit_to_points(geo, target, a.iters, num_samples=a.points, lr=a.lr, sdf_regularizer=a.sdf_regularizer, generator=gen,
                      callback=fit.progress("chamfer", a.iters))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save(geo.state_to_dict(), a.out)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
