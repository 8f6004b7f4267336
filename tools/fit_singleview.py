"""Fit a DMTet grid to ONE view of a mesh and write the partial DMTet that conditional generation reads, the way the reference's
fit_singleview.py does: `.obj` + one camera -> RGBD targets of that view (rendered with the project's own rasteriser) ->
DMTetGeometry fitted by `fit.fit_single_view` -> optionally the fixed-topology second pass (`fit.fit_fixed_topology`)
-> the visible-tet labelling (`singleview.single_view_partial`) -> `{'sdf', 'deform', 'vis', 'vis_rast'}` saved with torch.save.

    python tools/fit_singleview.py --obj shape.obj --tet_path data/tets/64_tets_cropped.npz --angle 0.7 --res 256 --out tets/dmtet.pt
    python main_diffusion.py --mode=cond_gen --config=... --config.eval.partial_dmtet_path=tets/dmtet.pt ...

The mesh is centred and scaled into the tet grid's volume (largest half-extent -> --fit_scale).  The camera looks at the origin
from distance --cam_radius: perspective(--fovy, 1, 0.1, 1000) @ translate(0, 0, -radius) @ rotate_x(--elevation) @
rotate_y(--angle).  --radius is the reference's depth_search_range (7 at its 512 x 512; scale it with --res).  GPU only."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from meshdiffusion_amd import fit
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    fit.add_fit_arguments(ap, iters=5000, out_example="tets/dmtet.pt",
                          pass2_help="> 0: this many iterations of the fixed-topology second pass before labelling")
    ap.add_argument("--angle", type=float, default=0.0, help="rotation of the camera around the y axis, radians")
    ap.add_argument("--elevation", type=float, default=-0.4)
    ap.add_argument("--radius", type=int, default=7, help="half-width of the depth window of the visibility pass, pixels (0..15)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fit_singleview.py needs a GPU: the HIP path has no CPU fallback")
    from meshdiffusion_amd import render, singleview
    from meshdiffusion_amd.pointcloud import sample_points

    torch.manual_seed(a.seed)
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    v, f = fit.load_normalised_obj(a.obj, a.fit_scale)
    mvp, campos = fit.look_at_cameras(1, a.cam_radius, a.fovy, "cuda", angle=a.angle, elevation=a.elevation)
    target = render.make_targets(v, f, mvp, campos, a.res, shaded=True)
    points = sample_points(v[None], f, a.points, generator=gen)[0][0] if a.points > 0 else None
    geo = fit.make_geometry(a)
    shared = dict(generator=gen, target_points=points, num_samples=max(a.points, 1))
    fit.fit_single_view(geo, target, a.iters, lr=a.lr, sdf_regularizer=a.sdf_regularizer, gt_mesh=(v, f),
                        callback=fit.progress("depth term", a.iters), **shared)
    if a.pass2_iters > 0:
        geo = fit.second_pass(geo, a, target, "depth term", **shared)
    partial = singleview.single_view_partial(geo, target, radius=a.radius)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save(partial, a.out)
    n = partial["vis"].numel()
    print(f"wrote {a.out}: {n} grid vertices, vis {int(partial['vis'].sum())}, vis_rast {int(partial['vis_rast'].sum())}")


if __name__ == "__main__":
    main()
