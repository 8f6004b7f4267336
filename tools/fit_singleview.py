"""Fit a DMTet grid to ONE view of a mesh and write the partial DMTet that conditional generation reads, the way the reference's
fit_singleview.py does: `.obj` + one camera -> RGBD targets of that view (rendered with the project's own rasteriser) ->
DMTetGeometry fitted by `singleview.fit_single_view` -> optionally the fixed-topology second pass (`render.fit_fixed_topology`)
-> the visible-tet labelling (`singleview.single_view_partial`) -> `{'sdf', 'deform', 'vis', 'vis_rast'}` saved with torch.save.

    python tools/fit_singleview.py --obj shape.obj --tet_path data/tets/64_tets_cropped.npz --angle 0.7 --res 256 --out tets/dmtet.pt
    python main_diffusion.py --mode=cond_gen --config=... --config.eval.partial_dmtet_path=tets/dmtet.pt ...

The mesh is centred and scaled into the tet grid's volume (largest half-extent -> --fit_scale).  The camera looks at the origin
from distance --cam_radius: perspective(--fovy, 1, 0.1, 1000) @ translate(0, 0, -radius) @ rotate_x(--elevation) @
rotate_y(--angle).  --radius is the reference's depth_search_range (7 at its 512 x 512; scale it with --res).  GPU only."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--obj", required=True, help="triangle mesh to fit")
    ap.add_argument("--tet_path", required=True, help="<R>_tets_cropped.npz (vertices, indices)")
    ap.add_argument("--out", required=True, help="path of the dict to write, e.g. tets/dmtet.pt")
    ap.add_argument("--angle", type=float, default=0.0, help="rotation of the camera around the y axis, radians")
    ap.add_argument("--elevation", type=float, default=-0.4)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--resolution", type=int, default=64, help="resolution of the tet grid")
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--sdf_regularizer", type=float, default=0.2)
    ap.add_argument("--points", type=int, default=0, help="> 0: add the chamfer term with this many target points and samples")
    ap.add_argument("--radius", type=int, default=7, help="half-width of the depth window of the visibility pass, pixels (0..15)")
    ap.add_argument("--mesh_scale", type=float, default=2.1)
    ap.add_argument("--deform_scale", type=float, default=2.0)
    ap.add_argument("--fit_scale", type=float, default=0.8, help="largest half-extent of the normalised target")
    ap.add_argument("--cam_radius", type=float, default=3.0)
    ap.add_argument("--fovy", type=float, default=math.radians(45.0))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pass2_iters", type=int, default=0, help="> 0: this many iterations of the fixed-topology second pass before labelling")
    ap.add_argument("--pass2_lr", type=float, default=0.01)
    ap.add_argument("--laplace_scale", type=float, default=10000.0)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fit_singleview.py needs a GPU: the HIP path has no CPU fallback")
    from meshdiffusion_amd import mesh_export, render, singleview
    from meshdiffusion_amd.dmtet import DMTetGeometry, DMTetGeometryFixedTopo
    from meshdiffusion_amd.pointcloud import sample_points

    torch.manual_seed(a.seed)
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    verts, faces = mesh_export.load_obj(a.obj)
    v = torch.as_tensor(verts, dtype=torch.float32).cuda()
    f = torch.as_tensor(faces).cuda()
    lo, hi = v.min(0).values, v.max(0).values
    v = (v - (lo + hi) / 2) * (a.fit_scale / float((hi - lo).max() / 2))
    mv = render.translate(0, 0, -a.cam_radius) @ render.rotate_x(a.elevation) @ render.rotate_y(a.angle)
    mvp = (render.perspective(a.fovy, 1.0, 0.1, 1000.0) @ mv)[None].cuda()
    campos = torch.linalg.inv(mv)[:3, 3][None].cuda()
    target = render.make_targets(v, f, mvp, campos, a.res, shaded=True)
    points = sample_points(v[None], f, a.points, generator=gen)[0][0] if a.points > 0 else None
    tet = np.load(a.tet_path)
    geo = DMTetGeometry(a.resolution, a.mesh_scale, None, tets=(tet["vertices"], tet["indices"]), deform_scale=a.deform_scale)

    def report(it, loss, mesh):
        if it % 100 == 0 or it == a.iters - 1:
            print(f"iter {it}: depth term {float(loss):.6f}  V {mesh.v_pos.shape[0]} F {mesh.t_pos_idx.shape[0]}", flush=True)

    singleview.fit_single_view(geo, target, a.iters, lr=a.lr, sdf_regularizer=a.sdf_regularizer, target_points=points,
                               gt_mesh=(v, f), num_samples=max(a.points, 1), generator=gen, callback=report)
    if a.pass2_iters > 0:
        fixed = DMTetGeometryFixedTopo(geo, a.resolution, a.mesh_scale, deform_scale=a.deform_scale)
        fixed.set_init_v_pos()

        def report2(it, loss, mesh):
            if it % 100 == 0 or it == a.pass2_iters - 1:
                print(f"pass 2 iter {it}: depth term {float(loss):.6f}  V {mesh.v_pos.shape[0]} F {mesh.t_pos_idx.shape[0]}", flush=True)

        render.fit_fixed_topology(fixed, target, a.pass2_iters, lr=a.pass2_lr, laplace_scale=a.laplace_scale, generator=gen,
                                  target_points=points, num_samples=max(a.points, 1), callback=report2)
        geo = fixed
    partial = singleview.single_view_partial(geo, target, radius=a.radius)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save(partial, a.out)
    n = partial["vis"].numel()
    print(f"wrote {a.out}: {n} grid vertices, vis {int(partial['vis'].sum())}, vis_rast {int(partial['vis_rast'].sum())}")


if __name__ == "__main__":
    main()
