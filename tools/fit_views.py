"""Fit a DMTet grid to a mesh under depth supervision, the way the reference's fit_dmtets.py supervises geometry: `.obj` ->
depth / silhouette targets of --views cameras (rendered with the project's own rasteriser) -> DMTetGeometry fitted with the
depth loss, the SDF regulariser, the silhouette carve, with --alpha_weight the antialiased coverage term, with --color_weight
the colour term of the normal-shaded image and, with --points, the chamfer distance -> the `{'sdf', 'deform'}` dict that `mesh_export.dicts_to_grids` turns into a training grid.

    python tools/fit_views.py --obj shape.obj --tet_path data/tets/64_tets_cropped.npz --views 16 --res 256 --out fitted/dmt_dict_00000.pt
and then `mesh_export.dicts_to_grids(tet_vertices, "fitted", "grids", 64, [0])` writes grids/grid_00000.pt.
    python tools/fit_views.py ... --alpha_weight 1 --color_weight 1 --dump_normals fitted/normals
adds the reference's image terms and writes the normal map of every view after the fit.
    python tools/fit_views.py ... --pass2_iters 500 --out fitted/tets/dmt_dict_00000.pt
adds the reference's second pass (fit_dmtets.py:758-793): the pass-1 dict goes to fitted/tets/tets_pre/dmt_dict_00000.pt, then the
sign of the SDF is frozen, `deform` is fine-tuned on the fixed topology with the umbrella Laplacian
(meshdiffusion_amd.fit.fit_fixed_topology), and --out receives `{'sdf': +-1, 'deform': masked, 'deform_unmasked'}`, the dict
the reference trains its diffusion model on.

The mesh is centred and scaled into the tet grid's volume (largest half-extent -> --fit_scale).  Camera k of N looks at the
origin from distance --cam_radius: perspective(--fovy, 1, 0.1, 1000) @ translate(0, 0, -radius) @ rotate_x(elevation_k) @
rotate_y(2 pi k / N), the elevations alternating between +-0.4.  The loop is meshdiffusion_amd.fit.fit_to_views.  GPU only."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from meshdiffusion_amd import fit
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    fit.add_fit_arguments(ap, iters=2000, out_example="fitted/dmt_dict_00000.pt", pass2_help="> 0: after the fit, this many iterations "
                          "of the fixed-topology second pass; the pass-1 dict goes to tets_pre/ next to --out")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--views_per_iter", type=int, default=4)
    ap.add_argument("--alpha_weight", type=float, default=0.0,
                    help="> 0: add this weight times the antialiased coverage term (the reference's weight is 1.0)")
    ap.add_argument("--color_weight", type=float, default=0.0,
                    help="> 0: add this weight times the colour term of the bsdf == 'normal' image (the reference's weight is 1.0)")
    ap.add_argument("--dump_normals", default=None, metavar="DIR",
                    help="write the final `shaded` view k (the normal map over the antialiased coverage) as DIR/view_<k>.npy")
    ap.add_argument("--sphere_init", type=float, default=0.0, help="start from a sphere of this radius instead of the random SDF")
    ap.add_argument("--mesh_init", action="store_true",
                    help="start from the signed distance of the normalised target at the grid's vertices (meshdist.init_sdf) instead of the random SDF")
    ap.add_argument("--second_stage_deform", type=float, default=None,
                    help="deform_scale of the second pass (default: --deform_scale); deform is rescaled by deform_scale / this")
    a = ap.parse_args(argv)
    if a.mesh_init and a.sphere_init > 0:
        ap.error("--mesh_init and --sphere_init exclude each other")
    if not torch.cuda.is_available():
        raise SystemExit("fit_views.py needs a GPU: the HIP path has no CPU fallback")
    from meshdiffusion_amd import render
    from meshdiffusion_amd.pointcloud import sample_points

    torch.manual_seed(a.seed)
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    v, f = fit.load_normalised_obj(a.obj, a.fit_scale)
    mvp, campos = fit.look_at_cameras(a.views, a.cam_radius, a.fovy, "cuda")
    targets = render.make_targets(v, f, mvp, campos, a.res, antialias=a.alpha_weight > 0, shaded=a.color_weight > 0)
    points = sample_points(v[None], f, a.points, generator=gen)[0][0] if a.points > 0 else None
    geo = fit.make_geometry(a)
    if a.mesh_init:
        from meshdiffusion_amd import meshdist
        meshdist.init_sdf(geo, v, f)
    shared = dict(views_per_iter=a.views_per_iter, generator=gen, target_points=points, num_samples=max(a.points, 1),
                  alpha_weight=a.alpha_weight, color_weight=a.color_weight)
    fit.fit_to_views(geo, targets, a.iters, lr=a.lr, sdf_regularizer=a.sdf_regularizer, callback=fit.progress("depth loss", a.iters), **shared)
    if a.dump_normals:
        os.makedirs(a.dump_normals, exist_ok=True)
        with torch.no_grad():
            mesh = geo.getMesh()
            shaded = render.render_buffers(mesh.v_pos, mesh.t_pos_idx, mvp, campos, a.res)["shaded"].cpu().numpy()
        for k in range(shaded.shape[0]):
            np.save(os.path.join(a.dump_normals, f"view_{k:03d}.npy"), shaded[k])
        print(f"wrote {shaded.shape[0]} views to {a.dump_normals}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.pass2_iters > 0:
        pre = os.path.join(os.path.dirname(os.path.abspath(a.out)), "tets_pre", os.path.basename(a.out))
        second = a.deform_scale if a.second_stage_deform is None else a.second_stage_deform
        geo = fit.second_pass(geo, a, targets, "depth loss", pre_dict=pre, second_deform_scale=second, **shared)
    torch.save(geo.state_to_dict(), a.out)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
