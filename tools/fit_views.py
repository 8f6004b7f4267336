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
(meshdiffusion_amd.render.fit_fixed_topology), and --out receives `{'sdf': +-1, 'deform': masked, 'deform_unmasked'}`, the dict
the reference trains its diffusion model on.

The mesh is centred and scaled into the tet grid's volume (largest half-extent -> --fit_scale).  Camera k of N looks at the
origin from distance --cam_radius: perspective(--fovy, 1, 0.1, 1000) @ translate(0, 0, -radius) @ rotate_x(elevation_k) @
rotate_y(2 pi k / N), the elevations alternating between +-0.4.  The loop is meshdiffusion_amd.render.fit_to_views.  GPU only."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def orbit_cameras(n, radius, fovy, device):
    """(mvp [n,4,4], campos [n,3]) of n cameras around the y axis."""
    from meshdiffusion_amd import render
    proj = render.perspective(fovy, 1.0, 0.1, 1000.0)
    mvps, cams = [], []
    for k in range(n):
        mv = render.translate(0, 0, -radius) @ render.rotate_x(-0.4 if k % 2 == 0 else 0.4) @ render.rotate_y(2 * math.pi * k / n)
        mvps.append(proj @ mv)
        cams.append(torch.linalg.inv(mv)[:3, 3])
    return torch.stack(mvps).to(device), torch.stack(cams).to(device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--obj", required=True, help="triangle mesh to fit")
    ap.add_argument("--tet_path", required=True, help="<R>_tets_cropped.npz (vertices, indices)")
    ap.add_argument("--out", required=True, help="path of the dict to write, e.g. fitted/dmt_dict_00000.pt")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views_per_iter", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=64, help="resolution of the tet grid")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--sdf_regularizer", type=float, default=0.2)
    ap.add_argument("--points", type=int, default=0, help="> 0: add the chamfer term with this many target points and samples")
    ap.add_argument("--alpha_weight", type=float, default=0.0,
                    help="> 0: add this weight times the antialiased coverage term (the reference's weight is 1.0)")
    ap.add_argument("--color_weight", type=float, default=0.0,
                    help="> 0: add this weight times the colour term of the bsdf == 'normal' image (the reference's weight is 1.0)")
    ap.add_argument("--dump_normals", default=None, metavar="DIR",
                    help="write the final `shaded` view k (the normal map over the antialiased coverage) as DIR/view_<k>.npy")
    ap.add_argument("--mesh_scale", type=float, default=2.1)
    ap.add_argument("--deform_scale", type=float, default=2.0)
    ap.add_argument("--fit_scale", type=float, default=0.8, help="largest half-extent of the normalised target")
    ap.add_argument("--cam_radius", type=float, default=3.0)
    ap.add_argument("--fovy", type=float, default=math.radians(45.0))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sphere_init", type=float, default=0.0, help="start from a sphere of this radius instead of the random SDF")
    ap.add_argument("--mesh_init", action="store_true",
                    help="start from the signed distance of the normalised target at the grid's vertices (meshdist.init_sdf) instead of the random SDF")
    ap.add_argument("--pass2_iters", type=int, default=0,
                    help="> 0: after the fit, this many iterations of the fixed-topology second pass; the pass-1 dict goes to tets_pre/ next to --out")
    ap.add_argument("--pass2_lr", type=float, default=0.01)
    ap.add_argument("--laplace_scale", type=float, default=10000.0)
    ap.add_argument("--second_stage_deform", type=float, default=None,
                    help="deform_scale of the second pass (default: --deform_scale); deform is rescaled by deform_scale / this")
    a = ap.parse_args(argv)
    if a.mesh_init and a.sphere_init > 0:
        ap.error("--mesh_init and --sphere_init exclude each other")
    if not torch.cuda.is_available():
        raise SystemExit("fit_views.py needs a GPU: the HIP path has no CPU fallback")
    from meshdiffusion_amd import mesh_export, render
    from meshdiffusion_amd.dmtet import DMTetGeometry
    from meshdiffusion_amd.pointcloud import sample_points

    torch.manual_seed(a.seed)
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    verts, faces = mesh_export.load_obj(a.obj)
    v = torch.as_tensor(verts, dtype=torch.float32).cuda()
    f = torch.as_tensor(faces).cuda()
    lo, hi = v.min(0).values, v.max(0).values
    v = (v - (lo + hi) / 2) * (a.fit_scale / float((hi - lo).max() / 2))
    mvp, campos = orbit_cameras(a.views, a.cam_radius, a.fovy, "cuda")
    targets = render.make_targets(v, f, mvp, campos, a.res, antialias=a.alpha_weight > 0, shaded=a.color_weight > 0)
    points = sample_points(v[None], f, a.points, generator=gen)[0][0] if a.points > 0 else None
    tet = np.load(a.tet_path)
    geo = DMTetGeometry(a.resolution, a.mesh_scale, None, tets=(tet["vertices"], tet["indices"]), deform_scale=a.deform_scale)
    if a.sphere_init > 0:
        with torch.no_grad():
            geo.sdf.copy_((a.sphere_init - geo.verts.norm(dim=1)).clamp(-1.0, 1.0))
    if a.mesh_init:
        from meshdiffusion_amd import meshdist
        meshdist.init_sdf(geo, v, f)

    def report(it, loss, mesh):
        if it % 100 == 0 or it == a.iters - 1:
            print(f"iter {it}: depth loss {float(loss):.6f}  V {mesh.v_pos.shape[0]} F {mesh.t_pos_idx.shape[0]}", flush=True)

    render.fit_to_views(geo, targets, a.iters, lr=a.lr, sdf_regularizer=a.sdf_regularizer, views_per_iter=a.views_per_iter,
                        generator=gen, target_points=points, num_samples=max(a.points, 1), callback=report,
                        alpha_weight=a.alpha_weight, color_weight=a.color_weight)
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
        from meshdiffusion_amd.dmtet import DMTetGeometryFixedTopo
        pre = os.path.join(os.path.dirname(os.path.abspath(a.out)), "tets_pre", os.path.basename(a.out))
        os.makedirs(os.path.dirname(pre), exist_ok=True)
        torch.save(geo.state_to_dict(), pre)
        print(f"wrote {pre}")
        second = a.deform_scale if a.second_stage_deform is None else a.second_stage_deform
        fixed = DMTetGeometryFixedTopo(geo, a.resolution, a.mesh_scale, deform_scale=second)
        with torch.no_grad():
            fixed.deform.data[:] = fixed.deform * a.deform_scale / second        # fit_dmtets.py:770
        fixed.set_init_v_pos()

        def report2(it, loss, mesh):
            if it % 100 == 0 or it == a.pass2_iters - 1:
                print(f"pass 2 iter {it}: depth loss {float(loss):.6f}  V {mesh.v_pos.shape[0]} F {mesh.t_pos_idx.shape[0]}", flush=True)

        render.fit_fixed_topology(fixed, targets, a.pass2_iters, lr=a.pass2_lr, laplace_scale=a.laplace_scale,
                                  views_per_iter=a.views_per_iter, generator=gen, target_points=points,
                                  num_samples=max(a.points, 1), callback=report2, alpha_weight=a.alpha_weight,
                                  color_weight=a.color_weight)
        geo = fixed
    torch.save(geo.state_to_dict(), a.out)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
