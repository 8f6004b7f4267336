"""Posed images -> a textured mesh: mesh.obj + mesh.mtl + mesh_kd.png and one preview.

    python tools/texture_from_views.py --obj mesh.obj --views views.npz --res 1024 [--fit_iters N] --out dir/

views.npz holds `images` float32 [V,H,W,3] (linear colour in [0, 1]), `viewmask` [V,H,W] (1 on the object), `mvp` [V,4,4] and
`campos` [V,3] (the conventions of meshdiffusion_amd.render).  The texture is baked by projection
(`texture.bake_from_views`: a face atlas at --res, visibility from the mesh's own depth, cos^2 weights, texels no view saw get
--fill), optionally refined by `fit.fit_texture` (Adam on the masked L1 between `render.render_textured` and the images; the
images are then taken as shaded under --light, or as raw colour with --unshaded), and written by `texture.save_textured_obj`.
`preview.png` is `render_textured` of the result at view --preview_view.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from meshdiffusion_amd import fit, mesh_export, render, texture  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--obj", required=True, help="the mesh (v / f lines)")
    ap.add_argument("--views", required=True, help=".npz with images, viewmask, mvp, campos")
    ap.add_argument("--res", type=int, default=1024, help="side of the texture atlas, at most 2048")
    ap.add_argument("--gutter", type=int, default=1, help="texels between a face's texels and its tile's border; dilation steps")
    ap.add_argument("--fill", type=float, nargs=3, default=(0.5, 0.5, 0.5), help="colour of texels no view saw")
    ap.add_argument("--fit_iters", type=int, default=0, help="> 0: refine the baked texture with this many Adam steps")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--unshaded", action="store_true", help="the images hold raw colour: fit and preview without the irradiance")
    ap.add_argument("--preview_view", type=int, default=0)
    ap.add_argument("--out", required=True, help="directory for mesh.obj, mesh.mtl, mesh_kd.png and preview.png")
    a = ap.parse_args(argv)
    dev = torch.device("cuda")
    v, f = mesh_export.load_obj(a.obj)
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    views = np.load(a.views)
    images, viewmask, mvp, campos = (torch.from_numpy(np.asarray(views[k], np.float32)).to(dev) for k in ("images", "viewmask", "mvp", "campos"))
    baked = texture.bake_from_views(verts, faces, images, viewmask, mvp, campos, a.res, gutter=a.gutter, fill=tuple(a.fill))
    tex = baked["tex"]
    seen = float((baked["weight"] > 0).sum()) / max(1.0, float((baked["weight"] >= 0).sum()))
    print(f"baked {faces.shape[0]} faces from {images.shape[0]} views into {a.res} x {a.res}: {100 * seen:.1f} % of the atlas seen")
    if a.fit_iters > 0:
        targets = {"images": images, "viewmask": viewmask, "mvp": mvp, "campos": campos}
        tex, hist = fit.fit_texture(verts, faces, baked["uvs"], baked["uv_idx"], targets, a.res, a.fit_iters, lr=a.lr, init=tex,
                                    shade=not a.unshaded)
        print(f"fit_texture: loss {float(hist['loss'][0]):.5f} -> {float(hist['loss'][-1]):.5f} in {a.fit_iters} iterations")
    os.makedirs(a.out, exist_ok=True)
    paths = texture.save_textured_obj(os.path.join(a.out, "mesh.obj"), verts, faces, baked["uvs"], baked["uv_idx"], tex.clamp(0, 1))
    k = a.preview_view
    with torch.no_grad():
        img = render.render_textured(verts, faces, baked["uvs"], baked["uv_idx"], tex, mvp[k:k + 1], campos[k:k + 1],
                                     tuple(images.shape[1:3]), shade=not a.unshaded)
    mesh_export.save_png(os.path.join(a.out, "preview.png"), img[0, ..., :3])
    print("wrote " + ", ".join(paths) + " and " + os.path.join(a.out, "preview.png"))


if __name__ == "__main__":
    main()
