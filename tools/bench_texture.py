"""What the texture path costs on 32 marching-tetrahedra meshes of the shipped 64 grid (spheres of seeded centre and radius), one
process, per mesh:
  * sample fwd / fwd+bwd : texture.sample at 512 x 512 x 8 views from a 1024 x 1024 x 3 texture (uv and rast of the mesh under
                           `face_atlas`), the backward with a reused SamplePlan, next to torch.nn.functional.grid_sample (bilinear,
                           border, align_corners=False) forward and backward on the same tensors; `plan build` is the one-off cost
                           of the SamplePlan's CSR (md_texture_codes, a stable sort, a searchsorted).
  * project_views, dilate: at 1024 x 1024, 16 views of 512 x 512.
  * fit iteration        : one step of fit.fit_texture's loop (render_textured, masked L1, backward, Adam) on the 8 views, with the
                           SamplePlan reused and with a new one every iteration.
Device events after a warm-up; the variants alternate round by round; per variant the median over the meshes of the per-mesh
median over rounds, with the smallest and largest mesh.
    python tools/bench_texture.py [--meshes 32] [--rounds 3] [--reps 3] [--out profiles/texture_bench.txt]"""
import argparse
import os
import statistics
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
    ap.add_argument("--meshes", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture.py needs a GPU: the HIP path has no CPU fallback")
    import raster_cases as rc
    import texture_cases as tc
    from meshdiffusion_amd import dmtet, render, texture
    dev = torch.device("cuda")
    tv, ti = rc.tet_grid()
    pos = torch.as_tensor(tv, dtype=torch.float32, device=dev) * rc.MESH_SCALE
    tets = torch.as_tensor(ti, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(0)
    mt = dmtet.DMTet()
    R, S, V_SAMPLE, V_BAKE = 1024, 512, 8, 16
    mvp16, cam16 = (x.to(dev) for x in tc.view_cameras(V_BAKE, S))
    mvp8, cam8 = mvp16[::2].contiguous(), cam16[::2].contiguous()
    results, faces_seen = {}, []
    for k in range(a.meshes):
        centre = torch.tensor(rng.uniform(-0.1, 0.1, 3), dtype=torch.float32, device=dev)
        radius = float(rng.uniform(0.5, 0.8))
        verts, faces, *_ = mt(pos, (pos - centre).norm(dim=1) - radius, tets)
        faces_seen.append(faces.shape[0])
        uvs, uv_idx = (x.to(dev) for x in texture.face_atlas(faces.shape[0], R))
        bake = texture.render_uv(verts, faces, uvs, uv_idx, R)
        tex = torch.where(bake["mask"][..., None] > 0.5, tc.smooth_color(bake["pos"]), torch.full_like(bake["pos"], 0.5)).contiguous()
        fixed = render.textured_fixed(verts, faces, uvs, uv_idx, tex.shape, mvp8, cam8, S, shade=False)
        uv, rast, plan = fixed["uv"], fixed["rast"], fixed["plan"]
        plan.csr()
        g = torch.randn(V_SAMPLE, S, S, 3, device=dev)
        tex_g = tex.clone().requires_grad_(True)
        nchw = tex.permute(2, 0, 1)[None].expand(V_SAMPLE, -1, -1, -1)
        nchw_g = tex.permute(2, 0, 1)[None].clone().requires_grad_(True)
        grid = (uv * 2 - 1).contiguous()
        buf = render.render_depth(verts, faces, mvp16, cam16, S)
        images = (tc.smooth_color(render.interpolate(verts, buf["rast"], faces)) * buf["mask"]).contiguous()
        depth, vmask = buf["depth"][..., 0].contiguous(), buf["mask"][..., 0].contiguous()
        target = (images[::2] * 0.9).contiguous()
        vm8 = vmask[::2, ..., None].contiguous()
        norm = 3.0 * vm8.sum()
        fit_tex = tex.clone().requires_grad_(True)
        opt = torch.optim.Adam([fit_tex], lr=1e-3)

        def sample_bwd():
            tex_g.grad = None
            texture.sample(tex_g, uv, rast, plan=plan).backward(g)

        def grid_bwd():
            nchw_g.grad = None
            torch.nn.functional.grid_sample(nchw_g.expand(V_SAMPLE, -1, -1, -1), grid, mode="bilinear", padding_mode="border",
                                            align_corners=False).backward(g.permute(0, 3, 1, 2))

        def fit_iter(reuse):
            fx = fixed if reuse else dict(fixed, plan=texture.SamplePlan(uv, rast, tex.shape))
            opt.zero_grad(set_to_none=True)
            img = render.render_textured(verts, faces, uvs, uv_idx, fit_tex, mvp8, cam8, S, shade=False, _fixed=fx)
            (((img[..., :3] - target).abs() * vm8).sum() / norm).backward()
            opt.step()

        variants = {
            "sample fwd": lambda: texture.sample(tex, uv, rast, plan=plan),
            "grid_sample fwd": lambda: torch.nn.functional.grid_sample(nchw, grid, mode="bilinear", padding_mode="border", align_corners=False),
            "sample fwd+bwd (plan reused)": sample_bwd,
            "grid_sample fwd+bwd": grid_bwd,
            "plan build": lambda: texture.SamplePlan(uv, rast, tex.shape).csr(),
            "project_views 16 views": lambda: texture.project_views(bake, images, depth, vmask, mvp16, cam16),
            "dilate 1 step": lambda: texture.dilate(tex, bake["mask"], 1),
            "fit iteration (plan reused)": lambda: fit_iter(True),
            "fit iteration (new plan)": lambda: fit_iter(False),
        }
        for fn in variants.values():                                            # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        med, _ = interleaved(variants, a.rounds, a.reps)
        for name, ms in med.items():
            results.setdefault(name, []).append(ms)
        # the two fetches agree, so the timing compares like with like.  grid_sample gets 2 u - 1 and maps it back to texels, which
        # moves a fetch by up to 1e-4 texel at 1024; across a tile border, where the atlas jumps, that is a few 1e-5 in the value
        with torch.no_grad():
            ours = texture.sample(tex, uv, rast, plan=plan)
            theirs = variants["grid_sample fwd"]().permute(0, 2, 3, 1) * (rast[..., 3:4] != 0)
        assert float((ours - theirs).abs().max()) < 1e-3
    lines = [f"texture path on {a.meshes} marching-tets meshes ({min(faces_seen)} to {max(faces_seen)} faces), atlas {R} x {R} x 3, "
             f"{V_SAMPLE} views of {S} x {S} sampled, {V_BAKE} views baked; {a.rounds} rounds x {a.reps} reps, device events",
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"{'variant':34s} {'median ms':>10s} {'min':>9s} {'max':>9s}   (per mesh; median / extremes over the meshes)"]
    for name, ms in results.items():
        lines.append(f"{name:34s} {statistics.median(ms):10.3f} {min(ms):9.3f} {max(ms):9.3f}")
    px = V_SAMPLE * S * S
    fwd = statistics.median(results["sample fwd"])
    lines.append(f"sample fwd moves at least uv 8 B + rast 16 B + out 12 B per pixel = {px * 36 / 1e6:.1f} MB: {px * 36 / fwd / 1e6:.1f} GB/s "
                 f"of compulsory traffic (texel reads come on top, mostly from cache)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
