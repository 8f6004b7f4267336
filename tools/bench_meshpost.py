"""What the mesh post-processing costs for the 32 meshes of one marching-tetrahedra launch on the shipped 64 grid, one process:
  * postprocess     : postprocess.postprocess(keep_largest=True, smooth_steps=3) -- md_mesh_components, the torch compaction, the
                      edge table, md_mesh_smooth -- against the same steps as plain torch ops on the device: label propagation by
                      scatter_reduce(amin) over the face corners until nothing changes (one host read per sweep), the same
                      compaction, and the umbrella step as index_add over the directed edges.
  * render_preview  : render.render_preview at 512 x 512 per mesh -- rasterize, md_shade_diffuse, antialias, composite, sRGB --
                      against the same with the shading as elementwise torch ops (the rasteriser and the antialiasing have no torch
                      form and are shared).
The meshes: the sign of a sphere plus a far-away blob per sample, with a seeded 0.05 % of the voxels' signs flipped, the kind of
floaters a sampled SDF leaves.  Device events after warm-up; the variants alternate round by round, medians over rounds.
    python tools/bench_meshpost.py [--rounds 5] [--reps 3] [--out profiles/meshpost_bench.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pc import interleaved  # noqa: E402


def torch_components(faces, V):
    label = torch.arange(V, dtype=torch.int64, device=faces.device)
    sweeps = 0
    while True:
        sweeps += 1
        m = label[faces].amin(1, keepdim=True).expand(-1, 3).reshape(-1)
        new = label.scatter_reduce(0, faces.reshape(-1), m, "amin", include_self=True)
        new = new[new]
        if torch.equal(new, label):
            return label, sweeps
        label = new


def torch_keep_largest(verts, faces, vert_mesh, label):
    V = verts.shape[0]
    vm = vert_mesh.to(torch.int64)
    cf = torch.bincount(label[faces[:, 0]], minlength=V)
    M = int(vm.max()) + 1
    largest = torch.zeros(M, dtype=torch.int64, device=verts.device).scatter_reduce(0, vm, cf, "amax", include_self=True)
    idx = torch.arange(V, device=verts.device)
    cand = torch.where((cf == largest[vm]) & (cf >= 1), idx, torch.full_like(idx, V))
    winner = torch.full((M,), V, dtype=torch.int64, device=verts.device).scatter_reduce(0, vm, cand, "amin", include_self=True)
    keep = (idx == winner[vm])[label]
    fk = keep[faces[:, 0]]
    vmap = torch.cumsum(keep.to(torch.int64), 0) - 1
    return verts[keep], vmap[faces[fk]], vert_mesh[keep]


def torch_smooth(verts, lo, hi, mult, steps, lam):
    V = verts.shape[0]
    bnd = mult == 1
    is_b = torch.zeros(V, dtype=torch.bool, device=verts.device)
    is_b[lo[bnd]] = True
    is_b[hi[bnd]] = True
    row, nbr, eb = torch.cat([lo, hi]), torch.cat([hi, lo]), torch.cat([bnd, bnd])
    use = ~is_b[row] | eb
    row, nbr = row[use], nbr[use]
    n = torch.bincount(row, minlength=V).to(verts.dtype)[:, None]
    x = verts
    for _ in range(steps):
        m = torch.zeros_like(x).index_add(0, row, x[nbr]) / n.clamp_min(1)
        x = torch.where(n > 0, x + lam * (m - x), x)
    return x


def torch_shade(rast, verts, faces, campos, sh, kd):
    F = faces.shape[0]
    cov = (rast[..., 3] >= 1) & (rast[..., 3] <= F)
    t3 = faces[(rast[..., 3].to(torch.int64) - 1).clamp(0, F - 1)]
    p0, p1, p2 = verts[t3[..., 0]], verts[t3[..., 1]], verts[t3[..., 2]]
    u, v = rast[..., 0:1], rast[..., 1:2]
    p = (u * p0 + v * p1) + ((1 - u) - v) * p2
    g = torch.linalg.cross(p1 - p0, p2 - p0)
    geo = g / torch.sqrt(torch.clamp((g * g).sum(-1, keepdim=True), min=1e-20))
    d = campos[:, None, None, :] - p
    view = d / torch.clamp(torch.sqrt((d * d).sum(-1, keepdim=True)), min=1e-12)
    n = torch.where((geo * view).sum(-1, keepdim=True) > 0, geo, -geo)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    Y = torch.stack([torch.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                     0.315392 * (3 * z * z - 1), 1.092548 * x * z, 0.546274 * (x * x - y * y)], -1)
    A = torch.tensor([1.0, 2 / 3, 2 / 3, 2 / 3, 0.25, 0.25, 0.25, 0.25, 0.25], device=rast.device)
    rgb = kd * torch.clamp((Y * A) @ sh, min=0)
    out = torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1)
    return torch.where(cov[..., None], out, torch.zeros_like(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--meshes", type=int, default=32)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the report there (profiles/meshpost_bench.txt)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshpost.py needs a GPU: the HIP path has no CPU fallback")
    import meshpost_cases as mc
    import raster_cases as rc
    from meshdiffusion_amd import postprocess, render
    from meshdiffusion_amd.dmtet import GridMesher

    samples = mc.sphere_and_blob_samples(M=a.meshes)
    flip = np.random.default_rng(0).random(samples[:, 0].shape) < 5e-4
    samples[:, 0] = np.where(flip, -samples[:, 0], samples[:, 0])
    tv, ti = rc.tet_grid()
    meshes = [(v.clone(), f.clone()) for v, f, _ in GridMesher(tv, ti, 64)(torch.from_numpy(samples))]
    verts, faces, vert_mesh = postprocess.concat_meshes(meshes)
    V, F = verts.shape[0], faces.shape[0]
    label, cf, rounds = postprocess.components(faces, V)
    n_comp = int((label == torch.arange(V, device=label.device)).sum())
    lines = [f"{a.meshes} marching-tets meshes, concatenated: V {V} F {F}, {n_comp} components, hook-and-compress rounds {rounds}"]

    def hip_post():
        return postprocess.postprocess(meshes, smooth_steps=3, keep_largest=True)

    def torch_post():
        lab, _ = torch_components(faces, V)
        v2, f2, vm2 = torch_keep_largest(verts, faces, vert_mesh, lab)
        a2, b2 = f2[:, [1, 2, 0]].reshape(-1), f2[:, [2, 0, 1]].reshape(-1)
        keys, mult = torch.unique(torch.minimum(a2, b2) * v2.shape[0] + torch.maximum(a2, b2), return_counts=True)
        x = torch_smooth(v2, torch.div(keys, v2.shape[0], rounding_mode="floor"), keys % v2.shape[0], mult, 3, 0.5)
        return postprocess.split_meshes(x, f2, vm2, a.meshes)

    got, want = hip_post(), torch_post()
    sweeps = torch_components(faces, V)[1]
    same_faces = all(torch.equal(g[1], w[1]) for g, w in zip(got, want))
    dist = rc.rel_l2(torch.cat([g[0] for g in got]), torch.cat([w[0] for w in want]))
    mvp, campos = render.preview_camera(0, a.res, device="cuda")
    light, kd = torch.as_tensor(render.default_light()).cuda(), torch.tensor(render.PREVIEW_KD).cuda()

    def hip_preview():
        return [render.render_preview(v, f, mvp, campos, a.res) for v, f in meshes]

    def torch_preview():
        out = []
        bg = torch.ones(3, device="cuda")
        for v, f in meshes:
            clip = render.xfm_points(v[None], mvp).contiguous()
            rast = render.rasterize(clip, f, a.res, num_layers=1)[0]
            col = render.antialias(torch_shade(rast, v, f, campos, light, kd), rast, clip, f)
            out.append(torch.clamp(render._tonemap_srgb(col[..., :3] + (1 - col[..., 3:]) * bg), 0, 1))
        return out

    img_dist = max(float((x - y).abs().max()) for x, y in zip(hip_preview(), torch_preview()))
    torch.cuda.synchronize()
    med, _ = interleaved({"hip_post": hip_post, "torch_post": torch_post, "hip_preview": hip_preview, "torch_preview": torch_preview},
                         a.rounds, a.reps)
    lines += [f"postprocess(keep_largest, 3 smoothing steps), whole batch: HIP {med['hip_post']:.3f} ms | plain torch "
              f"{med['torch_post']:.3f} ms ({sweeps} label sweeps) | x{med['torch_post'] / med['hip_post']:.2f}; faces equal: {same_faces}, "
              f"vertices differ by rel-L2 {dist:.1e}",
              f"render_preview {a.res} x {a.res}, {a.meshes} meshes one by one: HIP shading {med['hip_preview']:.3f} ms | torch shading "
              f"{med['torch_preview']:.3f} ms | x{med['torch_preview'] / med['hip_preview']:.2f}; largest pixel difference {img_dist:.1e}",
              f"medians of {a.rounds} rounds x {a.reps} calls, variants alternating; device events after warm-up"]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
