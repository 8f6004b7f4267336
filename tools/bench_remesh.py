"""What the isotropic remeshing costs for the 32 meshes of one marching-tetrahedra launch on the shipped 64 grid, one process:
postprocess.remesh(iters=3) on the concatenated batch, pass by pass.  The passes are driven here through the same public round
functions `remesh` calls, with the device synchronised around each, so the times are wall-clock milliseconds per pass; the torch
glue is timed by wrapping the table builder (`_remesh_tables`: two sorts, a unique and two searches per launch group) -- what is
left of a pass is its kernels, the 4-byte counter read and the compaction.  The meshes: the sign of a sphere per sample (radii
0.2 .. 0.45 of the grid, all closed) with a seeded uniform deformation in [-0.9, 0.9] of every tet-grid vertex, which gives the
short edges and slivers of a sampled mesh.  There is no parent to compare against: the figure is recorded, not barred.
    python tools/bench_remesh.py [--iters 3] [--meshes 32] [--out profiles/remesh_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Clock:
    def __init__(self):
        self.ms = {}

    def run(self, key, fn, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*args)
        torch.cuda.synchronize()
        self.ms[key] = self.ms.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--meshes", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the report there (profiles/remesh_bench.txt)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_remesh.py needs a GPU: the HIP path has no CPU fallback")
    import raster_cases as rc
    import remesh_cases as rm
    from meshdiffusion_amd import _lib, postprocess
    from meshdiffusion_amd.dmtet import GridMesher

    R = 64
    k = (torch.arange(R, dtype=torch.float32) + 0.5) / R - 0.5
    z, y, xg = torch.meshgrid(k, k, k, indexing="ij")
    samples = np.zeros((a.meshes, 4, R, R, R), np.float32)
    for m in range(a.meshes):
        samples[m, 0] = torch.sign(torch.sqrt(xg * xg + y * y + z * z) - (0.2 + 0.25 * m / max(a.meshes - 1, 1))).numpy()
    samples[:, 1:] = np.random.default_rng(0).uniform(-0.9, 0.9, samples[:, 1:].shape).astype(np.float32)
    tv, ti = rc.tet_grid()
    meshes = [(v.clone(), f.clone()) for v, f, _ in GridMesher(tv, ti, 64)(torch.from_numpy(samples))]
    verts, faces, vert_mesh = postprocess.concat_meshes(meshes)
    M = a.meshes
    lines = [f"{M} marching-tets meshes, concatenated: V {verts.shape[0]} F {faces.shape[0]}; remesh(iters={a.iters}), target = each mesh's mean "
             f"edge length, relax 0.5, flip angle 30 degrees"]

    def whole():
        return postprocess.remesh(verts, faces, iters=a.iters, vert_mesh=vert_mesh)

    whole()                                                              # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, f, vm, info = whole()
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    again = whole()
    same = all(torch.equal(p, q) for p, q in zip((x, f, vm), again[:3]))

    # the same passes, timed one by one
    clock, glue = Clock(), Clock()
    build = postprocess._remesh_tables
    postprocess._remesh_tables = lambda *args: glue.run(clock.key, build, *args)
    target = postprocess.remesh_default_target(verts, faces, vert_mesh, M)
    lo2, hi2 = (torch.as_tensor(t).cuda() for t in postprocess.remesh_bands(target))
    cos2 = float(rm.cos2_of(30.0))
    sx, sf, svm = verts.clone(), faces.clone(), vert_mesh.clone()
    for _ in range(a.iters):
        clock.key = "split"
        sx, sf, svm, _n = clock.run("split", postprocess.remesh_split, sx, sf, svm, hi2)
        clock.key = "collapse"
        for _r in range(_lib.REMESH_COLLAPSE_ROUNDS):
            sx, sf, svm, n = clock.run("collapse", postprocess.remesh_collapse_round, sx, sf, svm, lo2, hi2)
            if n == 0:
                break
        clock.key = "flip"
        for _r in range(_lib.REMESH_FLIP_ROUNDS):
            sf, n = clock.run("flip", postprocess.remesh_flip_round, sx, sf, cos2)
            if n == 0:
                break
        clock.key = "relax"
        sx = clock.run("relax", postprocess.remesh_relax, sx, sf, 0.5)
    postprocess._remesh_tables = build
    stepwise = torch.equal(sx, x) and torch.equal(sf, f)

    xn, fn = x.cpu().numpy(), f.cpu().numpy()
    L = float(np.mean(info["target"]))
    q0, q1 = rm.quality(verts.cpu().numpy(), faces.cpu().numpy(), L), rm.quality(xn, fn, L)
    bad0, bad = rm.problems(faces.cpu().numpy(), verts.shape[0]), rm.problems(fn, xn.shape[0])
    lines.append(f"whole call: {total:.1f} ms wall clock ({total / M:.2f} ms per mesh); V {verts.shape[0]} -> {x.shape[0]} F {faces.shape[0]} -> "
                 f"{f.shape[0]}; two runs equal: {same}; pass by pass gives the same mesh: {stepwise}")
    for r, rec in enumerate(info["iterations"]):
        lines.append(f"  iteration {r}: splits {rec['splits']} collapses {rec['collapses']} in {rec['collapse_rounds']} rounds, flips {rec['flips']} "
                     f"in {rec['flip_rounds']} rounds")
    sum_pass, sum_glue = sum(clock.ms.values()), sum(glue.ms.values())
    for key in ("split", "collapse", "flip", "relax"):
        lines.append(f"  {key:8s} {clock.ms[key]:8.1f} ms over {a.iters} iterations, of which the table builder (torch) {glue.ms[key]:8.1f} ms "
                     f"({100 * glue.ms[key] / clock.ms[key]:.0f} %)")
    lines.append(f"  torch glue share (table builder only): {100 * sum_glue / sum_pass:.0f} % of {sum_pass:.1f} ms synchronised pass time")
    lines.append(f"band share (at the mean target {L:.4f}) {q0[0]:.3f} -> {q1[0]:.3f}, minimum angle {q0[1]:.1f} -> {q1[1]:.1f} degrees; closed-manifold "
                 f"problems before: {bad0[:3] if bad0 else 'none'}, after: {bad[:3] if bad else 'none'}")
    lines.append("measured on one MI355X: python tools/bench_remesh.py --out profiles/remesh_bench.txt (one timed call after one warm-up call; "
                 "wall clock with the device synchronised)")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
