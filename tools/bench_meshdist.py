"""What the mesh distance (csrc/meshdist.hip) costs, one process:
  (a) md_mesh_query at Q = the vertices of a tet grid against T = 9024 (uv_sphere(48, 96)) and T ~ 100k (uv_sphere(160, 320))
      triangles, in three forms: closest point only, winding number only, both in one launch -- device events around `--calls`
      back-to-back calls after a warm-up, the median of `--repeats` such windows;
  (b) the baseline: the same arithmetic as chunked plain torch on the GPU in the same process (on the first `--baseline_queries`
      queries: at 100k triangles the whole grid would take minutes), compared by its rate in pair tests per second;
  (c) the re-projection's share of postprocess.remesh(iters=3, project=True) on the 32 marching-tets meshes of tools/bench_remesh.py;
  (d) with --fit_iters N: tools/fit_views.py on uvsphere48 and ptorus written as .obj, with the default start, --sphere_init 0.5 and
      --mesh_init, same seed and iteration count, each in a fresh child process; the depth loss it prints every 100 iterations.
No bar is set: the figures are recorded.  The share of the fp32 vector peak counts 79 FLOP per closest-point pair and 66 per winding
pair (every addition, multiplication, division, square root and atan2f as one), against 157.3 TFLOP/s.
    python tools/bench_meshdist.py [--tets full_size_tets.npz] [--fit_iters 1000] [--out profiles/meshdist_bench.txt]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FP32 = 157.3e12
FLOP = {"closest": 79, "winding": 66, "both": 79 + 66}


def _dot(u, v):
    return u[2] * v[2] + (u[1] * v[1] + u[0] * v[0])


def torch_query(p, tri, want_closest, want_winding, chunk_pairs=1 << 24):
    """The contract's arithmetic as elementwise torch over [queries of a chunk, T]: (dist2, face, closest, winding)."""
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    comp = lambda x, axis: tuple(x[:, c].unsqueeze(axis) for c in range(3))
    a, ab, ac = comp(a, 0), comp(ab, 0), comp(ac, 0)
    out = []
    step = max(chunk_pairs // max(tri.shape[0], 1), 1)
    zero, one = torch.zeros((), device=p.device), torch.ones((), device=p.device)
    for q0 in range(0, p.shape[0], step):
        q = comp(p[q0:q0 + step], 1)
        d2 = face = close = wind = None
        if want_closest:
            ap = tuple(q[k] - a[k] for k in range(3))
            d1, d2_ = _dot(ab, ap), _dot(ac, ap)
            bp = tuple(ap[k] - ab[k] for k in range(3))
            d3, d4 = _dot(ab, bp), _dot(ac, bp)
            cp = tuple(ap[k] - ac[k] for k in range(3))
            d5, d6 = _dot(ab, cp), _dot(ac, cp)
            vc, vb, va = d1 * d4 - d3 * d2_, d5 * d2_ - d1 * d6, d3 * d6 - d5 * d4
            e43, e56 = d4 - d3, d5 - d6
            den = (va + vb) + vc
            nv, dv, nw, dw, bc = vb, den, vc, den, torch.zeros_like(den, dtype=torch.bool)
            for flag, (rnv, rdv, rnw, rdw, rbc) in (((va <= 0) & (e43 >= 0) & (e56 >= 0), (nv, dv, e43, e43 + e56, True)),
                                                    ((vb <= 0) & (d2_ >= 0) & (d6 <= 0), (zero, one, d2_, d2_ - d6, False)),
                                                    ((vc <= 0) & (d1 >= 0) & (d3 <= 0), (d1, d1 - d3, zero, one, False)),
                                                    ((d6 >= 0) & (d5 <= d6), (zero, one, one, one, False)),
                                                    ((d3 >= 0) & (d4 <= d3), (one, one, zero, one, False)),
                                                    ((d1 <= 0) & (d2_ <= 0), (zero, one, zero, one, False))):
                nv, dv, nw, dw = torch.where(flag, rnv, nv), torch.where(flag, rdv, dv), torch.where(flag, rnw, nw), torch.where(flag, rdw, dw)
                bc = torch.where(flag, torch.full_like(bc, rbc), bc)
            w = nw / dw
            v = torch.where(bc, 1 - w, nv / dv)
            c = tuple(a[k] + (ab[k] * v + ac[k] * w) for k in range(3))
            d = tuple(q[k] - c[k] for k in range(3))
            dist = _dot(d, d)
            dist = torch.where(torch.isnan(dist), torch.full_like(dist, float("inf")), dist)
            d2, face = dist.min(dim=1)
            close = torch.stack([c[k].expand_as(dist).gather(1, face[:, None])[:, 0] for k in range(3)], 1)
        if want_winding:
            A = tuple(a[k] - q[k] for k in range(3))
            B = tuple(A[k] + ab[k] for k in range(3))
            C = tuple(A[k] + ac[k] for k in range(3))
            la, lb, lc = torch.sqrt(_dot(A, A)), torch.sqrt(_dot(B, B)), torch.sqrt(_dot(C, C))
            cr = (B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0])
            det = _dot(A, cr)
            dn = (((la * lb) * lc + _dot(A, B) * lc) + _dot(B, C) * la) + _dot(C, A) * lb
            wind = ((2 * torch.atan2(det, dn)).double().sum(1) / (4 * np.pi)).float()
        out.append((d2, face, close, wind))
    return tuple(None if out[0][k] is None else torch.cat([o[k] for o in out]) for k in range(4))


def event_ms(fn, calls, repeats):
    """The median over `repeats` windows of (device time of `calls` back-to-back calls) / calls, after one warm-up window."""
    fn()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _c in range(calls):
            fn()
        end.record()
        end.synchronize()
        rounds.append(start.elapsed_time(end) / calls)
    return float(np.median(rounds)), rounds


def bench_kernel(lines, grid_verts, a):
    import remesh_cases as rm
    from meshdiffusion_amd import meshdist
    p = (torch.as_tensor(grid_verts, dtype=torch.float32) * 2.1).cuda()
    Q = p.shape[0]
    for stacks, slices in ((48, 96), (160, 320)):
        v, f = rm.uv_sphere(stacks, slices)
        v, f = (v * 0.8).cuda(), f.cuda()
        tri, tri_ptr, face_of, M = meshdist.mesh_triangles(v, f)
        T = tri.shape[0]
        qb = min(Q, a.baseline_queries)
        for form, (wc, ww) in (("closest", (True, False)), ("winding", (False, True)), ("both", (True, True))):
            run = lambda: meshdist.mesh_query(p, tri, tri_ptr, face_of, M, None, "bench", wc, ww)
            ms, rounds = event_ms(run, a.calls, a.repeats)
            base = lambda: torch_query(p[:qb], tri, wc, ww)
            bms, brounds = event_ms(base, 1, 3)
            got, ref = run(), base()
            apart = []
            if wc:
                apart.append(f"dist2 bit-equal on {int((got[0][:qb] == ref[0]).sum())} of {qb}, faces equal on {int((got[1][:qb] == ref[1]).sum())}")
            if ww:
                apart.append(f"winding apart by {float((got[3][:qb] - ref[3]).abs().max()):.1e} at the most")
            rate, brate = Q * T / (ms * 1e-3), qb * T / (bms * 1e-3)
            lines.append(f"Q={Q} T={T} {form:8s}: md_mesh_query {ms:8.3f} ms (rounds {', '.join(f'{r:.3f}' for r in rounds)}) = {rate / 1e9:8.1f} G pair tests/s = "
                         f"{100 * rate * FLOP[form] / PEAK_FP32:4.1f} % of the fp32 vector peak at {FLOP[form]} FLOP per pair | chunked torch on {qb} queries "
                         f"{bms:9.3f} ms = {brate / 1e9:6.2f} G pair tests/s | x{rate / brate:.0f} | {'; '.join(apart)}")
            print(lines[-1], flush=True)


def bench_remesh(lines, a):
    import raster_cases as rc
    from meshdiffusion_amd import meshdist, postprocess
    from meshdiffusion_amd.dmtet import GridMesher
    R, n = 64, 32
    k = (torch.arange(R, dtype=torch.float32) + 0.5) / R - 0.5
    z, y, xg = torch.meshgrid(k, k, k, indexing="ij")
    samples = np.zeros((n, 4, R, R, R), np.float32)
    for m in range(n):
        samples[m, 0] = torch.sign(torch.sqrt(xg * xg + y * y + z * z) - (0.2 + 0.25 * m / (n - 1))).numpy()
    samples[:, 1:] = np.random.default_rng(0).uniform(-0.9, 0.9, samples[:, 1:].shape).astype(np.float32)
    tv, ti = rc.tet_grid()
    meshes = [(v.clone(), f.clone()) for v, f, _ in GridMesher(tv, ti, 64)(torch.from_numpy(samples))]
    verts, faces, vert_mesh = postprocess.concat_meshes(meshes)
    spent = [0.0]
    inner = meshdist.mesh_query

    def timed(*args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(*args)
        torch.cuda.synchronize()
        spent[0] += (time.perf_counter() - t0) * 1e3
        return out

    def wall(project):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = postprocess.remesh(verts, faces, iters=3, vert_mesh=vert_mesh, project=project)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    wall(True), wall(False)                                              # warm-up
    off = float(np.median([wall(False)[0] for _ in range(3)]))
    on = float(np.median([wall(True)[0] for _ in range(3)]))
    meshdist.mesh_query = timed
    _, (x, f, vm, info) = wall(True)
    meshdist.mesh_query = inner
    lines.append(f"remesh(iters=3) on {n} marching-tets meshes (V {verts.shape[0]} F {faces.shape[0]} -> V {x.shape[0]} F {f.shape[0]}): without projection "
                 f"{off:.1f} ms, with {on:.1f} ms wall clock (medians of 3); the three projections, synchronised: {spent[0]:.1f} ms = "
                 f"{100 * spent[0] / on:.0f} % of the call; vertices moved by at most {[round(r['max_project_dist2'] ** 0.5, 5) for r in info['iterations']]}")
    print(lines[-1], flush=True)


def bench_fit(lines, tets, a):
    import remesh_cases as rm
    from meshdiffusion_amd import mesh_export
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("uvsphere48", "ptorus"):
            v, f = rm.mesh(name)
            obj = os.path.join(tmp, name + ".obj")
            mesh_export.save_obj(obj, v, f)
            for tag, extra in (("default start", []), ("--sphere_init 0.5", ["--sphere_init", "0.5"]), ("--mesh_init", ["--mesh_init"])):
                cmd = [sys.executable, os.path.join(ROOT, "tools", "fit_views.py"), "--obj", obj, "--tet_path", tets, "--out",
                       os.path.join(tmp, "fit.pt"), "--iters", str(a.fit_iters), "--seed", "0"] + extra
                t0 = time.perf_counter()
                r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.fit_timeout)
                if r.returncode != 0:
                    raise SystemExit(f"fit_views.py failed ({r.returncode}): {r.stderr[-2000:]}")
                losses = [ln.split("depth loss")[1].split()[0] for ln in r.stdout.splitlines() if ln.startswith("iter ")]
                last = [ln for ln in r.stdout.splitlines() if ln.startswith("iter ")][-1]
                lines.append(f"fit_views.py {name} ({f.shape[0]} faces), {a.fit_iters} iterations, seed 0, {tag}: depth loss every 100 iterations "
                             f"{' '.join(losses)} | last: {last} | {time.perf_counter() - t0:.0f} s with start-up")
                print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tets", default=None, help="a full-size <R>_tets_cropped.npz; default: the golden 64 grid of the tests")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline_queries", type=int, default=2048)
    ap.add_argument("--fit_iters", type=int, default=0, help="> 0: also run the three starts of fit_views.py for this many iterations")
    ap.add_argument("--fit_timeout", type=int, default=600)
    ap.add_argument("--out", default=None, help="also write the report there (profiles/meshdist_bench.txt)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshdist.py needs a GPU: the HIP path has no CPU fallback")
    golden = os.path.join(ROOT, "tests", "golden", "64_tets_cropped.npz")
    tets = a.tets if a.tets and os.path.exists(a.tets) else golden
    grid = np.load(tets)["vertices"]
    lines = [f"tet grid: {'the golden 64 grid of the tests' if tets == golden else tets} ({grid.shape[0]} vertices, scaled by 2.1); targets: unit "
             f"uv spheres scaled by 0.8; {a.calls} calls per window, median of {a.repeats} windows, device events"]
    print(lines[0], flush=True)
    bench_kernel(lines, grid, a)
    bench_remesh(lines, a)
    if a.fit_iters > 0:
        bench_fit(lines, tets, a)
    lines.append(f"measured on one MI355X: python tools/bench_meshdist.py{f' --fit_iters {a.fit_iters}' if a.fit_iters > 0 else ''} --out profiles/meshdist_bench.txt")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
