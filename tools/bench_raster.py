"""Depth rasteriser cost, one process, at 512 x 512 with B = 1 and 8 views on the sphere and the noise mesh of
tests/raster_cases.py:
  (a) forward, two layers (`rasterize`) and forward + backward (`render_depth` and the gradient of both depth layers), in ms;
  (b) the split of (a) between the kernels (binning count / emit, tile kernel, depth, backward) and the torch glue around them
      (cumsum, the stable sort by tile, searchsorted, the CSR of the backward);
  (c) (pixel, triangle) coverage tests per second of the tile kernel: 256 x the (tile, triangle) pairs per launch;
  (d) the baseline: the fp32 torch restatement of the contract (tests/raster_cases.py) on the same GPU, forward and
      forward + backward, one repetition;
  (f) at B = 8: `antialias` of the layer-1 coverage mask, forward and forward + backward (color and pos_clip), next to the fp32
      torch restatement of tests/antialias_cases.py on the same GPU in interleaved rounds; `edge_neighbours`; `render_depth`
      forward + backward with and without antialias=True; the device kernels launched per call (torch.profiler);
  (g) at B = 8: `render_buffers` (the bsdf == 'normal' renderer: interpolation, vertex normals, shading normal, two antialiased
      images) forward and forward + backward next to `render_depth(antialias=True)` at equal shapes in interleaved rounds, and
      the split of its device time between the library's own kernels and the torch glue (elementwise chain, sorts, CSRs) with
      the launches of each (torch.profiler);
  (e) one fit_to_views iteration on the shipped 64 grid (sphere start, torus target, 8 views at 512 x 512), next to the
      chamfer iteration of tools/bench_pointcloud.py.
Device events after warm-up; each figure is the median over rounds.
    python tools/bench_raster.py [--res 512] [--rounds 5] [--reps 5] [--json PATH] [--no-baseline]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pc import timed  # noqa: E402


def median_ms(fn, rounds, reps):
    fn()
    torch.cuda.synchronize()
    return statistics.median(timed(fn, reps) for _ in range(rounds))


def interleaved_ms(fns, rounds, reps):
    """Medians of several callables timed in interleaved rounds (a, b, a, b, ...), so that drift hits all alike."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    samples = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            samples[k].append(timed(f, reps))
    return [statistics.median(x) for x in samples]


def launches(fn):
    """Device kernels launched by one call, or -1 when the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "mem" not in e.name.lower())
    except Exception:
        return -1


def device_split(fn):
    """(own kernels ms, own launches, torch glue ms, glue launches) of one call by torch.profiler: device time of the library's
    kernels (every one is named md_<...>_kernel) against every other device kernel; copies and memsets are left out.  None,
    with the reason printed, when the profiler cannot be used."""
    import re
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError as e:
        print(f"device_split: torch.profiler is not available ({e}); no split of kernel time against glue", flush=True)
        return None
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    except RuntimeError as e:
        print(f"device_split: the profiler failed ({e}); no split of kernel time against glue", flush=True)
        return None
    own, glue = [0.0, 0], [0.0, 0]
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA or e.name.startswith(("Memcpy", "Memset")):
            continue
        acc = own if re.search(r"\bmd_\w+_kernel\b", e.name) else glue
        acc[0] += e.device_time_total / 1000.0
        acc[1] += 1
    return own[0], own[1], glue[0], glue[1]


def bench_buffers(name, verts, faces, mvp, campos, H, W, a, rec):
    from meshdiffusion_amd import render
    B = mvp.shape[0]
    G1 = torch.randn(B, H, W, 1, device="cuda")
    G3, G4 = torch.randn(B, H, W, 3, device="cuda"), torch.randn(B, H, W, 4, device="cuda")

    def depth_fwd():
        with torch.no_grad():
            return render.render_depth(verts, faces, mvp, campos, (H, W), antialias=True)

    def depth_fwd_bwd():
        v = verts.detach().requires_grad_(True)
        out = render.render_depth(v, faces, mvp, campos, (H, W), antialias=True)
        ((out["depth"] * G1).sum() + (out["depth_second"] * G1).sum() + (out["alpha"] * G1).sum() + (out["alpha_second"] * G1).sum()).backward()
        return v.grad

    def buf_fwd():
        with torch.no_grad():
            return render.render_buffers(verts, faces, mvp, campos, (H, W))

    def buf_fwd_bwd():
        v = verts.detach().requires_grad_(True)
        out = render.render_buffers(v, faces, mvp, campos, (H, W))
        ((out["depth"] * G1).sum() + (out["depth_second"] * G1).sum() + (out["shaded"] * G4).sum() + (out["shaded_second"] * G4).sum()
         + (out["normal"] * G3).sum() + (out["pos"] * G3).sum()).backward()
        return v.grad

    t = interleaved_ms([depth_fwd, buf_fwd, depth_fwd_bwd, buf_fwd_bwd], a.rounds, a.reps)
    split = [device_split(f) for f in (buf_fwd, buf_fwd_bwd, depth_fwd_bwd)]
    line = (f"render_buffers {name} V={verts.shape[0]} F={faces.shape[0]} B={B} {H}x{W}: forward {t[1]:.3f} ms (render_depth(antialias=True) "
            f"{t[0]:.3f} ms, x{t[1] / t[0]:.2f}) | forward+backward {t[3]:.3f} ms (render_depth(antialias=True) {t[2]:.3f} ms, x{t[3] / t[2]:.2f})")
    for label, sp in zip(("forward", "forward+backward", "render_depth(antialias=True) forward+backward"), split):
        if sp is not None:
            line += (f" | {label} device time: own kernels {sp[0]:.3f} ms in {sp[1]} launches, torch glue {sp[2]:.3f} ms in {sp[3]} launches "
                     f"({100 * sp[2] / max(sp[0] + sp[2], 1e-9):.0f} % glue)")
    print(line, flush=True)
    rec["cases"][f"buffers_{name}_B{B}"] = dict(render_depth_aa_forward=round(t[0], 4), forward=round(t[1], 4),
                                               render_depth_aa_forward_backward=round(t[2], 4), forward_backward=round(t[3], 4),
                                               device_split=split)


def bench_antialias(name, verts, faces, mvp, campos, pc, H, W, a, rec):
    import antialias_cases as ac
    from meshdiffusion_amd import render
    B, V = pc.shape[0], verts.shape[0]
    rast = render.rasterize(pc, faces, (H, W))[0]
    nbr = render.edge_neighbours(faces, V)
    mask = (rast[..., 3:4] > 0).float()
    G = torch.randn(B, H, W, 1, device="cuda")
    _, pairs = render.antialias(mask, rast, pc, faces, nbr, return_pairs=True)
    active = int((pairs[..., 0] >= 0).sum())
    cand = int((rast[:, :, :-1, 3] != rast[:, :, 1:, 3]).sum() + (rast[:, :-1, :, 3] != rast[:, 1:, :, 3]).sum())

    def fwd():
        return render.antialias(mask, rast, pc, faces, nbr)

    def fwd_bwd():
        c, p = mask.clone().requires_grad_(True), pc.clone().requires_grad_(True)
        (render.antialias(c, rast, p, faces, nbr) * G).sum().backward()
        return p.grad

    def base_fwd():
        return ac.antialias_restated(mask, rast, pc, faces, nbr, torch.float32)

    def base_fwd_bwd():
        return ac.grads_restated(mask, rast, pc, faces, nbr, G, torch.float32)[2]

    def depth(aa):
        def run():
            v = verts.detach().requires_grad_(True)
            out = render.render_depth(v, faces, mvp, campos, (H, W), antialias=aa)
            loss = (out["depth"] * G).sum() + (out["depth_second"] * G).sum()
            if aa:
                loss = loss + (out["alpha"] * G).sum() + (out["alpha_second"] * G).sum()
            loss.backward()
            return v.grad
        return run

    t = interleaved_ms([fwd, base_fwd, fwd_bwd, base_fwd_bwd], a.rounds, a.reps)
    t_nbr, t_plain, t_aa = interleaved_ms([lambda: render.edge_neighbours(faces, V), depth(False), depth(True)], a.rounds, a.reps)
    n = [launches(f) for f in (fwd, fwd_bwd, lambda: render.edge_neighbours(faces, V), depth(False), depth(True))]
    print(f"antialias {name} V={V} F={faces.shape[0]} B={B} {H}x{W} C=1: candidate pairs {cand} active {active} | forward {t[0]:.3f} ms "
          f"({n[0]} launches; fp32 torch restatement {t[1]:.1f} ms, x{t[1] / t[0]:.0f}) | forward+backward {t[2]:.3f} ms ({n[1]} launches; "
          f"restatement {t[3]:.1f} ms, x{t[3] / t[2]:.0f}) | edge_neighbours {t_nbr:.3f} ms ({n[2]} launches) | render_depth forward+backward "
          f"{t_plain:.3f} ms ({n[3]} launches), with antialias=True {t_aa:.3f} ms ({n[4]} launches)", flush=True)
    rec["cases"][f"antialias_{name}_B{B}"] = dict(forward=round(t[0], 4), baseline_forward=round(t[1], 4), forward_backward=round(t[2], 4),
                                                 baseline_forward_backward=round(t[3], 4), edge_neighbours=round(t_nbr, 4),
                                                 render_depth=round(t_plain, 4), render_depth_antialias=round(t_aa, 4), launches=n,
                                                 candidates=cand, active=active)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--only-antialias", action="store_true", help="skip the rasteriser's own rows and the fit iteration")
    ap.add_argument("--only-buffers", action="store_true", help="only the render_buffers rows (g)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raster.py needs a GPU: the HIP path has no CPU fallback")
    import raster_cases as rc
    from meshdiffusion_amd import _lib, render
    from meshdiffusion_amd.dmtet import DMTetGeometry
    from meshdiffusion_amd.hip_ops import _ptr, _stream
    lib = _lib.load()
    H = W = a.res
    rec = {"res": a.res, "rounds": a.rounds, "reps": a.reps, "cases": {}}
    for name in ("sphere", "noise"):
        verts, faces = (t.cuda() for t in rc.mesh(name))
        V, F = verts.shape[0], faces.shape[0]
        for B in (1, 8):
            angles = [0.7 + 2 * 3.141592653589793 * k / B for k in range(B)]
            mvp, campos = (t.cuda() for t in rc.cameras(angles, H, W))
            pc = render.xfm_points(verts[None], mvp).contiguous()
            G = torch.randn(B, H, W, 1, device="cuda")
            if B == 8 and not a.only_buffers:
                bench_antialias(name, verts, faces, mvp, campos, pc, H, W, a, rec)
            if B == 8 and not a.only_antialias:
                bench_buffers(name, verts, faces, mvp, campos, H, W, a, rec)
            if a.only_antialias or a.only_buffers:
                continue

            def fwd():
                return render.rasterize(pc, faces, (H, W))

            def fwd_bwd():
                v = verts.detach().requires_grad_(True)
                out = render.render_depth(v, faces, mvp, campos, (H, W))
                ((out["depth"] * G).sum() + (out["depth_second"] * G).sum()).backward()
                return v.grad

            # the kernels alone, on buffers built once
            counts = torch.empty(B * F, dtype=torch.int32, device="cuda")
            k_count = lambda: _lib.check(lib.md_raster_bin_count(_ptr(pc), _ptr(faces), B, V, F, H, W, _ptr(counts), _stream()), "count")  # noqa: E731
            k_count()
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            total = int(ends[-1])
            offsets = (ends - counts).contiguous()
            pt, pf = torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int32, device="cuda")
            k_emit = lambda: _lib.check(lib.md_raster_bin_emit(_ptr(pc), _ptr(faces), _ptr(offsets), B, V, F, H, W, total, _ptr(pt), _ptr(pf), _stream()), "emit")  # noqa: E731
            tile_ptr, tile_faces = render._bin(pc, faces, H, W)
            r1 = torch.empty(B, H, W, 4, device="cuda")
            r2 = torch.empty_like(r1)
            k_tiles = lambda: _lib.check(lib.md_raster_tiles(_ptr(pc), _ptr(faces), _ptr(tile_ptr), _ptr(tile_faces), B, V, F, H, W, _ptr(r1), _ptr(r2), _stream()), "tiles")  # noqa: E731
            k_tiles()
            d1, d2, m1, m2 = (torch.empty(B, H, W, 1, device="cuda") for _ in range(4))
            k_depth = lambda: _lib.check(lib.md_raster_depth(_ptr(r1), _ptr(r2), _ptr(verts), _ptr(faces), _ptr(campos), B, V, F, H, W, _ptr(d1), _ptr(d2), _ptr(m1), _ptr(m2), _stream()), "depth")  # noqa: E731
            ids = torch.stack([r1[..., 3], r2[..., 3]], 1).reshape(-1)
            cov = torch.nonzero(ids > 0)[:, 0]
            N = cov.numel()
            vals, order = torch.sort(faces[ids[cov].long() - 1].reshape(-1), stable=True)
            ptr = torch.searchsorted(vals, torch.arange(V + 1, device="cuda")).to(torch.int32).contiguous()
            order, cov32 = order.to(torch.int32).contiguous(), cov.to(torch.int32).contiguous()
            cg, dv = torch.empty(N, 3, 3, device="cuda"), torch.empty(V, 3, device="cuda")
            g1 = G.reshape(B, H, W).contiguous()
            k_bwd = lambda: _lib.check(lib.md_raster_depth_bwd(_ptr(cov32), N, _ptr(r1), _ptr(r2), _ptr(g1), _ptr(g1), _ptr(pc), _ptr(verts), _ptr(faces), _ptr(mvp), _ptr(campos), _ptr(ptr), _ptr(order), B, V, F, H, W, _ptr(cg), _ptr(dv), _stream()), "bwd")  # noqa: E731

            ms = {k: median_ms(f, a.rounds, a.reps) for k, f in (("forward", fwd), ("forward_backward", fwd_bwd), ("k_bin_count", k_count),
                                                               ("k_bin_emit", k_emit), ("k_tiles", k_tiles), ("k_depth", k_depth),
                                                               ("k_backward", k_bwd))}
            k_fwd = ms["k_bin_count"] + ms["k_bin_emit"] + ms["k_tiles"]
            k_all = k_fwd + ms["k_depth"] + ms["k_backward"]
            tests = 256.0 * total / (ms["k_tiles"] * 1e-3)
            line = (f"{name} V={V} F={F} B={B} {H}x{W}: forward {ms['forward']:.3f} ms (kernels {k_fwd:.3f}: count {ms['k_bin_count']:.3f} emit "
                    f"{ms['k_bin_emit']:.3f} tiles {ms['k_tiles']:.3f}; torch glue {ms['forward'] - k_fwd:.3f}) | forward+backward "
                    f"{ms['forward_backward']:.3f} ms (kernels {k_all:.3f}: depth {ms['k_depth']:.3f} backward {ms['k_backward']:.3f}; torch glue "
                    f"{ms['forward_backward'] - k_all:.3f}) | {total} (tile, triangle) pairs, {tests / 1e9:.1f} G (pixel, triangle) tests/s | covered entries {N}")
            if not a.no_baseline:
                try:
                    def base_fwd():
                        return rc.rasterize_restated(pc, faces, H, W)["ids"]

                    def base_fwd_bwd():
                        return rc.grad_restated(verts, faces, mvp, campos, base_fwd(), torch.cat([G, G], 3).permute(0, 3, 1, 2), torch.float32)
                    ms["baseline_forward"] = median_ms(base_fwd, 1, 1)
                    ms["baseline_forward_backward"] = median_ms(base_fwd_bwd, 1, 1)
                    line += (f" | fp32 torch restatement: forward {ms['baseline_forward']:.1f} ms (x{ms['baseline_forward'] / ms['forward']:.0f}) "
                             f"forward+backward {ms['baseline_forward_backward']:.1f} ms (x{ms['baseline_forward_backward'] / ms['forward_backward']:.0f})")
                except torch.cuda.OutOfMemoryError:
                    line += " | fp32 torch restatement: out of memory at this size, not timed"
                    torch.cuda.empty_cache()
            print(line, flush=True)
            rec["cases"][f"{name}_B{B}"] = dict({k: round(v, 4) for k, v in ms.items()}, pairs=total, tests_per_s=tests, covered=N, V=V, F=F)

    # one fitting iteration: shipped grid, sphere start, torus target, 8 views
    geo = DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(rc.fit_initial_sdf(geo.verts))
    tv, tf = (t.cuda() for t in rc.mesh("torus"))
    for B, res in (() if a.only_antialias or a.only_buffers else ((4, 64), (8, a.res))):
        mvp, campos = (t.cuda() for t in rc.cameras([2 * 3.141592653589793 * k / B for k in range(B)], res, res))
        targets = render.make_targets(tv, tf, mvp, campos, res)
        state = {"it": 1}

        def fit_iter():
            render.fit_to_views(geo, targets, 1, lr=1e-4, carve=False, start_iteration=state["it"])
            state["it"] += 1
        t = median_ms(fit_iter, a.rounds, a.reps)
        print(f"fit_to_views iteration, {B} views at {res}x{res} (marching tets + render_depth + depth loss + regulariser + Adam, a new "
              f"optimiser each call): {t:.3f} ms  (the chamfer iteration of tools/bench_pointcloud.py: 3.2 ms)", flush=True)
        rec[f"fit_iter_B{B}_{res}"] = round(t, 4)
    print(json.dumps(rec), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
