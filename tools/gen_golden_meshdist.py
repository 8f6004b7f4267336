"""Generate tests/golden/meshdist.npz (build host only, CPU) from the numpy restatement of the mesh distance contract:
    python tools/gen_golden_meshdist.py

  closest/<mesh>/<queries>/unit_closest, unit_dist   the float32 restatement's OWN rel-L2 distance from the float64 one, for the closest
                      points and for sqrt(dist2), on the lattice and on the surface queries (vertices and edge midpoints) of every
                      case, and on the lattice of uvsphere48 -- the units of the GPU test's bar (4 units).
  winding/<mesh>/unit the float32 restatement's OWN max-abs distance from the float64 winding number on the lattice.
  project/<mesh>/<on|off>/share, angle, mean_dist, max_dist, faces   the restated remeshing pipeline (2 iterations, relax 0.5) with and
                      without re-projection: remesh_cases.quality of the (first) mesh, and the mean and maximum float64 distance of
                      the output vertices to the input surface.
The file holds only such numbers.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import meshdist_cases as md  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def generate():
    out = {}
    for name in md.CASES + (md.BIG,):
        for which in md.QUERY_SETS if name != md.BIG else ("lattice",):
            uc, ud = md.closest_units(name, which)
            out[f"closest/{name}/{which}/unit_closest"], out[f"closest/{name}/{which}/unit_dist"] = np.float64(uc), np.float64(ud)
            print(f"[meshdist] closest {name} {which}: T {md.case_triangles(name)[0].shape[0]} Q {md.queries(name, which)[0].shape[0]} "
                  f"fp32 restatement vs float64: closest {uc:.2e} dist {ud:.2e}")
        out[f"winding/{name}/unit"] = np.float64(md.winding_unit(name))
        w = md.case_winding(name, np.float64)
        print(f"[meshdist] winding {name}: fp32 restatement vs float64 {out[f'winding/{name}/unit']:.2e}, min | |w| - 0.5 | {np.abs(np.abs(w) - 0.5).min():.4f}")
    for name in md.PROJECT_CASES:
        for tag, project in (("on", True), ("off", False)):
            x, f, vm, info = md.project_restated(name, project)
            share, angle, mean, worst = md.project_figures(name, x, f, vm, info["target"])
            key = f"project/{name}/{tag}"
            out[f"{key}/share"], out[f"{key}/angle"] = np.float64(share), np.float64(angle)
            out[f"{key}/mean_dist"], out[f"{key}/max_dist"], out[f"{key}/faces"] = np.float64(mean), np.float64(worst), np.int64(f.shape[0])
            print(f"[meshdist] remesh {name} project {tag}: F {f.shape[0]} share {share:.3f} min angle {angle:.1f} "
                  f"distance to the input surface mean {mean:.2e} max {worst:.2e}")
    return out


def main():
    out = generate()
    path = os.path.join(GOLD, "meshdist.npz")
    np.savez_compressed(path, **out)
    print(f"[meshdist] wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
