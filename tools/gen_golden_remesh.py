"""Generate tests/golden/remesh.npz (build host only, CPU) from the numpy restatement of the remeshing contract:
    python tools/gen_golden_remesh.py

  relax/<mesh>/ref_err                the float32 restatement's OWN rel-L2 distance from the float64 one for one relax pass
                      (lam 0.5) on the mesh as given -- the unit of the GPU test's bar (4 units).
  quality/<mesh>/<scale>/...          the restatement's whole pipeline (5 iterations, relax 0.5) at the default target times scale:
                      share_before / share_after (edges within [4/5 L, 4/3 L]), angle_before / angle_after (minimum angle,
                      degrees), faces_after.
  fidelity/uvsphere/radial_dev        max | |x| - 1 | after that pipeline on the unit sphere at scale 1.
The file holds only such numbers.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raster_cases as rc  # noqa: E402
import remesh_cases as rm  # noqa: E402

RELAX = 0.5


def generate():
    out = {}
    for name in rm.EXACT_CASES:
        v, f = rm.mesh(name)
        x32, x64 = rm.relax_restated(v.numpy(), f.numpy(), RELAX, np.float32), rm.relax_restated(v.numpy(), f.numpy(), RELAX, np.float64)
        e = rc.rel_l2(x32, x64)
        out[f"relax/{name}/ref_err"] = np.float64(e)
        print(f"[remesh] relax {name}: V {v.shape[0]} moved {int((x32 != v.numpy()).any(1).sum())} fp32 restatement vs float64 {e:.2e}")
    for name, scale in rm.QUALITY_CASES:
        v, f = rm.mesh(name)
        x, g, _, info = rm.pipeline_restated(name, scale, RELAX)
        L = float(info["target"][0])
        before, after = rm.quality(v.numpy(), f.numpy(), L), rm.quality(x, g, L)
        key = f"quality/{name}/{scale}"
        out[f"{key}/share_before"], out[f"{key}/angle_before"] = np.float64(before[0]), np.float64(before[1])
        out[f"{key}/share_after"], out[f"{key}/angle_after"] = np.float64(after[0]), np.float64(after[1])
        out[f"{key}/faces_after"] = np.int64(g.shape[0])
        print(f"[remesh] {name} x {scale}: L {L:.4f} F {f.shape[0]} -> {g.shape[0]} share {before[0]:.3f} -> {after[0]:.3f} "
              f"min angle {before[1]:.1f} -> {after[1]:.1f} problems {rm.problems(g, x.shape[0])}")
        print("         per iteration (splits, collapses, flips, collapse rounds, flip rounds): "
              f"{[tuple(r.values()) for r in info['iterations']]}")
        if (name, scale) == ("uvsphere", 1.0):
            dev = float(np.abs(np.linalg.norm(x.astype(np.float64), axis=1) - 1).max())
            out["fidelity/uvsphere/radial_dev"] = np.float64(dev)
            print(f"[remesh] uvsphere: max | |x| - 1 | {dev:.4f}")
    return out


def main():
    out = generate()
    path = os.path.join(rc.GOLD, "remesh.npz")
    np.savez_compressed(path, **out)
    print(f"[remesh] wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
