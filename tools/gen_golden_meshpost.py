"""Generate tests/golden/meshpost.npz (build host only, CPU, seeded):
    python tools/gen_golden_meshpost.py

  smooth/<mesh>/<setting>/ref_err    per mesh and smoothing setting of tests/meshpost_cases.py: the fp32 torch restatement's OWN
                      rel-L2 distance from the float64 one -- the unit of the GPU tests' bars (4 units).
  shade/<case>/<light>/ref_err       the same for the rgb channels of the shading over the covered pixels of each case, on the rast of
                      the CPU restatement of the rasteriser, with the flip decided in float64.
  shade/<case>/flip_margin           the smallest |geo . view| of a covered pixel in float64.
The file holds only such numbers.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import interp_cases as ic  # noqa: E402
import meshpost_cases as mc  # noqa: E402
import raster_cases as rc  # noqa: E402


def main():
    out = {}
    for name in mc.CASES:
        verts, faces = mc.mesh(name)
        rows = mc.smoothing_rows(faces, verts.shape[0])
        for tag, steps, lam, mu in mc.SMOOTH_SETTINGS:
            x32 = mc.smooth_restated(verts, faces, steps, lam, mu, torch.float32, rows)
            x64 = mc.smooth_restated(verts, faces, steps, lam, mu, torch.float64, rows)
            e = rc.rel_l2(x32, x64)
            out[f"smooth/{name}/{tag}/ref_err"] = np.float64(e)
            print(f"[meshpost] smooth {name} {tag}: V {verts.shape[0]} F {faces.shape[0]} fp32 restatement vs float64 {e:.2e}")
    for case in mc.SHADE_CASES:
        verts, faces, mvp, campos, pc, H, W, rast = mc.shade_inputs(case)
        for light in mc.LIGHTS:
            sh, kd = mc.case_light(light)
            o64, gv, cov = mc.shade_restated(rast, verts, faces, campos, sh, kd, torch.float64)
            o32, _, _ = mc.shade_restated(rast, verts, faces, campos, sh, kd, torch.float32, front=gv > 0)
            e = mc.rgb_rel_l2(o32, o64, cov)
            out[f"shade/{ic.case_id(case)}/{light}/ref_err"] = np.float64(e)
            print(f"[meshpost] shade {ic.case_id(case)} {light}: covered {int(cov.sum())} range {float(o64[..., :3][cov].min()):.3f}-"
                  f"{float(o64[..., :3][cov].max()):.3f} fp32 restatement vs float64 {e:.2e}")
        margin = float(gv[cov].abs().min())
        out[f"shade/{ic.case_id(case)}/flip_margin"] = np.float64(margin)
        print(f"[meshpost] shade {ic.case_id(case)}: smallest |geo . view| {margin:.4f}; front pixels per view "
              f"{[int(((gv > 0) & cov)[b].sum()) for b in range(gv.shape[0])]} of {[int(cov[b].sum()) for b in range(gv.shape[0])]}")
    path = os.path.join(rc.GOLD, "meshpost.npz")
    np.savez_compressed(path, **out)
    print(f"[meshpost] wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
