"""Generate tests/golden/fixedtopo.npz (build host only, CPU, seeded):
    python tools/gen_golden_fixedtopo.py

  laplace/<mesh>/<nobase|base>/ref_err_{value,dx}   per mesh of tests/fixedtopo_cases.py, with and without `base`: the fp32 torch
                      restatement's OWN rel-L2 distance from the float64 one -- the unit of the GPU tests' bars (4 units).  The value
                      is a float32 scalar, which cannot be expected nearer to float64 than half an ulp: its unit is at least 2^-24.
                      A unit of 0 demands an exact result.
  laplace/x_seed, laplace/grad_out                  the seed of the displacement and the incoming gradient of the backward.
The file holds only such numbers.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fixedtopo_cases as fc  # noqa: E402
import raster_cases as rc  # noqa: E402


def main():
    out = {"laplace/x_seed": np.int64(fc.X_SEED), "laplace/grad_out": np.float64(fc.GRAD_OUT)}
    for name in fc.LAPLACE_MESHES:
        x, base, faces = fc.laplace_case(name)
        for kind in fc.BASES:
            b = base if kind == "base" else None
            v32, g32 = fc.laplace_grads_restated(x, faces, b, torch.float32)
            v64, g64 = fc.laplace_grads_restated(x, faces, b, torch.float64)
            e_v = max(rc.rel_l2(v32, v64), fc.HALF_ULP)
            e_g = rc.rel_l2(g32, g64)
            out[f"laplace/{name}/{kind}/ref_err_value"], out[f"laplace/{name}/{kind}/ref_err_dx"] = np.float64(e_v), np.float64(e_g)
            print(f"[fixedtopo] laplace {name} {kind}: V {x.shape[0]} F {faces.shape[0]} value {float(v64):.6e}  fp32 restatement vs "
                  f"float64: value {rc.rel_l2(v32, v64):.2e} (unit {e_v:.2e}) d x {e_g:.2e}")
    path = os.path.join(rc.GOLD, "fixedtopo.npz")
    np.savez_compressed(path, **out)
    print(f"[fixedtopo] wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
