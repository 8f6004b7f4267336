"""Writes tests/golden/latent.npz: the reference's own `slerp` (lib/diffusion/evaler.py:63-71, imported, not restated) evaluated
on the CPU on float64 copies of three seeded float32 pairs, at the positions alpha = 0, 0.25, 0.5, 0.8, 1.

    python tools/gen_golden_latent.py --reference /path/to/MeshDiffusion

The pairs are tests/latent_cases.GOLDEN_PAIRS, (seed, C, P, rho): b = rho*a + sqrt(1 - rho^2)*n from numpy's default_rng(seed), so the
file holds the seeds, shapes and positions and the float64 outputs only -- data, none of the reference's text.
tests/test_cpu_latent.py compares latent_cases.slerp_ref, the np.longdouble restatement the GPU tests use, against it.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import latent_cases as lc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation (holds lib/diffusion/evaler.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "latent.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from lib.diffusion import evaler                      # the reference's module: its slerp is what is recorded
    out = dict(alphas=np.array(lc.GOLDEN_ALPHAS), pairs=np.array(lc.GOLDEN_PAIRS, dtype=np.float64))
    for n, (seed, C, P, rho) in enumerate(lc.GOLDEN_PAIRS):
        a, b = lc.golden_pair(seed, C, P, rho)
        za, zb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
        rows = [evaler.slerp(za, zb, float(al)).numpy() for al in lc.GOLDEN_ALPHAS]
        out[f"out{n}"] = np.stack(rows)
        assert out[f"out{n}"].dtype == np.float64
        cos = float(torch.sum(za * zb) / (torch.norm(za) * torch.norm(zb)))
        out[f"cos{n}"] = np.float64(cos)
        print(f"pair {n}: seed {seed}, [{C}, {P}], rho {rho}: cos(theta) = {cos:+.4f}, max |out| = {np.abs(out[f'out{n}']).max():.4f}")
        assert abs(cos) <= 0.9, "the 1e-10 bar of the CPU test assumes 1/sin(theta) <= 2.3"
    np.savez(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
