"""Writes tests/golden/dpmpp.npz: how far the guided DPM-Solver++ recursion of the closed-form model moves under one float32
rounding per step -- the yardstick of tests/test_gpu_dpmpp.py::test_guided_loop_against_the_closed_form.  CPU only, seconds.

    python tools/gen_golden_dpmpp.py

Setup: guidance_cases.loop_setup() (8^3 grid, B = 2, grid mask, eps_hat = k_t x), x_T = randn(seed 9), SCHEDULE / STEPS / ORDER
below, zeta = 1.  For replacement on and off the float64 recursion (tests/dpmpp_cases.recursion, rows from sampling.dpmpp_tables)
runs twice: exactly, and with the guidance term evaluated at float(x), the state the sampler's network sees.  Stored: a_on / a_off,
the rel-L2 distance of the two final states; `moved_on` / `moved_off`, the distance of the guided from the unguided run; the
settings.  The test's bar is max(4 a, 1e-6): the probe injects one of the about four float32 roundings a guided step has (state,
eps_hat, cot, g)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dpmpp_cases as dc                                               # noqa: E402
import guidance_cases as gc                                            # noqa: E402
from meshdiffusion_amd.lib.diffusion import sampling                   # noqa: E402

SCHEDULE, STEPS, ORDER, SEED = "logsnr", 20, 2, 9


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def run(s, zeta, replace, round_input, schedule=SCHEDULE):
    sde, N, ch, y, pm, gm = s["sde"], s["N"], s["ch"], s["y"], s["pm"], s["gm"]
    times = sampling.dpmpp_schedule(sde, STEPS, schedule, 1e-3)
    rows, labels = sampling.dpmpp_tables(sde, times, order=ORDER, variant="taylor", tau=0)
    orders = sampling.dpmpp_orders(STEPS, ORDER)
    x_T = torch.randn(s["shape"], generator=torch.Generator().manual_seed(SEED))
    guide = dc.gaussian_guide(s["s"], N, rows, labels, y, pm, gm, zeta, ch, round_input=round_input) if zeta else None
    return dc.recursion(gc.GaussianEps(s["s"], N), x_T, rows, labels, orders, gm=gm, partial=y if replace else None, pm=pm, ch=ch,
                        guide=guide, round_state=False)


def main():
    s = gc.loop_setup()
    out = dict(schedule=np.array(SCHEDULE), steps=np.int64(STEPS), order=np.int64(ORDER), seed=np.int64(SEED))
    for schedule in ("logsnr", "uniform", "quad"):
        for tag, replace in (("on", True), ("off", False)):
            exact, probe = run(s, s["zeta"], replace, False, schedule), run(s, s["zeta"], replace, True, schedule)
            a, moved = rel_l2(probe, exact), rel_l2(exact, run(s, 0.0, True, False, schedule))
            print(f"{schedule:8s} replacement {tag:3s}: a = {a:.3e}, guided vs unguided {moved:.3e}")
            if schedule == SCHEDULE:
                out[f"a_{tag}"], out[f"moved_{tag}"] = np.float64(a), np.float64(moved)
    path = os.path.join(ROOT, "tests", "golden", "dpmpp.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
