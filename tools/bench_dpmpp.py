"""Times the DPM-Solver++ sampler (sampling.get_dpmpp_sampler) at res64, B = 8, on the GPU: device events around synchronised
work, after warm-up, the alternatives interleaved in one process (a, b, a, b, ...):
  * one dpmpp step (U-Net evaluation + md_multistep_step) beside one ddim step (U-Net evaluation + md_ddim_step);
  * md_multistep_step alone in windows of --inner calls, for the order-2 ODE update and the order-3 SDE update, with the bytes it
    moves computed here from the shapes (every operand read once, the three outputs written once, the [P] mask once) over its
    time, beside the measured HBM copy rate of MI355X_MICROARCH.md (6.29 TB/s; 8.0 TB/s is the datasheet's);
  * 20 dpmpp steps beside the 99-evaluation DDIM run (wall time of the whole sampler call, host clock around a synchronise);
  * 20 guided dpmpp steps beside 20 guided DDIM steps (reconstruction guidance, zeta = 1).

    python tools/bench_dpmpp.py [--batch 8] [--reps 3] [--inner 50] [--out profiles/dpmpp_bench.txt]

The weights are the synthetic sensitised ones (synth.sensitised_state_dict): the times do not depend on them.  Needs a GPU: there
is no CPU fallback.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_likelihood import stats, timed_alternating  # noqa: E402

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0


def update_bytes(B, Cc, P, nh, z, mask):
    """Bytes one md_multistep_step moves: x (8) + eps (4) + nh earlier predictions (8 each) + z (4) read, x_out (8) + x0_out (8) +
    x_f32 (4) written, per value; the mask once."""
    return B * Cc * P * (8 + 4 + 8 * nh + (4 if z else 0) + 20) + (4 * P if mask else 0)


def wall_alternating(fa, fb, reps, warm=()):
    """Host wall time (ms) of two whole sampler calls in alternating order, each ended by a device synchronise; `warm`: short
    runs of both, called once before, un-timed."""
    for fn in warm:
        fn()
    ma, mb = [], []
    for _ in range(reps):
        for fn, ms in ((fa, ma), (fb, mb)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
    return stats(ma), stats(mb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpmpp_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpmpp.py measures on the GPU: none found")
    from meshdiffusion_amd import config as mdc, hip_ops as ops, synth
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401

    cfg = mdc.get_config_res64()
    cfg.device = dev = torch.device("cuda", 0)
    R, B, steps = cfg.data.image_size, args.batch, args.steps
    P = R ** 3
    gm = synth.synthetic_grid_mask(R)
    model = mutils.create_model(cfg).eval()
    model.module.load_state_dict(synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=gm), strict=True)
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device=dev)
    shape = (B, 4, R, R, R)
    mask = gm.view(1, R, R, R).to(dev)
    gm_flat = gm.reshape(-1).float().to(dev).contiguous()
    model_fn = mutils.get_model_fn(model, train=False)
    g = torch.Generator().manual_seed(1)
    y = torch.sign(torch.randn((R, R, R), generator=g))
    pm = (torch.rand((R, R, R), generator=g) < 0.3).float() * gm.view(R, R, R)
    x_T = torch.randn(shape, generator=g).to(dev)
    lines = [f"DPM-Solver++ sampler, ddpm_res64 {R}^3, B = {B}; median [min .. max] of {args.reps} after {args.warmup} warm-up "
             f"repetitions, alternatives interleaved; {torch.cuda.get_device_name(0)}"]

    def say(name, t, note=""):
        lines.append(f"{name:<72s} {t[0]:10.3f} ms  [{t[1]:.3f} .. {t[2]:.3f}]{note}")
        print(lines[-1], flush=True)

    with torch.no_grad():
        # ---- one step of each sampler, at the middle of its schedule
        times = sampling.dpmpp_schedule(sde, steps)
        rows, labels = sampling.dpmpp_tables(sde, times, order=2)
        i = steps // 2
        coef = rows[i].to(dev).expand(B, 8).contiguous()
        lab = labels[i].float().to(dev).expand(B).contiguous()
        x64 = (x_T * mask).double().contiguous()
        x32 = x64.float()
        h1, h2 = x64 * 0.5, x64 * 0.25
        z = torch.randn_like(x32)
        out = (torch.empty_like(x64), torch.empty_like(x64), torch.empty_like(x32))
        pred = sampling.DDIMPredictor(sde, None)
        ts = sampling.ddim_schedule(sde.N)
        j = len(ts) // 2
        vt, vp = torch.ones(B, device=dev) * ts[j], torch.ones(B, device=dev) * ts[j - 1]
        dcoef = pred.coefficients(vt, vp)
        dlab = vt.float() * (sde.N - 1)

        def step_dpmpp():
            return ops.multistep_step(x64, model_fn(x32, lab), (h1,), None, gm_flat, coef, out=out)

        def step_ddim():
            return ops.ddim_step(x64, model_fn(x32, dlab), gm_flat, dcoef)
        t_a, t_b = timed_alternating(step_dpmpp, step_ddim, args.reps, args.warmup, 1)
        say("one dpmpp step (U-Net evaluation + md_multistep_step, order 2)", t_a)
        say("one ddim step (U-Net evaluation + md_ddim_step)", t_b)
        t_step = t_a[0]

        # ---- the update alone
        eps = torch.randn_like(x32)
        coef3 = sampling.dpmpp_tables(sde, times, order=3, tau=1)[0][i].to(dev).expand(B, 8).contiguous()

        def upd2():
            return ops.multistep_step(x64, eps, (h1,), None, gm_flat, coef, out=out)

        def upd3():
            return ops.multistep_step(x64, eps, (h1, h2), z, gm_flat, coef3, out=out)
        t_2, t_3 = timed_alternating(upd2, upd3, args.reps, args.warmup, args.inner)
        for name, t, nh, hz in (("order 2, tau 0", t_2, 1, False), ("order 3, tau 1", t_3, 2, True)):
            nbytes = update_bytes(B, 4, P, nh, hz, True)
            rate = nbytes / (t[0] * 1e-3) / 1e12
            say(f"md_multistep_step alone ({name}; windows of {args.inner} calls)", t,
                f"   {nbytes / 1e6:.1f} MB -> {rate:.2f} TB/s = {100 * rate / HBM_MEASURED_TBS:.0f} % of the measured HBM copy rate "
                f"({HBM_MEASURED_TBS} TB/s; {100 * rate / HBM_SPEC_TBS:.0f} % of the {HBM_SPEC_TBS} TB/s datasheet peak); "
                f"{100 * t[0] / t_step:.2f} % of a step")

        # ---- whole runs
        dp = sampling.get_dpmpp_sampler(sde, shape, lambda v: v, steps=steps, order=2, device=dev, grid_mask=mask)
        dd = sampling.get_ddim_sampler(sde, shape, sampling.get_predictor("ddim"), lambda v: v, device=dev, grid_mask=mask)
        t_a, t_b = wall_alternating(lambda: dp(model, x0=x_T), lambda: dd(model, x0=x_T), args.reps,
                                    warm=(lambda: dp(model, x0=x_T, n_iters=2), lambda: dd(model, x0=x_T, n_iters=2)))
        say(f"{steps} dpmpp steps (whole sampler call, host wall time)", t_a)
        say("the 99-evaluation DDIM run (likewise)", t_b, f"   {t_b[0] / t_a[0]:.2f} x the dpmpp run")
        kw = dict(partial=y, partial_mask=pm, partial_channel=0, guidance_scale=1.0)
        t_a, t_b = wall_alternating(lambda: dp(model, x0=x_T, **kw), lambda: dd(model, x0=x_T, n_iters=steps, **kw), args.reps,
                                    warm=(lambda: dp(model, x0=x_T, n_iters=2, **kw), lambda: dd(model, x0=x_T, n_iters=2, **kw)))
        say(f"{steps} guided dpmpp steps (zeta = 1, replacement on; host wall time)", t_a)
        say(f"{steps} guided DDIM steps (likewise)", t_b)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
