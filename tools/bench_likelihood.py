"""Times one right-hand-side evaluation of the likelihood ODE at res64, B = 8, on the GPU (device events, median of --reps after
--warmup un-timed repetitions), split into
  * the taped forward (eval mode, x.requires_grad),
  * the data-gradient-only backward (param_grads=False) and, for comparison, the full backward with every weight gradient
    (what the network could do before the input gradient existed),
  * md_conv3_stem_dgrad + md_fold_dx against the stem gradient on the generic route (bf16 split + dx-folded tile + md_fold_dx),
  * md_pf_ode_rhs with the divergence,
and, with --solve, runs one whole likelihood solve at --rtol (= atol) and records its nfe and wall time.

    python tools/bench_likelihood.py [--batch 8] [--reps 5] [--solve --rtol 1e-5] [--out profiles/likelihood_bench.txt]

profiles/likelihood_bench.txt is the output of one run with --solve.  The two stem routes are timed in alternating windows of 100
calls, md_pf_ode_rhs in windows of 2000 calls (a single call is tens of microseconds).

The weights are the synthetic sensitised ones (synth.sensitised_state_dict): the times do not depend on them, the nfe of a solve
does -- it is the figure of THIS synthetic network, not of a trained checkpoint.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, inner):
    """Device time of `inner` back-to-back calls of fn() in ms per call; fn's last result."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner, out


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def timed(fn, reps, warmup, inner=1):
    """Median / min / max device time of fn() in ms over `reps` windows of `inner` calls each; fn's result of the last call."""
    out = None
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(reps):
        t, out = window(fn, inner)
        ms.append(t)
    return stats(ms), out


def timed_alternating(fa, fb, reps, warmup, inner):
    """Two versions of one thing in alternating windows (a, b, a, b, ...) of `inner` calls: they see the same machine state."""
    for _ in range(warmup):
        fa(), fb()
    ma, mb = [], []
    for _ in range(reps):
        ma.append(window(fa, inner)[0])
        mb.append(window(fb, inner)[0])
    return stats(ma), stats(mb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--rtol", type=float, default=1e-5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_likelihood.py measures on the GPU: none found")
    from meshdiffusion_amd import config as mdc, hip_ops as ops, synth
    from meshdiffusion_amd.lib.diffusion import likelihood, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import backward as bw, ddpm_res64, utils as mutils  # noqa: F401

    cfg = mdc.get_config_res64()
    cfg.device = dev = torch.device("cuda", 0)
    R, B = cfg.data.image_size, args.batch
    gm = synth.synthetic_grid_mask(R)
    model = mutils.create_model(cfg).eval()
    model.module.load_state_dict(synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=gm), strict=True)
    net = model.module
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device=dev)
    mask = gm.view(1, 1, R, R, R).to(dev)
    x = (synth.synthetic_inputs(B, 4, R, seed=8).to(dev) * mask * 0.5).contiguous()
    probe = ((torch.randint(0, 2, x.shape, generator=torch.Generator().manual_seed(1)).float() * 2 - 1).to(dev) * mask).contiguous()
    labels = torch.full((B,), 0.5 * (sde.N - 1), device=dev)
    lines = [f"likelihood right-hand side, ddpm_res64 {R}^3, B = {B}, bf16x3; device events, median [min .. max] of {args.reps} "
             f"after {args.warmup} warm-up repetitions; {torch.cuda.get_device_name(0)}"]

    def say(name, t, note=""):
        lines.append(f"{name:<58s} {t[0]:9.3f} ms  [{t[1]:.3f} .. {t[2]:.3f}]{note}")
        print(lines[-1], flush=True)

    with torch.no_grad():
        t_fwd, _ = timed(lambda: net.forward_train(x, labels), args.reps, args.warmup)
        say("taped forward (forward_train)", t_fwd)

        def fwd_bwd(**kw):
            _, ctx = net.forward_train(x, labels)
            return net.backward(ctx, probe, **kw)
        t_vjp, g = timed(lambda: fwd_bwd(input_grad=True, param_grads=False), args.reps, args.warmup)
        say("taped forward + data-gradient-only backward", t_vjp, f"   backward alone {t_vjp[0] - t_fwd[0]:.3f} ms")
        t_full, _ = timed(lambda: fwd_bwd(input_grad=True, param_grads=True), args.reps, args.warmup)
        say("taped forward + full backward (with weight gradients)", t_full, f"   backward alone {t_full[0] - t_fwd[0]:.3f} ms"
            " (incl. the weight re-pack its parameter-epoch bump causes in the next forward)")
        for p in net.parameters():
            p.grad = None
        # the stem's data gradient: the kernel against the generic route, on a gradient tensor of h0's shape
        g0 = ops.ncdhw_to_f32b(torch.randn((B, net.nf, R, R, R), device=dev))
        stem = net.all_modules[2]
        ok = ops.conv3_stem_dgrad_ok

        def generic():
            ops.conv3_stem_dgrad_ok = lambda *a: False
            try:
                return net._stem_dgrad(stem, g0, B, R)
            finally:
                ops.conv3_stem_dgrad_ok = ok
        with ops.precision_scope(None, training=True):
            t_k, t_g = timed_alternating(lambda: net._stem_dgrad(stem, g0, B, R), generic, args.reps, args.warmup, inner=100)
        say("stem data gradient: md_conv3_stem_dgrad + md_fold_dx", t_k, "   (windows of 100 calls, alternating with the next line)")
        say("stem data gradient: split + generic dx-folded tile + md_fold_dx", t_g)
        eps_hat = torch.randn_like(x)
        cx, ce = likelihood.vp_coefficients(sde, 0.5)
        coef = torch.tensor([[cx, ce]] * B, dtype=torch.float64, device=dev)
        m32 = gm.reshape(-1).float().to(dev)
        t_r, _ = timed(lambda: ops.pf_ode_rhs(x, eps_hat, m32, coef, g=g, probe=probe), args.reps, args.warmup, inner=2000)
        nbytes = 5 * x.numel() * 4
        say("md_pf_ode_rhs with divergence (+ the 64-slab sum)", t_r,
            f"   (windows of 2000 calls on the same {nbytes / 1e6:.0f} MB of tensors, which stay in the last-level cache: not an HBM figure)")
    lines.append(f"one right-hand-side evaluation = taped forward + data-gradient-only backward + md_pf_ode_rhs: "
                 f"{t_vjp[0] + t_r[0]:.1f} ms; with the full backward instead: {t_full[0] + t_r[0]:.1f} ms")
    print(lines[-1], flush=True)
    if args.solve:
        fn = likelihood.get_likelihood_fn(sde, lambda v: v, rtol=args.rtol, atol=args.rtol, eps=1e-3, grid_mask=gm)
        torch.cuda.synchronize()
        t0 = time.time()
        bpd, _, nfe = fn(model, x, probe=probe)
        torch.cuda.synchronize()
        dt = time.time() - t0
        lines.append(f"whole solve t in [1e-3, 1], rtol = atol = {args.rtol:g}, this synthetic network: nfe {nfe}, {dt:.1f} s wall "
                     f"({1e3 * dt / nfe:.1f} ms per evaluation incl. the integrator), bits/dim {[round(float(v), 4) for v in bpd]}")
        print(lines[-1], flush=True)
    else:
        lines.append("whole solve: not run (--solve)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
