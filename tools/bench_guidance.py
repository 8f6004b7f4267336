"""Times one guided ancestral step (reconstruction guidance, sampling.guidance_terms) at res64, B = 8, on the GPU (device events,
median of --reps after --warmup un-timed repetitions), split into
  * the taped forward (eval mode, x.requires_grad),
  * the data-gradient-only backward (taped forward + backward, minus the forward),
  * md_guide_residual and md_guide_apply_f32 (windows of 2000 calls: a single call is tens of microseconds),
  * the whole guided step as pc_sampler runs it: guidance_terms + md_ancestral_step + md_guide_apply_f32,
beside the unguided inference step (eval-mode forward + md_ancestral_step) in the same process.

    python tools/bench_guidance.py [--batch 8] [--reps 5] [--chunk N] [--out profiles/guidance_bench.txt]

profiles/guidance_bench.txt is the output of one run.  The weights are the synthetic sensitised ones
(synth.sensitised_state_dict): the times do not depend on them.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_likelihood import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=None, help="samples per taped forward and backward (default: the whole batch)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guidance.py measures on the GPU: none found")
    from meshdiffusion_amd import config as mdc, hip_ops as ops, synth
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401

    cfg = mdc.get_config_res64()
    cfg.device = dev = torch.device("cuda", 0)
    R, B = cfg.data.image_size, args.batch
    gm = synth.synthetic_grid_mask(R)
    model = mutils.create_model(cfg).eval()
    model.module.load_state_dict(synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=gm), strict=True)
    net = model.module
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device=dev)
    shape = (B, 4, R, R, R)
    st = sampling.AncestralStepper(sde, shape, device=dev, grid_mask=gm)
    i = sde.N // 2                                       # the middle iteration's level
    mask = gm.view(1, 1, R, R, R).to(dev)
    x = (synth.synthetic_inputs(B, 4, R, seed=8).to(dev) * mask * 0.5).contiguous()
    g = torch.Generator().manual_seed(1)
    y = torch.sign(torch.randn(R ** 3, generator=g)).to(dev)
    pm = ((torch.rand(R ** 3, generator=g) < 0.3).float() * gm.reshape(-1)).to(dev)
    gm_flat = st.gm_flat
    k = int((st.timesteps[i] * (sde.N - 1) / sde.T).long())
    alpha, sigma = float(sde.sqrt_alphas_cumprod[k]), float(sde.sqrt_1m_alphas_cumprod[k])
    coef2 = torch.tensor([[alpha, sigma]] * B, dtype=torch.float64, device=dev)
    coef3 = torch.tensor([[alpha, sigma, 1.0]] * B, dtype=torch.float64, device=dev)
    labels = st.labels[i]
    model_fn = mutils.get_model_fn(model, train=False)
    lines = [f"one guided ancestral step, ddpm_res64 {R}^3, B = {B}; device events, median [min .. max] of {args.reps} after "
             f"{args.warmup} warm-up repetitions; {torch.cuda.get_device_name(0)}"]

    def say(name, t, note=""):
        lines.append(f"{name:<66s} {t[0]:9.3f} ms  [{t[1]:.3f} .. {t[2]:.3f}]{note}")
        print(lines[-1], flush=True)

    with torch.no_grad():
        t_fwd, _ = timed(lambda: net.forward_train(x, labels), args.reps, args.warmup)
        say("taped forward (eval mode, bf16x3)", t_fwd)
        cot0 = (torch.randn(shape, device=dev) * mask).contiguous()

        def fwd_bwd():
            _, ctx = net.forward_train(x, labels)
            return net.backward(ctx, cot0, input_grad=True, param_grads=False)
        t_vjp, gx = timed(fwd_bwd, args.reps, args.warmup)
        say("taped forward + data-gradient-only backward", t_vjp, f"   backward alone {t_vjp[0] - t_fwd[0]:.3f} ms")
        eps_hat = torch.randn_like(x)
        t_res, (cot, slabs) = timed(lambda: ops.guide_residual(x, eps_hat, y, pm, gm_flat, coef2, 0), args.reps, args.warmup, inner=2000)
        say("md_guide_residual (cotangent + 64 slab sums per sample)", t_res, "   (windows of 2000 calls, tensors stay in the "
            "last-level cache: not an HBM figure)")
        xa, xm = x.clone(), x.clone()
        t_app, _ = timed(lambda: ops.guide_apply_(xa, xm, cot, gx, gm_flat, coef3, slabs), args.reps, args.warmup, inner=2000)
        say("md_guide_apply_f32 on (x, x_mean)", t_app, "   (likewise)")

        def guided():
            e, c, gg, sl = sampling.guidance_terms(model, coef2, x, labels, None, None, y, pm, gm_flat, 0, chunk=args.chunk)
            z = torch.randn_like(x)
            xn, xmn = ops.ancestral_step(x, e, z, gm_flat, st.coef[i])
            ops.guide_apply_(xn, xmn, c, gg, gm_flat, coef3, sl)
            return xn
        t_g, _ = timed(guided, args.reps, args.warmup)
        say("guided step: guidance_terms + md_ancestral_step + md_guide_apply_f32", t_g,
            f"   chunk {args.chunk or B}")
        t_u, _ = timed(lambda: st.step(model_fn, x, i), args.reps, args.warmup)
        say(f"unguided inference step ({net.hip_precision} forward + md_ancestral_step)", t_u)
    assert all(p.grad is None for p in net.parameters())
    lines.append(f"a guided step costs {t_g[0] / t_u[0]:.2f} x the unguided one; the two guidance kernels are "
                 f"{1e3 * (t_res[0] + t_app[0]):.0f} us of its {t_g[0]:.1f} ms")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
