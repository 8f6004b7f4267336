"""Times classifier-free guidance at res64, B = 8, on the GPU (device events around windows of calls, after warm-up):
  * hip_ops.cfg_combine (md_cfg_combine) on a [2B, 4, 64, 64, 64] evaluation, without and with the guidance rescale
    (+ md_cfg_rescale), beside the same expressions in plain torch, alternating; the bytes each moves computed here from the
    shapes over its time, beside the measured HBM copy rate of MI355X_MICROARCH.md (6.29 TB/s; 8.0 TB/s is the datasheet's);
  * one DDIM step (U-Net evaluation + md_ddim_step) through sampling.ClassifierFreeModel at cfg_scale 1 (one evaluation at
    batch B) and at cfg_scale 3 (one evaluation at batch 2B + the combine), alternating.
The doubled evaluation dominates a guided step; no other figure is expected of this tool before it has run.

    python tools/bench_cfg.py [--batch 8] [--reps 5] [--inner 20] [--step-inner 3] [--out profiles/cfg_bench.txt]

The weights are the synthetic sensitised ones (synth.sensitised_state_dict) at model.num_classes = 3: the times do not depend on
them.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_likelihood import timed_alternating  # noqa: E402

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0


def torch_combine(eps2, w, phi=0.0):
    """The same guidance in plain torch, float32: eu + w (ec - eu), and the rescale with torch's own std over each sample."""
    B = eps2.shape[0] // 2
    ec, eu = eps2[:B], eps2[B:]
    out = eu + w.view(B, 1, 1, 1, 1) * (ec - eu)
    if phi > 0.0:
        f = phi * ec.flatten(1).std(dim=1, unbiased=False) / out.flatten(1).std(dim=1, unbiased=False) + (1.0 - phi)
        out = out * f.view(B, 1, 1, 1, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--step-inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfg_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cfg.py measures on the GPU: none found")
    from meshdiffusion_amd import config as mdc, hip_ops as ops, synth
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401

    cfg = mdc.get_config_res64()
    cfg.device = dev = torch.device("cuda", 0)
    cfg.model.num_classes = 3
    R, B, Cc = cfg.data.image_size, args.batch, cfg.data.num_channels
    n = Cc * R ** 3
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()

    def say(text):
        print(text, flush=True)
        with open(args.out, "a") as f:           # line by line: a run that is cut short keeps what it measured
            f.write(text + "\n")

    def row(name, t, note=""):
        say(f"{name:<78s} {t[0]:10.3f} ms  [{t[1]:.3f} .. {t[2]:.3f}]{note}")

    def rate(nbytes, ms):
        r = nbytes / (ms * 1e-3) / 1e12
        return (f"   {nbytes / 1e6:.1f} MB -> {r:.2f} TB/s = {100 * r / HBM_MEASURED_TBS:.0f} % of the measured HBM copy rate "
                f"({HBM_MEASURED_TBS} TB/s; {100 * r / HBM_SPEC_TBS:.0f} % of the {HBM_SPEC_TBS} TB/s datasheet peak)")

    say(f"classifier-free guidance, ddpm_res64 {R}^3, B = {B}; median [min .. max] of {args.reps} windows after {args.warmup} warm-up "
        f"repetitions; {torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        # ---- the combine, without and with the rescale
        g = torch.Generator().manual_seed(1)
        eps2 = torch.randn((2 * B, Cc, R, R, R), generator=g).to(dev)
        w = torch.full((B,), 3.0, device=dev)
        t_hip, t_torch = timed_alternating(lambda: ops.cfg_combine(eps2, w), lambda: torch_combine(eps2, w), args.reps, args.warmup,
                                           args.inner)
        row(f"hip_ops.cfg_combine: md_cfg_combine (windows of {args.inner} calls)", t_hip,
            rate(3 * B * n * 4, t_hip[0]) + "; 2 reads, 1 write per value; the same tensors in every call: what of them stays in "
            "the last-level cache is not HBM traffic")
        row("eu + w (ec - eu) in plain torch, float32 (likewise)", t_torch, f"   {t_torch[0] / t_hip[0]:.1f} x the HIP launch")
        t_hip, t_torch = timed_alternating(lambda: ops.cfg_combine(eps2, w, rescale=0.7), lambda: torch_combine(eps2, w, 0.7), args.reps,
                                           args.warmup, args.inner)
        row("hip_ops.cfg_combine(rescale=0.7): md_cfg_combine with slab sums + md_cfg_rescale", t_hip,
            rate(5 * B * n * 4, t_hip[0]) + "; 2 reads, 1 write, then 1 read, 1 write per value")
        row("the same with torch's std per sample, float32", t_torch, f"   {t_torch[0] / t_hip[0]:.1f} x the HIP pair")
        a, b = ops.cfg_combine(eps2, w, rescale=0.7), torch_combine(eps2, w, 0.7)
        say(f"  the two agree to rel-L2 {float((a.double() - b.double()).norm() / b.double().norm()):.2e} (the torch chain is float32 throughout)")
        del eps2, a, b

        # ---- one DDIM step at cfg_scale 1 and 3
        gm = synth.synthetic_grid_mask(R)
        model = mutils.create_model(cfg).eval()
        model.module.load_state_dict(synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=gm), strict=True)
        sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device=dev)
        gm_flat = gm.reshape(-1).float().to(dev).contiguous()
        pred = sampling.DDIMPredictor(sde, None)
        y = torch.arange(B) % cfg.model.num_classes
        x = (synth.synthetic_inputs(B, Cc, R, seed=8).to(dev) * gm.view(1, 1, R, R, R).to(dev)).double()
        t = torch.full((B,), 0.5, device=dev)
        tprev = torch.full((B,), 0.48, device=dev)
        one = sampling.ClassifierFreeModel(model, y, scale=1.0)
        three = sampling.ClassifierFreeModel(model, y, scale=3.0)
        step = lambda m: pred.update_fn(x, t, tprev, model=m, mask=gm_flat)     # noqa: E731
        t1, t3 = timed_alternating(lambda: step(one), lambda: step(three), args.reps, args.warmup, args.step_inner)
        row(f"one DDIM step, cfg_scale 1: one evaluation at batch {B} (windows of {args.step_inner})", t1)
        row(f"one DDIM step, cfg_scale 3: one evaluation at batch {2 * B} + md_cfg_combine", t3,
            f"   {t3[0] / t1[0]:.2f} x the step at cfg_scale 1: the doubled evaluation dominates")


if __name__ == "__main__":
    main()
