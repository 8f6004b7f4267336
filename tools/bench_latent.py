"""Times latent interpolation at res64, B = 8, on the GPU (device events around synchronised work, after warm-up; whole sampler
calls by the host clock around a synchronise):
  * hip_ops.slerp (md_slerp_dots + md_slerp_mix) with K = 8 on B / 2 pairs beside the same formula in plain torch, alternating;
    the bytes it moves computed here from the shapes -- a and b read twice (once per launch), K rows written, the [P] mask twice --
    over its time, beside the measured HBM copy rate of MI355X_MICROARCH.md (6.29 TB/s; 8.0 TB/s is the datasheet's);
  * one DDIM encode (ddim_sampler(encode=True), 99 evaluations) and one ODE encode (ode_sampler(encode=True), rtol = atol = 1e-5);
  * the round trips decode(encode(x)) against x as rel-L2, for both, x = synthetic grids on the mask;
  * one evaler.interp run with K = 8 (the model handed over in memory instead of a checkpoint: calibration + slerp + decode).

    python tools/bench_latent.py [--batch 8] [--reps 5] [--inner 20] [--no-ode] [--out profiles/latent_bench.txt]

The weights are the synthetic sensitised ones (synth.sensitised_state_dict): the times do not depend on them; the round-trip
figures do, and say nothing about a trained checkpoint.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_likelihood import timed_alternating  # noqa: E402

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0


def torch_slerp(a, b, alphas, mask):
    """The reference's formula (evaler.py:63-71) per pair and position in the tensors' float32, on the masked endpoints."""
    am, bm = a * mask, b * mask
    rows = []
    for p in range(a.shape[0]):
        theta = torch.acos(torch.sum(am[p] * bm[p]) / (torch.norm(am[p]) * torch.norm(bm[p])))
        rows.append(torch.stack([torch.sin((1 - al) * theta) / torch.sin(theta) * am[p] + torch.sin(al * theta) / torch.sin(theta) * bm[p]
                                 for al in alphas]))
    return torch.stack(rows)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), out


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-ode", action="store_true", help="skip the two ODE solves (about a minute each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent.py measures on the GPU: none found")
    from meshdiffusion_amd import config as mdc, hip_ops as ops, synth
    from meshdiffusion_amd.lib.diffusion import evaler, sampling, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401

    cfg = mdc.get_config_res64()
    cfg.device = dev = torch.device("cuda", 0)
    R, B, K = cfg.data.image_size, args.batch, args.points
    P, Cc, pairs = R ** 3, cfg.data.num_channels, args.batch // 2
    gm = synth.synthetic_grid_mask(R)
    model = mutils.create_model(cfg).eval()
    model.module.load_state_dict(synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=gm), strict=True)
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device=dev)
    shape = (B, Cc, R, R, R)
    mask = gm.view(1, R, R, R).to(dev)
    gm_flat = gm.reshape(-1).float().to(dev).contiguous()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    head = (f"latent interpolation, ddpm_res64 {R}^3, B = {B} ({pairs} pairs), K = {K}; median [min .. max] of {args.reps} after "
             f"{args.warmup} warm-up repetitions; {torch.cuda.get_device_name(0)}")

    def say(text):
        print(text, flush=True)
        with open(args.out, "a") as f:           # line by line: a run that is cut short keeps what it measured
            f.write(text + "\n")

    def row(name, t, note=""):
        say(f"{name:<72s} {t[0]:10.3f} ms  [{t[1]:.3f} .. {t[2]:.3f}]{note}")

    say(head)
    with torch.no_grad():
        # ---- the slerp
        g = torch.Generator().manual_seed(1)
        lat = torch.randn(shape, generator=g).to(dev)
        a, b = lat[0::2].contiguous(), lat[1::2].contiguous()
        alphas = torch.arange(K, dtype=torch.float64, device=dev) / (K - 1)
        al32 = [float(v) for v in alphas]
        m5 = gm_flat.view(1, R, R, R)
        t_hip, t_torch = timed_alternating(lambda: ops.slerp(a, b, alphas, gm_flat), lambda: torch_slerp(a, b, al32, m5), args.reps,
                                           args.warmup, args.inner)
        nbytes = pairs * Cc * P * 4 * (4 + K) + 2 * 4 * P
        rate = nbytes / (t_hip[0] * 1e-3) / 1e12
        row(f"hip_ops.slerp: md_slerp_dots + md_slerp_mix (windows of {args.inner} calls)", t_hip,
            f"   {nbytes / 1e6:.1f} MB (2 + 2 reads, {K} writes per value) -> {rate:.2f} TB/s = {100 * rate / HBM_MEASURED_TBS:.0f} % of the "
            f"measured HBM copy rate ({HBM_MEASURED_TBS} TB/s; {100 * rate / HBM_SPEC_TBS:.0f} % of the {HBM_SPEC_TBS} TB/s datasheet peak); the same tensors in every "
            f"call: what of them stays in the last-level cache is not HBM traffic")
        row("the same formula in plain torch, float32 (likewise)", t_torch, f"   {t_torch[0] / t_hip[0]:.1f} x the HIP pair")
        got, want = ops.slerp(a, b, alphas, gm_flat)[0], torch_slerp(a, b, al32, m5)
        say(f"  the two agree to rel-L2 {rel_l2(got, want):.2e} (the torch chain is float32 throughout)")

        # ---- encoders and round trips
        x = (synth.synthetic_inputs(B, Cc, R, seed=8) * 0.5).to(dev) * mask
        ddim = sampling.get_ddim_sampler(sde, shape, sampling.get_predictor("ddim"), lambda v: v, device=dev, grid_mask=mask)
        ddim(model, x0=x, encode=True, n_iters=2), ddim(model, x0=x, n_iters=2)              # warm-up: weight packs, allocator
        t_enc, (z, _) = wall(lambda: ddim(model, x0=x, encode=True))
        t_dec, (back, _) = wall(lambda: ddim(model, x0=z))
        say(f"one DDIM encode (99 evaluations, whole call, host wall time)            {t_enc:10.1f} ms; the decode {t_dec:.1f} ms")
        say(f"  DDIM round trip decode(encode(x)) vs x: rel-L2 {rel_l2(back, x):.3e}; |z| / |x| = {float(z.norm() / x.double().norm()):.3f} "
            f"(synthetic weights: this network's flow expands strongly on the way back, as tools/gen_golden_likelihood.py records; no figure for a trained checkpoint)")
        # ---- the whole driver, the model handed over in memory (no checkpoint file is read)
        with tempfile.TemporaryDirectory() as tmp:
            evaler._load_model = lambda config: (model, sde)
            evaler._grid_mask = lambda config, shp: gm.view(*shp).to(dev)
            cfg.eval.eval_dir = os.path.join(tmp, "out")
            cfg.eval.interp_points, cfg.sampling.method = K, "ddim"
            t_run, out = wall(lambda: evaler.interp(cfg))
            say(f"one evaler.interp run (noise endpoints, K = {K}, method ddim: calibration at batch {K} + slerp + 99-evaluation decode + "
                f"writing the .npy; host wall time) {t_run:.1f} ms; output {tuple(out.shape)}")

        # ---- the ODE route, last: the two solves take about a minute each
        if not args.no_ode:
            ode = sampling.get_ode_sampler(sde, shape, lambda v: v, rtol=1e-5, atol=1e-5, device=dev, grid_mask=mask)
            t_enc, (zo, nfe_e) = wall(lambda: ode(model, x0=x, encode=True))
            say(f"one ODE encode (rtol = atol = 1e-5: {nfe_e} evaluations, whole call, host wall time)   {t_enc:10.1f} ms; "
                f"|z| / |x| = {float(zo.double().norm() / x.double().norm()):.3f}")
            t_dec, (backo, nfe_d) = wall(lambda: ode(model, x0=zo))
            say(f"  its decode: {nfe_d} evaluations, {t_dec:.1f} ms; ODE round trip decode(encode(x)) vs x: rel-L2 {rel_l2(backo, x):.3e} (likewise)")


if __name__ == "__main__":
    main()
