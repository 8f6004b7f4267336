"""Predictor-corrector sampling cost at the headline shape (res64, B = 8, calibrated model), one process:
  * the Langevin corrector's own kernels (md_langevin_norms + md_langevin_step) in ms and GB/s, against the same update
    written as the reference's torch chain (sampling.py:280-286 plus the mask of :450);
  * one (ancestral_sampling, langevin) iteration against one ancestral_sampling iteration (the sampler loop bodies of
    lib/diffusion/sampling.py get_pc_sampler).
Device events after warm-up; the variants alternate round by round and each figure is the median over rounds.
    python tools/bench_pc.py [--batch 8] [--rounds 7] [--reps 20] [--iters 3] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(variants, rounds, reps):
    """{name: median ms per call} with the variants alternating inside every round."""
    out = {k: [] for k in variants}
    for r in range(rounds):
        order = list(variants) if r % 2 == 0 else list(reversed(list(variants)))
        for k in order:
            out[k].append(timed(variants[k], reps))
    return {k: statistics.median(v) for k, v in out.items()}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="corrector launches per timed window")
    ap.add_argument("--iters", type=int, default=3, help="sampler iterations per timed window")
    ap.add_argument("--snr", type=float, default=0.075)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pc.py needs a GPU: the HIP path has no CPU fallback")
    from meshdiffusion_amd import hip_ops as ops, synth
    from meshdiffusion_amd.config import get_config_res64
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401

    dev = torch.device("cuda")
    cfg = get_config_res64(); cfg.device = dev
    R, B, C = cfg.data.image_size, a.batch, cfg.data.num_channels
    shape = (B, C, R, R, R)
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device=dev)
    mask = synth.synthetic_grid_mask(R).view(1, R, R, R).to(dev)
    st = sampling.AncestralStepper(sde, shape, eps=1e-3, device=dev, grid_mask=mask)
    gm = st.gm_flat
    _, ccoef = sampling._pc_tables(sde, st.timesteps, B, sampling.AncestralSamplingPredictor, sampling.LangevinCorrector,
                                   a.snr, False)

    # ---- the corrector's own kernels vs the reference's torch chain (same x / eps / z / coefficients) ----
    g = torch.Generator().manual_seed(7)
    x, eps, z = ((torch.randn(shape, generator=g) * (mask.cpu() if k == 0 else 1)).to(dev) for k in range(3))
    coef = ccoef[500]
    sigma, alpha = coef[:, 0], coef[:, 1]
    b5 = (slice(None),) + (None,) * 4
    gm5 = mask.view(1, 1, R, R, R)

    def hip_corrector():
        return ops.langevin_step(x, eps, z, gm, coef, a.snr)

    def torch_corrector():
        grad = -eps / sigma[b5]
        gn = torch.norm(grad.reshape(B, -1), dim=-1).mean()
        nn_ = torch.norm(z.reshape(B, -1), dim=-1).mean()
        step = (a.snr * nn_ / gn) ** 2 * 2 * alpha
        x_mean = x + step[b5] * grad
        xn = x_mean + torch.sqrt(step * 2)[b5] * z
        return xn * gm5, x_mean * gm5

    with torch.no_grad():
        xh, xmh, _ = hip_corrector()
        xt, xmt = torch_corrector()
        agree = max(float((xh - xt).abs().max()), float((xmh - xmt).abs().max()))
        for _ in range(3):
            hip_corrector(); torch_corrector()
        torch.cuda.synchronize()
        med_c, raw_c = interleaved({"hip": hip_corrector, "torch": torch_corrector}, a.rounds, a.reps)
    n = B * C * R ** 3
    # md_langevin_norms reads eps, z; md_langevin_step reads x, eps, z (+ the [P] mask) and writes x, x_mean
    nbytes = 4 * (2 * n + 3 * n + 2 * n) + 4 * R ** 3
    print(f"corrector kernels (md_langevin_norms + md_langevin_step) B={B}: {med_c['hip']:.4f} ms "
          f"{nbytes / med_c['hip'] / 1e6:.0f} GB/s  | reference torch chain {med_c['torch']:.4f} ms  "
          f"| max |hip - torch| {agree:.2e}", flush=True)

    # ---- one PC iteration vs one ancestral iteration on the calibrated model ----
    model = mutils.create_model(cfg).eval()
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    del sd
    mutils.calibrate_model(model, cfg, batch=B)
    model_fn = mutils.get_model_fn(model, train=False)
    state = {"x": x.clone()}

    def ancestral_iter():
        xs = state["x"]
        for i in range(a.iters):
            xs, _ = st.step(model_fn, xs, i)
        state["x"] = xs

    def pc_iter():                                    # get_pc_sampler's loop body for (ancestral_sampling, langevin)
        xs = state["x"]
        for i in range(a.iters):
            e = model_fn(xs, st.labels[i])
            zz = torch.randn_like(xs)
            xs, _, _ = ops.langevin_step(xs, e, zz, gm, ccoef[i], a.snr, "langevin")
            xs, _ = st.step(model_fn, xs, i)
        state["x"] = xs

    with torch.no_grad():
        torch.manual_seed(3)
        for _ in range(2):
            ancestral_iter(); pc_iter()
            state["x"] = x.clone()
        torch.cuda.synchronize()
        med_i, raw_i = {}, {"ancestral": [], "pc": []}
        for r in range(a.rounds):
            order = ("ancestral", "pc") if r % 2 == 0 else ("pc", "ancestral")
            for k in order:
                state["x"] = x.clone()
                raw_i[k].append(timed(ancestral_iter if k == "ancestral" else pc_iter, 1) / a.iters)
        med_i = {k: statistics.median(v) for k, v in raw_i.items()}
    ratio = med_i["pc"] / med_i["ancestral"]
    print(f"sampler iteration B={B}: ancestral_sampling {med_i['ancestral']:.2f} ms | ancestral_sampling + langevin "
          f"{med_i['pc']:.2f} ms (x{ratio:.3f}; budget 2 x ancestral + 0.3 ms = {2 * med_i['ancestral'] + 0.3:.2f} ms)",
          flush=True)
    rec = {"batch": B, "shape": list(shape), "rounds": a.rounds,
           "corrector_kernels_ms": round(med_c["hip"], 5), "corrector_kernels_GBps": round(nbytes / med_c["hip"] / 1e6, 1),
           "corrector_torch_chain_ms": round(med_c["torch"], 5), "corrector_bytes": nbytes,
           "iteration_ancestral_ms": round(med_i["ancestral"], 3), "iteration_pc_langevin_ms": round(med_i["pc"], 3),
           "raw": {"corrector": raw_c, "iteration": raw_i}}
    print(json.dumps({k: v for k, v in rec.items() if k != "raw"}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
