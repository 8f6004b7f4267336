"""Generate the predictor-corrector sampler fixtures in tests/golden/ by running the UNMODIFIED reference
`get_sampling_fn` on CPU, imported from the reference checkout the way oracle/gen_golden.py does (build host only:
the GPU machines have no reference):
    python tools/gen_golden_pc.py [--skip-res64]

  sampler_pc_small.npz  small config, B = 2, first K = 6 iterations of every case in CASES (live cells of the
                        grid mask: the sampler zeroes every other cell, which the GPU test checks separately)
  sampler_pc_res64.npz  res64, B = 2, first K = 3 iterations of (ancestral_sampling, langevin): sample_stats + one row

Before anything is written, an in-script torch restatement of the PC loop driven by oracle.unet_oracle is asserted to
agree with the reference to <= 1e-5 (the pin that lets the GPU tests trust these numbers).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from meshdiffusion_amd import synth  # noqa: E402
from oracle import unet_oracle  # noqa: E402
from oracle.gen_golden import (GOLD, import_reference, live_cells, make_sd, ref_model, rel_l2,  # noqa: E402
                               run_ref_sampler, sample_stats)

# name -> (predictor, corrector, snr, n_steps_each, probability_flow, seed, conditional)
CASES = {
    "anc_langevin": ("ancestral_sampling", "langevin", 0.075, 1, False, 101, False),
    "anc_langevin_snr016_n2": ("ancestral_sampling", "langevin", 0.16, 2, False, 102, False),
    "rd_langevin": ("reverse_diffusion", "langevin", 0.075, 1, False, 103, False),
    "rd_pflow": ("reverse_diffusion", "none", 0.075, 1, True, 104, False),
    "em": ("euler_maruyama", "none", 0.075, 1, False, 105, False),
    "ald": ("none", "ald", 0.075, 1, False, 106, False),
    "cond_anc_langevin": ("ancestral_sampling", "langevin", 0.075, 1, False, 107, True),
}
COND_DATA_SEED, FREEZE_ITERS = 5, 4


def set_sampling(cfg, pred, corr, snr, n, pf):
    cfg.sampling.predictor, cfg.sampling.corrector = pred, corr
    cfg.sampling.snr, cfg.sampling.n_steps_each, cfg.sampling.probability_flow = snr, n, pf


def restated_pc_sampler(sd, ocfg, shape, mask, K, seed, pred, corr, snr, n_steps, pf, N=1000, cond=None):
    """The reference PC loop (sampling.py:397-481, predictors :185-237, correctors :259-321, sde_lib.py:93-111,
    :198-232) written out in float32 torch on the oracle U-Net: first K iterations, returns x_mean."""
    B = shape[0]
    betas = torch.linspace(0.1 / N, 20.0 / N, N)
    alphas = 1.0 - betas
    sq1m = torch.sqrt(1.0 - torch.cumprod(alphas, dim=0))
    gm = mask.reshape(1, 1, *shape[2:])
    timesteps = torch.linspace(1.0, 1e-3, N)
    b5 = (slice(None),) + (None,) * 4

    def score(x, t):
        labels = t * (N - 1)
        return -unet_oracle.unet_res64_forward(sd, ocfg, x, labels) / sq1m[labels.long()][b5]

    def std_of(t):
        lmc = -0.25 * t ** 2 * (20.0 - 0.1) - 0.5 * t * 0.1
        return lmc, torch.sqrt(1.0 - torch.exp(2.0 * lmc))

    torch.manual_seed(seed)
    x = torch.randn(*shape) * gm
    if cond is not None:
        partial, pmask, freeze = cond
        vec_t = torch.ones(B) * timesteps[0]
        x[:, 0] = partial[:, 0] * gm[:, 0]
        lmc, std = std_of(vec_t)
        mean = torch.exp(lmc)[b5] * x
        upd = mean[:, 0] + std[b5] * torch.randn_like(mean[:, 0])          # [B,B,R,R,R]: the reference's broadcast
        x[:, 0] = (x[:, 0] * (1 - pmask[:, 0]) + upd[:, 0] * pmask[:, 0]) * gm[:, 0]
    x_mean = x
    for i in range(K):
        t = torch.ones(B) * timesteps[i]
        k = (t * (N - 1)).long()
        for _ in range(n_steps if corr != "none" else 0):
            g = score(x, t)
            z = torch.randn_like(x)
            if corr == "langevin":
                gn = torch.norm(g.reshape(B, -1), dim=-1).mean()
                nn_ = torch.norm(z.reshape(B, -1), dim=-1).mean()
                step = (snr * nn_ / gn) ** 2 * 2 * alphas[k]
            else:
                step = (snr * std_of(t)[1]) ** 2 * 2 * alphas[k]
            x_mean = x + step[b5] * g
            x = x_mean + torch.sqrt(step * 2)[b5] * z
        x, x_mean = x * gm, x_mean * gm
        if pred == "ancestral_sampling":
            g = score(x, t)
            x_mean = (x + betas[k][b5] * g) / torch.sqrt(1.0 - betas[k])[b5]
            x = x_mean + torch.sqrt(betas[k])[b5] * torch.randn_like(x)
        elif pred == "reverse_diffusion":
            G = torch.sqrt(betas[k])
            f = torch.sqrt(alphas[k])[b5] * x - x
            rev_f = f - G[b5] ** 2 * score(x, t) * (0.5 if pf else 1.0)
            z = torch.randn_like(x)
            x_mean = x - rev_f
            x = x_mean + (torch.zeros_like(G) if pf else G)[b5] * z
        elif pred == "euler_maruyama":
            dt = -1.0 / N
            z = torch.randn_like(x)
            beta_t = 0.1 + t * (20.0 - 0.1)
            diffusion = torch.sqrt(beta_t)
            drift = -0.5 * beta_t[b5] * x - diffusion[b5] ** 2 * score(x, t)
            x_mean = x + drift * dt
            x = x_mean + diffusion[b5] * np.sqrt(-dt) * z
        else:
            x_mean = x
        x, x_mean = x * gm, x_mean * gm
        if cond is not None and i != N - 1 and i < freeze:
            x[:, 0] = (x[:, 0] * (1 - pmask[:, 0]) + partial[:, 0] * pmask[:, 0]) * gm[:, 0]
            x_mean[:, 0] = (x_mean[:, 0] * (1 - pmask[:, 0]) + partial[:, 0] * pmask[:, 0]) * gm[:, 0]
            lmc, std = std_of(torch.ones(B) * timesteps[i])
            upd = torch.exp(lmc)[:, None, None, None] * x[:, 0] + std[:, None, None, None] * torch.randn_like(x[:, 0])
            x[:, 0] = (x[:, 0] * (1 - pmask[:, 0]) + upd * pmask[:, 0]) * gm[:, 0]
            x_mean[:, 0] = x[:, 0]
    return x_mean


def cond_data(R, mask):
    """The partial grid / partial mask of sampler_small.npz's inpainting case (oracle/gen_golden.py)."""
    g = torch.Generator().manual_seed(COND_DATA_SEED)
    partial = torch.sign(torch.randn((1, 1, R, R, R), generator=g))
    pmask = (torch.rand((1, 1, R, R, R), generator=g) < 0.5).float() * mask.view(1, 1, R, R, R)
    return partial, pmask


def gen_small(rsampling, rsde, rmutils):
    cfg = synth.small_config(); cfg.device = torch.device("cpu")
    R, B, K = cfg.data.image_size, 2, 6
    sd = make_sd(cfg, R)
    model = ref_model(rmutils, cfg, sd)
    mask = synth.synthetic_grid_mask(R)
    li = live_cells(mask, 1)
    out = dict(K=np.int64(K), B=np.int64(B), sd_seed=np.int64(1234), cond_data_seed=np.int64(COND_DATA_SEED),
               freeze_iters=np.int64(FREEZE_ITERS), cases=np.array(list(CASES)))
    for name, (pred, corr, snr, n, pf, seed, is_cond) in CASES.items():
        set_sampling(cfg, pred, corr, snr, n, pf)
        shape = (B, 4, R, R, R)
        cond = None
        if is_cond:
            partial, pmask = cond_data(R, mask)
            cond = (partial, pmask, FREEZE_ITERS)
            xr = run_ref_sampler(rsampling, rsde, cfg, model, shape, mask.view(1, 1, R, R, R), K, seed, cond=cond)
        else:
            xr = run_ref_sampler(rsampling, rsde, cfg, model, shape, mask.view(1, R, R, R), K, seed)
        xo = restated_pc_sampler(sd, synth.oracle_cfg(cfg), shape, mask, K, seed, pred, corr, snr, n, pf, cond=cond)
        e = rel_l2(xo, xr)
        print(f"[small {name}] restatement vs reference {K} iterations rel-L2 = {e:.3e}", flush=True)
        assert e < 1e-5, name
        assert float((xr * (1 - mask)).abs().max()) == 0.0
        out[f"{name}/live"] = xr.reshape(B, 4, -1)[:, :, li].numpy().copy()
        out[f"{name}/seed"] = np.int64(seed)
        out[f"{name}/snr"], out[f"{name}/n_steps_each"] = np.float64(snr), np.int64(n)
        out[f"{name}/predictor"], out[f"{name}/corrector"] = np.array(pred), np.array(corr)
        out[f"{name}/probability_flow"], out[f"{name}/conditional"] = np.bool_(pf), np.bool_(is_cond)
    np.savez_compressed(os.path.join(GOLD, "sampler_pc_small.npz"), **out)


def gen_res64(rsampling, rsde, rmutils):
    from meshdiffusion_amd.config import get_config_res64
    cfg = get_config_res64(); cfg.device = torch.device("cpu")
    R, B, K, seed, stride = 64, 2, 3, 43, 8
    set_sampling(cfg, "ancestral_sampling", "langevin", 0.075, 1, False)
    sd = make_sd(cfg, R)
    model = ref_model(rmutils, cfg, sd)
    mask = synth.synthetic_grid_mask(R)
    t0 = time.time()
    xr = run_ref_sampler(rsampling, rsde, cfg, model, (B, 4, R, R, R), mask.view(1, R, R, R), K, seed)
    print(f"[res64] reference {K} PC iterations {time.time() - t0:.1f}s", flush=True)
    xo = restated_pc_sampler(sd, synth.oracle_cfg(cfg), (B, 4, R, R, R), mask, K, seed, "ancestral_sampling",
                             "langevin", 0.075, 1, False)
    e = rel_l2(xo, xr)
    print(f"[res64] restatement vs reference rel-L2 = {e:.3e}", flush=True)
    assert e < 1e-5
    np.savez_compressed(os.path.join(GOLD, "sampler_pc_res64.npz"), xm_norm=float(xr.double().norm()),
                        xm_row=xr[1, :, 33, 17, :].numpy(), K=K, B=B, seed=seed, snr=0.075, n_steps_each=1,
                        predictor=np.array("ancestral_sampling"), corrector=np.array("langevin"),
                        **sample_stats(xr, mask, stride))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-res64", action="store_true")
    ap.add_argument("--only", choices=["small", "res64"], default=None)
    a = ap.parse_args()
    torch.set_num_threads(os.cpu_count())
    rs = import_reference()
    with torch.no_grad():
        if a.only in (None, "small"):
            gen_small(*rs)
        if a.only == "res64" or (a.only is None and not a.skip_res64):
            gen_res64(*rs)
    print("predictor-corrector fixtures written to", GOLD)
