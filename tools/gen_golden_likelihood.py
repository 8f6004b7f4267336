"""Writes tests/golden/likelihood.npz: the probability-flow ODE likelihood of the small synthetic U-Net, on the CPU, from the
oracle (oracle/unet_oracle.py under torch autograd, float32 as the reference evaluates its model; the ODE state is float64) and scipy.integrate.solve_ivp(method='RK45') -- nothing of the
package's own likelihood code, integrator or kernels is used.

    python tools/gen_golden_likelihood.py            (about two minutes; needs scipy)

Setup (tests/test_gpu_likelihood.py rebuilds the same inputs): synth.small_config(), sensitised_state_dict(seed=1234) on the
synthetic grid mask; B = 2, x0 = synthetic_inputs(seed=8) * mask * 0.5; one masked Rademacher probe (stored as int8); ODE span
t in [1e-3, 1]; VP SDE beta in [0.1, 20], N = 1000, labels t * (N - 1).
Stored: delta_logp / z / nfev / accepted steps at rtol = atol = 1e-3 and 1e-5; u = |delta_logp(1e-3) - delta_logp(1e-5)| per
sample (the solver's own uncertainty at 1e-3) and the matching distance of z; the round trip decode(encode(x0)) at 1e-3 (the
ODE back from T to 1e-3 starting at z(1e-3), no divergence) with its distance to x0; the figures of the same decode at 1e-5
(roundtrip_u: its distance from the 1e-3 decode; roundtrip_dist_5: its distance from x0 -- the backward ODE of this synthetic
network expands so strongly that neither decode returns x0); roundtrip_sens: how far the 1e-3 decode moves when every eps_hat
is off by 1e-4 relative (the forward bar), the yardstick for a decode on another machine; the oracle's input gradient J^T c of
eps_hat at t = 0.5 for a fixed cotangent c = synthetic_inputs(seed=9).
"""
import os
import sys
import time

import numpy as np
import torch
from scipy import integrate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from meshdiffusion_amd import synth                                    # noqa: E402
from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: E402,F401
from oracle import unet_oracle as uo                                   # noqa: E402

N, BETA0, BETA1, T0, T1 = 1000, 0.1, 20.0, 1e-3, 1.0


def coefficients(t):
    """(c_x, c_e) = (-0.5 beta(t), 0.5 beta(t) / sigma(t)) of the VP SDE in float64."""
    beta = BETA0 + t * (BETA1 - BETA0)
    lmc = -0.25 * t * t * (BETA1 - BETA0) - 0.5 * t * BETA0
    return -0.5 * beta, 0.5 * beta / np.sqrt(1.0 - np.exp(2.0 * lmc))


def setup():
    cfg = synth.small_config()
    cfg.device = torch.device("cpu")
    R = cfg.data.image_size
    gm = synth.synthetic_grid_mask(R)
    template = mutils.create_model(cfg).module.state_dict()
    sd = synth.sensitised_state_dict(template, seed=1234, grid_mask=gm)
    mask = gm.view(1, 1, R, R, R).float()
    x0 = synth.synthetic_inputs(2, 4, R, seed=8) * mask * 0.5
    g = torch.Generator().manual_seed(20261019)
    probe = (torch.randint(0, 2, x0.shape, generator=g).float() * 2 - 1) * mask
    return cfg, sd, mask, x0, probe


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    cfg, sd, mask, x0, probe = setup()
    ocfg = synth.oracle_cfg(cfg)
    shape, B, n = tuple(x0.shape), x0.shape[0], x0.numel()

    # a fixed sign pattern: eps_hat * (1 + 1e-4 * signs) is eps_hat with a relative L2 error of exactly 1e-4, the project's bar for
    # a forward evaluation (tests/test_gpu_unet.py) -- what another machine's arithmetic may do to every evaluation
    signs = torch.randint(0, 2, x0.shape, generator=torch.Generator().manual_seed(77)).float() * 2 - 1

    def drift_of(x, t, rel_err=0.0):
        cx, ce = coefficients(t)
        e = uo.unet_res64_forward(sd, ocfg, x, torch.full((B,), t * (N - 1)))
        if rel_err:
            e = e * (1.0 + rel_err * signs)
        return (cx * x + ce * e) * mask

    def rhs_logp(t, y):
        x = torch.from_numpy(y[:n].reshape(shape)).float().requires_grad_(True)
        drift = drift_of(x, t)
        g, = torch.autograd.grad(torch.sum(drift * probe), x)
        div = torch.sum(g * probe, dim=(1, 2, 3, 4))
        return np.concatenate([drift.detach().numpy().reshape(-1), div.numpy()])

    def rhs_x(t, y, rel_err=0.0):
        with torch.no_grad():
            return drift_of(torch.from_numpy(y.reshape(shape)).float(), t, rel_err).numpy().reshape(-1)

    out = dict(probe=probe.numpy().astype(np.int8), t_span=np.array([T0, T1]))
    y0 = np.concatenate([x0.numpy().reshape(-1), np.zeros(B)])
    for tag, tol in (("3", 1e-3), ("5", 1e-5)):
        t = time.time()
        sol = integrate.solve_ivp(rhs_logp, (T0, T1), y0, rtol=tol, atol=tol, method="RK45")
        assert sol.status == 0
        out[f"z_{tag}"] = sol.y[:n, -1].reshape(shape).astype(np.float32)
        out[f"delta_logp_{tag}"] = sol.y[n:, -1].copy()
        out[f"nfev_{tag}"] = np.int64(sol.nfev)
        out[f"steps_{tag}"] = np.int64(len(sol.t) - 1)
        print(f"rtol = atol = {tol:g}: nfev {sol.nfev}, {len(sol.t) - 1} steps, delta_logp {sol.y[n:, -1]}, {time.time() - t:.1f} s", flush=True)
        if tag == "3":
            z3 = sol.y[:n, -1].copy()
    out["u"] = np.abs(out["delta_logp_3"] - out["delta_logp_5"])
    dz = (out["z_3"].astype(np.float64) - out["z_5"]).reshape(B, -1)
    out["z_dist"] = np.linalg.norm(dz, axis=1) / np.linalg.norm(out["z_5"].astype(np.float64).reshape(B, -1), axis=1)
    back = integrate.solve_ivp(rhs_x, (T1, T0), z3, rtol=1e-3, atol=1e-3, method="RK45")
    assert back.status == 0
    rt = back.y[:, -1].reshape(shape)
    x0 = x0.double()
    out["roundtrip"] = rt.astype(np.float32)
    out["roundtrip_nfev"] = np.int64(back.nfev)
    out["roundtrip_dist"] = np.linalg.norm((rt - x0.numpy()).reshape(B, -1), axis=1) / np.linalg.norm(x0.numpy().reshape(B, -1), axis=1)
    # the same decode from the same z(1e-3) at 1e-5: its distance from the 1e-3 decode is the solver's own uncertainty at 1e-3
    t = time.time()
    back5 = integrate.solve_ivp(rhs_x, (T1, T0), z3, rtol=1e-5, atol=1e-5, method="RK45")
    assert back5.status == 0
    rt5 = back5.y[:, -1].reshape(shape)
    out["roundtrip_nfev_5"] = np.int64(back5.nfev)
    out["roundtrip_u"] = np.linalg.norm((rt - rt5).reshape(B, -1), axis=1) / np.linalg.norm(rt5.reshape(B, -1), axis=1)
    out["roundtrip_dist_5"] = np.linalg.norm((rt5 - x0.numpy()).reshape(B, -1), axis=1) / np.linalg.norm(x0.numpy().reshape(B, -1), axis=1)
    # the 1e-3 decode once more with every eps_hat off by 1e-4 relative: how far a decode moves under arithmetic at the forward bar
    backp = integrate.solve_ivp(lambda t, y: rhs_x(t, y, 1e-4), (T1, T0), z3, rtol=1e-3, atol=1e-3, method="RK45")
    assert backp.status == 0
    rtp = backp.y[:, -1].reshape(shape)
    out["roundtrip_sens"] = np.linalg.norm((rtp - rt).reshape(B, -1), axis=1) / np.linalg.norm(rt.reshape(B, -1), axis=1)
    out["roundtrip_sens_nfev"] = np.int64(backp.nfev)
    print(f"decode at 1e-3 with eps_hat off by 1e-4: nfev {backp.nfev}, distance from the decode {out['roundtrip_sens']}", flush=True)
    print(f"decode at 1e-5: nfev {back5.nfev}, {time.time() - t:.1f} s; |decode(1e-3) - decode(1e-5)| / |decode(1e-5)| {out['roundtrip_u']}; "
          f"|decode(1e-5) - x0| / |x0| {np.linalg.norm((rt5 - x0.numpy()).reshape(B, -1), axis=1) / np.linalg.norm(x0.numpy().reshape(B, -1), axis=1)}", flush=True)
    # the oracle's input gradient for a fixed cotangent
    cot = synth.synthetic_inputs(2, 4, shape[-1], seed=9)
    xr = x0.float().requires_grad_(True)
    e = uo.unet_res64_forward(sd, ocfg, xr, torch.full((B,), 0.5 * (N - 1)))
    out["input_grad"] = torch.autograd.grad(e, xr, cot)[0].numpy().astype(np.float32)
    print("u", out["u"], "z_dist", out["z_dist"], "roundtrip_dist", out["roundtrip_dist"], "nfev back", back.nfev)
    path = os.path.join(ROOT, "tests", "golden", "likelihood.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
