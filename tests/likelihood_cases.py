"""Shared cases of the likelihood tests (no GPU needed to import): the float64 host restatement of md_pf_ode_rhs, the analytic
Gaussian score model, the right-hand sides the integrator is compared with scipy on, and the inputs of tests/golden/likelihood.npz
(tools/gen_golden_likelihood.py builds the same ones)."""
import math

import numpy as np
import torch

N_SCALES, BETA0, BETA1 = 1000, 0.1, 20.0


def vp_coefficients_f64(t):
    """(c_x, c_e, alpha, sigma) of the VP SDE at time t in float64, from the closed forms (sde_lib.py:198-214)."""
    beta = BETA0 + t * (BETA1 - BETA0)
    lmc = -0.25 * t * t * (BETA1 - BETA0) - 0.5 * t * BETA0
    sigma = math.sqrt(1.0 - math.exp(2.0 * lmc))
    return -0.5 * beta, 0.5 * beta / sigma, math.exp(lmc), sigma


def pf_ode_rhs_f64(x, eps_hat, mask, coef, g=None, probe=None):
    """md_pf_ode_rhs restated in float64 numpy.  x, eps_hat, g, probe: [B, C, P] float32; mask [P] or None; coef [B, 2] float64.
    Returns (drift float32 -- the float64 value rounded once, div [B] float64 or None, sum of |terms| [B] or None)."""
    x, e = np.asarray(x, np.float64), np.asarray(eps_hat, np.float64)
    m = np.ones(x.shape[-1]) if mask is None else np.asarray(mask, np.float64)
    cx, ce = coef[:, 0][:, None, None], coef[:, 1][:, None, None]
    drift = ((cx * x + ce * e) * m).astype(np.float32)
    if g is None:
        return drift, None, None
    p, gg = np.asarray(probe, np.float64), np.asarray(g, np.float64)
    terms = (p * (cx * p + ce * gg)) * m
    B = x.shape[0]
    div = np.array([math.fsum(terms[b].ravel()) for b in range(B)])
    return drift, div, np.abs(terms).reshape(B, -1).sum(1)


def gaussian_eps_model(s, dtype=torch.float64):
    """eps_hat(x, labels) of data ~ N(0, s^2 I) under the VP SDE, exactly: the marginal at t is N(0, (alpha_t^2 s^2 + sigma_t^2) I),
    its score -x / (alpha_t^2 s^2 + sigma_t^2), and eps_hat = -sigma_t * score.  Its Jacobian is a multiple of the identity."""
    def model(x, labels):
        t = labels.to(dtype) / (N_SCALES - 1)
        lmc = -0.25 * t ** 2 * (BETA1 - BETA0) - 0.5 * t * BETA0
        a2, s2 = torch.exp(2.0 * lmc), 1.0 - torch.exp(2.0 * lmc)
        k = torch.sqrt(s2) / (a2 * s * s + s2)
        return k.view(-1, *([1] * (x.dim() - 1))) * x
    return model


def gaussian_logp(x, var, n_dim):
    """log N(x; 0, var I) per sample over n_dim dimensions (x zero outside them), float64."""
    x = x.double().reshape(x.shape[0], -1)
    return -0.5 * n_dim * math.log(2 * math.pi * var) - 0.5 * (x * x).sum(1) / var


# ---- right-hand sides for the integrator-vs-scipy test: fun(t: float, y: float64 torch vector) --------------------------------
def rhs_linear(t, y):
    """A small time-dependent linear system: a rotation whose rate grows with t, with unequal damping and a forcing term."""
    a = torch.tensor([[-0.5, 1.0 + 3.0 * t, 0.0], [-(1.0 + 3.0 * t), -0.1, 0.2 * t], [0.0, -0.2 * t, -1.5]], dtype=torch.float64)
    return a @ y + torch.tensor([math.sin(5.0 * t), 0.0, 1.0], dtype=torch.float64)


def rhs_nonlinear(t, y):
    """Van der Pol (mu = 2) coupled to a logistic variable."""
    return torch.stack([y[1], 2.0 * (1.0 - y[0] ** 2) * y[1] - y[0] + 0.3 * y[2], y[2] * (1.0 - y[2]) * math.cos(t)])


ODE_CASES = {
    "linear": (rhs_linear, (0.0, 3.0), [1.0, 0.0, -0.5]),
    "nonlinear": (rhs_nonlinear, (0.0, 6.0), [2.0, 0.0, 0.25]),
    "nonlinear_backwards": (rhs_nonlinear, (2.0, 0.0), [0.5, -1.0, 0.6]),       # the ODE sampler integrates from T down to eps
}


# ---- the golden's inputs ---------------------------------------------------------------------------------------------------
def golden_setup(device="cpu"):
    """(cfg, grid mask [R,R,R], x0 [2,4,R,R,R] float32) of tests/golden/likelihood.npz; golden_state_dict has the weights."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    cfg = synth.small_config()
    cfg.device = torch.device(device)
    R = cfg.data.image_size
    gm = synth.synthetic_grid_mask(R)
    x0 = synth.synthetic_inputs(2, 4, R, seed=8) * gm.view(1, 1, R, R, R) * 0.5
    return cfg, gm, x0


def golden_state_dict(cfg, template, gm):
    from meshdiffusion_amd import synth
    return synth.sensitised_state_dict(template, seed=1234, grid_mask=gm)
