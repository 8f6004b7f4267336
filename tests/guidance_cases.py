"""Shared cases of the reconstruction-guidance tests (no GPU needed to import): numpy restatements of md_guide_residual,
md_guide_apply_f32 and md_guide_apply_f64 (double where the contract says double, np.float32 operations where it says fl), the
closed-form score model of data ~ N(0, s^2 I) with its vector-Jacobian product, and float64 recursions of the guided ancestral
and DDIM loops for that model, which take the noise as input."""
import math

import numpy as np
import torch

BETA0, BETA1 = 0.1, 20.0
SLABS = 64


# ---- the three kernels -------------------------------------------------------------------------------------------------------
def guide_residual_ref(x, eps_hat, src, pm, gm, coef, ch):
    """md_guide_residual.  x, eps_hat: [B, C, P] float32; src [P] or [B, P]; pm [P]; gm [P] or None; coef [B, 2] float64.
    Returns (cot float32 [B, C, P]: the float64 r rounded once in channel ch, +0 elsewhere; r in float64 [B, P];
    sum of the squares of the rounded r [B] float64, added exactly)."""
    x, e = np.asarray(x, np.float64), np.asarray(eps_hat, np.float64)
    B, C, P = x.shape
    y = np.broadcast_to(np.asarray(src, np.float64).reshape(-1, P), (B, P))
    m = np.asarray(pm, np.float64) * (1.0 if gm is None else np.asarray(gm, np.float64))
    alpha, sigma = coef[:, 0][:, None], coef[:, 1][:, None]
    x0 = (x[:, ch] - sigma * e[:, ch]) / alpha
    r = m[None] * (x0 - y)
    cot = np.zeros((B, C, P), np.float32)
    cot[:, ch] = r.astype(np.float32)
    sq = cot[:, ch].astype(np.float64) ** 2
    return cot, r, np.array([math.fsum(sq[b]) for b in range(B)])


def _guide_d(cot, g, gm, coef, slabs):
    """d of md_guide_apply in float64 [B, C, P]: the slabs are added in ascending order, k = zeta/(alpha*n), 0 where n == 0."""
    B = cot.shape[0]
    k = np.zeros(B)
    for b in range(B):
        s = np.float64(0.0)
        for v in np.asarray(slabs[b], np.float64):
            s = s + v
        n = np.sqrt(s)
        k[b] = 0.0 if n == 0.0 else coef[b, 2] / (coef[b, 0] * n)
    m = 1.0 if gm is None else np.asarray(gm, np.float64)[None, None]
    with np.errstate(invalid="ignore"):
        return (k[:, None, None] * (np.asarray(cot, np.float64) - coef[:, 1][:, None, None] * np.asarray(g, np.float64))) * m


def guide_apply_f32_ref(x, x_mean, cot, g, gm, coef, slabs):
    """md_guide_apply_f32: d rounded to float once, x = fl(x - d), x_mean (or None) likewise.  coef [B, 3] float64."""
    d = _guide_d(cot, g, gm, coef, slabs).astype(np.float32)
    x = np.asarray(x, np.float32) - d
    return x, (None if x_mean is None else np.asarray(x_mean, np.float32) - d)


def guide_apply_f64_ref(x64, cot, g, gm, coef, slabs):
    """md_guide_apply_f64: x64 -= d with d in double; the float32 copy is float(x64)."""
    x = np.asarray(x64, np.float64) - _guide_d(cot, g, gm, coef, slabs)
    return x, x.astype(np.float32)


def guide_d_f64(x, eps_hat, jt, src, pm, gm, alpha, sigma, zeta, ch):
    """d = zeta/(alpha*||r||) * (r - sigma*J^T r) * gm of the issue in torch float64, for one level (alpha, sigma floats).
    x, eps_hat [B, C, P]; jt: callable r_full [B, C, P] -> J^T r_full.  Returns (d, ||r|| [B])."""
    m = pm if gm is None else pm * gm
    x0 = (x - sigma * eps_hat) / alpha
    r = torch.zeros_like(x)
    r[:, ch] = m * (x0[:, ch] - src)
    n = r.flatten(1).norm(dim=1)
    k = torch.where(n == 0, torch.zeros_like(n), zeta / (alpha * n))
    d = k.view(-1, 1, 1) * (r - sigma * jt(r))
    return (d if gm is None else d * gm), n


# ---- the closed-form model ---------------------------------------------------------------------------------------------------
def gaussian_k(labels, s, N, dtype=torch.float64):
    """k_t of eps_hat = k_t x for data ~ N(0, s^2 I) under the VP SDE with N levels (labels = t (N-1)): the marginal at t is
    N(0, (alpha_t^2 s^2 + sigma_t^2) I), eps_hat = -sigma_t * score, so k_t = sigma_t / (alpha_t^2 s^2 + sigma_t^2)."""
    t = labels.to(dtype) / (N - 1)
    lmc = -0.25 * t ** 2 * (BETA1 - BETA0) - 0.5 * t * BETA0
    a2, s2 = torch.exp(2.0 * lmc), 1.0 - torch.exp(2.0 * lmc)
    return torch.sqrt(s2) / (a2 * s * s + s2)


class GaussianEps(torch.nn.Module):
    """eps_hat(x, labels) = k_t x in x's dtype (k_t formed in float64).  Its Jacobian is k_t I, so J^T r = k_t r; a module, so that
    the samplers can put it in eval mode."""

    def __init__(self, s, N):
        super().__init__()
        self.s, self.N = s, N

    def forward(self, x, labels):
        k = gaussian_k(labels, self.s, self.N)
        return (k.view(-1, *([1] * (x.dim() - 1))) * x.double()).to(x.dtype)


# ---- float64 recursions of the guided loops for that model ---------------------------------------------------------------------
def _guided_d(x, k, y, pm, gm, alpha, sigma, zeta, ch):
    """d for eps_hat = k x (k [B] float64) on [B, C, R, R, R] float64 states; y, pm, gm: [R, R, R]."""
    flat, kk = x.reshape(x.shape[0], x.shape[1], -1), k.view(-1, 1, 1)
    d, _ = guide_d_f64(flat, kk * flat, lambda r: kk * r, y.reshape(-1), pm.reshape(-1), gm.reshape(-1), alpha, sigma, zeta, ch)
    return d.view_as(x)


def ancestral_recursion(sde, s, x_init, y, pm, gm, ch, zeta, replace, noise, eps=1e-3):
    """sampling.pc_sampler's conditional ancestral loop (no corrector) in float64 for the closed-form model, with guidance when
    zeta > 0 and with the replacement / re-noise lines when `replace`.  The coefficient tables are the sampler's own float32 ones,
    widened.  x_init [B, C, R, R, R]: the masked prior draw; y, pm, gm: [R, R, R] float64; noise: iterator over the sampler's
    draws, in its order.  Returns (x, x_mean)."""
    N, B = sde.N, x_init.shape[0]
    x = x_init.double().clone()
    timesteps = torch.linspace(sde.T, eps, N)
    labels = timesteps * (N - 1)
    kidx = (timesteps * (N - 1) / sde.T).long()
    beta, sig, alp = (t[kidx].double() for t in (sde.discrete_betas, sde.sqrt_1m_alphas_cumprod, sde.sqrt_alphas_cumprod))
    draw = lambda: next(noise).double()                                                 # noqa: E731
    if replace:                                        # the initial conditioning, with the reference's broadcasting quirk
        x[:, ch] = y * gm
        lmc0 = -0.25 * timesteps[0] ** 2 * (sde.beta_1 - sde.beta_0) - 0.5 * timesteps[0] * sde.beta_0
        mean, std = torch.exp(lmc0).double() * x, torch.sqrt(1.0 - torch.exp(2.0 * lmc0)).double()
        z0 = draw()
        upd = mean[ch, ch][None] + std * z0[ch][None]
        x[:, ch] = (x[:, ch] * (1 - pm) + upd * pm) * gm
    x_mean = x
    for i in range(N):
        k = gaussian_k(labels[i].expand(B), s, N)
        e = k.view(-1, 1, 1, 1, 1) * x
        d = _guided_d(x, k, y, pm, gm, alp[i], sig[i], zeta, ch) if zeta else 0.0
        z = draw()
        x_mean = (x + beta[i] * (-e / sig[i])) / torch.sqrt(1.0 - beta[i].float()).double()
        x = (x_mean + torch.sqrt(beta[i].float()).double() * z) * gm - d
        x_mean = x_mean * gm - d
        if replace and i != N - 1:
            x[:, ch] = (x[:, ch] * (1 - pm) + y * pm) * gm
            x_mean[:, ch] = (x_mean[:, ch] * (1 - pm) + y * pm) * gm
            t_i = timesteps[i]
            lmc = -0.25 * t_i ** 2 * (sde.beta_1 - sde.beta_0) - 0.5 * t_i * sde.beta_0
            rc0, rc1 = torch.exp(lmc).double(), torch.sqrt(1.0 - torch.exp(2.0 * lmc)).double()
            z2 = draw()
            upd = rc0 * x[:, ch] + rc1 * z2
            x[:, ch] = (x[:, ch] * (1 - pm) + upd * pm) * gm
            x_mean[:, ch] = x[:, ch]
    return x, x_mean


def ddim_recursion(sde, s, x0, y, pm, gm, ch, zeta, replace, timesteps, round_input=False):
    """sampling.ddim_sampler's loop in float64 for the closed-form model on the sub-sequence `timesteps` (ddim_schedule's), with
    guidance when zeta > 0; `replace`: the replacement of the known voxels at the start and in every step (the sampler's unguided
    run with `partial` always replaces).  round_input: the guidance term is evaluated at float(x), the state the sampler's
    network sees -- a probe of how the loop amplifies a float32 rounding, never the reference.  Returns the last state."""
    N, B = sde.N, x0.shape[0]
    x = x0.double() * gm
    if replace:
        x[:, ch] = x[:, ch] * (1 - pm) + y * pm
    sa, s1 = sde.sqrt_alphas_cumprod.double(), sde.sqrt_1m_alphas_cumprod.double()
    for i in reversed(range(1, len(timesteps))):
        t, tp = timesteps[i], timesteps[i - 1]
        k_, kp = int((t * (N - 1) / sde.T).long()), int((tp * (N - 1) / sde.T).long())
        a1, a2 = sa[k_], s1[k_]
        r1, r2 = sa[kp] / a1, s1[kp] / a2
        k = gaussian_k((t.float() * (N - 1)).expand(B), s, N)
        e = k.view(-1, 1, 1, 1, 1) * x
        d = _guided_d(x.float().double() if round_input else x, k, y, pm, gm, a1, a2, zeta, ch) if zeta else 0.0
        x0s = x - a2 * e
        xn = (r1 * x + (r2 - r1) * (x - x0s)) * gm
        if replace:
            xn[:, ch] = xn[:, ch] * (1 - pm) + y * pm
        x = xn - d
    return x


def loop_setup(device="cpu"):
    """The inputs of the loop tests: VPSDE(N = 50) (no beta reaches 1), an 8^3 grid with synth.synthetic_grid_mask(8), pm = a
    half-space of the grid mask, y = +-1, s = 1, zeta = 1, B = 2.  `ddim`: the DDIM loop's schedule, 25 uniform points.  Not the
    default 100-point quadratic one: it ends with a dozen updates on level 0, where ||r|| has fallen below the fixed step length
    zeta alpha^2 and the normalised step overshoots back and forth; the float64 recursion itself then amplifies one float32
    rounding of the guidance input to 5.5e-6 of the final state (test_cpu_guidance measures it), above the GPU test's bar."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import sde_lib
    R, B, C, N = 8, 2, 4, 50
    sde = sde_lib.VPSDE(BETA0, BETA1, N, device=device)
    gm = synth.synthetic_grid_mask(R).reshape(R, R, R).double()
    half = torch.zeros(R, R, R, dtype=torch.float64)
    half[: R // 2] = 1.0
    g = torch.Generator().manual_seed(11)
    y = torch.sign(torch.randn((R, R, R), generator=g, dtype=torch.float64))
    return dict(sde=sde, R=R, B=B, C=C, N=N, gm=gm, pm=half * gm, y=y, s=1.0, zeta=1.0, ch=0, shape=(B, C, R, R, R),
                ddim=("uniform", 25))


def loop_noise(shape, seed, n):
    """`n` rounds of the ancestral sampler's draws, as a list: the initial conditioning's [B, R, R, R], then per iteration the
    step's [B, C, R, R, R] and the re-noise's [B, R, R, R].  A run without replacement reads only the steps' entries."""
    g = torch.Generator().manual_seed(seed)
    B, C, R = shape[0], shape[1], shape[2]
    out = [torch.randn((B, R, R, R), generator=g)]
    for _ in range(n):
        out += [torch.randn(shape, generator=g), torch.randn((B, R, R, R), generator=g)]
    return out


def noise_for(noise, replace, N):
    """The entries of loop_noise's list that a run draws, in its order: with replacement all but the last iteration's re-noise
    (the sampler's last iteration has none); without it the steps' entries only."""
    if replace:
        return noise[:2 * N]
    return noise[1::2][:N]
