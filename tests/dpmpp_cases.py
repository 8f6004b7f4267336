"""Shared cases of the DPM-Solver++ tests (no GPU needed to import): the VP schedule and the defining integrals of the update's
weights restated in float64 without the package's host code, md_multistep_step restated in extended precision with the sums its
error bars are written in, and the float64 recursion of sampling.dpmpp_sampler's loop for any eps function (the closed-form model
of guidance_cases, or the oracle U-Net), with the loop's two float32 roundings, replacement, guidance and noise as options."""
import math

import numpy as np
import torch

import guidance_cases as gc

BETA0, BETA1 = gc.BETA0, gc.BETA1
U = 2.0 ** -53


# ---- the schedule and the weights, from their definitions ------------------------------------------------------------------------
def alpha_sigma_lambda(t):
    """(alpha, sigma, lambda) of the continuous VP schedule at t, float64, written out once more."""
    lmc = -0.25 * t * t * (BETA1 - BETA0) - 0.5 * t * BETA0
    sigma = math.sqrt(-math.expm1(2.0 * lmc))
    return math.exp(lmc), sigma, lmc - math.log(sigma)


def lagrange(nodes, j, u):
    """l_j(u) on `nodes`."""
    v = 1.0
    for i, n in enumerate(nodes):
        if i != j:
            v *= (u - n) / (nodes[j] - n)
    return v


def nodes_for(order, rs):
    """Nodes of the last `order` predictions in u = (lambda - lambda_s)/h: 0, -r_1, -r_1-r_2."""
    return [0.0, -rs[0] if order > 1 else None, -(rs[0] + rs[1]) if order > 2 else None][:order]


def weights_by_quadrature(h, rs, order, tau):
    """[(w_j, quad's own error estimate)]: w_j = g int_0^1 exp(-g (1-u)) l_j(u) du, g = h (tau 0) or 2h (tau 1), by scipy."""
    from scipy import integrate
    g = h * (2.0 if tau else 1.0)
    nodes = nodes_for(order, rs)
    out = []
    for j in range(order):
        v, err = integrate.quad(lambda u: g * math.exp(-g * (1.0 - u)) * lagrange(nodes, j, u), 0.0, 1.0, epsabs=0.0, epsrel=2e-14,
                                limit=200)
        out.append((v, err))
    return out


def exact_step(ts, tt, x_s, x0_of_lambda, tau):
    """The variation-of-constants solution from t_s to t_t for a given x0(lambda), without noise, by quadrature:
    tau 0: x_t = sigma_t/sigma_s x_s + sigma_t int e^lambda x0 dlambda ; tau 1: the mean sigma_t/sigma_s e^-h x_s + 2 alpha_t int
    e^(-2 (lambda_t - lambda)) x0 dlambda."""
    from scipy import integrate
    a_s, s_s, l_s = alpha_sigma_lambda(ts)
    a_t, s_t, l_t = alpha_sigma_lambda(tt)
    h = l_t - l_s
    if tau:
        v, _ = integrate.quad(lambda lam: 2.0 * math.exp(-2.0 * (l_t - lam)) * x0_of_lambda(lam), l_s, l_t, epsabs=0.0, epsrel=2e-14)
        return s_t / s_s * math.exp(-h) * x_s + a_t * v
    v, _ = integrate.quad(lambda lam: math.exp(-(l_t - lam)) * x0_of_lambda(lam), l_s, l_t, epsabs=0.0, epsrel=2e-14)
    return s_t / s_s * x_s + a_t * v


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
def multistep_ref(x, eps, h1, h2, z, mask, coef, partial, pmask, ch):
    """md_multistep_step in np.longdouble.  x, h1, h2: [B, C, P] float64 (h1 / h2 / z / mask / partial may be None); eps, z float32;
    coef [B, 8] float64.  Returns a dict: x0 / x_new (exact, before mask and replacement, longdouble), x0_bar = (|x| + |sigma eps|) /
    alpha, terms = sum of |term| of x_new, and keep [B, C, P] bool: the voxels that are neither masked out nor replaced."""
    L = np.longdouble
    B, C, P = x.shape
    r = lambda j: coef[:, j].astype(L)[:, None, None]                                       # noqa: E731
    xl, el = x.astype(L), eps.astype(L)
    x0 = (xl - r(1) * el) / r(0)
    terms = [r(2) * xl, r(3) * x0]
    for c, t in ((r(4), h1), (r(5), h2), (r(6), z)):
        if t is not None:
            terms.append(c * t.astype(L))
    keep = np.ones((B, C, P), bool)
    if mask is not None:
        keep &= (mask != 0)[None, None]
    if partial is not None:
        keep[:, ch] &= (pmask == 0)[None]
    return dict(x0=x0, x_new=sum(terms), x0_bar=(np.abs(xl) + np.abs(r(1) * el)) / r(0), terms=sum(np.abs(t) for t in terms), keep=keep)


def multistep_chain_f64(x, eps, h1, h2, z, mask, coef, partial, pmask, ch):
    """The same update as a plain float64 numpy chain in the kernel's order (no contraction): what the kernel should return bit for
    bit if the compiler keeps the order; used on the CPU to see that the bars of the GPU test leave room for such a chain."""
    r = lambda j: coef[:, j][:, None, None]                                                 # noqa: E731
    x0 = (x - r(1) * eps.astype(np.float64)) / r(0)
    xn = r(2) * x + r(3) * x0
    for c, t in ((r(4), h1), (r(5), h2), (r(6), z)):
        if t is not None:
            xn = xn + c * t.astype(np.float64)
    if mask is not None:
        m = mask.astype(np.float64)[None, None]
        xn, x0 = xn * m, x0 * m
    if partial is not None:
        pm, pv = pmask.astype(np.float64)[None], partial.astype(np.float64)[None]
        xn[:, ch] = xn[:, ch] * (1.0 - pm) + pv * pm
        x0[:, ch] = x0[:, ch] * (1.0 - pm) + pv * pm
    return xn, x0, xn.astype(np.float32)


def kernel_inputs(B, C, P, seed):
    """Operands of one kernel case: state, eps, two histories, noise, a grid mask, a partial grid with its mask."""
    g = torch.Generator().manual_seed(seed)
    x, h1, h2 = (torch.randn((B, C, P), generator=g, dtype=torch.float64) for _ in range(3))
    eps, z = (torch.randn((B, C, P), generator=g) for _ in range(2))
    mask = (torch.rand(P, generator=g) < 0.6).float()
    pm = (torch.rand(P, generator=g) < 0.4).float()
    mask[0], pm[0] = 1.0, 1.0
    part = torch.sign(torch.randn(P, generator=g))
    return dict(x=x, eps=eps, h1=h1, h2=h2, z=z, mask=mask, partial=part, pmask=pm)


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def recursion(eps_fn, x_init, rows, labels, orders, gm=None, partial=None, pm=None, ch=0, noise=None, guide=None, denoise=False,
              round_state=True):
    """sampling.dpmpp_sampler's loop in float64.  eps_fn(x, labels [B]) -> eps_hat; round_state: the model sees float(x) and its
    float32 answer is widened (the loop's two float32 roundings), else it sees the float64 state.  rows [steps, 8], labels [steps]
    as dpmpp_tables returns them, orders as dpmpp_orders does; gm / partial / pm: [R, R, R] float64 or None (partial: replacement at
    the start and in every step); noise: per-step tensors for c_z; guide(x_before_the_step, i) -> d, subtracted after the step.
    Returns the last state, or the last clean-grid prediction with `denoise`."""
    B = x_init.shape[0]
    x = x_init.double()
    if gm is not None:
        x = x * gm
    if partial is not None:
        x = x.clone()
        x[:, ch] = x[:, ch] * (1 - pm) + partial * pm
    rows = torch.as_tensor(rows, dtype=torch.float64)
    lab32 = torch.as_tensor(labels, dtype=torch.float64).float()
    hist, x0 = [], x
    for i in range(rows.shape[0]):
        a_s, s_s, cx, c0, c1, c2, cz = (float(v) for v in rows[i, :7])
        lab = lab32[i].expand(B)
        e = eps_fn(x.float(), lab).double() if round_state else eps_fn(x, lab.double())
        d = guide(x, i) if guide is not None else 0.0
        x0 = (x - s_s * e) / a_s
        xn = cx * x + c0 * x0
        for c, hprev in zip((c1, c2), hist[:orders[i] - 1]):
            xn = xn + c * hprev
        if cz != 0.0:
            xn = xn + cz * noise[i].double()
        if gm is not None:
            xn, x0 = xn * gm, x0 * gm
        if partial is not None:
            xn[:, ch] = xn[:, ch] * (1 - pm) + partial * pm
            x0[:, ch] = x0[:, ch] * (1 - pm) + partial * pm
        hist = [x0] + hist[:1]
        x = xn - d
    return x0 if denoise else x


def gaussian_guide(s, N, rows, labels, y, pm, gm, zeta, ch, round_input=False):
    """guide(x, i) of the closed-form model eps_hat = k_t x: guidance_cases' d at the level (alpha_s, sigma_s) of step i.
    round_input: evaluated at float(x), the state the sampler's network sees -- a probe, never the reference."""
    lab32 = torch.as_tensor(labels, dtype=torch.float64).float()

    def guide(x, i):
        k = gc.gaussian_k(lab32[i].expand(x.shape[0]), s, N)
        xg = x.float().double() if round_input else x
        return gc._guided_d(xg, k, y, pm, gm, float(rows[i, 0]), float(rows[i, 1]), zeta, ch)
    return guide


def gaussian_exact(x_T, s, t0, t1):
    """The probability-flow ODE's exact solution for data ~ N(0, s^2 I) from t0 down to t1."""
    a0, s0, _ = alpha_sigma_lambda(t0)
    a1, s1, _ = alpha_sigma_lambda(t1)
    return x_T * math.sqrt((a1 * a1 * s * s + s1 * s1) / (a0 * a0 * s * s + s0 * s0))
