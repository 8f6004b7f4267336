"""Shared cases of the latent-interpolation tests (no GPU needed to import): the slerp case list with its seeded inputs, the
np.longdouble restatement of md_slerp_dots + md_slerp_mix, the pairs behind tests/golden/latent.npz, the float64 recursion of the
DDIM encode loop for the closed-form model of guidance_cases, the same loop around the oracle's U-Net forward, and the closed-form
probability flow of that model."""
import numpy as np
import torch

import guidance_cases as gc

LINEAR_BELOW = 2.0 ** -40          # (1-c)(1+c) below this: parallel or antiparallel endpoints, linear interpolation

# (pairs, K, C, P): most slabs empty; CP = 6912, no multiple of 1024; every slab non-empty, two float4s per thread of the dots
# kernel; one float4 in all; K at the cap
SLERP_CASES = [(1, 5, 4, 512), (2, 3, 4, 1728), (1, 2, 4, 32768), (3, 1, 1, 4), (1, 256, 4, 512)]
# cos(theta) of pair p of a case, over the live values
SLERP_RHO = (0.03, 0.60, -0.50, 0.66)

# tests/golden/latent.npz: (seed, C, P, rho) of each pair, and the positions
GOLDEN_PAIRS = [(101, 4, 512, 0.0), (102, 4, 1728, 0.6), (103, 1, 4, 0.3)]
GOLDEN_ALPHAS = (0.0, 0.25, 0.5, 0.8, 1.0)


def golden_pair(seed, C, P, rho):
    """A seeded float32 pair [C, P] with b = rho*a + sqrt(1 - rho^2)*n."""
    g = np.random.default_rng(seed)
    a, n = g.standard_normal((C, P)), g.standard_normal((C, P))
    return a.astype(np.float32), (rho * a + np.sqrt(1.0 - rho * rho) * n).astype(np.float32)


def binary_mask(P, seed):
    """A binary float32 mask [P] in the manner of synth.synthetic_grid_mask for any P: about 60 % live, the first two always."""
    m = (np.random.default_rng(seed).random(P) < 0.6).astype(np.float32)
    m[:2] = 1.0
    return m


def slerp_alphas(K):
    """K positions: both ends and K-2 evenly between them; a single interior one for K = 1, and an interior one beside the far end
    for K = 2 (the near end is covered by every larger K), so that the largest case also forms weights."""
    if K <= 2:
        return np.array([0.3, 1.0][:K])
    return np.arange(K, dtype=np.float64) / float(K - 1)


def slerp_inputs(case, masked):
    """(a, b [pairs, C, P] float32, mask [P] float32 or None, alphas [K] float64) of a case.  Pair p has cos(theta) =
    SLERP_RHO[p] over its live values up to float32 rounding: b = rho*a + sqrt(1 - rho^2)*n with n made orthogonal to a and as long
    as a there, so that the smallest case (four values) is as well conditioned as the largest."""
    pairs, K, C, P = case
    seed = 7 * P + 13 * K + pairs + (1000 if masked else 0)
    mask = binary_mask(P, seed + 1) if masked else None
    m = np.ones(P) if mask is None else mask.astype(np.float64)
    g = np.random.default_rng(seed)
    a = g.standard_normal((pairs, C, P))
    n = g.standard_normal((pairs, C, P))
    b = np.empty_like(a)
    for p in range(pairs):
        am, nm = a[p] * m, n[p] * m
        nm = nm - am * (np.sum(am * nm) / np.sum(am * am))
        nm = nm * np.sqrt(np.sum(am * am) / np.sum(nm * nm))
        rho = SLERP_RHO[p]
        # outside the mask b keeps plain noise: the kernel must not read it into the angle
        b[p] = np.where(m > 0, rho * am + np.sqrt(1.0 - rho * rho) * nm, n[p])
    return a.astype(np.float32), b.astype(np.float32), mask, slerp_alphas(K)


def slerp_ref(a, b, mask, alphas):
    """md_slerp_dots + md_slerp_mix in np.longdouble.  a, b: [pairs, C, P] float32; mask [P] or None; alphas [K].
    Returns (v [pairs, K, C, P]: the exact (w1*a + w2*b)*mask, w1 [pairs, K], w2 [pairs, K], theta [pairs]), all longdouble.
    Same rule as the kernel for parallel pairs: (1-c)(1+c) < 2^-40 gives the weights (1-alpha, alpha)."""
    ld = np.longdouble
    a, b = np.asarray(a, ld), np.asarray(b, ld)
    pairs = a.shape[0]
    m = np.ones(a.shape[-1], ld) if mask is None else np.asarray(mask, ld)
    al = np.asarray(alphas, ld)
    am, bm = a * m, b * m
    v = np.empty((pairs, len(al)) + a.shape[1:], ld)
    w1, w2, theta = np.empty((pairs, len(al)), ld), np.empty((pairs, len(al)), ld), np.empty(pairs, ld)
    with np.errstate(invalid="ignore", divide="ignore"):
        for p in range(pairs):
            c = np.sum(am[p] * bm[p]) / (np.sqrt(np.sum(am[p] * am[p])) * np.sqrt(np.sum(bm[p] * bm[p])))
            c = ld(-1) if c < -1 else (ld(1) if c > 1 else c)
            theta[p] = np.arccos(c)
            if (1 - c) * (1 + c) < LINEAR_BELOW:
                w1[p], w2[p] = 1 - al, al
            else:
                w1[p], w2[p] = np.sin((1 - al) * theta[p]) / np.sin(theta[p]), np.sin(al * theta[p]) / np.sin(theta[p])
            for k in range(len(al)):
                v[p, k] = (w1[p, k] * a[p] + w2[p, k] * b[p]) * m
    return v, w1, w2, theta


def slerp_bound(a, b, mask, v, w1, w2):
    """The per-element bar of the kernel against slerp_ref: half a float32 spacing at v for the single rounding, and
    1e-10*(|w1 a| + |w2 b|) for the weights (slab order, the device's double sin and acos)."""
    m = np.ones(a.shape[-1]) if mask is None else np.asarray(mask, np.float64)
    a64, b64 = np.asarray(a, np.float64)[:, None] * m, np.asarray(b, np.float64)[:, None] * m
    w1, w2 = np.asarray(w1, np.float64)[:, :, None, None], np.asarray(w2, np.float64)[:, :, None, None]
    half_ulp = 0.5 * np.spacing(np.abs(np.asarray(v, np.float64).astype(np.float32))).astype(np.float64)
    return half_ulp + 1e-10 * (np.abs(w1 * a64) + np.abs(w2 * b64))


# ---- the DDIM encode loop ----------------------------------------------------------------------------------------------------
def encode_levels(sde, timesteps):
    """(k, k_next) table indices of the upward steps i = 1 .. len-1 of sampling.ddim_sampler(encode=True)."""
    N = sde.N
    idx = [int((t * (N - 1) / sde.T).long()) for t in timesteps]
    return [(idx[i - 1], idx[i]) for i in range(1, len(timesteps))]


def encode_rows(sde, timesteps):
    """[steps, 4] float64 rows {a1, a2, a1_next/a1, a2_next/a2} of those steps, from the SDE's float32 tables widened."""
    sa, s1 = sde.sqrt_alphas_cumprod.double().cpu(), sde.sqrt_1m_alphas_cumprod.double().cpu()
    return torch.stack([torch.stack([sa[k], s1[k], sa[kn] / sa[k], s1[kn] / s1[k]]) for k, kn in encode_levels(sde, timesteps)])


def ddim_encode_recursion(sde, s, x, gm, timesteps, n_iters=None):
    """sampling.ddim_sampler(encode=True) in float64 for the closed-form model eps_hat = k_t x, written like
    guidance_cases.ddim_recursion: the network input is the state rounded to float32 and eps_hat is rounded to float32, as in the
    loop.  x [B, C, R, R, R] data grids; gm [R, R, R] float64.  Returns the state at the top level."""
    N, B = sde.N, x.shape[0]
    x = x.double() * gm
    rows = encode_rows(sde, timesteps)
    steps = range(1, len(timesteps)) if n_iters is None else range(1, len(timesteps))[:n_iters]
    for i in steps:
        a1, a2, r1, r2 = rows[i - 1]
        k = gc.gaussian_k((timesteps[i - 1].float() * (N - 1)).expand(B), s, N)
        e = (k.view(-1, 1, 1, 1, 1) * x.float().double()).float().double()
        x0s = x - a2 * e
        x = (r1 * x + (r2 - r1) * (x - x0s)) * gm
    return x


def ddim_encode_oracle(eps_fn, x, mask, N=1000, n_iters=None):
    """The same loop around an oracle forward eps_fn(x float32, labels) on the CPU, on the 100-point quadratic schedule, with the
    oracle's own ddim_step (its coefficient row serves either direction of time)."""
    from oracle import unet_oracle as uo
    seq = [int(v) for v in list(np.linspace(0, np.sqrt(N * 0.8), 100) ** 2)]
    timesteps = torch.tensor(seq) / N
    x = x.double() * mask
    steps = range(1, len(timesteps)) if n_iters is None else range(1, len(timesteps))[:n_iters]
    for i in steps:
        vec_t = torch.ones(x.shape[0]) * timesteps[i - 1]
        vec_tn = torch.ones(x.shape[0]) * timesteps[i]
        e = eps_fn(x.float(), vec_t.float() * (N - 1))
        x = uo.ddim_step(x, e, vec_t, vec_tn, N)[0] * mask
    return x


# ---- the closed-form probability flow ----------------------------------------------------------------------------------------
def gaussian_flow_factor(s, t0, t1):
    """The probability flow of data ~ N(0, s^2 I) under the VP SDE scales a point by the ratio of the marginal standard deviations:
    x(t1) = x(t0) * sqrt((alpha_1^2 s^2 + sigma_1^2) / (alpha_0^2 s^2 + sigma_0^2))."""
    def var(t):
        lmc = -0.25 * t * t * (gc.BETA1 - gc.BETA0) - 0.5 * t * gc.BETA0
        return np.exp(2.0 * lmc) * s * s - np.expm1(2.0 * lmc)
    return float(np.sqrt(var(t1) / var(t0)))
