"""Log-likelihood in bits/dim through the probability-flow ODE -- mirror of the reference's lib/diffusion/likelihood.py
(get_div_fn :26-37, get_likelihood_fn :40-113): the ODE  dx/dt = -0.5 beta(t) x - 0.5 beta(t) score(x, t)  is integrated from
`eps` to T together with  d(logp)/dt = div(drift), the divergence estimated with ONE Hutchinson probe drawn per solve.

What differs from the reference:
  * it runs.  The reference builds its score with `get_score_fn(continuous=True)`, which asserts; here the
    continuous-time score is formed in this file: labels t*(N-1), sigma(t) = sde.marginal_prob(., t)[1], beta(t) from sde.sde.
    `mutils.get_score_fn(continuous=True)` keeps asserting.
  * the integrator is Dormand-Prince 5(4) in torch ops (`rk45`): scipy's tableau, initial-step selection and step controller
    (scipy.integrate.solve_ivp(method='RK45'): safety 0.9, factors in [0.2, 10], RMS error norm over the whole flattened state,
    the B log-density entries included), so on the same right-hand side it takes scipy's steps -- with the float64 state on the
    model's device throughout.  scipy is not imported.
  * for a DDPMUNet3D on a GPU one evaluation is: eval-mode taped forward with x.requires_grad, the data-gradient-only HIP backward
    with the probe as cotangent (J^T probe; no weight-gradient work, no `.grad`), and one md_pf_ode_rhs launch for drift and
    divergence.  Any other callable takes the reference's div_fn in plain torch autograd, in the dtype of `data`.
  * `grid_mask`: state, probe and drift are masked and the dimension count is C * mask.sum() in the prior term and the division.
"""
import math

import numpy as np
import torch

from . import sde_lib
from .models import utils as mutils

# Dormand-Prince 5(4) (Dormand & Prince 1980; the coefficients scipy's RK45 uses)
_C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0)
_A = ((),
      (1 / 5,),
      (3 / 40, 9 / 40),
      (44 / 45, -56 / 15, 32 / 9),
      (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
      (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656))
_B = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84)
_E = (-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40)
_SAFETY, _MIN_FACTOR, _MAX_FACTOR, _ERR_EXP = 0.9, 0.2, 10.0, -1.0 / 5.0


def _rms(v):
    return float(torch.linalg.vector_norm(v)) / math.sqrt(v.numel())


def _combine(y, h, ks, ws):
    """y + h * sum_i ws[i] * ks[i], skipping zero weights (y None: the sum times h alone)."""
    out = None
    for k, w in zip(ks, ws):
        if w != 0.0:
            out = k * w if out is None else out.add_(k, alpha=w)
    out.mul_(h)
    return out if y is None else out.add_(y)


def rk45(fun, t_span, y0, rtol=1e-3, atol=1e-6):
    """Integrate dy/dt = fun(t, y) over t_span = (t0, t1) from the flat float64 torch vector y0.  fun(t: float, y) returns a
    float64 vector like y on y's device.  Returns (y(t1), nfev, accepted steps).  The algorithm of
    scipy.integrate.solve_ivp(method='RK45') with its defaults (no max_step, no first_step)."""
    t0, t1 = float(t_span[0]), float(t_span[1])
    assert y0.dtype == torch.float64 and y0.dim() == 1
    rtol = max(float(rtol), 100 * np.finfo(float).eps)
    direction = float(np.sign(t1 - t0)) if t1 != t0 else 1.0
    nfev = [0]

    def f(t, y):
        nfev[0] += 1
        return fun(t, y)

    t, y = t0, y0.clone()
    fy = f(t, y)
    # first step (Hairer, Norsett, Wanner, Solving ODEs I, II.4)
    length = abs(t1 - t0)
    if length == 0.0:
        return y, nfev[0], 0
    scale = atol + y.abs() * rtol
    d0, d1 = _rms(y / scale), _rms(fy / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    h0 = min(h0, length)
    f1 = f(t + h0 * direction, y + (h0 * direction) * fy)
    d2 = _rms((f1 - fy) / scale) / h0
    h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1.0 / 5.0)
    h_abs = min(100 * h0, h1, length)
    del f1, scale
    steps = 0
    while direction * (t - t1) < 0:
        min_step = 10 * abs(float(np.nextafter(t, direction * np.inf)) - t)
        h_abs = max(h_abs, min_step)
        rejected = False
        while True:
            if h_abs < min_step:
                raise RuntimeError("rk45: the required step size is below the spacing between numbers")
            t_new = t + h_abs * direction
            if direction * (t_new - t1) > 0:
                t_new = t1
            h = t_new - t
            h_abs = abs(h)
            ks = [fy]
            for s in range(1, 6):
                ks.append(f(t + _C[s] * h, _combine(y, h, ks, _A[s])))
            y_new = _combine(y, h, ks, _B)
            f_new = f(t + h, y_new)
            ks.append(f_new)
            scale = atol + torch.maximum(y.abs(), y_new.abs()) * rtol
            err = _rms(_combine(None, h, ks, _E) / scale)
            del ks, scale
            if err < 1.0:
                factor = _MAX_FACTOR if err == 0.0 else min(_MAX_FACTOR, _SAFETY * err ** _ERR_EXP)
                if rejected:
                    factor = min(1.0, factor)
                h_abs *= factor
                break
            h_abs *= max(_MIN_FACTOR, _SAFETY * err ** _ERR_EXP)
            rejected = True
        t, y, fy = t_new, y_new, f_new
        steps += 1
    return y, nfev[0], steps


def vp_coefficients(sde, t):
    """(c_x, c_e) = (-0.5 beta(t), 0.5 beta(t) / sigma(t)) as Python floats, formed in float64 from the SDE's own expressions:
    drift of the probability-flow ODE = c_x x + c_e eps_hat with score = -eps_hat / sigma(t)."""
    tt = torch.tensor([float(t)], dtype=torch.float64)
    one = torch.ones((1, 1, 1, 1, 1), dtype=torch.float64)
    beta = float(sde.sde(one, tt)[1][0]) ** 2
    sigma = float(sde.marginal_prob(one, tt)[1][0])
    return -0.5 * beta, 0.5 * beta / sigma


def _hip_net(model, data):
    """The DDPMUNet3D behind `model` when the HIP right-hand side applies (data on a GPU; the network always sees the float32
    cast of the float64 state, whatever the dtype of `data`), else None."""
    from .models.ddpm_res64 import DDPMUNet3D
    net = getattr(model, "module", model)
    return net if (isinstance(net, DDPMUNet3D) and data.is_cuda) else None


def _eps_fn(model):
    """eps_hat(x, labels) of a score model in eval mode (an nn.Module), or of any callable as it is."""
    return mutils.get_model_fn(model, train=False) if isinstance(model, torch.nn.Module) else model


def get_ode_rhs(sde, model, shape, data_like, grid_mask=None, probe=None):
    """fun(t, y) for `rk45` on the flat float64 state [x | logp (B entries, only with `probe`)].
    With `probe` the log-density entries get the Hutchinson estimate probe . d(drift)/dx . probe; without it the state is x alone
    and no gradient is taken (the ODE sampler: the model's inference path under no_grad)."""
    if not isinstance(sde, sde_lib.VPSDE):
        raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
    B, n = shape[0], int(np.prod(shape))
    dev = data_like.device
    net = _hip_net(model, data_like)
    eps_fn = _eps_fn(model)
    mask_flat = None if grid_mask is None else grid_mask.to(dev).reshape(-1).contiguous()

    if net is not None:
        from ... import hip_ops as ops
        m32 = None if mask_flat is None else mask_flat.float().contiguous()
        p32 = None if probe is None else probe.float().contiguous()

        def fun(t, y):
            x = y[:n].view(shape).float()
            labels = torch.full((B,), float(t) * (sde.N - 1), dtype=torch.float32, device=dev)
            cx, ce = vp_coefficients(sde, t)
            coef = torch.tensor([[cx, ce]] * B, dtype=torch.float64, device=dev)
            if p32 is None:
                with torch.no_grad():
                    eps_hat = eps_fn(x, labels)
                return ops.pf_ode_rhs(x, eps_hat, m32, coef)[0].double().view(-1)
            with torch.enable_grad():
                xr = x.detach().requires_grad_(True)
                eps_hat = eps_fn(xr, labels)
                g, = torch.autograd.grad(eps_hat, xr, p32)          # J^T probe: the data-gradient-only HIP backward
            drift, div = ops.pf_ode_rhs(x, eps_hat.detach(), m32, coef, g=g, probe=p32)
            return torch.cat([drift.double().view(-1), div])
        return fun

    dtype = data_like.dtype
    mask = None if mask_flat is None else mask_flat.to(dtype).view((1, 1) + tuple(shape[2:]))
    pr = None if probe is None else probe.to(dtype)
    dims = tuple(range(1, len(shape)))

    def drift_of(x, t):
        cx, ce = vp_coefficients(sde, t)
        labels = torch.full((B,), float(t) * (sde.N - 1), dtype=dtype, device=dev)
        d = cx * x + ce * eps_fn(x, labels)
        return d if mask is None else d * mask

    def fun(t, y):
        x = y[:n].view(shape).to(dtype)
        if pr is None:
            with torch.no_grad():
                return drift_of(x, t).double().reshape(-1)
        with torch.enable_grad():
            xr = x.detach().requires_grad_(True)
            drift = drift_of(xr, t)
            g, = torch.autograd.grad(torch.sum(drift * pr), xr)
        div = torch.sum(g * pr, dim=dims)
        return torch.cat([drift.detach().double().reshape(-1), div.double()])
    return fun


def get_likelihood_fn(sde, inverse_scaler, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45', eps=1e-5,
                      grid_mask=None, generator=None):
    """Returns likelihood_fn(model, data, return_parts=False, probe=None) -> (bpd [B], z like data, nfe); with return_parts also
    (delta_logp, prior_logp) in nats (float64): the fixed offset of bits/dim hides errors that they show.
    grid_mask: binary tensor with the grid's D*H*W entries; generator: torch.Generator of the probe's draw (on data's device);
    probe: a given Hutchinson probe instead of a drawn one."""
    if method != 'RK45':
        raise NotImplementedError(f"ODE method {method!r}: only 'RK45' (Dormand-Prince 5(4)) is implemented")
    if hutchinson_type not in ('Rademacher', 'Gaussian'):
        raise NotImplementedError(f"Hutchinson type {hutchinson_type} unknown.")

    def likelihood_fn(model, data, return_parts=False, probe=None):
        from .sampling import _refuse_cfg
        _refuse_cfg(model, "the likelihood (the divergence needs the Jacobian of the combined output)")
        with torch.no_grad():
            shape, dev = tuple(data.shape), data.device
            B = shape[0]
            mask = None if grid_mask is None else grid_mask.to(dev).reshape((1, 1) + shape[2:]).to(data.dtype)
            if probe is None:
                if hutchinson_type == 'Gaussian':
                    probe = torch.randn(shape, dtype=data.dtype, device=dev, generator=generator)
                else:
                    probe = torch.randint(0, 2, shape, device=dev, generator=generator).to(data.dtype) * 2 - 1.
            probe = probe.to(device=dev, dtype=data.dtype)
            x0 = data
            if mask is not None:
                probe, x0 = probe * mask, data * mask
            fun = get_ode_rhs(sde, model, shape, data, grid_mask=grid_mask, probe=probe)
            y0 = torch.cat([x0.double().reshape(-1), torch.zeros(B, dtype=torch.float64, device=dev)])
            y1, nfe, _ = rk45(fun, (eps, sde.T), y0, rtol=rtol, atol=atol)
            z64 = y1[:-B].view(shape)
            delta_logp = y1[-B:].clone()
            z = z64.to(data.dtype)
            n_dim = float(np.prod(shape[1:])) if mask is None else float(shape[1] * mask.sum().item())
            if mask is None:
                prior_logp = sde.prior_logp(z).double()
            else:                   # the masked entries of z are zero and are no dimensions of the density
                prior_logp = -n_dim / 2.0 * np.log(2 * np.pi) - torch.sum(z64 ** 2, dim=tuple(range(1, len(shape)))) / 2.0
            bpd = -(prior_logp + delta_logp) / np.log(2)
            bpd = bpd / n_dim
            bpd = bpd + (7. - inverse_scaler(-1.))          # the reference's offset from nats/dim of scaled data to bits/dim
            bpd = bpd.to(torch.float32)
            if return_parts:
                return bpd, z, nfe, delta_logp, prior_logp
            return bpd, z, nfe

    return likelihood_fn
