"""Probability-flow ODE likelihood, host side (no GPU): the torch Dormand-Prince integrator takes scipy's steps; the likelihood
of an analytic Gaussian score model equals its closed form, with and without a grid mask; the float64 restatement of
md_pf_ode_rhs (the GPU test's reference) agrees with autograd; refusals."""
import math

import numpy as np
import pytest
import torch

import likelihood_cases as lc


def _sde():
    from meshdiffusion_amd.lib.diffusion import sde_lib
    return sde_lib.VPSDE(lc.BETA0, lc.BETA1, lc.N_SCALES, device="cpu")


@pytest.mark.parametrize("tol", [1e-3, 1e-6])
@pytest.mark.parametrize("case", sorted(lc.ODE_CASES))
def test_rk45_takes_scipys_steps(case, tol):
    integrate = pytest.importorskip("scipy.integrate")
    from meshdiffusion_amd.lib.diffusion import likelihood
    fun, span, y0 = lc.ODE_CASES[case]
    sol = integrate.solve_ivp(lambda t, y: fun(float(t), torch.from_numpy(np.asarray(y, np.float64))).numpy(), span,
                              np.array(y0), rtol=tol, atol=tol, method="RK45")
    assert sol.status == 0
    y, nfev, steps = likelihood.rk45(fun, span, torch.tensor(y0, dtype=torch.float64), rtol=tol, atol=tol)
    ref = sol.y[:, -1]
    err = np.abs(y.numpy() - ref).max() / np.abs(ref).max()
    print(f"{case} tol {tol:g}: nfev {nfev} / scipy {sol.nfev}, steps {steps} / scipy {len(sol.t) - 1}, rel err {err:.2e}")
    assert nfev == sol.nfev and steps == len(sol.t) - 1
    assert err <= 1e-9


@pytest.mark.parametrize("masked", [False, True])
def test_analytic_gaussian_likelihood(masked):
    """data ~ N(0, s^2 I): prior_logp + delta_logp is the log-density of N(0, (alpha_eps^2 s^2 + sigma_eps^2) I) at the data.
    The Jacobian of the exact eps-prediction is a multiple of the identity, so one Rademacher probe gives the exact divergence."""
    from meshdiffusion_amd.lib.diffusion import likelihood
    s, eps, R, B, C = 0.7, 1e-5, 4, 3, 4
    sde = _sde()
    g = torch.Generator().manual_seed(5)
    data = torch.randn((B, C, R, R, R), generator=g, dtype=torch.float64) * s
    mask = (torch.rand((R, R, R), generator=g) < 0.4).double() if masked else None
    n_dim = C * (int(mask.sum()) if masked else R ** 3)
    assert 0 < n_dim < C * R ** 3 or not masked
    inverse_scaler = lambda x: (x + 1.0) / 2.0          # noqa: E731   a non-trivial one: the offset is 7 - inverse_scaler(-1) = 7
    fn = likelihood.get_likelihood_fn(sde, inverse_scaler, rtol=1e-8, atol=1e-8, eps=eps, grid_mask=mask,
                                      generator=torch.Generator().manual_seed(6))
    calls = [0]
    model = lc.gaussian_eps_model(s)

    def counted(x, labels):
        calls[0] += 1
        return model(x, labels)

    bpd, z, nfe, delta_logp, prior_logp = fn(counted, data, return_parts=True)
    assert nfe == calls[0] and nfe > 8 and (nfe - 2) % 6 == 0       # f(t0), the first-step probe, six per attempted step
    assert z.shape == data.shape and z.dtype == data.dtype and bpd.shape == (B,)
    x = data * mask.view(1, 1, R, R, R) if masked else data
    _, _, a, sg = lc.vp_coefficients_f64(eps)
    want = lc.gaussian_logp(x, a * a * s * s + sg * sg, n_dim)
    got = prior_logp + delta_logp
    rel = ((got - want).abs() / want.abs()).max().item()
    print(f"masked={masked}: n_dim {n_dim}, nfe {nfe}, logp {got.tolist()} vs {want.tolist()}, rel {rel:.2e}")
    assert rel <= 1e-5
    if masked:
        assert float((z * (1 - mask.view(1, 1, R, R, R))).abs().max()) == 0.0       # the masked entries never move
    # z is the data pushed to the prior: N(0, (alpha_T^2 s^2 + sigma_T^2) I) scaled from the eps marginal
    _, _, aT, sT = lc.vp_coefficients_f64(1.0)
    scale = math.sqrt((aT * aT * s * s + sT * sT) / (a * a * s * s + sg * sg))
    assert float((z - x * scale).abs().max()) <= 1e-6
    # bits/dim: the reference's three lines (likelihood.py:105-110), with the masked dimension count
    ref_bpd = -(prior_logp + delta_logp) / np.log(2)
    ref_bpd = ref_bpd / n_dim
    ref_bpd = ref_bpd + (7. - inverse_scaler(-1.))
    assert torch.allclose(bpd.double(), ref_bpd, rtol=0, atol=1e-6 * float(ref_bpd.abs().max()))
    # without return_parts: the reference's triple
    out = fn(model, data, probe=torch.ones_like(data))
    assert len(out) == 3 and torch.allclose(out[0], bpd, rtol=1e-6, atol=0)


def test_refusals():
    from meshdiffusion_amd.lib.diffusion import likelihood, sampling
    from meshdiffusion_amd.lib.diffusion.models import utils as mutils
    sde = _sde()
    with pytest.raises(AssertionError):         # continuous-time score functions stay asserted away, as in the reference
        mutils.get_score_fn(sde, lambda x, t: x, train=False, continuous=True)
    with pytest.raises(NotImplementedError):
        likelihood.get_likelihood_fn(sde, lambda x: x, method="RK23")
    with pytest.raises(NotImplementedError):
        likelihood.get_likelihood_fn(sde, lambda x: x, hutchinson_type="Sobol")
    import inspect
    sig = inspect.signature(likelihood.get_likelihood_fn)
    assert [(k, v.default) for k, v in sig.parameters.items()][2:7] == [
        ("hutchinson_type", "Rademacher"), ("rtol", 1e-5), ("atol", 1e-5), ("method", "RK45"), ("eps", 1e-5)]
    from meshdiffusion_amd import synth
    cfg = synth.small_config()
    cfg.device = torch.device("cpu")
    cfg.sampling.method = "ode"
    assert callable(sampling.get_sampling_fn(cfg, sde, (2, 4, 16, 16, 16), lambda x: x, 1e-3))


def test_ode_sampler_inverts_the_encoding_on_the_analytic_model():
    """get_ode_sampler(x0=z) runs the same ODE backwards: the data comes back (CPU route, float64)."""
    from meshdiffusion_amd.lib.diffusion import likelihood, sampling
    sde, s, R = _sde(), 0.7, 4
    data = torch.randn((2, 4, R, R, R), generator=torch.Generator().manual_seed(1), dtype=torch.float64) * s
    model = lc.gaussian_eps_model(s)
    _, z, _ = likelihood.get_likelihood_fn(sde, lambda x: x, rtol=1e-8, atol=1e-8, eps=1e-3)(model, data)
    back, nfe = sampling.get_ode_sampler(sde, data.shape, lambda x: x, rtol=1e-8, atol=1e-8, eps=1e-3, device="cpu")(model, x0=z)
    assert nfe > 8 and float((back - data).abs().max()) <= 1e-6


def test_host_restatement_of_pf_ode_rhs_against_autograd():
    """pf_ode_rhs_f64 (the GPU test's reference) is the drift of the masked ODE and probe . d(drift)/dx . probe of a model whose
    Jacobian is known: eps_hat = tanh(w * x) elementwise, so J^T probe = w (1 - tanh^2) probe."""
    g = torch.Generator().manual_seed(3)
    B, C, P = 3, 4, 64
    x = torch.randn((B, C, P), generator=g)
    w = torch.randn((C, P), generator=g)
    probe = (torch.randint(0, 2, (B, C, P), generator=g).float() * 2 - 1)
    mask = (torch.rand(P, generator=g) < 0.5).float()
    coef = np.array([lc.vp_coefficients_f64(t)[:2] for t in (1e-3, 0.5, 1.0)])
    xr = x.double().requires_grad_(True)
    cc = torch.from_numpy(coef)
    drift = (cc[:, 0].view(B, 1, 1) * xr + cc[:, 1].view(B, 1, 1) * torch.tanh(w.double() * xr)) * mask.double()
    pm = probe.double() * mask.double()
    gr, = torch.autograd.grad((drift * pm).sum(), xr)
    want_div = (gr * pm).sum(dim=(1, 2)).numpy()
    eps_hat = torch.tanh(w * x)
    jt = (w.double() * (1 - torch.tanh(w.double() * x.double()) ** 2) * pm).float()
    d, div, mag = lc.pf_ode_rhs_f64(x.numpy(), eps_hat.numpy(), mask.numpy(), coef, g=jt.numpy(), probe=pm.float().numpy())
    assert d.dtype == np.float32 and np.abs(d - drift.detach().numpy()).max() <= 1e-5 * np.abs(d).max()
    assert np.all(np.abs(div - want_div) <= 1e-5 * mag)
    d2, none, _ = lc.pf_ode_rhs_f64(x.numpy(), eps_hat.numpy(), None, coef)
    assert none is None and np.array_equal(d2 * mask.numpy(), d)


def test_pf_ode_rhs_refuses_bad_arguments(hip_lib):
    import ctypes as C
    from meshdiffusion_amd import _lib
    buf = C.create_string_buffer(4096 + 64)
    one = C.c_void_p((C.addressof(buf) + 63) & ~63)
    odd = C.c_void_p(one.value + 4)
    nul = C.c_void_p(0)
    f = hip_lib.md_pf_ode_rhs
    bad = _lib.ERR_BAD_ARG
    assert f(nul, one, nul, nul, nul, one, one, nul, 2, 4, 64, nul) == bad           # no state
    assert f(one, one, nul, nul, nul, nul, one, nul, 2, 4, 64, nul) == bad           # no coefficients
    assert f(one, one, nul, nul, nul, one, one, nul, 2, 4, 66, nul) == bad           # P % 4
    assert f(one, one, one, nul, nul, one, one, one, 2, 4, 64, nul) == bad           # g without probe
    assert f(one, one, one, one, nul, one, one, nul, 2, 4, 64, nul) == bad           # divergence without slabs
    assert f(odd, one, nul, nul, nul, one, one, nul, 2, 4, 64, nul) == bad           # misaligned
    assert f(one, one, nul, nul, nul, one, one, nul, 0, 4, 64, nul) == bad           # empty batch
    sd = hip_lib.md_conv3_stem_dgrad
    assert sd(nul, one, one, 1, 32, 16, 8, 8, 8, nul) == bad and sd(one, one, odd, 1, 32, 16, 8, 8, 8, nul) == bad
    assert sd(one, one, one, 0, 32, 16, 8, 8, 8, nul) == bad
    for args in ((1, 48, 16, 8, 8, 8), (1, 32, 16, 6, 8, 8), (1, 32, 16, 8, 12, 8), (1, 32, 16, 8, 8, 4), (1, 32, 40, 8, 8, 8), (1, 32, 12, 8, 8, 8)):
        assert sd(one, one, one, *args, nul) == _lib.ERR_UNSUPPORTED, args
