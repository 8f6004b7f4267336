"""DPM-Solver++ on the host (no GPU): the closed-form inverse of the half-log-SNR, the update's weights against quadrature of
their defining integrals, exactness on polynomials, the rows' identities, the convergence order on a closed-form model and the
order sequence under lower_order_final."""
import math

import numpy as np
import pytest
import torch

import dpmpp_cases as dc
import guidance_cases as gc
from meshdiffusion_amd.lib.diffusion import sampling, sde_lib


@pytest.fixture(scope="module")
def sde():
    return sde_lib.VPSDE(dc.BETA0, dc.BETA1, 1000, device="cpu")


def test_inverse_lambda(sde):
    lam = np.linspace(sampling.vp_lambda(sde, 1.0), sampling.vp_lambda(sde, 1e-3), 20001)
    t = sampling.vp_t_of_lambda(sde, lam)
    err = float(np.abs(sampling.vp_lambda(sde, t) - lam).max())
    print(f"max |lambda(t(lambda)) - lambda| over [{lam[0]:.3f}, {lam[-1]:.3f}]: {err:.2e}")
    assert np.all(np.diff(t) < 0) and abs(t[0] - 1.0) < 1e-12 and abs(t[-1] - 1e-3) < 1e-12
    assert err <= 1e-12
    for t0 in (1e-3, 0.3, 1.0):                       # the schedule against the restatement of the tests
        a, s, l = dc.alpha_sigma_lambda(t0)
        lmc, sig = sampling.vp_log_alpha_sigma(sde, t0)
        assert abs(math.exp(lmc) - a) <= 1e-15 and abs(sig - s) <= 1e-15 and abs(sampling.vp_lambda(sde, t0) - l) <= 1e-14
    for kind in ("logsnr", "uniform", "quad"):
        ts = sampling.dpmpp_schedule(sde, 20, kind, 1e-3)
        assert ts.dtype == torch.float64 and ts.shape == (21,) and float(ts[0]) == 1.0 and float(ts[-1]) == 1e-3
        assert bool((ts[1:] < ts[:-1]).all())
    d = np.diff(sampling.vp_lambda(sde, sampling.dpmpp_schedule(sde, 20).numpy()))
    assert np.abs(d - d.mean()).max() <= 1e-12        # 'logsnr' is uniform in lambda
    assert np.abs(np.diff(np.sqrt(sampling.dpmpp_schedule(sde, 20, "quad").numpy()), 2)).max() <= 1e-15
    with pytest.raises(ValueError):
        sampling.dpmpp_schedule(sde, 20, "cosine")


@pytest.mark.parametrize("tau", [0, 1])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_weights_against_quadrature(order, tau):
    worst = 0.0
    for h in (1e-4, 1e-3, 1e-2, 0.1, 1.0, 3.0):
        for r in (0.5, 1.0, 2.0):
            rs = [r] * (order - 1)
            got = sampling.dpmpp_weights(h, rs, order, "taylor", tau)
            for j, (want, est) in enumerate(dc.weights_by_quadrature(h, rs, order, tau)):
                tol = max(1e-11 * abs(want), est)
                err = abs(got[j] - want)
                worst = max(worst, err / abs(want))
                assert err <= tol, (h, r, j, got[j], want, est)
    print(f"order {order} tau {tau}: worst relative distance from quadrature {worst:.2e}")


def test_the_plain_recursion_would_fail_at_small_h():
    """What the series branch is for: I_2 from the recursion alone is off by more than the bar at h <= 1e-3."""
    for h in (1e-4, 1e-3):
        i0 = -math.expm1(-h)
        i1 = 1.0 - i0 / h
        i2 = 1.0 - 2.0 * i1 / h
        want = dc.weights_by_quadrature(h, [1.0, 1.0], 3, 0)                     # l_2 = (u^2 + u)/2 on the nodes 0, -1, -2
        got = sampling.dpmpp_moments(h, 2)
        plain = (i2 + i1) / 2.0
        assert abs(plain - want[2][0]) > 1e-11 * abs(want[2][0])
        assert abs((got[2] + got[1]) / 2.0 - want[2][0]) <= 1e-11 * abs(want[2][0])


@pytest.mark.parametrize("tau", [0, 1])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_exact_on_polynomials(sde, order, tau):
    """x0(lambda) a polynomial of degree order-1: one step of that order from the exact state is exact (to 1e-12)."""
    times = np.array([0.9, 0.8, 0.68, 0.55])[3 - order:]                    # non-uniform steps; the last one is the step under test
    lam = [dc.alpha_sigma_lambda(t)[2] for t in times]
    pc = [0.7, -0.4, 0.25][:order]
    x0 = lambda l: sum(c * (l - lam[-2]) ** k for k, c in enumerate(pc))     # noqa: E731
    rows, labels = sampling.dpmpp_tables(sde, times, order=order, variant="taylor", tau=tau, lower_order_final=False)
    assert rows.shape == (order, 8) and rows.dtype == torch.float64 and float(labels[-1]) == times[-2] * 999
    row = rows[-1].numpy()
    x_s = 1.3
    got = row[2] * x_s + sum(row[3 + j] * x0(lam[-2 - j]) for j in range(order))
    want = dc.exact_step(times[-2], times[-1], x_s, x0, tau)
    a_s, s_s, _ = dc.alpha_sigma_lambda(times[-2])
    print(f"order {order} tau {tau}: |step - exact| = {abs(got - want):.2e}")
    assert abs(got - want) <= 1e-12 and row[0] == a_s and row[1] == s_s and row[7] == 0.0
    assert (row[6] > 0.0) == bool(tau) and np.all(row[3 + order:6] == 0.0)


def test_row_identities(sde):
    ts, tm, tt = 0.7, 0.52, 0.4
    (a_s, s_s, l_s), (a_m, s_m, l_m), (a_t, s_t, l_t) = (dc.alpha_sigma_lambda(t) for t in (ts, tm, tt))
    # order 1, tau 0 is DDIM: x_t = alpha_t x0 + sigma_t eps with eps = (x - alpha_s x0)/sigma_s
    row = sampling.dpmpp_tables(sde, [ts, tt], order=1, tau=0)[0][0].numpy()
    assert abs(row[2] - s_t / s_s) <= 1e-13 and abs(row[3] - (a_t - s_t * a_s / s_s)) <= 1e-13 and row[6] == 0.0
    # order 1, tau 1: two steps compose into one
    two = sampling.dpmpp_tables(sde, [ts, tm, tt], order=1, tau=1)[0].numpy()
    one = sampling.dpmpp_tables(sde, [ts, tt], order=1, tau=1)[0][0].numpy()
    assert abs(two[1, 2] * two[0, 2] - one[2]) <= 1e-13
    assert abs(two[1, 2] * two[0, 3] + two[1, 3] - one[3]) <= 1e-13
    assert abs(two[1, 6] ** 2 + two[1, 2] ** 2 * two[0, 6] ** 2 - one[6] ** 2) <= 1e-13
    # order 2 'midpoint' equals its formula, under both tau
    for tau in (0, 1):
        row = sampling.dpmpp_tables(sde, [ts, tm, tt], order=2, variant="midpoint", tau=tau, lower_order_final=False)[0][1].numpy()
        h, r = l_t - l_m, (l_m - l_s) / (l_t - l_m)
        i0 = -math.expm1(-(2.0 * h if tau else h))
        assert abs(row[3] - a_t * i0 * (1.0 + 0.5 / r)) <= 1e-13 and abs(row[4] + a_t * i0 * 0.5 / r) <= 1e-13 and row[5] == 0.0
        assert abs(row[2] - s_t / s_m * (math.exp(-h) if tau else 1.0)) <= 1e-13
    with pytest.raises(ValueError):
        sampling.dpmpp_tables(sde, [tt, ts], order=1)
    with pytest.raises(ValueError):
        sampling.dpmpp_tables(sde, [ts, tt], order=4)


BANDS = {(1, "taylor"): (1.8, 2.2), (2, "taylor"): (3.5, 4.5), (2, "midpoint"): (3.5, 4.5), (3, "taylor"): (8.0, math.inf)}


@pytest.mark.parametrize("s", [1.0, 0.5])
@pytest.mark.parametrize("order,variant", list(BANDS))
def test_convergence_order(order, variant, s):
    """eps_hat = k_t x (data ~ N(0, s^2 I)): the error against the exact solution of the probability-flow ODE falls by 2^order per
    doubling of the steps.  Measured here: order 1 ratios 1.9-2.0, order 2 3.7-4.1 (both variants), order 3 15.8-16.6."""
    N = 1000
    sde = sde_lib.VPSDE(dc.BETA0, dc.BETA1, N, device="cpu")
    model = gc.GaussianEps(s, N)
    x_T = torch.randn((1, 1, 4, 4, 4), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    want = dc.gaussian_exact(x_T, s, 1.0, 1e-3)
    errs = []
    for steps in (20, 40, 80):
        times = sampling.dpmpp_schedule(sde, steps, "logsnr", 1e-3)
        rows, labels = sampling.dpmpp_tables(sde, times, order=order, variant=variant, tau=0, lower_order_final=False)
        got = dc.recursion(model, x_T, rows, labels, sampling.dpmpp_orders(steps, order, False), round_state=False)
        errs.append(float((got - want).norm() / want.norm()))
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print(f"order {order} {variant} s {s}: errors {['%.3e' % e for e in errs]}, ratios {['%.2f' % r for r in ratios]}")
    lo, hi = BANDS[(order, variant)]
    assert all(lo <= r <= hi for r in ratios)


def test_order_sequence():
    assert sampling.dpmpp_orders(10, 3) == [1, 2, 3, 3, 3, 3, 3, 3, 2, 1]
    assert sampling.dpmpp_orders(10, 2) == [1, 2, 2, 2, 2, 2, 2, 2, 2, 1]
    assert sampling.dpmpp_orders(20, 3) == [1, 2] + [3] * 18                 # 15 steps or more: only the history caps
    assert sampling.dpmpp_orders(10, 3, lower_order_final=False) == [1, 2] + [3] * 8
    sde = sde_lib.VPSDE(dc.BETA0, dc.BETA1, 1000, device="cpu")
    rows = sampling.dpmpp_tables(sde, sampling.dpmpp_schedule(sde, 10), order=3)[0].numpy()
    used = [1 + int(r[4] != 0.0) + int(r[5] != 0.0) for r in rows]
    assert used == sampling.dpmpp_orders(10, 3)


def test_kernel_bars_leave_room_for_a_float64_chain():
    """The bars of tests/test_gpu_dpmpp.py::test_multistep_kernel hold for a plain float64 chain in the kernel's order, on the
    same inputs and rows: the GPU test asks nothing that float64 arithmetic cannot give."""
    sde = sde_lib.VPSDE(dc.BETA0, dc.BETA1, 1000, device="cpu")
    rows = sampling.dpmpp_tables(sde, sampling.dpmpp_schedule(sde, 20), order=3, tau=1, lower_order_final=False)[0].numpy()
    for B, C, P in ((1, 1, 4), (3, 4, 1028)):
        t = {k: v.numpy() for k, v in dc.kernel_inputs(B, C, P, seed=P).items()}
        coef = rows[[5, 11, 17][:B]]
        args = (t["x"], t["eps"], t["h1"], t["h2"], t["z"], t["mask"], coef, t["partial"], t["pmask"], C - 1)
        ref = dc.multistep_ref(*args)
        xn, x0, _ = dc.multistep_chain_f64(*args)
        k = ref["keep"]
        assert np.all(np.abs(x0 - ref["x0"])[k] <= (4 * dc.U * ref["x0_bar"])[k])
        assert np.all(np.abs(xn - ref["x_new"])[k] <= (8 * dc.U * ref["terms"])[k])


def test_multistep_step_refuses_aliased_outputs(hip_lib):
    """The aliasing table of md_multistep_step on host addresses (nothing here may reach a kernel): every output against every
    input and against the outputs after it, whole tensors and partial overlaps."""
    import ctypes as C
    from meshdiffusion_amd import _lib
    B, Cc, P = 2, 4, 64                                                                # 4 KiB per float64 tensor, 2 KiB per float32 one
    names = ["x", "eps", "h1", "h2", "z", "mask", "coef", "partial", "pmask", "x_out", "x0_out", "x_f32"]
    buf = C.create_string_buffer(8192 * len(names) + 64)
    base = (C.addressof(buf) + 63) & ~63
    good = {n: base + 8192 * i for i, n in enumerate(names)}

    def call(**change):
        v = dict(good, **change)
        p = lambda n: C.c_void_p(v[n])                                                   # noqa: E731
        return hip_lib.md_multistep_step(p("x"), p("eps"), p("h1"), p("h2"), p("z"), p("mask"), p("coef"), p("partial"), p("pmask"), 0,
                                         p("x_out"), p("x0_out"), p("x_f32"), B, Cc, P, C.c_void_p(0))

    for out in ("x_out", "x0_out", "x_f32"):
        for inp in names[:9]:
            assert call(**{out: good[inp]}) == _lib.ERR_BAD_ARG, (out, inp)
    assert call(x_out=good["x0_out"]) == _lib.ERR_BAD_ARG and call(x_out=good["x_f32"]) == _lib.ERR_BAD_ARG
    assert call(x0_out=good["x_f32"]) == _lib.ERR_BAD_ARG
    assert call(x0_out=good["x_out"] + 2048) == _lib.ERR_BAD_ARG                          # one output starts inside another
    assert call(x_f32=good["x0_out"] + 4080) == _lib.ERR_BAD_ARG                          # ... in its last 16 bytes
    assert call(x_out=good["h1"] - 4080) == _lib.ERR_BAD_ARG                              # an output's tail reaches into an input
    assert call(x_f32=good["coef"] + 112) == _lib.ERR_BAD_ARG                             # the last 16 of the 128 coefficient bytes


# ---- the samplers' shared setup ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_prepare_run_never_hands_back_the_callers_x0(sde, masked):
    """prepare_run on CPU tensors: the start state is a copy of x0 (times the grid mask), with and without a grid mask, so the
    initial replacement -- and every in-place kernel after it -- leaves the caller's x0 as it was."""
    shape = (2, 4, 4, 4, 4)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(shape, generator=g)
    keep = x0.clone()
    gm = (torch.rand((1,) + shape[2:], generator=g) < 0.7).float() if masked else None
    partial, pmask = torch.randn(shape[2:], generator=g), (torch.rand(shape[2:], generator=g) < 0.5).float()
    dev = torch.device("cpu")
    for replace in (False, True):
        x, gm_dev, gm_flat, part, pm = sampling.prepare_run(sde, shape, dev, gm, x0, partial, pmask, ch=1, replace=replace)
        assert x.untyped_storage().data_ptr() != x0.untyped_storage().data_ptr() and x.is_contiguous()
        assert torch.equal(x0, keep)
        want = keep * gm if masked else keep.clone()
        if replace:
            want[:, 1] = want[:, 1] * (1 - pmask) + partial * pmask
        assert torch.equal(x, want)
        assert (gm_flat is None and gm_dev is None) if not masked else (gm_flat.shape == (64,) and gm_flat.dtype == torch.float32)
        assert part.shape == pm.shape == (64,) and torch.equal(part.view(4, 4, 4), partial) and torch.equal(pm.view(4, 4, 4), pmask)
        x.zero_()                                                                        # what an in-place kernel would do
        assert torch.equal(x0, keep)
    x, _, _, part, pm = sampling.prepare_run(sde, shape, dev, gm)                        # no x0: a prior draw; no partial
    assert x.shape == shape and part is None and pm is None
