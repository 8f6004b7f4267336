"""Latent interpolation without a GPU: the np.longdouble slerp restatement against the reference's own formula (recorded in
tests/golden/latent.npz), the conditioning of the seeded cases, the host logic of evaler.interp and the CLI, the level order and
coefficient rows of the DDIM encode loop, and ODE inversion on the float64 CPU path against the closed-form flow."""
import os
import sys

import numpy as np
import pytest
import torch

import guidance_cases as gc
import latent_cases as lc
from conftest import GOLD, ROOT, rel_l2


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_slerp_restatement_against_the_reference_formula():
    """slerp_ref (np.longdouble, the kernels' order of operations) against the reference's slerp in float64.  They differ in the
    summation order of at most 2^13 float64 terms (about 1e-12 relative), amplified by 1/sin(theta) <= 2.3: the bar is 1e-10 of
    the largest output.  Measured on a CPU: at most 4e-16."""
    gold = np.load(os.path.join(GOLD, "latent.npz"))
    assert np.array_equal(gold["alphas"], np.array(lc.GOLDEN_ALPHAS))
    assert np.array_equal(gold["pairs"], np.array(lc.GOLDEN_PAIRS, dtype=np.float64))
    for n, (seed, C, P, rho) in enumerate(lc.GOLDEN_PAIRS):
        a, b = lc.golden_pair(seed, C, P, rho)
        v, w1, w2, theta = lc.slerp_ref(a[None], b[None], None, lc.GOLDEN_ALPHAS)
        want = gold[f"out{n}"]
        assert want.dtype == np.float64 and want.shape == (len(lc.GOLDEN_ALPHAS), C, P)
        assert abs(float(np.cos(theta[0])) - float(gold[f"cos{n}"])) < 1e-12 and abs(float(gold[f"cos{n}"])) <= 0.9
        err = float(np.abs(v[0].astype(np.float64) - want).max() / np.abs(want).max())
        print(f"pair {n}: max |slerp_ref - reference| / max |reference| = {err:.3e}")
        assert err <= 1e-10


def test_slerp_restatement_edges():
    """Ends, parallel and antiparallel pairs, a zero endpoint."""
    a, b = lc.golden_pair(5, 2, 8, 0.2)
    a, b = a[None], b[None]
    v, w1, w2, _ = lc.slerp_ref(a, b, None, [0.0, 1.0])
    assert np.array_equal(v[0, 0].astype(np.float32), a[0]) and np.array_equal(v[0, 1].astype(np.float32), b[0])
    al = np.array([0.0, 0.25, 0.5, 1.0])
    for scale, theta_want in ((1.0, 0.0), (2.0, 0.0), (-1.0, np.pi)):
        v, w1, w2, theta = lc.slerp_ref(a, scale * a, None, al)
        assert np.array_equal(w1[0].astype(np.float64), 1 - al) and np.array_equal(w2[0].astype(np.float64), al)
        assert abs(float(theta[0]) - theta_want) < 1e-9
    assert float(np.abs(lc.slerp_ref(a, -a, None, [0.5])[0]).max()) == 0.0
    assert np.isnan(lc.slerp_ref(a, 0 * a, None, [0.5])[0].astype(np.float64)).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", lc.SLERP_CASES)
def test_slerp_cases_are_well_conditioned(case, masked):
    """|cos(theta)| <= 0.9 on every seeded pair (1/sin(theta) <= 2.3: what the GPU test's weight term assumes), pair p at its
    SLERP_RHO; the masks keep live and dead values."""
    a, b, mask, alphas = lc.slerp_inputs(case, masked)
    pairs, K, C, P = case
    assert a.shape == b.shape == (pairs, C, P) and a.dtype == b.dtype == np.float32 and alphas.shape == (K,)
    assert (mask is None) == (not masked)
    if masked and P > 4:
        assert 0 < mask.sum() < P and set(np.unique(mask)) == {0.0, 1.0}
    _, _, _, theta = lc.slerp_ref(a, b, mask, alphas)
    cos = np.cos(theta.astype(np.float64))
    print(f"{case} masked={masked}: cos(theta) = {cos}")
    assert np.all(np.abs(cos) <= 0.9)
    assert np.all(np.abs(cos - np.array(lc.SLERP_RHO[:pairs])) < 1e-6)


# ---- host logic of evaler.interp ------------------------------------------------------------------------------------------------
def _cfg(method="ddim", batch=6, **ev):
    from meshdiffusion_amd import synth
    cfg = synth.small_config()
    cfg.sampling.method = method
    cfg.eval.batch_size = batch
    for k, v in ev.items():
        setattr(cfg.eval, k, v)
    return cfg


def test_interp_field_defaults(monkeypatch):
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.lib.diffusion import evaler
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert _lib.SLERP_MAX_K == 256
    assert evaler.interp_plan(_cfg()) == (1, 6, "ddim", False)                               # one pair, K = batch_size
    assert evaler.interp_plan(_cfg(interp_pairs=2)) == (2, 3, "ddim", False)                 # K = batch_size // Np
    assert evaler.interp_plan(_cfg(interp_pairs=2, interp_points=5)) == (2, 5, "ddim", False)
    assert evaler.interp_plan(_cfg("ode", interp_sources="g.npy"), 4) == (2, 3, "ode", True)        # Np = rows / 2
    assert evaler.interp_plan(_cfg(interp_sources="g.npy", interp_pairs=1, interp_points=9), 4) == (1, 9, "ddim", True)
    assert evaler.interp_plan(_cfg(interp_pairs=3, interp_points=4), fields=False) == (1, 6, "ddim", False)   # uncond_gen_interp
    for bad in (dict(interp_points=1), dict(interp_points=257), dict(interp_pairs=0), dict(interp_pairs=4)):  # 6 // 4 = 1 point
        with pytest.raises(ValueError, match="interp_p"):
            evaler.interp_plan(_cfg(**bad))
    assert evaler.interp_plan(_cfg(interp_points=256))[1] == 256
    for rows in (None, 1, 3):
        with pytest.raises(ValueError, match="2\\*Np grids"):
            evaler.interp_plan(_cfg(interp_sources="g.npy"), rows)
    with pytest.raises(ValueError, match="holds 2 pairs"):
        evaler.interp_plan(_cfg(interp_sources="g.npy", interp_pairs=3), 4)


def test_interp_method_constraints(monkeypatch):
    from meshdiffusion_amd.lib.diffusion import evaler
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for method in ("ddim", "dpmpp", "ode"):
        assert evaler.interp_plan(_cfg(method))[2:] == (method, False)
    with pytest.raises(NotImplementedError, match="'ddim', 'dpmpp' with dpmpp_tau = 0, or 'ode', got 'pc'"):
        evaler.interp_plan(_cfg("pc"))
    cfg = _cfg("dpmpp")
    cfg.sampling.dpmpp_tau = 1
    with pytest.raises(NotImplementedError, match="dpmpp_tau = 0 only"):
        evaler.interp_plan(cfg)
    for method in ("dpmpp", "pc"):
        with pytest.raises(NotImplementedError, match="'ddim' \\(DDIM inversion\\) or 'ode' \\(ODE inversion\\)"):
            evaler.interp_plan(_cfg(method, interp_sources="g.npy"), 2)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="single process"):
        evaler.interp_plan(_cfg())


def test_cli_parses_the_interp_mode():
    sys.path.insert(0, ROOT)
    import main_diffusion
    cfg, mode = main_diffusion.parse(["--config=res64", "--mode=interp", "--config.sampling.method=ddim", "--config.eval.interp_points=3",
                                      "--config.eval.interp_sources=grids.npy"])
    assert mode == "interp" and cfg.eval.interp_points == 3 and cfg.eval.interp_sources == "grids.npy" and cfg.sampling.method == "ddim"
    with pytest.raises(SystemExit, match="train\\|uncond_gen\\|cond_gen\\|likelihood\\|interp"):
        main_diffusion.parse(["--config=res64", "--mode=interpolate"])


def test_return_traj_still_raises():
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    sde = sde_lib.VPSDE(0.1, 20.0, 50, device="cpu")
    with pytest.raises(NotImplementedError, match="return_traj"):
        sampling.get_pc_sampler(sde, (1, 4, 8, 8, 8), sampling.get_predictor("ancestral_sampling"), sampling.get_corrector("none"),
                                lambda v: v, 0.1, device="cpu", return_traj=True)


# ---- the encode loop's order and rows -------------------------------------------------------------------------------------------
def test_ddim_encode_loop_levels_and_rows(monkeypatch):
    """The loop on the CPU with md_ddim_step stood in for by its float64 torch chain, which also records what it is handed: a
    5-point schedule is walked upward 0 -> 10 -> 20 -> 30 -> 40, the network sees the CURRENT level's label and the float32 state,
    and each row is {a1, a2, a1_next/a1, a2_next/a2} of the SDE's tables.  The result is the recursion's."""
    from meshdiffusion_amd.lib.diffusion import sampling
    s = gc.loop_setup()
    sde, N, gm, shape = s["sde"], s["N"], s["gm"], s["shape"]
    B = shape[0]
    rows, labels, inputs = [], [], []

    def fake_step(x64, eps, mask, coef, partial=None, pmask=None, ch=0):
        assert x64.dtype == torch.float64 and eps.dtype == torch.float32 and partial is None and pmask is None
        rows.append(coef.clone())
        a1, a2, r1, r2 = (coef[:, j].view(-1, 1, 1, 1, 1) for j in range(4))
        x0s = x64 - a2 * eps.double()
        xn = (r1 * x64 + ((-r1) + r2) * (x64 - x0s)) * mask.view(x64.shape[2:]).double()
        return xn, x0s / a1, xn.float()

    class Spy(gc.GaussianEps):
        def forward(self, x, lab):
            labels.append(lab.clone())
            inputs.append(x.clone())
            return super().forward(x, lab)

    monkeypatch.setattr(sampling.ops, "ddim_step", fake_step)
    fn = sampling.get_ddim_sampler(sde, shape, sampling.get_predictor("ddim"), lambda v: v + 100.0, denoise=True, device="cpu",
                                   grid_mask=gm.float())
    data = torch.randn(shape, generator=torch.Generator().manual_seed(3)) * 0.5
    ts = sampling.ddim_schedule(N, "uniform", 5)
    assert [int(round(float(t) * N)) for t in ts] == [0, 10, 20, 30, 40]
    out, nfe = fn(Spy(s["s"], N), schedule="uniform", num_steps=5, x0=data, encode=True)
    assert nfe == 2 * N and out.dtype == torch.float64                                  # neither denoise nor the inverse scaler
    want_rows = lc.encode_rows(sde, ts)
    assert len(rows) == len(labels) == 4
    for i in range(4):
        assert torch.equal(labels[i], (torch.ones(B) * ts[i]).float() * (N - 1)), i      # the level the step starts from
        assert inputs[i].dtype == torch.float32
        assert torch.equal(rows[i], want_rows[i].expand(B, 4)), i
    sa, s1 = sde.sqrt_alphas_cumprod.double(), sde.sqrt_1m_alphas_cumprod.double()
    ks = [int(float(t) * (N - 1)) for t in ts]
    assert torch.equal(want_rows[:, 0], sa[ks[:-1]]) and torch.equal(want_rows[:, 3], s1[ks[1:]] / s1[ks[:-1]])
    assert float((out * (1 - gm)).abs().max()) == 0.0
    assert rel_l2(out, lc.ddim_encode_recursion(sde, s["s"], data, gm, ts)) < 1e-12
    first, _ = fn(Spy(s["s"], N), schedule="uniform", num_steps=5, x0=data, encode=True, n_iters=1)
    assert len(rows) == 5 and rel_l2(first, lc.ddim_encode_recursion(sde, s["s"], data, gm, ts, n_iters=1)) < 1e-12
    with pytest.raises(NotImplementedError, match="encode=True"):
        fn(Spy(s["s"], N), x0=data, encode=True, partial=s["y"].float(), partial_mask=s["pm"].float())
    with pytest.raises(ValueError, match="needs x0"):
        fn(Spy(s["s"], N), encode=True)


# ---- ODE inversion --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_data", [0.5, 2.0])
def test_ode_inversion_against_the_closed_form_flow(s_data):
    """ode_sampler(encode=True) on the float64 CPU path of get_ode_rhs, rtol = atol = 1e-8, for data ~ N(0, s^2 I): the flow scales
    a grid by sqrt((alpha_T^2 s^2 + sigma_T^2)/(alpha_eps^2 s^2 + sigma_eps^2)).  Bar rel-L2 1e-5: three orders above the local
    tolerance over the few dozen steps the solver takes, four below any mistake in span, sign or time (O(1)).  Measured on a CPU:
    4.8e-8 (s = 0.5) and 2.3e-8 (s = 2) in 110 evaluations, below 1e-6: the bar leaves two orders."""
    from meshdiffusion_amd.lib.diffusion import sampling
    s = gc.loop_setup()
    sde, N, gm, shape = s["sde"], s["N"], s["gm"], s["shape"]
    eps = 1e-3
    fn = sampling.get_ode_sampler(sde, shape, lambda v: v + 100.0, rtol=1e-8, atol=1e-8, eps=eps, device="cpu", grid_mask=gm)
    data = torch.randn(shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * s_data
    model = gc.GaussianEps(s_data, N)
    z, nfe = fn(model, x0=data, encode=True)
    want = data * gm * lc.gaussian_flow_factor(s_data, eps, float(sde.T))
    err = rel_l2(z, want)
    print(f"s = {s_data}: ODE inversion vs the closed-form flow {err:.3e}, nfe {nfe}")
    assert z.dtype == torch.float64 and nfe > 0 and float((z * (1 - gm)).abs().max()) == 0.0
    assert err <= 1e-5
    back, _ = fn(model, x0=z)                                                            # and the sampler brings it back
    assert rel_l2(back - 100.0, data * gm) <= 1e-5
    with pytest.raises(ValueError, match="needs x0"):
        fn(model, encode=True)
