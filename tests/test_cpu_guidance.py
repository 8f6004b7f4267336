"""Reconstruction guidance, host side (no GPU): the restated step d is zeta * grad ||r|| under float64 autograd; the float64
recursions of the guided loops (the GPU loop test's reference) meet that test's conditions; the three exports and the wrappers
refuse what they must before any launch."""
import numpy as np
import pytest
import torch

import guidance_cases as gc

FLOOR = 1e-6            # the floor of the GPU loop test's bar max(2u, 1e-6)


def _level(sde, i):
    return float(sde.sqrt_alphas_cumprod[i].double()), float(sde.sqrt_1m_alphas_cumprod[i].double())


@pytest.mark.parametrize("model", ["closed_form", "dense_linear"])
def test_restated_step_is_the_gradient_of_the_residual_norm(model):
    """d = zeta/(alpha n) (r - sigma J^T r) gm against zeta * d||r||/dx * gm from autograd, 1e-12 relative: the sign and the
    1/alpha.  Then the numpy restatements of the kernels (float32 roundings) against that d at float32 precision."""
    g = torch.Generator().manual_seed(4)
    B, C, P, ch, zeta = 3, 4, 32, 1, 0.7
    s = gc.loop_setup()
    sde = s["sde"]
    x = torch.randn((B, C, P), generator=g).double()                       # float32 values: the kernels' operand
    y = torch.sign(torch.randn(P, generator=g, dtype=torch.float64))
    pm = (torch.rand(P, generator=g) < 0.5).double()
    gm = (torch.rand(P, generator=g) < 0.7).double()
    assert float((pm * gm).sum()) > 0
    A = torch.randn((C * P, C * P), generator=g, dtype=torch.float64) / (C * P) ** 0.5
    # levels of the 50: low, middle and high noise.  Not the last few: there r - sigma J^T r of the closed form keeps
    # alpha^2 s^2 < 1e-4 of r, and the float64 rounding of either side alone, 2^-53 / 1e-4, is the 1e-12 being asked for
    for lvl in (1, 25, 40):
        alpha, sigma = _level(sde, lvl)
        if model == "closed_form":
            k = gc.gaussian_k(torch.full((B,), float(lvl)), 1.3, sde.N).view(B, 1, 1)
            eps_fn, jt = (lambda v: k * v), (lambda r: k * r)
        else:
            eps_fn = lambda v: (v.reshape(B, -1) @ A.T).view(B, C, P)                      # noqa: E731
            jt = lambda r: (r.reshape(B, -1) @ A).view(B, C, P)                             # noqa: E731
        xr = x.clone().requires_grad_(True)
        x0 = (xr - sigma * eps_fn(xr)) / alpha
        norm = ((pm * gm) * (x0[:, ch] - y)).flatten(1).norm(dim=1)
        grad, = torch.autograd.grad(norm.sum(), xr)
        want = zeta * grad * gm
        d, n = gc.guide_d_f64(x, eps_fn(x), jt, y, pm, gm, alpha, sigma, zeta, ch)
        rel = float((d - want).norm() / want.norm())
        print(f"{model} level {lvl}: |d - zeta grad||r|| | / |.| = {rel:.2e}")
        assert rel <= 1e-12 and torch.allclose(n, norm.detach(), rtol=1e-14)
        # the kernels' restatements, chained: float32 operands, the cotangent rounded once, d rounded once
        x32, e32 = x.float(), eps_fn(x).float()
        coef = np.array([[alpha, sigma, zeta]] * B)
        cot, r64, sumsq = gc.guide_residual_ref(x32.numpy(), e32.numpy(), y.float().numpy(), pm.numpy(), gm.numpy(), coef[:, :2], ch)
        assert np.all(cot[:, [c for c in range(C) if c != ch]] == 0) and np.all(cot[:, ch][:, (pm * gm).numpy() == 0] == 0)
        slabs = np.zeros((B, gc.SLABS))
        slabs[:, 0] = sumsq
        g32 = jt(torch.from_numpy(cot).double()).float().numpy()
        xn, xm = gc.guide_apply_f32_ref(x32.numpy(), x32.numpy(), cot, g32, gm.numpy(), coef, slabs)
        assert np.array_equal(xn, xm)
        got = x32.numpy().astype(np.float64) - xn
        rel32 = np.linalg.norm(got - want.numpy()) / np.linalg.norm(want.numpy())
        x64n, x64f = gc.guide_apply_f64_ref(x32.double().numpy(), cot, g32, gm.numpy(), coef, slabs)
        rel64 = np.linalg.norm((x32.double().numpy() - x64n) - want.numpy()) / np.linalg.norm(want.numpy())
        print(f"    kernel restatements against it: f32 {rel32:.2e}, f64 {rel64:.2e}")
        # eps_hat, the cotangent and g are rounded to float32 once each; r - sigma g keeps no less than alpha^2 of r (high noise)
        assert rel64 <= 8 * 2.0 ** -24 / (alpha * alpha) and np.array_equal(x64f, x64n.astype(np.float32))


def test_conditions_of_the_gpu_loop_test_on_the_float64_recursion():
    """On the inputs the GPU loop test uses: guidance moves the final state by far more than that test's bar, and with
    replacement off it lowers the RMS of pm (x[ch] - y) below the unguided run's.  A third condition, without which that bar would
    measure the inputs and not the code: the GPU loop evaluates the guidance term at the float32 copy of its float64 DDIM state,
    and the recursion must not amplify that one rounding to more than a tenth of the bar's floor.  The default 100-point quadratic
    schedule does (5.5e-6: its last dozen updates sit on level 0 with ||r|| below the step length zeta alpha^2, where the
    normalised step overshoots), so the loop tests run the DDIM sampler on 25 uniform points."""
    from meshdiffusion_amd.lib.diffusion import sampling
    s = gc.loop_setup()
    sde, N, ch, y, pm, gm = s["sde"], s["N"], s["ch"], s["y"], s["pm"], s["gm"]
    assert float(sde.discrete_betas.max()) < 1.0 and float(pm.sum()) >= 8
    torch.manual_seed(3)
    x_init = sde.prior_sampling(s["shape"]) * gm.float()
    noise = gc.loop_noise(s["shape"], 5, N)
    rms = lambda v: float(((pm * (v[:, ch] - y)) ** 2).sum().div(pm.sum() * s["B"]).sqrt())         # noqa: E731
    rel = lambda a, b: float((a - b).norm() / b.norm())                                              # noqa: E731

    def anc(zeta, replace):
        return gc.ancestral_recursion(sde, s["s"], x_init, y, pm, gm, ch, zeta, replace, iter(gc.noise_for(noise, replace, N)))[1]

    ts = sampling.ddim_schedule(N, *s["ddim"])
    x0 = torch.randn(s["shape"], generator=torch.Generator().manual_seed(9))
    ddim = lambda zeta, replace, **kw: gc.ddim_recursion(sde, s["s"], x0, y, pm, gm, ch, zeta, replace, ts, **kw)   # noqa: E731
    for replace in (True, False):
        amp = rel(ddim(s["zeta"], replace, round_input=True), ddim(s["zeta"], replace))
        quad = sampling.ddim_schedule(N)
        amp_q = rel(gc.ddim_recursion(sde, s["s"], x0, y, pm, gm, ch, s["zeta"], replace, quad, round_input=True),
                    gc.ddim_recursion(sde, s["s"], x0, y, pm, gm, ch, s["zeta"], replace, quad))
        print(f"ddim, replacement {'on' if replace else 'off'}: one float32 rounding of the guidance input moves the final state by "
              f"{amp:.2e} ({len(ts)} uniform points; {amp_q:.2e} on the 100-point quadratic schedule)")
        assert amp <= FLOOR / 10
    for name, run in (("ancestral", anc), ("ddim", ddim)):
        plain, guided, free, free_guided = run(0.0, True), run(s["zeta"], True), run(0.0, False), run(s["zeta"], False)
        for v in (plain, guided, free, free_guided):
            assert torch.isfinite(v).all() and float((v * (1 - gm)).abs().max()) == 0.0
        d_on, d_off = rel(guided, plain), rel(free_guided, free)
        print(f"{name}: guided vs unguided rel-L2 {d_on:.3e} (replacement on), {d_off:.3e} (off); RMS of pm (x[ch] - y) without "
              f"replacement: unguided {rms(free):.4f}, guided {rms(free_guided):.4f}")
        assert d_on >= 100 * FLOOR and d_off >= 100 * FLOOR
        assert rms(free_guided) < rms(free)


def test_exports_refuse_bad_arguments_in_order(hip_lib):
    """Null or misaligned pointers, batch <= 0, P % 4, ch outside [0, C), src_bstride not in {0, P}, an output that is an input:
    MD_ERR_BAD_ARG, before any launch (host addresses: nothing here may reach a kernel)."""
    import ctypes as C
    from meshdiffusion_amd import _lib
    buf = C.create_string_buffer(16 * 8192 + 64)
    at = lambda i: C.c_void_p(((C.addressof(buf) + 63) & ~63) + 8192 * i)       # noqa: E731   distinct 8 KiB regions
    x, e, src, pm, gm, coef, cot, slabs, g, xm = (at(i) for i in range(10))
    ptr = dict(x=x, e=e, src=src, pm=pm, gm=gm, coef=coef, cot=cot, slabs=slabs)
    nul, bad = C.c_void_p(0), _lib.ERR_BAD_ARG
    odd16, odd8 = (lambda p: C.c_void_p(p.value + 8)), (lambda p: C.c_void_p(p.value + 4))
    B, Cc, P = 2, 4, 64
    res = hip_lib.md_guide_residual

    def residual(**kw):
        a = dict(x=x, e=e, src=src, bstride=0, pm=pm, gm=gm, coef=coef, ch=0, cot=cot, slabs=slabs, B=B, C=Cc, P=P)
        a.update(kw)
        return res(a["x"], a["e"], a["src"], a["bstride"], a["pm"], a["gm"], a["coef"], a["ch"], a["cot"], a["slabs"], a["B"], a["C"],
                   a["P"], nul)

    for name in ("x", "e", "src", "pm", "coef", "cot", "slabs"):
        assert residual(**{name: nul}) == bad, name                              # null
    for name in ("x", "e", "src", "pm", "gm", "cot"):
        assert residual(**{name: odd16(ptr[name])}) == bad, name            # 8 mod 16
    for name in ("coef", "slabs"):
        assert residual(**{name: odd8(ptr[name])}) == bad, name             # 4 mod 8
    assert residual(B=0) == bad and residual(B=-1) == bad and residual(C=0) == bad and residual(P=0) == bad
    assert residual(P=66) == bad
    assert residual(ch=-1) == bad and residual(ch=Cc) == bad
    assert residual(bstride=4) == bad and residual(bstride=-P) == bad and residual(bstride=2 * P) == bad
    for name in ("x", "e", "src", "pm", "gm"):
        assert residual(cot=ptr[name]) == bad, name                         # the cotangent written over an input
    assert residual(slabs=coef) == bad
    assert residual(cot=C.c_void_p(x.value + 1024)) == bad                        # inside x's [B][C][P] floats
    assert residual(slabs=C.c_void_p(cot.value + 1024)) == bad                    # one output starts inside the other
    assert residual(slabs=C.c_void_p(x.value - 512)) == bad                       # the slabs' tail reaches into an input

    for fname, state_bytes in (("md_guide_apply_f32", 4), ("md_guide_apply_f64", 8)):
        fn = getattr(hip_lib, fname)

        def apply(**kw):
            a = dict(x=x, aux=xm, cot=cot, g=g, gm=gm, coef=coef, slabs=slabs, B=B, C=Cc, P=P)
            a.update(kw)
            return fn(a["x"], a["aux"], a["cot"], a["g"], a["gm"], a["coef"], a["slabs"], a["B"], a["C"], a["P"], nul)

        for name in ("x", "cot", "g", "coef", "slabs"):
            assert apply(**{name: nul}) == bad, (fname, name)
        if state_bytes == 8:
            assert apply(aux=nul) == bad                                         # the float64 state always has its float copy
        for name, val in (("x", x), ("aux", xm), ("cot", cot), ("g", g), ("gm", gm)):
            assert apply(**{name: odd16(val)}) == bad, (fname, name)
        assert apply(coef=odd8(coef)) == bad and apply(slabs=odd8(slabs)) == bad
        assert apply(B=0) == bad and apply(C=0) == bad and apply(P=0) == bad and apply(P=62) == bad
        for name, val in (("cot", cot), ("g", g), ("gm", gm)):
            assert apply(x=val) == bad and apply(aux=val) == bad, (fname, name)  # a state written over an input
        assert apply(aux=x) == bad                                               # the two outputs are one tensor
        assert apply(aux=C.c_void_p(x.value + 64)) == bad                        # one output starts inside the other
        assert apply(x=C.c_void_p(cot.value - 16 * state_bytes)) == bad          # the state's tail reaches into cot


def test_wrappers_refuse_before_any_gpu_call(hip_lib):
    from meshdiffusion_amd import _lib, hip_ops as ops
    from meshdiffusion_amd.lib.diffusion import sampling
    B, C, R = 2, 4, 4
    P = R ** 3
    x = torch.zeros((B, C, R, R, R))
    m, coef2, coef3, slabs = torch.ones(P), torch.ones((B, 2), dtype=torch.float64), torch.ones((B, 3), dtype=torch.float64), \
        torch.ones((B, 64), dtype=torch.float64)
    with pytest.raises(_lib.MeshDiffusionHipError, match="GPU"):
        ops.guide_residual(x, x.clone(), m, m, m, coef2, 0)
    with pytest.raises(_lib.MeshDiffusionHipError, match="GPU"):
        ops.guide_apply_(x, x.clone(), x.clone(), x.clone(), m, coef3, slabs)
    with pytest.raises(_lib.MeshDiffusionHipError, match="GPU"):
        ops.guide_apply64_(x.double(), x.clone(), x.clone(), x.clone(), m, coef3, slabs)

    s = gc.loop_setup()
    sde, shape = s["sde"], s["shape"]
    model = gc.GaussianEps(1.0, s["N"])
    part = torch.zeros((1, C) + shape[2:])
    P_ = sampling.get_predictor
    Cr = sampling.get_corrector

    def pc(pred, corr, **kw):
        return sampling.get_pc_sampler(sde, shape, P_(pred), Cr(corr), lambda v: v, 0.1, n_steps=1, device="cuda",
                                       grid_mask=s["gm"].float(), **kw)

    with pytest.raises(NotImplementedError, match="partial"):
        pc("ancestral_sampling", "none")(model, guidance_scale=1.0)
    with pytest.raises(NotImplementedError, match="corrector"):
        pc("ancestral_sampling", "langevin")(model, partial=part, partial_mask=part, guidance_scale=1.0)
    with pytest.raises(NotImplementedError, match="ancestral"):
        pc("reverse_diffusion", "none")(model, partial=part, partial_mask=part, guidance_scale=1.0)
    with pytest.raises(NotImplementedError, match="probability flow"):
        pc("reverse_diffusion", "none", probability_flow=True)(model, partial=part, partial_mask=part, guidance_scale=1.0)
    with pytest.raises(NotImplementedError, match="[Pp]robability flow"):
        pc("ancestral_sampling", "none", probability_flow=True)
    with pytest.raises(ValueError):
        pc("ancestral_sampling", "none")(model, partial=part, partial_mask=part, guidance_scale=-1.0)
    ddim = sampling.get_ddim_sampler(sde, shape, P_("ddim"), lambda v: v, device="cuda", grid_mask=s["gm"].float())
    with pytest.raises(NotImplementedError, match="partial"):
        ddim(model, guidance_scale=1.0)
    ode = sampling.get_ode_sampler(sde, shape, lambda v: v, device="cuda", grid_mask=s["gm"].float())
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        ode(model, guidance_scale=1.0)
