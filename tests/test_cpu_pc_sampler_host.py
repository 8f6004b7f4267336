"""Predictor-corrector sampler, host side (no GPU): registries, refused pairs, fixtures, C ABI 16."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD


def _cfg(pred, corr, pf=False, continuous=False, n_steps=1):
    from meshdiffusion_amd import synth
    cfg = synth.small_config()
    cfg.device = torch.device("cpu")
    cfg.sampling.predictor, cfg.sampling.corrector = pred, corr
    cfg.sampling.probability_flow, cfg.sampling.n_steps_each = pf, n_steps
    cfg.training.continuous = continuous
    return cfg


def test_registries_hold_the_reference_names():
    from meshdiffusion_amd.lib.diffusion import sampling
    for name in ("euler_maruyama", "reverse_diffusion", "ancestral_sampling", "none", "ddim"):
        assert sampling.get_predictor(name).__name__
    for name in ("langevin", "ald", "none"):
        assert sampling.get_corrector(name).__name__
    assert sampling.get_predictor("reverse_diffusion").kind == "reverse_diffusion"
    assert sampling.get_predictor("euler_maruyama").kind == "euler_maruyama"
    assert sampling.get_corrector("langevin").mode == "langevin" and sampling.get_corrector("ald").mode == "ald"


@pytest.mark.parametrize("pred,corr,pf,continuous,n_steps", [
    ("euler_maruyama", "none", True, False, 1),        # the reference indexes the float diffusion 0. of its ODE
    ("euler_maruyama", "langevin", True, False, 1),
    ("ancestral_sampling", "none", True, False, 1),    # asserted away by AncestralSamplingPredictor
    ("ancestral_sampling", "langevin", False, True, 1),  # continuous: models/utils.py asserts it away
    ("reverse_diffusion", "none", False, True, 1),
    ("ddim", "none", False, False, 1),                 # DDIMPredictor.update_fn needs tprev: method 'ddim' only
    ("ancestral_sampling", "langevin", False, False, 0),  # a corrector with no step returns an unbound x_mean
])
def test_unsupported_pairs_raise_before_gpu_work(pred, corr, pf, continuous, n_steps):
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    cfg = _cfg(pred, corr, pf, continuous, n_steps)
    R = cfg.data.image_size
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cpu")
    with pytest.raises(NotImplementedError):
        sampling.get_sampling_fn(cfg, sde, (2, 4, R, R, R), lambda x: x, 1e-3)


@pytest.mark.parametrize("pred,corr,pf", [
    ("ancestral_sampling", "langevin", False), ("reverse_diffusion", "langevin", False), ("reverse_diffusion", "none", True),
    ("euler_maruyama", "ald", False), ("none", "langevin", False), ("none", "none", False),
])
def test_supported_pairs_build_a_sampler_without_gpu(pred, corr, pf):
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    cfg = _cfg(pred, corr, pf)
    R = cfg.data.image_size
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cpu")
    assert callable(sampling.get_sampling_fn(cfg, sde, (2, 4, R, R, R), lambda x: x, 1e-3))


def test_pc_coefficient_tables_follow_the_reference_expressions():
    """The rows handed to md_sde_step / md_langevin_step are the reference's float32 expressions, row by row."""
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cpu")
    ts = torch.linspace(1.0, 1e-3, 1000)
    k = (ts * 999).long()
    p, c = sampling._pc_tables(sde, ts, 3, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, 0.16, True)
    assert p.shape == (1000, 3, 5) and c.shape == (1000, 3, 3)
    i = 17
    beta, alpha = sde.discrete_betas[k[i]], sde.alphas[k[i]]
    assert torch.equal(p[i, 2, 2], torch.sqrt(beta) ** 2)          # G^2 of the reference, not beta itself
    assert torch.equal(p[i, 1], torch.stack([sde.sqrt_1m_alphas_cumprod[k[i]], torch.sqrt(alpha), torch.sqrt(beta) ** 2,
                                             torch.tensor(0.5), torch.tensor(0.0)]))
    _, std = sde.marginal_prob(torch.zeros(1, 1, 1, 1, 1), ts[i:i + 1])
    assert torch.equal(c[i, 0, 2], ((0.16 * std) ** 2 * 2 * alpha)[0])
    p, _ = sampling._pc_tables(sde, ts, 2, sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, 0.075, False)
    beta_t = 0.1 + ts[i:i + 1] * (20.0 - 0.1)
    d = torch.sqrt(beta_t)
    want = torch.stack([sde.sqrt_1m_alphas_cumprod[k[i]], (-0.5 * beta_t)[0], (d ** 2)[0], torch.tensor(-1.0 / 1000),
                        (d * np.sqrt(1.0 / 1000))[0]])
    assert torch.equal(p[i, 0], want)


def test_pc_goldens_load_and_carry_their_seeds():
    g = np.load(os.path.join(GOLD, "sampler_pc_small.npz"))
    assert int(g["K"]) == 6 and int(g["B"]) == 2
    cases = [str(c) for c in g["cases"]]
    assert len(cases) == 7 and len({int(g[f"{c}/seed"]) for c in cases}) == 7
    for c in cases:
        live = g[f"{c}/live"]
        assert live.shape[:2] == (2, 4) and np.isfinite(live).all() and np.abs(live).max() > 0.1
    pairs = {(str(g[f"{c}/predictor"]), str(g[f"{c}/corrector"]), bool(g[f"{c}/probability_flow"])) for c in cases}
    assert {("ancestral_sampling", "langevin", False), ("reverse_diffusion", "langevin", False),
            ("reverse_diffusion", "none", True), ("euler_maruyama", "none", False), ("none", "ald", False)} <= pairs
    assert any(bool(g[f"{c}/conditional"]) for c in cases)
    r = np.load(os.path.join(GOLD, "sampler_pc_res64.npz"))
    assert int(r["K"]) == 3 and int(r["B"]) == 2 and int(r["seed"]) > 0
    assert r["live"].shape[:2] == (2, 4) and r["norms"].shape == (2,) and str(r["corrector"]) == "langevin"
    for name in ("sampler_pc_small.npz", "sampler_pc_res64.npz"):
        assert os.path.getsize(os.path.join(GOLD, name)) < 1 << 20


def test_header_lib_and_abi_16_agree():
    from meshdiffusion_amd import _lib
    assert _lib.LANGEVIN_SLABS == 64
    assert _lib.CORRECTOR_LANGEVIN == 0 and _lib.CORRECTOR_ALD == 1
    assert _lib.SDE_REVERSE_DIFFUSION == 0
    assert _lib.SDE_EULER_MARUYAMA == 1
    from meshdiffusion_amd import build
    assert "sde_steps.hip" in build.SOURCES


def test_new_entry_points_reject_bad_arguments(hip_lib):
    """Argument validation returns MD_ERR_BAD_ARG before any launch (no GPU needed)."""
    import ctypes as C
    nul, one = C.c_void_p(0), C.c_void_p(16)
    assert hip_lib.md_langevin_norms(one, one, 2, 4, 4096, nul, nul) == -1          # no slab workspace
    assert hip_lib.md_langevin_norms(one, one, 2, 4, 4098, one, nul) == -1          # P % 4
    assert hip_lib.md_langevin_step(one, one, one, nul, one, nul, 0.075, 0, one, one, one, 2, 4, 4096, nul) == -1  # langevin, no slabs
    assert hip_lib.md_langevin_step(one, one, one, nul, one, one, 0.075, 7, one, one, one, 2, 4, 4096, nul) == -1  # unknown mode
    assert hip_lib.md_sde_step(one, one, one, nul, one, 2, one, one, 2, 4, 4096, nul) == -1                       # unknown kind
    assert hip_lib.md_sde_step(one, one, one, nul, one, 0, one, one, 0, 4, 4096, nul) == -1                       # empty batch


# The exports that took their argument checks from md_args.h last.  Per export: the arguments in order -- a pointer as (name,
# required, alignment), a scalar as its name -- and whether the kernel moves four values at a time (P % 4 refused).
_PTR16 = lambda *names: [(n, True, 16) for n in names]                                   # noqa: E731
STEP_EXPORTS = {
    "md_ancestral_step": (_PTR16("x", "eps", "z") + [("mask", False, 16), ("coef", True, 4)] + _PTR16("x_out", "x_mean_out")
                          + ["batch", "C", "P"], True),
    "md_ddim_step": ([("x", True, 8), ("eps", True, 4), ("mask", False, 4), ("coef", True, 8), ("partial", False, 4),
                      ("pmask", False, 4), "ch", ("x_out", True, 8), ("x0_out", True, 8), ("x_f32", True, 4), "batch", "C", "P"], False),
    "md_inpaint_blend": ([("x", True, 4), ("src", True, 4), ("pmask", True, 4), ("gmask", False, 4), "batch", "C", "ch", "P",
                          "src_bstride"], False),
    "md_inpaint_renoise": ([("x", True, 4), ("x_mean", False, 4), ("z", True, 4), ("pmask", True, 4), ("gmask", False, 4),
                            ("coef", True, 4), "batch", "C", "ch", "P"], False),
    "md_langevin_norms": (_PTR16("eps", "z") + ["batch", "C", "P"] + _PTR16("slabs"), True),
    "md_langevin_step": (_PTR16("x", "eps", "z") + [("mask", False, 16), ("coef", True, 4), ("slabs", False, 16), "snr", "mode"]
                         + _PTR16("x_out", "x_mean_out") + [("step_out", True, 4), "batch", "C", "P"], True),
    "md_sde_step": (_PTR16("x", "eps", "z") + [("mask", False, 16), ("coef", True, 4), "kind"] + _PTR16("x_out", "x_mean_out")
                    + ["batch", "C", "P"], True),
}


@pytest.mark.parametrize("export", sorted(STEP_EXPORTS))
def test_step_exports_refuse_bad_arguments_in_order(hip_lib, export):
    """Null required pointers, a 16-byte operand at 8 mod 16, an element 2 bytes off, batch / C / P <= 0, P % 4 where the kernel
    is four-wide, ch outside [0, C): MD_ERR_BAD_ARG before any launch.  Host addresses: nothing here may reach a kernel, so
    what must be ACCEPTED -- a coefficient row 4 bytes into a 16-byte line, as coef[i] of a [N,B,3] table is; P % 4 != 0 in the
    scalar kernels -- is probed only where no GPU is visible: there the launch itself fails, with another code."""
    import ctypes as C
    from meshdiffusion_amd import _lib
    args, four_wide = STEP_EXPORTS[export]
    buf = C.create_string_buffer(8192 * len(args) + 64)
    base = (C.addressof(buf) + 63) & ~63
    scalars = dict(batch=2, C=4, P=64, ch=0, src_bstride=0, snr=0.075, mode=0, kind=0)
    good = {a[0]: base + 8192 * i for i, a in enumerate(args) if not isinstance(a, str)}   # distinct 8 KiB regions, 64-byte aligned
    bad, fn = _lib.ERR_BAD_ARG, getattr(hip_lib, export)

    def call(**change):
        v = dict(scalars, **good)
        v.update(change)
        return fn(*[v[a] if isinstance(a, str) else C.c_void_p(v[a[0]]) for a in args], C.c_void_p(0))

    for name, required, align in (a for a in args if not isinstance(a, str)):
        if required:
            assert call(**{name: 0}) == bad, (name, "null")
        if align == 16:
            assert call(**{name: good[name] + 8}) == bad, (name, "8 mod 16")
        assert call(**{name: good[name] + 2}) == bad, (name, "2 bytes into an element")
    for name in ("batch", "C", "P"):
        assert call(**{name: 0}) == bad and call(**{name: -1}) == bad, name
    if four_wide:
        assert call(P=66) == bad
    if "ch" in args:                                                                      # (md_ddim_step: with its partial, as here)
        assert call(ch=-1) == bad and call(ch=4) == bad
    if export == "md_ddim_step":
        assert call(partial=0) == bad and call(pmask=0) == bad                            # one without the other
    if export == "md_langevin_step":
        assert call(mode=7) == bad and call(slabs=0) == bad and call(slabs=0, mode=1, P=66) == bad
    if export == "md_sde_step":
        assert call(kind=2) == bad
    if not torch.cuda.is_available():
        probes = [dict(coef=good["coef"] + 4)] if "coef" in good and export != "md_ddim_step" else []
        probes += [dict(P=66), dict(P=1)] if not four_wide else []
        probes += [dict(slabs=0, mode=1)] if export == "md_langevin_step" else []         # ALD reads no slabs
        for change in probes:
            assert call(**change) not in (bad, _lib.OK), change
