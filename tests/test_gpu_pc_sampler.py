"""Predictor-corrector sampling on the GPU: the md_sde_step / md_langevin_norms / md_langevin_step kernels against the
reference's torch expressions (bit for bit), and the samplers against the unmodified reference's recorded outputs
(tests/golden/sampler_pc_*.npz, tools/gen_golden_pc.py).  K-step sampled grids: rel-L2 < 1e-3 (BASELINE north_star)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, rel_l2

pytestmark = pytest.mark.gpu

TOL_SAMPLE = 1e-3
B5 = (slice(None),) + (None,) * 4


@pytest.fixture(scope="module")
def env(hip_lib):
    assert torch.cuda.is_available()
    from meshdiffusion_amd import hip_ops, synth
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    return dict(synth=synth, mutils=mutils, ops=hip_ops, sampling=sampling, sde_lib=sde_lib)


# flat grids (C, P) next to the cubes: 1028 values end in a workgroup of one wave's first lane (1028 / 4 = 257 threads), and
# 4 * (32^3 + 4) = 131088 values are 16 past the 131072 that one trip of stream_blocks' 128 workgroups covers at B = 8
FLAT_ODD, FLAT_TWO_TRIPS = (1, 1028), (4, 32 ** 3 + 4)


def _inputs(B, R, seed, masked):
    """R: the edge of a cubic grid of 4 channels, or (C, P) for a flat grid [1, 1, P] of C channels."""
    g = torch.Generator().manual_seed(seed)
    Cc, grid = (4, (R, R, R)) if isinstance(R, int) else (R[0], (1, 1, R[1]))
    x, eps, z = (torch.randn((B, Cc) + grid, generator=g).cuda() for _ in range(3))
    mask = None
    if masked:
        from meshdiffusion_amd import synth
        mask = synth.synthetic_grid_mask(R).cuda() if isinstance(R, int) else (torch.rand(grid, generator=g) < 0.6).float().cuda()
        x = x * mask
    return x, eps, z, mask


def _rows(env, B, pred, corr, snr, pf, seed):
    """Per-sample coefficient rows from the sampler's own tables, a different time level for every sample."""
    sampling, sde_lib = env["sampling"], env["sde_lib"]
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    ts = torch.linspace(1.0, 1e-3, 1000, device="cuda")
    pc, cc = sampling._pc_tables(sde, ts, 1, pred, corr, snr, pf)
    idx = torch.randint(0, 999, (B,), generator=torch.Generator().manual_seed(seed)).cuda()
    # the rows start 4 bytes into their allocation, as a sampler's coef[i] may: the exports ask the coefficients for no more
    off4 = lambda t: None if t is None else torch.cat([t.new_zeros(1), t[idx, 0].reshape(-1)])[1:].view(B, -1)   # noqa: E731
    return off4(pc), off4(cc)


def _masked(t, mask):
    return t if mask is None else t * mask.view(1, 1, *mask.shape)


@pytest.mark.parametrize("dims", [1, 3, 8, pytest.param((1, FLAT_ODD), id="1x1x1028"), pytest.param((8, FLAT_TWO_TRIPS), id="8x4x32772")])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind,pf", [("reverse_diffusion", False), ("reverse_diffusion", True), ("euler_maruyama", False)])
def test_sde_step_bit_identical_to_reference_expression(env, dims, masked, kind, pf):
    """dims: B on the 16^3 grid, or (B, (C, P)) on a flat one."""
    sampling, ops = env["sampling"], env["ops"]
    pred = sampling.get_predictor(kind)
    B, R = (dims, 16) if isinstance(dims, int) else dims
    x, eps, z, mask = _inputs(B, R, seed=10 + B, masked=masked)
    coef, _ = _rows(env, B, pred, sampling.NoneCorrector, 0.075, pf, seed=B)
    with torch.no_grad():
        torch.cuda.set_sync_debug_mode("error")
        try:
            xo, xmo = ops.sde_step(x, eps, z, None if mask is None else mask.reshape(-1).float().contiguous(), coef, kind)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        c = [coef[:, j][B5] for j in range(5)]
        score = -eps / c[0]                                           # models/utils.py:191-198
        if kind == "reverse_diffusion":                               # sde_lib.py:106-111 + VPSDE.discretize, sampling.py:204-209
            f = c[1] * x - x
            rev_f = f - c[2] * score * (0.5 if pf else 1.0)
            x_mean = x - rev_f
            xn = x_mean + c[4] * z
        else:                                                         # sampling.py:190-196 with VPSDE.sde
            drift = c[1] * x - c[2] * score * 1.0
            x_mean = x + drift * (-1.0 / 1000)
            xn = x_mean + c[4] * z
        xn, x_mean = _masked(xn, mask), _masked(x_mean, mask)
    assert torch.equal(xo, xn) and torch.equal(xmo, x_mean)
    if pf:
        assert torch.equal(xo, xmo)
    if masked:
        assert float(_masked(xo, 1 - mask).abs().max()) == 0.0


def _langevin_expr(x, eps, z, sigma, step, mask):
    """sampling.py:280-286 (and :315-316) with the kernel's own step size, then the mask of :450."""
    score = -eps / sigma[B5]
    x_mean = x + step[B5] * score
    xn = x_mean + torch.sqrt(step * 2)[B5] * z
    return _masked(xn, mask), _masked(x_mean, mask)


@pytest.mark.parametrize("B,R,masked", [(1, 16, False), (3, 16, True), (8, 16, True), (8, 64, True),
                                        pytest.param(1, FLAT_ODD, True, id="1-1x1028-True"),
                                        pytest.param(8, FLAT_TWO_TRIPS, False, id="8-4x32772-False")])
@pytest.mark.parametrize("mode", ["langevin", "ald"])
def test_langevin_step_vs_reference_and_deterministic(env, B, R, masked, mode):
    sampling, ops = env["sampling"], env["ops"]
    snr = 0.16
    salt = R if isinstance(R, int) else R[1]
    x, eps, z, mask = _inputs(B, R, seed=20 + B + salt, masked=masked)
    eps = eps * torch.linspace(0.5, 2.0, B, device="cuda")[B5]       # samples of different norm: the mean is not trivial
    _, coef = _rows(env, B, sampling.AncestralSamplingPredictor, sampling.get_corrector(mode), snr, False, seed=B + salt)
    gm = None if mask is None else mask.reshape(-1).float().contiguous()
    with torch.no_grad():
        torch.cuda.set_sync_debug_mode("error")
        try:
            xo, xmo, step = ops.langevin_step(x, eps, z, gm, coef, snr, mode)
            xo2, xmo2, step2 = ops.langevin_step(x, eps, z, gm, coef, snr, mode)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        sigma, alpha = coef[:, 0], coef[:, 1]
        if mode == "langevin":
            gn = (eps.double().reshape(B, -1).norm(dim=1) / sigma.double()).mean()
            nn_ = z.double().reshape(B, -1).norm(dim=1).mean()
            want = (snr * nn_ / gn) ** 2 * 2 * alpha.double()
            err = float(((step.double() - want).abs() / want).max())
            print(f"Langevin step size vs fp64 restatement (B={B}, grid {R}): max rel {err:.2e}")
            assert err <= 1e-6
        else:
            assert torch.equal(step, coef[:, 2])
        xn, xm = _langevin_expr(x, eps, z, sigma, step, mask)
    assert torch.equal(xo, xn) and torch.equal(xmo, xm)
    assert torch.equal(xo, xo2) and torch.equal(xmo, xmo2) and torch.equal(step, step2)


def _small_model(env):
    synth, mutils = env["synth"], env["mutils"]
    cfg = synth.small_config(); cfg.device = torch.device("cuda")
    model = mutils.create_model(cfg)
    R = cfg.data.image_size
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    return cfg, model.eval()


def _cpu_noise(x):      # replay the reference's CPU generator stream on the host, ship to the GPU
    return torch.randn(x.shape).to(x.device)


def test_pc_samplers_small_vs_reference_golden(env):
    sampling, sde_lib, synth = env["sampling"], env["sde_lib"], env["synth"]
    cfg, model = _small_model(env)
    gold = np.load(os.path.join(GOLD, "sampler_pc_small.npz"))
    R, K, B = cfg.data.image_size, int(gold["K"]), int(gold["B"])
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cuda")
    mask = synth.synthetic_grid_mask(R)
    li = torch.nonzero(mask.reshape(-1) > 0).reshape(-1)
    errs = {}
    for name in (str(c) for c in gold["cases"]):
        cfg.sampling.predictor, cfg.sampling.corrector = str(gold[f"{name}/predictor"]), str(gold[f"{name}/corrector"])
        cfg.sampling.snr, cfg.sampling.n_steps_each = float(gold[f"{name}/snr"]), int(gold[f"{name}/n_steps_each"])
        cfg.sampling.probability_flow = bool(gold[f"{name}/probability_flow"])
        torch.manual_seed(int(gold[f"{name}/seed"]))
        if bool(gold[f"{name}/conditional"]):
            g = torch.Generator().manual_seed(int(gold["cond_data_seed"]))
            partial = torch.sign(torch.randn((1, 1, R, R, R), generator=g))
            pmask = (torch.rand((1, 1, R, R, R), generator=g) < 0.5).float() * mask.view(1, 1, R, R, R)
            fn = sampling.get_sampling_fn(cfg, sde, (B, 4, R, R, R), lambda x: x, 1e-3, grid_mask=mask.view(1, 1, R, R, R).cuda())
            out, nfe = fn(model, partial=partial.cuda(), partial_mask=pmask.cuda(), freeze_iters=int(gold["freeze_iters"]),
                          n_iters=K, noise_fn=_cpu_noise)
        else:
            fn = sampling.get_sampling_fn(cfg, sde, (B, 4, R, R, R), lambda x: x, 1e-3, grid_mask=mask.view(1, R, R, R).cuda())
            out, nfe = fn(model, n_iters=K, noise_fn=_cpu_noise)
        out = out.cpu()
        assert nfe == sde.N * (cfg.sampling.n_steps_each + 1)
        assert float((out * (1 - mask)).abs().max()) == 0.0                      # masked cells exactly zero
        errs[name] = rel_l2(out.reshape(B, 4, -1)[:, :, li], gold[f"{name}/live"])
        print(f"{K}-iteration PC sampler {name} vs reference: {errs[name]:.3e}")
    assert max(errs.values()) < TOL_SAMPLE, errs


def test_pc_sampler_res64_b2_vs_reference_golden(env):
    """res64, B = 2, first 3 iterations of (ancestral_sampling, langevin): the batch mean couples two real samples."""
    from meshdiffusion_amd.config import get_config_res64
    from oracle.gen_golden import sample_stats
    sampling, sde_lib, synth, mutils = env["sampling"], env["sde_lib"], env["synth"], env["mutils"]
    gold = np.load(os.path.join(GOLD, "sampler_pc_res64.npz"))
    cfg = get_config_res64(); cfg.device = torch.device("cuda")
    cfg.sampling.predictor, cfg.sampling.corrector = str(gold["predictor"]), str(gold["corrector"])
    cfg.sampling.snr, cfg.sampling.n_steps_each = float(gold["snr"]), int(gold["n_steps_each"])
    model = mutils.create_model(cfg)
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(64))
    model.module.load_state_dict(sd, strict=True)
    del sd
    model.eval()
    B = int(gold["B"])
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cuda")
    mask = synth.synthetic_grid_mask(64)
    fn = sampling.get_sampling_fn(cfg, sde, (B, 4, 64, 64, 64), lambda x: x, 1e-3, grid_mask=mask.view(1, 64, 64, 64).cuda())
    torch.manual_seed(int(gold["seed"]))
    out, nfe = fn(model, n_iters=int(gold["K"]), noise_fn=_cpu_noise)
    out = out.cpu()
    assert nfe == 2000
    mine = sample_stats(out, mask, int(gold["stride"]))
    assert float(np.abs(gold["live"]).max()) > 0.1
    e_live = rel_l2(mine["live"], gold["live"])
    e_row = rel_l2(out[1, :, 33, 17, :], gold["xm_row"])
    e_norm = abs(float(out.double().norm()) - float(gold["xm_norm"])) / float(gold["xm_norm"])
    e_sum = float((np.abs(mine["sums"] - gold["sums"]) / mine["l1"]).max())
    print(f"res64 B=2 (ancestral_sampling, langevin) {int(gold['K'])} iterations vs reference: live cells {e_live:.3e} "
          f"row {e_row:.3e} norm {e_norm:.3e} sums {e_sum:.3e}")
    assert e_live < TOL_SAMPLE and e_row < TOL_SAMPLE and e_norm < TOL_SAMPLE and e_sum < TOL_SAMPLE
    assert float((out * (1 - mask)).abs().max()) == 0.0


def test_cli_uncond_and_cond_gen_with_langevin_corrector(hip_lib, tmp_path, monkeypatch):
    """`main_diffusion.py --config.sampling.corrector=langevin` end to end (40-level schedule, small U-Net)."""
    sys.path.insert(0, ROOT)
    import main_diffusion
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import losses
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    from meshdiffusion_amd.lib.diffusion.models.ema import ExponentialMovingAverage
    from meshdiffusion_amd.lib.diffusion.utils import save_checkpoint
    cfg = synth.small_config(); cfg.device = torch.device("cuda")
    cfg.model.num_scales = 40
    R = cfg.data.image_size
    model = mutils.create_model(cfg)
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    ema = ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    ck = tmp_path / "ckpt" / "checkpoint.pth"
    os.makedirs(ck.parent)
    save_checkpoint(str(ck), dict(optimizer=losses.get_optimizer(cfg, model.parameters()), model=model, ema=ema, step=7))
    os.makedirs(tmp_path / "data")
    torch.save(synth.synthetic_grid_mask(R), tmp_path / "data" / f"grid_mask_{R}.pt")
    cdir = tmp_path / "configs"; cdir.mkdir()
    (cdir / "small.py").write_text(
        "from meshdiffusion_amd import synth\n\ndef get_config():\n    c = synth.small_config()\n"
        "    c.model.num_scales = 40\n    return c\n")
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "out"
    m = synth.synthetic_grid_mask(R).numpy()
    common = ["--config", str(cdir / "small.py"), f"--config.eval.eval_dir={out}", f"--config.eval.ckpt_path={ck}",
              "--config.eval.batch_size=2"]
    torch.manual_seed(0)
    main_diffusion.main(common + ["--mode=uncond_gen", "--config.sampling.corrector=langevin"])
    x = np.load(out / "0.npy")
    assert x.shape == (2, 4, R, R, R) and x.dtype == np.float32 and np.isfinite(x).all()
    assert np.abs(x * (1 - m)).max() == 0.0 and np.abs(x).max() > 0

    idx = np.argwhere(m > 0).astype(np.float32)
    verts = (idx / (R - 1) - 0.5).astype(np.float32)
    tet_path = tmp_path / "tets.npz"
    np.savez(tet_path, vertices=verts, indices=np.zeros((1, 4), np.int32))
    g = torch.Generator().manual_seed(1)
    part = {"sdf": torch.sign(torch.randn(len(verts), generator=g)), "vis": torch.rand(len(verts), generator=g) < 0.5}
    ppath = tmp_path / "dmtet.pt"
    torch.save(part, ppath)
    main_diffusion.main(common + ["--mode=cond_gen", "--config.sampling.predictor=reverse_diffusion",
                                  "--config.sampling.corrector=langevin", f"--config.eval.partial_dmtet_path={ppath}",
                                  f"--config.eval.tet_path={tet_path}", "--config.eval.freeze_iters=30"])
    xc = np.load(out / "0.npy")
    assert xc.shape == (2, 4, R, R, R) and np.isfinite(xc).all() and np.abs(xc * (1 - m)).max() == 0.0
    assert np.abs(xc).max() > 0
