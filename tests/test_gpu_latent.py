"""Latent interpolation on the GPU: md_slerp_dots + md_slerp_mix against the np.longdouble restatement of latent_cases, their
edges (ends, parallel pairs, NaN, refused arguments); DDIM inversion against the float64 recursion of a closed-form model and, for
the small U-Net, against the oracle's forward; evaler.interp with the closed-form model; the CLI."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import guidance_cases as gc
import latent_cases as lc
from conftest import ROOT, rel_l2

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _slerp(a, b, alphas, mask):
    from meshdiffusion_amd import hip_ops as ops
    out, theta = ops.slerp(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(np.asarray(alphas, np.float64)),
                           None if mask is None else torch.from_numpy(mask).cuda())
    return out.cpu().numpy(), theta.cpu().numpy()


# ---- md_slerp_dots + md_slerp_mix --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", lc.SLERP_CASES)
def test_slerp_kernels(hip_lib, case, masked):
    """Per element |out - v| <= spacing(float32(v))/2 + 1e-10 (|w1 a| + |w2 b|): the single rounding to float32, and the weights
    (slab order: 2e-16 in a CPU emulation; the device's double sin / acos: a few ulp; 1e-10 leaves six orders).  theta within 1e-12,
    zero outside the mask, the alpha = 0 and alpha = 1 rows bit-equal to the masked endpoints, two runs bit-equal."""
    pairs, K, Cc, P = case
    a, b, mask, alphas = lc.slerp_inputs(case, masked)
    out, theta = _slerp(a, b, alphas, mask)
    assert out.shape == (pairs, K, Cc, P) and out.dtype == np.float32 and theta.shape == (pairs,) and theta.dtype == np.float64
    v, w1, w2, theta_ref = lc.slerp_ref(a, b, mask, alphas)
    err = np.abs(out.astype(np.longdouble) - v).astype(np.float64)
    bound = lc.slerp_bound(a, b, mask, v, w1, w2)
    live = np.ones(P, bool) if mask is None else mask > 0
    worst = float((err[..., live] / bound[..., live]).max())
    dth = float(np.abs(theta - theta_ref.astype(np.float64)).max())
    print(f"{case} masked={masked}: worst |out - v| / bar = {worst:.3f}, |theta - ref| = {dth:.2e}")
    assert np.all(err <= bound)
    assert dth <= 1e-12
    if masked:
        assert np.all(out[..., ~live] == 0.0)
    m = np.float32(1.0) if mask is None else mask
    for k, end in ((0, a), (K - 1, b)):
        if alphas[k] in (0.0, 1.0):
            assert np.array_equal(_bits(out[:, k][..., live]), _bits((end * m)[..., live])), f"alpha = {alphas[k]}"
    out2, theta2 = _slerp(a, b, alphas, mask)
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(theta.view(np.int64), theta2.view(np.int64))


def test_slerp_parallel_and_antiparallel_pairs(hip_lib):
    """b = a and b = 2a: the rows are float((1-alpha) a + alpha b) formed in double, bit for bit, theta = 0.  b = -a: theta = pi and
    the alpha = 1/2 row is all zero.  A zero endpoint: NaN, as in the reference."""
    a, _, mask, _ = lc.slerp_inputs((1, 5, 4, 512), True)
    al = np.array([0.0, 0.25, 0.5, 0.8, 1.0])
    live = mask > 0
    a64 = a.astype(np.float64)
    for scale, theta_want in ((1.0, 0.0), (2.0, 0.0), (-1.0, np.pi)):
        b = (scale * a).astype(np.float32)
        out, theta = _slerp(a, b, al, mask)
        want = (((1.0 - al)[None, :, None, None] * a64[:, None] + al[None, :, None, None] * b.astype(np.float64)[:, None]) * mask).astype(np.float32)
        assert np.array_equal(_bits(out[..., live]), _bits(want[..., live])), scale
        assert np.all(out[..., ~live] == 0.0)
        assert abs(float(theta[0]) - theta_want) <= 1e-7, (scale, theta)     # acos near +-1: c is 1 to an ulp, theta to its root
        if scale < 0:
            assert float(np.abs(out[:, 2]).max()) == 0.0
    out, theta = _slerp(a, np.zeros_like(a), al, mask)
    assert np.isnan(out[..., live]).all() and np.isnan(theta).all()


def test_slerp_nan_stays_in_its_pair(hip_lib):
    """One NaN in `a` of pair 0 makes theta and every output of pair 0 NaN inside the mask; pair 1 keeps the bits of a clean run."""
    case = (2, 3, 4, 1728)
    a, b, mask, alphas = lc.slerp_inputs(case, True)
    clean, theta_clean = _slerp(a, b, alphas, mask)
    live = mask > 0
    bad = a.copy()
    bad[0, 2, int(np.flatnonzero(live)[17])] = np.nan
    out, theta = _slerp(bad, b, alphas, mask)
    assert np.isnan(theta[0]) and np.isnan(out[0][..., live]).all()
    assert theta[1] == theta_clean[1] and np.array_equal(_bits(out[1]), _bits(clean[1]))


def test_slerp_refused_arguments(hip_lib):
    """Every refused argument gives MD_ERR_BAD_ARG from the host checks of both exports: nothing is launched, the outputs keep
    their bytes."""
    from meshdiffusion_amd import _lib
    pairs, K, Cc, P = 2, 3, 4, 64
    g = torch.Generator().manual_seed(1)
    dev = "cuda"
    t = dict(a=torch.randn((pairs, Cc, P), generator=g).to(dev), b=torch.randn((pairs, Cc, P), generator=g).to(dev),
             mask=torch.ones(P, device=dev), alpha=torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64, device=dev),
             slabs=torch.full((pairs, _lib.LANGEVIN_SLABS, 4), 7.0, dtype=torch.float64, device=dev),
             out=torch.full((pairs, K, Cc, P), 7.0, device=dev), theta=torch.full((pairs,), 7.0, dtype=torch.float64, device=dev))
    base = dict(t, K=K, pairs=pairs, C=Cc, P=P)
    ints = ("K", "pairs", "C", "P")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                     # noqa: E731

    def go(fn, order, change):
        v = dict(base, **change)
        args = [v[k] if k in ints else C.c_void_p(v[k].data_ptr() if torch.is_tensor(v[k]) else v[k]) for k in order]
        return fn(*args, stream())

    dots = lambda **ch: go(hip_lib.md_slerp_dots, ["a", "b", "mask", "pairs", "C", "P", "slabs"], ch)                    # noqa: E731
    mix = lambda **ch: go(hip_lib.md_slerp_mix, ["a", "b", "mask", "slabs", "alpha", "K", "out", "theta", "pairs", "C", "P"], ch)   # noqa: E731
    addr = lambda name, off=0: base[name].data_ptr() + off                                   # noqa: E731
    bad_mix = [dict(K=0), dict(K=-1), dict(K=_lib.SLERP_MAX_K + 1), dict(P=6), dict(P=0), dict(pairs=0), dict(C=0),
               dict(a=None), dict(b=None), dict(out=None), dict(slabs=None), dict(alpha=None),
               dict(a=addr("a", 8)), dict(b=addr("b", 4)), dict(out=addr("out", 8)), dict(mask=addr("mask", 8)),
               dict(slabs=addr("slabs", 4)), dict(alpha=addr("alpha", 4)), dict(theta=addr("theta", 4)),
               dict(out=addr("a")), dict(out=addr("b")), dict(out=addr("mask")), dict(out=addr("slabs")), dict(out=addr("alpha")),
               dict(theta=addr("a")), dict(theta=addr("out")),
               dict(a=addr("out", 4 * Cc * P * (pairs * K - pairs)))]                        # only the tail of out overlaps a
    for change in bad_mix:
        assert mix(**change) == _lib.ERR_BAD_ARG, change
    bad_dots = [dict(P=6), dict(P=0), dict(pairs=0), dict(C=0), dict(a=None), dict(b=None), dict(slabs=None),
                dict(a=addr("a", 8)), dict(b=addr("b", 4)), dict(mask=addr("mask", 4)), dict(slabs=addr("slabs", 4)),
                dict(slabs=addr("a")), dict(slabs=addr("b")), dict(slabs=addr("mask"))]
    for change in bad_dots:
        assert dots(**change) == _lib.ERR_BAD_ARG, change
    torch.cuda.synchronize()
    assert all(bool((t[k] == 7.0).all()) for k in ("slabs", "out", "theta"))
    assert dots() == _lib.OK and mix() == _lib.OK and mix(mask=None, theta=None, K=1) == _lib.OK
    assert mix(slabs=addr("slabs", 8), pairs=1) == _lib.OK                                   # doubles: 8-byte alignment suffices
    torch.cuda.synchronize()
    assert not bool((t["out"] == 7.0).any()) and not bool((t["theta"] == 7.0).any())


# ---- DDIM inversion, closed form -----------------------------------------------------------------------------------------------
def test_ddim_encode_against_the_closed_form(hip_lib):
    """ddim_sampler(GaussianEps, x0=data, encode=True) on the 25 uniform points of guidance_cases.loop_setup against the float64
    recursion: rel-L2 <= 2e-6 (what can separate them is a float32 rounding flip of eps_hat, <= 2^-24 per element and step over 24
    steps = 1.4e-6 if every element flipped every time; the loop itself moves the grid by 6 %, |z| / |x| = 0.936, and
    test_cpu_latent pins its levels and rows exactly).  decode(encode(data)) against
    ddim_recursion of the recursion's latent: 4e-6, two loops.  No closeness to the identity is asked: DDIM inversion is first
    order."""
    from meshdiffusion_amd.lib.diffusion import sampling
    s = gc.loop_setup()
    sde, N, gm, shape = s["sde"], s["N"], s["gm"], s["shape"]
    model = gc.GaussianEps(s["s"], N)
    fn = sampling.get_ddim_sampler(sde, shape, sampling.get_predictor("ddim"), lambda v: v, denoise=False, device="cuda",
                                   grid_mask=gm.float())
    schedule, num_steps = s["ddim"]
    ts = sampling.ddim_schedule(N, schedule, num_steps)
    data = torch.randn(shape, generator=torch.Generator().manual_seed(12))
    kw = dict(schedule=schedule, num_steps=num_steps)
    z, nfe = fn(model, x0=data, encode=True, **kw)
    assert z.dtype == torch.float64 and z.is_cuda and nfe == 2 * N
    z_ref = lc.ddim_encode_recursion(sde, s["s"], data, gm, ts)
    e_enc = rel_l2(z.cpu(), z_ref)
    back = fn(model, x0=z, **kw)[0].cpu()
    back_ref = gc.ddim_recursion(sde, s["s"], z_ref, None, None, gm, 0, 0.0, False, ts)
    e_rt = rel_l2(back, back_ref)
    print(f"DDIM encode vs recursion {e_enc:.3e}; decode(encode) vs recursion {e_rt:.3e}; "
          f"decode(encode(x)) vs x {rel_l2(back, data.double() * gm):.3e}; |z| / |x| {float(z.norm() / (data.double() * gm).norm()):.3f}")
    assert float((z.cpu() * (1 - gm)).abs().max()) == 0.0
    assert e_enc <= 2e-6
    assert e_rt <= 4e-6
    first = fn(model, x0=data, encode=True, n_iters=3, **kw)[0].cpu()
    assert rel_l2(first, lc.ddim_encode_recursion(sde, s["s"], data, gm, ts, n_iters=3)) <= 2e-6
    with pytest.raises(NotImplementedError, match="encode=True"):
        fn(model, x0=data, encode=True, partial=s["y"].float(), partial_mask=s["pm"].float(), **kw)
    with pytest.raises(NotImplementedError, match="encode=True"):
        fn(model, x0=data, encode=True, guidance_scale=1.0, **kw)


# ---- DDIM inversion, small U-Net -----------------------------------------------------------------------------------------------
def test_ddim_encode_small_unet_against_the_oracle(hip_lib):
    """The first 8 upward steps of the quadratic schedule on the small sensitised U-Net against the same loop around the oracle's
    forward on the CPU: rel-L2 < 1e-3, the project's parity bar for sampler states (test_gpu_ddim); zero outside the mask."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from oracle import unet_oracle as uo
    from test_gpu_ddim import _small
    cfg, model, sd = _small("ddim", False)
    R = cfg.data.image_size
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, R, R, R)
    fn = sampling.get_sampling_fn(cfg, sde, (2, 4, R, R, R), lambda v: v, 1e-3, grid_mask=mask.cuda())
    data = synth.synthetic_inputs(2, 4, R, seed=31) * 0.5
    z, _ = fn(model, x0=data.cuda(), encode=True, n_iters=8)
    with torch.no_grad():
        ref = lc.ddim_encode_oracle(lambda xx, lb: uo.unet_res64_forward(sd, synth.oracle_cfg(cfg), xx, lb), data, mask,
                                    cfg.model.num_scales, n_iters=8)
    e, moved = rel_l2(z.cpu(), ref), rel_l2(ref, data.double() * mask)
    print(f"DDIM encode (8 upward steps, small U-Net) vs the oracle loop: {e:.3e}; the 8 steps move the grid by {moved:.3e}")
    assert z.dtype == torch.float64 and float((z.cpu() * (1 - mask)).abs().max()) == 0.0
    assert e < 1e-3


# ---- evaler.interp with the closed-form model ---------------------------------------------------------------------------------------
def _closed_form_evaler(monkeypatch, tmp_path, method="ddim"):
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import evaler
    s = gc.loop_setup()
    cfg = synth.small_config(image_size=s["R"])
    cfg.device = torch.device("cuda")
    cfg.model.num_scales = s["N"]
    cfg.sampling.method, cfg.sampling.noise_removal = method, False
    cfg.eval.eval_dir = str(tmp_path / "out")
    monkeypatch.setattr(evaler, "_load_model", lambda config: (gc.GaussianEps(s["s"], s["N"]), s["sde"]))
    monkeypatch.setattr(evaler, "_grid_mask", lambda config, shape: s["gm"].float().view(*shape).cuda())
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return s, cfg, evaler


def test_interp_driver_against_the_closed_form(hip_lib, tmp_path, monkeypatch):
    """evaler.interp with GaussianEps standing in for the checkpoint, K = 4, noise endpoints: the decoded rows equal ddim_recursion
    of slerp_ref's rows within 4e-6 (the decode loop's 2e-6 twice over; the slerp itself is one rounding, 6e-8), and rows 0 and K-1
    equal the plain decode of the two endpoints."""
    from meshdiffusion_amd.lib.diffusion import sampling
    s, cfg, evaler = _closed_form_evaler(monkeypatch, tmp_path)
    sde, N, gm, R, Cc = s["sde"], s["N"], s["gm"], s["R"], s["C"]
    K = 4
    cfg.eval.interp_points = K
    torch.manual_seed(5)
    got = evaler.interp(cfg)
    torch.manual_seed(5)
    ends = torch.randn(2, Cc, R, R, R)
    assert got.shape == (K, Cc, R, R, R) and got.dtype == torch.float32
    saved = np.load(tmp_path / "out" / "interp.npy")
    assert saved.dtype == np.float32 and np.array_equal(saved, got.numpy())
    meta = np.load(tmp_path / "out" / "interp_meta.npz")
    alpha = np.arange(K) / (K - 1.0)
    mflat = gm.reshape(-1).numpy()
    v, _, _, theta = lc.slerp_ref(ends[0:1].reshape(1, Cc, -1).numpy(), ends[1:2].reshape(1, Cc, -1).numpy(), mflat, alpha)
    assert np.array_equal(meta["alpha"], alpha) and abs(float(meta["theta"][0]) - float(theta[0])) <= 1e-12
    assert str(meta["method"]) == "ddim" and not bool(meta["encoded"])
    ts = sampling.ddim_schedule(N)
    rows = torch.from_numpy(v[0].astype(np.float64)).view(K, Cc, R, R, R)
    want = gc.ddim_recursion(sde, s["s"], rows, None, None, gm, 0, 0.0, False, ts)
    e = rel_l2(got, want)
    fn = sampling.get_sampling_fn(cfg, sde, (2, Cc, R, R, R), lambda x: x, 1e-3, grid_mask=gm.float().view(1, R, R, R).cuda())
    plain = fn(gc.GaussianEps(s["s"], N), x0=ends.cuda())[0].float().cpu()
    e_ends = rel_l2(got[[0, K - 1]], plain)
    print(f"interp (K = 4, closed-form model): decoded rows vs ddim_recursion(slerp_ref) {e:.3e}; ends vs their plain decode {e_ends:.3e}")
    assert e <= 4e-6
    assert e_ends <= 4e-6
    assert float((got * (1 - gm.float())).abs().max()) == 0.0


def test_interp_driver_encodes_sources_and_keeps_the_reference_entry_point(hip_lib, tmp_path, monkeypatch):
    """With interp_sources the rows are encoded by the inverse of the configured sampler first: the result is the decode of the
    slerp of the recursion's latents.  Bar 1e-5: the encode loop's 2e-6 times the slerp's |w1| + |w2| <= 1.5 (theta is near pi/2
    for independent grids), plus the 4e-6 of the decoded rows above, 7e-6, rounded up; theta moves by the encode error over
    sin(theta).  uncond_gen_interp writes {idx}.npy with one pair of K = eval.batch_size points."""
    from meshdiffusion_amd.lib.diffusion import sampling
    s, cfg, evaler = _closed_form_evaler(monkeypatch, tmp_path)
    sde, N, gm, R, Cc = s["sde"], s["N"], s["gm"], s["R"], s["C"]
    K = 3
    data = torch.randn((2, Cc, R, R, R), generator=torch.Generator().manual_seed(6)) * gm.float()
    np.save(tmp_path / "src.npy", data.numpy())
    cfg.eval.interp_sources, cfg.eval.interp_points = str(tmp_path / "src.npy"), K
    got = evaler.interp(cfg, save_fname="walk")
    meta = np.load(tmp_path / "out" / "walk_meta.npz")
    assert bool(meta["encoded"]) and got.shape == (K, Cc, R, R, R) and np.array_equal(np.load(tmp_path / "out" / "walk.npy"), got.numpy())
    ts = sampling.ddim_schedule(N)
    lat = lc.ddim_encode_recursion(sde, s["s"], data, gm, ts).float()
    v, _, _, theta = lc.slerp_ref(lat[0:1].reshape(1, Cc, -1).numpy(), lat[1:2].reshape(1, Cc, -1).numpy(), gm.reshape(-1).numpy(),
                                  np.arange(K) / (K - 1.0))
    want = gc.ddim_recursion(sde, s["s"], torch.from_numpy(v[0].astype(np.float64)).view(K, Cc, R, R, R), None, None, gm, 0, 0.0,
                             False, ts)
    e = rel_l2(got, want)
    print(f"interp from sources (closed-form model): vs the recursions {e:.3e}; theta {float(meta['theta'][0]):.4f} vs {float(theta[0]):.4f}")
    assert e <= 1e-5 and abs(float(meta["theta"][0]) - float(theta[0])) <= 1e-5
    cfg.eval.batch_size, cfg.eval.interp_sources = 5, None
    torch.manual_seed(8)
    walk = evaler.uncond_gen_interp(cfg, idx=3)
    assert walk.shape == (5, Cc, R, R, R) and np.array_equal(np.load(tmp_path / "out" / "3.npy"), walk.numpy())
    cfg.sampling.method = "pc"
    with pytest.raises(NotImplementedError, match="sampling.method"):
        evaler.interp(cfg)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(hip_lib, tmp_path_factory):
    """The small checkpoint of test_gpu_cli with its cwd-relative grid mask, and run(out, *flags): one `--mode=interp` call with
    interp_points = 3 from that directory, returning (interp.npy, interp_meta.npz)."""
    import os
    sys.path.insert(0, ROOT)
    import main_diffusion
    from meshdiffusion_amd import synth
    from test_gpu_cli import _write_ckpt_and_mask
    tmp = tmp_path_factory.mktemp("interp_cli")
    cfg = synth.small_config(); cfg.device = torch.device("cuda")
    ck = _write_ckpt_and_mask(tmp, cfg, synth)
    cdir = tmp / "configs"; cdir.mkdir()
    (cdir / "small.py").write_text("from meshdiffusion_amd import synth\n\ndef get_config():\n    return synth.small_config()\n")
    R = cfg.data.image_size

    def run(out, *more):
        cwd, world = os.getcwd(), os.environ.pop("WORLD_SIZE", None)
        os.chdir(tmp)                                  # the mask path is cwd-relative in the reference
        try:
            torch.manual_seed(0)
            main_diffusion.main(["--config", str(cdir / "small.py"), "--mode=interp", f"--config.eval.eval_dir={tmp / out}",
                                 f"--config.eval.ckpt_path={ck}", "--config.eval.interp_points=3", *more])
        finally:
            os.chdir(cwd)
            if world is not None:
                os.environ["WORLD_SIZE"] = world
        return np.load(tmp / out / "interp.npy"), np.load(tmp / out / "interp_meta.npz")

    first = run("out", "--config.sampling.method=ddim")
    return dict(run=run, first=first, R=R, mask=synth.synthetic_grid_mask(R).numpy(), tmp=tmp)


def test_cli_interp_mode(cli):
    """`main_diffusion.py --mode=interp --config.sampling.method=ddim --config.eval.interp_points=3` on the small checkpoint writes
    interp.npy (3, 4, R, R, R), finite, zero outside the mask, rows distinct, and the meta file."""
    (x, meta), R, m = cli["first"], cli["R"], cli["mask"]
    assert x.shape == (3, 4, R, R, R) and x.dtype == np.float32 and np.isfinite(x).all()
    assert np.abs(x * (1 - m)).max() == 0.0 and np.abs(x).max() > 0
    assert all(not np.array_equal(x[i], x[j]) for i in range(3) for j in range(i))
    assert np.array_equal(meta["alpha"], [0.0, 0.5, 1.0]) and meta["theta"].shape == (1,) and 0.0 < float(meta["theta"][0]) < np.pi
    assert not bool(meta["encoded"]) and str(meta["method"]) == "ddim"


def test_cli_interp_sources(cli):
    """With interp_sources set to two earlier rows the run encodes them first and the meta file says so; sampling.method=pc exits
    with the constraint's message."""
    (x, _), R, m, tmp = cli["first"], cli["R"], cli["mask"], cli["tmp"]
    np.save(tmp / "src.npy", x[[0, 2]])
    x2, meta2 = cli["run"]("out2", "--config.sampling.method=ddim", f"--config.eval.interp_sources={tmp / 'src.npy'}")
    assert bool(meta2["encoded"]) and x2.shape == (3, 4, R, R, R) and np.isfinite(x2).all() and np.abs(x2 * (1 - m)).max() == 0.0
    assert meta2["theta"].shape == (1,) and 0.0 < float(meta2["theta"][0]) < np.pi
    with pytest.raises(SystemExit, match="sampling.method 'ddim', 'dpmpp' with dpmpp_tau = 0, or 'ode', got 'pc'"):
        cli["run"]("out3", "--config.sampling.method=pc")
