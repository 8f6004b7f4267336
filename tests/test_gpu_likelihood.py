"""Probability-flow ODE likelihood on the GPU: md_pf_ode_rhs against its float64 restatement; one right-hand-side evaluation
(taped forward + data-gradient-only backward + md_pf_ode_rhs) against the oracle; the whole solve, the ODE sampler's round trip
and the CLI against tests/golden/likelihood.npz (tools/gen_golden_likelihood.py: oracle + scipy on the CPU)."""
import os
import sys

import numpy as np
import pytest
import torch

import likelihood_cases as lc
from conftest import ROOT, rel_l2

pytestmark = pytest.mark.gpu


# ---- md_pf_ode_rhs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_div", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,P", [(3, 64), (2, 16 ** 3), (1, 1028), (8, 32 ** 3 + 4)])
def test_pf_ode_rhs_kernel(hip_lib, B, P, masked, with_div):
    """The last two shapes are flat grids.  P = 1028 with one channel: 257 threads, a last workgroup of one lane.  B = 8, C = 4,
    P = 32^3 + 4: C*P = 131088 is 16 past the 131072 values one trip of the 128 workgroups covers (without the divergence)."""
    from meshdiffusion_amd import _lib, hip_ops as ops
    g = torch.Generator().manual_seed(B * 1000 + P)
    C = 1 if P == 1028 else 4
    side = round(P ** (1 / 3))
    shape = (B, C, side, side, side) if side ** 3 == P else (B, C, 1, 1, P)
    x, e, jt = (torch.randn(shape, generator=g) for _ in range(3))
    probe = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    mask = (torch.rand(P, generator=g) < 0.3).float() if masked else None
    coef = np.array([lc.vp_coefficients_f64(t)[:2] for t in (1e-3, 0.5, 1.0, 0.25, 0.75, 0.1, 0.9, 0.6)][:B])
    kw = dict(g=jt.cuda(), probe=probe.cuda()) if with_div else {}
    args = (x.cuda(), e.cuda(), mask.cuda() if masked else None, torch.from_numpy(coef).cuda())
    drift, div = ops.pf_ode_rhs(*args, **kw)
    r_drift, r_div, mag = lc.pf_ode_rhs_f64(x.view(B, C, P).numpy(), e.view(B, C, P).numpy(), mask.numpy() if masked else None, coef,
                                            g=jt.view(B, C, P).numpy() if with_div else None,
                                            probe=probe.view(B, C, P).numpy() if with_div else None)
    d = drift.cpu().view(B, C, P).numpy()
    ulp = np.spacing(np.abs(r_drift))
    assert np.all(np.abs(d.astype(np.float64) - r_drift.astype(np.float64)) <= ulp), "drift: more than 1 ulp of fp32 from float64"
    if masked:
        assert np.all(d[:, :, mask.numpy() == 0] == 0)
    if with_div:
        err = np.abs(div.cpu().numpy() - r_div) / mag
        print(f"divergence B={B} P={P} masked={masked}: |err| / sum|terms| {err}")
        assert np.all(err <= 1e-12)
    else:
        assert div is None
    drift2, div2 = ops.pf_ode_rhs(*args, **kw)                                # deterministic: the same bits again
    assert torch.equal(drift, drift2) and (div is None or torch.equal(div, div2))
    lib = _lib.load()
    rc = lib.md_pf_ode_rhs(ops._ptr(args[0]), ops._ptr(args[1]), None, None, None, ops._ptr(args[3]), ops._ptr(drift), None, B, C, P - 2,
                           ops._stream())
    assert rc == _lib.ERR_BAD_ARG                                              # P % 4


# ---- the small network of the golden ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(gold_dir):
    return dict(np.load(os.path.join(gold_dir, "likelihood.npz")))


@pytest.fixture(scope="module")
def net():
    from meshdiffusion_amd.lib.diffusion import sde_lib
    from meshdiffusion_amd.lib.diffusion.models import utils as mutils
    cfg, gm, x0 = lc.golden_setup("cuda:0")
    model = mutils.create_model(cfg).eval()
    sd = lc.golden_state_dict(cfg, model.module.state_dict(), gm)
    model.module.load_state_dict(sd, strict=True)
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device=cfg.device)
    return dict(cfg=cfg, model=model, sd=sd, gm=gm, x0=x0, sde=sde)


@pytest.mark.parametrize("t", [1e-3, 0.5, 1.0])
def test_one_rhs_evaluation_against_the_oracle(hip_lib, net, gold, t):
    """fun(t, y) of likelihood.get_ode_rhs on the golden's x0 and probe: the network part of the drift within 1e-4 (the forward
    bar), probe . J^T probe within 2e-3 relative (the whole-net gradient bar)."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import likelihood
    from oracle import unet_oracle as uo
    cfg, x0, gm = net["cfg"], net["x0"], net["gm"]
    R, B = cfg.data.image_size, 2
    mask = gm.view(1, 1, R, R, R)
    probe = torch.from_numpy(gold["probe"]).float()
    xr = x0.clone().requires_grad_(True)
    e = uo.unet_res64_forward(net["sd"], synth.oracle_cfg(cfg), xr, torch.full((B,), t * 999))
    jt, = torch.autograd.grad(e, xr, probe)
    ref_net = (e.detach() * mask).double()
    ref_pjp = (probe * jt).double().sum(dim=(1, 2, 3, 4))
    fun = likelihood.get_ode_rhs(net["sde"], net["model"], tuple(x0.shape), x0.cuda(), grid_mask=gm, probe=probe.cuda())
    y = torch.cat([x0.double().reshape(-1), torch.zeros(B, dtype=torch.float64)]).cuda()
    out = fun(t, y).cpu()
    cx, ce = lc.vp_coefficients_f64(t)[:2]
    got_net = (out[:-B].view(x0.shape) - cx * x0.double() * mask) / ce
    got_pjp = (out[-B:] - cx * (probe * probe).double().sum(dim=(1, 2, 3, 4))) / ce
    err_n, err_j = rel_l2(got_net, ref_net), ((got_pjp - ref_pjp).abs() / ref_pjp.abs()).max().item()
    print(f"t={t}: eps_hat part of the drift rel-L2 {err_n:.2e}; probe.J^T probe {got_pjp.tolist()} vs {ref_pjp.tolist()}: rel {err_j:.2e}")
    assert err_n < 1e-4 and err_j < 2e-3
    assert all(p.grad is None for p in net["model"].parameters())


@pytest.fixture(scope="module")
def solve(net, gold):
    """The GPU solve at rtol = atol = 1e-3, once for the tests below."""
    from meshdiffusion_amd.lib.diffusion import likelihood
    fn = likelihood.get_likelihood_fn(net["sde"], lambda x: x, rtol=1e-3, atol=1e-3, eps=1e-3, grid_mask=net["gm"])
    bpd, z, nfe, delta_logp, prior_logp = fn(net["model"], net["x0"].cuda(), return_parts=True,
                                             probe=torch.from_numpy(gold["probe"]).float().cuda())
    return dict(bpd=bpd.cpu(), z=z.cpu(), nfe=nfe, delta_logp=delta_logp.cpu().numpy(), prior_logp=prior_logp.cpu().numpy())


def test_likelihood_end_to_end(hip_lib, net, gold, solve):
    """|delta_logp - golden(1e-5)| <= 2 u: one u = |golden(1e-3) - golden(1e-5)| for the 1e-3 solve itself, one for an accept /
    reject decision flipping under 2e-3-level arithmetic differences; z within twice the golden's own 1e-3-vs-1e-5 distance;
    nfe within two steps (12 evaluations) of the golden's."""
    B = 2
    d5, u = gold["delta_logp_5"], gold["u"]
    z5 = torch.from_numpy(gold["z_5"])
    dist = [rel_l2(solve["z"][b], z5[b]) for b in range(B)]
    print(f"delta_logp {solve['delta_logp']} (golden 1e-5 {d5}, 1e-3 {gold['delta_logp_3']}, u {u}); |diff| / u "
          f"{np.abs(solve['delta_logp'] - d5) / u}; z distance {dist} (golden 1e-3 vs 1e-5 {gold['z_dist']}); nfe {solve['nfe']} "
          f"(golden {int(gold['nfev_3'])}); bits/dim {solve['bpd'].tolist()}")
    assert np.all(np.abs(solve["delta_logp"] - d5) <= 2 * u)
    assert all(dist[b] <= 2 * gold["z_dist"][b] for b in range(B))
    assert abs(solve["nfe"] - int(gold["nfev_3"])) <= 12
    n_dim = 4 * float(net["gm"].sum())
    ref_bpd = -(solve["prior_logp"] + solve["delta_logp"]) / np.log(2) / n_dim + 8.0
    assert np.allclose(solve["bpd"].numpy(), ref_bpd, rtol=1e-6) and np.isfinite(ref_bpd).all()
    assert float((solve["z"] * (1 - net["gm"].view(1, 1, *net["gm"].shape))).abs().max()) == 0.0


def test_ode_sampler_round_trip(hip_lib, net, gold, solve):
    """get_ode_sampler(x0=z) runs the ODE back from T to 1e-3 on the inference path (through get_sampling_fn, method 'ode').
    The backward ODE of this synthetic network expands so strongly that no decode at 1e-3 returns x0 (the golden's CPU round trip
    ends 50 |x0| away, and still 37 |x0| away at 1e-5), so the issue's bar -- twice the CPU round-trip distance -- says little;
    what pins the sampler is the decode itself: started from the golden's z it must land on scipy's decode of the same z, within
    twice the distance `roundtrip_sens` that scipy's own decode moves when every eps_hat is off by 1e-4 relative (the forward
    bar: one such distance for this machine's arithmetic, one for an accept / reject decision flipping), with scipy's nfe
    give or take two steps."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import sampling
    x0 = net["x0"]
    cfg = synth.small_config()
    cfg.device = torch.device("cuda", 0)
    cfg.sampling.method = "ode"
    cfg.sampling.ode_rtol = cfg.sampling.ode_atol = 1e-3
    fn = sampling.get_sampling_fn(cfg, net["sde"], tuple(x0.shape), lambda x: x, 1e-3, grid_mask=net["gm"])
    mask = net["gm"].view(1, 1, *net["gm"].shape)
    ref = torch.from_numpy(gold["roundtrip"])
    back, nfe = fn(net["model"], x0=torch.from_numpy(gold["z_3"]).cuda())
    back = back.cpu()
    dist = [rel_l2(back[b], ref[b]) for b in range(2)]
    print(f"decode of the golden's z against scipy's decode: rel-L2 {dist} (yardstick roundtrip_sens {gold['roundtrip_sens']}), nfe {nfe} "
          f"(scipy {int(gold['roundtrip_nfev'])})")
    assert torch.isfinite(back).all() and float((back * (1 - mask)).abs().max()) == 0.0
    assert all(dist[b] <= 2 * gold["roundtrip_sens"][b] for b in range(2))
    assert abs(nfe - int(gold["roundtrip_nfev"])) <= 12
    # the issue's bar, on the GPU solve's own z
    back2, nfe2 = fn(net["model"], x0=solve["z"].cuda())
    rt = [rel_l2(back2[b].cpu(), x0[b]) for b in range(2)]
    print(f"round trip distance {rt} (golden CPU round trip {gold['roundtrip_dist']}; at 1e-5 {gold['roundtrip_dist_5']}), nfe {nfe2}")
    assert all(rt[b] <= 2 * gold["roundtrip_dist"][b] for b in range(2))
    with pytest.raises(NotImplementedError):
        fn(net["model"], partial=x0)


def test_cli_likelihood_mode(hip_lib, tmp_path, monkeypatch):
    """`main_diffusion.py --mode=likelihood` on a synthetic checkpoint and a two-grid dataset writes likelihood.npz."""
    import json
    sys.path.insert(0, ROOT)
    import main_diffusion
    from meshdiffusion_amd import synth
    from test_gpu_cli import _write_ckpt_and_mask
    cfg = synth.small_config(); cfg.device = torch.device("cuda")
    ck = _write_ckpt_and_mask(tmp_path, cfg, synth)
    R = cfg.data.image_size
    g = torch.Generator().manual_seed(5)
    paths = []
    for i in range(2):
        grid = torch.cat([torch.sign(torch.randn((1, R, R, R), generator=g)), torch.rand((3, R, R, R), generator=g) - 0.5])
        p = tmp_path / f"grid_{i:05d}.pt"
        torch.save(grid, p)
        paths.append(str(p))
    json.dump(paths, open(tmp_path / "meta.json", "w"))
    json.dump([0, 1], open(tmp_path / "keep.json", "w"))
    cdir = tmp_path / "configs"; cdir.mkdir()
    (cdir / "small.py").write_text("from meshdiffusion_amd import synth\n\ndef get_config():\n    return synth.small_config()\n")
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "out"
    main_diffusion.main(["--config", str(cdir / "small.py"), "--mode=likelihood", f"--config.eval.eval_dir={out}",
                         f"--config.eval.ckpt_path={ck}", "--config.eval.batch_size=2", f"--config.data.meta_path={tmp_path / 'meta.json'}",
                         f"--config.data.filter_meta_path={tmp_path / 'keep.json'}", "--config.eval.ode_rtol=1e-2",
                         "--config.eval.ode_atol=1e-2", "--config.eval.ode_eps=1e-3"])
    res = np.load(out / "likelihood.npz")
    assert set(res.files) == {"bpd", "logp", "delta_logp", "nfe", "index"}
    assert res["bpd"].shape == res["logp"].shape == res["delta_logp"].shape == (2,) and res["nfe"].shape == (1,)
    assert list(res["index"]) == [0, 1] and res["nfe"][0] > 8
    assert all(np.isfinite(res[k]).all() for k in ("bpd", "logp", "delta_logp"))
