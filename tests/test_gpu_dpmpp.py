"""DPM-Solver++ on the GPU: md_multistep_step against extended precision with bars from its operation count, the arguments it
refuses, the sampler's loop against the float64 recursion of a closed-form model (orders 1-3, both order-2 variants, ODE and SDE),
against the oracle U-Net on the small network, under reconstruction guidance, and from the CLI."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import dpmpp_cases as dc
import guidance_cases as gc
from conftest import GOLD, ROOT, rel_l2

pytestmark = pytest.mark.gpu

BIG = (2, 4, 131076)


def _trip(B, CP):
    """Values per sample that one trip of the kernel's grid-stride loop covers: stream_blocks(CP, B) workgroups of 256 threads,
    four values each (csrc/sde_steps.hip)."""
    return min((CP // 4 + 255) // 256, 1 if B >= 1024 else 1024 // B) * 1024


def _rows(B, tau):
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    sde = sde_lib.VPSDE(dc.BETA0, dc.BETA1, 1000, device="cpu")
    rows = sampling.dpmpp_tables(sde, sampling.dpmpp_schedule(sde, 20), order=3, tau=tau, lower_order_final=False)[0]
    return rows[[5, 11, 17][:B]].contiguous()            # one level per sample, all three history coefficients non-zero


SETS = list(itertools.product((0, 1, 2), (False, True), (False, True), (None, "first", "last")))
FEW = [(0, False, False, None), (1, False, True, "first"), (2, True, True, "last"), (2, True, False, None)]


@pytest.mark.parametrize("B,Cc,P", [(1, 1, 4), (2, 4, 64), (3, 4, 1028), BIG])
def test_multistep_kernel(hip_lib, B, Cc, P):
    """Every operand set (0 / 1 / 2 earlier predictions, with and without z, mask, replacement on the first and the last channel)
    on the small shapes; on the big one -- C*P = 524304 is past the 524288 values that one trip of the grid-stride loop covers at
    B = 2, so its last 16 values per sample come from a second trip -- four sets that between them hold every operand.
    Bars from the operation count (three roundings in x0; at most five products and four sums in x_new, plus x0's own error):
    |x0 - exact| <= 4 u (|x| + |sigma eps|)/alpha, |x_new - exact| <= 8 u sum|term|, u = 2^-53, exact in longdouble."""
    from meshdiffusion_amd import hip_ops as ops
    big = (B, Cc, P) == BIG
    assert (Cc * P > _trip(B, Cc * P)) == big
    t = dc.kernel_inputs(B, Cc, P, seed=B * 1000 + P)
    cu = {k: v.cuda() for k, v in t.items()}
    n = {k: v.numpy() for k, v in t.items()}
    worst0 = worst1 = 0.0
    for nh, has_z, masked, rep in (FEW if big else SETS):
        ch = {None: 0, "first": 0, "last": Cc - 1}[rep]
        coef = _rows(B, 1 if has_z else 0)
        pick = lambda d: ((d["h1"], d["h2"])[:nh], d["z"] if has_z else None, d["mask"] if masked else None,           # noqa: E731
                          d["partial"] if rep else None, d["pmask"] if rep else None)
        hist, z, mask, part, pm = pick(cu)
        xn, x0, x32 = (v.cpu().numpy().reshape(B, Cc, P) for v in
                       ops.multistep_step(cu["x"], cu["eps"], hist, z, mask, coef.cuda(), part, pm, ch))
        hist, z, mask, part, pm = pick(n)
        ref = dc.multistep_ref(n["x"], n["eps"], hist[0] if nh > 0 else None, hist[1] if nh > 1 else None, z, mask, coef.numpy(), part, pm, ch)
        k = ref["keep"]
        e0 = np.abs(x0 - ref["x0"])[k] / ref["x0_bar"][k] / dc.U
        e1 = np.abs(xn - ref["x_new"])[k] / ref["terms"][k] / dc.U
        worst0, worst1 = max(worst0, float(e0.max())), max(worst1, float(e1.max()))
        assert e0.max() <= 4.0 and e1.max() <= 8.0, (nh, has_z, masked, rep, float(e0.max()), float(e1.max()))
        assert x32.dtype == np.float32 and np.array_equal(x32.view(np.uint32), xn.astype(np.float32).view(np.uint32))
        if masked:                                       # the replacement comes after the mask: a replaced voxel is not zeroed
            dead = np.broadcast_to(n["mask"] == 0, (B, Cc, P)).copy()
            if rep:
                dead[:, ch] &= n["pmask"] == 0
            assert np.all(xn[dead] == 0.0) and np.all(x0[dead] == 0.0)
        if rep:
            vis = n["pmask"] == 1
            assert np.all(xn[:, ch][:, vis] == n["partial"][vis]) and np.all(x0[:, ch][:, vis] == n["partial"][vis])
    print(f"({B},{Cc},{P}): worst |x0 - exact| = {worst0:.2f} u (|x|+|sigma eps|)/alpha, worst |x_new - exact| = {worst1:.2f} u sum|term|")


def test_refused_arguments(hip_lib):
    """Every refused argument gives MD_ERR_BAD_ARG from the host checks: nothing is launched, the outputs keep their bytes."""
    from meshdiffusion_amd import _lib
    B, Cc, P = 2, 4, 64
    t = {k: v.cuda() for k, v in dc.kernel_inputs(B, Cc, P, seed=1).items()}
    coef = _rows(B, 1).cuda()
    outs = dict(x_out=torch.full((B, Cc, P), 7.0, dtype=torch.float64, device="cuda"),
                x0_out=torch.full((B, Cc, P), 7.0, dtype=torch.float64, device="cuda"),
                x_f32=torch.full((B, Cc, P), 7.0, device="cuda"))
    order = ["x", "eps", "h1", "h2", "z", "mask", "coef", "partial", "pmask", "ch", "x_out", "x0_out", "x_f32", "batch", "C", "P"]
    base = dict(t, coef=coef, ch=0, batch=B, C=Cc, P=P, **outs)

    def call(**change):
        a = dict(base, **change)
        args = [(C.c_void_p(v.data_ptr()) if torch.is_tensor(v) else C.c_void_p(v) if (k not in ("ch", "batch", "C", "P")) else v)
                for k, v in ((k, a[k]) for k in order)]
        return hip_lib.md_multistep_step(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    addr = lambda name, off=0: base[name].data_ptr() + off                                  # noqa: E731
    bad = [dict(P=6), dict(P=0), dict(batch=0), dict(C=0), dict(ch=-1), dict(ch=Cc), dict(partial=None), dict(pmask=None),
           dict(h1=None), dict(x=None), dict(eps=None), dict(coef=None), dict(x_out=None), dict(x0_out=None), dict(x_f32=None),
           dict(coef=addr("coef", 4))]
    bad += [{k: addr(k, 8)} for k in ("x", "eps", "h1", "h2", "z", "mask", "partial", "pmask", "x_out", "x0_out", "x_f32")]
    bad += [dict(x_out=addr("x")), dict(x0_out=addr("h1")), dict(x0_out=addr("h2")), dict(x_f32=addr("eps")), dict(x_f32=addr("z")),
            dict(x_out=addr("x0_out")), dict(x0_out=addr("x_f32")), dict(x_out=addr("x_f32")), dict(x_f32=addr("mask")),
            dict(x_f32=addr("partial")), dict(x_f32=addr("pmask")), dict(x_out=addr("coef")),
            dict(x_out=addr("x", 16 * (B * Cc * P // 2 - 2)))]                                # only the tails overlap
    for change in bad:
        assert call(**change) == _lib.ERR_BAD_ARG, change
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in outs.values())
    assert call() == _lib.OK and call(h1=None, h2=None, z=None, mask=None, partial=None, pmask=None) == _lib.OK
    torch.cuda.synchronize()
    assert not any(bool((v == 7.0).any()) for v in outs.values())


# ---- the loop against the closed form ------------------------------------------------------------------------------------------
def _replay(noise):
    it = iter(noise)

    def draw(like):
        z = next(it)
        assert z.shape == like.shape and z.dtype == like.dtype
        return z
    return draw


CONFIGS = [(1, "taylor"), (2, "taylor"), (2, "midpoint"), (3, "taylor")]


def test_loop_against_the_closed_form(hip_lib):
    """dpmpp_sampler on eps_hat = k_t x (8^3, B = 2, grid mask, 20 'logsnr' steps) against the float64 recursion that restates the
    loop's two float32 roundings (the state the model sees, eps_hat as it returns it); rows, ring slots and noise as the sampler
    uses them.  Past those roundings every operation is a float64 one on host-made coefficients: rel-L2 <= 1e-10.
    Measured on an MI355X: 0 (bit-equal) in all eight runs; order 1 vs order 2 1.3e-1, 'taylor' vs 'midpoint' 1.2e-2."""
    from meshdiffusion_amd.lib.diffusion import sampling
    s = gc.loop_setup()
    sde, N, gm, shape = s["sde"], s["N"], s["gm"], s["shape"]
    model = gc.GaussianEps(s["s"], N)
    steps = 20
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(5)
    noise = [torch.randn(shape, generator=g) for _ in range(steps)]
    times = sampling.dpmpp_schedule(sde, steps, "logsnr", 1e-3)
    got = {}
    for tau in (0, 1):
        for order, variant in CONFIGS:
            fn = sampling.get_dpmpp_sampler(sde, shape, lambda v: v, steps=steps, order=order, variant=variant, tau=tau,
                                            device="cuda", grid_mask=gm.float())
            out, nfe = fn(model, x0=x_T, draw=_replay([z.cuda() for z in noise]))
            rows, labels = sampling.dpmpp_tables(sde, times, order=order, variant=variant, tau=tau)
            want = dc.recursion(model, x_T, rows, labels, sampling.dpmpp_orders(steps, order), gm=gm, noise=noise)
            dist = rel_l2(out, want)
            got[(tau, order, variant)] = out.cpu()
            print(f"tau {tau} order {order} {variant}: loop vs float64 recursion rel-L2 {dist:.3e}")
            assert nfe == steps and out.dtype == torch.float64 and float((out.cpu() * (1 - gm)).abs().max()) == 0.0
            assert dist <= 1e-10
            den, _ = sampling.get_dpmpp_sampler(sde, shape, lambda v: v, steps=steps, order=order, variant=variant, tau=tau,
                                                denoise=True, device="cuda", grid_mask=gm.float())(model, x0=x_T, draw=_replay([z.cuda() for z in noise]))
            assert rel_l2(den, dc.recursion(model, x_T, rows, labels, sampling.dpmpp_orders(steps, order), gm=gm, noise=noise,
                                            denoise=True)) <= 1e-10
    apart = rel_l2(got[(0, 1, "taylor")], got[(0, 2, "taylor")])
    print(f"order 1 vs order 2: {apart:.3e}; taylor vs midpoint: {rel_l2(got[(0, 2, 'midpoint')], got[(0, 2, 'taylor')]):.3e}; "
          f"order 2 vs 3: {rel_l2(got[(0, 3, 'taylor')], got[(0, 2, 'taylor')]):.3e}")
    assert apart >= 1e-3                                 # the case can tell a wrong row or ring slot from the right one


def test_guided_loop_against_the_closed_form(hip_lib):
    """The guided loop (zeta = 1, order 2, 20 'logsnr' steps, replacement on and off) against the exact guided float64 recursion.
    Bar max(4 a, 1e-6): a (tests/golden/dpmpp.npz, tools/gen_golden_dpmpp.py) is how far that recursion itself moves when the
    guidance input is rounded to float32, one of the about four float32 roundings of a guided step.  a = 0 with replacement on
    (the visible voxels stay a multiple of the +-1 partial grid, and the normalised step does not see their common factor) and
    5.4e-7 with it off: below 1e-6 on 'logsnr', so the default schedule stays.
    Measured on an MI355X: guided distance 4.0e-8 (replacement on, bar 1e-6), 1.9e-6 (off, bar 2.2e-6); guided vs unguided
    8.1e-2 / 4.6e-2; the unguided run against the exact recursion 4.1e-8."""
    from meshdiffusion_amd.lib.diffusion import sampling
    gold = np.load(os.path.join(GOLD, "dpmpp.npz"))
    s = gc.loop_setup()
    sde, N, ch, y, pm, gm, shape = s["sde"], s["N"], s["ch"], s["y"], s["pm"], s["gm"], s["shape"]
    steps, order = int(gold["steps"]), int(gold["order"])
    assert str(gold["schedule"]) == "logsnr" and max(float(gold["a_on"]), float(gold["a_off"])) <= 1e-6
    model = gc.GaussianEps(s["s"], N)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(int(gold["seed"])))
    fn = sampling.get_dpmpp_sampler(sde, shape, lambda v: v, steps=steps, order=order, device="cuda", grid_mask=gm.float())
    rows, labels = sampling.dpmpp_tables(sde, sampling.dpmpp_schedule(sde, steps), order=order)
    orders = sampling.dpmpp_orders(steps, order)

    def gpu(zeta, replace, **kw):
        return fn(model, x0=x_T, partial=y.float(), partial_mask=pm.float(), partial_channel=ch, guidance_scale=zeta,
                  guidance_replace=replace, **kw)[0].cpu()

    def ref(zeta, replace):
        guide = dc.gaussian_guide(s["s"], N, rows, labels, y, pm, gm, zeta, ch) if zeta else None
        return dc.recursion(model, x_T, rows, labels, orders, gm=gm, partial=y if replace else None, pm=pm, ch=ch, guide=guide,
                            round_state=False)

    plain = gpu(0.0, True)
    print(f"unguided, replacement on: loop vs exact float64 recursion {rel_l2(plain, ref(0.0, True)):.3e}")
    for tag, replace in (("on", True), ("off", False)):
        bar = max(4.0 * float(gold[f"a_{tag}"]), 1e-6)
        got, want = gpu(s["zeta"], replace), ref(s["zeta"], replace)
        dist, moved = rel_l2(got, want), rel_l2(got, plain)
        print(f"replacement {tag}: a = {float(gold[f'a_{tag}']):.3e}, bar {bar:.3e}, guided distance {dist:.3e}, guided vs unguided {moved:.3e}")
        assert torch.isfinite(got).all() and float((got * (1 - gm)).abs().max()) == 0.0
        assert moved >= 100 * bar
        assert dist <= bar
        assert torch.equal(gpu(s["zeta"], replace, guidance_chunk=1), got)          # the callable is per-sample: chunking is exact


# ---- the small U-Net ---------------------------------------------------------------------------------------------------------------
def test_small_unet_against_the_oracle(hip_lib):
    """get_sampling_fn(method='dpmpp') on the small network (R = 16, B = 2, grid mask, 12 steps, order 2, tau 0), unconditional
    and with replacement on channel 0, against the float64 recursion driven by the oracle U-Net in fp32 on the CPU: rel-L2 < 1e-3
    (the project's parity bar), exactly 0 outside the mask, nfe == steps.  Measured on an MI355X: 9.1e-6 and 9.0e-6."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from oracle import unet_oracle as uo
    from test_gpu_ddim import _small
    cfg, model, sd = _small("dpmpp", False)
    cfg.sampling.dpmpp_steps = 12
    R, B, steps = cfg.data.image_size, 2, 12
    N = cfg.model.num_scales
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, N, device="cuda")
    gm = synth.synthetic_grid_mask(R).view(R, R, R)
    mask = gm.view(1, R, R, R)
    fn = sampling.get_sampling_fn(cfg, sde, (B, 4, R, R, R), lambda v: v, 1e-3, grid_mask=mask.cuda())
    g = torch.Generator().manual_seed(7)
    x_T = torch.randn((B, 4, R, R, R), generator=g)
    y = torch.sign(torch.randn((R, R, R), generator=g))
    pm = (torch.rand((R, R, R), generator=g) < 0.3).float() * gm
    sde_cpu = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, N, device="cpu")
    rows, labels = sampling.dpmpp_tables(sde_cpu, sampling.dpmpp_schedule(sde_cpu, steps), order=2)
    ocfg = synth.oracle_cfg(cfg)

    def eps_oracle(x, lab):
        with torch.no_grad():
            return uo.unet_res64_forward(sd, ocfg, x, lab)

    for tag, part in (("unconditional", None), ("replacement on channel 0", y)):
        kw = {} if part is None else dict(partial=part, partial_mask=pm, partial_channel=0)
        out, nfe = fn(model, x0=x_T.cuda(), **kw)
        want = dc.recursion(eps_oracle, x_T, rows, labels, sampling.dpmpp_orders(steps, 2), gm=gm.double(),
                            partial=None if part is None else part.double(), pm=pm.double(), ch=0)
        e = rel_l2(out, want)
        print(f"small U-Net, 12 steps, {tag}: vs oracle recursion {e:.3e}")
        assert nfe == steps and out.dtype == torch.float64 and e < 1e-3
        assert float((out.cpu() * (1 - mask)).abs().max()) == 0.0
        if part is not None:
            vis = pm.bool()
            assert torch.equal(out.cpu()[:, 0][:, vis], y.double()[vis].expand(B, -1))


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------
def test_cli_dpmpp(hip_lib, tmp_path, monkeypatch):
    """`main_diffusion.py --mode=uncond_gen|cond_gen --config.sampling.method=dpmpp` (cond_gen with and without guidance) writes
    the .npy with the batch's shape and zeros outside the mask."""
    sys.path.insert(0, ROOT)
    import main_diffusion
    from meshdiffusion_amd import synth
    from test_gpu_cli import _write_ckpt_and_mask
    cfg = synth.small_config(); cfg.device = torch.device("cuda")
    ck = _write_ckpt_and_mask(tmp_path, cfg, synth)
    cdir = tmp_path / "configs"; cdir.mkdir()
    (cdir / "small.py").write_text("from meshdiffusion_amd import synth\n\ndef get_config():\n    return synth.small_config()\n")
    monkeypatch.chdir(tmp_path)
    R = cfg.data.image_size
    m = synth.synthetic_grid_mask(R).numpy()
    idx = np.argwhere(m > 0).astype(np.float32)
    verts = (idx / (R - 1) - 0.5).astype(np.float32)
    tet_path = tmp_path / "tets.npz"
    np.savez(tet_path, vertices=verts, indices=np.zeros((1, 4), np.int32))
    g = torch.Generator().manual_seed(1)
    part = {"sdf": torch.sign(torch.randn(len(verts), generator=g)), "vis": torch.rand(len(verts), generator=g) < 0.5}
    ppath = tmp_path / "dmtet.pt"
    torch.save(part, ppath)

    def run(out, mode, *more):
        torch.manual_seed(0)
        main_diffusion.main(["--config", str(cdir / "small.py"), f"--mode={mode}", f"--config.eval.eval_dir={out}",
                             f"--config.eval.ckpt_path={ck}", "--config.eval.batch_size=2", "--config.sampling.method=dpmpp",
                             "--config.sampling.dpmpp_steps=6", *more])
        x = np.load(out / "0.npy")
        assert x.shape == (2, 4, R, R, R) and np.isfinite(x).all() and np.abs(x * (1 - m)).max() == 0.0 and np.abs(x).max() > 0
        return x

    cond = [f"--config.eval.partial_dmtet_path={ppath}", f"--config.eval.tet_path={tet_path}", "--config.eval.calibrate=False"]
    xu = run(tmp_path / "uncond", "uncond_gen", "--config.sampling.dpmpp_order=3", "--config.sampling.dpmpp_tau=1")
    xc = run(tmp_path / "cond", "cond_gen", *cond)
    xg = run(tmp_path / "guided", "cond_gen", *cond, "--config.eval.guidance_scale=1.0", "--config.eval.guidance_replace=False")
    assert not np.array_equal(xu, xc) and not np.array_equal(xc, xg)
    sdf = np.zeros((R, R, R), np.float32)
    vis = np.zeros((R, R, R), bool)
    ii = np.round((verts - verts.min()) / (np.unique(verts)[1] - np.unique(verts)[0])).astype(int)
    sdf[ii[:, 0], ii[:, 1], ii[:, 2]], vis[ii[:, 0], ii[:, 1], ii[:, 2]] = part["sdf"].numpy(), part["vis"].numpy()
    assert np.array_equal(xc[:, 0][:, vis], np.broadcast_to(sdf[vis], (2, int(vis.sum()))))       # the known voxels are kept
