"""Kernels on non-finite and out-of-range operands: NaN / +inf / -inf values injected at chosen voxels, elements and vertices, and
finite values far outside the calibrated range.  The reference is the same operation in torch float64 on the CPU (the optimiser:
torch's own clip_grad_norm_ + Adam + the project's EMA on the same device).  "Non-finite" = inf or NaN; the checks do not tell them apart.
  R1  where the reference is finite everywhere, so is the output
  R2  every non-finite position of the reference is non-finite in the output
  R3  output non-finites lie in the reference's non-finite set (Winograd: dilated by +-1 voxel along w, the F(2,3) tile pair reads
      w-1..w+2); finite outputs outside it keep the path's budget
  R4  a non-finite value in one sample reaches another only where the reference's does"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL_MFMA = 3e-5
TOL = {"bf16x3": TOL_MFMA, "f16f8": TOL_MFMA, "f16f6": 4e-5}
VALUES = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}
# (sample, part, w) of the injected voxel: both ends of a row, both sides of a tile pair, the second part of a two-part input
PLACES = {"w0": (0, 0, 0), "wlast": (1, 1, 15), "even": (1, 0, 6), "odd": (0, 1, 9)}


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _bad(t):
    return ~torch.isfinite(t)


def _dilate_w(m):
    d = m.clone()
    d[..., 1:] |= m[..., :-1]
    d[..., :-1] |= m[..., 1:]
    return d


def _check_spread(y, ref, tol, what, dilate=True):
    """R1 - R3 of one output against its float64 reference; returns the error of the finite outputs outside the non-finite set."""
    bad_ref, bad_y = _bad(ref), _bad(y)
    allowed = _dilate_w(bad_ref) if dilate else bad_ref
    assert not bool((bad_ref & ~bad_y).any()), f"{what}: hidden non-finites (R2): {int((bad_ref & ~bad_y).sum())}"
    assert not bool((bad_y & ~allowed).any()), f"{what}: invented non-finites (R1 / R3): {int((bad_y & ~allowed).sum())}"
    keep = ~allowed
    e = rel_l2(y[keep], ref[keep]) if bool(keep.any()) else 0.0
    assert e < tol, f"{what}: finite outputs {e:.2e} (budget {tol:.0e})"
    return e


def _pair(layers, cin, cout, gamma, beta, w):
    class Pair(layers.HipLayer):
        def __init__(self):
            super().__init__()
            self.gn = torch.nn.GroupNorm(32, cin, eps=1e-6)
            self.conv = torch.nn.Conv3d(cin, cout, 3, padding=1)

    pair = Pair()
    with torch.no_grad():
        pair.gn.weight.copy_(gamma); pair.gn.bias.copy_(beta); pair.conv.weight.copy_(w)
    return pair.cuda()


# ---- forward Winograd convs through the product dispatch ------------------------------------------------------------------------------
@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("val", list(VALUES))
@pytest.mark.parametrize("mode", ["bf16x3", "f16f8", "f16f6"])
def test_wino_conv_gn_silu_operand_nonfinite_voxel(ops, mode, val, place, monkeypatch):
    """GroupNorm affine + SiLU operand (statistics of the clean tensor: the affine folded per (sample, channel), as a fused epilogue
    hands it over) of a two-part input, one non-finite voxel -> layers.run_conv3 under precision_scope(mode), vs torch float64 of
    silu(a x + c) -> conv3d.  R1 - R3, and R4: the other sample is bit-identical to the clean run."""
    from meshdiffusion_amd.lib.diffusion.models import layers
    monkeypatch.setattr(ops, "WINO_MIN_WGS", 1)
    B, S, cout, cs = 2, 16, 128, [96, 32]
    cin = sum(cs)
    gamma, beta = 1.0 + 0.2 * _rand((cin,), 601), 0.5 * _rand((cin,), 602)
    w = _rand((cout, cin, 3, 3, 3), 603, 0.05)
    bias = _rand((B, cout), 604)
    xs = [_rand((B, k, S, S, S), 610 + i) * 1.5 + 0.3 for i, k in enumerate(cs)]
    pair = _pair(layers, cin, cout, gamma, beta, w)
    clean = [(ops.ncdhw_to_f32b(t.cuda()), k) for t, k in zip(xs, cs)]
    _, ac = ops.gn_params(clean, pair.gn.weight, pair.gn.bias, B, S ** 3, want_ac=True)
    pw = layers.conv3_packed(pair, "w", pair.conv, ops.conv_cfg_for(S))
    b, part, wx = PLACES[place]
    xb = [t.clone() for t in xs]
    xb[part][b, 5, 7, 3, wx] = VALUES[val]
    parts = [(ops.ncdhw_to_f32b(t.cuda()), k) for t, k in zip(xb, cs)]

    def run(ps):
        ops.PROFILE = []
        try:
            with ops.precision_scope(mode):
                out = layers.run_conv3(pw, None, B, S, bias=bias.cuda(), bias_bstride=cout, b_f32=ops.F32Operand(ps, ac, silu=True),
                                       wino=layers.conv3_wino_packed(pair, "w", pair.conv, gn=pair.gn))
            tags = [r[5] for r in ops.PROFILE if r[0] == "wino"]
        finally:
            ops.PROFILE = None
        return ops.f32b_to_ncdhw(out, (S, S, S)).cpu(), tags

    y, tags = run(parts)
    assert len(tags) == 1 and (tags[0].endswith("/" + mode[3:]) if mode != "bf16x3" else "/f" not in tags[0]), tags
    y0, _ = run(clean)
    acd = ac.cpu().double().view(B, cin, 2)
    ref_in = F.silu(torch.cat(xb, 1).double() * acd[..., 0, None, None, None] + acd[..., 1, None, None, None])
    ref = F.conv3d(ref_in, w.double(), padding=1) + bias.double()[:, :, None, None, None]
    e = _check_spread(y, ref, TOL[mode], f"{mode} {val} at {place}")
    assert torch.equal(y[1 - b], y0[1 - b]), "R4: the clean sample changed"
    print(f"{mode} GN+SiLU operand, {val} at {place}: finite outputs vs torch fp64 {e:.2e}")


@pytest.mark.parametrize("val", list(VALUES))
@pytest.mark.parametrize("mode", ["f16f8", "f16f6"])
def test_wino_conv_calibrated_upsample_nonfinite_voxel(ops, mode, val, monkeypatch):
    """The calibrated raw Upsample operand with the nearest-x2 fold: one non-finite coarse voxel (8 fine voxels) in sample 1."""
    from meshdiffusion_amd.lib.diffusion.models import layers
    monkeypatch.setattr(ops, "WINO_MIN_WGS", 1)
    B, S, cin, cout = 2, 16, 128, 128
    x = _rand((B, cin, S // 2, S // 2, S // 2), 620)
    up = layers.Upsample(cin, with_conv=True)
    with torch.no_grad():
        up.Conv_0.weight.copy_(_rand((cout, cin, 3, 3, 3), 621, 0.05)); up.Conv_0.bias.zero_()
    up = up.cuda().eval()
    ops.CALIBRATE = {}
    try:
        with ops.precision_scope(mode), torch.no_grad():
            up(x.cuda())
        cal = ops.CALIBRATE
    finally:
        ops.CALIBRATE = None
    for owner, site, tot, n in cal.values():
        owner._md_act_ms = {site: (tot / n).contiguous()}
    xb = x.clone()
    xb[1, 17, 2, 5, 3] = VALUES[val]

    def run(t):
        ops.PROFILE = []
        try:
            with ops.precision_scope(mode), torch.no_grad():
                y = up(t.cuda()).cpu()
            return y, [r[5] for r in ops.PROFILE if r[0] == "wino"]
        finally:
            ops.PROFILE = None

    y, tags = run(xb)
    assert tags and all(t.endswith("/" + mode[3:]) for t in tags), tags
    y0, _ = run(x)
    ref = F.conv3d(F.interpolate(xb.double(), scale_factor=2, mode="nearest"), up.Conv_0.weight.detach().double().cpu(), padding=1)
    e = _check_spread(y, ref, TOL[mode], f"upsample {mode} {val}")
    assert torch.equal(y[0], y0[0])
    print(f"calibrated Upsample {mode}, {val}: finite outputs vs torch fp64 {e:.2e}")


# ---- out-of-range finite operands: R1 plus accuracy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16f8", "f16f6"])
def test_raw_stream_equaliser_quiet_channel_then_active(ops, mode, monkeypatch):
    """An Upsample conv calibrated on a stream where channel 5 is quiet (rms 1e-8: a noise-only batch), evaluated with that channel at
    the scale of the others: the measured equaliser must not lift it out of fp16 (nor let it swamp its e2m3 block).  Then one voxel
    x 1e6 (R1 only; error printed)."""
    from meshdiffusion_amd.lib.diffusion.models import layers
    monkeypatch.setattr(ops, "WINO_MIN_WGS", 1)
    B, S, cin, cout = 1, 16, 128, 128
    x = _rand((B, cin, S // 2, S // 2, S // 2), 630)
    xq = x.clone()
    xq[:, 5] *= 1e-8
    up = layers.Upsample(cin, with_conv=True)
    with torch.no_grad():
        up.Conv_0.weight.copy_(_rand((cout, cin, 3, 3, 3), 631, 0.05)); up.Conv_0.bias.zero_()
    up = up.cuda().eval()
    ops.CALIBRATE = {}
    try:
        with ops.precision_scope(mode), torch.no_grad():
            up(xq.cuda())
        cal = ops.CALIBRATE
    finally:
        ops.CALIBRATE = None
    for owner, site, tot, n in cal.values():
        owner._md_act_ms = {site: (tot / n).contiguous()}
    wd = up.Conv_0.weight.detach().double().cpu()
    for name, xin in (("active", x), ("outlier1e6", x.clone().index_put_((torch.tensor([0]), torch.tensor([9]), torch.tensor([3]),
                                                                         torch.tensor([4]), torch.tensor([5])), torch.tensor(1e6)))):
        ops.PROFILE = []
        try:
            with ops.precision_scope(mode), torch.no_grad():
                y = up(xin.cuda()).cpu()
            tags = [r[5] for r in ops.PROFILE if r[0] == "wino"]
        finally:
            ops.PROFILE = None
        assert tags and all(t.endswith("/" + mode[3:]) for t in tags), tags
        ref = F.conv3d(F.interpolate(xin.double(), scale_factor=2, mode="nearest"), wd, padding=1)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(y).all()), f"{mode} {name}: non-finite output (R1)"
        e = rel_l2(y, ref)
        print(f"raw-stream equaliser, channel quiet at calibration, {name} ({mode}): vs torch fp64 {e:.2e}")
        if name == "active":
            assert e < TOL[mode]
    eq = up._md_cache["w/wino_eqm"][1].cpu()
    assert float(eq[5] / eq.median()) <= 2.0 ** 6          # the bound, seen from outside: not 2^13 x its neighbours


@pytest.mark.parametrize("mode", ["f16f8", "f16f6"])
def test_groupnorm_operand_dominant_voxel(ops, mode, monkeypatch):
    """One GroupNorm group holds a voxel at ~150 sigma (z ~ sqrt(N)): the 8|gamma| + |beta| headroom bound assumes |z| <= 8.  R1; the
    error is printed."""
    from meshdiffusion_amd.lib.diffusion.models import layers
    monkeypatch.setattr(ops, "WINO_MIN_WGS", 1)
    B, S, cin, cout = 1, 16, 128, 128
    gamma, beta = 1.0 + 0.2 * _rand((cin,), 641), 0.5 * _rand((cin,), 642)
    w = _rand((cout, cin, 3, 3, 3), 643, 0.05)
    x = _rand((B, cin, S, S, S), 644)
    x[0, 8, 4, 4, 4] = 150.0 * float(np.sqrt(4 * S ** 3))       # its group: 4 channels x 16^3
    pair = _pair(layers, cin, cout, gamma, beta, w)
    parts = [(ops.ncdhw_to_f32b(x.cuda()), cin)]
    _, ac = ops.gn_params(parts, pair.gn.weight, pair.gn.bias, B, S ** 3, want_ac=True)
    pw = layers.conv3_packed(pair, "w", pair.conv, ops.conv_cfg_for(S))
    with ops.precision_scope(mode):
        out = layers.run_conv3(pw, None, B, S, b_f32=ops.F32Operand(parts, ac, silu=True),
                               wino=layers.conv3_wino_packed(pair, "w", pair.conv, gn=pair.gn))
    y = ops.f32b_to_ncdhw(out, (S, S, S)).cpu()
    ref = F.conv3d(F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), eps=1e-6)), w.double(), padding=1)
    assert bool(torch.isfinite(y).all())
    print(f"GroupNorm group with a dominant voxel ({mode}): vs torch fp64 {rel_l2(y, ref):.2e}")


# ---- f16f6 data gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["w0", "odd"])
@pytest.mark.parametrize("val", list(VALUES))
@pytest.mark.parametrize("lift", ["dyn", "const64"])
def test_wino_data_gradient_f16f6_nonfinite_dy(ops, lift, val, place):
    """md_absmax + md_wino_prep_dual_f6 + md_conv3_wino_f6_scaled (as test_gpu_wino.test_conv3_wino_data_gradient_f16f6) with one
    non-finite element of dy: dx against torch.nn.grad.conv3d_input in float64.  The lift saturates finite values only."""
    B, S, ci, co = 2, 16, 128, 160
    w = _rand((co, ci, 3, 3, 3), 650, 0.05)
    dy = _rand((B, co, S, S, S), 651)
    b, _, wx = PLACES[place]
    dy[b, 40, 9, 2, wx] = VALUES[val]
    parts = [(ops.ncdhw_to_f32b(dy.cuda()), co)]
    amax = ops.absmax_word(parts[0][0]) if lift == "dyn" else None
    t, _ = ops.wino_prep(parts, None, False, False, B, S, dual=True, sums=None, f8="f6", tscale=64.0, amax=amax)
    ww = ops.WinoWeightF6Dgrad(w.cuda(), "cuda")
    dx = ops.f32b_to_ncdhw(ops.conv3_wino(ww, t, B, S, out_scale=1.0 if amax is not None else 1.0 / 64.0, amax=amax), (S, S, S)).cpu()
    ref = torch.nn.grad.conv3d_input((B, ci, S, S, S), w.double(), dy.double(), padding=1)
    e = _check_spread(dx, ref, 4e-5, f"f16f6 dgrad {lift} {val} at {place}")
    assert bool(torch.isfinite(dx[1 - b]).all())
    print(f"f16f6 data gradient, {val} in dy at {place}, lift {lift}: finite outputs vs torch fp64 {e:.2e}")


# ---- fused clip + Adam + EMA -----------------------------------------------------------------------------------------------------------
def _agree(mine, ref, what):
    mine, ref = mine.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.equal(torch.isnan(mine), torch.isnan(ref)), f"{what}: NaN pattern {int(torch.isnan(mine).sum())} vs {int(torch.isnan(ref).sum())}"
    ok = ~torch.isnan(ref)
    assert torch.equal(torch.isinf(mine[ok]), torch.isinf(ref[ok])), what
    fin = ok & torch.isfinite(ref)
    d = (mine[fin] - ref[fin]).abs()
    assert bool((d <= 1e-6 * ref[fin].abs().clamp_min(1.0)).all()), f"{what}: max diff {float(d.max()):.3e}"


@pytest.mark.parametrize("case", ["nan", "pinf", "huge1e20"])
def test_fused_clip_adam_ema_nonfinite_gradient(hip_lib, case):
    """FusedAdamEMA (md_grad_sqnorm + md_adam_ema_step) against torch's clip_grad_norm_ + Adam + EMA on the same device, one clean step
    then one whose gradient holds a NaN / +inf / 1e20 element: NaN at exactly torch's positions in p, m, v and the EMA shadows, the
    values elsewhere within 1e-6.  (torch: a NaN norm poisons every gradient; an inf norm -- also 1e20^2 in fp32 -- zeroes the finite
    ones and turns inf x 0 into NaN.)"""
    from meshdiffusion_amd.lib.diffusion.losses import FusedAdamEMA
    from meshdiffusion_amd.lib.diffusion.models.ema import ExponentialMovingAverage
    shapes = [(64, 32, 3, 3, 3), (64,), (257, 5), (1000,)]
    ref_p = [torch.nn.Parameter(_rand(s, 660 + i).cuda()) for i, s in enumerate(shapes)]
    my_p = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]
    opt = torch.optim.Adam(ref_p, lr=2e-5, betas=(0.9, 0.999), eps=1e-8)
    ema = ExponentialMovingAverage(ref_p, decay=0.9999)
    fused = FusedAdamEMA(my_p, lr=2e-5, grad_clip=1.0, warmup=5)
    bad = {"nan": float("nan"), "pinf": float("inf"), "huge1e20": 1e20}[case]
    for step in (1, 2):
        grads = [_rand(s, 670 + 10 * step + i).cuda() * 0.01 for i, s in enumerate(shapes)]
        if step == 2:
            grads[2][100, 3] = bad
        for p, q, g in zip(ref_p, my_p, grads):
            p.grad = g.clone()
            q.grad.copy_(g)
        for gr in opt.param_groups:
            gr["lr"] = 2e-5 * np.minimum(step / 5, 1.0)
        torch.nn.utils.clip_grad_norm_(ref_p, max_norm=1.0)
        opt.step()
        ema.update(ref_p)
        fused.step(step)
    for i, (p, q) in enumerate(zip(ref_p, my_p)):
        _agree(q, p, f"param {i}")
        st = opt.state[p]
        _agree(fused._views(fused.m)[i], st["exp_avg"], f"m {i}")
        _agree(fused._views(fused.v)[i], st["exp_avg_sq"], f"v {i}")
    for i, (mine, s) in enumerate(zip(fused.ema_shadow_params(), ema.shadow_params)):
        _agree(mine, s, f"ema {i}")
    n_nan = sum(int(torch.isnan(p).sum()) for p in ref_p)
    print(f"fused clip + Adam + EMA, {case} gradient element: torch's NaN parameters {n_nan}")


# ---- sampler step kernels --------------------------------------------------------------------------------------------------------------
B5 = (slice(None),) + (None,) * 4


def _same(a, b, what):
    assert torch.equal(_bad(a), _bad(b)), f"{what}: non-finite pattern {int(_bad(a).sum())} vs {int(_bad(b).sum())}"
    ok = ~_bad(b)
    assert torch.equal(a[ok], b[ok]), what


def _step_inputs(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, 4, R, R, R), generator=g).cuda() for _ in range(3)]


def test_ancestral_and_sde_steps_nan_score(hip_lib):
    """md_ancestral_step and md_sde_step (reverse diffusion, probability flow, Euler-Maruyama) with a NaN in one sample's score at a
    live voxel: the torch expressions of test_gpu_kernels / test_gpu_pc_sampler, bit for bit, NaN where they have NaN."""
    from meshdiffusion_amd import hip_ops as ops, synth
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from oracle import unet_oracle as uo
    B, R = 3, 16
    x, eps, z = _step_inputs(B, R, 680)
    mask = synth.synthetic_grid_mask(R).cuda()
    live = torch.nonzero(mask.reshape(-1) > 0).reshape(-1)[7].item()
    eps.view(B, 4, -1)[1, 2, live] = float("nan")
    x = x * mask
    t = torch.tensor(0.731)
    betas, _, sq1m = uo.vpsde_tables()
    k = (t * 999).long()
    coef = torch.stack([betas[k], sq1m[k], torch.sqrt(1.0 - betas[k]), torch.sqrt(betas[k])]).expand(B, 4).contiguous()
    xn, xm = ops.ancestral_step(x, eps, z, mask.reshape(-1).float().contiguous(), coef.cuda())
    rn, rm = uo.ancestral_step(x.cpu(), eps.cpu(), z.cpu(), t, mask.cpu())
    _same(xn.cpu(), rn, "ancestral x"); _same(xm.cpu(), rm, "ancestral x_mean")
    assert bool(torch.isfinite(xn[[0, 2]]).all())
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    ts = torch.linspace(1.0, 1e-3, 1000, device="cuda")
    idx = torch.tensor([10, 500, 990], device="cuda")
    for kind, pf in (("reverse_diffusion", False), ("reverse_diffusion", True), ("euler_maruyama", False)):
        pc, _ = sampling._pc_tables(sde, ts, 1, sampling.get_predictor(kind), sampling.NoneCorrector, 0.075, pf)
        cf = pc[idx, 0].contiguous()
        with torch.no_grad():
            xo, xmo = ops.sde_step(x, eps, z, mask.reshape(-1).float().contiguous(), cf, kind)
            c = [cf[:, j][B5] for j in range(5)]
            score = -eps / c[0]
            if kind == "reverse_diffusion":
                x_mean = x - ((c[1] * x - x) - c[2] * score * (0.5 if pf else 1.0))
            else:
                x_mean = x + (c[1] * x - c[2] * score * 1.0) * (-1.0 / 1000)
            xr = (x_mean + c[4] * z) * mask
            x_mean = x_mean * mask
        _same(xo, xr, f"{kind} pf={pf} x"); _same(xmo, x_mean, f"{kind} pf={pf} x_mean")
        assert bool(torch.isfinite(xo[[0, 2]]).all())


@pytest.mark.parametrize("mode", ["langevin", "ald"])
def test_langevin_nan_score(hip_lib, mode):
    """md_langevin_norms / md_langevin_step with a NaN in one sample's score: upstream's step size is a BATCH mean of the score norms,
    so Langevin poisons every sample (exactly as the torch expression does); ALD's per-sample table step keeps the others finite."""
    from meshdiffusion_amd import hip_ops as ops
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    B, R, snr = 3, 16, 0.16
    x, eps, z = _step_inputs(B, R, 690)
    eps[1, 0, 3, 4, 5] = float("nan")
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    ts = torch.linspace(1.0, 1e-3, 1000, device="cuda")
    _, cc = sampling._pc_tables(sde, ts, 1, sampling.AncestralSamplingPredictor, sampling.get_corrector(mode), snr, False)
    coef = cc[torch.tensor([20, 400, 800], device="cuda"), 0].contiguous()
    with torch.no_grad():
        xo, xmo, step = ops.langevin_step(x, eps, z, None, coef, snr, mode)
        sigma, alpha = coef[:, 0], coef[:, 1]
        if mode == "langevin":
            gn = (eps.double().reshape(B, -1).norm(dim=1) / sigma.double()).mean()
            nn_ = z.double().reshape(B, -1).norm(dim=1).mean()
            want = (snr * nn_ / gn) ** 2 * 2 * alpha.double()
            assert torch.equal(torch.isnan(step.cpu()), torch.isnan(want.cpu())) and bool(torch.isnan(step).all())
        else:
            assert torch.equal(step, coef[:, 2])
        score = -eps / sigma[B5]
        x_mean = x + step[B5] * score
        xr = x_mean + torch.sqrt(step * 2)[B5] * z
    _same(xo, xr, f"{mode} x"); _same(xmo, x_mean, f"{mode} x_mean")
    if mode == "langevin":
        assert bool(_bad(xo).all())
    else:
        assert bool(torch.isfinite(xo[[0, 2]]).all()) and int(_bad(xo[1]).sum()) == 1


# ---- marching tets ---------------------------------------------------------------------------------------------------------------------
def test_marching_tets_nonfinite_and_signed_zero_sdf(hip_lib, gold_dir):
    """NaN, +inf, -inf, +0.0 and -0.0 SDF values at chosen vertices (both ends of one edge included) against oracle.dmtet_oracle:
    faces and the face -> tet map bit-exact, vertices equal with NaN == NaN."""
    import os
    from meshdiffusion_amd.dmtet import DMTet
    from oracle import dmtet_oracle
    t = np.load(os.path.join(gold_dir, "64_tets_cropped.npz"))
    verts, idx = t["vertices"].astype(np.float32), t["indices"]
    n = len(verts)
    sdf = torch.randn(n, generator=torch.Generator().manual_seed(700)).numpy().astype(np.float32)
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    for j, v in enumerate(specials[:4]):                    # one tet with NaN, +inf, -inf, +0 at its four vertices
        sdf[idx[1000][j]] = v
    for j, v in enumerate(specials):                        # one special vertex in otherwise ordinary tets
        sdf[idx[3000 + 17 * j][1]] = v
    sdf[idx[2000][0]], sdf[idx[2000][1]] = np.inf, -np.inf  # both ends of one edge
    sdf[idx[4000][0]], sdf[idx[4000][2]] = np.nan, -0.0
    sdf[idx[5000][1]], sdf[idx[5000][3]] = 0.0, -np.inf
    v, f, _, _, ft, _ = DMTet()(torch.as_tensor(verts).cuda(), torch.as_tensor(sdf).cuda(), torch.as_tensor(idx, dtype=torch.long).cuda())
    vo, fo, fto = dmtet_oracle.marching_tets(verts, sdf, idx)
    assert np.array_equal(f.cpu().numpy(), fo) and np.array_equal(ft.cpu().numpy(), fto)
    assert np.array_equal(v.cpu().numpy(), vo, equal_nan=True)
    print(f"marching tets with non-finite / signed-zero SDFs: V={len(vo)} F={len(fo)}, non-finite vertices {int((~np.isfinite(vo)).any(1).sum())}")


# ---- dispatch: a calibrated raw stream without its equaliser stays in bf16x3 ------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f8", "f6"])
def test_measured_operand_without_equaliser_stays_bf16x3(ops, fmt, monkeypatch):
    """MD_WINO_EQ=0 (hip_ops.WINO_EQ False): a calibrated Upsample conv has no equaliser to put its raw operand at unit scale, so the
    measurement alone must not move it onto the reduced-precision path: a 1e-5 stream would go subnormal in fp16."""
    from meshdiffusion_amd.lib.diffusion.models import layers
    monkeypatch.setattr(ops, "WINO_MIN_WGS", 1)
    B, S, cin, cout = 1, 16, 128, 128
    x = _rand((B, cin, S // 2, S // 2, S // 2), 710) * 1e-5
    up = layers.Upsample(cin, with_conv=True)
    with torch.no_grad():
        up.Conv_0.weight.copy_(_rand((cout, cin, 3, 3, 3), 711, 0.05)); up.Conv_0.bias.zero_()
    up = up.cuda().eval()
    ops.CALIBRATE = {}
    try:
        with ops.precision_scope("f16" + fmt), torch.no_grad():
            up(x.cuda())
        cal = ops.CALIBRATE
    finally:
        ops.CALIBRATE = None
    for owner, site, tot, n in cal.values():
        owner._md_act_ms = {site: (tot / n).contiguous()}
    monkeypatch.setattr(ops, "WINO_EQ", False)
    ops.PROFILE = []
    try:
        with ops.precision_scope("f16" + fmt), torch.no_grad():
            y = up(x.cuda()).cpu()
        tags = [r[5] for r in ops.PROFILE if r[0] in ("wino", "wino_prep")]
    finally:
        ops.PROFILE = None
    assert tags and all("/f" not in t for t in tags), tags
    ref = F.conv3d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), up.Conv_0.weight.detach().double().cpu(), padding=1)
    e = rel_l2(y, ref)
    print(f"calibrated raw 1e-5 operand, MD_WINO_EQ=0, f16{fmt} scope: {e:.2e} ({tags})")
    assert e < TOL_MFMA
