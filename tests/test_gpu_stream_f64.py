"""The streaming kernels on their own, against float64, at their edges: GroupNorm (csrc/norm.hip), the training step
(csrc/train.hip) and the small kernels of csrc/elementwise.hip: dense layer, timestep embedding, layout conversion (the sampler
updates are in csrc/sde_steps.hip and have their own tests).

Everything is called through hip_ops, losses and _lib.load().  Inputs, float64 references and the bounds live in
tests/stream_cases.py; every bound is derived by counting the roundings of the kernel source (its docstring has the count),
none is a blanket tolerance.  tests/test_cpu_stream_cases.py proves without a GPU that an emulation of each kernel lies inside
these bounds and that the usual one-line mistakes land at least 4x outside.  Every case prints what it measured next to its bound.

  GroupNorm (B, parts, grid)     owns
  1 (32,)     4x4x4              cpg = 1, one block
  3 (96,)     5x6x7              cpg = 3 straddles 8-channel blocks, odd P, odd batch; mean/std 0, 4, 8, 64; channel means; constant group
  2 (40, 56)  3x3x5              part boundary inside group 13, per-part c_off
  1 (64,)     P = 2047/2048/2049 the edge of the 2048-position chunk
  1 (32,)     4x25x41            three blocks adding onto one double; mean/std 0, 4, 8, 64; constant group
  1 (2080,)   2x2x2              cpg = 65: the strided loop of md_gn_finalize

Measured on an MI355X: see DESIGN.md, "Direct tests of the streaming kernels".
Non-finite inputs to these kernels stay with tests/test_gpu_nonfinite.py.
"""
import math

import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu

GN_CASES = sc.gn_cases()


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def lib(hip_lib):
    from meshdiffusion_amd import _lib
    return _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------
def _gn_parts(case):
    return [(sc.to_f32b(t).cuda(), c) for t, c in zip(torch.split(case["x"], list(case["parts"]), 1), case["parts"])]


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: c["name"])
def test_groupnorm_vs_float64(ops, case):
    B, C, P = case["B"], case["C"], case["P"]
    parts = _gn_parts(case)
    params, ac = ops.gn_params(parts, case["gamma"].cuda(), case["beta"].cuda(), B, P, eps=sc.GN_EPS, groups=sc.GN_GROUPS, want_ac=True)
    params, ac = params.cpu(), ac.cpu()
    pb = sc.gn_param_bounds(case)
    ref = sc.gn_reference(case, False)
    got = dict(mean=params[..., 0], a=params[..., 1], rstd=params[..., 3], c=ac[..., 1])
    for k in ("mean", "a", "rstd", "c"):
        err = (got[k].double() - ref[k]).abs()
        print(f"{case['name']} {k}: max err {float(err.max()):.3e}, worst err/bound {float((err / pb[k].clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= pb[k]).all()), k
    assert torch.equal(params[..., 2], case["beta"][None].expand(B, C))
    assert torch.equal(ac[..., 0], params[..., 1])
    x5 = case["x"].reshape(B, C, *case["grid"])
    raw_ref = ops.ncdhw_to_s16b(x5.cuda(), C).cpu()
    for norm in (True, False):
        for silu in (False, True):
            out, raw = ops.gn_apply(parts, params.cuda() if norm else None, B, P, norm=norm, silu=silu, want_raw=True)
            hi, lo = sc.from_s16b(out.cpu())
            ref64 = sc.gn_reference(case, silu, norm)["out"]
            bound = sc.gn_bound(case, silu, norm)
            rel, worst = sc.gn_measure(hi.double() + lo.double(), ref64, bound)
            t32 = torch.nn.functional.group_norm(case["x"], sc.GN_GROUPS, case["gamma"], case["beta"], sc.GN_EPS) if norm else case["x"]
            t32 = torch.nn.functional.silu(t32) if silu else t32
            rel32, _ = sc.gn_measure(t32.double(), ref64, bound)
            print(f"{case['name']} norm={int(norm)} silu={int(silu)}: elementwise {rel:.3e} (torch fp32 {rel32:.3e}), worst err/bound {worst:.3f}")
            assert worst <= 1.0
            if norm and case["ratio"] == sc.GN_SERVED_RATIO:
                assert rel <= sc.GN_SERVED_TOL
            assert torch.equal(_bits(raw.cpu()), _bits(raw_ref))


def test_groupnorm_entry_points_reject_bad_arguments(lib):
    t = torch.zeros(1 << 14, device="cuda")
    p = t.data_ptr()
    st = lambda *a: lib.md_gn_stats(*a, None)
    assert st(None, p, 1, 8, 64, 8, 0) != 0 and st(p, None, 1, 8, 64, 8, 0) != 0                  # x, sums
    assert st(p, p, 0, 8, 64, 8, 0) != 0 and st(p, p, 1, 0, 64, 8, 0) != 0                         # batch, C
    assert st(p, p, 1, 12, 64, 12, 0) != 0 and st(p, p, 1, 8, 0, 8, 0) != 0                        # C % 8, P
    assert st(p, p, 1, 8, 64, 16, -8) != 0 and st(p, p, 1, 8, 64, 8, 8) != 0                       # c_off < 0, c_off + C > c_total
    fin = lambda *a: lib.md_gn_finalize(*a, None)
    assert fin(None, p, p, p, 1, 32, 32, 64, 1e-6, None) != 0 and fin(p, None, p, p, 1, 32, 32, 64, 1e-6, None) != 0
    assert fin(p, p, None, p, 1, 32, 32, 64, 1e-6, None) != 0 and fin(p, p, p, None, 1, 32, 32, 64, 1e-6, None) != 0
    assert fin(p, p, p, p, 0, 32, 32, 64, 1e-6, None) != 0 and fin(p, p, p, p, 1, 32, 0, 64, 1e-6, None) != 0
    assert fin(p, p, p, p, 1, 40, 32, 64, 1e-6, None) != 0                                         # c_total % groups
    assert fin(p, p, p, p, 1, 0, 32, 64, 1e-6, None) != 0 and fin(p, p, p, p, 1, 32, 32, 0, 1e-6, None) != 0   # c_total, P
    ap = lambda *a: lib.md_gn_apply(*a, None)
    ok = (p, p + (1 << 14), p + (1 << 15), None, 1, 8, 64, 8, 0, 1, 1, 0.0, 0)       # x, params and out apart: this one launches
    assert ap(*ok) == 0
    torch.cuda.synchronize()

    def bad(**kw):
        names = ("x", "params", "out", "raw", "batch", "C", "P", "c_total", "c_off", "norm", "silu", "drop_p", "seed")
        a = dict(zip(names, ok)); a.update(kw)
        return ap(*[a[n] for n in names]) != 0
    assert bad(drop_p=-0.1) and bad(drop_p=1.0) and bad(drop_p=float("nan"))
    assert bad(x=None) and bad(out=None) and bad(params=None) and not bad(params=None, norm=0)
    assert bad(batch=0) and bad(C=0) and bad(C=12, c_total=16) and bad(c_off=4, c_total=16) and bad(c_total=12)
    assert bad(c_off=8) and bad(c_off=-8, c_total=16) and bad(P=0)
    torch.cuda.synchronize()


def test_groupnorm_dropout_is_the_mask_times_the_plain_output(ops):
    """drop = (p, seed): bit for bit the output without dropout times md_dropout_scale's mask (p = 0.5: the factor 2 is exact in
    both planes), and the kept fraction is the threshold's, within 5 binomial sigma."""
    case = next(c for c in GN_CASES if c["name"] == "P210-ratio0")
    B, C, P = case["B"], case["C"], case["P"]
    parts = _gn_parts(case)
    params = ops.gn_params(parts, case["gamma"].cuda(), case["beta"].cuda(), B, P, eps=sc.GN_EPS, groups=sc.GN_GROUPS)
    plain = ops.gn_apply(parts, params, B, P, norm=True, silu=True).cpu()
    seed = 0x1234567890ABCDE
    scale = ops.dropout_scale(B, C, P, 0.5, seed, "cuda").cpu()                    # F32B [B][C/8][P][8]
    assert set(scale.unique().tolist()) == {0.0, 2.0}
    got = ops.gn_apply(parts, params, B, P, norm=True, silu=True, drop=(0.5, seed)).cpu()
    keep = (scale != 0)[:, :, None].expand_as(plain)
    want = torch.where(keep, plain.float() * 2.0, torch.zeros(())).to(torch.bfloat16)
    assert torch.equal(_bits(got), _bits(want))
    for p in (0.5, 0.1):
        thr16 = int(sc.f32(p) * 65536.0 + 0.5)
        q = 1.0 - thr16 / 65536.0
        m = ops.dropout_scale(B, C, P, p, seed + 1, "cuda")
        kept, n = float((m != 0).double().mean()), m.numel()
        sigma = math.sqrt(q * (1 - q) / n)
        print(f"dropout p={p}: kept {kept:.5f}, expected {q:.5f}, {abs(kept - q) / sigma:.2f} sigma of {n}")
        assert abs(kept - q) <= 5 * sigma


# ---------------------------------------------------------------------------------------------------------------
# md_ddpm_perturb, md_masked_sq_err, md_grad_sqnorm
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sde(hip_lib):
    from meshdiffusion_amd.lib.diffusion import sde_lib
    return sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")


@pytest.mark.parametrize("B,C,grid,masked", [(3, 1, (6, 10, 14), True), (3, 5, (6, 10, 14), True), (3, 5, (6, 10, 14), False),
                                             (1, 4, (64, 64, 132), True)])
def test_perturb_bit_exact(sde, B, C, grid, masked):
    from meshdiffusion_amd.lib.diffusion import losses
    g = torch.Generator().manual_seed(60 + C)
    x0, noise = torch.randn(B, C, *grid, generator=g), torch.randn(B, C, *grid, generator=g)
    mask = (torch.rand(1, 1, *grid, generator=g) < 0.3).float() if masked else None
    labels = torch.tensor([0, 417, 999][:B]) if B == 3 else torch.tensor([417])
    xt = losses.ddpm_perturb(sde, x0.cuda(), labels.cuda(), noise.cuda(), mask.reshape(-1).cuda() if masked else None).cpu()
    sa, s1 = sde.sqrt_alphas_cumprod.cpu(), sde.sqrt_1m_alphas_cumprod.cpu()
    ref = sa[labels, None, None, None, None] * x0 + s1[labels, None, None, None, None] * noise
    ref = ref * mask if masked else ref
    if C * grid[0] * grid[1] * grid[2] > 2048 * 256 * 4:
        print("perturb: the grid-stride loop takes a second trip")
    assert torch.equal(xt, ref)


def test_perturb_rejects_positions_not_in_fours(sde):
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.lib.diffusion import losses
    x = torch.zeros(1, 4, 3, 3, 5, device="cuda")
    with pytest.raises(_lib.MeshDiffusionHipError):
        losses.ddpm_perturb(sde, x, torch.tensor([5], device="cuda"), x, None)
    with pytest.raises(_lib.MeshDiffusionHipError):
        losses.masked_sq_err(x, x, None)


@pytest.mark.parametrize("case", sc.sq_err_cases(), ids=lambda c: c["name"])
def test_masked_sq_err_vs_float64(ops, lib, case):
    from meshdiffusion_amd.lib.diffusion import losses
    ref, bound, gref = sc.sq_err_reference(case)
    eh, noise = case["eps_hat"].cuda(), case["noise"].cuda()
    mask = case["mask"].cuda() if case["mask"] is not None else None
    sums = case["sums0"].clone().cuda()
    grad = torch.empty_like(eh)
    rc = lib.md_masked_sq_err(ops._ptr(eh), ops._ptr(noise), ops._ptr(mask), ops._ptr(sums), ops._ptr(grad), case["gscale"],
                              case["B"], case["C"], case["P"], ops._stream())
    assert rc == 0
    err = (sums.cpu() - ref).abs()
    print(f"sq_err {case['name']}: worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, "
          f"rel {float((err / ref.abs().clamp_min(1e-300)).max()):.2e}")
    assert bool((err <= bound).all())
    assert sc.ulp_distance(grad.cpu(), gref) <= 1
    if case["name"] == "zero-mask":
        assert float(sums.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0
    if float(case["sums0"].abs().max()) == 0.0:                      # the wrapper zeroes `sums` itself and may skip the gradient
        s2, g2 = losses.masked_sq_err(eh, noise, mask, want_grad=False)
        assert g2 is None and bool(((s2.cpu() - ref).abs() <= bound).all())


@pytest.mark.parametrize("n,scale,mixed", sc.sqnorm_params())
def test_grad_sqnorm_vs_float64(ops, lib, n, scale, mixed):
    case = sc.sqnorm_case(n, scale, mixed=mixed)
    ref, bound = sc.sqnorm_reference(case)
    g = case["g"].cuda()
    out = torch.tensor([case["out0"]], dtype=torch.float64, device="cuda")
    assert lib.md_grad_sqnorm(ops._ptr(g), n, ops._ptr(out), ops._stream()) == 0
    err = abs(float(out) - ref)
    print(f"sqnorm n={n} scale={scale} mixed={mixed}: err/bound {err / bound:.3f}, rel {err / ref:.2e}")
    assert err <= bound


# ---------------------------------------------------------------------------------------------------------------
# md_adam_ema_step_d
# ---------------------------------------------------------------------------------------------------------------
def _adam_step(ops, lib, case, entry="md_adam_ema_step_d"):
    """One launch on copies of the case's state; returns (p, m, v, ema) on the host."""
    p, g, m, v = (case[k].clone().cuda() for k in ("p", "g", "m", "v"))
    s = case["ema"].clone().cuda() if case["ema"] is not None else None
    sq = torch.tensor([case["sq"]], dtype=torch.float64, device="cuda") if case["sq"] is not None else None
    hp = [case[k] for k in ("lr", "b1", "b2", "eps", "wd")]
    d = case["d"]
    if entry == "md_adam_ema_step":
        hp, d = [sc.f32(x) for x in hp], sc.f32(d)
    rc = getattr(lib, entry)(ops._ptr(p), ops._ptr(g), ops._ptr(m), ops._ptr(v), ops._ptr(s), case["n"], *hp, case["step"], d,
                             ops._ptr(sq), case["max_norm"], ops._stream())
    assert rc == 0
    return p.cpu(), m.cpu(), v.cpu(), s.cpu() if s is not None else None


def _ema_fp32(case, p_new):
    """models/ema.py `update` in fp32 on the host, from the parameters the kernel produced."""
    rate = torch.tensor(1.0 - case["d"], dtype=torch.float32)      # the double 1.0 - d, rounded once
    return case["ema"] - rate * (case["ema"] - p_new)


@pytest.mark.parametrize("case", sc.adam_cases(), ids=lambda c: c["name"])
def test_adam_ema_step_vs_float64(ops, lib, case):
    ref = sc.adam_reference(case)
    got = _adam_step(ops, lib, case)
    w = sc.adam_worst(got, case, ref)
    print(f"adam {case['name']}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert max(w.values()) <= 1.0, w
    if case["ema"] is not None:
        assert sc.ulp_distance(got[3], _ema_fp32(case, got[0])) <= 1
    else:
        assert got[3] is None


def test_adam_ema_three_steps_carry_state(ops, lib):
    case = sc.adam_case("carry", 257, 1, wd=0.01, clip="over", d=0.9999)
    for step in (1, 2, 3):
        case = dict(case, step=step, d=sc.ema_decay(0.9999, step))
        ref = sc.adam_reference(case)
        p, m, v, s = _adam_step(ops, lib, case)
        w = sc.adam_worst((p, m, v, s), case, ref)
        print(f"adam carry step {step}: " + ", ".join(f"{k} {x:.3f}" for k, x in w.items()))
        assert max(w.values()) <= 1.0, w
        g = torch.randn(257, generator=torch.Generator().manual_seed(900 + step)) * 0.0631
        case = dict(case, p=p, m=m, v=v, ema=s, g=g, sq=float((g.double() ** 2).sum()))


def test_adam_float_entry_point_is_the_double_one_on_widened_floats(ops, lib):
    """md_adam_ema_step (ABI 16) stays: it forwards its floats widened, so it is md_adam_ema_step_d for hyper-parameters that ARE
    floats -- and, unlike it, not the reference's step for a decay such as 0.9999 that is not one."""
    case = next(c for c in sc.adam_cases() if c["name"] == "d0.9999")
    widened = dict(case, **{k: sc.f32(case[k]) for k in ("lr", "b1", "b2", "eps", "wd", "d")})
    old, new = _adam_step(ops, lib, case, entry="md_adam_ema_step"), _adam_step(ops, lib, widened)
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    assert sc.ulp_distance(old[3], _ema_fp32(case, old[0])) > 1


# ---------------------------------------------------------------------------------------------------------------
# md_linear, md_timestep_embedding, md_ncdhw_to_s16b
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.linear_cases(), ids=lambda c: c["name"])
def test_linear_vs_float64(ops, case):
    ref, _ = sc.linear_reference(case)
    bound = sc.linear_bound(case)
    y = ops.linear(case["x"].cuda(), case["w"].cuda(), case["bias"].cuda() if case["bias"] is not None else None, silu_in=case["silu"]).cpu()
    err = (y.double() - ref).abs()
    print(f"linear {case['name']}: max err {float(err.max()):.3e}, worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dim", sc.TEMB_DIMS)
def test_timestep_embedding_vs_float64(ops, dim):
    ref, bound = sc.temb_reference(dim)
    emb = ops.timestep_embedding(torch.tensor(sc.TEMB_T).cuda(), dim).cpu()
    err = (emb.double() - ref).abs()
    live = bound > 0
    print(f"temb dim={dim}: max err {float(err.max()):.3e}, worst err/bound {float((err[live] / bound[live]).max()):.3f}")
    assert bool((err <= bound).all())
    if dim % 2:
        assert torch.equal(emb[:, -1], torch.zeros(len(sc.TEMB_T)))


@pytest.mark.parametrize("C,c_pad", sc.S16B_CASES)
def test_ncdhw_to_s16b_bit_exact(ops, C, c_pad):
    x = torch.randn(2, C, 5, 6, 7, generator=torch.Generator().manual_seed(80 + C))
    hi, lo = sc.from_s16b(ops.ncdhw_to_s16b(x.cuda(), c_pad).cpu())
    rhi, rlo = sc.split_bf16(x.reshape(2, C, 210))
    assert torch.equal(_bits(hi[:, :C]), _bits(rhi)) and torch.equal(_bits(lo[:, :C]), _bits(rlo))
    assert int(_bits(hi[:, C:]).abs().max()) == 0 and int(_bits(lo[:, C:]).abs().max()) == 0      # pad channels: +0 in both planes
