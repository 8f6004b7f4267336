"""The streaming kernels of the backward pass (csrc/backward.hip) on their own, against float64 on the CPU.

Until now they were only seen through ResnetBlock / AttnBlock gradients at 2e-4, where the bf16x3 contractions around
them set the tolerance.  Here every reference is fed the SAME fp32 parameters the kernel reads (for GroupNorm the
(mu, a, beta, rstd) rows of hip_ops.gn_params, copied to the host), so it isolates the kernel: fp32 streaming kernels
meet TOL_F32 = 2e-6 rel-L2 and 1e-5 on the elementwise measure max |got - ref| / max |ref|; layout kernels are bit-exact.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL_F32 = 2e-6          # tests/test_gpu_kernels.py
TOL_ELEM = 1e-5


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def bw(ops):
    from meshdiffusion_amd.lib.diffusion.models import backward
    return backward


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _elem(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _close(got, ref, what, tol_l2=TOL_F32, tol_elem=TOL_ELEM):
    e2, ee = rel_l2(got, ref), _elem(got, ref)
    print(f"  {what}: rel-L2 {e2:.2e} elementwise {ee:.2e}")
    assert e2 <= tol_l2 and ee <= tol_elem, (what, e2, ee)


def _f32b(ops, x5):
    return ops.ncdhw_to_f32b(x5.cuda())


def _from_f32b(ops, t, shape):
    return ops.f32b_to_ncdhw(t, shape).cpu()


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm (+ SiLU) backward
# ---------------------------------------------------------------------------------------------------------------
def _gn_ref(x, dy, params, gamma, groups, silu, mask=None):
    """float64 GroupNorm(+SiLU) backward from the kernel's own fp32 (mu, a, beta, rstd): x, dy [B][C][P]."""
    x, dy, gamma = x.double(), dy.double(), gamma.double()
    mu, a, bt, r = (params[..., i].double()[:, :, None] for i in range(4))
    B, C, P = x.shape
    xc = x - mu
    xhat = xc * r
    z = xc * a + bt
    if mask is not None:
        dy = dy * mask.double()
    if silu:
        s = torch.sigmoid(z)
        dz = dy * s * (1 + z * (1 - s))
    else:
        dz = dy
    S1, S2 = dz.sum(2), (dz * xhat).sum(2)                                 # [B][C]
    cpg = C // groups
    G1 = (gamma[None] * S1).view(B, groups, cpg).sum(2).repeat_interleave(cpg, 1)
    G2 = (gamma[None] * S2).view(B, groups, cpg).sum(2).repeat_interleave(cpg, 1)
    n = cpg * P
    dx = (r * gamma[None, :, None]) * dz - (r[:, :, 0] * G1 / n)[:, :, None] - xhat * (r[:, :, 0] * G2 / n)[:, :, None]
    return dx, S2.sum(0), S1.sum(0)


def test_gn_reference_formula_is_autograd_of_group_norm():
    """The float64 formula above, fed exact float64 statistics, IS torch autograd of group_norm (+ SiLU)."""
    B, C, P, groups = 2, 64, 96, 32
    x, dy = _randn((B, C, P), 1, torch.float64) * 2 + 0.5, _randn((B, C, P), 2, torch.float64) + 0.3
    gamma, beta = 1 + 0.3 * _randn((C,), 3, torch.float64), 0.2 * _randn((C,), 4, torch.float64)
    eps = 1e-6
    xg = x.view(B, groups, -1)
    mu = xg.mean(2).repeat_interleave(C // groups, 1)
    r = (xg.var(2, unbiased=False) + eps).rsqrt().repeat_interleave(C // groups, 1)
    params = torch.stack([mu, r * gamma[None], beta[None].expand(B, C), r], 2)
    for silu in (False, True):
        xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = F.group_norm(xr, groups, gr, br, eps=eps)
        (F.silu(y) if silu else y).backward(dy)
        dx, dg, db = _gn_ref(x, dy, params, gamma, groups, silu)
        assert _elem(dx, xr.grad) < 1e-11 and _elem(dg, gr.grad) < 1e-11 and _elem(db, br.grad) < 1e-11


def _gn_inputs(kind, B, C, P, seed):
    x = _randn((B, C, P), seed) * 1.5 + 0.3
    dy = _randn((B, C, P), seed + 1)
    gamma, beta = 1 + 0.2 * _randn((C,), seed + 2), 0.1 * _randn((C,), seed + 3)
    if kind == "mean50":            # x - mu cancels
        x = 50 + 0.1 * _randn((B, C, P), seed)
    elif kind == "const_group":     # group 1 nearly constant: rstd near eps^-1/2 = 1000
        cpg = C // 32
        x[:, cpg:2 * cpg] = 3.0 + 1e-4 * _randn((B, cpg, P), seed + 4)
    elif kind == "dy_mean":         # the k2 term matters
        dy = dy + 2.0
    elif kind == "bigz":            # |z| up to ~30 for md_silu_grad
        gamma = 8 * gamma
    else:
        assert kind == "randn"
    return x, dy, gamma, beta


def _gn_module(C, gamma, beta):
    gn = torch.nn.GroupNorm(32, C, eps=1e-6).cuda()
    with torch.no_grad():
        gn.weight.copy_(gamma); gn.bias.copy_(beta)
    return gn


GN_CASES = [
    # kind, B, parts, grid, silu
    ("randn", 1, (32,), (4, 4, 4), True),
    ("dy_mean", 3, (128,), (8, 8, 8), False),
    ("mean50", 1, (256,), (16, 16, 16), True),
    ("bigz", 3, (64, 64), (12, 12, 12), True),
    ("const_group", 1, (128, 128), (8, 8, 8), False),
    ("randn", 3, (16, 16), (4, 4, 4), True),
    ("dy_mean", 1, (128,), (12, 12, 12), True),
    ("mean50", 3, (96, 32), (8, 8, 8), False),
    ("const_group", 3, (256,), (4, 4, 4), True),
    ("bigz", 1, (32,), (16, 16, 16), True),
]


@pytest.mark.parametrize("kind,B,cparts,grid,silu", GN_CASES)
def test_gn_backward(ops, bw, kind, B, cparts, grid, silu):
    """md_gn_bwd_stats -> md_gn_bwd_finalize -> md_gn_bwd_apply through backward.gn_backward: one part and two parts
    (c_off, dy_ctotal), 1 / 4 / 8 channels per group, P = 64, 512, 1728 (not a multiple of the 2048-position chunk), 4096."""
    C, P = sum(cparts), grid[0] * grid[1] * grid[2]
    x, dy, gamma, beta = _gn_inputs(kind, B, C, P, 100 + C + P)
    xs = torch.split(x, list(cparts), 1)
    parts = [(_f32b(ops, t.reshape(B, c, *grid)), c) for t, c in zip(xs, cparts)]
    gn = _gn_module(C, gamma, beta)
    params = ops.gn_params(parts, gn.weight, gn.bias, B, P, eps=gn.eps, groups=32)
    g0, b0 = _randn((C,), 7), _randn((C,), 8)           # the parameter gradients ACCUMULATE: start from non-zero
    gn.weight.grad, gn.bias.grad = g0.clone().cuda(), b0.clone().cuda()
    outs = bw.gn_backward(parts, _f32b(ops, dy.reshape(B, C, *grid)), params, gn, B, P, silu)
    got = torch.cat([_from_f32b(ops, o, grid).reshape(B, c, P) for o, c in zip(outs, cparts)], 1)
    ref, dg, db = _gn_ref(x, dy, params.cpu(), gamma, 32, silu)
    print(f"gn_backward {kind} B={B} C={cparts} P={P} silu={silu}: max rstd {float(params[..., 3].max()):.1f}")
    _close(got, ref, "dx")
    _close(gn.weight.grad.cpu(), g0.double() + dg, "dgamma")
    _close(gn.bias.grad.cpu(), b0.double() + db, "dbeta")
    if kind == "randn":     # ... and the formula with the kernel's fp32 statistics is autograd of group_norm to fp32 statistics' accuracy
        xr = x.double().requires_grad_(True)
        y = F.group_norm(xr, 32, gamma.double(), beta.double(), eps=1e-6)
        (F.silu(y) if silu else y).backward(dy.double())
        assert _elem(got, xr.grad) < 1e-5


@pytest.mark.parametrize("two_parts", [False, True])
def test_gn_backward_accumulate(ops, bw, two_parts):
    B, grid, silu = 3, (8, 8, 8), True
    cparts = (64, 64) if two_parts else (128,)
    C, P = sum(cparts), 512
    x, dy, gamma, beta = _gn_inputs("dy_mean", B, C, P, 31)
    prev = _randn((B, C, P), 32) * 3 + 1
    parts = [(_f32b(ops, t.reshape(B, c, *grid)), c) for t, c in zip(torch.split(x, list(cparts), 1), cparts)]
    gn = _gn_module(C, gamma, beta)
    params = ops.gn_params(parts, gn.weight, gn.bias, B, P, eps=gn.eps, groups=32)
    outs = bw.gn_backward(parts, _f32b(ops, dy.reshape(B, C, *grid)), params, gn, B, P, silu,
                          d_into=_f32b(ops, prev.reshape(B, C, *grid)))
    got = torch.cat([_from_f32b(ops, o, grid).reshape(B, -1, P) for o in outs], 1)
    ref, _, _ = _gn_ref(x, dy, params.cpu(), gamma, 32, silu)
    _close(got, prev.double() + ref, "accumulated dx")
    _close(got.double() - prev.double(), ref, "the added part")


@pytest.mark.parametrize("B,C,grid,with_res", [(3, 128, (8, 8, 8), True), (1, 32, (12, 12, 12), False), (1, 256, (16, 16, 16), True),
                                               (3, 256, (12, 12, 12), False)])
def test_gn_backward_residual_sums_amax(ops, bw, B, C, grid, with_res):
    """residual (identity shortcut: result = residual + gradient), ch_sums and amax_bits (max |.| of the RETURNED tensor,
    bit-exact: it is a max, not a sum).
    ch_sums are the per-(sample, channel) sums of the GRADIENT (backward.gn_backward's contract: the producer's bias / FiLM
    gradient); without a residual that is the returned tensor, with one it is the returned tensor minus the residual (the
    training path never combines the two).  dy carries a per-channel offset so that the sums of channels that share a group do not
    cancel and TOL_F32 means something; with one channel per group (C = 32) every exact sum is 0 and only the bound derived from the
    summation applies: (16 serial adds + 5 shuffles + 4 waves x P / 2048 chunks of atomics + 1) * 2^-24 * sum_p |g| per entry."""
    P = grid[0] * grid[1] * grid[2]
    x, dy, gamma, beta = _gn_inputs("randn", B, C, P, 41)
    dy = dy + (torch.arange(C) % 8).float()[None, :, None] * 0.5
    res = _randn((B, C, P), 42) + 0.5 if with_res else None
    parts = [(_f32b(ops, x.reshape(B, C, *grid)), C)]
    gn = _gn_module(C, gamma, beta)
    params = ops.gn_params(parts, gn.weight, gn.bias, B, P, eps=gn.eps, groups=32)
    sums0 = _randn((B, C), 43)
    sums = sums0.clone().cuda()
    out = bw.gn_backward(parts, _f32b(ops, dy.reshape(B, C, *grid)), params, gn, B, P, True,
                         residual=_f32b(ops, res.reshape(B, C, *grid)) if with_res else None, sums_out=sums, want_amax=True)[0]
    got = _from_f32b(ops, out, grid).reshape(B, C, P)
    ref, _, _ = _gn_ref(x, dy, params.cpu(), gamma, 32, True)
    _close(got, ref + (res.double() if with_res else 0), "dx (+ residual)")
    grad_sums = ref.sum(2) if with_res else got.double().sum(2)
    added = sums.cpu().double() - sums0.double()
    depth = 16 + 5 + 4 * ((P + 2047) // 2048) + 1
    bound = depth * 2.0 ** -24 * (ref.abs().sum(2) + sums0.abs().double())
    worst = float(((added - grad_sums).abs() / bound).max())
    print(f"  ch_sums: largest error / summation bound {worst:.3f}")
    assert worst <= 1.0
    if C > 32:
        _close(added, grad_sums, "ch_sums")
    word = out._md_amax.cpu().view(torch.float32)
    assert float(word) == float(got.abs().max()), (float(word), float(got.abs().max()))


@pytest.mark.parametrize("p,two_parts", [(0.1, False), (0.5, True)])
def test_gn_backward_dropout_gate(ops, bw, p, two_parts):
    """dropout (p, seed): the gate is the mask hip_ops.dropout_scale returns for the same seed."""
    B, grid, silu, seed = 2, (8, 8, 8), True, 0x1234567890ABCDE
    cparts = (64, 64) if two_parts else (128,)
    C, P = sum(cparts), 512
    x, dy, gamma, beta = _gn_inputs("dy_mean", B, C, P, 51)
    parts = [(_f32b(ops, t.reshape(B, c, *grid)), c) for t, c in zip(torch.split(x, list(cparts), 1), cparts)]
    gn = _gn_module(C, gamma, beta)
    params = ops.gn_params(parts, gn.weight, gn.bias, B, P, eps=gn.eps, groups=32)
    mask = _from_f32b(ops, ops.dropout_scale(B, C, P, p, seed, "cuda"), grid).reshape(B, C, P)
    kept = float((mask != 0).double().mean())
    assert abs(kept - (1 - p)) < 0.01 and set(mask.unique().tolist()) == {0.0, float(torch.tensor(1.0) / (torch.tensor(1.0) - p))}
    outs = bw.gn_backward(parts, _f32b(ops, dy.reshape(B, C, *grid)), params, gn, B, P, silu, drop=(p, seed))
    got = torch.cat([_from_f32b(ops, o, grid).reshape(B, -1, P) for o in outs], 1)
    ref, dg, db = _gn_ref(x, dy, params.cpu(), gamma, 32, silu, mask=mask)
    _close(got, ref, f"dx with dropout p={p}")
    _close(gn.weight.grad.cpu(), dg, "dgamma")
    _close(gn.bias.grad.cpu(), db, "dbeta")


def test_gn_backward_entry_points_reject_bad_arguments(ops):
    from meshdiffusion_amd import _lib
    lib = _lib.load()
    t = torch.zeros(1 << 14, device="cuda")
    p = t.data_ptr()
    assert lib.md_gn_bwd_stats(p, p, p, p, 1, 12, 64, 12, 0, 12, 1, 0.0, 0, None) != 0            # C % 8
    assert lib.md_gn_bwd_stats(p, p, p, p, 1, 16, 64, 16, 8, 16, 1, 0.0, 0, None) != 0            # c_off + C > c_total
    assert lib.md_gn_bwd_stats(p, p, p, p, 1, 16, 64, 16, 0, 16, 1, 1.0, 0, None) != 0            # p = 1
    assert lib.md_gn_bwd_apply(p, p, p, p, p, 1, 16, 64, 16, 4, 16, 1, 0, 0.0, 0, None, None, None, None) != 0   # c_off % 8
    assert lib.md_gn_bwd_finalize(p, p, p, p, None, None, 1, 30, 32, 64, None) != 0               # c_total % groups
    assert lib.md_channel_sums(p, p, 1, 12, 64, None) != 0
    assert lib.md_grad_resample(p, p, 1, 8, 2, 2, 2, 2, 0, None) != 0                             # mode
    assert lib.md_s16b_transpose(p, p, 1, 12, 8, None) != 0
    assert lib.md_to_pb16(p, p, 1, 8, 8, 4, 4, 4, 40, 1, 0, 0, 0, 3, 1, None) != 0                # zsplit not a power of two
    assert lib.md_to_pb16(p, p, 1, 8, 16, 4, 4, 4, 40, 1, 0, 0, 0, 1, 1, None) != 0               # c_src > C
    assert lib.md_to_pb16(p, p, 1, 8, 8, 3, 4, 4, 40, 1, 0, 1, 0, 1, 1, None) != 0                # up on an odd grid
    assert lib.md_wgrad_finish(p, p, 8, 8, 4, 1, 0, 8, 1, 0, None) != 0                           # cols_alloc < cols


# ---------------------------------------------------------------------------------------------------------------
# md_channel_sums
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,grid", [(1, 32, (4, 4, 4)), (3, 128, (8, 8, 8)), (3, 32, (12, 12, 12)), (1, 256, (16, 16, 16))])
def test_channel_sums(ops, bw, B, C, grid):
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.hip_ops import _ptr, _stream
    P = grid[0] * grid[1] * grid[2]
    x = _randn((B, C, *grid), 60 + C) + 0.25
    t = _f32b(ops, x)
    ref = x.double().reshape(B, C, P).sum(2)
    _close(bw.channel_sums(t, B, C, P).cpu(), ref, f"channel sums B={B} C={C} P={P}")
    out0 = _randn((B, C), 61) * 10
    out = out0.clone().cuda()
    assert _lib.load().md_channel_sums(_ptr(t), _ptr(out), B, C, P, _stream()) == 0
    _close(out.cpu(), out0.double() + ref, "accumulated onto a non-zero out")


# ---------------------------------------------------------------------------------------------------------------
# md_grad_resample
# ---------------------------------------------------------------------------------------------------------------
def _resample(ops, t, B, C, dims_c, mode, acc_into=None):
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.hip_ops import _ptr, _stream
    Dc, Hc, Wc = dims_c
    Pc = Dc * Hc * Wc
    out = acc_into if acc_into is not None else torch.full((B, C // 8, Pc * (1 if mode == 0 else 8), 8), 7.0, device="cuda")
    assert _lib.load().md_grad_resample(_ptr(t), _ptr(out), B, C, Dc, Hc, Wc, mode, 1 if acc_into is not None else 0, _stream()) == 0
    return out


@pytest.mark.parametrize("B,C,dims_c", [(1, 8, (2, 3, 5)), (3, 32, (4, 6, 3)), (2, 16, (1, 1, 1)), (1, 64, (8, 8, 8))])
def test_grad_resample(ops, B, C, dims_c):
    Dc, Hc, Wc = dims_c
    fine = (2 * Dc, 2 * Hc, 2 * Wc)
    g = _randn((B, C, *fine), 70)
    # mode 0: sum of the 8 children = autograd of nearest-neighbour upsampling
    got = _from_f32b(ops, _resample(ops, _f32b(ops, g), B, C, dims_c, 0), dims_c)
    ref = g.double().view(B, C, Dc, 2, Hc, 2, Wc, 2).sum((3, 5, 7))
    _close(got, ref, f"mode 0 {dims_c}")
    xr = torch.zeros(B, C, *dims_c, dtype=torch.float64, requires_grad=True)
    F.interpolate(xr, scale_factor=2, mode="nearest").backward(g.double())
    assert _elem(ref, xr.grad) < 1e-14
    prev = _randn((B, C, *dims_c), 71) * 2 + 1
    acc = _from_f32b(ops, _resample(ops, _f32b(ops, g), B, C, dims_c, 0, acc_into=_f32b(ops, prev)), dims_c)
    _close(acc, prev.double() + ref, "mode 0 accumulate")
    # mode 1: zero-stuffing at odd positions, bit-exact
    c = _randn((B, C, *dims_c), 72)
    stuffed = _resample(ops, _f32b(ops, c), B, C, dims_c, 1)
    want = torch.zeros(B, C, *fine)
    want[:, :, 1::2, 1::2, 1::2] = c
    assert torch.equal(_from_f32b(ops, stuffed, fine).view(torch.int32), want.view(torch.int32))
    # mode 0 o mode 1 = identity, bit-exact
    back = _from_f32b(ops, _resample(ops, stuffed, B, C, dims_c, 0), dims_c)
    assert torch.equal(back.view(torch.int32), c.view(torch.int32))


def test_grad_resample_cubic_wrapper(ops, bw):
    B, C, Sc = 2, 16, 4
    g = _randn((B, C, 8, 8, 8), 73)
    got = _from_f32b(ops, bw.resample(_f32b(ops, g), B, C, Sc, 0), (Sc,) * 3)
    _close(got, g.double().view(B, C, Sc, 2, Sc, 2, Sc, 2).sum((3, 5, 7)), "backward.resample mode 0")


# ---------------------------------------------------------------------------------------------------------------
# md_s16b_transpose
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,Cn", [(3, 8, 40), (3, 24, 8), (1, 64, 136), (2, 8, 8), (3, 256, 64)])
def test_s16b_transpose(ops, bw, B, R, Cn):
    bits = torch.randint(-32768, 32767, (B, R // 8, 2, Cn, 8), generator=torch.Generator().manual_seed(R + Cn), dtype=torch.int16)
    t = bits.cuda().view(torch.bfloat16)
    out = bw.s16b_transpose(t, B, R, Cn)
    assert out.shape == (B, Cn // 8, 2, R, 8)
    logical = bits.permute(0, 2, 1, 4, 3).reshape(B, 2, R, Cn)                       # [b][plane][r][c]
    want = logical.reshape(B, 2, R, Cn // 8, 8).permute(0, 3, 1, 2, 4).contiguous()   # [b][c/8][plane][r][8]
    assert torch.equal(out.view(torch.int16).cpu(), want)
    again = bw.s16b_transpose(out, B, Cn, R)
    assert torch.equal(again.view(torch.int16).cpu(), bits)


# ---------------------------------------------------------------------------------------------------------------
# md_to_pb16
# ---------------------------------------------------------------------------------------------------------------
def _bits(x):
    return x.to(torch.bfloat16).view(torch.int16)


def _pb16_reference(hi, lo, B, C, grid, zs, pad, zhalo, up, stuff, guard):
    """hi, lo: bf16 planes of the SOURCE tensor as int16 [B][Cs][Ds][Hs][Ws].  Returns the whole PB16 buffer (int16):
    [guard + Pp + guard][ceil(B zs / 8)][2][C][8 virtual samples]."""
    Dfull, H, W = grid
    Dz = Dfull // zs
    planes = torch.stack([hi, lo])                                                  # [2][B][Cs][..]
    if up:
        planes = planes.repeat_interleave(2, 3).repeat_interleave(2, 4).repeat_interleave(2, 5)
    if stuff:
        z = torch.zeros(2, B, planes.shape[2], Dfull, H, W, dtype=torch.int16)
        z[:, :, :, 1::2, 1::2, 1::2] = planes
        planes = z
    assert planes.shape[3:] == (Dfull, H, W)
    full = torch.zeros(2, B, C, Dfull + 2 * pad, H + 2 * pad, W + 2 * pad, dtype=torch.int16)
    full[:, :, :planes.shape[2], pad:pad + Dfull, pad:pad + H, pad:pad + W] = planes
    VB, bg_n = B * zs, (B * zs + 7) // 8
    Pp = (Dz + 2 * pad) * (H + 2 * pad) * (W + 2 * pad)
    body = torch.zeros(Pp, bg_n, 2, C, 8, dtype=torch.int16)
    for v in range(VB):
        b, slab = divmod(v, zs)
        blk = full[:, b, :, slab * Dz:slab * Dz + Dz + 2 * pad].clone()             # [2][C][Dz + 2 pad][..]: halo = neighbouring slab
        if not zhalo:
            blk[:, :, :pad] = 0
            blk[:, :, pad + Dz:] = 0
        body[:, v // 8, :, :, v % 8] = blk.reshape(2, C, Pp).permute(2, 0, 1)
    g = torch.zeros(guard, bg_n, 2, C, 8, dtype=torch.int16)
    return torch.cat([g, body, g]).reshape(-1)


PB16_CASES = [
    # B, C, c_src, grid (Dfull, H, W), pad, mode, up, stuff, zhalo
    (1, 16, 16, (8, 8, 8), 1, 0, 0, 0, 1),
    (1, 16, 16, (8, 8, 8), 1, 0, 0, 0, 0),
    (3, 16, 8, (8, 8, 8), 1, 1, 0, 0, 1),
    (3, 8, 8, (8, 8, 8), 2, 0, 0, 0, 1),
    (3, 8, 8, (8, 8, 8), 2, 1, 0, 0, 0),
    (6, 16, 16, (8, 8, 8), 1, 0, 1, 0, 1),
    (6, 16, 16, (8, 8, 8), 1, 1, 0, 1, 0),
    (6, 8, 8, (8, 8, 8), 2, 0, 0, 0, 1),
    (8, 16, 8, (8, 8, 8), 1, 0, 0, 0, 1),
    (8, 8, 8, (4, 4, 4), 2, 1, 1, 0, 0),
    (11, 8, 8, (8, 8, 8), 1, 0, 0, 1, 0),
    (11, 16, 16, (8, 8, 8), 1, 1, 0, 0, 1),
    (11, 8, 8, (8, 8, 8), 2, 0, 1, 0, 1),
    (2, 8, 8, (4, 6, 10), 1, 0, 0, 0, 1),          # non-cubic, zsplit 4 -> one plane per slab
    (1, 8, 8, (8, 6, 4), 2, 0, 0, 1, 1),
]


@pytest.mark.parametrize("B,C,c_src,grid,pad,mode,up,stuff,zhalo", PB16_CASES)
def test_to_pb16(ops, bw, B, C, c_src, grid, pad, mode, up, stuff, zhalo):
    """Every form decoded on the host, bit for bit: the padded, sample-blocked tensor; zsplit = 8, 8, 4, 1, 8 for
    B = 1, 3, 6, 8, 11 as zsplit_for picks it; halo planes hold the neighbouring slab for the activation operand (zhalo = 1) and
    zeros for the dY operand; the partial last block of 8 and both guards are zero although the buffer held a pattern."""
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.hip_ops import _ptr, _stream
    lib = _lib.load()
    Dfull, H, W = grid
    zs = bw.zsplit_for(B, Dfull)
    if grid == (8, 8, 8):
        assert zs == {1: 8, 3: 8, 6: 4, 8: 1, 11: 8}[B]
    Dz = Dfull // zs
    sgrid = tuple(s // 2 for s in grid) if (up or stuff) else grid
    x = _randn((B, c_src, *sgrid), 80 + B + C) * 3
    if mode == 0:
        src = _f32b(ops, x)
        hi = _bits(x)
        lo = _bits(x - x.to(torch.bfloat16).float())                                    # md_split, as md_gn_apply's
    else:
        src = ops.ncdhw_to_s16b(x.cuda(), c_src)                                        # [B][c_src/8][2][P][8]
        pl = src.view(torch.int16).cpu()
        hi = pl[:, :, 0].permute(0, 1, 3, 2).reshape(B, c_src, *sgrid)
        lo = pl[:, :, 1].permute(0, 1, 3, 2).reshape(B, c_src, *sgrid)
        assert torch.equal(hi, _bits(x))
    sp = max(grid) + 2 * pad
    guard = ((pad * (sp * sp + sp + 1) + bw.GUARD_EXTRA + 3) // 4) * 4
    if grid[0] == grid[1] == grid[2]:
        assert guard == bw._guard(grid[0], pad)
    nbytes = lib.md_pb16_bytes(B * zs, C, Dz, H, W, guard, pad)
    assert nbytes > 0
    canary = 64
    out = torch.full((nbytes // 2 + canary,), 0x7F7F, dtype=torch.int16, device="cuda")
    rc = lib.md_to_pb16(_ptr(src), _ptr(out), B, C, c_src, Dz, H, W, guard, pad, mode, up, stuff, zs, zhalo, _stream())
    assert rc == 0
    got = out.cpu()
    want = _pb16_reference(hi, lo, B, C, grid, zs, pad, zhalo, up, stuff, guard)
    assert want.numel() == nbytes // 2
    assert bool((got[nbytes // 2:] == 0x7F7F).all()), "wrote past the end of the PB16 tensor"
    assert torch.equal(got[:nbytes // 2], want)
    if grid[0] == grid[1] == grid[2] and mode in (0, 1):     # the wrapper the training path uses gives the same bits
        w = bw.to_pb16(src, B, C, grid[0], mode, up=up, stuff=stuff, c_src=c_src, pad=pad, zhalo=bool(zhalo))
        assert torch.equal(w.view(torch.int16).cpu()[:nbytes // 2], want)


# ---------------------------------------------------------------------------------------------------------------
# md_wgrad_finish
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows,cols,cols_alloc,ntap,tap0,taps_total,conv", [
    ("conv3 [co][ci][27]", 20, 24, 24, 27, 0, 27, True),
    ("conv5 [co][ci][125], taps 50..74", 12, 8, 16, 25, 50, 125, True),
    ("NIN [ci][co]", 13, 40, 48, 1, 0, 1, False),
    ("conv3, rows % 8 == 0, one tap at tap0 = 26", 16, 8, 8, 1, 26, 27, True),
])
def test_wgrad_finish(ops, name, rows, cols, cols_alloc, ntap, tap0, taps_total, conv):
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.hip_ops import _ptr, _stream
    rows8 = (rows + 7) // 8
    g = _randn((ntap, rows8, cols_alloc, 8), 90 + rows)
    if conv:
        dw0 = _randn((rows, cols, taps_total), 91)
        s_row, s_k, s_tap = cols * taps_total, taps_total, 1
    else:
        dw0 = _randn((cols, rows), 91)
        s_row, s_k, s_tap = 1, rows, 0
    dw = dw0.clone().cuda()
    assert _lib.load().md_wgrad_finish(_ptr(g.cuda()), _ptr(dw), rows, cols, cols_alloc, ntap, tap0, s_row, s_k, s_tap, _stream()) == 0
    add = g.permute(0, 1, 3, 2).reshape(ntap, rows8 * 8, cols_alloc)[:, :rows, :cols].double()   # [ntap][rows][cols]
    ref = dw0.double().clone()
    if conv:
        ref[:, :, tap0:tap0 + ntap] += add.permute(1, 2, 0)
    else:
        ref += add[0].t()
    _close(dw.cpu(), ref, name, tol_l2=1e-7, tol_elem=2e-7)      # one fp32 addition per element
