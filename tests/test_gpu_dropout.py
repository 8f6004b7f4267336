"""Training dropout on the HIP path against tests/dropout_cases.py, the host restatement of the mask contract of csrc/md_common.h.

No expected mask in this file comes from the GPU: every one is dropout_cases.factor / keep (plain numpy).

  bit for bit (torch.equal on the raw words)
    md_dropout_scale                   == factor(...), c_off != 0 included; exactly 1.0 where thr16 == 0
    md_gn_apply(drop), raw mode        == the bf16 / fp16 operand split of fl32(x * scale) or +0; the raw planes stay unmasked
    md_wino_prep / _v2 (drop), raw     T(drop) on x == T on fl32(x * scale) * keep, kept T and scratch T, one and two parts
  against float64
    md_gn_apply(drop), GN + SiLU       kept values under stream_cases.gn_bound x scale, dropped ones exactly +0 in both planes
    md_wino_prep / _v2 (drop), GN+SiLU within 4 x the distance of an fp32 torch restatement (same bf16 split) from float64
    md_gn_bwd_stats / md_gn_bwd_apply  test_gpu_backward_kernels' float64 formula and bars, the gate from the restatement
    ResnetBlockDDPM                    the three routes of forward_blocked / backward_blocked, each named by what it launched,
                                       against autograd through the oracle with the restated mask (1e-4 forward, 2e-4 gradients)
    the whole U-Net step at p = 0.1    loss and every parameter gradient against oracle autograd under the recorded seeds

Measured on an MI355X: DESIGN.md, "Training dropout".
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_cases as dc
import stream_cases as sc
from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 2e-4          # tests/test_gpu_backward.py: gradients through two bf16x3 contractions
TOL_FWD = 1e-4


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def bw(ops):
    from meshdiffusion_amd.lib.diffusion.models import backward
    return backward


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _factor(seed, p, B, c_total, c_off, C, grid):
    """dropout_cases.factor as a torch tensor [B, C, *grid]."""
    P = int(np.prod(grid))
    return torch.from_numpy(dc.factor(seed, p, B, c_total, c_off, C, P)).reshape(B, C, *grid)


def _masked(x, seed, p, c_total, c_off):
    """fl32(x * scale) where kept, +0 where dropped: x [B, C, P] fp32 (one fp32 multiply per value, as every user does it)."""
    B, C, P = x.shape
    k = torch.from_numpy(dc.keep(seed, p, B, c_total, c_off, C, P))
    s = float(dc.scale(p)) if dc.thr16(p) else 1.0
    return torch.where(k, x * torch.tensor(s, dtype=torch.float32), torch.zeros(()))


# ---------------------------------------------------------------------------------------------------------------
# (a) md_dropout_scale
# ---------------------------------------------------------------------------------------------------------------
def _dropout_scale(ops, B, C, P, c_total, c_off, p, seed):
    from meshdiffusion_amd import _lib
    out = torch.full((B, C // 8, P, 8), float("nan"), device="cuda")
    _lib.check(_lib.load().md_dropout_scale(ops._ptr(out), B, C, P, c_total, c_off, float(p), int(seed), ops._stream()), "md_dropout_scale")
    return out.cpu().permute(0, 1, 3, 2).reshape(B, C, P)          # F32B -> [B, C, P]


@pytest.mark.parametrize("shape", dc.SCALE_SHAPES, ids=lambda s: "B{}-C{}-P{}-of{}-at{}".format(*s))
def test_dropout_scale_is_the_restated_factor(ops, shape):
    """md_dropout_scale through the export itself (hip_ops.dropout_scale cannot pass c_off), every seed x p, raw words."""
    B, C, P, c_total, c_off = shape
    for seed in dc.GPU_SEEDS:
        for p in dc.SCALE_PS:
            got = _dropout_scale(ops, B, C, P, c_total, c_off, p, seed)
            want = torch.from_numpy(dc.factor(seed, p, B, c_total, c_off, C, P))
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (seed, p, float((got != want).double().mean()))
    # thr16 == 0: the identity in every user, so the factors are exactly 1.0 (not 1 / (1 - p))
    assert dc.thr16(dc.P_IDENTITY) == 0
    got = _dropout_scale(ops, B, C, P, c_total, c_off, dc.P_IDENTITY, 5)
    assert torch.equal(got, torch.ones(B, C, P))


def test_thr16_zero_is_the_identity_in_every_user(ops, bw):
    """p = 1e-6 (thr16 == 0): md_gn_apply, md_wino_prep (both kernels) and md_gn_bwd_* give the bits of the run without dropout."""
    B, C, grid = 2, 32, (8, 8, 8)
    P, drop = 512, (dc.P_IDENTITY, 9)
    x, dy = _randn((B, C, P), 1), _randn((B, C, P), 2)
    parts = [(sc.to_f32b(x).cuda(), C)]
    gn = torch.nn.GroupNorm(32, C, eps=1e-6).cuda()
    params, ac = ops.gn_params(parts, gn.weight, gn.bias, B, P, want_ac=True)
    assert torch.equal(_bits(ops.gn_apply(parts, params, B, P, drop=drop)), _bits(ops.gn_apply(parts, params, B, P)))
    keep = ops.WINO_PREP_V2
    try:
        for v2 in (False, True):
            ops.WINO_PREP_V2 = v2
            t0 = ops.wino_prep(parts, ac, True, False, B, 8, keep=True)
            t1 = ops.wino_prep(parts, ac, True, False, B, 8, keep=True, drop=drop)
            assert torch.equal(_bits(t0), _bits(t1))
    finally:
        ops.WINO_PREP_V2 = keep
    dyb = sc.to_f32b(dy).cuda()
    d0 = bw.gn_backward(parts, dyb, params, gn, B, P, True, param_grads=False)[0]
    d1 = bw.gn_backward(parts, dyb, params, gn, B, P, True, param_grads=False, drop=drop)[0]
    assert torch.equal(d0, d1)
    _ = grid


# ---------------------------------------------------------------------------------------------------------------
# (b) md_gn_apply(drop)
# ---------------------------------------------------------------------------------------------------------------
RAW_B, RAW_PARTS, RAW_P = 3, (8, 16), 210          # the second part runs with c_off = 8; P = 5 * 6 * 7


@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("seed", dc.GPU_SEEDS, ids=hex)
def test_gn_apply_raw_mode_is_the_split_of_the_masked_input(ops, seed, p):
    B, P, ctot = RAW_B, RAW_P, sum(RAW_PARTS)
    x = _randn((B, ctot, P), 31) * 3
    xs = torch.split(x, list(RAW_PARTS), 1)
    parts = [(sc.to_f32b(t).cuda(), c) for t, c in zip(xs, RAW_PARTS)]
    want = _masked(x, seed, p, ctot, 0)                                   # channel = c_off + c of the concatenated tensor
    assert torch.equal(want, torch.cat([_masked(t, seed, p, ctot, off) for t, off in zip(xs, (0, RAW_PARTS[0]))], 1))
    whi, wlo = sc.split_bf16(want)
    out, raw = ops.gn_apply(parts, None, B, P, norm=False, silu=False, drop=(p, seed), want_raw=True)
    hi, lo = sc.from_s16b(out.cpu())
    assert torch.equal(_bits(hi), _bits(whi)) and torch.equal(_bits(lo), _bits(wlo))
    dropped = want == 0
    assert 0 < int(dropped.sum()) < want.numel() and not _bits(hi)[dropped].any() and not _bits(lo)[dropped].any()
    # the raw planes (the shortcut NIN's operand) are NOT masked: the bits of the run without `drop`
    plain, raw0 = ops.gn_apply(parts, None, B, P, norm=False, silu=False, want_raw=True)
    assert torch.equal(_bits(raw), _bits(raw0)) and torch.equal(_bits(raw0), _bits(plain))
    # fp16 operand format: plane 0 = fp16(fl32(x * scale)) or +0, plane 1 is not written
    pre = torch.full((B, ctot // 8, 2, P, 8), 7.0, dtype=torch.bfloat16, device="cuda")
    o16 = ops.gn_apply(parts, None, B, P, norm=False, silu=False, drop=(p, seed), fp16=True, out=pre).cpu()
    got16 = o16[:, :, 0].permute(0, 1, 3, 2).reshape(B, ctot, P)
    assert torch.equal(_bits(got16), _bits(want.to(torch.float16)))
    assert bool((o16[:, :, 1] == 7.0).all())


def test_gn_apply_norm_silu_dropout_vs_float64(ops):
    """GroupNorm + SiLU + dropout 0.3 on a two-part P = 210 case (GroupNorm needs 32 groups: parts (32, 64), so the second part
    runs with c_off = 32).  Dropped elements are exactly +0 in both planes, kept ones are non-zero (beta is shifted by +4, so no
    activated value is 0) and meet stream_cases.gn_bound -- the bar of test_groupnorm_vs_float64 -- times the scale."""
    p, seed = 0.3, dc.GPU_SEEDS[2]
    case = sc._gn_case("dropout-P210", 3, (32, 64), (5, 6, 7), 77)
    case["beta"] = case["beta"] + 4.0
    B, C, P = case["B"], case["C"], case["P"]
    parts = [(sc.to_f32b(t).cuda(), c) for t, c in zip(torch.split(case["x"], list(case["parts"]), 1), case["parts"])]
    params = ops.gn_params(parts, case["gamma"].cuda(), case["beta"].cuda(), B, P, eps=sc.GN_EPS, groups=sc.GN_GROUPS)
    hi, lo = sc.from_s16b(ops.gn_apply(parts, params, B, P, norm=True, silu=True, drop=(p, seed)).cpu())
    keep = torch.from_numpy(dc.keep(seed, p, B, C, 0, C, P))
    ref = sc.gn_reference(case, True)["out"]
    assert float(ref.abs().min()) > 1e-30
    assert not _bits(hi)[~keep].any() and not _bits(lo)[~keep].any()
    assert bool((hi[keep] != 0).all())
    s64 = float(dc.scale(p))
    got = hi.double() + lo.double()
    err = (got - ref * s64).abs()[keep]
    bound = (sc.gn_bound(case, True) * s64)[keep]
    worst = float((err / bound).max())
    print(f"gn_apply GN + SiLU + dropout {p}: kept {int(keep.sum())} of {keep.numel()}, worst err/bound {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# (c) md_wino_prep(drop)
# ---------------------------------------------------------------------------------------------------------------
PREP_B, PREP_C = 2, 16


def _prep_parts(x, two_parts):
    cs = (8, 8) if two_parts else (PREP_C,)
    return [(sc.to_f32b(t.contiguous()).cuda(), c) for t, c in zip(torch.split(x, list(cs), 1), cs)]


def _wino_transform(y):
    """y [B, C, D, H, W] (activation, any float dtype) -> [4, B, C, D, H, W/2]: zero padded along w AFTER the activation,
    d_k = y[2i - 1 + k], (d0 - d2, d1 + d2, d2 - d1, d1 - d3) -- tests/test_gpu_wino.py::test_wino_prep_layout_and_values."""
    W = y.shape[-1]
    yp = F.pad(y, (1, 1))
    d = [yp[..., k:k + W:2] for k in range(4)]
    return torch.stack([d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]])


def _t_planes(t, B, C, dims):
    """T[b][c/8][f][plane][z][y][pair][8] -> (hi, lo) as [4, B, C, D, H, W/2] bf16."""
    D, H, W = dims
    t = t.cpu().view(B, C // 8, 4, 2, D, H, W // 2, 8)
    v = t.permute(3, 2, 0, 1, 7, 4, 5, 6).reshape(2, 4, B, C, D, H, W // 2)
    return v[0], v[1]


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "scratch"])
@pytest.mark.parametrize("v2", [True, False], ids=["v2", "v1"])
@pytest.mark.parametrize("two_parts", [False, True], ids=["one_part", "two_parts"])
@pytest.mark.parametrize("dims", [(8, 8, 8), (8, 8, 16)], ids=["8x8x8", "8x8x16"])
def test_wino_prep_dropout_is_one_multiply_in_front_of_the_transform(ops, monkeypatch, dims, two_parts, v2, keep):
    """Raw operand: T with drop = (p, seed) on x equals, bit for bit, T without drop on fl32(x * scale) * keep -- for the
    one-thread-per-pair kernel and the two-phase one, the kept tensor (md_wgrad_wino reads it) and the scratch one."""
    monkeypatch.setattr(ops, "WINO_PREP_V2", v2)
    B, C, P = PREP_B, PREP_C, dims[0] * dims[1] * dims[2]
    x = _randn((B, C, P), 41) * 2
    parts = _prep_parts(x, two_parts)
    for p, seed in ((0.1, dc.GPU_SEEDS[3]), (0.5, dc.GPU_SEEDS[2])):
        xm = _masked(x, seed, p, C, 0)
        want = ops.wino_prep(_prep_parts(xm, two_parts), None, False, False, B, None, dims=dims, keep=keep).clone()
        got = ops.wino_prep(parts, None, False, False, B, None, dims=dims, keep=keep, drop=(p, seed)).clone()
        assert torch.equal(_bits(got), _bits(want)), (p, seed)
        plain = ops.wino_prep(parts, None, False, False, B, None, dims=dims, keep=keep)
        assert not torch.equal(_bits(got), _bits(plain))
    # ... and T of the masked input is the transform's layout and values (so `want` is not wrong in the same way)
    hi, lo = _t_planes(want, B, C, dims)
    whi, wlo = sc.split_bf16(_wino_transform(xm.reshape(B, C, *dims)))
    assert torch.equal(_bits(hi), _bits(whi)) and torch.equal(_bits(lo), _bits(wlo))


@pytest.mark.parametrize("v2", [True, False], ids=["v2", "v1"])
@pytest.mark.parametrize("dims", [(8, 8, 8), (8, 8, 16)], ids=["8x8x8", "8x8x16"])
def test_wino_prep_dropout_on_an_upsampled_operand_masks_the_source_grid(ops, monkeypatch, dims, v2):
    """Nearest-x2 upsampling in the operand pass: the mask belongs to the SOURCE tensor (its P positions index the quads), so
    T(drop, ups) on x is T(ups) on the masked x.  No layer of the registered models combines the two; the kernels take both
    arguments, and the quad index is the one place where the source and the output grid can be confused."""
    monkeypatch.setattr(ops, "WINO_PREP_V2", v2)
    B, C, p, seed = PREP_B, PREP_C, 0.3, dc.GPU_SEEDS[1]
    Pin = (dims[0] // 2) * (dims[1] // 2) * (dims[2] // 2)
    x = _randn((B, C, Pin), 47)
    xm = _masked(x, seed, p, C, 0)
    for two_parts in (False, True):
        want = ops.wino_prep(_prep_parts(xm, two_parts), None, False, True, B, None, dims=dims, keep=True)
        got = ops.wino_prep(_prep_parts(x, two_parts), None, False, True, B, None, dims=dims, keep=True, drop=(p, seed))
        assert torch.equal(_bits(got), _bits(want)), two_parts


@pytest.mark.parametrize("v2", [True, False], ids=["v2", "v1"])
@pytest.mark.parametrize("two_parts", [False, True], ids=["one_part", "two_parts"])
@pytest.mark.parametrize("dims", [(8, 8, 8), (8, 8, 16)], ids=["8x8x8", "8x8x16"])
def test_wino_prep_gn_silu_dropout_vs_float64(ops, monkeypatch, dims, two_parts, v2):
    """GroupNorm affine + SiLU + dropout 0.1: T (hi + lo) against float64 transform(silu(a x + c) * factor) with the (a, c) the
    kernel reads.  Bar: 4 x the distance of the same chain in torch fp32 (same bf16 split) from that float64 value, on the
    largest elementwise error and on rel-L2."""
    monkeypatch.setattr(ops, "WINO_PREP_V2", v2)
    B, C, P, p, seed = PREP_B, PREP_C, dims[0] * dims[1] * dims[2], 0.1, dc.GPU_SEEDS[2]
    x = _randn((B, C, P), 43) * 1.5 + 0.3
    parts = _prep_parts(x, two_parts)
    gamma, beta = 1.0 + 0.2 * _randn((C,), 44), 0.5 * _randn((C,), 45)
    _, ac = ops.gn_params(parts, gamma.cuda(), beta.cuda(), B, P, groups=2, want_ac=True)
    t = ops.wino_prep(parts, ac, True, False, B, None, dims=dims, keep=True, drop=(p, seed))
    hi, lo = _t_planes(t, B, C, dims)
    got = hi.double() + lo.double()
    ac = ac.cpu()
    fac = _factor(seed, p, B, C, 0, C, dims)
    x5 = x.reshape(B, C, *dims)
    a, c = ac[..., 0][:, :, None, None, None], ac[..., 1][:, :, None, None, None]
    ref = _wino_transform(F.silu(a.double() * x5.double() + c.double()) * fac.double())
    h32, l32 = sc.split_bf16(_wino_transform(F.silu(a * x5 + c) * fac))
    r32 = h32.double() + l32.double()
    e_max, e_max32 = float((got - ref).abs().max()), float((r32 - ref).abs().max())
    e_l2, e_l232 = rel_l2(got, ref), rel_l2(r32, ref)
    print(f"wino_prep GN + SiLU + dropout {dims} parts={1 + two_parts} v2={v2}: max err {e_max:.3e} (fp32 torch {e_max32:.3e}), "
          f"rel-L2 {e_l2:.3e} (fp32 torch {e_l232:.3e})")
    assert e_max <= 4 * e_max32 and e_l2 <= 4 * e_l232
    kp = F.pad(fac != 0, (1, 1))
    d = [kp[..., k:k + dims[2]:2] for k in range(4)]
    zero = ~torch.stack([d[0] | d[2], d[1] | d[2], d[2] | d[1], d[1] | d[3]])     # both taps of the entry dropped (or outside the grid)
    assert int(zero.sum()) > 0 and not _bits(hi)[zero].any() and not _bits(lo)[zero].any()


# ---------------------------------------------------------------------------------------------------------------
# (d) md_gn_bwd_stats / md_gn_bwd_apply
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,cparts,grid", [(0.1, (128,), (8, 8, 8)), (0.5, (64, 64), (8, 8, 8)), (0.3, (64, 64), (5, 6, 7)),
                                           (0.1, (32,), (5, 6, 7))])
def test_gn_backward_dropout_gate_is_the_restated_factor(ops, bw, p, cparts, grid):
    """test_gpu_backward_kernels.test_gn_backward_dropout_gate with the gate from the restatement (not md_dropout_scale), its
    float64 formula and bars; P = 210 (5 x 6 x 7) added."""
    import test_gpu_backward_kernels as bk
    B, silu, seed = 2, True, 0x1234567890ABCDE
    C, P = sum(cparts), grid[0] * grid[1] * grid[2]
    x, dy, gamma, beta = bk._gn_inputs("dy_mean", B, C, P, 51)
    parts = [(ops.ncdhw_to_f32b(t.reshape(B, c, *grid).cuda()), c) for t, c in zip(torch.split(x, list(cparts), 1), cparts)]
    gn = bk._gn_module(C, gamma, beta)
    params = ops.gn_params(parts, gn.weight, gn.bias, B, P, eps=gn.eps, groups=32)
    mask = torch.from_numpy(dc.factor(seed, p, B, C, 0, C, P))
    outs = bw.gn_backward(parts, ops.ncdhw_to_f32b(dy.reshape(B, C, *grid).cuda()), params, gn, B, P, silu, drop=(p, seed))
    got = torch.cat([ops.f32b_to_ncdhw(o, grid).cpu().reshape(B, -1, P) for o in outs], 1)
    ref, dg, db = bk._gn_ref(x, dy, params.cpu(), gamma, 32, silu, mask=mask)
    bk._close(got, ref, f"dx with dropout p={p}")
    bk._close(gn.weight.grad.cpu(), dg, "dgamma")
    bk._close(gn.bias.grad.cpu(), db, "dbeta")


# ---------------------------------------------------------------------------------------------------------------
# (e), (f) the routes of ResnetBlockDDPM
# ---------------------------------------------------------------------------------------------------------------
PARAM_NAMES = ("Conv_0.weight", "Conv_1.weight", "Conv_1.bias", "GroupNorm_0.weight", "GroupNorm_0.bias", "GroupNorm_1.weight",
               "GroupNorm_1.bias")
BLOCK_TORCH_SEED = 99


def _block(cin, cout, p):
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import layers
    blk = layers.ResnetBlockDDPM(act=torch.nn.SiLU(), in_ch=cin, out_ch=cout, temb_dim=128, dropout=p)
    sd = synth.sensitised_state_dict(blk.state_dict(), seed=5)
    blk.load_state_dict(sd)
    return blk.cuda().train(), sd


def _block_inputs(cin_parts, cout, S, B):
    xs = [_randn((B, c, S, S, S), 20 + i) for i, c in enumerate(cin_parts)]
    return xs, _randn((B, 128), 22), _randn((B, cout, S, S, S), 23)


def _run_block(ops, blk, xs, cin_parts, temb, dy, S, param_grads=True, tape=None):
    """forward_blocked + backward_blocked under torch.manual_seed(BLOCK_TORCH_SEED).  Returns a dict: y, dparts, grads, dbias0,
    tape entry, PROFILE tags, and the `drop` argument of every hip_ops.gn_apply / wino_prep call (what each launch was given)."""
    B, P = xs[0].shape[0], S ** 3
    parts = [(ops.ncdhw_to_f32b(x.cuda()), c) for x, c in zip(xs, cin_parts)]
    for q in blk.parameters():
        q.grad = None
    seen = dict(gn_apply=[], wino_prep=[])
    real_gn, real_prep = ops.gn_apply, ops.wino_prep
    ops.gn_apply = lambda *a, **k: (seen["gn_apply"].append(k.get("drop")), real_gn(*a, **k))[1]
    ops.wino_prep = lambda *a, **k: (seen["wino_prep"].append((k.get("drop"), bool(k.get("keep")))), real_prep(*a, **k))[1]
    ops.PROFILE = []
    try:
        with torch.no_grad():
            if tape is None:
                tape = []
                torch.manual_seed(BLOCK_TORCH_SEED)
                y = blk.forward_blocked(parts, B, P, temb.cuda(), tape=tape)
            else:
                y = None
            dparts, dbias0 = blk.backward_blocked(tape[0], ops.ncdhw_to_f32b(dy.cuda()), param_grads=param_grads)
        tags = [e[0] for e in ops.PROFILE]
    finally:
        ops.PROFILE, ops.gn_apply, ops.wino_prep = None, real_gn, real_prep
    sp = (S, S, S)
    return dict(y=None if y is None else ops.f32b_to_ncdhw(y, sp).cpu(), dparts=[ops.f32b_to_ncdhw(g, sp).cpu() for g in dparts],
                grads={n: q.grad.detach().cpu().clone() for n, q in blk.named_parameters() if q.grad is not None},
                dbias0=None if dbias0 is None else dbias0.cpu(), tape=tape, tags=tags, seen=seen)


@functools.lru_cache(maxsize=None)
def _block_oracle(cin_parts, cout, S, B, p, seed):
    """torch autograd (fp32, CPU) through oracle.unet_oracle.resnet_block with the restated factors.  Computed once per case and
    shared; callers must not modify what it returns."""
    from oracle import unet_oracle as uo
    _, sd = _block(sum(cin_parts), cout, p)
    xs, temb, dy = _block_inputs(cin_parts, cout, S, B)
    fac = _factor(seed, p, B, cout, 0, cout, (S, S, S))
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = [x.clone().requires_grad_(True) for x in xs]
    tr = temb.clone().requires_grad_(True)
    y = uo.resnet_block(sdr, torch.cat(xr, 1), tr, drop=fac)
    y.backward(dy)
    return dict(y=y.detach(), dx=[x.grad for x in xr], grads={k: v.grad for k, v in sdr.items() if v.grad is not None})


def _check_block(run, ref, cin, cout, what):
    worst = {}
    worst["y"] = rel_l2(run["y"], ref["y"])
    assert worst["y"] < TOL_FWD, (what, worst)
    for i, (g, r) in enumerate(zip(run["dparts"], ref["dx"])):
        worst[f"dx{i}"] = rel_l2(g, r)
    for n in PARAM_NAMES + (("NIN_0.W", "NIN_0.b") if cin != cout else ()):
        worst[n] = rel_l2(run["grads"][n], ref["grads"][n])
    # FiLM: dbias0 [B, cout] summed over the batch is the gradient of Dense_0.bias (and of Conv_0.bias)
    worst["dbias0"] = rel_l2(run["dbias0"].sum(0), ref["grads"]["Dense_0.bias"])
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if k != "y" and not v < TOL}
    assert not bad, (what, bad)
    return worst


def test_block_direct_route_identity_shortcut(ops):
    """64 -> 64 at 8^3, B = 3, p = 0.1: no Winograd kernel; the mask is the one md_gn_apply(drop) writes into the S16B activation
    a1, read by the direct forward conv and the weight gradient; identity shortcut (residual in GroupNorm_0's backward)."""
    cin_parts, cout, S, B, p = (64,), 64, 8, 3, 0.1
    blk, _ = _block(64, cout, p)
    xs, temb, dy = _block_inputs(cin_parts, cout, S, B)
    run = _run_block(ops, blk, xs, cin_parts, temb, dy, S)
    tp = run["tape"][0]
    (pd, seed) = tp["drop"]
    assert pd == p and not hasattr(blk, "NIN_0")
    assert "wino" not in run["tags"] and "wino_prep" not in run["tags"] and "wgrad_wino" not in run["tags"], run["tags"]
    assert tp["a1"] is not None and tp["t0"] is None and tp["t1"] is None
    assert run["seen"]["gn_apply"].count((p, seed)) == 1 and not run["seen"]["wino_prep"]
    _check_block(run, _block_oracle(cin_parts, cout, S, B, p, seed), 64, cout, "direct route 64->64 @8^3 B=3")


WW_CASES = [((128, 128), 2), ((128,), 2), ((128,), 3)]


def _conv1_wgrad_f64(ops, tp, blk, dy, fac):
    """float64 Conv_1 weight gradient on the GPU, from the block's own fp32 h (tape) through float64 GroupNorm_1 + SiLU times the
    restated factors, as 27 shifted matmuls: dW[co][ci][kd][kh][kw] = sum_{b, pos} dy[b][co][pos] * act[b][ci][pos + k - 1]."""
    B, S, C = tp["B"], tp["S"], blk.out_ch
    h = ops.f32b_to_ncdhw(tp["h"], (S, S, S)).double()
    gn = blk.GroupNorm_1
    act = F.silu(F.group_norm(h, gn.num_groups, gn.weight.double(), gn.bias.double(), gn.eps)) * fac.cuda().double()
    ap = F.pad(act, (1, 1, 1, 1, 1, 1))
    dyf = dy.cuda().double().permute(1, 0, 2, 3, 4).reshape(C, -1)
    dw = torch.empty(C, C, 3, 3, 3, dtype=torch.float64, device="cuda")
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                a = ap[:, :, kd:kd + S, kh:kh + S, kw:kw + S].permute(1, 0, 2, 3, 4).reshape(C, -1)
                dw[:, :, kd, kh, kw] = dyf @ a.t()
    return dw.cpu()


@pytest.mark.parametrize("cin_parts,B", WW_CASES, ids=["256to128-B2", "128to128-B2", "128to128-B3"])
def test_block_winograd_forward_and_winograd_weight_gradient(ops, cin_parts, B):
    """32^3, p = 0.1: the route of the training benchmark.  md_gn_apply writes NO activation for Conv_1 (a1 is None): the mask
    lives only in the kept operand T of md_wino_prep(drop, keep), which feeds the forward conv and md_wgrad_wino; the data
    gradients are the f16f6 Winograd convs with the dynamic lift.  Against oracle autograd with the restated mask, against a
    float64 Conv_1 weight gradient of the masked activation, and against the direct kernels (ops.WINO off) on the same mask."""
    cout, S, p = 128, 32, 0.1
    cin = sum(cin_parts)
    assert ops.WINO and ops.WINO_TRAIN_FWD and ops.wgrad_wino_ok(cout, cin, S, B) and B * (S ** 3 // 256) >= ops.WINO_MIN_WGS_TRAIN
    blk, _ = _block(cin, cout, p)
    xs, temb, dy = _block_inputs(cin_parts, cout, S, B)
    run = _run_block(ops, blk, xs, cin_parts, temb, dy, S)
    tp, tags, seen = run["tape"][0], run["tags"], run["seen"]
    (pd, seed) = tp["drop"]
    assert pd == p
    assert tp["a1"] is None and tp["a0"] is None and tp["t0"] is not None and tp["t1"] is not None
    assert tags.count("wgrad_wino") == 2 and tags.count("wino") == 4, tags
    assert (p, seed) not in seen["gn_apply"]                                   # no S16B activation carries the mask
    assert seen["wino_prep"].count(((p, seed), True)) == 1                     # one kept T holds it
    what = f"wino fwd + wino wgrad {cin}->{cout} @32^3 B={B}"
    fac = _factor(seed, p, B, cout, 0, cout, (S, S, S))
    e64 = rel_l2(run["grads"]["Conv_1.weight"], _conv1_wgrad_f64(ops, tp, blk, dy, fac))
    print(f"{what}: Conv_1.weight gradient (md_wgrad_wino on the dropped T) vs float64 of the masked activation {e64:.2e}")
    assert e64 < TOL
    _check_block(run, _block_oracle(cin_parts, cout, S, B, p, seed), cin, cout, what)
    # the direct kernels on the same inputs and mask, at the bars of test_resnet_block_training_through_winograd_path
    ops.WINO = False
    try:
        run2 = _run_block(ops, blk, xs, cin_parts, temb, dy, S)
    finally:
        ops.WINO = True
    assert "wino" not in run2["tags"] and "wgrad_wino" not in run2["tags"] and run2["tape"][0]["drop"] == (pd, seed)
    assert run2["tape"][0]["a1"] is not None and run2["seen"]["gn_apply"].count((p, seed)) == 1
    e = dict(y=rel_l2(run["y"], run2["y"]))
    e.update({f"dx{i}": rel_l2(a, b) for i, (a, b) in enumerate(zip(run["dparts"], run2["dparts"]))})
    e.update({n: rel_l2(run["grads"][n], run2["grads"][n]) for n in run["grads"]})
    print(f"{what} vs direct kernels: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["y"] < 2e-5 and all(v < 5e-5 for k, v in e.items() if k != "y"), e


def test_block_input_gradient_only_in_training_mode(ops):
    """param_grads=False on the 32^3 128 -> 128 block (the input gradient of a training-mode forward): the gate of
    md_gn_bwd_apply under the seed of the tape, against the oracle with the restated mask; no `.grad`, no dbias0."""
    cin_parts, cout, S, B, p = (128,), 128, 32, 2, 0.1
    blk, _ = _block(128, cout, p)
    xs, temb, dy = _block_inputs(cin_parts, cout, S, B)
    fwd = _run_block(ops, blk, xs, cin_parts, temb, dy, S)
    run = _run_block(ops, blk, xs, cin_parts, temb, dy, S, param_grads=False, tape=fwd["tape"])
    (pd, seed) = fwd["tape"][0]["drop"]
    assert run["dbias0"] is None and not run["grads"] and not [t for t in run["tags"] if "wgrad" in str(t)]
    ref = _block_oracle(cin_parts, cout, S, B, p, seed)
    e = rel_l2(run["dparts"][0], ref["dx"][0])
    print(f"input gradient alone, training mode, 128->128 @32^3 B=2 p={p}: {e:.2e}")
    assert e < TOL


# ---------------------------------------------------------------------------------------------------------------
# the whole step with dropout on
# ---------------------------------------------------------------------------------------------------------------
class record_seeds:
    """Wraps hip_ops.next_dropout_seed: records what it returns, replaces nothing."""

    def __init__(self, ops):
        self.ops, self.seeds = ops, []

    def __enter__(self):
        self.real = self.ops.next_dropout_seed
        self.ops.next_dropout_seed = lambda: (self.seeds.append(self.real()), self.seeds[-1])[1]
        return self.seeds

    def __exit__(self, *exc):
        self.ops.next_dropout_seed = self.real


def _atomic_sums(net):
    """Names of the gradients that end in float atomics or derive from such sums: two identical backwards differ in them by the
    order of fp32 additions.  tests/test_gpu_input_grad.py's list (conv / NIN / Linear biases, the FiLM table Dense_0, the timestep
    MLP behind it) and, at B >= 3, the GroupNorm parameters: md_gn_bwd_finalize adds each sample's share with a float atomicAdd
    (csrc/backward.hip), which commutes for two samples only."""
    names = set()
    for mn, mod in net.named_modules():
        for pn, _ in mod.named_parameters(recurse=False):
            n = f"{mn}.{pn}" if mn else pn
            if (isinstance(mod, torch.nn.GroupNorm) or pn in ("bias", "b") or n.endswith("Dense_0.weight")
                    or n in ("all_modules.0.weight", "all_modules.1.weight")):
                names.add(n)
    return names


@pytest.mark.parametrize("arch,B", [("ddpm_res64", 3), ("ddpm_res128", 8)])
def test_whole_unet_step_with_dropout_vs_oracle_autograd(ops, arch, B):
    """test_gpu_train.test_whole_unet_backward_and_train_step_vs_oracle_autograd with cfg.model.dropout = 0.1: the seeds the
    step drew are recorded (not replaced), the factors are built from the restatement, and loss and every parameter gradient
    are compared with torch autograd through the oracle on the CPU at that test's bars (1e-4, 2e-3 per tensor, 5e-4 of the
    global norm).  Also: the same torch seed repeats the step (loss and every gradient that does not end in float atomics bit
    for bit; the atomic sums, _atomic_sums, to 1e-5 of the global gradient norm: the order of fp32 additions costs sqrt(n) 2^-24,
    far below it, while another mask moves them by their own size), the next step draws other seeds, eval mode draws none and is the dropout-free forward, and the
    input gradient in training mode is the oracle's under the same masks."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, ddpm_res128, layers, utils as mutils  # noqa: F401
    from oracle import unet_oracle as uo
    p = 0.1
    cfg = synth.small_config() if arch == "ddpm_res64" else synth.small_config_res128()
    cfg.device = torch.device("cuda")
    cfg.model.dropout = p
    model = mutils.create_model(cfg)
    R = cfg.data.image_size
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    n_blocks = sum(isinstance(m, layers.ResnetBlockDDPM) for m in model.modules())
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, 1, R, R, R).cuda()
    loss_fn = losses.get_ddpm_loss_fn(sde, train=True, mask=mask)
    batch = (synth.synthetic_inputs(B, 4, R, seed=8) * mask.cpu()).cuda()

    def step(torch_seed=321):
        for q in model.parameters():
            q.grad = None
        if torch_seed is not None:
            torch.manual_seed(torch_seed)
        with record_seeds(ops) as seeds:
            loss = loss_fn(model, batch)
            loss.backward()
        return (float(loss.detach()), {n: q.grad.detach().cpu().clone() for n, q in model.module.named_parameters() if q.grad is not None},
                list(seeds))
    loss, grads, seeds = step()
    assert len(seeds) == n_blocks and len(set(seeds)) == n_blocks and all(0 <= s < 2 ** 62 for s in seeds)
    # ---- reference: autograd through the oracle, same labels / noise stream, the restated masks ----
    torch.manual_seed(321)
    labels = torch.randint(0, 1000, (B,), device="cuda").cpu()
    noise = torch.randn_like(batch).cpu()
    b, m = batch.cpu(), mask.cpu()
    _, sa, s1 = uo.vpsde_tables()
    xt = (sa[labels, None, None, None, None] * b + s1[labels, None, None, None, None] * noise) * m
    drops = [functools.partial(lambda shape, s: _factor(s, p, shape[0], shape[1], 0, shape[1], shape[2:]), s=s) for s in seeds]
    sdr = {k: v.clone().requires_grad_(v.dtype == torch.float32 and k not in ("coords", "mask")) for k, v in sd.items()}
    e = uo.unet_res64_forward(sdr, synth.oracle_cfg(cfg), xt, labels, drops=drops)
    ls = (torch.square(e - noise) * m).reshape(B, -1).mean(-1)
    ref_loss = ls.mean() / m.sum() * m.numel()
    ref_loss.backward()
    print(f"{arch} B={B} p={p}: loss {loss:.6f}, oracle {float(ref_loss):.6f}, {n_blocks} ResnetBlocks")
    assert abs(loss - float(ref_loss)) / float(ref_loss) < 1e-4
    worst = ("", 0.0)
    gnorm = torch.sqrt(sum((sdr[n].grad.double() ** 2).sum() for n in grads))
    for n, g in grads.items():
        r = sdr[n].grad
        err = float((g.double() - r.double()).norm() / gnorm)     # error relative to the whole gradient
        if err > worst[1]:
            worst = (n, err)
        if float(r.norm()) > 1e-3 * float(gnorm):
            assert rel_l2(g, r) < 2e-3, n
    print("worst per-tensor error relative to the global grad norm:", worst)
    assert worst[1] < 5e-4
    assert set(grads) == {n for n, v in sdr.items() if v.grad is not None}
    # ---- the same torch seed repeats the step; the next step draws other seeds ----
    loss2, grads2, seeds2 = step()
    loss3, grads3, seeds3 = step(torch_seed=None)
    assert seeds2 == seeds and loss2 == loss
    atomic = _atomic_sums(model.module)
    exact = [n for n in grads if n not in atomic]
    differ = [n for n in exact if not torch.equal(grads[n], grads2[n])]
    # measured against the whole gradient, like the errors above: the exact gradient of an attention key bias is 0, so both
    # runs hold round-off only and its own norm is no yardstick
    gn1 = math.sqrt(sum(float(g.double().square().sum()) for g in grads.values()))
    spread = max(float((grads2[n].double() - grads[n].double()).norm()) / gn1 for n in grads)
    print(f"same torch seed twice: {len(exact)} gradients expected bit-identical, {len(differ)} differ {differ[:4]}; "
          f"worst difference over all {len(grads)} relative to the global grad norm: {spread:.2e}")
    assert len(exact) > 20 and not differ
    assert spread < 1e-5
    assert not set(seeds3) & set(seeds) and len(set(seeds3)) == n_blocks and loss3 != loss
    # ---- eval mode draws no seed and is the dropout-free forward, bit for bit ----
    x_in, lab = xt.cuda(), labels.float().cuda()
    with torch.no_grad(), record_seeds(ops) as drawn:
        y_eval = model.eval()(x_in, lab)
    assert not drawn
    for mod in model.modules():
        if isinstance(mod, layers.ResnetBlockDDPM):
            mod.Dropout_0.p = 0.0
    with torch.no_grad():
        assert torch.equal(model.eval()(x_in, lab), y_eval)
    for mod in model.modules():
        if isinstance(mod, layers.ResnetBlockDDPM):
            mod.Dropout_0.p = p
    # ---- x.requires_grad_() in training mode: the oracle's input gradient under the same masks ----
    cot = _randn(tuple(xt.shape), 12)
    for q in model.parameters():
        q.grad = None
    xg = xt.cuda().requires_grad_(True)
    torch.manual_seed(5)
    with record_seeds(ops) as seeds_x:
        model.train()(xg, lab).backward(cot.cuda())
    assert len(seeds_x) == n_blocks
    xr = xt.clone().requires_grad_(True)
    drops = [functools.partial(lambda shape, s: _factor(s, p, shape[0], shape[1], 0, shape[1], shape[2:]), s=s) for s in seeds_x]
    uo.unet_res64_forward(sd, synth.oracle_cfg(cfg), xr, labels.float(), drops=drops).backward(cot)
    e_dx = rel_l2(xg.grad, xr.grad)
    print(f"training-mode input gradient under dropout vs oracle: {e_dx:.2e}")
    assert e_dx < 2e-3                                                  # tests/test_gpu_input_grad.py's bar for this gradient


_ = math
