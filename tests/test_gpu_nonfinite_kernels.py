"""NaN and +-inf operands to the kernels tests/test_gpu_nonfinite.py does not reach: the direct convs and GEMMs behind
md_gemm_conv, md_conv3_s2 / _stem / _head, md_nin_f32, md_attn_fwd, md_softmax_keys(_bwd), GroupNorm forward and backward, the
three weight-gradient kernels and md_masked_sq_err.

The contract, the poison places and the launches are those of tests/nonfinite_cases.py (`check`): against the float64 reference of
the SAME poisoned operands nothing is hidden, nothing is invented (judged against the reference with inf -> NaN in the operand:
md_split makes (inf, NaN) of an inf), every other value is torch.equal to float64 on the exact cases -- bit-identical to the clean
launch or within the existing finite test's tolerance on the others -- and a sample or GroupNorm group without poison is
bit-identical to the clean launch.  tests/test_cpu_nonfinite_cases.py proves on the CPU that every launch here can fail.  Every
test prints the sizes of the three sets (hidden, invented, compared) before it asserts.  The launch code is that of the
neighbouring modules (test_gpu_conv_exact, test_gpu_attention, test_gpu_wgrad_exact, test_gpu_backward_kernels), imported.

Out of scope here:
  - training dropout in md_gn_apply / md_gn_bwd_apply: a dropped NaN becomes 0 by select where torch multiplies; settled by the
    mask contract of tests/test_gpu_dropout.py
  - the block pass: tests/test_gpu_block_pass.py::test_nan_and_inf_at_row_segment_and_tile_ends
  - the Winograd kernels: tests/test_gpu_nonfinite.py
  - the sampler kernels beyond tests/test_gpu_nonfinite.py, tests/test_gpu_guidance.py and tests/test_gpu_latent.py: still open
  - finite values beyond fp32's square root range in GroupNorm (|x| > 1.8e19): the statistics square in fp32, so the group's
    rstd becomes 0 and its outputs beta; here only finiteness of the output is demanded for x = 1e30 (still open)

Measured on an MI355X: see DESIGN.md, "Non-finite operands to the direct convs, attention, GroupNorm, wgrad and the loss"."""
import pytest
import torch
import torch.nn.functional as F

import attn_cases as ac
import conv_cases as cc
import nonfinite_cases as nf
import test_gpu_attention as ta
import test_gpu_backward_kernels as tb
import test_gpu_conv_exact as ce
import test_gpu_wgrad_exact as tw
import wgrad_cases as wc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NAN, INF = nf.NAN, nf.INF


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def bw(ops):
    from meshdiffusion_amd.lib.diffusion.models import backward
    return backward


def _same(a, b):
    """Bit-for-bit as values: equal where finite, and non-finite at the same positions."""
    return torch.equal(nf.bad(a), nf.bad(b)) and torch.equal(torch.nan_to_num(a, 0.0, 0.0, 0.0), torch.nan_to_num(b, 0.0, 0.0, 0.0))


# ---------------------------------------------------------------------------------------------------------------
# a. direct convs and GEMMs
# ---------------------------------------------------------------------------------------------------------------
RUNNERS = {"gemm": ce.gemm_run, "s2": ce.s2_run, "stem": ce.stem_run, "nin": ce.nin_run}


def _conv_launch(case, run, stats, ksplit=1):
    y, st = run(case, stats, ksplit)
    return ce._sel(case, y).cpu(), (None if st is None else ce._sel(case, st).cpu())


@pytest.mark.parametrize("case_id", nf.IDS)
def test_conv_poisoned_operand(ops, case_id):
    """Launch A (NaN at `first`, +inf at `last`), launch B (-inf at `mid`) and the clean launch of the smallest spec of every
    (entry, cfg) pair and operand / output form; GroupNorm sums where the spec has them; the largest split-K of the spec equals
    the single pass, poison included.  The fp16x2 spec takes its operand from md_gn_apply(fp16=True): on the parent commit
    md_f2h made -65504 of the NaN there and this case failed (hidden)."""
    spec = nf.spec_of(case_id)
    run = RUNNERS[spec["entry"]](ops, spec)
    case = cc.build(spec)
    stats = bool(spec.get("stats"))
    others = range(1, case["B"])
    y0, st0 = _conv_launch(case, run, stats)
    msg = cc.describe_mismatch(y0, cc.reference(case).float(), case_id + " clean")
    assert not msg, msg
    for launch in nf.LAUNCHES:
        p = nf.poison(case, launch)
        ref, ref_sub = nf.references(p)
        what = f"{case_id} launch {launch}"
        y, st = _conv_launch(p, run, stats)
        nf.check(y, ref, ref_sub, y0, others, what)
        if st is not None:
            nf.check_stats(st, ref, st0, what)
        if spec.get("ksplit"):
            ks = max(spec["ksplit"])
            yk, stk = _conv_launch(p, run, stats, ks)
            nf.check(yk, ref, ref_sub, y0, others, f"{what} ksplit={ks}")
            assert _same(yk, y), f"{what}: ksplit={ks} differs from the single pass"
            if stk is not None:
                _, st0k = _conv_launch(case, run, stats, ks)
                nf.check_stats(stk, ref, st0k, f"{what} ksplit={ks} (finish kernel)")


@pytest.mark.parametrize("case_id", [s["id"] for s in nf.SPECS if s.get("bias") == "sample"])
def test_conv_nan_in_per_sample_bias(ops, case_id):
    """A NaN in bias[1, row] poisons exactly that (sample, row)."""
    spec = nf.spec_of(case_id)
    run = RUNNERS[spec["entry"]](ops, spec)
    case = cc.build(spec)
    y0, _ = _conv_launch(case, run, False)
    p = nf.poison(case, ("bias", 1, case["cout"] - 1))
    ref, ref_sub = nf.references(p)
    y, _ = _conv_launch(p, run, False)
    nf.check(y, ref, ref_sub, y0, [0], f"{case_id} NaN in bias[1, {case['cout'] - 1}]")
    assert bool(nf.bad(y[1, case["cout"] - 1]).all()) and int(nf.bad(y).sum()) == y[1, 0].numel()


@pytest.mark.parametrize("case_id", [s["id"] for s in nf.SPECS if s.get("res") == "sample"])
def test_conv_nan_in_residual(ops, case_id):
    """A NaN in res[1, row, voxel] poisons exactly that voxel."""
    spec = nf.spec_of(case_id)
    run = RUNNERS[spec["entry"]](ops, spec)
    case = cc.build(spec)
    D, H, W = case["dims"]
    y0, _ = _conv_launch(case, run, False)
    vox = (D - 1, H // 2, W - 2)
    p = nf.poison(case, ("res", 1, 3, vox))
    ref, ref_sub = nf.references(p)
    y, _ = _conv_launch(p, run, False)
    nf.check(y, ref, ref_sub, y0, [0], f"{case_id} NaN in res[1, 3, {vox}]")
    assert int(nf.bad(y).sum()) == 1


def test_fp16x2_nan_weight(ops):
    """The fp16x2 weight pack (md_split_f16 in md_pack.h / pack_batch.hip): a NaN in w[co0, ci0, tap] makes row co0 non-finite
    wherever the tap reaches the grid.  On the parent commit md_f2h packed -65504 for it and the row came out finite (hidden)."""
    spec = next(s for s in nf.SPECS if s.get("prec") == "fp16x2")
    run = ce.gemm_run(ops, spec)
    case = cc.build(spec)
    y0, _ = _conv_launch(case, run, False)
    p = nf.poison(case, ("w", 7, 11, (0, 1, 2)))
    ref, ref_sub = nf.references(p)
    y, _ = _conv_launch(p, run, False)
    nf.check(y, ref, ref_sub, y0, [], f"{spec['id']} NaN in w[7, 11, (0, 1, 2)]")
    rows = [r for r in range(case["cout"]) if r != 7]
    assert torch.equal(y[:, rows], y0[:, rows])


def test_bf16x3_nan_weight(ops):
    """The same through md_split of the bf16x3 pack (the control of the test above)."""
    spec = nf.spec_of("gemm-CFG_C3_128_FAST-hi_only-8x8x8-32-128-B2")
    run = ce.gemm_run(ops, spec)
    case = cc.build(spec)
    y0, _ = _conv_launch(case, run, False)
    p = nf.poison(case, ("w", 7, 11, (0, 1, 2)))
    ref, ref_sub = nf.references(p)
    y, _ = _conv_launch(p, run, False)
    nf.check(y, ref, ref_sub, y0, [], f"{spec['id']} NaN in w[7, 11, (0, 1, 2)]")


@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_conv3_head_poisoned_operand(ops, value):
    """md_conv3_head (GroupNorm affine + SiLU in the loader, then md_fold_dx) with the launch of
    tests/test_gpu_kernels.py::test_conv3_head_fused_kernel at its smallest shape, the affine taken from the CLEAN tensor.  Not an
    exact case: outside the reference's non-finite set the clean launch computes the same value, so the output is bit-identical
    to it there (no tolerance is needed)."""
    B, cin, S, co = 2, 64, 8, 4
    r = lambda shape, seed, scale=1.0: torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    x = r((B, cin, S, S, S), 90) * 1.5 + 0.2
    gamma, beta = 1.0 + 0.2 * r((cin,), 91), 0.5 * r((cin,), 92)
    w, bias = r((co, cin, 3, 3, 3), 93, 0.05), r((co,), 94)
    clean = [(ops.ncdhw_to_f32b(x.cuda()), cin)]
    _, acd = ops.gn_params(clean, gamma.cuda(), beta.cuda(), B, S ** 3, want_ac=True)
    w2 = w.permute(0, 4, 1, 2, 3).reshape(co * 3, cin, 3, 3, 1).contiguous().cuda()
    pw = ops.PackedWeight(w2, "conv", ops.CFG_HEAD_PACK, "cuda")
    head = lambda t: ops.fold_dx(ops.conv3_head(pw, ops.ncdhw_to_f32b(t.cuda()), acd, B, S, 16), bias.cuda(), B, co, 3, 16, S).cpu()
    y0 = head(x)
    a64 = acd.cpu().double().view(B, cin, 2)
    for ch, vox in ((0, (0, 0, 0)), (cin - 1, (S - 1, S - 1, S - 1)), (cin // 2, (S // 2, S // 2, S // 2))):
        xb = x.clone()
        xb[(0, ch) + vox] = value
        refs = [F.conv3d(F.silu(t.double() * a64[..., 0, None, None, None] + a64[..., 1, None, None, None]), w.double(), bias.double(), padding=1)
                for t in (xb, nf.nan_sub(xb))]
        nf.check(head(xb), refs[0], refs[1], y0, [1], f"md_conv3_head {value} at channel {ch} voxel {vox}", exact=False,
                 same_as_clean=~nf.bad(refs[1]))


# ---------------------------------------------------------------------------------------------------------------
# b. attention
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(nf.ATTN_CASES))
def test_attention_poisoned_operands(ops, name):
    """md_attn_fwd and the unfused chain (GEMM, md_softmax_keys, GEMM) on exact operands with one NaN / +-inf in q, v or k of
    sample 0: NaN in q[c, i0] -> column i0; in v[c0, key0] -> channel c0, every query; in k[c0, key0] -> all of sample 0; +-inf
    in k: nothing hidden against `ref`, nothing invented against `ref_sub`.  Everything outside the non-finite set is
    bit-identical to the clean launch (it computes the same value there), on both paths."""
    case = nf.ATTN_CASES[name]()
    qk, vT = ta._pack(ops, case)
    clean = {"fused": ta._fused(ops, case, qk, vT), "unfused": ta._unfused(ops, case, qk, vT)[0]}
    for pname, operand, where, value in nf.attn_poisons(case["N"]):
        p = nf.attn_apply(case, operand, where, value)
        ref, ref_sub = nf.attn_references(p)
        qk, vT = ta._pack(ops, p)
        for path, out in (("fused", ta._fused(ops, p, qk, vT)), ("unfused", ta._unfused(ops, p, qk, vT)[0])):
            what = f"{name} {pname} {path}"
            nf.check(out, ref, ref_sub, clean[path], range(1, case["B"]), what, exact=False, same_as_clean=~nf.bad(ref_sub), names=("b", "c", "query"))
            if value != value:
                assert torch.equal(nf.bad(out), nf.attn_expected(case, operand, where)), f"{what}: the non-finite set is not the expected one"


# ---------------------------------------------------------------------------------------------------------------
# c. softmax over keys on raw fp32 logits
# ---------------------------------------------------------------------------------------------------------------
def _softmax(ops, s32):
    B, nk, nq = s32.shape
    hi, lo = ac.s16b_planes(ops.softmax_keys(ac.block_keys(s32).cuda(), B, nk, nq))
    return (hi.double() + lo.double()).float()


@pytest.mark.parametrize("nk,nq,B", nf.SOFTMAX_SHAPES)
def test_softmax_keys_poisoned_logits(ops, nk, nq, B):
    """md_softmax_keys at the shapes of test_softmax_keys_uneven_key_slices.  Some keys of a column at -inf: p is exactly 0 there
    and the rest of the column within that test's own bound (ta._softmax_check: elementwise / column max <= 2e-5); a column
    entirely -inf: NaN as torch gives; one +inf or one NaN: the column is non-finite; all other columns bit-identical to clean."""
    s = nf.softmax_logits(nk, nq, B)
    clean = _softmax(ops, s)
    for pname, items in nf.softmax_poisons(nk, nq):
        sp = nf.softmax_apply(s, items)
        ref = torch.softmax(sp.double(), dim=1)
        got = _softmax(ops, sp)
        cols = torch.zeros_like(ref, dtype=torch.bool)
        cols[0, :, sorted({q for _, q, _ in items})] = True
        what = f"md_softmax_keys n_keys={nk} n_q={nq} B={B} {pname}"
        nf.check(got, ref, ref, clean, range(1, B), what, exact=False, same_as_clean=~cols, names=("b", "key", "query"))
        if pname == "some_ninf":
            for k, q, _ in items:
                assert float(got[0, k, q]) == 0.0, f"{what}: p[{k}, {q}] = {float(got[0, k, q])!r}, not exactly 0"
            err = float(((got.double() - ref).abs() / ref.amax(1, keepdim=True)).max())
            print(f"{what}: elementwise / column max {err:.3e}")
            assert err <= 2e-5


@pytest.mark.parametrize("nk,nq,B", nf.SOFTMAX_SHAPES)
def test_softmax_keys_bwd_poisoned_dp(ops, bw, nk, nq, B):
    """md_softmax_keys_bwd: a NaN in dp[key, q] makes column q of ds non-finite; the other columns are bit-identical."""
    s = nf.softmax_logits(nk, nq, B)
    p16 = ops.softmax_keys(ac.block_keys(s).cuda(), B, nk, nq)
    hi, lo = ac.s16b_planes(p16)
    p64 = hi.double() + lo.double()
    dp = torch.randn(B, nk, nq, generator=torch.Generator().manual_seed(nk + 1))

    def run(d):
        h, l = ac.s16b_planes(bw.softmax_keys_bwd(p16, ac.block_keys(d).cuda(), B, nk, nq, 0.0625))
        return (h.double() + l.double()).float()

    clean = run(dp)
    last = (min(nk // 8, 4) - 1) * 8 + 7
    for key, q in ((0, 4), (last, 21), (nk - 1, 30)):
        d = dp.clone()
        d[0, key, q] = NAN
        ref = 0.0625 * p64 * (d.double() - (p64 * d.double()).sum(1, keepdim=True))
        col = torch.zeros_like(ref, dtype=torch.bool)
        col[0, :, q] = True
        assert torch.equal(nf.bad(ref), col)
        nf.check(run(d), ref, ref, clean, range(1, B), f"md_softmax_keys_bwd n_keys={nk} NaN in dp[{key}, {q}]", exact=False, same_as_clean=~col,
                 names=("b", "key", "query"))


# ---------------------------------------------------------------------------------------------------------------
# d. AttnBlock
# ---------------------------------------------------------------------------------------------------------------
def test_attn_block_nan_stays_in_its_sample(ops):
    """The sharpened AttnBlock of test_attn_block_sharp_backward, forward and backward: a NaN in sample 0 of the input leaves
    sample 1's output and sample 1's input gradient bit-identical to the clean run (R4)."""
    Cc, S, B = 256, 8, 2
    blk, _ = ta._sharp_block(Cc)
    blk = blk.cuda().train()
    x, dy = ta._randn((B, Cc, S, S, S), 5), ta._randn((B, Cc, S, S, S), 6)

    def run(t):
        tape = []
        with torch.no_grad():
            y = blk.forward_blocked(ops.ncdhw_to_f32b(t.cuda()), B, S ** 3, tape=tape)
            dx = blk.backward_blocked(tape[0], ops.ncdhw_to_f32b(dy.cuda()))
        return ops.f32b_to_ncdhw(y, (S, S, S)).cpu(), ops.f32b_to_ncdhw(dx, (S, S, S)).cpu()

    y0, dx0 = run(x)
    xb = x.clone()
    xb[0, 77, 3, 4, 5] = NAN
    y, dx = run(xb)
    print(f"AttnBlock NaN in sample 0: non-finite outputs {int(nf.bad(y[0]).sum())} of {y[0].numel()} in sample 0, {int(nf.bad(y[1]).sum())} in sample 1; "
          f"input gradient {int(nf.bad(dx[0]).sum())} / {int(nf.bad(dx[1]).sum())}")
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(dx0).all())
    assert bool(nf.bad(y[0]).any()) and bool(nf.bad(dx[0]).any()), "the NaN is hidden in its own sample (R2)"
    assert torch.equal(y[1], y0[1]), "R4: sample 1's output changed"
    assert torch.equal(dx[1], dx0[1]), "R4: sample 1's input gradient changed"


# ---------------------------------------------------------------------------------------------------------------
# e. GroupNorm forward
# ---------------------------------------------------------------------------------------------------------------
GN_TOL = 1e-5            # rel-L2 of tests/test_gpu_kernels.py::test_groupnorm_silu_split (the S16B output: its hi + lo round trip alone is 2.4e-6)
GN_TOL_FP16 = 2.0 ** -11  # one fp16 rounding per element (RNE: half an ulp of 11 bits) bounds the rel-L2; the fp32 arithmetic in front adds < 1e-6


def _gn_run(ops, case, form):
    B, (D, H, W) = 2, case["grid"]
    P = D * H * W
    parts = [(ops.ncdhw_to_f32b(t.contiguous().cuda()), t.shape[1]) for t in torch.split(case["x"], case["parts"], dim=1)]
    prm = ops.gn_params(parts, case["gamma"].cuda(), case["beta"].cuda(), B, P)
    if form == "fp16":
        out = ops.gn_apply(parts, prm, B, P, norm=True, silu=True, fp16=True)
        y = out[:, :, 0].contiguous().view(torch.float16).float().permute(0, 1, 3, 2).reshape(B, nf.GN_C, D, H, W)
        return y.cpu(), None
    if form == "raw":
        out, raw = ops.gn_apply(parts, prm, B, P, norm=True, silu=True, want_raw=True)
        return ops.s16b_to_ncdhw(out, case["grid"]).cpu(), ops.s16b_to_ncdhw(raw, case["grid"]).cpu()
    return ops.s16b_to_ncdhw(ops.gn_apply(parts, prm, B, P, norm=True, silu=True), case["grid"]).cpu(), None


@pytest.mark.parametrize("form", ["split", "raw", "fp16"])
@pytest.mark.parametrize("two_parts", [False, True])
@pytest.mark.parametrize("grid", nf.GN_GRIDS)
def test_groupnorm_forward_poisoned_voxel(ops, grid, two_parts, form):
    """md_gn_stats + md_gn_finalize + md_gn_apply (norm + SiLU split; want_raw; the fp16 form) with x[0, c0, p0] in {NaN, +inf,
    -inf, 1e30}, p0 the first and the last voxel: non-finite over exactly (sample 0, group of c0), the raw output at exactly the
    voxel; 1e30 is finite in float64, so the output is finite; other groups and the other sample bit-identical to clean.  On the
    parent commit the fp16 form failed here: md_f2h wrote -65504 for every NaN of the group (hidden)."""
    case = nf.gn_case(grid, two_parts)
    y0, raw0 = _gn_run(ops, case, form)
    ref0 = nf.gn_reference(case)
    e0 = rel_l2(y0, ref0)
    print(f"GroupNorm {grid} parts {case['parts']} {form}: clean rel-L2 {e0:.3e}")
    assert e0 < (GN_TOL_FP16 if form == "fp16" else GN_TOL)
    for vname, value in nf.GN_VALUES.items():
        for last in (False, True):
            p = nf.gn_poison(case, value, last)
            ref = nf.gn_reference(p)
            ref_sub = nf.gn_reference(dict(p, x=nf.nan_sub(p["x"])))
            group = nf.gn_group_mask(p)
            y, raw = _gn_run(ops, p, form)
            what = f"GroupNorm {grid} parts {case['parts']} {form} {vname} at {p['vox']}"
            nf.check(y, ref, ref_sub, y0, [1], what, exact=False, same_as_clean=~group)
            if vname == "1e30":
                assert bool(torch.isfinite(y).all()), f"{what}: finite in float64, non-finite here"
            else:
                assert torch.equal(nf.bad(y), group), f"{what}: the non-finite set is not exactly (sample 0, group of c0)"
            if raw is not None:
                voxel = torch.zeros_like(group)
                voxel[(0, case["c0"]) + p["vox"]] = True
                assert torch.equal(nf.bad(raw), voxel & (vname != "1e30")), f"{what}: the raw output is not non-finite at exactly the voxel"
                assert torch.equal(raw[~voxel], raw0[~voxel]), f"{what}: the raw output changed away from the voxel"
                if vname == "1e30":
                    assert float(raw[voxel]) == 1e30 or abs(float(raw[voxel]) / 1e30 - 1) <= 2.0 ** -17


@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_gn_finalize_poisoned_group_params(ops, value):
    """md_gn_stats + md_gn_finalize on their own: the (mean, rstd * gamma, beta, rstd) rows and the folded affine (a, c) of the
    poisoned (sample, group) are non-finite in mean, a, rstd and in both of (a, c), as the float64 statistics are (mean NaN or
    +-inf, variance NaN); every other row is bit-identical to the clean launch.  The output of md_gn_apply alone cannot see a
    variance clamp that maps NaN to 0: the NaN mean poisons it either way."""
    case = nf.gn_case((4, 4, 4), False)
    B, P = 2, 64

    def run(c):
        parts = [(ops.ncdhw_to_f32b(c["x"].cuda()), nf.GN_C)]
        prm, acd = ops.gn_params(parts, c["gamma"].cuda(), c["beta"].cuda(), B, P, want_ac=True)
        return prm.cpu(), acd.cpu()

    prm0, ac0 = run(case)
    p = nf.gn_poison(case, value, True)
    prm, acd = run(p)
    xg = p["x"].double().reshape(B, nf.GN_GROUPS, -1)
    assert bool(nf.bad(xg.mean(2)[0, p["c0"] // 2])) and bool(torch.isnan(xg.var(2, unbiased=False)[0, p["c0"] // 2]))
    rows = nf.gn_group_mask(p)[:, :, 0, 0, 0]                                # [B, C]
    want = torch.stack([rows, rows, torch.zeros_like(rows), rows], -1)
    print(f"md_gn_finalize {value}: non-finite params {int(nf.bad(prm).sum())} (expected {int(want.sum())}), affine {int(nf.bad(acd).sum())} (expected {2 * int(rows.sum())})")
    assert torch.equal(nf.bad(prm), want), "params: the non-finite set is not (mean, a, rstd) of the poisoned group's rows"
    assert torch.equal(nf.bad(acd), torch.stack([rows, rows], -1)), "the folded affine is not non-finite in exactly the poisoned group's rows"
    assert torch.equal(prm[~want], prm0[~want]) and torch.equal(acd[~rows], ac0[~rows])


# ---------------------------------------------------------------------------------------------------------------
# f. GroupNorm backward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [NAN, INF])
@pytest.mark.parametrize("cparts", [(32,), (32, 32)])
def test_groupnorm_backward_poisoned_dy(ops, bw, cparts, value):
    """md_gn_bwd_stats / _finalize / _apply through backward.gn_backward at the smallest shape of test_gn_backward (4^3, SiLU) with
    B = 2, and with two channels per group over two parts: one NaN / +inf voxel of dy.  dx is non-finite over exactly that (sample,
    group) and bit-identical to clean elsewhere; dgamma / dbeta, the channel sums (sample 0) and the amax word follow the float64
    formula of that test (tb._gn_ref).  amax: the bit pattern of max |dx| over the non-NaN elements (md_absmax: NaN never wins,
    +inf does)."""
    B, grid, silu = 2, (4, 4, 4), True
    C, P = sum(cparts), 64
    x, dy, gamma, beta = tb._gn_inputs("randn", B, C, P, 100 + C + P)
    c0, p0 = C - 3, 37
    dyb = dy.clone()
    dyb[0, c0, p0] = value
    parts = [(tb._f32b(ops, t.reshape(B, c, *grid)), c) for t, c in zip(torch.split(x, list(cparts), 1), cparts)]
    gn = tb._gn_module(C, gamma, beta)
    params = ops.gn_params(parts, gn.weight, gn.bias, B, P, eps=gn.eps, groups=32)
    single = len(cparts) == 1

    def run(d):
        gn.weight.grad, gn.bias.grad = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        sums = torch.zeros((B, C), device="cuda") if single else None
        outs = bw.gn_backward(parts, tb._f32b(ops, d.reshape(B, C, *grid)), params, gn, B, P, silu, sums_out=sums, want_amax=single)
        got = torch.cat([tb._from_f32b(ops, o, grid).reshape(B, c, P) for o, c in zip(outs, cparts)], 1)
        word = outs[0]._md_amax.cpu().view(torch.float32) if single else None
        return got, gn.weight.grad.cpu(), gn.bias.grad.cpu(), (sums.cpu() if single else None), word

    dx0, dg0, db0, cs0, _ = run(dy)
    dx, dg, db, cs, word = run(dyb)
    ref, rdg, rdb = tb._gn_ref(x, dyb, params.cpu(), gamma, 32, silu)
    cpg = C // 32
    group = torch.zeros_like(ref, dtype=torch.bool)
    group[0, (c0 // cpg) * cpg:(c0 // cpg + 1) * cpg] = True
    assert torch.equal(nf.bad(ref), group)
    what = f"gn_backward C={cparts} {value} in dy[0, {c0}, {p0}]"
    nf.check(dx, ref, ref, dx0, [1], what + " dx", exact=False, same_as_clean=~group, names=("b", "c", "p"))
    for name, got, want, clean in (("dgamma", dg, rdg, dg0), ("dbeta", db, rdb, db0)):
        nf.check(got, want, want, clean, [], f"{what} {name}", exact=False, same_as_clean=~nf.bad(want), names=("c",))
        assert bool(nf.bad(want[c0])) and int(nf.bad(want).sum()) == 1
    if single:
        rs = ref.sum(2)
        nf.check(cs, rs, rs, cs0, [1], what + " ch_sums", exact=False, same_as_clean=~nf.bad(rs), names=("b", "c"))
        finite_max = dx[~torch.isnan(dx)].abs().max()
        print(f"{what}: amax word {float(word)!r}, max |dx| over the non-NaN elements {float(finite_max)!r}")
        assert torch.equal(word.view(torch.int32), finite_max.reshape(1).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------
# g. weight gradients
# ---------------------------------------------------------------------------------------------------------------
ROW_END_OPEN = pytest.mark.xfail(strict=True, reason="md_wgrad, S % 8 != 0: the masked dY position behind a row's end (a zero) meets the row's last "
                                "activation voxel in the MFMA, 0 * NaN = NaN in the dx = -1 taps that never reach it; the A fragment is shared with "
                                "live positions, so only predication inside the MFMA main loop could remove it (DESIGN.md: open)")
WINO_ACT_OPEN = pytest.mark.xfail(strict=True, reason="md_wgrad_wino: F(2, 3) along w -- the output transform dg2 = (n1 + n2) / 2 - n3 carries the NaN of a "
                                 "position pair into the dx tap that never reaches it, and the y halo of dY is a multiplied zero: 18 taps of the "
                                 "column instead of 8.  Inherent in the transform and the MFMA contraction (DESIGN.md: open)")


@pytest.mark.parametrize("entry,which", [(e, w) for e in ("pb", "nin") for w in ("dy", "act")] + [("wino", "dy"), ("wino", "act_dilated"),
                                                                                                 pytest.param("wino", "act", marks=WINO_ACT_OPEN),
                                                                                                 pytest.param("pb", "act_row_end", marks=ROW_END_OPEN)])
def test_wgrad_poisoned_operand(ops, bw, entry, which):
    """md_wgrad (27 taps), md_wgrad_wino, md_wgrad_nin at their smallest spec with B >= 2: a NaN in dy[0, co0, interior voxel] ->
    dW[co0, :, :]; a NaN in act[0, ci0, corner voxel] -> dW[:, ci0, the taps that reach it].  The dy poison is interior only (at
    least one voxel from every face): at a face the answer depends on whether padding is a multiplied zero or an absent term,
    and neither is wrong.  Set equality with wgrad_cases.reference, torch.equal elsewhere, the sentinel margin untouched; also
    at the largest ksplit of the spec.  md_wgrad's 4^3 spec walks stages of 8 dY positions over rows of 4: the loader zeroes the
    activation window behind what live positions read, so the zeros of the masked positions do not meet the NEXT row's voxels (the
    corner case failed before that: 256 invented); the row's own last voxel is still met (`act_row_end`, open).
    md_wgrad_wino cannot meet the activation case as stated (`act`, open); `act_dilated` holds it to what a Winograd kernel with a
    multiplied-zero halo can give, the analogue of R3's dilation in tests/test_gpu_nonfinite.py: nothing hidden, and non-finites
    only inside column ci0 of dW (any tap)."""
    spec = nf.wgrad_spec(entry)
    case = wc.build(spec)
    p = nf.wgrad_poison(case, "act" if which == "act_dilated" else which)
    ref, ref_sub = nf.references(p)
    if which == "act_dilated":
        ref_sub = ref.clone()
        ref_sub[:, 9, :] = NAN
    prepare = {"pb": lambda: tw._prepare_pb(ops, bw), "wino": lambda: tw._prepare_wino(ops, verify=False), "nin": lambda: tw._prepare_nin(ops)}[entry]()
    launch = prepare(p)
    idx = wc.dw_index(case) + wc.MARGIN
    outside = torch.ones(int(idx.max()) + 1 + wc.MARGIN, dtype=torch.bool)
    outside[idx.reshape(-1)] = False
    splits = [spec["ksplit"][0]] + ([max(k for k in spec["ksplit"] if k is not None)] if any(k is not None for k in spec["ksplit"][1:]) else [])
    for ks in splits:
        buf = wc.dw_buffer(case, case["dw0"]).cuda()
        launch(buf[wc.MARGIN:], ks)
        got = buf.cpu()
        nf.check(got[idx.reshape(-1)].reshape(idx.shape), ref, ref_sub, None, [], f"{spec['id']} NaN in {which}, ksplit={ks}", names=("co", "ci", "tap"))
        assert bool((got[outside] == wc.SENTINEL).all()), f"{spec['id']}: floats outside the addressed elements of dW changed"


# ---------------------------------------------------------------------------------------------------------------
# h. the loss
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked_in", [True, False])
def test_masked_sq_err_poisoned_eps_hat(hip_lib, masked_in):
    """md_masked_sq_err at the shape of test_perturb_bit_exact_and_masked_loss (B = 3): a NaN in eps_hat of sample 0 at a voxel
    with mask 1 and at one with mask 0.  Reference: the float64 expression of oracle/unet_oracle.py's loss, where the mask is a
    FACTOR (0 * NaN = NaN).  Sample 0's sum and the gradient voxel follow it; the other samples' sums and gradients are
    bit-identical to clean."""
    from meshdiffusion_amd.lib.diffusion import losses
    case = nf.loss_case()
    run = lambda c: tuple(t.cpu() for t in losses.masked_sq_err(c["eh"].cuda(), c["noise"].cuda(), c["mask"].reshape(-1).cuda(), want_grad=True,
                                                                   gscale=c["gscale"]))
    s0, g0 = run(case)
    p = nf.loss_poison(case, masked_in)
    rs, rg = nf.loss_reference(p)
    s, g = run(p)
    what = f"md_masked_sq_err NaN at a voxel with mask {int(masked_in)}"
    nf.check(s, rs, rs, s0, [1, 2], what + " sums", exact=False, same_as_clean=~nf.bad(rs), names=("b",))
    nf.check(g, rg, rg, g0, [1, 2], what + " grad", exact=False, same_as_clean=~nf.bad(rg))
