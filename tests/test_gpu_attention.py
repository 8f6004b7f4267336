"""The attention kernels on their own, against float64, at the edges of the online softmax.

md_attn_fwd (fused, inference), md_softmax_keys / md_softmax_keys_bwd and the GEMM chain around them (training) are
called through hip_ops directly on packed operands.  The float64 reference is computed from the DE-QUANTISED operands
(hi + lo as the kernels read them), the error measure is elementwise (per sample max |got - ref| / max |ref|), and
every rescale case first asserts, on the CPU, that its inputs drive the kernel's lazy-rescale schedule the way its
name says (attn_cases.replay / check_precondition; tests/test_cpu_attention_cases.py proves the same without a GPU).

Which path of the online softmax each case owns (waves x tiles; "live" = rescales after tile 0 with 0 < corr < 1):

  case                    N     B   regime
  plateau_spike-N128-B1   128   1   one visible rescale per query, in the first / middle / last third of the keys; one workgroup
  plateau_spike-N1024-B3  1024  3   the same + queries with TWO visible rescales (>= 1 % of the final mass in front of each)
  plateau_spike-N4096-B3  4096  3   the product shape; odd batch (sample = blockIdx.x % batch)
  rising-N*               <=1024    every tile after the first rescales live accumulators (8.66 log2 per tile)
  lazy-N*                           steps of 1.44 / 0.72 log2: m_run stays while p grows to 2^7.2, then one rescale;
                                    at N = 4096 the logits rise by 183 log2 in all (a missing rescale overflows fp32)
  falling-N512-B1                   maximum in tile 0, no rescale after it, later tiles underflow to p = 0
  dominant-N*                       one key with weight > 0.99 at position 0, 31, 32, N - 1
  mixed-N*                          gains 1, 2, 0.5, -1 in one wave: corr = 2^-8, 2^-16, 2^-4 and exactly 1 on one firing;
                                    the spike in either half of the lane pair (j, j + 32)
  uniform-N*                        all logits of a query equal: the control
  randn-N4096-B2                    ordinary operands (lo planes in use), logit spread ~37 log2, most waves rescale

Measured on an MI355X: see DESIGN.md, "Direct tests of the attention kernels".
Non-finite operands to the attention kernels: tests/test_gpu_nonfinite_kernels.py (on the exact cases of this module).
"""
import pytest
import torch

import attn_cases as ac
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL_MFMA = 3e-5          # the project's bound for a bf16x3 contraction (tests/test_gpu_kernels.py)
C = ac.AT_C


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


# ---------------------------------------------------------------------------------------------------------------
# packing, references
# ---------------------------------------------------------------------------------------------------------------
def _pack(ops, case):
    B, N = case["B"], case["N"]
    qk = ops.ncdhw_to_s16b(torch.cat([case["q"], case["k"]], 1).reshape(B, 2 * C, 1, 1, N).cuda(), 2 * C)     # [B][2C][N]
    vT = ops.ncdhw_to_s16b(case["v"].permute(0, 2, 1).reshape(B, N, 1, 1, C).cuda(), N)                       # [B][N][C]
    return qk, vT


def _dequantised(qk, vT):
    """(qhi, qlo, khi, klo, v) as the kernels read them: fp32 planes [B][C][N]; v = hi + lo in float64 [B][C][N]."""
    hi, lo = ac.s16b_planes(qk)
    vh, vl = ac.s16b_planes(vT)
    v = (vh.double() + vl.double()).permute(0, 2, 1).contiguous()
    return hi[:, :C], lo[:, :C], hi[:, C:], lo[:, C:], v


def _fused(ops, case, qk, vT):
    B, N = case["B"], case["N"]
    o = ops.attn_fwd(qk, vT, case["bias"].cuda(), B, C, N, ops.attn_scale(C))
    return ops.s16b_to_ncdhw(o, (1, 1, N)).cpu().reshape(B, C, N)


def _unfused(ops, case, qk, vT):
    """GEMM, md_softmax_keys, GEMM as AttnBlock.forward_blocked builds them with `tape` set; returns (o, P as S16B, S^T)."""
    B, N = case["B"], case["N"]
    dev = qk.device
    qk_bstride = (2 * C // 8) * 2 * N * 8
    k_view = qk.view(-1)[(C // 8) * 2 * N * 8:]
    sT = ops.f32b_empty(B, N, N, dev)
    ops.gemm_conv(cfg=ops.gemm_cfg_for(N, N), a=k_view, b=qk, out=sT, batch=B, rows=N, rows_alloc=N, kdim=C, dims=(1, 1, N),
                  a_src=ops.A_S16B, a_rows=N, a_bstride=qk_bstride, b_bstride=qk_bstride, alpha=ops.attn_scale(C))
    pr = ops.softmax_keys(sT, B, N, N)
    o = ops.s16b_empty(B, C, N, dev)
    ops.gemm_conv(cfg=ops.gemm_cfg_for(N, C), a=vT, b=pr, out=o, batch=B, rows=C, rows_alloc=C, kdim=N, dims=(1, 1, N),
                  a_src=ops.A_S16B, a_rows=C, a_bstride=(N // 8) * 2 * C * 8, bias=case["bias"].cuda(), out_mode=ops.OUT_S16B)
    return ops.s16b_to_ncdhw(o, (1, 1, N)).cpu().reshape(B, C, N), pr, sT


def _reference_exact(case, deq):
    """float64 reference of every sample from the de-quantised operands; asserts the precondition of each sample."""
    qh, ql, kh, kl, v = deq
    refs, logits = [], []
    for b in range(case["B"]):
        l64 = ac.logits64(qh[b].double() + ql[b].double(), kh[b].double() + kl[b].double())
        out, p, rep = ac.analyse(dict(case, v=v), b, l64)
        ac.check_precondition(case, b, rep)
        refs.append(out)
        logits.append(l64)
    return torch.stack(refs), logits


# ---------------------------------------------------------------------------------------------------------------
# A.1  fused kernel, exactly representable operands
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ac.EXACT_IDS)
def test_attn_fwd_exact_operands(ops, case_id):
    """Logits are exact in fp32, so what remains is the hi + lo split of P and V, v_exp_f32 and fp32 accumulation over
    N keys: TOL_MFMA on the elementwise measure.  Fails by a factor > 1e4 if a rescale is skipped or doubled
    (tests/test_cpu_attention_cases.py::test_emulated_mutations_move_the_output)."""
    case = ac.exact_case(case_id)
    qk, vT = _pack(ops, case)
    deq = _dequantised(qk, vT)
    assert torch.equal(deq[0], case["q"]) and torch.equal(deq[2], case["k"]) and not bool(deq[1].any()) and not bool(deq[3].any())
    assert torch.equal(deq[4], case["v"].double())
    ref, _ = _reference_exact(case, deq)             # precondition asserted before anything is launched
    got = _fused(ops, case, qk, vT)
    assert bool(torch.isfinite(got).all()), f"{case_id}: non-finite output"
    err = ac.elementwise_err(got, ref)
    print(f"md_attn_fwd {case_id}: elementwise {err:.3e}  rel-L2 {rel_l2(got, ref):.3e}")
    assert err < TOL_MFMA


# ---------------------------------------------------------------------------------------------------------------
# A.2  fused kernel, ordinary operands
# ---------------------------------------------------------------------------------------------------------------
def test_attn_fwd_randn_operands(ops):
    """Against the float64 restatement of the kernel's declared arithmetic (logits from hi*hi + hi*lo + lo*hi, all else
    exact) at TOL_MFMA, elementwise; the distance to exact float64 of the same operands is printed, not asserted."""
    case = ac.randn_case()
    B = case["B"]
    qk, vT = _pack(ops, case)
    qh, ql, kh, kl, v = _dequantised(qk, vT)
    refs, exact = [], []
    for b in range(B):
        l3 = ac.logits64_bf16x3(qh[b], ql[b], kh[b], kl[b])
        out, p, rep = ac.analyse(dict(case, v=v), b, l3)
        ac.check_precondition(case, b, rep)
        refs.append(out)
        exact.append(ac.attention64(ac.logits64(qh[b].double() + ql[b].double(), kh[b].double() + kl[b].double()), v[b], case["bias"])[0])
        absprod = (kh[b].abs().double().t() @ qh[b].abs().double()).max()
        delta = 2.0 ** -24 * 768 * float(absprod) * ac.SCALE
        print(f"sample {b}: live rescales {int(rep['live'].view(rep['live'].shape[0], -1, ac.AT_QW).any(2).sum())} over "
              f"{case['N'] // ac.AT_QW} waves; first-order worst-case fp32 accumulation bound e^(2 delta) - 1 = {2 * delta:.2e}")
    ref, exact = torch.stack(refs), torch.stack(exact)
    got = _fused(ops, case, qk, vT)
    err = ac.elementwise_err(got, ref)
    print(f"md_attn_fwd {case['name']}: vs bf16x3 restatement elementwise {err:.3e} rel-L2 {rel_l2(got, ref):.3e}; "
          f"vs exact float64 elementwise {ac.elementwise_err(got, exact):.3e}; restatement vs exact {ac.elementwise_err(ref, exact):.3e}")
    assert err < TOL_MFMA


# ---------------------------------------------------------------------------------------------------------------
# A.3  the unfused path on the same inputs
# ---------------------------------------------------------------------------------------------------------------
def _softmax_check(ops, logits64, tag):
    """md_softmax_keys on float64 logits rounded to fp32: [B][keys][queries]."""
    B, nk, nq = logits64.shape
    s32 = logits64.float()
    p16 = ops.softmax_keys(ac.block_keys(s32).cuda(), B, nk, nq)
    hi, lo = ac.s16b_planes(p16)
    got = hi.double() + lo.double()                                    # [B][keys][queries]
    ref = torch.softmax(s32.double(), dim=1)
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite softmax"
    err = float(((got - ref).abs() / ref.amax(1, keepdim=True)).max())
    sums = float((got.sum(1) - 1).abs().max())
    print(f"md_softmax_keys {tag}: elementwise / column max {err:.3e}, |column sum - 1| {sums:.3e}")
    assert err <= 2e-5 and sums <= 1e-5
    return p16, got


def _softmax_bwd_check(ops, p16, p64, dp, alpha, tag):
    """md_softmax_keys_bwd on the S16B P above.  Bound per case: the fp32 dot product over n_keys and the 2^-17 output
    split, n_keys * 2^-24 * max|dP| / max|ref| + 2^-16, from the inputs.  With a dominant key the exact gradient nearly
    vanishes (dP - tot cancels) and that bound is large; the per-column first-order bound below is asserted as well."""
    B, nk, nq = p64.shape
    from meshdiffusion_amd.lib.diffusion.models import backward as bw
    ds16 = bw.softmax_keys_bwd(p16, ac.block_keys(dp).cuda(), B, nk, nq, alpha)
    hi, lo = ac.s16b_planes(ds16)
    got = hi.double() + lo.double()
    dp64 = dp.double()
    ref = alpha * p64 * (dp64 - (p64 * dp64).sum(1, keepdim=True))
    colmax = ref.abs().amax(1, keepdim=True).clamp_min(1e-300)
    err = float(((got - ref).abs() / colmax).max())
    bound = float((nk * 2.0 ** -24 * dp64.abs().amax(1, keepdim=True) / colmax).max()) + 2.0 ** -16
    # The same reasoning with the factors the error of the dot product actually meets on its way into dS:
    # |tot_fp32 - tot| <= (n + 2) u sum_key |P dP| (u = 2^-24; + 2: the fp32 sum hi + lo), it enters dS[key] as alpha P[key] * that;
    # dv - tot, the two products and the split add (4 u + 2^-16) |ref|.
    u = 2.0 ** -24
    tight = (alpha * p64.amax(1, keepdim=True) * (nk + 2) * u * (p64 * dp64).abs().sum(1, keepdim=True) / colmax + 4 * u + 2.0 ** -16)
    ratio = float((((got - ref).abs() / colmax).amax(1, keepdim=True) / tight).max())
    print(f"md_softmax_keys_bwd {tag}: per-column elementwise {err:.3e}, derived bound {bound:.3e}; "
          f"largest error / per-column first-order bound {ratio:.3f}")
    assert bool(torch.isfinite(got).all())
    assert err <= bound
    assert ratio <= 1.0


@pytest.mark.parametrize("case_id", ac.UNFUSED_IDS)
def test_unfused_path_same_inputs(ops, case_id):
    case = ac.exact_case(case_id)
    B, N = case["B"], case["N"]
    qk, vT = _pack(ops, case)
    deq = _dequantised(qk, vT)
    ref, logits = _reference_exact(case, deq)
    l64 = torch.stack(logits)                                           # [B][keys][queries]
    # md_softmax_keys and its backward on their own
    p16, p64 = _softmax_check(ops, l64, case_id)
    g = torch.Generator().manual_seed(11)
    dp = torch.randn(B, N, N, generator=g)
    _softmax_bwd_check(ops, p16, p64, dp, ops.attn_scale(C), case_id + " dP=randn")
    offs = 100.0 * torch.randn(B, 1, N, generator=g)
    _softmax_bwd_check(ops, p16, p64, dp + offs, ops.attn_scale(C), case_id + " dP=randn+100*offset[q]")
    # the chain against the reference and against the fused kernel
    o_unf, _, _ = _unfused(ops, case, qk, vT)
    o_fus = _fused(ops, case, qk, vT)
    e_unf, e_x = ac.elementwise_err(o_unf, ref), ac.elementwise_err(o_fus, o_unf.double())
    print(f"unfused chain {case_id}: vs float64 {e_unf:.3e}; fused vs unfused {e_x:.3e}")
    assert e_unf < TOL_MFMA
    assert e_x <= 2 * TOL_MFMA


@pytest.mark.parametrize("nk,nq,B", [(40, 32, 2), (72, 64, 1), (8, 32, 1), (24, 32, 3), (264, 32, 1)])
def test_softmax_keys_uneven_key_slices(ops, nk, nq, B):
    """n_keys a multiple of 8 but not of 32: the four key slices of a workgroup are uneven, and with n_keys < 32 some are
    EMPTY (their running maximum stays at its initial value); n_q = 32 is one workgroup."""
    g = torch.Generator().manual_seed(nk)
    s = torch.randn(B, nk, nq, generator=g, dtype=torch.float64) * 6
    s[:, nk - 1, ::3] += 20.0                                           # a dominant key in the last (odd) block
    p16, p64 = _softmax_check(ops, s, f"n_keys={nk} n_q={nq} B={B}")
    dp = torch.randn(B, nk, nq, generator=g)
    _softmax_bwd_check(ops, p16, p64, dp, 0.0625, f"n_keys={nk} n_q={nq} B={B}")


def test_attention_entry_points_reject_unsupported_shapes(ops):
    """Argument checks only: nothing is launched."""
    from meshdiffusion_amd import _lib
    lib = _lib.load()
    t = torch.zeros(1 << 16, device="cuda")
    p = t.data_ptr()
    assert lib.md_attn_fwd(p, p, p, p, 1, 128, 128, 0.1, None) != 0          # C != 256
    assert lib.md_attn_fwd(p, p, p, p, 1, 256, 96, 0.1, None) != 0           # N % 128
    assert lib.md_attn_fwd(p, p, p, p, 0, 256, 128, 0.1, None) != 0
    assert lib.md_softmax_keys(p, p, 1, 12, 32, None) != 0                   # n_keys % 8
    assert lib.md_softmax_keys(p, p, 1, 16, 48, None) != 0                   # n_q % 32
    assert lib.md_softmax_keys_bwd(p, p, p, 1, 12, 32, 1.0, None) != 0
    assert lib.md_softmax_keys_bwd(p, p, p, 1, 16, 48, 1.0, None) != 0


# ---------------------------------------------------------------------------------------------------------------
# A.4  block level, sharp attention
# ---------------------------------------------------------------------------------------------------------------
def _sharp_block(Cc, seed=4):
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import layers
    blk = layers.AttnBlock(channels=Cc)
    sd = ac.sharpen(synth.sensitised_state_dict(blk.state_dict(), seed=seed))
    blk.load_state_dict(sd)
    return blk, sd


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def test_attn_block_sharp_forward(ops):
    """tests/test_gpu_unet.py::test_attn_block[256-16] with NIN_0.W, NIN_1.W x 3 (logits x 9): the oracle's largest softmax
    weight exceeds 0.5 for more than a tenth of the queries (sensitised weights alone: 0.04).  Same assertions."""
    from oracle import unet_oracle as uo
    Cc, S = 256, 16
    blk, sd = _sharp_block(Cc)
    x = _randn((2, Cc, S, S, S), 5)
    share = float((ac.oracle_max_weight(sd, x[:1]) > 0.5).double().mean())
    assert share >= 0.1, share
    blk = blk.cuda().eval()
    with torch.no_grad():
        y = blk(x.cuda()).cpu()
        ref = uo.attn_block(sd, x)
        ref64 = uo.attn_block({k: v.double() for k, v in sd.items()}, x.double())
    e, eb = rel_l2(y, ref), rel_l2(y - x, ref - x)
    print(f"sharp AttnBlock C={Cc} S={S}: share of queries with max weight > 0.5 = {share:.3f}; rel-L2 {e:.3e}, branch {eb:.3e}; "
          f"vs float64 oracle: HIP branch {rel_l2(y - x, ref64 - x.double()):.3e}, fp32 oracle branch {rel_l2(ref - x, ref64 - x.double()):.3e}")
    assert e < 1e-4
    assert eb < 5e-4
    ops.FUSE_ATTN = False
    try:
        with torch.no_grad():
            y2 = blk(x.cuda()).cpu()
    finally:
        ops.FUSE_ATTN = True
    e2 = rel_l2(y - x, y2 - x)
    print(f"  fused vs GEMM + softmax path: branch rel-L2 {e2:.3e}")
    assert e2 < 1e-4


def test_attn_block_sharp_backward(ops):
    """tests/test_gpu_backward.py::test_attn_block_backward at C = 256, S = 8 with the sharpened weights.  Same assertions."""
    from oracle import unet_oracle as uo
    Cc, S, B = 256, 8, 2
    TOL = 2e-4
    blk, sd = _sharp_block(Cc)
    x, dy = _randn((B, Cc, S, S, S), 5), _randn((B, Cc, S, S, S), 6)
    share = float((ac.oracle_max_weight(sd, x) > 0.5).double().mean())
    assert share >= 0.1, share
    blk = blk.cuda().train()
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    y_ref = uo.attn_block(sdr, xr)
    y_ref.backward(dy)
    tape = []
    with torch.no_grad():
        y = blk.forward_blocked(ops.ncdhw_to_f32b(x.cuda()), B, S ** 3, tape=tape)
        dx = blk.backward_blocked(tape[0], ops.ncdhw_to_f32b(dy.cuda()))
    y = ops.f32b_to_ncdhw(y, (S, S, S)).cpu()
    dx = ops.f32b_to_ncdhw(dx, (S, S, S)).cpu()
    params = dict(blk.named_parameters())
    names = ["NIN_0.W", "NIN_0.b", "NIN_1.W", "NIN_2.W", "NIN_2.b", "NIN_3.W", "NIN_3.b", "GroupNorm_0.weight", "GroupNorm_0.bias"]
    errs = {n: rel_l2(params[n].grad.cpu(), sdr[n].grad) for n in names}
    print(f"sharp AttnBlock backward C={Cc} S={S} B={B}: share {share:.3f}; forward {rel_l2(y, y_ref.detach()):.3e}, branch "
          f"{rel_l2(y - x, y_ref.detach() - x):.3e}; dx {rel_l2(dx, xr.grad):.3e}, branch {rel_l2(dx - dy, xr.grad - dy):.3e}; "
          + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert rel_l2(y, y_ref.detach()) < 1e-4 and rel_l2(y - x, y_ref.detach() - x) < 5e-4
    assert rel_l2(dx, xr.grad) < TOL
    assert rel_l2(dx - dy, xr.grad - dy) < 5e-4
    for n in names:
        assert errs[n] < 5e-4, n
    scale = float(sdr["NIN_0.b"].grad.abs().max())
    assert float(params["NIN_1.b"].grad.abs().max()) < 1e-2 * scale + 1e-4
