"""The small-level launches of md_gemm_conv word for word: the 4^3-level 3x3x3 conv (MD_CFG_C3_LOW, fp32 parts through the GroupNorm +
SiLU loader, split-K; served by md_conv3_low_kernel) and the MD_CFG_G1_128 GEMM with F32B output, through hip_ops.gemm_conv on the
inputs of tests/small_level_cases.py.  Every fp32 word of the output must equal what the generic tile wrote on the commit before the
dedicated kernel existed (tests/golden/small_level_bits.npz, recorded by tools/gen_small_level_golden.py: one CRC-32 per (sample,
8-channel group) slab, the small outputs whole).  B = 1, 3, 5 leave part of a four-sample block empty; 72 + 184 channels put the part
boundary inside a 32-channel chunk; 100 rows of 104 leave rows_alloc above the rows; the GroupNorm gains span 2^6 and a hashed eighth of
the face voxels holds +-large values, so a halo entry from the wrong side or a rim that is not zero moves a sum by far more than a rounding.

The exact cases (small integers, tests/conv_cases.py) guard the golden itself: there the result must equal the float64 convolution."""
import os

import numpy as np
import pytest
import torch

import conv_cases as cc
import small_level_cases as sc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_level_bits.npz")


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case_id", sc.CONV_IDS + sc.GEMM_IDS)
def test_words_equal_the_generic_tile(ops, gold, case_id):
    words = sc.run(ops, sc.CASES[case_id])
    assert not np.isnan(words.view(np.float32)).any(), f"{case_id}: an output word was not written"
    if "whole/" + case_id in gold:
        want = gold["whole/" + case_id]
        bad = np.argwhere(words != want)
        assert not len(bad), (f"{case_id}: {len(bad)} of {want.size} words differ; first (b, group, position, channel) {bad[0].tolist()}: "
                              f"got {words.view(np.float32)[tuple(bad[0])]!r} want {want.view(np.float32)[tuple(bad[0])]!r}")
    msg = sc.describe(sc.slab_crcs(words), gold["crc/" + case_id])
    assert not msg, f"{case_id}: {msg}"


@pytest.mark.parametrize("spec", sc.EXACT, ids=[s["id"] for s in sc.EXACT])
def test_exact_on_small_integers(ops, spec):
    case = cc.build(spec)
    ref = cc.reference(case).float()
    B, cout, dims = case["B"], case["cout"], case["dims"]
    P = dims[0] * dims[1] * dims[2]
    rows_alloc = (cout + 7) // 8 * 8
    cfg = getattr(ops, spec["cfg"])
    kw = dict(cfg=cfg, batch=B, rows=cout, rows_alloc=rows_alloc, dims=dims)
    if case["bias"] is not None:
        kw.update(bias=case["bias"].cuda(), bias_bstride=cout if case["bias"].shape[0] > 1 else 0)
    if case["res"] is not None:
        kw.update(residual=ops.ncdhw_to_f32b(case["res"].cuda()), res_bstride=rows_alloc * P if case["res"].shape[0] > 1 else 0)
    if case["kshape"] == (1, 1, 1):
        pw = ops.PackedWeight(case["w"][:, :, 0, 0, 0].t().contiguous().cuda(), "nin", cfg, "cuda")
    else:
        pw = ops.PackedWeight(case["w"].cuda(), "conv", cfg, "cuda")
    if spec.get("b_f32"):
        parts = [(ops.ncdhw_to_f32b(t.cuda()), t.shape[1]) for t in case["x_raw"]]
        kw.update(b=None, b_f32=ops.F32Operand(parts, case["ac"].cuda() if case["ac"] is not None else None, silu=False))
    else:
        kw.update(b=ops.ncdhw_to_s16b(case["x"].cuda(), pw.kdim))
    outs = []
    for ks in (spec.get("ksplit", 1), spec.get("ksplit", 1)):        # twice: the same launch must repeat itself
        out = torch.full((B, rows_alloc // 8, P, 8), float("nan"), device="cuda")
        ops.gemm_conv(a=pw.data, out=out, kdim=pw.kdim, ksplit=ks, **kw)
        outs.append(ops.f32b_to_ncdhw(out, dims)[:, :cout].cpu())
    msg = cc.describe_mismatch(outs[0], ref, spec["id"])
    assert not msg, msg
    assert torch.equal(outs[0], outs[1]), f"{spec['id']}: the same launch twice differs"
