"""What the direct attention tests (tests/test_gpu_attention.py) rest on, proven without a GPU:
every case builder of tests/attn_cases.py is in the regime it claims (replay of the kernel's rescale schedule,
exact representability), the float64 references agree with the oracle's formulation, and a float64 emulation of
the kernel's loop shows that the three rescale mutations move the output of the rescale cases far beyond the
tolerance the GPU tests apply."""
import pytest
import torch

import attn_cases as ac

TOL_MFMA = 3e-5


@pytest.mark.parametrize("case_id", ac.EXACT_IDS)
def test_exact_case_is_exact_and_in_its_regime(case_id):
    case = ac.exact_case(case_id)
    assert case["name"] == case_id
    for name in ("q", "k", "v"):
        assert ac.bf16_exact(case[name]), f"{case_id}: {name} is not bf16-representable"
        hi, lo = ac.split_bf16(case[name])
        assert torch.equal(hi, case[name]) and not bool(lo.any())
    for b in range(case["B"]):
        # the fp32 logits the kernel forms (products and 256-term sums) are the float64 ones
        l32 = (case["k"][b].t() @ case["q"][b]) * float(ac.SCALE)
        l64 = ac.logits64(case["q"][b], case["k"][b])
        assert torch.equal(l32.double(), l64)
        out, p, rep = ac.analyse(case, b, l64)
        ac.check_precondition(case, b, rep)
        # the levels that carry mass stay within a few hundred log2 units of 0
        assert float((l64 * ac.LOG2E).abs()[p > 1e-6].max()) < 300.0


def test_randn_case_regime():
    case = ac.randn_case()
    spreads = []
    for b in range(case["B"]):
        qh, ql = ac.split_bf16(case["q"][b]); kh, kl = ac.split_bf16(case["k"][b])
        l64 = ac.logits64(qh.double() + ql.double(), kh.double() + kl.double())
        _, p, rep = ac.analyse(case, b, l64)
        ac.check_precondition(case, b, rep)
        tv = l64 * ac.LOG2E
        spreads.append(float((tv.amax(0) - tv.amin(0)).median()))
    assert 30.0 <= min(spreads) and max(spreads) <= 45.0, spreads


def test_case_ids_match_builders():
    assert len(ac.EXACT_IDS) == len(ac.EXACT_CASES) == len(set(ac.EXACT_IDS))
    assert set(ac.UNFUSED_IDS) <= set(ac.EXACT_IDS)


def test_reference_matches_oracle_formulation():
    """attention64 against oracle.unet_oracle.attn_block's own einsum + F.softmax lines, in float64."""
    from oracle import unet_oracle as uo  # noqa: F401  (the formulation restated below is attn_block's, lines 77-79)
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    B, C, N = 2, 256, 128
    q, k, v = (torch.randn(B, C, N, generator=g, dtype=torch.float64) for _ in range(3))
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    w = torch.einsum("bcq,bck->bqk", q, k) * (int(C) ** (-0.5))
    w = F.softmax(w, dim=-1)
    ref = torch.einsum("bqk,bck->bcq", w, v + bias[None, :, None])      # NIN_2's bias is part of v in the oracle
    got = torch.stack([ac.attention64(ac.logits64(q[b], k[b]), v[b], bias)[0] for b in range(B)])
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12


def test_oracle_attn_block_agrees_with_reference_through_the_block():
    """The same through the oracle's function itself: identity GroupNorm / NINs turn attn_block into x + attention(x)."""
    from oracle import unet_oracle as uo
    g = torch.Generator().manual_seed(4)
    B, C, S = 1, 32, 4
    x = torch.randn(B, C, S, S, S, generator=g, dtype=torch.float64)
    eye = torch.eye(C, dtype=torch.float64)
    bv = torch.randn(C, generator=g, dtype=torch.float64)
    sd = {"GroupNorm_0.weight": torch.ones(C, dtype=torch.float64), "GroupNorm_0.bias": torch.zeros(C, dtype=torch.float64),
          "NIN_0.W": eye, "NIN_0.b": torch.zeros(C, dtype=torch.float64), "NIN_1.W": eye, "NIN_1.b": torch.zeros(C, dtype=torch.float64),
          "NIN_2.W": eye, "NIN_2.b": bv, "NIN_3.W": eye, "NIN_3.b": torch.zeros(C, dtype=torch.float64)}
    ref = uo.attn_block(sd, x) - x
    h = uo.group_norm(x, sd["GroupNorm_0.weight"], sd["GroupNorm_0.bias"]).reshape(B, C, -1)
    got = ac.attention64(ac.logits64(h[0], h[0], scale=C ** -0.5), h[0], bv)[0].reshape(ref.shape[1:])
    assert float((got - ref[0]).abs().max() / ref.abs().max()) < 1e-12


def test_bf16x3_restatement_equals_exact_when_lo_is_zero():
    case = ac.exact_case("mixed-N512-B1")
    qh, ql = ac.split_bf16(case["q"][0]); kh, kl = ac.split_bf16(case["k"][0])
    assert torch.equal(ac.logits64_bf16x3(qh, ql, kh, kl), ac.logits64(case["q"][0], case["k"][0]))
    # and differs from it by exactly the dropped lo*lo term otherwise
    r = ac.randn_case(N=128, B=1)
    qh, ql = ac.split_bf16(r["q"][0]); kh, kl = ac.split_bf16(r["k"][0])
    full = ac.logits64(qh.double() + ql.double(), kh.double() + kl.double())
    kept = ac.logits64_bf16x3(qh, ql, kh, kl)
    lolo = ac.logits64(ql, kl)
    assert float((full - kept - lolo).abs().max()) < 1e-12 and float(lolo.abs().max()) > 0


def test_split_and_layout_helpers():
    x = torch.randn(4, 64, 32, generator=torch.Generator().manual_seed(5))
    hi, lo = ac.split_bf16(x)
    assert float((hi.double() + lo.double() - x.double()).abs().max() / x.abs().max()) < 2.0 ** -16
    assert torch.equal(ac.unblock_keys(ac.block_keys(x)), x)


@pytest.mark.parametrize("case_id,flags,least", [
    ("plateau_spike-N1024-B3", dict(skip_oacc=True), 1.0),
    ("plateau_spike-N1024-B3", dict(skip_l=True), 0.5),
    ("plateau_spike-N128-B1", dict(skip_oacc=True), 1.0),
    ("rising-N1024-B3", dict(skip_oacc=True), 1e-2),
    ("mixed-N512-B1", dict(skip_l=True), 0.5),
])
def test_emulated_mutations_move_the_output(case_id, flags, least):
    """float64 emulation of the kernel's loop: unmodified it reproduces the reference to 1e-13; with a rescale
    mutation the elementwise error is at least `least` (the GPU tests assert 3e-5)."""
    case = ac.exact_case(case_id)
    ref, _, rep = ac.analyse(case, 0)
    plain = ac.emulate_kernel(rep["logits"], case["v"][0], case["bias"])
    assert ac.elementwise_err(plain[None], ref[None]) < 1e-13
    mut = ac.emulate_kernel(rep["logits"], case["v"][0], case["bias"], **flags)
    err = ac.elementwise_err(mut[None], ref[None])
    print(f"{case_id} {flags}: elementwise error {err:.3g}")
    assert err > least and err > 100 * TOL_MFMA


@pytest.mark.parametrize("case_id", ["rising-N1024-B3", "lazy-N4096-B1"])
def test_emulated_missing_rescale_overflows_fp32(case_id):
    """Never rescaling after tile 0 is exact in real arithmetic (and in float64 here); in the kernel's fp32 it shows where
    a query's logits rise by more than 128 log2 units after tile 0: p overflows and the output is not finite.  These two
    cases own that mutation; plateau_spike does not see it (p <= 2^16.05)."""
    case = ac.exact_case(case_id)
    ref, _, rep = ac.analyse(case, 0)
    m64 = ac.emulate_kernel(rep["logits"], case["v"][0], case["bias"], never_after0=True)
    assert ac.elementwise_err(m64[None], ref[None]) < 1e-12
    m32 = ac.emulate_kernel(rep["logits"], case["v"][0], case["bias"], never_after0=True, dtype=torch.float32)
    assert not bool(torch.isfinite(m32).all())
    ok32 = ac.emulate_kernel(rep["logits"], case["v"][0], case["bias"], dtype=torch.float32)
    assert ac.elementwise_err(ok32[None], ref[None]) < TOL_MFMA


def test_sharp_block_precondition():
    """NIN_0.W, NIN_1.W x SHARP_GAIN: the oracle's largest softmax weight exceeds 0.5 for a tenth of the queries
    (the unscaled sensitised state: 0.15 at most at S = 8)."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import layers
    blk = layers.AttnBlock(channels=256)
    sd = synth.sensitised_state_dict(blk.state_dict(), seed=4)
    for S, B in ((8, 2), (16, 1)):
        x = torch.randn((2, 256, S, S, S), generator=torch.Generator().manual_seed(5))[:B]
        plain = ac.oracle_max_weight(sd, x)
        sharp = ac.oracle_max_weight(ac.sharpen(sd), x)
        share = float((sharp > 0.5).double().mean())
        print(f"S={S}: largest weight plain {float(plain.max()):.3f}, sharp: share of queries above 0.5 = {share:.3f}")
        assert share >= 0.1
