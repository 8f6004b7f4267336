"""layers.fold_upsample_weight: the 3x3x3 conv on a nearest-x2 upsampled input as four phase convs on the SOURCE rows.

Output plane Z = 2z + a reads source planes z - 1, z, z + 1 with the pre-summed taps (w0, w1 + w2, 0) for a = 0 and (0, w0 + w1, w2)
for a = 1, likewise along h with Y = 2y + b; the w axis keeps its three taps on the upsampled row.  The zero padding agrees on both
sides (Z + kd - 1 = -1 <=> z - 1 = -1, Z + kd - 1 = D <=> z + 1 = D / 2), which the sources of edge 2 below exercise at every border.
On small integers every sum is exact, so the two sides must be EQUAL; on random float64 input they differ by the reassociation of
at most four taps (bound 1e-12, float64 has 2^-53)."""
import pytest
import torch
import torch.nn.functional as F

from meshdiffusion_amd.lib.diffusion.models.layers import fold_upsample_weight

CIN, COUT = 3, 5
SOURCES = [(2, 3, 4), (4, 4, 4)]


def _reference(x, w):
    return F.conv3d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)


def _phases(x, wf, cout):
    """The four phase convs on the source (d, h) rows and the x2-along-w row, scattered to (2z + a, 2y + b)."""
    B, _, Ds, Hs, Ws = x.shape
    xw = x.repeat_interleave(2, dim=4)
    out = torch.full((B, cout, 2 * Ds, 2 * Hs, 2 * Ws), float("nan"), dtype=x.dtype)
    for a in (0, 1):
        for b in (0, 1):
            p = 2 * a + b
            out[:, :, a::2, b::2, :] = F.conv3d(xw, wf[p * cout:(p + 1) * cout], padding=1)
    return out


def _ints(shape, seed):
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed)).double()


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: "x".join(map(str, s)))
def test_phase_convs_equal_the_upsampled_conv_on_integers(src):
    x, w = _ints((2, CIN) + src, 1), _ints((COUT, CIN, 3, 3, 3), 2)
    ref, got = _reference(x, w), _phases(x, fold_upsample_weight(w), COUT)
    assert float(ref.abs().max()) > 0 and torch.equal(got, ref)


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: "x".join(map(str, s)))
def test_phase_convs_match_the_upsampled_conv_on_random_input(src):
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, CIN) + src, generator=g, dtype=torch.float64)
    w = torch.randn((COUT, CIN, 3, 3, 3), generator=g, dtype=torch.float64)
    ref, got = _reference(x, w), _phases(x, fold_upsample_weight(w), COUT)
    rel = float((got - ref).norm() / ref.norm())
    print(f"source {src}: rel-L2 {rel:.2e}")
    assert rel <= 1e-12


def test_row_order_dead_taps_and_sums():
    w = torch.randn((COUT, CIN, 3, 3, 3), generator=torch.Generator().manual_seed(4))
    wf = fold_upsample_weight(w)
    assert wf.shape == (4 * COUT, CIN, 3, 3, 3) and wf.dtype == torch.float32 and wf.is_contiguous()
    live = {0: (0, 1), 1: (1, 2)}
    for a in (0, 1):
        for b in (0, 1):
            blk = wf[(2 * a + b) * COUT:(2 * a + b + 1) * COUT]
            for kd in range(3):
                for kh in range(3):
                    if kd in live[a] and kh in live[b]:
                        continue
                    assert bool((blk[:, :, kd, kh, :] == 0).all()), (a, b, kd, kh)      # the five dead (kd, kh) taps: exact zeros
            assert sum(1 for kd in range(3) for kh in range(3) if not (kd in live[a] and kh in live[b])) == 5
    # fixed order: kd first, then kh, in fp32 -- restated for every live tap of every phase
    along = {0: lambda v, d: [v.select(d, 0), v.select(d, 1) + v.select(d, 2), None],
             1: lambda v, d: [None, v.select(d, 0) + v.select(d, 1), v.select(d, 2)]}
    for a in (0, 1):
        for b in (0, 1):
            blk = wf[(2 * a + b) * COUT:(2 * a + b + 1) * COUT]
            for kd, vd in enumerate(along[a](w, 2)):
                if vd is None:
                    continue
                for kh, vh in enumerate(along[b](vd, 2)):      # vd: [Cout, Cin, 3 (kh), 3 (kw)]
                    if vh is not None:
                        assert torch.equal(blk[:, :, kd, kh, :], vh), (a, b, kd, kh)
    # phase (0, 0) keeps w[0, 0] alone at its corner tap, phase (1, 1) keeps w[2, 2]
    assert torch.equal(wf[:COUT, :, 0, 0], w[:, :, 0, 0]) and torch.equal(wf[3 * COUT:, :, 2, 2], w[:, :, 2, 2])
