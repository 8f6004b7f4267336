"""CPU side of tests/test_gpu_nonfinite.py: the torch semantics its optimiser test relies on, and the raw-stream bound of the measured
Winograd equaliser (md_wino_equaliser_level_kernel with gamma = null) restated by test_gpu_wino._equaliser_reference."""
import torch

from test_gpu_wino import _equaliser_reference


def _clip(grads, max_norm=1.0):
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(ps, max_norm=max_norm)
    return [p.grad for p in ps]


def test_clip_grad_norm_nan_norm_poisons_every_gradient():
    g = [torch.randn(10, generator=torch.Generator().manual_seed(1)), torch.randn(3, 4, generator=torch.Generator().manual_seed(2))]
    g[1][2, 1] = float("nan")
    out = _clip(g)
    assert all(bool(torch.isnan(t).all()) for t in out)


def test_clip_grad_norm_inf_norm_zeroes_the_finite_gradients():
    g = [torch.randn(10, generator=torch.Generator().manual_seed(3)), torch.randn(3, 4, generator=torch.Generator().manual_seed(4))]
    g[0][4] = float("inf")
    out = _clip(g)
    assert bool(torch.isnan(out[0][4])) and int(torch.isnan(out[0]).sum()) == 1
    fin = torch.ones(10, dtype=torch.bool); fin[4] = False
    assert bool((out[0][fin] == 0).all()) and bool((out[1] == 0).all())


def test_clip_grad_norm_fp32_square_overflow_is_an_inf_norm():
    """1e20^2 does not fit fp32: torch's norm is inf and the clip coefficient 0 -- md_grad_sqnorm squares in fp32 too."""
    g = [torch.full((4,), 0.01)]
    g[0][1] = 1e20
    norm = torch.linalg.vector_norm(g[0])
    out = _clip(g)
    if bool(torch.isinf(norm)):
        assert bool((out[0] == 0).all())
    else:                          # a CPU norm that rescales: the device path is what the GPU test pins
        assert bool(torch.isfinite(out[0]).all())


def test_raw_stream_equaliser_bound():
    """gamma = beta = None (the raw stream in front of an Upsample conv): after the level shift, a channel at the largest measured rms R
    lands at most 2^5 above unit (eq_c R <= 2^5) -- a channel quiet at calibration (rms 1e-8) no longer gets 2^13 -- while a stream
    whose channels lie within 2^+-3 of each other is untouched by the bound."""
    cin, cout = 64, 128
    w = torch.randn((cout, cin, 3, 3, 3), generator=torch.Generator().manual_seed(5)) * 0.05
    a2 = torch.ones(cin)
    a2[5] = 1e-16
    eq, _ = _equaliser_reference(None, None, w, a2m=a2)
    R = float(a2.sqrt().max())
    assert float(eq[5]) * R <= 2.0 ** 5 and float(eq[5]) >= float(eq.median())
    assert float(eq[5] / eq.median()) <= 2.0 ** 6
    # ordinary spread: the same exponents as the rule without the raw-stream bound
    s = torch.exp2((torch.rand(cin, generator=torch.Generator().manual_seed(6)) * 2 - 1) * 3.0)
    a2s = s ** 2
    eq_s, ex = _equaliser_reference(None, None, w, a2m=a2s)
    e = torch.round(ex).clamp(-14, 14)
    u = -torch.round(torch.log2((torch.exp2(e) * a2s.double().sqrt()).max()))
    assert torch.equal(eq_s, torch.exp2(torch.minimum(e + u, torch.full_like(e, 14.0))).float())
