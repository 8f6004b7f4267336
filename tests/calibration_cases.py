"""Inputs, float64 references and bounds of the calibration tests (tests/test_cpu_calibration_cases.py, tests/test_gpu_calibration.py):
GroupNorm(32) -> SiLU -> Conv3d(3x3x3) (+ per-sample bias, + residual) pairs on which the f16f6 arithmetic of the Winograd convs is
within its budget, and pairs on which it is not -- the operands DDPMUNet3D.calibrate exists for.

  friendly      i.i.d. weights, (gamma, beta) near (1, 0)
  span6 / span3 per-channel s = 2^U(-6,6) / 2^U(-3,3) on (gamma, beta), the weights divided by s (the gamma_span recipe of
                tests/test_gpu_wino.py): every channel matters equally, their activations differ by up to 2^12 / 2^6 inside one
                16-channel e2m3 block.  With the layer's equaliser the format is back in its budget, without it 3e-4 / 1e-4.
  residual30    span6 with a residual of 30 x the conv output's rms in the epilogue: an error relative to the launch's OUTPUT is
                diluted by sqrt(1 + 30^2)

Two sizes: "gpu" (B 2, 16^3, cout 128: what the Winograd kernels take) and "cpu" (8^3, cout 32: what the torch restatement of the
arithmetic in tests/test_gpu_wino.py evaluates in a second).  Everything is computed once per process and never modified."""
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

BAR = 4e-5                      # DDPMUNet3D.calibrate's default bar; the f16f6 budget of tests/test_gpu_wino.py
RESIDUAL_FACTOR = 30.0
SIZES = {"gpu": dict(B=2, S=16, cout=128), "cpu": dict(B=2, S=8, cout=32)}

# name: channel parts, span of the per-channel scale (log2), equaliser on, residual in the epilogue
LAYER_CASES = {
    "friendly": dict(cs=(128,), span=0.0, eq=True, residual=False),
    "span6_noeq": dict(cs=(128,), span=6.0, eq=False, residual=False),
    "span6_eq": dict(cs=(128,), span=6.0, eq=True, residual=False),
    "two_parts": dict(cs=(96, 32), span=3.0, eq=False, residual=False),
    "residual30": dict(cs=(128,), span=6.0, eq=False, residual=True),
}


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def span_scale(cin, span, seed):
    """s_c = 2^U(-span, span), one per channel (all ones for span 0)."""
    if not span:
        return torch.ones(cin)
    return torch.exp2((torch.rand(cin, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * span)


class LayerCase(NamedTuple):
    name: str
    cs: tuple                   # channels per input part
    cout: int
    S: int
    B: int
    eq: bool                    # the layer's equaliser (hip_ops.WINO_EQ) on
    xs: tuple                   # fp32 [B, c, S, S, S] per part
    gamma: torch.Tensor
    beta: torch.Tensor
    w: torch.Tensor             # [cout, cin, 3, 3, 3]
    bias: torch.Tensor          # [B, cout]: per sample, like a ResnetBlock's FiLM bias
    residual: object            # fp32 [B, cout, S, S, S] or None
    ref_in: torch.Tensor        # float64 silu(group_norm(cat(xs)))
    ref_conv: torch.Tensor      # float64 conv + bias
    ref: torch.Tensor           # float64 conv + bias + residual: what the launch writes


@functools.lru_cache(maxsize=None)
def layer_case(name, size="gpu", seed=1):
    c, z = LAYER_CASES[name], SIZES[size]
    B, S, cout, cs = z["B"], z["S"], z["cout"], c["cs"]
    cin = sum(cs)
    s = span_scale(cin, c["span"], 1000 + seed)
    w = randn((cout, cin, 3, 3, 3), 1100 + seed, 0.05) / s.view(1, -1, 1, 1, 1)
    gamma, beta = (1.0 + 0.2 * randn((cin,), 1200 + seed)) * s, 0.5 * randn((cin,), 1300 + seed) * s
    xs = tuple(randn((B, k, S, S, S), 1400 + 10 * seed + i) * (1.5 + i) + 0.3 for i, k in enumerate(cs))
    bias = randn((B, cout), 1500 + seed)
    ref_in = F.silu(F.group_norm(torch.cat(xs, 1).double(), 32, gamma.double(), beta.double(), eps=1e-6))
    ref_conv = F.conv3d(ref_in, w.double(), padding=1) + bias.double()[:, :, None, None, None]
    residual = None
    if c["residual"]:
        rms = ref_conv.pow(2).mean(dim=(1, 2, 3, 4), keepdim=True).sqrt()                    # per sample
        residual = (randn((B, cout, S, S, S), 1600 + seed).double() * rms * RESIDUAL_FACTOR).float()
    ref = ref_conv if residual is None else ref_conv + residual.double()
    return LayerCase(name, cs, cout, S, B, c["eq"], xs, gamma, beta, w, bias, residual, ref_in, ref_conv, ref)


def rel(a, b):
    """|a - b| / |b| in float64."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def triangle_bounds(e_r, e_b):
    """With r the exact result, y_r / y_b the reduced-precision / bf16x3 launches, e_r = |y_r - r| / |r|, e_b = |y_b - r| / |r|:
    |y_r - y_b| lies in [|y_r - r| - |y_b - r|, |y_r - r| + |y_b - r|] and |y_b| in [(1 - e_b) |r|, (1 + e_b) |r|], so the audit
    figure |y_r - y_b| / |y_b| lies in [(e_r - e_b) / (1 + e_b), (e_r + e_b) / (1 - e_b)]."""
    return (e_r - e_b) / (1.0 + e_b), (e_r + e_b) / (1.0 - e_b)


def emulated_f16f6(case):
    """The launch of `case` in the f16f6 arithmetic as tests/test_gpu_wino.py restates it in torch (float64 activation, the static
    equaliser's restatement where the case has it on), residual included: fp32 [B, cout, S, S, S]."""
    from test_gpu_wino import _conv_f16f6_reference, _equaliser_reference
    x, w = case.ref_in.float(), case.w
    if case.eq:
        eq, _ = _equaliser_reference(case.gamma, case.beta, case.w)
        eq = eq.view(1, -1, 1, 1, 1)
        x, w = x * eq, w / eq
    y = _conv_f16f6_reference(x, w) + case.bias[:, :, None, None, None]
    return y if case.residual is None else y + case.residual


# ---------------------------------------------------------------------------------------------------------------------------------
# whole-model cases: the smallest U-Net in which hip_ops.wino_ok (rows % 128, S % 8) holds at all -- 16^3 x 128 and 8^3 x 256
# levels, ResnetBlocks with and without a NIN shortcut, one Downsample, one Upsample conv, concatenated inputs
# ---------------------------------------------------------------------------------------------------------------------------------
MODEL = dict(image_size=16, nf=128, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=())
MODEL_LABELS = (900.0, 60.0)
POISONED_BLOCK = "all_modules.3"          # the first 16^3 ResnetBlock: 128 -> 128, identity shortcut = the residual of Conv_1's epilogue


def model_config(synth, precision):
    cfg = synth.small_config(**MODEL)
    cfg.model.hip_precision = precision
    return cfg


def model_state_dict(synth, template, seed=1234):
    return synth.sensitised_state_dict(template, seed=seed, grid_mask=synth.synthetic_grid_mask(MODEL["image_size"]))


def model_input(synth, seed=5):
    return synth.synthetic_inputs(len(MODEL_LABELS), 4, MODEL["image_size"], seed=seed)


def poison(sd, block, which, span=6.0, seed=77):
    """The span recipe on the GroupNorm_{which} / Conv_{which} pair of ResnetBlock `block` of a state dict: (gamma, beta) times s,
    the conv's input channels divided by s.  In exact arithmetic the block computes what it computed before only where SiLU is
    linear -- it is a DIFFERENT network; the oracle evaluates the poisoned state dict.  Returns a new dict."""
    out = {k: v.clone() for k, v in sd.items()}
    gw, gb, cw = f"{block}.GroupNorm_{which}.weight", f"{block}.GroupNorm_{which}.bias", f"{block}.Conv_{which}.weight"
    s = span_scale(out[gw].numel(), span, seed).to(out[gw].dtype)
    out[gw] = out[gw] * s
    out[gb] = out[gb] * s
    out[cw] = out[cw] / s.view(1, -1, 1, 1, 1)
    return out
