"""md_conv3_wino_upsfold: the f16f6 Upsample conv as four phase convs of 4 live (kd, kh) taps on the source rows
(layers.fold_upsample_weight; tests/test_cpu_ups_fold.py proves the fold itself).

Shapes are the smallest at which the kernel can go wrong: Cin 32 = one body of the K loop, 96 = three chunk pairs (both halo buffers
are refilled, the last body requests chunks that do not exist); Cout 256 = two channel blocks per phase; output grid (8, 16, 8) = one
source tile with every halo side padded, (16, 32, 16) = 2 x 2 x 2 source tiles with interior halos; a per-sample bias; with and
without GroupNorm sums.  hip_ops.UPS_FOLD_MIN_WGS only routes (layers.plan_conv3); the direct launches below do not consult it.

  exact inputs     small integers (tests/conv_cases.py, class f16: one fp16 holds every operand, also the sums of four taps): the fold
                   on either operand layout, the existing compact route and the float64 reference agree bit for bit
  random inputs    equalised f16f6: rel-L2 against float64 within TOL["f16f6"] and within 1.25 x the existing route's on the same inputs
                   (the fold removes roundings -- two to four products become one -- so the ratio is expected <= 1; 1.25 is seed scatter)
  non-finite       one NaN / +inf / -inf source voxel: rules R1 - R3 of tests/test_gpu_nonfinite.py, the other sample untouched
  routing          a calibrated layers.Upsample takes the fold at 256 workgroups and not at 128"""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from conftest import rel_l2
from test_gpu_nonfinite import TOL, VALUES, _check_spread

pytestmark = pytest.mark.gpu

# (cin, cout, output grid, B, statistics)
CASES = {
    "c32_r128_tile_b1": (32, 128, (8, 16, 8), 1, False),
    "c96_r256_tile_b2_stats": (96, 256, (8, 16, 8), 2, True),
    "c32_r256_grid_b1": (32, 256, (16, 32, 16), 1, False),
    "c96_r128_grid_b2_stats": (96, 128, (16, 32, 16), 2, True),
}


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def fold():
    from meshdiffusion_amd.lib.diffusion.models.layers import fold_upsample_weight
    return fold_upsample_weight


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _routes(ops, fold, x, w, bias, eq, B, cin, cout, dims, stats, routes=("fold_compact", "fold_full", "old")):
    """{route: (y [B, cout, D, H, W] on the CPU, sums or None)}: the fold on the compact and on the full operand, the existing
    compact route (md_conv3_wino_upsdh, 9 taps) -- same operand pass, same equaliser."""
    parts = [(ops.ncdhw_to_f32b(x.cuda()), cin)]
    ww = ops.WinoWeightF8(w.cuda(), "cuda", "f6", eq=eq)
    wf = ops.WinoWeightF8(fold(w).cuda(), "cuda", "f6", eq=eq)
    assert wf.rows == 4 * cout
    res = {}
    for name in routes:
        t = ops.wino_prep(parts, None, False, True, B, None, f8="f6", eq=eq, dims=dims, compact=name != "fold_full")
        st = torch.zeros((B, cout, 2), dtype=torch.float64, device="cuda") if stats else None
        kw = dict(bias=bias.cuda(), bias_bstride=cout, stats=st, dims=dims)
        out = ops.conv3_wino(ww, t, B, None, **kw) if name == "old" else ops.conv3_wino_upsfold(wf, t, B, None, **kw)
        res[name] = (ops.f32b_to_ncdhw(out, dims).cpu(), st.cpu() if stats else None)
    return res


def _check_sums(y, st, what):
    yd = y.double()      # the route's own output, the tolerance of tests/test_gpu_wino.py for the same quantity
    assert rel_l2(st[..., 0], yd.sum(dim=(2, 3, 4))) < 1e-6, what
    assert rel_l2(st[..., 1], (yd * yd).sum(dim=(2, 3, 4))) < 1e-6, what


@pytest.mark.parametrize("name", list(CASES))
def test_exact_inputs_bit_for_bit(ops, fold, name):
    cin, cout, dims, B, stats = CASES[name]
    case = cc.build(dict(id="ups_fold/" + name, cls="f16", B=B, parts=[cin], cout=cout, dims=dims, ups=1, bias="sample", seed=len(name) + cin))
    ref = cc.reference(case)
    assert float(ref.abs().max()) < cc.LIMIT
    got = _routes(ops, fold, case["x"], case["w"], case["bias"], None, B, cin, cout, dims, stats)
    for route, (y, st) in got.items():
        msg = cc.describe_mismatch(y.double(), ref, f"{name} / {route}")
        assert not msg, msg
        if stats:
            _check_sums(y, st, f"{name} / {route}")
    assert torch.equal(got["fold_compact"][0].view(torch.int32), got["fold_full"][0].view(torch.int32))


def _random_case(ops, cin, cout, dims, B, seed):
    D, H, W = dims
    x = _rand((B, cin, D // 2, H // 2, W // 2), seed) * torch.logspace(-1, 1, cin).view(1, cin, 1, 1, 1)
    w = _rand((cout, cin, 3, 3, 3), seed + 1, 0.05)
    bias = _rand((B, cout), seed + 2)
    ms = ops.wino_operand_ms([(ops.ncdhw_to_f32b(x.cuda()), cin)], None, False, B, (D // 2) * (H // 2) * (W // 2))
    eq = ops.wino_equaliser(None, None, w.cuda(), a2m=ms)      # the measured equaliser of the ORIGINAL weights, as the layer builds it
    return x, w, bias, eq


def _reference(x, w, bias):
    return F.conv3d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), padding=1) + bias.double()[:, :, None, None, None]


@pytest.mark.parametrize("name", list(CASES))
def test_random_inputs_equalised_f6(ops, fold, name):
    cin, cout, dims, B, stats = CASES[name]
    x, w, bias, eq = _random_case(ops, cin, cout, dims, B, 700 + cin + cout)
    ref = _reference(x, w, bias)
    got = _routes(ops, fold, x, w, bias, eq, B, cin, cout, dims, stats)
    e_new, e_old = rel_l2(got["fold_compact"][0], ref), rel_l2(got["old"][0], ref)
    print(f"ups fold {name}: rel-L2 vs float64 fold {e_new:.3e}, 9-tap route {e_old:.3e}, ratio {e_new / e_old:.3f}")
    assert torch.equal(got["fold_compact"][0].view(torch.int32), got["fold_full"][0].view(torch.int32))
    assert e_new < TOL["f16f6"] and e_new <= 1.25 * e_old
    if stats:
        for route in ("fold_compact", "fold_full"):
            _check_sums(*got[route], f"{name} / {route}")


@pytest.mark.parametrize("val", list(VALUES))
def test_nonfinite_source_voxel(ops, fold, val):
    cin, cout, dims, B = 96, 128, (16, 32, 16), 2
    x, w, bias, eq = _random_case(ops, cin, cout, dims, B, 900)
    xb = x.clone()
    xb[1, 17, 2, 5, 3] = VALUES[val]      # one source voxel = 8 upsampled ones, in sample 1
    ref = _reference(xb, w, bias)
    y = _routes(ops, fold, xb, w, bias, eq, B, cin, cout, dims, False, routes=("fold_compact",))["fold_compact"][0]
    y0 = _routes(ops, fold, x, w, bias, eq, B, cin, cout, dims, False, routes=("fold_compact",))["fold_compact"][0]
    e = _check_spread(y, ref, TOL["f16f6"], f"ups fold {val}")
    assert torch.equal(y[0].view(torch.int32), y0[0].view(torch.int32))
    print(f"ups fold, {val}: finite outputs vs float64 {e:.2e}")


def test_refuses_what_it_does_not_take(hip_lib):
    from meshdiffusion_amd import _lib
    B, cout, dims = 1, 128, (8, 16, 8)
    t = torch.zeros(1 << 20, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(B * cout * 8 * 16 * 8, dtype=torch.float32, device="cuda")

    def call(fmt, cin, residual=None, dims=dims):
        return hip_lib.md_conv3_wino_upsfold(_lib.WINO_FMT[fmt], t.data_ptr(), 0, t.data_ptr(), o.data_ptr(), None, 0, residual, 0, None, B, cin,
                                             cout, *dims, None)

    assert call("f6", 48) == -2                                    # no whole 32-channel body, as md_conv3_wino_f6
    assert call("f8", 32) == -2 and call(False, 32) == -2          # f16f6 only
    assert call("f6", 32, residual=o.data_ptr()) == -2             # no residual operand
    assert call("f6", 32, dims=(4, 16, 8)) == -2 and call("f6", 32, dims=(8, 8, 8)) == -2      # D / 2 % 4, H / 2 % 8


def test_calibrated_upsample_layer_takes_the_fold_at_256_workgroups(ops):
    """256 -> 256, 8^3 -> 16^3: B = 8 is 256 workgroups of the unfolded launch (the default floor: the fold), B = 4 is 128 (the existing
    route).  Both log an f16f6 Winograd launch; sample 0 of either against float64."""
    from meshdiffusion_amd.lib.diffusion.models import layers
    C, S = 256, 16
    x = _rand((8, C, S // 2, S // 2, S // 2), 620)
    up = layers.Upsample(C, with_conv=True)
    with torch.no_grad():
        up.Conv_0.weight.copy_(_rand((C, C, 3, 3, 3), 621, 0.05)); up.Conv_0.bias.copy_(_rand((C,), 622))
    up = up.cuda().eval()
    ops.CALIBRATE = {}
    try:
        with ops.precision_scope("f16f6"), torch.no_grad():
            up(x.cuda())
        cal = ops.CALIBRATE
    finally:
        ops.CALIBRATE = None
    for owner, site, tot, n in cal.values():
        owner._md_act_ms = {site: (tot / n).contiguous()}

    def run(t):
        ops.PROFILE = []
        try:
            with ops.precision_scope("f16f6"), torch.no_grad():
                y = up(t.cuda()).cpu()
            return y, [r[5] for r in ops.PROFILE if r[0] == "wino"]
        finally:
            ops.PROFILE = None

    ref0 = _reference(x[:1], up.Conv_0.weight.detach().cpu(), up.Conv_0.bias.detach().cpu()[None])
    y8, tags8 = run(x)
    y4, tags4 = run(x[:4])
    assert len(tags8) == 1 and tags8[0].endswith("/fold/f6"), tags8
    assert len(tags4) == 1 and tags4[0].endswith("/f6") and "/fold" not in tags4[0], tags4
    e8, e4 = rel_l2(y8[:1], ref0), rel_l2(y4[:1], ref0)
    print(f"calibrated Upsample 256 -> 256 @ 16^3: fold (B = 8) {e8:.3e}, 9-tap route (B = 4) {e4:.3e}, ratio {e8 / e4:.3f}")
    assert e8 < TOL["f16f6"] and e8 <= 1.25 * e4
