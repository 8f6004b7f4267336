"""md_conv3_wino_splitk: the Winograd conv on slices of the input channels + the split-K finish kernel (the 8^3-level route of
layers.plan_conv3; tests/test_cpu_wino_splitk.py has the gate and the address replay).

Shapes are the smallest that exercise each index the slices add:
    c64_ks2      Cin 64 in 2 slices of 2 chunks (9 pair-steps each), Cout 128, B = 1, 8^3: the slice's start inside the weight row block
    c128_ks4     Cin 128 in 4 slices, Cout 256 = two row blocks (their stride is the FULL step count), B = 2 (the (sample, slice)
                 split of the workgroup index and of the output slab); per-sample bias rows, per-sample residual, statistics
    c64_ks2_grid the first on an 8 x 16 x 8 grid (two tiles per sample: tile and slice indices do not mix)

  exact     small integers (tests/conv_cases.py): split, unsplit and float64 agree bit for bit in bf16x3, f16f8 and f16f6
  random    equalised f16f6: rel-L2 against float64 within TOL["f16f6"] = 4e-5 and within 1.25 x the unsplit route's on the same inputs
            (the bounds of tests/test_gpu_ups_fold.py; figures printed with -s)
  sums      the GroupNorm sums equal the sums of the returned tensor (1e-6, as tests/test_gpu_wino.py and test_gpu_ups_fold.py)
  nonfinite a NaN / +inf / -inf in one input channel of one slice: the non-finite outputs of the unsplit route, R1 - R3 of
            tests/test_gpu_nonfinite.py against float64, the other sample bit-identical to the clean run
  refusals  a workspace one byte short, ksplit = 1, cin = 96 in two slices: the error code, the output untouched
  routing   ResnetBlockDDPM 512 -> 512 at 8^3, B = 8: the new export with the switch on, md_gemm_conv with it off
  twice     two runs give the same bits (every test above that launches twice compares them; one test of its own with statistics)"""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from conftest import rel_l2
from test_gpu_nonfinite import TOL, VALUES, _check_spread

pytestmark = pytest.mark.gpu

# (cin, ksplit, cout, output grid, B, extras: per-sample bias + per-sample residual + statistics)
CASES = {
    "c64_ks2": (64, 2, 128, (8, 8, 8), 1, False),
    "c128_ks4": (128, 4, 256, (8, 8, 8), 2, True),
    "c64_ks2_grid": (64, 2, 128, (8, 16, 8), 1, False),
}
FORMS = {"bf16x3": (False, "hi_only"), "f16f8": ("f8", "f16"), "f16f6": ("f6", "f16")}      # name -> (fmt, exact class of conv_cases)


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _route(ops, fmt, x, w, eq, bias, res, dims, ks, stats):
    """(y [B, cout, D, H, W] on the CPU, sums [B, cout, 2] or None) of the unsplit launch (ks = 0) or of `ks` slices; the same
    operand pass, weights and equaliser either way.  bias [B, cout] and res [B, cout, D, H, W] per sample, or None."""
    B, cin = x.shape[:2]
    cout, (D, H, W) = w.shape[0], dims
    P = D * H * W
    ww = ops.WinoWeightF8(w.cuda(), "cuda", fmt, eq=eq) if fmt else ops.WinoWeight(w.cuda(), "cuda")
    t = ops.wino_prep([(ops.ncdhw_to_f32b(x.cuda()), cin)], None, False, False, B, None, f8=fmt, eq=eq, dims=dims)
    st = torch.zeros((B, cout, 2), dtype=torch.float64, device="cuda") if stats else None
    out = ops.f32b_empty(B, cout, P, "cuda")
    out.fill_(float("nan"))                       # a position the launch does not write cannot equal a reference
    kw = dict(bias=bias.cuda() if bias is not None else None, bias_bstride=cout if bias is not None else 0,
              residual=ops.ncdhw_to_f32b(res.cuda()) if res is not None else None, res_bstride=cout * P if res is not None else 0,
              stats=st, out=out, dims=dims)
    if ks:
        ops.conv3_wino_splitk(ww, t, B, None, ks, **kw)
    else:
        ops.conv3_wino(ww, t, B, None, **kw)
    return ops.f32b_to_ncdhw(out, dims).cpu(), (st.cpu() if stats else None)


def _bits(y):
    return y.contiguous().view(torch.int32)


def _check_sums(y, st, what):
    yd = y.double()
    assert rel_l2(st[..., 0], yd.sum(dim=(2, 3, 4))) < 1e-6, what
    assert rel_l2(st[..., 1], (yd * yd).sum(dim=(2, 3, 4))) < 1e-6, what


# ---- (a) exact inputs, (c) sums, (g) twice ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_exact_inputs_bit_for_bit(ops, name, form):
    cin, ks, cout, dims, B, extras = CASES[name]
    fmt, cls = FORMS[form]
    case = cc.build(dict(id=f"wino_splitk/{name}/{form}", cls=cls, B=B, parts=[cin], cout=cout, dims=dims,
                         bias="sample" if extras else None, res="sample" if extras else None, seed=len(name) + cin))
    ref = cc.reference(case)
    margin = cc.exactness_margin(case, "wino_f16" if fmt else "wino")
    assert margin["lolo_zero"] and margin["split_exact"] and max(margin["max_sum"].values()) < cc.LIMIT      # every partial sum is an exact integer
    args = (ops, fmt, case["x"], case["w"], None, case["bias"], case["res"], dims)
    y, st = _route(*args, ks, extras)
    msg = cc.describe_mismatch(y.double(), ref, f"{name} / {form} / {ks} slices")
    assert not msg, msg
    y1, _ = _route(*args, 0, False)
    assert torch.equal(_bits(y), _bits(y1)), f"{name} / {form}: the slices differ from the unsplit launch"
    assert torch.equal(_bits(y), _bits(_route(*args, ks, False)[0])), f"{name} / {form}: the same launch twice (with / without statistics) differs"
    if extras:
        _check_sums(y, st, f"{name} / {form}")


# ---- (b) random equalised f16f6, (c) sums ---------------------------------------------------------------------------
def _random_case(ops, cin, cout, dims, B, seed, extras):
    D, H, W = dims
    x = _rand((B, cin, D, H, W), seed) * torch.logspace(-1, 1, cin).view(1, cin, 1, 1, 1)
    w = _rand((cout, cin, 3, 3, 3), seed + 1, 0.05)
    bias = _rand((B, cout), seed + 2) if extras else None
    res = _rand((B, cout, D, H, W), seed + 3) if extras else None
    ms = ops.wino_operand_ms([(ops.ncdhw_to_f32b(x.cuda()), cin)], None, False, B, D * H * W)
    return x, w, bias, res, ops.wino_equaliser(None, None, w.cuda(), a2m=ms)      # the measured equaliser, as a calibrated layer builds it


def _reference(x, w, bias, res):
    y = F.conv3d(x.double(), w.double(), padding=1)
    if bias is not None:
        y = y + bias.double()[:, :, None, None, None]
    return y + res.double() if res is not None else y


@pytest.mark.parametrize("name", list(CASES))
def test_random_inputs_equalised_f6(ops, name):
    cin, ks, cout, dims, B, extras = CASES[name]
    x, w, bias, res, eq = _random_case(ops, cin, cout, dims, B, 1300 + cin + cout, extras)
    ref = _reference(x, w, bias, res)
    y, st = _route(ops, "f6", x, w, eq, bias, res, dims, ks, extras)
    y1, st1 = _route(ops, "f6", x, w, eq, bias, res, dims, 0, extras)
    e_new, e_old = rel_l2(y, ref), rel_l2(y1, ref)
    print(f"wino split-K {name}: rel-L2 vs float64 {ks} slices {e_new:.3e}, unsplit {e_old:.3e}, ratio {e_new / e_old:.3f}")
    assert e_new < TOL["f16f6"] and e_new <= 1.25 * e_old
    if extras:
        _check_sums(y, st, name)
        _check_sums(y1, st1, name + " (unsplit)")


# ---- (d) non-finite input ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("val", list(VALUES))
@pytest.mark.parametrize("form", ["bf16x3", "f16f6"])
def test_nonfinite_channel_of_one_slice(ops, form, val):
    cin, ks, cout, dims, B, _ = CASES["c128_ks4"]
    fmt = FORMS[form][0]
    x, w, bias, res, eq = _random_case(ops, cin, cout, dims, B, 1500, True)
    eq = eq if fmt else None
    xb = x.clone()
    xb[1, 70, 2, 5, 3] = VALUES[val]              # channel 70: slice 2 of 4 (channels 64 .. 95), sample 1
    ref = _reference(xb, w, bias, res)
    y, _ = _route(ops, fmt, xb, w, eq, bias, res, dims, ks, False)
    y1, _ = _route(ops, fmt, xb, w, eq, bias, res, dims, 0, False)
    y0, _ = _route(ops, fmt, x, w, eq, bias, res, dims, ks, False)
    assert torch.equal(~torch.isfinite(y), ~torch.isfinite(y1)), f"{form} {val}: the slices' non-finite outputs are not the unsplit route's"
    assert torch.equal(torch.isnan(y), torch.isnan(y1))
    e = _check_spread(y, ref, TOL[form], f"wino split-K {form} {val}")
    assert torch.equal(_bits(y[0]), _bits(y0[0]))
    print(f"wino split-K {form}, {val}: {int((~torch.isfinite(y)).sum())} non-finite outputs, finite ones vs float64 {e:.2e}")


# ---- (e) bad arguments ---------------------------------------------------------------------------------------------------
def test_refuses_what_it_does_not_take(hip_lib):
    from meshdiffusion_amd import _lib
    B, cout, dims, P = 1, 128, (8, 8, 8), 512
    t = torch.zeros(1 << 20, dtype=torch.bfloat16, device="cuda")
    o = torch.full((B * cout * P,), 7.0, device="cuda")
    ws = torch.zeros(4 * B * cout * P, dtype=torch.float32, device="cuda")

    def call(cin, ks, nbytes=None, fmt="f6", dims=dims, cout=cout, out=None, ws_ptr=None):
        need = hip_lib.md_conv3_wino_splitk_workspace_bytes(B, cout, *dims, max(ks, 2))
        return hip_lib.md_conv3_wino_splitk(_lib.WINO_FMT[fmt], t.data_ptr(), t.data_ptr(), ws.data_ptr() if ws_ptr is None else ws_ptr,
                                            need if nbytes is None else nbytes, o.data_ptr() if out is None else out, None, 0, None, 0, None,
                                            B, cin, cout, *dims, ks, None)

    assert hip_lib.md_conv3_wino_splitk_workspace_bytes(B, cout, *dims, 2) == 2 * B * cout * P * 4
    assert hip_lib.md_conv3_wino_splitk_workspace_bytes(B, cout, *dims, 1) == _lib.ERR_BAD_ARG
    assert call(64, 2, nbytes=2 * B * cout * P * 4 - 1) == _lib.ERR_BAD_ARG              # a workspace one byte short
    assert call(64, 1) == _lib.ERR_BAD_ARG and call(64, 0) == _lib.ERR_BAD_ARG            # not a split
    for fmt in (False, "f8", "f6"):
        assert call(96, 2, fmt=fmt) == _lib.ERR_UNSUPPORTED                               # slices of 48 channels: no whole pair-steps
    assert call(64, 4) == _lib.ERR_UNSUPPORTED                                            # slices of 16 channels
    assert call(64, 2, cout=192) == _lib.ERR_UNSUPPORTED and call(64, 2, dims=(4, 4, 8)) == _lib.ERR_UNSUPPORTED
    assert call(64, 2, out=o.data_ptr() + 4) == _lib.ERR_BAD_ARG and call(64, 2, ws_ptr=ws.data_ptr() + 8) == _lib.ERR_BAD_ARG
    assert call(64, 2, out=0) == _lib.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((ws == 0).all()), "a refused call launched something"


# ---- (f) routing -----------------------------------------------------------------------------------------------------------
def test_resnet_block_at_8_cubed_takes_the_slices(ops, hip_lib, monkeypatch):
    """512 -> 512 at 8^3, B = 8: 64 unsplit workgroups.  Switch on: both convs through md_conv3_wino_splitk (4 slices, f16f6), none
    through md_gemm_conv; switch off: both through md_gemm_conv.  The two results agree within the f16f6 tolerance."""
    from meshdiffusion_amd.lib.diffusion.models import layers
    C, S, B = 512, 8, 8
    blk = layers.ResnetBlockDDPM(act=torch.nn.SiLU(), in_ch=C, out_ch=C, temb_dim=None, dropout=0.0)
    with torch.no_grad():
        blk.Conv_0.weight.copy_(_rand((C, C, 3, 3, 3), 1701, 0.02)); blk.Conv_1.weight.copy_(_rand((C, C, 3, 3, 3), 1702, 0.02))
    blk = blk.cuda().eval()
    x = _rand((B, C, S, S, S), 1703).cuda()
    calls = {}
    for fn in ("md_conv3_wino_splitk", "md_gemm_conv", "md_conv3_wino_f6"):
        real = getattr(hip_lib, fn)
        monkeypatch.setattr(hip_lib, fn, lambda *a, _f=real, _n=fn: (calls.__setitem__(_n, calls.get(_n, 0) + 1), _f(*a))[1])

    def run(on):
        monkeypatch.setattr(ops, "WINO_SPLITK", on)
        calls.clear()
        ops.PROFILE = []
        try:
            with ops.precision_scope("f16f6"), torch.no_grad():
                y = blk(x).cpu()
            return y, dict(calls), [r[5] for r in ops.PROFILE if r[0] == "wino_splitk"], [r[5] for r in ops.PROFILE if r[0] == "wino"]
        finally:
            ops.PROFILE = None

    y_on, c_on, tags_on, wino_on = run(True)
    y_off, c_off, tags_off, wino_off = run(False)
    assert c_on == {"md_conv3_wino_splitk": 2}, c_on
    assert tags_on == ["512->512@8x8x8/ks4/stats/f6", "512->512@8x8x8/ks4/res/stats/f6"], tags_on
    assert c_off == {"md_gemm_conv": 2} and tags_off == [], (c_off, tags_off)
    assert wino_on == [] and wino_off == []      # "wino" records are launches of the conv kernel alone; conv + finish is a "wino_splitk" record
    e = rel_l2(y_on, y_off.double())
    print(f"ResnetBlock 512 -> 512 @ 8^3, B = 8: slices (f16f6) vs direct (bf16x3) rel-L2 {e:.3e}")
    # each conv is within its format's TOL of float64 on its own (the tests above); through two convs the first-order errors add
    assert e < 2 * (TOL["f16f6"] + TOL["bf16x3"])


# ---- (g) determinism -------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(ops):
    cin, ks, cout, dims, B, _ = CASES["c128_ks4"]
    x, w, bias, res, eq = _random_case(ops, cin, cout, dims, B, 1900, True)
    y, st = _route(ops, "f6", x, w, eq, bias, res, dims, ks, True)
    y2, st2 = _route(ops, "f6", x, w, eq, bias, res, dims, ks, True)
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(st.view(torch.int64), st2.view(torch.int64))
