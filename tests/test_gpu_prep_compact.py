"""The compact operand of an Upsample conv (md_wino_prep_upsdh + md_conv3_wino_upsdh): T once per source (z', y') row instead
of the four identical rows of ups = 1.  Nothing may change: the compact T is rows (2z', 2y') of the full T, and the conv's output and
GroupNorm sums are the full layout's bit for bit, with and without a residual, on finite and non-finite operands.

Cin = 48 is no multiple of the conv's 32-channel pair-step (md_conv3_wino* answer MD_ERR_UNSUPPORTED in either layout): that case
checks the operand, and that both layouts are refused alike."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMS = [False, "f8", "f6"]


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _bits(t):
    return t.contiguous().view(torch.int32)


def _operands(ops, x, cin, B, dims, fmt):
    """(full T, compact T) of the nearest-x2 upsampled x as [B][cin/8][4][2][rows..][W/2][8] 16-bit views."""
    D, H, W = dims
    parts = [(ops.ncdhw_to_f32b(x.cuda()), cin)]
    tf = ops.wino_prep(parts, None, False, True, B, None, f8=fmt, dims=dims)
    full = tf.clone().view(torch.int16).view(B, cin // 8, 4, 2, D, H, W // 2, 8)
    tc = ops.wino_prep(parts, None, False, True, B, None, f8=fmt, dims=dims, compact=True)
    assert tc.numel() * 4 == tf.numel()
    comp = tc.clone().view(torch.int16).view(B, cin // 8, 4, 2, D // 2, H // 2, W // 2, 8)
    return parts, full, comp


def _conv_both(ops, x, w, B, cin, cout, dims, fmt, res):
    D, H, W = dims
    P = D * H * W
    parts = [(ops.ncdhw_to_f32b(x.cuda()), cin)]
    ww = ops.WinoWeightF8(w.cuda(), "cuda", fmt) if fmt else ops.WinoWeight(w.cuda(), "cuda")
    bias = _rand((B, cout), 7).cuda()
    res_f = ops.ncdhw_to_f32b(res.cuda()) if res is not None else None
    outs = []
    for compact in (False, True):
        t = ops.wino_prep(parts, None, False, True, B, None, f8=fmt, dims=dims, compact=compact)
        stats = torch.zeros((B, cout, 2), dtype=torch.float64, device="cuda")
        out = ops.conv3_wino(ww, t, B, None, bias=bias, bias_bstride=cout, residual=res_f, res_bstride=cout * P if res is not None else 0,
                             stats=stats, dims=dims)
        outs.append((out.clone(), stats.clone()))
    return outs


@pytest.mark.parametrize("fmt", FORMS)
@pytest.mark.parametrize("cin,dims", [(32, (8, 16, 16)), (48, (8, 16, 16)), (64, (8, 16, 16)), (128, (16, 16, 16))])
def test_compact_operand_is_the_even_rows_of_the_full_one(ops, fmt, cin, dims):
    B = 2
    D, H, W = dims
    x = _rand((B, cin, D // 2, H // 2, W // 2), 100 + cin) * torch.logspace(-3, 3, cin).view(1, cin, 1, 1, 1)
    _, full, comp = _operands(ops, x, cin, B, dims, fmt)
    assert torch.equal(comp, full[:, :, :, :, ::2, ::2])
    for i in (0, 1):
        for j in (0, 1):      # what the compact layout relies on: the four rows of the full operand are the same bits
            assert torch.equal(full[:, :, :, :, i::2, j::2], comp)


@pytest.mark.parametrize("fmt", FORMS)
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cin,dims", [(32, (8, 16, 16)), (64, (8, 16, 16)), (128, (16, 16, 16))])
def test_conv_on_compact_operand_is_bit_identical(ops, fmt, residual, cin, dims):
    B, cout = 2, 128
    D, H, W = dims
    x = _rand((B, cin, D // 2, H // 2, W // 2), 200 + cin)
    w = _rand((cout, cin, 3, 3, 3), 201, 0.05)
    res = _rand((B, cout, D, H, W), 202) if residual else None
    (o_full, s_full), (o_comp, s_comp) = _conv_both(ops, x, w, B, cin, cout, dims, fmt, res)
    assert bool(torch.isfinite(o_full).all()) and float(o_full.abs().max()) > 0
    assert torch.equal(o_full, o_comp) and torch.equal(_bits(o_full), _bits(o_comp))
    assert torch.equal(s_full, s_comp)


@pytest.mark.parametrize("fmt", FORMS)
def test_conv_refuses_cin_48_in_both_layouts(ops, hip_lib, fmt):
    B, cin, cout, dims = 2, 48, 128, (8, 16, 16)
    from meshdiffusion_amd import _lib
    t = torch.zeros(1 << 20, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(B * cout * 8 * 16 * 16, dtype=torch.float32, device="cuda")
    args = (t.data_ptr(), t.data_ptr(), o.data_ptr(), None, 0, None, 0, None, B, cin, cout, *dims)
    full = {False: lambda: hip_lib.md_conv3_wino(*args, 0, None), "f8": lambda: hip_lib.md_conv3_wino_f8(*args, None),
            "f6": lambda: hip_lib.md_conv3_wino_f6(*args, None)}[fmt]()
    assert full == -2 and hip_lib.md_conv3_wino_upsdh(_lib.WINO_FMT[fmt], *args, None) == -2


@pytest.mark.parametrize("fmt", FORMS)
def test_non_finite_operands_come_out_alike(ops, fmt):
    B, cin, cout, dims = 2, 32, 128, (8, 16, 16)
    D, H, W = dims
    x = _rand((B, cin, D // 2, H // 2, W // 2), 300)
    x[0, 3, 1, 2, 3] = float("nan")
    x[0, 17, 0, 0, 0] = float("inf")
    x[1, 8, 3, 7, 7] = float("-inf")
    x[1, 31, 2, 4, 0] = float("nan")
    _, full, comp = _operands(ops, x, cin, B, dims, fmt)
    assert torch.equal(comp, full[:, :, :, :, ::2, ::2])
    w = _rand((cout, cin, 3, 3, 3), 301, 0.05)
    for res in (None, _rand((B, cout, D, H, W), 302)):
        (o_full, s_full), (o_comp, s_comp) = _conv_both(ops, x, w, B, cin, cout, dims, fmt, res)
        assert not bool(torch.isfinite(o_full).all()) and bool(torch.isfinite(o_full[1, :, :, :]).any())
        for a, b in ((o_full, o_comp), (s_full, s_comp)):
            assert torch.equal(torch.isnan(a), torch.isnan(b))                                  # the positions of the NaNs
            assert torch.equal(torch.nan_to_num(a, nan=0.0, posinf=1e30, neginf=-1e30),
                               torch.nan_to_num(b, nan=0.0, posinf=1e30, neginf=-1e30))         # everything else, +-inf included


def test_unet_evaluation_is_bit_identical_with_the_compact_operand_switched_off(ops):
    """A U-Net small enough for a test whose 16^3 level is on the Winograd path (128 / 256 channels, B = 8) and whose Upsample conv
    (256 -> 256, 8^3 -> 16^3) therefore takes the compact operand: evaluated with it and with hip_ops.PREP_COMPACT_UPS off, before and
    after a calibration (which may move the Upsample conv from bf16x3 to the reduced-precision form, and audits it) -- the same bits."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    cfg = synth.small_config(image_size=16, nf=128, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=())
    cfg.device = torch.device("cuda")
    model = mutils.create_model(cfg).eval()
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(16))
    model.module.load_state_dict(sd, strict=True)
    x = synth.synthetic_inputs(8, 4, 16, seed=42).cuda()
    labels = torch.full((8,), 500.0, device="cuda")
    seen = []
    wino_prep = ops.wino_prep

    def spy(*a, **k):
        seen.append(bool(k.get("compact")))
        return wino_prep(*a, **k)

    def evaluate(compact):
        del seen[:]
        old = ops.PREP_COMPACT_UPS
        ops.PREP_COMPACT_UPS, ops.wino_prep = compact, spy
        try:
            with torch.no_grad():
                y = model(x, labels).clone()
        finally:
            ops.PREP_COMPACT_UPS, ops.wino_prep = old, wino_prep
        return y, sum(seen)

    for stage in ("uncalibrated", "calibrated"):
        y_on, n_on = evaluate(True)
        y_off, n_off = evaluate(False)
        assert bool(torch.isfinite(y_on).all())
        assert n_on == 1 and n_off == 0, (stage, n_on, n_off)          # the one Upsample conv of this U-Net
        assert torch.equal(y_on, y_off), stage
        if stage == "uncalibrated":      # measured equalisers + the audit (its bf16x3 repeat takes the audited launch's layout)
            xc = synth.synthetic_inputs(8, 4, 16, seed=77).cuda()
            rep = model.module.calibrate([xc], [torch.full((8,), 400.0, device="cuda")], bar=4e-5)
            assert rep["measured"] >= 1 and rep["audited"] >= 1
