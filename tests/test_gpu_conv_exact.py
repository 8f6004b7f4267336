"""The convolution kernels bit for bit: every case of tests/conv_cases.py (small hashed integers, one live lo plane at most;
tests/test_cpu_conv_cases.py proves that the kernels' arithmetic is exact on them) through the entry point it names, on cubes and
on grids with three different extents, and torch.equal with the float64 convolution at EVERY voxel after the (exact) layout
conversion.  Split-K equals the single pass; the same launch twice is identical.  A failure prints how many elements differ,
where, and the first few values.

GroupNorm sums.  The kernels add a tile's (the split-K finish: a whole grid's) values and squares in fp32 before their float64
atomic, so on the ordinary cases (outputs ~1e5) the sums are held to what fp32 partial sums can lose (cc.stats_tolerance), and
every case with sums is launched a second time on its `tiny` twin (sum o^2 of a grid < 2^24), where they must equal the float64
(sum, sum of squares) of the reference EXACTLY -- one position left out or counted twice changes the integer.

The references are torch float64 on the CPU from the tensors the case builds; at 64^3 / 32^3 with 128 input channels only a few
output rows spread over the row tiles are checked (`ref_rows` of the case).

The loaders that round (arbitrary GroupNorm affine + SiLU: MD_B_F32B_GN of CFG_C3_128_FAST / CFG_C3_LOW, md_wino_prep* with
silu = 1, md_conv3_head) are checked per element through a TRANSPARENT conv (one power-of-two tap per row) against silu(x a + c)
in float64 and the bound derived in conv_cases.loader_bound / wino_transparent_bound; the zero rim must be exactly zero.  The
f16f8 / f16f6 operand passes are left out of that part (their cross-term images round the activation a second time)."""
import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


def _ids(*entries):
    return [s["id"] for s in cc.SPECS if s["entry"] in entries]


def _sel(case, t):
    """[B, rows_alloc, ...] -> the rows the reference has."""
    t = t[:, :case["cout"]]
    return t if case["rows"] is None else t[:, case["rows"]]


def _check(case, y, ref, what):
    msg = cc.describe_mismatch(_sel(case, y).cpu(), ref.float(), what)
    assert not msg, msg


def _check_stats(case, stats, ref, what, exact, whole_grid=False):
    got, want = _sel(case, stats.cpu()), cc.reference_stats(ref)
    if exact:
        msg = cc.describe_mismatch(got, want, what + ": GroupNorm (sum, sum of squares)")
        assert not msg, msg
    else:
        bad = (got - want).abs() > cc.stats_tolerance(ref, whole_grid)
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} GroupNorm sums beyond the fp32 partial-sum bound; first (b, row, which) "
                                     f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()!r} want {want[bad][0].item()!r}")


def _drive(spec, run):
    """run(case, stats: bool, ksplit: int) -> (NCDHW result on the device, stats tensor or None).  The checks every entry point gets."""
    for sp, exact in ((spec, False), (cc.stats_twin(spec), True)):
        if sp is None:
            continue
        case = cc.build(sp)
        ref = cc.reference(case)
        y1, st = run(case, bool(sp.get("stats")), 1)
        _check(case, y1, ref, sp["id"])
        if st is not None:
            _check_stats(case, st, ref, sp["id"], exact)
        y2, _ = run(case, False, 1)
        assert torch.equal(y2, y1), f"{sp['id']}: the same launch twice (with / without statistics) differs"
        for ks in sp.get("ksplit", []):
            yk, st = run(case, bool(sp.get("stats")), ks)
            _check(case, yk, ref, f"{sp['id']} ksplit={ks}")
            assert torch.equal(yk, y1), f"{sp['id']}: ksplit={ks} differs from the single pass"
            if st is not None:
                _check_stats(case, st, ref, f"{sp['id']} ksplit={ks} (finish kernel)", exact, whole_grid=True)


def _parts(ops, case):
    return [(ops.ncdhw_to_f32b(t.cuda()), t.shape[1]) for t in case["x_raw"]]


def _epilogue(ops, case, rows_alloc):
    """bias / residual launch arguments: (bias, bias_bstride, residual F32B, res_bstride)."""
    D, H, W = case["dims"]
    bias, bstride, res, rstride = None, 0, None, 0
    if case["bias"] is not None:
        bias, bstride = case["bias"].contiguous().cuda(), (case["cout"] if case["bias"].shape[0] > 1 else 0)
    if case["res"] is not None:
        assert rows_alloc == case["cout"]
        res, rstride = ops.ncdhw_to_f32b(case["res"].cuda()), (rows_alloc * D * H * W if case["res"].shape[0] > 1 else 0)
    return bias, bstride, res, rstride


def _zstats(B, rows_alloc):
    return torch.zeros((B, rows_alloc, 2), dtype=torch.float64, device="cuda")


def _nan_f32b(ops, B, rows_alloc, P):
    out = ops.f32b_empty(B, rows_alloc, P, "cuda")
    out.fill_(float("nan"))                       # a position the kernel does not write cannot equal the reference
    return out


# ---------------------------------------------------------------------------------------------------------------
# md_gemm_conv
# ---------------------------------------------------------------------------------------------------------------
XFOLD_CFGS = ("CFG_C3X_128_K16", "CFG_C5X_128")       # operand from md_ncdhw_to_s16b_xfold
FOLD_CFGS = ("CFG_C3X_32", "CFG_C5X_32_K16")           # result through md_fold_dx


def gemm_run(ops, spec):
    """The md_gemm_conv launcher of a "gemm" spec (tests/test_gpu_nonfinite_kernels.py launches poisoned cases through it too)."""
    cfg = getattr(ops, spec["cfg"])
    fast = spec["cfg"] == "CFG_C3_128_FAST"
    prec = ops.PREC_FP16X2 if spec.get("prec") == "fp16x2" else ops.PREC_BF16X3
    out_kind = spec.get("out", "f32b")

    def run(case, stats, ksplit):
        B, cin, cout, dims = case["B"], case["cin"], case["cout"], case["dims"]
        D, H, W = dims
        P = D * H * W
        x, w = case["x"].cuda(), case["w"]
        kw = dict(cfg=cfg, batch=B, dims=dims, ups=case["ups"], prec=prec)
        fold = False
        # ---- weights and the K they are packed for
        k = case["kshape"][0]
        if spec["cfg"] in XFOLD_CFGS:                       # dx-folded stem: K = 4 channels x k dx, taps k x k x 1
            w2 = w.permute(0, 1, 4, 2, 3).reshape(cout, cin * k, k, k, 1).contiguous()
            pw, rows, rows_alloc = ops.PackedWeight(w2.cuda(), "conv", cfg, "cuda"), cout, cout
        elif spec["cfg"] in FOLD_CFGS:                      # dx-folded head: rows = (co, kw); md_fold_dx adds the k columns + bias
            w2 = w.permute(0, 4, 1, 2, 3).reshape(cout * k, cin, k, k, 1).contiguous()
            pw, rows, rows_alloc, fold = ops.PackedWeight(w2.cuda(), "conv", cfg, "cuda"), cout * k, ((cout * k + 7) // 8) * 8, True
        elif case["kshape"] == (1, 1, 1):
            pw, rows, rows_alloc = ops.PackedWeight(w[:, :, 0, 0, 0].t().contiguous().cuda(), "nin", cfg, "cuda"), cout, cout
        else:
            pw, rows, rows_alloc = ops.PackedWeight(w.cuda(), "conv", cfg, "cuda", prec), cout, ((cout + 7) // 8) * 8
        # ---- operand
        if spec.get("b_f32"):
            kw.update(b=None, b_f32=ops.F32Operand(_parts(ops, case), case["ac"].cuda() if case["ac"] is not None else None, silu=False))
        elif spec["cfg"] in XFOLD_CFGS:
            kw.update(b=ops.ncdhw_to_s16b_xfold(x, k, pw.kdim))
        elif prec == ops.PREC_FP16X2:
            kw.update(b=ops.gn_apply(_parts(ops, case), None, B, P, norm=False, silu=False, fp16=True))
        else:
            kw.update(b=ops.ncdhw_to_s16b(x, pw.kdim))
        bias, bstride, res, rstride = (None, 0, None, 0) if fold else _epilogue(ops, case, rows_alloc)
        kw.update(a=pw.data, rows=rows, rows_alloc=rows_alloc, kdim=pw.kdim, bias=bias, bias_bstride=bstride, residual=res, res_bstride=rstride)
        if out_kind == "ncdhw":                             # rows 4 of rows_alloc 8, written straight to NCDHW
            out = torch.full((B, cout, D, H, W), float("nan"), device="cuda")
            ops.gemm_conv(out=out, out_mode=ops.OUT_NCDHW, **kw)
            return out, None
        if out_kind == "s16b":
            out = ops.s16b_empty(B, rows_alloc, P, "cuda")
            ops.gemm_conv(out=out, out_mode=ops.OUT_S16B, **kw)
            return ops.s16b_to_ncdhw(out, dims), None
        st = _zstats(B, rows_alloc) if stats and (fast or ksplit > 1) else None      # the dedicated kernel's epilogue, or the split-K finish
        out = ops.gemm_conv(out=_nan_f32b(ops, B, rows_alloc, P), ksplit=ksplit, stats=st, **kw)
        if fold:
            return ops.fold_dx(out, case["bias"].reshape(-1).cuda() if case["bias"] is not None else None, B, cout, k, rows_alloc, None, dims=dims), None
        return ops.f32b_to_ncdhw(out, dims), st

    return run


@pytest.mark.parametrize("case_id", _ids("gemm"))
def test_gemm_conv_exact(ops, case_id):
    spec = cc.spec_of(case_id)
    _drive(spec, gemm_run(ops, spec))


# ---------------------------------------------------------------------------------------------------------------
# the dedicated kernels
# ---------------------------------------------------------------------------------------------------------------
def s2_run(ops, spec=None):
    def run(case, stats, ksplit):
        B, cout, dims = case["B"], case["cout"], case["dims"]
        pw = ops.PackedWeight(case["w"].cuda(), "conv", ops.CFG_S2_PACK, "cuda")
        bias, bstride, _, _ = _epilogue(ops, case, cout)
        st = _zstats(B, cout) if stats else None
        out = ops.conv3_s2(pw, ops.ncdhw_to_f32b(case["x"].cuda()), B, None, bias=bias, bias_bstride=bstride, stats=st,
                           out=_nan_f32b(ops, B, cout, dims[0] * dims[1] * dims[2]), dims=dims)
        return ops.f32b_to_ncdhw(out, dims), st

    return run


@pytest.mark.parametrize("case_id", _ids("s2"))
def test_conv3_s2_exact(ops, case_id):
    """md_conv3_s2 on the raw fp32 tensor; the far-face zero padding sits in every tile position of the non-cubic grids."""
    _drive(cc.spec_of(case_id), s2_run(ops))


def stem_run(ops, spec=None):
    def run(case, stats, ksplit):
        B, cout, dims = case["B"], case["cout"], case["dims"]
        w2 = case["w"].permute(0, 1, 4, 2, 3).reshape(cout, 12, 3, 3, 1).contiguous().cuda()
        pw = ops.PackedWeight(w2, "conv", ops.CFG_C3X_128_K16, "cuda")
        bias, bstride, res, rstride = _epilogue(ops, case, cout)
        assert bstride == 0 and rstride == 0                  # the stem's bias and residual are batch-shared by construction
        st = _zstats(B, cout) if stats else None
        out = ops.conv3_stem(pw, ops.ncdhw_to_s16b_xfold(case["x"].cuda(), 3, 16), B, None, bias=bias, residual=res, stats=st, dims=dims)
        return ops.f32b_to_ncdhw(out, dims), st

    return run


@pytest.mark.parametrize("case_id", _ids("stem"))
def test_conv3_stem_exact(ops, case_id):
    """md_ncdhw_to_s16b_xfold + md_conv3_stem with the batch-shared residual and the GroupNorm sums."""
    _drive(cc.spec_of(case_id), stem_run(ops))


def nin_run(ops, spec=None):
    def run(case, stats, ksplit):
        pw = ops.PackedWeight(case["w"][:, :, 0, 0, 0].t().contiguous().cuda(), "nin", ops.CFG_G1_128, "cuda")
        B, P = case["B"], case["dims"][2]
        out = ops.nin_f32(_parts(ops, case), pw, case["bias"].reshape(-1).cuda(), B, P, out=_nan_f32b(ops, B, 128, P))
        return ops.f32b_to_ncdhw(out, case["dims"]), None

    return run


@pytest.mark.parametrize("case_id", _ids("nin"))
def test_nin_f32_exact(ops, case_id):
    """md_nin_f32: one and two parts, 128 and 256 channels, more tiles than workgroups (ragged) and fewer."""
    _drive(cc.spec_of(case_id), nin_run(ops))


# ---------------------------------------------------------------------------------------------------------------
# Winograd
# ---------------------------------------------------------------------------------------------------------------
def _wino_launch(ops, case, ww, t, stats, **extra):
    B, cout, dims = case["B"], case["cout"], case["dims"]
    bias, bstride, res, rstride = _epilogue(ops, case, cout)
    st = _zstats(B, cout) if stats else None
    out = _nan_f32b(ops, B, cout, dims[0] * dims[1] * dims[2])
    ops.conv3_wino(ww, t, B, None, bias=bias, bias_bstride=bstride, residual=res, res_bstride=rstride, stats=st, out=out, dims=dims, **extra)
    return ops.f32b_to_ncdhw(out, dims), st


@pytest.mark.parametrize("case_id", _ids("wino"))
def test_conv3_wino_bf16x3_exact(ops, case_id):
    """md_wino_prep / md_wino_prep_v2 (whichever takes the grid; both where both do, bit-identical) + md_wino_pack_weights
    (flip = 1 for the data-gradient cases) + md_conv3_wino."""
    spec = cc.spec_of(case_id)

    def run(case, stats, ksplit):
        B, dims = case["B"], case["dims"]
        ww = ops.WinoWeight(case["w"].cuda(), "cuda", kind="conv_dgrad" if spec.get("dgrad") else "conv")
        assert (ww.rows, ww.kdim) == (case["cout"], case["cin"])
        parts = _parts(ops, case)
        ac = case["ac"].cuda() if case["ac"] is not None else None
        v2_takes = 256 % dims[2] == 0 and (dims[0] * dims[1] * dims[2]) % 256 == 0
        keep, ts = ops.WINO_PREP_V2, {}
        try:
            for v2 in ([False, True] if v2_takes else [False]):
                ops.WINO_PREP_V2 = v2
                ts[v2] = ops.wino_prep(parts, ac, False, bool(case["ups"]), B, None, dims=dims, keep=True)
        finally:
            ops.WINO_PREP_V2 = keep
        if v2_takes:
            assert torch.equal(ts[False].view(torch.int16), ts[True].view(torch.int16)), f"{case_id}: md_wino_prep_v2 != md_wino_prep"
        return _wino_launch(ops, case, ww, ts[v2_takes], stats)

    _drive(spec, run)


@pytest.mark.parametrize("case_id", _ids("wino_f8", "wino_f6"))
def test_conv3_wino_f16_planes_exact(ops, case_id):
    """md_wino_prep_f8 / _f6 + md_wino_pack_weights_f8 / _f6 + md_conv3_wino_f8 / _f6 on operands that ONE fp16 holds: the fp16
    MFMA is exact and both cross terms are zero.  `eq`: a hand-made power-of-two equaliser (an exact rescaling by construction)."""
    spec = cc.spec_of(case_id)
    fmt = spec["entry"][-2:]

    def run(case, stats, ksplit):
        eq = None
        if spec.get("eq"):
            eq = cc.equaliser(spec, case["cin"]).cuda()
        ww = ops.WinoWeightF8(case["w"].cuda(), "cuda", fmt, eq=eq)
        ac = case["ac"].cuda() if case["ac"] is not None else None
        t = ops.wino_prep(_parts(ops, case), ac, False, bool(case["ups"]), case["B"], None, f8=fmt, eq=eq, dims=case["dims"])
        return _wino_launch(ops, case, ww, t, stats)

    _drive(spec, run)


@pytest.mark.parametrize("case_id", _ids("wino_dgrad_f6"))
def test_conv3_wino_f6_data_gradient_exact(ops, case_id):
    """The training data gradient: md_absmax + md_wino_prep_dual_f6 (the lift 2^k is a power of two: exact) + the flipped f16f6
    fragments of md_pack_batch + md_conv3_wino_f6_scaled, against the float64 data gradient; the channel sums of the same pass."""
    spec = cc.spec_of(case_id)

    def run(case, stats, ksplit):
        B, cin, dims = case["B"], case["cin"], case["dims"]
        ww = ops.WinoWeightF6Dgrad(case["w"].cuda(), "cuda")
        assert (ww.rows, ww.kdim) == (case["cout"], cin)
        parts = _parts(ops, case)
        sums = torch.zeros((B, cin), device="cuda")
        amax = ops.absmax_word(parts[0][0]) if spec["lift"] == "dyn" else None
        t, _ = ops.wino_prep(parts, None, False, False, B, None, dual=True, sums=sums, f8="f6", tscale=cc.LIFT_CONST, amax=amax, dims=dims)
        msg = cc.describe_mismatch(sums.cpu().double(), case["x"].double().sum(dim=(2, 3, 4)), case_id + ": channel sums")   # integers below 2^24
        assert not msg, msg
        return _wino_launch(ops, case, ww, t, False, out_scale=1.0 if amax is not None else 1.0 / cc.LIFT_CONST, amax=amax)

    _drive(spec, run)


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm affine + SiLU in the halo loaders, seen through a transparent conv
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.TRANSPARENT_IDS)
def test_silu_loaders_through_a_transparent_conv(ops, name):
    case = cc.transparent_of(name)
    kind = name.split("-")[0]
    B, cin, cout, dims = case["B"], case["cin"], case["cout"], case["dims"]
    D, H, W = dims
    P = D * H * W
    act, abound = cc.activation64(case), cc.loader_bound(case)
    parts, ac = _parts(ops, case), case["ac"].cuda()
    worst, where, nrim = 0.0, None, 0
    # one weight set where the rows meet every channel and tap; the head's four rows take cin / 4 (at least 27) sets for that
    for wset in range(cc.transparent_sets(cout, cin)):
        w = cc.transparent_weights(cout, cin, case["seed"], wset)
        ref, bound = cc.transparent_reference(case, w, act, abound)
        if kind in ("fast", "low"):
            cfg = ops.CFG_C3_128_FAST if kind == "fast" else ops.CFG_C3_LOW
            pw = ops.PackedWeight(w.cuda(), "conv", cfg, "cuda")
            out = ops.gemm_conv(cfg=cfg, a=pw.data, b=None, out=_nan_f32b(ops, B, cout, P), batch=B, rows=cout, rows_alloc=cout, kdim=cin, dims=dims,
                                b_f32=ops.F32Operand(parts, ac, silu=True))
            y = ops.f32b_to_ncdhw(out, dims)
        elif kind == "wino":
            bound = cc.wino_transparent_bound(dict(case, w=w, w_eff=w))
            t = ops.wino_prep(parts, ac, True, False, B, None, dims=dims)
            y, _ = _wino_launch(ops, case, ops.WinoWeight(w.cuda(), "cuda"), t, False)
        else:                                          # md_conv3_head: rows (co, kw) of the dx-folded taps, then md_fold_dx (adds two zeros)
            w2 = w.permute(0, 4, 1, 2, 3).reshape(cout * 3, cin, 3, 3, 1).contiguous().cuda()
            pw = ops.PackedWeight(w2, "conv", ops.CFG_HEAD_PACK, "cuda")
            y = ops.fold_dx(ops.conv3_head(pw, parts[0][0], ac, B, None, 16, dims=dims), None, B, cout, 3, 16, None, dims=dims)
        y = y.cpu()
        err = (y.double() - ref).abs()
        rim = bound == 0                               # the tap leaves the grid: the ACTIVATED tensor is zero padded (act(0) = silu(c) != 0)
        nrim += int(rim.sum())
        assert bool((y[rim] == 0).all()), f"{name} set {wset}: {int((y[rim] != 0).sum())} rim outputs are not exactly zero"
        ratio = err / bound.clamp_min(1e-300)
        ratio[rim] = 0
        if float(ratio.max()) >= worst:
            idx = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
            worst, where = float(ratio.max()), (wset, idx, float(ref[idx]))
        assert float(ratio.max()) <= 1.0, (f"{name} set {wset}: {int((ratio > 1).sum())} elements beyond the loader bound; worst {float(ratio.max()):.3f} "
                                           f"at (b, co, z, y, x) = {tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))}")
    assert nrim > 0
    print(f"transparent {name}: max |err| / bound = {worst:.3f} at (set, (b, co, z, y, x), value) = {where}")
