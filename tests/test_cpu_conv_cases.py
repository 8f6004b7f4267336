"""What the bit-for-bit convolution tests (tests/test_gpu_conv_exact.py) rest on, proven without a GPU: for every case of
tests/conv_cases.py, in the domain of every kernel it is fed to, (a) no lo * lo pair is non-zero and the hi / lo split
reproduces every operand, (b) sum |term| stays below 2^24 lsb for every frequency accumulator and every output, bias and
residual included, the x_lo / w_lo cases really have a live lo plane THERE (for Winograd: after the transform), and an fp32
evaluation of hi*hi + hi*lo + lo*hi in two summation orders equals the float64 reference bit for bit.  With that the
reference alone meets "bit for bit"; a mismatch on the GPU is the kernel's.  The conditions are caps, not measurements."""
import pytest
import torch

import conv_cases as cc


def _check(case, domain):
    spec = case["spec"]
    m = cc.exactness_margin(case, domain)
    assert m["split_exact"], f"{spec['id']} [{domain}]: hi + lo does not reproduce an operand"
    assert m["lolo_zero"], f"{spec['id']} [{domain}]: a lo * lo product is non-zero"
    worst = max(m["max_sum"].items(), key=lambda kv: kv[1])
    print(f"{spec['id']} [{domain}]: max sum |term| = 2^24 x {worst[1] / cc.LIMIT:.3f} ({worst[0]})")
    for name, v in m["max_sum"].items():
        assert v < cc.LIMIT, f"{spec['id']} [{domain}]: sum |term| of {name} = {v:.4g} lsb >= 2^24"
    anyof = (lambda v: any(v)) if domain != "direct" else bool
    # nearest x2 makes d1 == d2 for every output pair: the third transformed input d2 - d1 is identically zero there
    allof = (lambda v: all(q for f, q in enumerate(v) if not (case["ups"] and f == 2))) if domain != "direct" else bool
    if spec["cls"] in ("hi_only", "tiny") or (spec["cls"] == "f16" and domain == "wino_f16"):
        assert not anyof(m["x_lo_live"]) and not anyof(m["w_lo_live"])
    elif spec["cls"] == "x_lo":
        assert allof(m["x_lo_live"]) and not anyof(m["w_lo_live"]), f"{spec['id']} [{domain}]: lo planes {m['x_lo_live']} {m['w_lo_live']}"
    elif spec["cls"] == "w_lo":
        assert allof(m["w_lo_live"]) and not anyof(m["x_lo_live"]), f"{spec['id']} [{domain}]: lo planes {m['x_lo_live']} {m['w_lo_live']}"
    ref = cc.reference(case)
    for order in (0, 1):
        got = cc.eval_fp32(case, domain, order)
        msg = cc.describe_mismatch(got.double(), ref, f"{spec['id']} [{domain}] fp32 evaluation, order {order}")
        assert not msg, msg
    return ref


@pytest.mark.parametrize("case_id", cc.IDS)
def test_case_is_exact_in_every_domain_it_is_fed_to(case_id):
    spec = cc.spec_of(case_id)
    case = cc.build(spec)
    assert case["x"].dtype == torch.float32 and torch.equal(case["x"], case["x"].round())
    if case["ac"] is not None:           # the hand-made affine: x_raw * a + c is exact in fp32 and never 0 where x_raw is 0
        raw = torch.cat(case["x_raw"], 1).double()
        a, c = case["ac"][..., 0].double()[:, :, None, None, None], case["ac"][..., 1].double()[:, :, None, None, None]
        assert torch.equal((raw * a + c).float().double(), raw * a + c) and torch.equal(case["x"].double(), raw * a + c)
        assert bool((case["ac"][..., 1] != 0).all())
    for domain in spec["domains"]:
        ref = _check(case, domain)
    if spec.get("out") == "s16b":        # hi + lo of every output is exact
        hi, lo = cc.split_bf16(ref.float())
        assert torch.equal((hi + lo).double(), ref)
    if spec.get("prec") == "fp16x2":     # ONE fp16 holds the operand; the weights' fp16 split is exact
        assert torch.equal(case["x"].half().float(), case["x"])
        hi, lo = cc.split_fp16(case["w_eff"])
        assert torch.equal(hi + lo, case["w_eff"])
    if spec["entry"].startswith("wino_f") or spec["entry"] == "wino_dgrad_f6":
        # fp16 range: the scaled operand and weight images the kernels form (equaliser, pre-scale, lift: cc.fp16_extremes computes
        # them from the case's tensors and the scales its launcher passes) stay in the lower half of the fp16 range, and no
        # non-zero element falls under the smallest normal
        t, g = cc.fp16_extremes(case)
        print(f"{spec['id']}: largest fp16 operand {t:g}, largest fp16 weight {g:g}")
        assert 2.0 ** -14 <= t < 32768 and 2.0 ** -14 <= g < 32768, (t, g)
    if spec.get("stats"):
        assert float(cc.reference_stats(ref).abs().max()) < 2.0 ** 53
    twin = cc.stats_twin(spec)
    if twin is not None:                 # the exact GroupNorm sums are checked on this one: exact as a conv, and every fp32 partial sum exact
        tcase = cc.build(twin)
        for domain in spec["domains"]:
            tref = _check(tcase, domain)
        assert cc.stats_margin(tref) < cc.LIMIT, f"{twin['id']}: sum o^2 over a (sample, channel) grid = {cc.stats_margin(tref):.4g} >= 2^24"
    if spec.get("dgrad"):                # w_eff IS the data-gradient conv of w
        x = cc.conv_input(case)
        want = torch.nn.grad.conv3d_input((case["B"], case["cout"]) + case["dims"], case["w"].double(), x, padding=1)
        want = want if case["rows"] is None else want[:, case["rows"]]
        extra = ref - torch.nn.functional.conv3d(x, (case["w_eff"] if case["rows"] is None else case["w_eff"][case["rows"]]).double(), padding=1)
        assert torch.equal(want + extra, ref)


def test_every_entry_point_has_a_cube_and_three_non_cubic_orders():
    """The table itself: per launcher the smallest cube, a cube of several tiles and non-cubic grids in more than one order."""
    for entry in sorted({(s["entry"], s.get("cfg", "")) for s in cc.SPECS}):
        grids = [s["dims"] for s in cc.SPECS if (s["entry"], s.get("cfg", "")) == entry]
        if entry[0] == "nin" or entry[1].startswith("CFG_G1_"):
            assert all(d[0] == d[1] == 1 for d in grids)
            continue                                         # GEMMs over flat positions: no grid
        assert any(d[0] == d[1] == d[2] for d in grids), entry
        noncubic = {d for d in grids if len({d[0], d[1], d[2]}) == 3}
        orders = {tuple(sorted(range(3), key=lambda i: d[i])) for d in noncubic}
        assert len(orders) >= 2, (entry, noncubic)


def test_classes_differ_where_they_claim():
    """A dropped cross term is visible: the x_lo / w_lo references change when the lo plane of the live side is removed."""
    for cls, side in (("x_lo", "x"), ("w_lo", "w_eff")):
        spec = next(s for s in cc.SPECS if s["cls"] == cls and s["entry"] == "wino")
        case = cc.build(spec)
        ref = cc.reference(case)
        hi, _ = cc.split_bf16(case[side])
        broken = dict(case)
        broken[side] = hi
        assert not torch.equal(cc.reference(broken), ref)


@pytest.mark.parametrize("name", cc.TRANSPARENT_IDS)
def test_transparent_case_and_loader_bound_headroom(name):
    """Part of the GPU file's SiLU checks that needs no GPU: the weights are transparent (one power-of-two tap per row, all 27
    taps and many channels in use), the inputs cover |z| up to 12 with both signs and |a| from 2^-6 to 2^6, and an fp32
    restatement of the loader's formula (correctly rounded exp2 and reciprocal) leaves HALF of the derived bound free.  The half is
    taken of everything the hardware may do differently (the affine's contraction, v_exp_f32, v_rcp_f32); the bf16 split's share
    is attained exactly by construction (the same RNE on both sides), so it is allowed in full -- "half of the whole bound" cannot
    hold for any bound of the split that is tight."""
    case = cc.transparent_of(name)
    w = case["w_eff"].reshape(case["cout"], case["cin"], 27)
    assert bool(((w != 0).sum(dim=(1, 2)) == 1).all())
    nz = w[w != 0]
    assert torch.equal(torch.exp2(torch.log2(nz).round()), nz)
    nsets = cc.transparent_sets(case["cout"], case["cin"])
    ws = torch.stack([cc.transparent_weights(case["cout"], case["cin"], case["seed"], k) for k in range(nsets)])
    assert torch.equal(ws[0], case["w_eff"]) and bool(((ws != 0).sum(dim=(2, 3, 4, 5)) == 1).all())
    used = (ws != 0).reshape(nsets * case["cout"], case["cin"], 27)
    assert bool(used.any(0).any(1).all()) and bool(used.any(0).any(0).all()), "the weight sets of the case miss a channel or a tap"
    _, z, _ = cc._azc(case)
    a = case["ac"][..., 0].abs()
    assert float(z.max()) > 11 and float(z.min()) < -11 and float(a.min()) < 2 ** -5 and float(a.max()) > 2 ** 5
    assert bool((case["ac"][..., 1].abs() >= 0.25).all())
    act = cc.activation64(case)
    free = cc.loader_bound(case, split=False)
    ratio = ((cc.loader_fp32(case, split=False).double() - act).abs() / free).max()
    whole = ((cc.loader_fp32(case).double() - act).abs() / (cc.loader_bound(case) - 0.5 * free)).max()
    print(f"{name}: fp32 restatement uses {float(ratio):.3f} of the bound in front of the split, {float(whole):.3f} of (split + half of the rest)")
    assert float(ratio) <= 0.5 and float(whole) <= 1.0
    if name.startswith("wino"):
        ref, _ = cc.transparent_reference(case)
        bound, fixed = cc.wino_transparent_bound(case, parts=True)
        err = (cc.wino_loader_fp32(case).double() - ref).abs()
        assert bool((err[bound == 0] == 0).all())
        r = float((err / (fixed + 0.5 * (bound - fixed)).clamp_min(1e-300)).max())
        print(f"{name}: fp32 restatement of the Winograd path uses {r:.3f} of (transform + split + accumulation, and half of the rest)")
        assert r <= 1.0
