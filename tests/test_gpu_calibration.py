"""The calibration safety net with the net firing: hip_ops.AUDIT's figure per layer against float64, and DDPMUNet3D.calibrate /
models.utils.calibrate_model on a whole model whose convs ARE demoted (inputs, references and bounds: tests/calibration_cases.py;
their CPU-side preconditions: tests/test_cpu_calibration_cases.py; measured figures: DESIGN.md section 5).

Per layer (layers.run_conv3 under precision_scope("f16f6"), B 2, 16^3, cout 128): the audited launch is the product launch bit for
bit; the record's figure IS |y_r - y_b| / |y_b| of the reduced-precision and the bf16x3 launch; against the float64 result r it lies
between (e_r - e_b) / (1 + e_b) and (e_r + e_b) / (1 - e_b) (triangle inequality); one record per reduced-precision launch and none
for a bf16x3 one.  Whole model (nf 128, ch_mult (1, 2), 16^3: 16^3 x 128 and 8^3 x 256 levels, blocks with and without a NIN
shortcut, concatenated inputs, one Upsample conv): bar 0 demotes everything and the model then IS the bf16x3 model; a bar inside the
largest gap of the measured figures demotes exactly the sites above it; one poisoned GroupNorm / conv pair is the one site demoted at
the default bar, and the evaluation against the CPU oracle improves.

Mutations, each tried once on a scratch copy and seen to fail the named test:
  * layers._conv3_wino: the audit's difference taken against `out` itself (figure 0)
      -> test_audit_figure_against_float64[all five cases] (the figure is not the test's own |y_r - y_b| / |y_b|)
  * DDPMUNet3D.calibrate: `r["rel_l2"] > bar` turned into `<`
      -> test_calibrate_selective_bar_demotes_exactly_the_sites_above_it, test_calibrate_poisoned_conv0_is_the_one_site_demoted
  * DDPMUNet3D.calibrate: the demotion written to another owner (the model itself instead of r["owner"])
      -> test_calibrate_bar_zero_demotes_every_site_and_the_model_is_the_bf16x3_model (the reported module holds no demotion)
  * layers.plan_conv3: md_bf16x3_sites ignored where the block pass applies (fmt kept when operand.nin and block_pass_ok)
      -> test_block_pass_site_audited_then_demoted, tests/test_cpu_calibration_cases.py::test_plan_of_a_demoted_site[nin_s32_block_pass]"""
import pytest
import torch
import torch.nn.functional as F

import calibration_cases as cc

pytestmark = pytest.mark.gpu

TOL_MFMA = 3e-5          # the bf16x3 budget of tests/test_gpu_wino.py
TOL_EVAL = 1e-4          # one U-Net evaluation against the oracle: tests/test_gpu_unet.py


@pytest.fixture(scope="module")
def env(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops, synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, layers, utils as mutils  # noqa: F401
    from oracle import unet_oracle as uo
    return dict(ops=hip_ops, synth=synth, layers=layers, mutils=mutils, uo=uo)


@pytest.fixture(autouse=True)
def _setup(env, monkeypatch):
    ops = env["ops"]
    if ops.FORCE_PRECISION:
        pytest.skip("the calibration is about the configured arithmetic, which MD_FORCE_PRECISION overrides")
    monkeypatch.setattr(ops, "WINO_MIN_WGS", 1)
    yield
    assert ops.AUDIT is None and ops.CALIBRATE is None and ops.PROFILE is None


class _Collected:
    """What one launch / evaluation left in hip_ops.PROFILE (and AUDIT)."""

    def __init__(self, out, profile, recs):
        self.out, self.recs = out, recs
        self.wino = [r[5] for r in profile if r[0] == "wino"]
        self.prep = [r[5] for r in profile if r[0] == "wino_prep"]

    @property
    def reduced(self):
        return [t for t in self.wino if t.endswith(("/f6", "/f8"))]


def _collect(ops, fn, audit=False):
    assert ops.PROFILE is None and ops.AUDIT is None
    ops.PROFILE = []
    if audit:
        ops.AUDIT = []
    try:
        with torch.no_grad():
            out = fn()
        return _Collected(out, ops.PROFILE, ops.AUDIT)
    finally:
        ops.PROFILE = ops.AUDIT = None


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the audit figure against float64, per layer
# ---------------------------------------------------------------------------------------------------------------------------------
class _Pair:
    """GroupNorm -> SiLU -> conv of a calibration_cases.LayerCase as a HipLayer on the device, launched the way a ResnetBlock does."""

    def __init__(self, env, case):
        ops, layers = env["ops"], env["layers"]
        cin = sum(case.cs)

        class Pair(layers.HipLayer):
            def __init__(self):
                super().__init__()
                self.gn = torch.nn.GroupNorm(32, cin, eps=1e-6)
                self.conv = torch.nn.Conv3d(cin, case.cout, 3, padding=1)

        self.layer = Pair()
        with torch.no_grad():
            self.layer.gn.weight.copy_(case.gamma); self.layer.gn.bias.copy_(case.beta); self.layer.conv.weight.copy_(case.w)
        self.layer = self.layer.cuda()
        self.ops, self.layers, self.case = ops, layers, case
        self.parts = [(ops.ncdhw_to_f32b(x.cuda()), k) for x, k in zip(case.xs, case.cs)]
        _, self.ac = ops.gn_params(self.parts, self.layer.gn.weight, self.layer.gn.bias, case.B, case.S ** 3, want_ac=True)
        self.pw = layers.conv3_packed(self.layer, "w", self.layer.conv, ops.conv_cfg_for(case.S))
        self.bias = case.bias.cuda()
        self.res = ops.ncdhw_to_f32b(case.residual.cuda()) if case.residual is not None else None

    def launch(self, mode, audit=False, residual=True):
        """-> _Collected with .y (NCDHW on the CPU) and .sums (the GroupNorm sums of the output, float64 [B, cout, 2])."""
        ops, layers, c, lay = self.ops, self.layers, self.case, self.layer

        def go():
            with ops.precision_scope(mode):
                return layers.run_conv3(self.pw, None, c.B, c.S, bias=self.bias, bias_bstride=c.cout, residual=self.res if residual else None,
                                        want_stats=True, b_f32=ops.F32Operand(self.parts, self.ac, silu=True),
                                        wino=layers.conv3_wino_packed(lay, "w", lay.conv, gn=lay.gn))
        got = _collect(ops, go, audit)
        got.sums = got.out._md_sums.clone().cpu()
        got.y = ops.f32b_to_ncdhw(got.out, (c.S,) * 3).cpu()
        return got


def _check_audited_launch(case_name, pair, r, owner, site, cin):
    """The assertions every layer case shares; returns the audit figure."""
    c = pair.case
    a, p, b = pair.launch("f16f6", audit=True), pair.launch("f16f6"), pair.launch("bf16x3", audit=True)
    assert len(a.wino) == 2 and a.wino[0].endswith("/f6") and "/f" not in a.wino[1], a.wino      # the product launch, then its bf16x3 repeat
    assert len(p.wino) == 1 and p.wino[0].endswith("/f6") and len(b.wino) == 1 and "/f" not in b.wino[0], (p.wino, b.wino)
    assert b.recs == [], "a bf16x3 launch is not audited"
    assert len(a.recs) == 1, a.recs
    rec = a.recs[0]
    assert rec["owner"] is owner and rec["site"] == site
    assert (rec["fmt"], rec["cin"], rec["cout"], rec["S"]) == ("f6", cin, c.cout, c.S)
    assert torch.equal(a.y, p.y), "the audit disturbs the product launch"
    yd = p.y.double()
    for got in (a, p):
        assert cc.rel(got.sums[..., 0], yd.sum(dim=(2, 3, 4))) < 1e-6 and cc.rel(got.sums[..., 1], (yd * yd).sum(dim=(2, 3, 4))) < 1e-6
    assert cc.rel(a.sums, p.sums) < 1e-12
    fig = rec["rel_l2"]
    pairwise = cc.rel(p.y, b.y)
    e_r, e_b = cc.rel(p.y, r), cc.rel(b.y, r)
    lo, hi = cc.triangle_bounds(e_r, e_b)
    print(f"audit {case_name}: figure {fig:.4e} (|y_r - y_b| / |y_b| by the test {pairwise:.4e}); vs float64 e_r {e_r:.3e} e_b {e_b:.3e}; "
          f"bounds [{lo:.3e}, {hi:.3e}]")
    assert abs(fig - pairwise) <= 1e-6 * pairwise
    assert e_b < TOL_MFMA
    assert lo <= fig <= hi
    return fig


@pytest.mark.parametrize("name", list(cc.LAYER_CASES))
def test_audit_figure_against_float64(env, name, monkeypatch):
    ops = env["ops"]
    case = cc.layer_case(name)
    monkeypatch.setattr(ops, "WINO_EQ", case.eq)
    pair = _Pair(env, case)
    fig = _check_audited_launch(name, pair, case.ref, pair.layer, "w", sum(case.cs))
    if name in ("friendly", "span6_eq"):
        assert fig < cc.BAR
    elif name == "span6_noeq":
        assert fig > 2 * cc.BAR                      # the precondition of every demotion test below
    elif name == "two_parts":
        assert fig > cc.BAR
    elif name == "residual30":
        a, b = pair.launch("f16f6", audit=True, residual=False), pair.launch("bf16x3", residual=False)
        bare = a.recs[0]["rel_l2"]
        assert abs(bare - cc.rel(a.y, b.y)) <= 1e-6 * bare
        lo, hi = cc.triangle_bounds(cc.rel(a.y, case.ref_conv), cc.rel(b.y, case.ref_conv))
        print(f"audit residual30: the same launch without the residual {bare:.4e} (bounds [{lo:.3e}, {hi:.3e}]), dilution {bare / fig:.1f}")
        assert lo <= bare <= hi and bare > 2 * cc.BAR
        assert bare >= 10.0 * fig
    # a demoted site: the bf16x3 launch, bit for bit, and nothing to audit
    pair.layer.md_bf16x3_sites = ("w",)
    d, b = pair.launch("f16f6", audit=True), pair.launch("bf16x3")
    assert d.recs == [] and len(d.wino) == 1 and "/f" not in d.wino[0]
    assert torch.equal(d.y, b.y)


def test_audit_upsample_calibrated(env, monkeypatch):
    """layers.Upsample on a 1e-5-magnitude raw stream with a 2^+-2 channel spread, 8^3 -> 16^3, after a CALIBRATE pass: the compact
    operand, the measured equaliser, no GroupNorm."""
    ops, layers = env["ops"], env["layers"]
    monkeypatch.setattr(ops, "WINO_EQ", True)
    B, S, cin = 2, 16, 128
    spread = cc.span_scale(cin, 2.0, 9)
    x = cc.randn((B, cin, S // 2, S // 2, S // 2), 330) * 1e-5 * spread.view(1, -1, 1, 1, 1)
    up = layers.Upsample(cin, with_conv=True)
    with torch.no_grad():
        up.Conv_0.weight.copy_(cc.randn((cin, cin, 3, 3, 3), 331, 0.05) / spread.view(1, -1, 1, 1, 1))
        up.Conv_0.bias.copy_(cc.randn((cin,), 332, 1e-5))
    r = F.conv3d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), up.Conv_0.weight.detach().double(),
                 up.Conv_0.bias.detach().double(), padding=1)
    up = up.cuda().eval()
    xd = x.cuda()
    preps = []
    real_prep = ops.wino_prep

    def spy(*a, **kw):
        preps.append((kw.get("f8", False), kw.get("compact", False)))
        return real_prep(*a, **kw)
    monkeypatch.setattr(ops, "wino_prep", spy)

    def launch(mode, audit=False):
        def go():
            with ops.precision_scope(mode):
                return up(xd)
        got = _collect(ops, go, audit)
        got.y = got.out.cpu()
        return got

    u = launch("f16f6", audit=True)
    assert u.recs == [] and u.reduced == [], "an uncalibrated raw stream stays in bf16x3"
    ops.CALIBRATE = {}
    try:
        launch("f16f6")
        cal = ops.CALIBRATE
    finally:
        ops.CALIBRATE = None
    (owner, site, tot, n), = cal.values()
    assert owner is up and site == "w" and n == 1
    up._md_act_ms = {site: (tot / n).contiguous()}
    del preps[:]
    a = launch("f16f6", audit=True)
    assert preps == [("f6", True), (False, True)], preps          # product and repeat both in the compact layout
    p, b = launch("f16f6"), launch("bf16x3")
    assert len(a.recs) == 1 and a.recs[0]["owner"] is up and a.recs[0]["site"] == "w"
    assert (a.recs[0]["fmt"], a.recs[0]["cin"], a.recs[0]["cout"], a.recs[0]["S"]) == ("f6", cin, cin, S)
    assert len(p.reduced) == 1 and b.reduced == []
    assert torch.equal(a.y, p.y)
    fig, pairwise = a.recs[0]["rel_l2"], cc.rel(p.y, b.y)
    e_r, e_b = cc.rel(p.y, r), cc.rel(b.y, r)
    lo, hi = cc.triangle_bounds(e_r, e_b)
    print(f"audit upsample_calibrated: figure {fig:.4e} (by the test {pairwise:.4e}); vs float64 e_r {e_r:.3e} e_b {e_b:.3e}; bounds [{lo:.3e}, {hi:.3e}]")
    assert abs(fig - pairwise) <= 1e-6 * pairwise
    assert e_b < TOL_MFMA and lo <= fig <= hi
    up.md_bf16x3_sites = ("w",)
    d = launch("f16f6", audit=True)
    assert d.recs == [] and d.reduced == [] and torch.equal(d.y, b.y)


def test_block_pass_site_audited_then_demoted(env, monkeypatch):
    """A ResnetBlock 128 + 128 -> 128 with a NIN shortcut at 32^3, B 1: the smallest shape hip_ops.block_pass_ok takes, so the
    audited Conv_0 launch is the one whose operand pass writes the shortcut too.  Demoted, the conv is the bf16x3 launch bit for
    bit, hands no shortcut back (the block runs its own NIN), and the block is within the bf16x3 budget of float64."""
    ops, layers, synth, uo = env["ops"], env["layers"], env["synth"], env["uo"]
    monkeypatch.setattr(ops, "WINO_EQ", True)
    B, S, cs, cout, tdim = 1, 32, (128, 128), 128, 512
    P, cin = S ** 3, sum(cs)
    assert ops.block_pass_ok([(None, c) for c in cs], cout, B, S, S, S) and not ops.block_pass_ok([(None, c) for c in cs], cout, B, S, S, S // 2)
    blk = layers.ResnetBlockDDPM(act=torch.nn.SiLU(), in_ch=cin, out_ch=cout, temb_dim=tdim, dropout=0.0)
    sd = synth.sensitised_state_dict(blk.state_dict(), seed=3)
    blk.load_state_dict(sd); blk = blk.cuda().eval()
    xs = [cc.randn((B, c, S, S, S), 700 + i) * (1.0 + 0.5 * i) for i, c in enumerate(cs)]
    temb = cc.randn((B, tdim), 710)
    with torch.no_grad():
        r = uo.resnet_block({k: v.double() for k, v in sd.items()}, torch.cat(xs, 1).double(), temb.double())
    parts = [(ops.ncdhw_to_f32b(x.cuda()), c) for x, c in zip(xs, cs)]
    temb_d = temb.cuda()
    g0 = blk.GroupNorm_0
    with torch.no_grad():
        _, ac0 = ops.gn_params(parts, g0.weight, g0.bias, B, P, eps=g0.eps, groups=g0.num_groups, want_ac=True)
        bias0, bias0_stride = blk._film_bias(temb_d, None, None)
    pw0 = layers.conv3_packed(blk, "w0", blk.Conv_0, ops.conv_cfg_for(S))
    pwn = blk.NIN_0.packed(P, hbm_bound=True)

    def conv0(mode, audit=False):
        """Conv_0 as ResnetBlockDDPM.forward_blocked launches it."""
        f0 = ops.F32Operand(parts, ac0, silu=True, nin=(pwn, blk.NIN_0.b))

        def go():
            with ops.precision_scope(mode):
                return layers.run_conv3(pw0, None, B, S, bias=bias0, bias_bstride=bias0_stride, want_stats=True, b_f32=f0,
                                        wino=layers.conv3_wino_packed(blk, "w0", blk.Conv_0, gn=g0)).clone()
        got = _collect(ops, go, audit)
        got.shortcut = f0.shortcut
        return got

    def block(mode, audit=False):
        def go():
            with ops.precision_scope(mode):
                return ops.f32b_to_ncdhw(blk.forward_blocked(parts, B, P, temb=temb_d), (S, S, S)).cpu()
        return _collect(ops, go, audit)

    a, p, b = conv0("f16f6", audit=True), conv0("f16f6"), conv0("bf16x3")
    assert a.prep[0].endswith("/f6/nin") and a.shortcut is not None and p.shortcut is not None, a.prep      # the block pass
    assert b.shortcut is None and b.reduced == []
    assert len(a.recs) == 1 and a.recs[0]["owner"] is blk and a.recs[0]["site"] == "w0"
    assert (a.recs[0]["fmt"], a.recs[0]["cin"], a.recs[0]["cout"], a.recs[0]["S"]) == ("f6", cin, cout, S)
    assert torch.equal(a.out, p.out) and torch.equal(a.shortcut, p.shortcut)
    fig, pairwise = a.recs[0]["rel_l2"], cc.rel(p.out, b.out)
    print(f"audit block_pass: Conv_0 figure {fig:.4e} (by the test {pairwise:.4e})")
    assert abs(fig - pairwise) <= 1e-6 * pairwise and fig < cc.BAR
    whole = block("f16f6", audit=True)
    assert [(x["owner"] is blk, x["site"]) for x in whole.recs] == [(True, "w0"), (True, "w1")]
    assert abs(whole.recs[0]["rel_l2"] - fig) <= 1e-3 * fig        # the block launches what conv0() launches
    e_f6 = cc.rel(whole.out, r)
    blk.md_bf16x3_sites = ("w0",)
    d = conv0("f16f6", audit=True)
    assert d.recs == [] and d.reduced == [] and not any(t.endswith("/nin") for t in d.prep), (d.wino, d.prep)
    assert d.shortcut is None                                      # the caller runs its own NIN
    assert torch.equal(d.out, b.out)
    whole_d = block("f16f6", audit=True)
    assert [x["site"] for x in whole_d.recs] == ["w1"]
    assert len(whole_d.reduced) == 1 and len(whole_d.wino) == 3    # Conv_0 bf16x3; Conv_1 f16f6 and its audit repeat
    e_d = cc.rel(whole_d.out, r)
    print(f"audit block_pass: block vs float64 {e_f6:.3e} with the block pass, {e_d:.3e} with Conv_0 demoted")
    assert e_d < TOL_MFMA


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. DDPMUNet3D.calibrate on a whole model
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(env, precision, sd=None):
    synth, mutils = env["synth"], env["mutils"]
    cfg = cc.model_config(synth, precision); cfg.device = torch.device("cuda")
    model = mutils.create_model(cfg).eval()
    if sd is None:
        sd = cc.model_state_dict(synth, model.module.state_dict())
    model.module.load_state_dict(sd, strict=True)
    return cfg, model, sd


def _inputs(env):
    return cc.model_input(env["synth"]).cuda(), torch.tensor(cc.MODEL_LABELS).cuda()


def _evaluate(env, model, audit=False):
    x, labels = _inputs(env)
    return _collect(env["ops"], lambda: model(x, labels).cpu(), audit)


_ORACLE = {}


def _oracle(env, key, cfg, sd):
    if key not in _ORACLE:
        with torch.no_grad():
            _ORACLE[key] = env["uo"].unet_res64_forward(sd, env["synth"].oracle_cfg(cfg), cc.model_input(env["synth"]), torch.tensor(cc.MODEL_LABELS))
    return _ORACLE[key]


def _measure_by_hand(env, model, batches=None):
    """Step 1 of DDPMUNet3D.calibrate, restated: one evaluation per batch with hip_ops.CALIBRATE on, every site's mean squares (mean over
    the batches) kept on its layer.  Returns the number of distinct Winograd sites."""
    ops = env["ops"]
    batches = batches or [_inputs(env)]
    ops.CALIBRATE = {}
    try:
        with torch.no_grad():
            for x, labels in batches:
                model(x, labels)
        cal = ops.CALIBRATE
    finally:
        ops.CALIBRATE = None
    for owner, site, tot, n in cal.values():
        assert n == len(batches)
        owner.__dict__.setdefault("_md_act_ms", {})[site] = (tot / float(n)).contiguous()
    return len(cal)


def _site_figures(net, recs):
    """{(module name, site): worst audit figure}."""
    names = {id(m): n for n, m in net.named_modules()}
    out = {}
    for r in recs:
        key = (names[id(r["owner"])], r["site"])
        out[key] = max(out.get(key, 0.0), r["rel_l2"])
    return out


def _demote_by_hand(net, sites):
    mods = dict(net.named_modules())
    for name, site in sites:
        m = mods[name]
        m.md_bf16x3_sites = tuple(sorted(set(getattr(m, "md_bf16x3_sites", ())) | {site}))


def _all_sites(net):
    return sorted((n, s) for n, m in net.named_modules() for s in getattr(m, "md_bf16x3_sites", ()))


def test_calibrate_bar_zero_demotes_every_site_and_the_model_is_the_bf16x3_model(env, monkeypatch):
    ops = env["ops"]
    monkeypatch.setattr(ops, "WINO_EQ", True)
    x, labels = _inputs(env)
    _, model, sd = _model(env, "f16f6")
    net = model.module
    before = _evaluate(env, model)
    assert before.reduced, "the model has no reduced-precision conv to calibrate"
    rep = net.calibrate(x, labels, bar=0.0)
    print(f"calibrate(bar=0): {rep['measured']} measured, {rep['audited']} audited, worst {rep['worst']}, demoted {len(rep['demoted'])}: "
          + ", ".join(f"{n}/{s} {v:.2e}" for n, s, v in rep["demoted"]))
    mods = dict(net.named_modules())
    assert rep["worst"] == 0.0
    assert rep["audited"] == rep["measured"] == len(before.wino)            # one batch: every Winograd site launches once, all are audited
    assert len(rep["demoted"]) == rep["audited"] and len({(n, s) for n, s, _ in rep["demoted"]}) == rep["audited"]
    for name, site, diff in rep["demoted"]:
        assert name != "?" and name in mods and diff > 0.0
        assert site in getattr(mods[name], "md_bf16x3_sites", ()), f"{name}/{site} is reported demoted, its module does not hold it"
    assert _all_sites(net) == sorted((n, s) for n, s, _ in rep["demoted"])   # and nowhere else
    after = _evaluate(env, model, audit=True)
    assert after.reduced == [] and after.recs == [] and len(after.wino) == len(before.wino), after.wino
    _, twin, _ = _model(env, "bf16x3", sd)
    ref = _evaluate(env, twin)
    assert ref.reduced == [] and ref.wino == after.wino
    assert torch.equal(after.out, ref.out), f"the fully demoted model differs from the bf16x3 model: {cc.rel(after.out, ref.out):.3e}"
    # demotions are for good: a second calibration with a bar nothing reaches audits nothing and keeps them
    sites = _all_sites(net)
    rep2 = net.calibrate(x, labels, bar=1.0)
    assert rep2["audited"] == 0 and rep2["demoted"] == [] and rep2["worst"] == 0.0 and rep2["measured"] == rep["measured"]
    assert _all_sites(net) == sites
    assert torch.equal(_evaluate(env, model).out, ref.out)


SELECTIVE_MIN_GAP = 1.2


def test_calibrate_selective_bar_demotes_exactly_the_sites_above_it(env, monkeypatch):
    ops = env["ops"]
    monkeypatch.setattr(ops, "WINO_EQ", True)
    x, labels = _inputs(env)
    _, hand, sd = _model(env, "f16f6")
    n_sites = _measure_by_hand(env, hand)
    audited = _evaluate(env, hand, audit=True)
    figs = _site_figures(hand.module, audited.recs)
    order = sorted(figs.items(), key=lambda kv: kv[1])
    ratios = [order[i + 1][1] / order[i][1] for i in range(len(order) - 1)]
    i = max(range(len(ratios)), key=ratios.__getitem__)
    bar = (order[i][1] * order[i + 1][1]) ** 0.5
    print("audit by hand: " + ", ".join(f"{n}/{s} {v:.3e}" for (n, s), v in order))
    print(f"selective: largest gap x{ratios[i]:.3f} between {order[i][1]:.3e} and {order[i + 1][1]:.3e}; bar {bar:.3e}; "
          f"{len(order) - i - 1} of {len(order)} sites above it")
    assert ratios[i] >= SELECTIVE_MIN_GAP, "no gap to put a bar in: choose another seed"
    above = sorted(k for k, v in figs.items() if v > bar)
    assert len(audited.recs) == len(audited.reduced) == len(figs) and n_sites == len(audited.wino) - len(audited.recs)

    _, model, _ = _model(env, "f16f6", sd)
    rep = model.module.calibrate(x, labels, bar=bar)
    print(f"calibrate(bar={bar:.3e}): {rep}")
    assert sorted((n, s) for n, s, _ in rep["demoted"]) == above
    assert all(v == figs[(n, s)] for n, s, v in rep["demoted"])
    assert rep["worst"] == order[i][1]
    assert rep["audited"] == len(audited.reduced) and rep["measured"] == n_sites
    assert _all_sites(model.module) == above
    after = _evaluate(env, model)
    assert len(after.reduced) == len(audited.reduced) - len(above) and len(after.wino) == n_sites
    _demote_by_hand(hand.module, above)
    twin = _evaluate(env, hand)
    assert twin.wino == after.wino
    assert torch.equal(after.out, twin.out)


def test_calibrate_keeps_each_sites_worst_figure_over_the_batches(env, monkeypatch):
    """Two batches (other noise, other timesteps): the operand is measured over both, every launch of both is audited, and a site's
    figure is the larger of its two -- each audited by hand on a twin."""
    ops, synth = env["ops"], env["synth"]
    monkeypatch.setattr(ops, "WINO_EQ", True)
    batches = [_inputs(env), (cc.model_input(synth, seed=6).cuda(), torch.tensor((400.0, 10.0)).cuda())]
    _, hand, sd = _model(env, "f16f6")
    n_sites = _measure_by_hand(env, hand, batches)
    per_batch = []
    for x, labels in batches:
        got = _collect(ops, lambda: hand(x, labels), audit=True)
        per_batch.append(_site_figures(hand.module, got.recs))
    assert len(per_batch[0]) == len(per_batch[1]) == n_sites
    want = {k: max(per_batch[0][k], per_batch[1][k]) for k in per_batch[0]}
    n_second = sum(per_batch[1][k] > per_batch[0][k] for k in want)
    print(f"two batches: the second one holds the worst figure of {n_second} of {n_sites} sites")
    assert 0 < n_second < n_sites, "both batches must matter: choose other inputs"
    _, model, _ = _model(env, "f16f6", sd)
    rep = model.module.calibrate([b[0] for b in batches], [b[1] for b in batches], bar=0.0)
    assert rep["measured"] == n_sites and rep["audited"] == 2 * n_sites
    assert {(n, s): v for n, s, v in rep["demoted"]} == want


def _poisoned(env, which, monkeypatch):
    """The span6 recipe on GroupNorm_{which} / Conv_{which} of the first 16^3 ResnetBlock, equaliser off, default bar.
    -> (report, evaluation before, evaluation after, e_before, e_after) with the errors against the CPU oracle on the same weights"""
    ops = env["ops"]
    monkeypatch.setattr(ops, "WINO_EQ", False)
    x, labels = _inputs(env)
    cfg, model, sd = _model(env, "f16f6")
    sd_p = cc.poison(sd, cc.POISONED_BLOCK, which)
    model.module.load_state_dict(sd_p, strict=True)
    oracle = _oracle(env, f"poisoned{which}", cfg, sd_p)
    before = _evaluate(env, model)
    rep = model.module.calibrate(x, labels, bar=cc.BAR)
    after = _evaluate(env, model)
    e_before, e_after = cc.rel(before.out, oracle), cc.rel(after.out, oracle)
    print(f"poisoned Conv_{which} of {cc.POISONED_BLOCK}: demoted {rep['demoted']}, worst kept {rep['worst']:.3e} (bar / 1.5 = {cc.BAR / 1.5:.3e}); "
          f"vs oracle {e_before:.3e} -> {e_after:.3e}")
    # the block is the first one the evaluation reaches and the stem is no Winograd conv: its Conv_0 / Conv_1 are launches 0 / 1
    assert before.wino[which].startswith("128->128@16x16x16") and before.wino[which].endswith("/f6")
    return rep, before, after, e_before, e_after


def _assert_one_site_demoted(rep, before, after, e_before, e_after, which):
    assert [(n, s) for n, s, _ in rep["demoted"]] == [(cc.POISONED_BLOCK, f"w{which}")]
    assert rep["demoted"][0][2] > cc.BAR
    assert rep["worst"] < cc.BAR / 1.5                                     # every other site is clearly under the bar
    changed = [i for i, (a, b) in enumerate(zip(before.wino, after.wino)) if a != b]
    assert len(before.wino) == len(after.wino) and changed == [which], changed
    assert after.wino[which] == before.wino[which][:-len("/f6")]           # that launch is bf16x3 now, all others as before
    assert len(after.reduced) == len(before.reduced) - 1
    assert e_after < e_before and e_after < TOL_EVAL


def test_calibrate_poisoned_conv0_is_the_one_site_demoted(env, monkeypatch):
    rep, before, after, e_before, e_after = _poisoned(env, 0, monkeypatch)
    _assert_one_site_demoted(rep, before, after, e_before, e_after, 0)


def test_calibrate_poisoned_conv1_behind_its_residual(env, monkeypatch):
    """Conv_1's launch adds the block's residual in its epilogue, and the audit compares the launches' outputs: the figure is
    relative to conv + residual.  Either the site is demoted like Conv_0's, or -- the residual hides the conv from the audit -- the
    model must still be within its budget of the oracle."""
    rep, before, after, e_before, e_after = _poisoned(env, 1, monkeypatch)
    if rep["demoted"]:
        _assert_one_site_demoted(rep, before, after, e_before, e_after, 1)
    else:
        assert after.wino == before.wino
        assert e_after < TOL_EVAL, "a conv over the bar hides behind its residual"


def test_calibrate_leaves_no_mode_switched_on_when_the_forward_raises(env, monkeypatch):
    ops = env["ops"]
    x, labels = _inputs(env)
    _, model, _ = _model(env, "f16f6")
    net = model.module
    with pytest.raises(AssertionError):
        net.calibrate(x[:, :, :8, :8, :8].contiguous(), labels)            # the wrong grid: the first (measuring) evaluation raises
    assert ops.CALIBRATE is None and ops.AUDIT is None and not ops._SCOPES
    real, calls = net._forward_eval, []

    def second_raises(xi, li):
        calls.append(1)
        if len(calls) == 2:
            assert ops.AUDIT == [] and ops.CALIBRATE is None               # step 2: the audited evaluation
            raise RuntimeError("boom")
        return real(xi, li)
    monkeypatch.setattr(net, "_forward_eval", second_raises)
    with pytest.raises(RuntimeError, match="boom"):
        net.calibrate(x, labels)
    assert ops.CALIBRATE is None and ops.AUDIT is None and not ops._SCOPES
    assert _all_sites(net) == []


def test_calibrate_model_reaches_the_net_and_demotions_survive(env, monkeypatch):
    """models.utils.calibrate_model (what evaler, bench.py and the tools call): through `.module`, training flag restored, None for a
    bf16x3 model; a demotion survives train() / eval() and an in-place load_state_dict of the same weights."""
    ops, mutils = env["ops"], env["mutils"]
    monkeypatch.setattr(ops, "WINO_EQ", True)
    cfg, model, sd = _model(env, "f16f6")
    net = model.module
    n_before = len(_evaluate(env, model).reduced)
    model.train()
    rep = mutils.calibrate_model(model, cfg, batch=2, timesteps=(900.0, 60.0), bar=0.0)
    assert net.training and model.training                                  # restored
    model.eval()
    assert rep is not None and rep["measured"] >= n_before and rep["audited"] == 2 * rep["measured"]
    assert len(rep["demoted"]) == rep["measured"] and _all_sites(net) == sorted((n, s) for n, s, _ in rep["demoted"])
    out = _evaluate(env, model)
    assert out.reduced == []
    # the bare network (no wrapper) is reached too, in eval mode, and stays there
    _, other, _ = _model(env, "f16f6", sd)
    rep_b = mutils.calibrate_model(other.module, cfg, batch=2, timesteps=(900.0, 60.0), bar=0.0)
    assert not other.module.training and [d[:2] for d in rep_b["demoted"]] == [d[:2] for d in rep["demoted"]]
    cfg3, plain, _ = _model(env, "bf16x3", sd)
    assert mutils.calibrate_model(plain, cfg3, batch=2, timesteps=(900.0,), bar=0.0) is None
    assert _all_sites(plain.module) == []
    sites = _all_sites(net)
    model.train(); model.eval()
    net.load_state_dict(sd, strict=True)
    again = _evaluate(env, model)
    assert _all_sites(net) == sites and again.reduced == [] and again.wino == out.wino
    assert torch.equal(again.out, out.out)
