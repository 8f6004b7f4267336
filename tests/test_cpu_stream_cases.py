"""The cases of tests/test_gpu_stream_f64.py, proven without a GPU (tests/stream_cases.py holds them).

For every kernel family an fp32 torch emulation with the kernel's summation tree must lie INSIDE the derived bound of every
case, and one-line mutations of that emulation -- the mistakes such kernels make -- must land OUTSIDE it by at least MARGIN.
So the GPU test can fail, and does not fail on a correct kernel.  Each case is also shown to be in the regime its name claims.
"""
import math

import pytest
import torch

import stream_cases as sc

MARGIN = 4.0

GN_CASES = sc.gn_cases()
ADAM_CASES = sc.adam_cases()


def _by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------
def _gn_worst(case, emu, silu):
    """Largest |emulation - float64| / bound over the output and over each stored parameter."""
    ref, pb = sc.gn_reference(case, silu), sc.gn_param_bounds(case)
    got = emu["hi"].double() + emu["lo"].double()
    rel, w_out = sc.gn_measure(got, ref["out"], sc.gn_bound(case, silu))
    w = dict(out=w_out, rel=rel)
    for k in ("mean", "rstd", "a", "c"):
        w[k] = float(((emu[k].double() - ref[k]).abs() / pb[k].clamp_min(1e-300)).max())
    return w


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: c["name"])
def test_gn_emulation_inside_bound(case):
    for silu in (False, True):
        w = _gn_worst(case, sc.emulate_gn(case, silu), silu)
        print(f"{case['name']} silu={int(silu)}: elementwise {w['rel']:.2e}, worst/bound out {w['out']:.3f} mean {w['mean']:.3f} "
              f"rstd {w['rstd']:.3f} a {w['a']:.3f} c {w['c']:.3f}")
        assert max(w["out"], w["mean"], w["rstd"], w["a"], w["c"]) <= 1.0, w
        if case["ratio"] == sc.GN_SERVED_RATIO:
            assert w["rel"] <= sc.GN_SERVED_TOL
    assert torch.equal(sc.emulate_gn(case, False)["beta"], case["beta"][None].expand(case["B"], -1))


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: c["name"])
def test_gn_case_regime(case):
    mean, var, n, _, _ = sc.gn_group_stats(case)
    live = torch.ones(sc.GN_GROUPS, dtype=torch.bool)
    if case["const_group"] is not None:
        live[case["const_group"]] = False
        assert float(var[:, case["const_group"]].abs().max()) == 0.0            # exact: the kernel must return beta
        assert float(mean[:, case["const_group"]].min()) == 3.25 == float(mean[:, case["const_group"]].max())
    ratio = mean.abs() / var.sqrt().clamp_min(1e-300)
    if case["ratio"]:
        assert float((ratio[:, live] / case["ratio"] - 1).abs().max()) < 0.01, "mean/std is not what the name says"
    elif not case["spread"]:
        assert float(ratio[:, live].max()) < 0.5
    if case["spread"]:      # channel means inside one group differ by several of the channel's own std (1)
        cm = case["x"].double().mean(-1).reshape(case["B"], sc.GN_GROUPS, case["cpg"])
        assert float((cm.amax(-1) - cm.amin(-1)).min()) > 3.0
    assert case["C"] % sc.GN_GROUPS == 0 and case["C"] % 8 == 0 and all(p % 8 == 0 for p in case["parts"])
    if case["name"].startswith("concat"):
        edge, cpg = case["parts"][0], case["cpg"]
        assert edge % cpg != 0 and edge // cpg == 13                             # the boundary is inside group 13
    if case["name"].startswith("chunk"):
        assert case["P"] in (sc.GN_CHUNK - 1, sc.GN_CHUNK, sc.GN_CHUNK + 1)
    if case["name"].startswith("P4100"):
        assert -(-case["P"] // sc.GN_CHUNK) == 3
    if case["name"].startswith("P210"):
        assert case["cpg"] == 3 and case["P"] % 2 == 0 and case["P"] % 4 != 0 and case["B"] % 2 == 1
    if case["name"].startswith("cpg65"):
        assert case["cpg"] > 64


@pytest.mark.parametrize("name,mut", [("chunk-P2049", "drop_tail"), ("chunk-P2049", "padded_n"), ("P4100-ratio0", "padded_n"),
                                      ("concat40+56-P45", "neighbour_part"), ("chunk-P2048", "swap_pair")])
def test_gn_mutation_outside_bound(name, mut):
    case = _by_name(GN_CASES, name)
    for silu in (False, True):
        w = _gn_worst(case, sc.emulate_gn(case, silu, mut=mut), silu)
        print(f"{name} {mut} silu={int(silu)}: worst/bound out {w['out']:.1f} mean {w['mean']:.1f} rstd {w['rstd']:.1f} a {w['a']:.1f}")
        assert w["out"] >= MARGIN                                                # the elementwise check sees it
        assert max(w["mean"], w["rstd"], w["a"]) >= MARGIN                       # and so does the check of the stored parameters


def test_gn_rounding_counts():
    assert sc.gn_stat_roundings(64) == (5, 6)            # one value per accumulator: the butterfly only
    assert sc.gn_stat_roundings(210) == (6, 7)
    assert sc.gn_stat_roundings(2048) == (sc.GN_KS, sc.GN_KQ) == (12, 13)       # capped: the source counts 20 and 21
    assert sc.GN_CHUNK == sc.GN_ITEMS * sc.GN_STRIDE


def test_network_groupnorm_offsets():
    """The largest group |mean| / std at any GroupNorm of the small nets, measured with the oracle: the ratio the GroupNorm cases
    must serve (GN_SERVED_RATIO) is twice it, rounded up to a power of two."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, ddpm_res128, utils as mutils  # noqa: F401
    from oracle import unet_oracle as uo
    seen = []
    plain = uo.group_norm

    def recording(x, w, b):
        xg = x.double().reshape(x.shape[0], sc.GN_GROUPS, -1)
        seen.append(float((xg.mean(-1).abs() / xg.var(-1, unbiased=False).sqrt().clamp_min(1e-30)).max()))
        return plain(x, w, b)

    uo.group_norm = recording
    try:
        worst = {}
        for arch, make in (("res64", synth.small_config), ("res128", synth.small_config_res128)):
            cfg = make(); cfg.device = torch.device("cpu")
            model = mutils.create_model(cfg)
            R = cfg.data.image_size
            tmpl = getattr(model, "module", model).state_dict()
            for wname, fn in (("sensitised", synth.sensitised_state_dict), ("trained_like", synth.trained_like_state_dict)):
                sd = fn(tmpl, grid_mask=synth.synthetic_grid_mask(R))
                seen.clear()
                for labels in ([0, 999], [417, 50]):
                    with torch.no_grad():
                        uo.unet_res64_forward(sd, synth.oracle_cfg(cfg), synth.synthetic_inputs(2, 4, R, seed=42), torch.tensor(labels))
                worst[arch, wname] = max(seen)
    finally:
        uo.group_norm = plain
    print({k: round(v, 3) for k, v in worst.items()})
    top = max(worst.values())
    assert abs(top - sc.GN_NETWORK_RATIO) < 0.01, top
    assert sc.GN_SERVED_RATIO == 2 ** math.ceil(math.log2(2 * top))


# ---------------------------------------------------------------------------------------------------------------
# small kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.linear_cases(), ids=lambda c: c["name"])
def test_linear_emulation_inside_bound(case):
    ref, _ = sc.linear_reference(case)
    bound = sc.linear_bound(case)
    w = float(((sc.emulate_linear(case).double() - ref).abs() / bound).max())
    assert w <= 1.0, w
    # one dropped input (the last lane of the last trip) and a batch row served by its neighbour are both far outside
    if case["x"].shape[1] > 1:
        short = dict(case, x=torch.cat([case["x"][:, :-1], torch.zeros(case["x"].shape[0], 1)], 1))
        assert float(((sc.emulate_linear(short).double() - ref).abs() / bound).max()) >= MARGIN
    if case["x"].shape[0] > 8:
        rolled = dict(case, x=torch.cat([case["x"][:8], case["x"][:1].expand(case["x"].shape[0] - 8, -1)]))
        assert float(((sc.emulate_linear(rolled).double() - ref).abs() / bound).max()) >= MARGIN


def test_linear_cases_cover_every_value():
    cs = sc.linear_cases()
    assert {c["x"].shape[0] for c in cs} == {1, 8, 9, 19} and {c["x"].shape[1] for c in cs} == {1, 63, 64, 65, 512}
    assert {c["w"].shape[0] for c in cs} == {5, 510, 512}
    assert {(c["bias"] is None, c["silu"]) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}


@pytest.mark.parametrize("dim", sc.TEMB_DIMS)
def test_temb_emulation_inside_bound(dim):
    ref, bound = sc.temb_reference(dim)
    emu = sc.emulate_temb(dim)
    half = dim // 2
    assert bool(((emu.double() - ref).abs() <= bound).all())
    if dim % 2:
        assert float(bound[:, -1].max()) == 0.0 and float(ref[:, -1].abs().max()) == 0.0
    # the frequency table built with half instead of half - 1 in the divisor is outside
    if half > 2:
        neg = torch.tensor(-(math.log(10000.0) / half), dtype=torch.float64).float()
        arg = torch.tensor(sc.TEMB_T)[:, None] * torch.exp(torch.arange(half, dtype=torch.float32) * neg)[None]
        assert float(((torch.sin(arg).double() - ref[:, :half]).abs() / bound[:, :half]).max()) >= MARGIN


# ---------------------------------------------------------------------------------------------------------------
# md_masked_sq_err, md_grad_sqnorm
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.sq_err_cases(), ids=lambda c: c["name"])
def test_sq_err_emulation_inside_bound(case):
    ref, bound, _ = sc.sq_err_reference(case)
    err = (sc.emulate_sq_err(case) - ref).abs()
    assert bool((err <= bound).all()), (err / bound.clamp_min(1e-300)).max()
    d = (case["eps_hat"] - case["noise"]).abs()
    assert 0 < float(d.max()) < 1e-5                                   # the cancelling regime: eps_hat - noise is ulps of noise
    if case["name"] == "zero-mask":
        assert float(ref.abs().max()) == 0.0
    if case["name"] == "onto-nonzero":
        assert float(case["sums0"].min()) >= 1.0
    if case["name"].startswith("wrap"):
        assert case["C"] * case["P"] > 256 * 256 * 4
        miss = (sc.emulate_sq_err(case, mut="skip_second_trip") - ref).abs()
        assert float((miss / bound).min()) >= MARGIN
    else:
        assert case["C"] * case["P"] <= 256 * 256 * 4 and case["P"] % 4 == 0


@pytest.mark.parametrize("n,scale,mixed", sc.sqnorm_params())
def test_sqnorm_emulation_inside_bound(n, scale, mixed):
    case = sc.sqnorm_case(n, scale, mixed=mixed)
    ref, bound = sc.sqnorm_reference(case)
    assert abs(sc.emulate_sqnorm(case) - ref) <= bound
    assert math.isfinite(ref) and ref > 0
    if mixed:
        a = case["g"].abs()
        assert float(a.max() / a[a > 0].min()) > 1e12
    if n % 4 and not mixed:                                            # the tail matters at every size, 1 048 579 included
        assert abs(sc.emulate_sqnorm(case, mut="skip_tail") - ref) >= MARGIN * bound
    if n // 4 > 1024 * 256:
        assert abs(sc.emulate_sqnorm(case, mut="skip_second_trip") - ref) >= MARGIN * bound


def test_sqnorm_sizes():
    assert {n % 4 for n in sc.SQNORM_N} == {0, 1, 2, 3}
    assert (1048576 + 3) // 4 == 1024 * 256                           # the size the cases were specified with stops at the first trip,
    assert max(sc.SQNORM_N) // 4 > 1024 * 256                         # so one more size takes the second


# ---------------------------------------------------------------------------------------------------------------
# md_adam_ema_step
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ADAM_CASES, ids=lambda c: c["name"])
def test_adam_emulation_inside_bound(case):
    ref = sc.adam_reference(case)
    w = sc.adam_worst(sc.emulate_adam(case), case, ref)
    print(case["name"], {k: round(v, 3) for k, v in w.items()})
    assert max(w.values()) <= 1.0, w
    # the regime: what a step moves dominates what the roundings of p and ema themselves cost
    assert float((ref["dp"].abs() / (sc.U * ref["p"].abs()).clamp_min(1e-300)).median()) > 1e4
    if case["ema"] is not None:
        assert float((ref["dema"].abs() / (sc.U * ref["ema"].abs()).clamp_min(1e-300)).median()) > 1e3
    norm = float(case["g"].double().norm())
    if case["clip"] == "under":
        assert 0.985 < norm / sc.ADAM_MAX_NORM < 0.995 and ref["clip"] == 1.0
    if case["clip"] == "over":
        assert 1.005 < norm / sc.ADAM_MAX_NORM < 1.015 and 0.985 < ref["clip"] < 0.995
    if case["clip"] in ("off", "nosq"):
        assert ref["clip"] == 1.0 and case["sq"] is None and (case["max_norm"] < 0) == (case["clip"] == "off")


def test_adam_cases_cover_every_value():
    assert {c["n"] for c in ADAM_CASES} >= {1, 3, 255, 257, 524288 + 5} and 524288 + 5 > 2048 * 256
    assert {c["step"] for c in ADAM_CASES} == {1, 2, 1000, 10 ** 6}
    assert {(c["clip"], c["wd"]) for c in ADAM_CASES} >= {(k, w) for k in ("off", "nosq", "under", "over") for w in (0.0, 0.01)}
    assert {c["d"] for c in ADAM_CASES if c["ema"] is not None} == {2 / 11, 0.999, 0.9999}
    assert any(c["ema"] is None for c in ADAM_CASES)
    assert sc.ema_decay(0.9999, 1) == 2 / 11 and sc.ema_decay(0.9999, 10 ** 6) == 0.9999


ADAM_MUTATIONS = [("no_clip", "clip-over-wd0.0", "dp"), ("no_clip", "n524293", "dp"),
                  ("bc_step_minus_1", "step2", "dp"), ("bc_step_minus_1", "step1000", "dp"),
                  ("mul_bc2", "step1", "dp"), ("mul_bc2", "step2", "dp"), ("mul_bc2", "step1000", "dp"),
                  ("ema_rate_f32", "d0.9999", "dema"), ("ema_rate_f32", "d0.9990", "dema"), ("ema_rate_f32", "n524293", "dema"),
                  ("skip_second_trip", "n524293", "dp"), ("skip_second_trip", "n524293", "dema"), ("skip_second_trip", "n524293", "v"),
                  ("no_wd", "clip-off-wd0.01", "dp"), ("no_wd", "clip-over-wd0.01", "dp"),
                  # betas that went through a float before 1 - beta and the bias corrections were formed: the kernel before this suite
                  ("betas_f32", "step1", "v"), ("betas_f32", "step2", "dp"), ("betas_f32", "step1000", "dp"), ("betas_f32", "n524293", "dp")]


@pytest.mark.parametrize("mut,name,key", ADAM_MUTATIONS)
def test_adam_mutation_outside_bound(mut, name, key):
    case = _by_name(ADAM_CASES, name)
    ref = sc.adam_reference(case)
    w = sc.adam_worst(sc.emulate_adam(case, mut=mut), case, ref)
    print(mut, name, {k: round(v, 1) for k, v in w.items()})
    assert w[key] >= MARGIN, w


def test_ema_rate_of_the_old_kernel():
    """1.f - (float)d against the reference's (float)(1.0 - d): 1.66e-4 relative at d = 0.9999, and the same kind of error in the
    second-moment weight 1.f - (float)beta2: 1.3e-5 at 0.999."""
    T = lambda x: torch.tensor(x, dtype=torch.float32)
    old, new = float(T(1.0) - T(0.9999)), sc.f32(1.0 - 0.9999)
    assert abs(old / new - 1) == pytest.approx(1.66e-4, rel=0.01)
    old, new = float(T(1.0) - T(0.999)), sc.f32(1.0 - 0.999)
    assert abs(old / new - 1) == pytest.approx(1.29e-5, rel=0.01)


def test_adam_three_steps_carry_state():
    """Three emulated steps on one state stay inside the bounds of three float64 steps taken from the fp32 state before each."""
    case = sc.adam_case("carry", 257, 1, wd=0.01, clip="over", d=0.9999)
    for step in (1, 2, 3):
        case = dict(case, step=step, d=sc.ema_decay(0.9999, step))
        ref = sc.adam_reference(case)
        p, m, v, s = sc.emulate_adam(case)
        assert max(sc.adam_worst((p, m, v, s), case, ref).values()) <= 1.0
        g = torch.randn(257, generator=torch.Generator().manual_seed(900 + step)) * 0.0631
        case = dict(case, p=p, m=m, v=v, ema=s, g=g, sq=float((g.double() ** 2).sum()))
