"""The preconditions of tests/test_gpu_calibration.py on the CPU, so that they are not hopes: the torch restatement of the f16f6
arithmetic (tests/test_gpu_wino.py) on tests/calibration_cases.py at the reduced size (cin 128, cout 32, 8^3, B 2), against float64;
and layers.plan_conv3 on a demoted site (a stub builder: owner, site, measured) at every f16f6 row of tests/test_cpu_conv_plan.py."""
import functools

import pytest
import torch

import calibration_cases as cc
from test_cpu_conv_plan import CASES, _plan, env  # noqa: F401  (env: the module fixture of the plan tests)

SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _figure(name, seed):
    case = cc.layer_case(name, "cpu", seed)
    return cc.rel(cc.emulated_f16f6(case), case.ref)


@pytest.mark.parametrize("seed", SEEDS)
def test_emulated_f16f6_is_over_the_bar_exactly_where_the_gpu_tests_need_it(seed):
    fig = {n: _figure(n, seed) for n in cc.LAYER_CASES}
    print(f"emulated f16f6 vs float64, seed {seed}: " + ", ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    assert fig["span6_noeq"] > 2 * cc.BAR
    assert fig["two_parts"] > cc.BAR
    assert fig["friendly"] < cc.BAR / 2 and fig["span6_eq"] < cc.BAR / 2


@pytest.mark.parametrize("seed", SEEDS)
def test_a_residual_in_the_epilogue_dilutes_the_figure(seed):
    """The same un-equalised span6 launch with and without a residual of 30 x the conv's rms: against an output that contains the
    residual the error is ~sqrt(1 + 30^2) times smaller, and under the bar."""
    case = cc.layer_case("residual30", "cpu", seed)
    y = cc.emulated_f16f6(case)
    diluted, bare = cc.rel(y, case.ref), cc.rel(y - case.residual, case.ref_conv)
    print(f"residual30 seed {seed}: conv alone {bare:.2e}, with the residual {diluted:.2e}, factor {bare / diluted:.1f}")
    rms = lambda t: t.double().pow(2).mean().sqrt()                          # noqa: E731
    assert abs(float(rms(case.residual) / rms(case.ref_conv)) - cc.RESIDUAL_FACTOR) < 0.5
    assert bare > 2 * cc.BAR and bare / diluted >= 10.0


def test_triangle_bounds_hold_for_vectors():
    """The derivation of cc.triangle_bounds, on random vectors at the magnitudes of the tests."""
    g = torch.Generator().manual_seed(0)
    r = torch.randn(4096, generator=g, dtype=torch.float64)
    for er, eb in ((3e-4, 6e-6), (1.8e-5, 6e-6), (6e-6, 6e-6), (1e-6, 2e-5)):
        y_r = r + er * torch.randn(4096, generator=g, dtype=torch.float64)
        y_b = r + eb * torch.randn(4096, generator=g, dtype=torch.float64)
        lo, hi = cc.triangle_bounds(cc.rel(y_r, r), cc.rel(y_b, r))
        assert lo <= cc.rel(y_r, y_b) <= hi


def test_poison_rescales_one_pair_only():
    sd = {f"all_modules.3.{k}": torch.rand(s) + 0.5 for k, s in (("GroupNorm_0.weight", (128,)), ("GroupNorm_0.bias", (128,)),
                                                                  ("Conv_0.weight", (32, 128, 3, 3, 3)), ("GroupNorm_1.weight", (32,)),
                                                                  ("GroupNorm_1.bias", (32,)), ("Conv_1.weight", (32, 32, 3, 3, 3)))}
    out = cc.poison(sd, "all_modules.3", 0)
    s = out["all_modules.3.GroupNorm_0.weight"] / sd["all_modules.3.GroupNorm_0.weight"]
    assert float(s.max() / s.min()) > 2.0 ** 8 and float(s.max()) <= 64.0 and float(s.min()) >= 1 / 64.0
    assert torch.allclose(out["all_modules.3.GroupNorm_0.bias"], sd["all_modules.3.GroupNorm_0.bias"] * s)
    assert torch.allclose(out["all_modules.3.Conv_0.weight"] * s.view(1, -1, 1, 1, 1), sd["all_modules.3.Conv_0.weight"])
    assert all(torch.equal(out[k], sd[k]) for k in sd if "_1." in k)
    assert out["all_modules.3.Conv_0.weight"] is not sd["all_modules.3.Conv_0.weight"]


F16F6_ROWS = [c for c in CASES if c[2] == "f16f6"]


@pytest.mark.parametrize("case", F16F6_ROWS, ids=[c[0] for c in F16F6_ROWS])
def test_plan_of_a_demoted_site(env, case):  # noqa: F811
    """A site in md_bf16x3_sites: no reduced-precision format and no block pass (which exists in f16f6 only), whatever the row's
    operand; path, compact layout, statistics and every direct-kernel field as without the demotion.  A demotion of ANOTHER site of
    the same layer changes nothing."""
    ops, layers = env
    _, conv, scope, opt, want = case
    demoted_row = "sites" in opt                                                 # the row that is already a hand-demoted site
    opt = {k: v for k, v in opt.items() if k != "sites"}
    plain = _plan(ops, layers, conv, scope, opt)
    assert demoted_row or plain == layers.Conv3Plan(*want)
    demoted = _plan(ops, layers, conv, scope, dict(opt, sites=("w0",)))          # the stub builder's site is "w0"
    assert demoted.fmt is False and demoted.shortcut_in_pass is False
    assert demoted == plain._replace(fmt=False, shortcut_in_pass=False)
    assert demoted.compact == plain.compact
    assert _plan(ops, layers, conv, scope, dict(opt, sites=("w1", "w"))) == plain
