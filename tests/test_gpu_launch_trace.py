"""Which exports the U-Net's host path launches, in which order, with which scalar arguments: equal, element for element, to
tests/golden/launch_trace.json.gz (tools/gen_golden_launch_trace.py; recorded on the commit named in the file, the parent of the
conv-dispatch refactor).  Routes that are bit-identical by construction (block pass vs. prep + NIN, compact vs. full upsampled
operand) are invisible to every numerical test; this one sees them.  It only observes: the scenarios are the generator's own."""
import functools
import os
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENARIOS = ["a_small_eval_then_train", "b_res128_s32_f16f6", "b_res128_s16_f16f6", "b_res128_s32_bf16x3", "b_res128_s32_f16f8",
             "c_nin_s32_block_pass", "c_nin_s16_b8", "c_nin_s32_parts_72_184", "c_nin_s32_demoted_w0", "d_ups_8_uncalibrated",
             "d_ups_8_measured", "d_ups_4", "e_down_64", "e_down_32", "f_attn_fused", "f_attn_unfused", "g_train_s32_b2",
             "g_train_s32_b1", "h_res64_eval_b1"]


@functools.lru_cache(maxsize=None)
def _golden():
    import gen_golden_launch_trace as gen
    return gen.load_golden()["scenarios"]


def test_golden_covers_the_generators_scenarios(hip_lib):
    import gen_golden_launch_trace as gen
    assert list(gen.SCENARIOS) == SCENARIOS == list(_golden())


@pytest.mark.parametrize("name", SCENARIOS)
def test_launch_trace_equals_golden(hip_lib, name):
    import gen_golden_launch_trace as gen
    want = _golden()[name]
    got = gen.record(gen.SCENARIOS[name])
    assert len(want) > 0
    diff = gen.first_difference(got, want)
    assert diff is None, f"{name}: {diff}"
    assert got == want
