"""The K-sliced Winograd route of the 8^3 level on the CPU (hip_ops.wino_splitk_for, layers.plan_conv3, md_conv3_wino_splitk):

  gate      the plan at the bench shapes (512 output channels at 8^3, B = 8) and on both sides of every bound: unsplit workgroups
            n = 62 | 64 and 126 | 128 (n is even at 8^3; the floor moved to 65 shows the side 64 lies on), kdim 224 / 256, an
            upsampled input, a training scope, the switch off
  addresses a host replay of the three prologue addresses of csrc/conv3_wino.hip that depend on the slice: every (row block, slice,
            step) weight offset is the offset of the same (row block, global step) of the unsplit launch, for the bf16x3 step layout
            and the f16f8 / f16f6 pair-step layout; the operand of "sample" b * ks + s of the T view [B ks][cs / 8].. is the slice's
            part of sample b of the unsplit T; the output slabs of the workspace are disjoint and in the finish kernel's order."""
import itertools

import pytest

from test_cpu_conv_plan import GN, TRAIN, _plan


@pytest.fixture()
def env(hip_lib, monkeypatch):
    from meshdiffusion_amd import hip_ops as ops
    from meshdiffusion_amd.lib.diffusion.models import layers
    assert ops.FORCE_PRECISION is None and ops.WINO and ops.WINO_MIN_WGS == 128
    monkeypatch.setattr(ops, "WINO_SPLITK", True)
    return ops, layers


def _wino(layers, ks, stats=True):
    return layers.Conv3Plan("wino", "f6", False, False, False, stats, ks, False)


# the 8^3 convs of one sampling step at B = 8 (kdim -> 512) and the slices the issue names for them
BENCH = [(512, 4), (1024, 4), (768, 4), (256, 4)]


@pytest.mark.parametrize("cin,ks", BENCH)
def test_bench_shapes_take_four_slices(env, cin, ks):
    ops, layers = env
    assert ops.wino_splitk_for(512, cin, 8, 8) == ks
    assert _plan(ops, layers, (cin, 512, 8, 8), "f16f6", GN) == _wino(layers, ks)
    # a site the calibration audit demoted runs the same route in bf16x3
    assert _plan(ops, layers, (cin, 512, 8, 8), "f16f6", dict(GN, sites=("w0",))) == _wino(layers, ks)._replace(fmt=False)
    assert _plan(ops, layers, (cin, 512, 8, 8), "bf16x3", GN) == _wino(layers, ks)._replace(fmt=False)


def test_workgroup_bounds(env, monkeypatch):
    """n = B * 2 * (rows / 128) unsplit workgroups: 64 <= n < WINO_MIN_WGS."""
    ops, layers = env
    # (rows, B) -> n
    assert ops.wino_splitk_for(128, 256, 8, 31) == 0 and _plan(ops, layers, (256, 128, 8, 31), "f16f6", GN).path == "direct"          # n = 62
    assert ops.wino_splitk_for(896, 256, 8, 4) == 0                                                                                   # n = 56
    # n is even at 8^3 (two tiles per sample), so 63 and 127 do not occur: 62 | 64 and 126 | 128 are the neighbours, and the floor
    # moved by one shows on which side of it 64 lies
    assert ops.WINO_SPLITK_MIN_WGS == 64
    with monkeypatch.context() as m:
        m.setattr(ops, "WINO_SPLITK_MIN_WGS", 65)
        assert ops.wino_splitk_for(512, 512, 8, 8) == 0                             # n = 64
    assert ops.wino_splitk_for(512, 512, 8, 8) == 4
    assert ops.wino_splitk_for(128, 256, 8, 32) == 4                                # n = 64: 256 workgroups
    assert ops.wino_splitk_for(128, 512, 8, 63) == 2                                # n = 126: 252 workgroups
    assert _plan(ops, layers, (512, 128, 8, 63), "f16f6", GN) == _wino(layers, 2)
    assert ops.wino_splitk_for(128, 512, 8, 64) == 0                                # n = 128: the unsplit launch (wino_ok)
    assert _plan(ops, layers, (512, 128, 8, 64), "f16f6", GN) == _wino(layers, 1)
    assert ops.wino_splitk_for(768, 512, 8, 8) == 2                                 # n = 96: 4 slices would be 384 workgroups
    assert ops.wino_splitk_for(1024, 512, 8, 8) == 0 and ops.wino_ok(1024, 512, 8, 8)
    # other levels never: 4^3 is not a grid of the kernel, 16^3 has its own floor
    assert ops.wino_splitk_for(512, 512, 4, 64) == 0 and ops.wino_splitk_for(512, 512, 16, 1) == 0


def test_kdim_bounds_and_slice_size(env):
    ops, layers = env
    assert ops.wino_splitk_for(512, 224, 8, 8) == 0 and _plan(ops, layers, (224, 512, 8, 8), "f16f6", GN).path == "direct"
    assert ops.wino_splitk_for(512, 256, 8, 8) == 4
    assert ops.wino_splitk_for(512, 288, 8, 8) == 0          # 288 = 9 x 32: no even number of whole 32-channel slices
    assert ops.wino_splitk_for(512, 320, 8, 8) == 2          # 10 x 32
    assert ops.wino_splitk_for(512, 384, 8, 8) == 4
    for rows, kdim, B in itertools.product((128, 256, 512, 640), range(256, 1089, 32), (4, 8, 16, 24)):
        ks = ops.wino_splitk_for(rows, kdim, 8, B)
        n = B * 2 * (rows // 128)
        if ks:
            assert ks in (2, 4, 8) and kdim % (32 * ks) == 0 and 64 <= n < 128 and n * ks <= 256
            assert all(kdim % (32 * k) or n * k > 256 for k in (8, 4, 2) if k > ks)      # the largest that fits


def test_ups_training_and_switch(env, monkeypatch):
    ops, layers = env
    conv = (512, 512, 8, 8)
    assert ops.wino_splitk_for(512, 512, 8, 8, ups=1) == 0
    assert _plan(ops, layers, conv, "f16f6", dict(ups=1, measured=True)).path == "direct"
    assert _plan(ops, layers, conv, "train", TRAIN).path == "direct"
    assert _plan(ops, layers, conv, "train", dict(TRAIN, keep=True)).path == "direct"
    assert _plan(ops, layers, conv, "f16f6", dict(GN, drop=(0.1, 7))).path == "direct"        # dropout: a training operand
    assert _plan(ops, layers, conv, "f16f6", dict(GN, out_mode="OUT_S16B")).path == "direct"
    assert _plan(ops, layers, conv, "f16f6", dict(operand=False)).path == "direct"
    with monkeypatch.context() as m:
        m.setattr(ops, "WINO", False)
        assert _plan(ops, layers, conv, "f16f6", GN).path == "direct"
    with monkeypatch.context() as m:
        m.setattr(ops, "WINO_SPLITK", False)
        plan = _plan(ops, layers, conv, "f16f6", GN)
        assert plan == layers.Conv3Plan("direct", False, False, False, False, True, 4, True)      # what the parent ran


def test_pinned_plans_do_not_move_with_the_switch_on(env):
    import test_cpu_conv_plan as pinned
    ops, layers = env
    for _, conv, scope, opt, want in pinned.CASES:
        assert _plan(ops, layers, conv, scope, opt) == layers.Conv3Plan(*want)


# ---- host replay of the slice-dependent addresses (csrc/conv3_wino.hip: tbase, wbase / wbase8, outp) --------------------------------
def _unsplit_weight_item(rtb, gstep, wid, nsteps_full, pair):
    """16-byte item of (row block, global step or pair-step, frequency) in the packed image, lane 0, piece 0."""
    if pair:
        return ((rtb * (nsteps_full // 2)) * 4 + wid) * 1024 + gstep * 4096
    return ((rtb * nsteps_full) * 4 + wid) * 512 + gstep * 2048


def _split_weight_item(rtb, sl, step, wid, nsteps_full, nsteps, pair):
    if pair:
        return ((rtb * (nsteps_full // 2) + sl * (nsteps // 2)) * 4 + wid) * 1024 + step * 4096
    return ((rtb * nsteps_full + sl * nsteps) * 4 + wid) * 512 + step * 2048


@pytest.mark.parametrize("cin,ks,row_blocks", [(64, 2, 1), (128, 4, 2), (512, 4, 4), (1024, 4, 4), (768, 4, 4), (256, 4, 4), (512, 8, 2)])
@pytest.mark.parametrize("pair", [False, True], ids=["bf16x3_steps", "pair_steps"])
def test_weight_offsets_equal_the_unsplit_layout(cin, ks, row_blocks, pair):
    cs = cin // ks
    assert cs % 32 == 0
    nsteps_full, nsteps = (cin // 16) * 9, (cs // 16) * 9
    assert nsteps % 2 == 0                       # 9 taps x an even chunk count: a slice starts on a pair-step boundary
    seen = set()
    for rtb, sl, wid in itertools.product(range(row_blocks), range(ks), range(4)):
        for step in range(nsteps // 2 if pair else nsteps):
            gstep = sl * (nsteps // 2 if pair else nsteps) + step
            off = _split_weight_item(rtb, sl, step, wid, nsteps_full, nsteps, pair)
            assert off == _unsplit_weight_item(rtb, gstep, wid, nsteps_full, pair)
            seen.add(off)
    # together the slices read every (row block, step, frequency) of the image exactly once: cout * cin * 36 * 4 bytes in all
    per = 1024 if pair else 512
    assert len(seen) == row_blocks * (nsteps_full // 2 if pair else nsteps_full) * 4
    assert (max(seen) + per) * 16 == row_blocks * 128 * cin * 36 * 4


@pytest.mark.parametrize("B,cin,ks", [(1, 64, 2), (2, 128, 4), (8, 512, 4), (8, 1024, 4)])
def test_operand_view_and_output_slabs(B, cin, ks):
    Ph, P, cout = 8 * 8 * 4, 512, 128
    cs = cin // ks
    slabs = []
    for b, sl, wid in itertools.product(range(B), range(ks), range(4)):
        bp = b * ks + sl
        assert (bp % ks, bp // ks) == (sl, b)
        for chunk in range(cs // 16):
            split = (bp * (cs // 8) * 8 + wid * 2) * Ph + chunk * 16 * Ph                       # tbase + chunk * 16 * Ph, CG = cs / 8
            unsplit = (b * (cin // 8) * 8 + wid * 2) * Ph + (sl * (cs // 16) + chunk) * 16 * Ph
            assert split == unsplit
        if wid == 0:
            slabs.append((sl * B + b) * cout * P)                                                 # outp, floats
    # workspace [ks][B][cout / 8][P][8]: slice-major, as md_splitk_reduce_kernel strides it (slice = B * rows * P floats)
    assert sorted(slabs) == [i * cout * P for i in range(ks * B)]
    assert all(off == sl * (B * cout * P) + b * cout * P for off, (b, sl) in zip(slabs, itertools.product(range(B), range(ks))))
