"""layers.plan_conv3 on the CPU: the route of a 3x3x3 convolution at the shapes on both sides of every dispatch boundary (the
scenarios b-d and g of tools/gen_golden_launch_trace.py and one step to the other side of each).  The expected plans are written
out; each agrees with what the hip_ops predicates (wino_ok, wino_f8_ok, prep_compact_ok, block_pass_ok, ksplit_for) return."""
import pytest


class _PW:
    """What plan_conv3 reads of a PackedWeight."""

    def __init__(self, ops, cin, cout, S):
        self.rows, self.kdim, self.cfg, self.prec = cout, (cin + 31) // 32 * 32, ops.conv_cfg_for(S), ops.PREC_BF16X3


class _Owner:
    md_bf16x3_sites = ()


class _Wino:
    """What plan_conv3 reads of a conv3_wino_packed builder."""

    def __init__(self, ms=None, sites=()):
        self.owner, self.site, self._ms = _Owner(), "w0", ms
        self.owner.md_bf16x3_sites = sites

    def measured(self):
        return self._ms


class _NIN:
    rows = 128


# (id, conv (cin, cout, S_out, B), scope, operand / call options, expected plan fields
#  (path, fmt, compact, shortcut_in_pass, keep, stats, ksplit, fused_loader))
GN = dict(ac=True, silu=True)
TRAIN = dict(ac=True, silu=True, wino_only=True)
CASES = [
    # b: ResnetBlock 128 -> 128 in f16f6: 32^3 at B = 1 is exactly the 128-workgroup floor; 16^3 is below it
    ("res128_s32_f16f6", (128, 128, 32, 1), "f16f6", GN, ("wino", "f6", False, False, False, True, 1, False)),
    ("res128_s16_f16f6", (128, 128, 16, 1), "f16f6", GN, ("direct", False, False, False, False, False, 4, True)),
    ("res128_s32_f16f8", (128, 128, 32, 1), "f16f8", GN, ("wino", "f8", False, False, False, True, 1, False)),
    ("res128_s32_bf16x3", (128, 128, 32, 1), "bf16x3", GN, ("wino", False, False, False, False, True, 1, False)),
    # g: the same conv in a training scope needs 256 workgroups: B = 1 direct on the taped S16B activation, B = 2 Winograd with T kept
    ("train_s32_b1", (128, 128, 32, 1), "train", TRAIN, ("direct", False, False, False, False, False, 2, False)),
    ("train_s32_b2_keep", (128, 128, 32, 2), "train", dict(TRAIN, keep=True), ("wino", False, False, False, True, True, 1, False)),
    ("train_s32_b2_keep_drop", (128, 128, 32, 2), "train", dict(TRAIN, keep=True, drop=(0.1, 7)), ("wino", False, False, False, True, True, 1, False)),
    ("train_s32_b2_no_keep", (128, 128, 32, 2), "train", TRAIN, ("wino", False, False, False, False, True, 1, False)),
    # c: 256 -> 128 with a NIN shortcut: P = 32768 is the block pass's lower bound
    ("nin_s32_block_pass", (256, 128, 32, 1), "f16f6", dict(GN, nin=True), ("wino", "f6", False, True, False, True, 1, False)),
    ("nin_s16_b8", (256, 128, 16, 8), "f16f6", dict(GN, nin=True), ("wino", "f6", False, False, False, True, 1, False)),
    ("nin_s32_parts_72_184", (256, 128, 32, 1), "f16f6", dict(GN, nin=True, split=(72, 184)), ("wino", "f8", False, False, False, True, 1, False)),
    ("nin_s32_demoted", (256, 128, 32, 1), "f16f6", dict(GN, nin=True, sites=("w0",)), ("wino", False, False, False, False, True, 1, False)),
    ("nin_s32_bf16x3", (256, 128, 32, 1), "bf16x3", dict(GN, nin=True), ("wino", False, False, False, False, True, 1, False)),
    # d: Upsample 128 at B = 8: the raw residual stream stays bf16x3 until a calibration measured it; 16^3 compact, 8^3 direct
    ("ups_16_uncalibrated", (128, 128, 16, 8), "f16f6", dict(ups=1), ("wino", False, True, False, False, True, 1, False)),
    ("ups_16_measured", (128, 128, 16, 8), "f16f6", dict(ups=1, measured=True), ("wino", "f6", True, False, False, True, 1, False)),
    ("ups_16_train", (128, 128, 16, 16), "train", dict(ups=1, wino_only=True, keep=False), ("wino", False, False, False, False, True, 1, False)),
    ("ups_8", (128, 128, 8, 8), "f16f6", dict(ups=1), ("direct", False, False, False, False, False, 4, True)),
    # the output layout: anything but F32B without padded rows goes to the direct kernel, without statistics
    ("out_s16b", (128, 128, 32, 1), "f16f6", dict(GN, out_mode="OUT_S16B"), ("direct", False, False, False, False, False, 1, True)),
    ("rows_padded", (128, 128, 32, 1), "f16f6", dict(GN, rows_alloc=136), ("direct", False, False, False, False, False, 2, True)),
    ("no_operand", (128, 128, 32, 1), "f16f6", dict(operand=False), ("direct", False, False, False, False, False, 2, False)),
    # statistics of the direct kernel: its epilogue without split-K, the split-K finish kernel at P <= 512 with B * rows >= 2048
    ("direct_splitk_stats", (256, 256, 8, 8), "f16f6", GN, ("direct", False, False, False, False, True, 8, True)),
    ("direct_splitk_no_stats", (256, 256, 8, 4), "f16f6", GN, ("direct", False, False, False, False, False, 8, True)),      # 8 K chunks cap the split
]


def _plan(ops, layers, conv, scope, opt, want_stats=True):
    cin, cout, S, B = conv
    pw = _PW(ops, cin, cout, S)
    operand = None
    if opt.get("operand", True):
        parts = [(None, c) for c in opt.get("split", (cin,))]      # plan_conv3 reads the channel counts only
        operand = ops.F32Operand(parts, ac=object() if opt.get("ac") else None, silu=opt.get("silu", False), drop=opt.get("drop"),
                                 keep=opt.get("keep", False), wino_only=opt.get("wino_only", False),
                                 nin=(_NIN(), None) if opt.get("nin") else None)
    wino = _Wino(ms=object() if opt.get("measured") else None, sites=opt.get("sites", ())) if operand is not None else None
    ctx = ops.precision_scope(None, training=True) if scope == "train" else ops.precision_scope(scope)
    with ctx:
        return layers.plan_conv3(pw, operand, B, S, ups=opt.get("ups", 0), out_mode=getattr(ops, opt.get("out_mode", "OUT_F32B")),
                                 rows_alloc=opt.get("rows_alloc", pw.rows), want_stats=want_stats, wino=wino)


@pytest.fixture(scope="module")
def env(hip_lib):       # ksplit_for asks the library for the tile geometry (host code: no GPU)
    from meshdiffusion_amd import hip_ops as ops
    from meshdiffusion_amd.lib.diffusion.models import layers
    assert ops.FORCE_PRECISION is None and ops.WINO and ops.WINO_EQ and ops.WINO_PREP_V2 and ops.PREP_COMPACT_UPS and ops.WINO_TRAIN_FWD
    return ops, layers


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_at_dispatch_boundaries(env, case):
    ops, layers = env
    _, conv, scope, opt, want = case
    plan = _plan(ops, layers, conv, scope, opt)
    assert plan == layers.Conv3Plan(*want)
    assert plan.fmt is False or plan.fmt in ("f8", "f6")
    # nothing accumulates statistics that were not asked for
    assert _plan(ops, layers, conv, scope, opt, want_stats=False) == plan._replace(stats=False)


def test_wino_off_is_direct_everywhere(env, monkeypatch):
    ops, layers = env
    monkeypatch.setattr(ops, "WINO", False)
    for _, conv, scope, opt, _ in CASES:
        plan = _plan(ops, layers, conv, scope, opt)
        assert plan[:5] == ("direct", False, False, False, False)
        assert plan.fused_loader == (opt.get("operand", True) and not opt.get("wino_only", False))
    # the dedicated kernel without split-K records the statistics in its epilogue
    assert _plan(ops, layers, (128, 128, 32, 8), "f16f6", GN) == layers.Conv3Plan("direct", False, False, False, False, True, 1, True)


def test_switches_the_plan_reads(env, monkeypatch):
    ops, layers = env
    ups, nin = CASES[14], CASES[8]
    assert ups[0] == "ups_16_measured" and nin[0] == "nin_s32_block_pass"
    with monkeypatch.context() as m:
        m.setattr(ops, "PREP_COMPACT_UPS", False)
        assert _plan(ops, layers, *ups[1:4]) == layers.Conv3Plan(*ups[4])._replace(compact=False)
    with monkeypatch.context() as m:
        m.setattr(ops, "WINO_EQ", False)       # a measured vector counts only with its equaliser
        assert _plan(ops, layers, *ups[1:4]).fmt is False
    with monkeypatch.context() as m:
        m.setattr(ops, "WINO_PREP_V2", False)  # block pass and compact operand are forms of the two-phase pass
        assert _plan(ops, layers, *nin[1:4]) == layers.Conv3Plan(*nin[4])._replace(shortcut_in_pass=False)
        assert not _plan(ops, layers, *ups[1:4]).compact
    with monkeypatch.context() as m:
        m.setattr(ops, "WINO_MIN_WGS", 129)
        assert _plan(ops, layers, *CASES[0][1:4]).path == "direct"
    with monkeypatch.context() as m:
        m.setattr(ops, "FUSE_GN_STATS", False)
        assert not any(_plan(ops, layers, *c[1:4]).stats for c in CASES)


def test_operand_fields_are_fixed(env):
    ops, _ = env
    op = ops.F32Operand([(None, 8)], silu=1)
    assert (op.ac, op.silu, op.drop, op.keep, op.wino_only, op.nin, op.t_kept, op.shortcut) == (None, True, None, False, False, None, None, None)
    with pytest.raises(AttributeError):
        op.res_out
    with pytest.raises(AttributeError):
        op.kep = True
    with pytest.raises(TypeError):
        ops.F32Operand([(None, 8)], slu=True)
    # a dict of the input fields (callers older than the class) is turned into an operand; a key it does not have raises there too
    old_style = ops.F32Operand.of(dict(parts=[(None, 8)], ac=None, silu=True))
    assert isinstance(old_style, ops.F32Operand) and old_style.silu and old_style.shortcut is None
    assert ops.F32Operand.of(None) is None and ops.F32Operand.of(op) is op
    with pytest.raises(TypeError):
        ops.F32Operand.of(dict(parts=[(None, 8)], slu=True))
