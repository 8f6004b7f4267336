"""The weight-gradient kernels bit for bit: every case of tests/wgrad_cases.py (small hashed integers, sparse even dY, one live lo
plane at most; tests/test_cpu_wgrad_cases.py proves that the kernels' arithmetic is exact on them) through the operand passes and
the entry point it names -- md_to_pb16 + md_wgrad (taps 27 / 125 / 1), md_wino_prep(_v2) + md_wino_prep_dual + md_wgrad_wino,
md_wgrad_nin -- and torch.equal with the float64 gradient at EVERY element of dW, no channel sub-sampling.

Every case accumulates onto a non-zero integer dW0 inside a sentinel-filled buffer (margins in front and behind, gaps between the
rows where the strides leave some): the whole buffer is compared, so a write outside the addressed elements fails as well.  Every
K split of a case must equal its first one bit for bit, and the first launch is repeated.  A failure prints how many elements
differ, their (co, ci, tap) ranges and the first few values.

One randn case per kernel stays at the project's TOL_MFMA, per tap and per 128 x 128 tile against float64."""
import pytest
import torch

import wgrad_cases as wc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL_MFMA = 3e-5            # the bf16x3 budget of tests/test_gpu_wino.py / test_gpu_kernels.py


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def bw(ops):
    from meshdiffusion_amd.lib.diffusion.models import backward
    return backward


def _ids(entry, taps=None):
    return [s["id"] for s in wc.SPECS if s["entry"] == entry and (taps is None or s["taps"] == taps)]


def _check(case, got, ref, what):
    """got: the whole buffer after the launch (CPU); ref: float64 [co, ci, taps] = dW0 + gradient."""
    if torch.equal(got, wc.dw_buffer(case, ref)):
        return
    idx = wc.dw_index(case) + wc.MARGIN
    msg = wc.describe_mismatch(got[idx.reshape(-1)].reshape(idx.shape), ref.float(), what + " (co, ci, tap)")
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[idx.reshape(-1)] = False
    stray = (mask & (got != wc.SENTINEL)).nonzero().reshape(-1)
    if stray.numel():
        msg += f"; {stray.numel()} floats OUTSIDE the addressed elements changed, first at offset {int(stray[0]) - wc.MARGIN} from dW"
    raise AssertionError(msg)


def _drive(spec, prepare):
    """prepare(case) -> launch(dw view on the device, ksplit).  The checks every entry point gets."""
    case = wc.build(spec)
    ref = wc.reference(case)
    launch = prepare(case)
    first = None
    for ks in spec["ksplit"]:
        buf = wc.dw_buffer(case, case["dw0"]).cuda()
        launch(buf[wc.MARGIN:], ks)
        got = buf.cpu()
        _check(case, got, ref, f"{spec['id']} ksplit={ks}")
        if first is None:
            first = got
            buf = wc.dw_buffer(case, case["dw0"]).cuda()
            launch(buf[wc.MARGIN:], ks)
            assert torch.equal(buf.cpu(), first), f"{spec['id']}: the same launch twice differs"
        assert torch.equal(got, first), f"{spec['id']}: ksplit={ks} differs from ksplit={spec['ksplit'][0]}"


# ---------------------------------------------------------------------------------------------------------------
# md_to_pb16 + md_wgrad
# ---------------------------------------------------------------------------------------------------------------
def _pb_operands(ops, bw, case):
    """(dy_pb, act_pb, dims): dY as F32B (what the backward holds), A as S16B or F32B by turns; cubes go through the wrappers exactly
    as the training path calls them (dims=None)."""
    spec, B, (D, H, W) = case["spec"], case["B"], case["dims"]
    pad = 2 if case["taps"] == 125 else 1
    dims = None if D == H == W else (D, H, W)
    assert bw.zsplit_for(B, D) == wc.zsplit_for(B, D)
    dy_pb = bw.to_pb16(ops.ncdhw_to_f32b(case["dy"].cuda()), B, case["a_ch"], H, 0, stuff=spec.get("stuff", 0), pad=pad, zhalo=False, dims=dims)
    if spec["seed"] % 2:
        act_pb = bw.to_pb16(ops.ncdhw_to_f32b(case["a"].cuda()), B, case["b_ch"], H, 0, up=spec.get("up", 0), pad=pad, dims=dims)
    else:
        act_pb = bw.to_pb16(ops.ncdhw_to_s16b(case["a"].cuda(), case["b_ch"]), B, case["b_ch"], H, 1, up=spec.get("up", 0), pad=pad, dims=dims)
    return dy_pb, act_pb, dims


def _prepare_pb(ops, bw):
    def prepare(case):
        dy_pb, act_pb, dims = _pb_operands(ops, bw, case)

        def launch(dw, ks):
            bw.wgrad(dy_pb, act_pb, case["B"], case["co"], case["ci"], case["dims"][1], case["taps"], dw, *case["strides"],
                     a_ch=case["a_ch"], b_ch=case["b_ch"], dims=dims, ksplit=ks)
        return launch
    return prepare


@pytest.mark.parametrize("case_id", _ids("pb", 27))
def test_wgrad_27_exact(ops, bw, case_id):
    _drive(wc.spec_of(case_id), _prepare_pb(ops, bw))


@pytest.mark.parametrize("case_id", _ids("pb", 125))
def test_wgrad_125_exact(ops, bw, case_id):
    _drive(wc.spec_of(case_id), _prepare_pb(ops, bw))


@pytest.mark.parametrize("case_id", _ids("pb", 1))
def test_wgrad_1_exact(ops, bw, case_id):
    _drive(wc.spec_of(case_id), _prepare_pb(ops, bw))


# ---------------------------------------------------------------------------------------------------------------
# md_wino_prep / _v2 + md_wino_prep_dual + md_wgrad_wino
# ---------------------------------------------------------------------------------------------------------------
def _planes(ts):
    return [wc.split_bf16(t) for t in ts]


def _wino_T_direct(ops, fn, x_f, c, B, dims):
    """md_wino_prep or md_wino_prep_v2 called by name: T in a tensor of its own."""
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.hip_ops import _ptr, _stream
    lib = _lib.load()
    nbytes = lib.md_wino_operand_bytes(B, c, *dims)
    assert nbytes > 0
    t = torch.empty(nbytes // 2, dtype=torch.bfloat16, device="cuda")
    assert getattr(lib, fn)(_ptr(x_f), None, c, 0, None, 0, 0, _ptr(t), B, *dims, 0.0, 0, _stream()) == 0
    return t


def _prepare_wino(ops, verify=True):
    """verify=False (tests/test_gpu_nonfinite_kernels.py: a NaN operand, whose payload and sign bits the host does not restate)
    leaves out the bit-for-bit comparison of T and U with the host's planes."""
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.hip_ops import _ptr, _stream
    lib = _lib.load()

    def prepare(case):
        spec, B, co, ci, dims = case["spec"], case["B"], case["co"], case["ci"], case["dims"]
        a_f, dy_f = ops.ncdhw_to_f32b(case["a"].cuda()), ops.ncdhw_to_f32b(case["dy"].cuda())
        if spec.get("prep") == "v1":
            t_act = _wino_T_direct(ops, "md_wino_prep", a_f, ci, B, dims)
        else:
            t_act = ops.wino_prep([(a_f, ci)], None, False, False, B, 0, keep=True, dims=dims)
        _, u_dy = ops.wino_prep([(dy_f, co)], None, False, False, B, 0, dual=True, dims=dims)
        # the operands in the kernel's own domain, bit for bit: a mismatch below is then md_wgrad_wino's
        shape = (B, -1, 4, 2, dims[0], dims[1], dims[2] // 2, 8)
        if verify:
            assert torch.equal(t_act.view(torch.int16).cpu().view(shape), wc.t_layout(_planes(wc.wino_T(case["a"])), B, ci)), f"{spec['id']}: T"
            assert torch.equal(u_dy.view(torch.int16).cpu().view(shape), wc.t_layout(_planes(wc.wino_U(case["dy"])), B, co)), f"{spec['id']}: U"

        def launch(dw, ks):
            if case["strides"] == (ci * 27, 27, 1):
                ops.wgrad_wino(u_dy, t_act, B, co, ci, 0, dw, dims=dims, ksplit=ks)
                return
            ks = min(256 // ((co // 128) * (ci // 128) * 12), B * (dims[0] - 1)) if ks is None else ks
            nbytes = lib.md_wgrad_wino_workspace_bytes(co, ci, ks)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
            assert lib.md_wgrad_wino(_ptr(u_dy), _ptr(t_act), _ptr(dw), _ptr(ws), nbytes, B, co, ci, *dims, ks, *case["strides"], _stream()) == 0
        return launch
    return prepare


@pytest.mark.parametrize("case_id", _ids("wino"))
def test_wgrad_wino_exact(ops, case_id):
    _drive(wc.spec_of(case_id), _prepare_wino(ops))


@pytest.mark.parametrize("B,c,dims", wc.DUAL_CASES)
def test_wino_prep_dual_exact(ops, B, c, dims):
    """md_wino_prep_dual alone on non-cubic grids at W = 8, 16, 32, 64: T identical to md_wino_prep_v2's and to the host's, U bit for
    bit, and the channel sums EXACTLY (integers: every partial sum is exact), accumulated onto a non-zero start."""
    x = wc.dual_input(B, c, dims)
    x_f = ops.ncdhw_to_f32b(x.cuda())
    t_ref = _wino_T_direct(ops, "md_wino_prep_v2", x_f, c, B, dims)
    sums = torch.full((B, c), 7.0, device="cuda")
    t, u = ops.wino_prep([(x_f, c)], None, False, False, B, 0, dual=True, sums=sums, dims=dims)
    assert torch.equal(t.view(torch.int16), t_ref.view(torch.int16))
    shape = (B, c // 8, 4, 2, dims[0], dims[1], dims[2] // 2, 8)
    assert torch.equal(t.view(torch.int16).cpu().view(shape), wc.t_layout(_planes(wc.wino_T(x)), B, c))
    msg = wc.describe_mismatch(u.view(torch.int16).cpu().view(shape), wc.t_layout(_planes(wc.wino_U(x)), B, c), "U [b][c/8][f][plane][z][y][pair][8]")
    assert not msg, msg
    msg = wc.describe_mismatch(sums.cpu().double(), 7.0 + x.double().sum(dim=(2, 3, 4)), "channel sums")
    assert not msg, msg


# ---------------------------------------------------------------------------------------------------------------
# md_wgrad_nin
# ---------------------------------------------------------------------------------------------------------------
def _prepare_nin(ops):
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.hip_ops import _ptr, _stream
    lib = _lib.load()

    def prepare(case):
        B, co, ci, P = case["B"], case["co"], case["ci"], case["dims"][2]
        xs, dys = ops.ncdhw_to_s16b(case["a"].cuda(), ci), ops.ncdhw_to_s16b(case["dy"].cuda(), co)

        def launch(dw, ks):
            if case["strides"] == (1, co, 0):
                ops.wgrad_nin(dys, xs, B, co, ci, P, dw, ksplit=ks)
                return
            ks = max(1, min(256 // ((co // 128) * (ci // 128)), B * P // 16 // 8)) if ks is None else ks
            nbytes = lib.md_wgrad_nin_workspace_bytes(co, ci, ks)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
            assert lib.md_wgrad_nin(_ptr(dys), _ptr(xs), _ptr(dw), _ptr(ws), nbytes, B, co, ci, P, ks, *case["strides"][:2], _stream()) == 0
        return launch
    return prepare


@pytest.mark.parametrize("case_id", _ids("nin"))
def test_wgrad_nin_exact(ops, case_id):
    _drive(wc.spec_of(case_id), _prepare_nin(ops))


# ---------------------------------------------------------------------------------------------------------------
# ordinary operands
# ---------------------------------------------------------------------------------------------------------------
def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tile_errors(got, ref, what):
    """rel-L2 per tap and per 128 x 128 tile of [co, ci, taps] against float64; prints the largest and returns it."""
    worst = (0.0, None)
    for r0 in range(0, ref.shape[0], 128):
        for c0 in range(0, ref.shape[1], 128):
            for t in range(ref.shape[2]):
                e = rel_l2(got[r0:r0 + 128, c0:c0 + 128, t], ref[r0:r0 + 128, c0:c0 + 128, t])
                worst = max(worst, (e, (r0, c0, t)))
    print(f"{what}: largest rel-L2 of a (128 x 128 tile, tap) against float64 {worst[0]:.2e} at (co0, ci0, tap) {worst[1]}; whole tensor {rel_l2(got, ref):.2e}")
    return worst[0]


@pytest.mark.parametrize("kernel", ["md_wgrad", "md_wgrad_wino", "md_wgrad_nin"])
def test_wgrad_randn_within_the_bf16x3_budget(ops, bw, kernel):
    """Ordinary (randn) operands: every tap of every 128 x 128 tile within TOL_MFMA of the float64 gradient."""
    B, co, ci, dims = {"md_wgrad": (8, 256, 128, (8, 8, 8)), "md_wgrad_wino": (2, 128, 256, (8, 16, 32)), "md_wgrad_nin": (3, 256, 128, (1, 1, 4096))}[kernel]
    a, dy = _randn((B, ci) + dims, 70), _randn((B, co) + dims, 71, 0.1)
    k = 1 if kernel == "md_wgrad_nin" else 3
    ref = wc.contract(wc._rows(dy.double()), wc.shifted(a.double(), k, k, k))
    if kernel == "md_wgrad":
        dw = torch.zeros((co, ci, 27), device="cuda")
        dy_pb = bw.to_pb16(ops.ncdhw_to_f32b(dy.cuda()), B, co, 8, 0, zhalo=False)
        act_pb = bw.to_pb16(ops.ncdhw_to_s16b(a.cuda(), ci), B, ci, 8, 1)
        bw.wgrad(dy_pb, act_pb, B, co, ci, 8, 27, dw, ci * 27, 27, 1)
        got = dw.cpu()
    elif kernel == "md_wgrad_wino":
        dw = torch.zeros((co, ci, 27), device="cuda")
        t_act = ops.wino_prep([(ops.ncdhw_to_f32b(a.cuda()), ci)], None, False, False, B, 0, keep=True, dims=dims)
        _, u_dy = ops.wino_prep([(ops.ncdhw_to_f32b(dy.cuda()), co)], None, False, False, B, 0, dual=True, dims=dims)
        ops.wgrad_wino(u_dy, t_act, B, co, ci, 0, dw, dims=dims)
        got = dw.cpu()
    else:
        dw = torch.zeros((ci, co), device="cuda")
        ops.wgrad_nin(ops.ncdhw_to_s16b(dy.cuda(), co), ops.ncdhw_to_s16b(a.cuda(), ci), B, co, ci, dims[2], dw)
        got = dw.cpu().t().reshape(co, ci, 1)
    assert _tile_errors(got.double(), ref, kernel) < TOL_MFMA
