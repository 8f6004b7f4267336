"""md_wino_prep_f6_nin (csrc/block_pass.hip): one pass over a shortcut block's input writes Conv_0's f16f6 operand T and the NIN
shortcut `res`.  Both are held to the BITS of the two kernels it replaces -- hip_ops.wino_prep(..., f8="f6", eq=eq) and
hip_ops.nin_f32(...) on the same inputs -- T compared as int16, res as int32.

Grids: 2 x 4 x 64 (a wave's 32-position segment is half a row: the interior neighbour comes from the halo load) and 2 x 8 x 32 (a
segment is a whole row: both ends are padding).  B = 2, P = 512: 4 tiles; with n_cu = 3 workgroups the tile loop is ragged and
the prefetch of a workgroup's next tile crosses the sample boundary.  The reference is computed once per (parts, grid)."""
import ctypes

import pytest
import torch

PARTS = [(128, 128), (256, 0), (128, 0), (64, 64)]
GRIDS = [(2, 4, 64), (2, 8, 32)]
B = 2
_REF = {}


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


def _inputs(ops, cs, dims, special=False, plain=False):
    """parts (F32B [B][c/8][P][8]), ac [B][C][2], eq [C] (powers of two), packed NIN weights, bias."""
    D, H, W = dims
    P, cin = D * H * W, sum(cs)
    g = torch.Generator().manual_seed(1000 * cin + 10 * W + len([c for c in cs if c]) + (5 if special else 0))
    xs = [torch.randn((B, c // 8, P, 8), generator=g) * 1.5 for c in cs if c]
    if special:
        # row end / row start (x = 63 | 31, x = 0), the end and the start of a wave's segment (positions 31, 32), tile end / start (255, 256)
        nan, inf = float("nan"), float("inf")
        for pos, ch, v in ((31, 3, nan), (32, 12, inf), (W - 1, 0, inf), (W, 9, -inf), (255, 21, -inf), (256, 17, nan), (P - 1, 5, nan)):
            for b, x in enumerate(xs):
                x[b, ch // 8, pos, ch % 8] = v
    a = 0.5 + torch.rand((B, cin), generator=g)
    c = torch.randn((B, cin), generator=g) * 0.3
    ac = torch.stack([a, c], dim=2).contiguous()
    eq = torch.exp2(torch.randint(-3, 4, (cin,), generator=g).float())
    Wn, bias = torch.randn((cin, 128), generator=g) * 0.1, torch.randn((128,), generator=g)
    parts = [(x.cuda(), c) for x, c in zip(xs, [c for c in cs if c])]
    pw = ops.PackedWeight(Wn.cuda(), "nin", ops.CFG_G1_128, "cuda")
    if plain:
        return parts, None, None, pw, bias.cuda()
    return parts, ac.cuda(), eq.cuda(), pw, bias.cuda()


def _reference(ops, key, cs, dims, **kw):
    if key not in _REF:
        parts, ac, eq, pw, bias = _inputs(ops, cs, dims, **kw)
        D, H, W = dims
        t = ops.wino_prep(parts, ac, ac is not None, 0, B, None, f8="f6", eq=eq, dims=dims).view(torch.int16).clone()
        res = ops.nin_f32(parts, pw, bias, B, D * H * W).view(torch.int32).clone()
        torch.cuda.synchronize()
        _REF[key] = (parts, ac, eq, pw, bias, t, res)
    return _REF[key]


def _compare(ops, ref, dims, n_cu, what, with_nin=True):
    parts, ac, eq, pw, bias, t_ref, res_ref = ref
    t, res = ops.wino_prep_nin(parts, ac, ac is not None, B, None, eq, pw if with_nin else None, bias if with_nin else None, dims=dims, n_cu=n_cu)
    assert t._md_fmt == "f6" and t._md_compact is False and t._md_eq == (eq.data_ptr() if eq is not None else 0)
    t = t.view(torch.int16)
    assert t.shape == t_ref.shape
    bad = (t != t_ref).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {t.numel()} int16 words of T differ, first at {bad[0].item()}"
    if with_nin:
        res = res.view(torch.int32)
        assert res.shape == res_ref.shape
        bad = (res != res_ref).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {res.numel()} words of res differ, first at {bad[0].tolist()}"
    else:
        assert res is None


@pytest.mark.gpu
@pytest.mark.parametrize("n_cu", [0, 3])
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("cs", PARTS, ids=lambda c: f"{c[0]}+{c[1]}")
def test_operand_and_shortcut_equal_the_two_kernels_bit_for_bit(ops, cs, dims, n_cu):
    """GroupNorm affine + SiLU + a power-of-two equaliser, one and two parts, K = 128 and 256."""
    ref = _reference(ops, (cs, dims), cs, dims)
    _compare(ops, ref, dims, n_cu, f"parts {cs} grid {dims} n_cu {n_cu}")


@pytest.mark.gpu
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_nan_and_inf_at_row_segment_and_tile_ends(ops, dims):
    """NaN, +inf and -inf at a row end, at the ends of a wave's segment and at a tile end: they reach exactly the pairs they reach in
    the two-phase pass (the padding is a select, not a product), with the same bits."""
    cs = (128, 128)
    ref = _reference(ops, (cs, dims, "special"), cs, dims, special=True)
    assert not bool(torch.isfinite(ref[6].view(torch.float32)).all())          # the special values did reach the shortcut
    for n_cu in (0, 3):
        _compare(ops, ref, dims, n_cu, f"non-finite inputs, grid {dims} n_cu {n_cu}")


@pytest.mark.gpu
@pytest.mark.parametrize("cs", [(128, 128), (128, 0)], ids=lambda c: f"{c[0]}+{c[1]}")
def test_raw_operand_and_operand_only_mode(ops, cs):
    """No affine, no SiLU, no equaliser (the null branches); and wpk == NULL: the operand alone, no shortcut."""
    dims = GRIDS[0]
    ref = _reference(ops, (cs, dims, "plain"), cs, dims, plain=True)
    _compare(ops, ref, dims, 3, f"raw operand, parts {cs}")
    ref = _reference(ops, (cs, dims), cs, dims)
    _compare(ops, ref, dims, 0, f"operand only, parts {cs}", with_nin=False)
    _compare(ops, ref, dims, 3, f"operand only, parts {cs}, n_cu 3", with_nin=False)


def test_entry_point_answers_the_parents_error_codes(hip_lib):
    """Checked before any launch (no GPU needed): md_wino_prep_f6's argument errors, md_nin_f32's, and the shapes neither takes."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = hip_lib.md_wino_prep_f6_nin
    #        x1 x2    c1   c2  ac    silu eq    T  wpk bias res B  D  H  W  n_cu stream
    assert f(None, None, 128, 0, None, 0, None, p, p, p, p, 1, 4, 8, 8, 0, None) == -1          # no input
    assert f(p, None, 128, 0, None, 0, None, None, p, p, p, 1, 4, 8, 8, 0, None) == -1          # no operand buffer
    assert f(p, None, 128, 0, None, 1, None, p, p, p, p, 1, 4, 8, 8, 0, None) == -1             # SiLU without the folded affine
    assert f(p, None, 120, 0, None, 0, None, p, p, p, p, 1, 4, 8, 8, 0, None) == -1             # 120 channels: not whole K blocks
    assert f(p, p, 120, 8, None, 0, None, p, p, p, p, 1, 4, 8, 8, 0, None) == -1                # second part of 8 channels
    assert f(p, None, 64, 64, None, 0, None, p, p, p, p, 1, 4, 8, 8, 0, None) == -1             # second part without its tensor
    assert f(p, None, 128, 0, None, 0, None, p, p, p, p, 1, 4, 8, 7, 0, None) == -1             # odd W
    assert f(p, None, 128, 0, None, 0, None, p, p, p, p, 0, 4, 8, 8, 0, None) == -1             # empty batch
    assert f(p, None, 128, 0, None, 0, None, p, p, None, p, 1, 4, 8, 8, 0, None) == -1          # weights without bias
    assert f(p, None, 128, 0, None, 0, None, p, p, p, None, 1, 4, 8, 8, 0, None) == -1          # weights without res
    assert f(p, None, 128, 0, None, 0, None, p, p, p, p, 1, 4, 8, 24, 0, None) == -2            # W does not divide 256
    assert f(p, None, 128, 0, None, 0, None, p, p, p, p, 1, 3, 5, 8, 0, None) == -2             # D H W not a multiple of 256
    assert f(p, None, 64, 0, None, 0, None, p, p, p, p, 1, 4, 8, 8, 0, None) == -2              # K = 64
    assert f(p, p, 256, 128, None, 0, None, p, p, p, p, 1, 4, 8, 8, 0, None) == -2              # K = 384
    assert f(p, None, 64, 0, None, 0, None, p, None, None, None, 1, 4, 8, 8, 0, None) == -2     # operand only: the same K
