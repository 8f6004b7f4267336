"""Inputs of the f16f6 operand bit tests (tests/test_gpu_operand_bits.py) and of the script that recorded their golden words
(tools/gen_operand_bits_golden.py): everything here is numpy with a legacy RandomState, so the inputs are the same wherever they
are made.

Shapes (B = 2, so the per-sample (a, c) switch of the block pass is crossed):
  block pass  parts (128, 128), (64, 64), (128, 0) on grids 2 x 4 x 64 (a wave's 32-position segment ends inside a row) and
              2 x 8 x 32 (it ends at the row end) -- the cases of tests/test_gpu_block_pass.py;
  plain pass  16 + 16 channels on 2 x 4 x 64 and 4 x 8 x 8.
Two variants per shape:
  "act"  seeded normals through GroupNorm affine + SiLU + a power-of-two equaliser, with NaN, +-inf and 1e30 planted at segment ends,
         tile ends and mid-segment;
  "raw"  no affine, no SiLU, no equaliser: what is planted reaches the Winograd transform as it is.  The tensor is cut into regions of
         128 consecutive positions (whole rows; one wave of either pass lies inside one region of one 16-channel K block) of four
         kinds, kind = (2 kb + region) % 4 for K block kb:
           0 calm   normals, and every special that does not by itself ask for the fp16 saturation (NaN among them: the clamp passes
                    it): the region has no inf and nothing at or above 65520 -- every wave of it takes the split's plain path;
           1 hot    normals, channel 15 of the block at 1e7 x normal (all but a few 16-channel blocks reach 65520: every wave saturates),
                    and ALL specials;
           2 zero   all-zero blocks, with -0 and fp32 denormals planted (the block exponent's lower clamp);
           3 edge   isolated values 7.5 2^k, 7.75 2^k and the float under 8 2^k (the e2m3 block-scale edges), everything else zero:
                    the value IS the block's maximum.
         A planted special has zeros at the two positions on either side in its channel, so some frequency of the transform holds it
         exactly (d1 + d2 with d2 = 0) and its neighbours hold it negated."""
import zlib

import numpy as np

B = 2
BLOCK_CASES = [(cs, dims) for cs in ((128, 128), (64, 64), (128, 0)) for dims in ((2, 4, 64), (2, 8, 32))]
PLAIN_CASES = [((16, 16), (2, 4, 64)), ((16, 16), (4, 8, 8))]
VARIANTS = ("act", "raw")
REGION = 128

_F = np.float32
NAN, INF = _F("nan"), _F("inf")
JUST_UNDER_65520 = _F(65519.996)                     # rounds to fp16 65504 by itself
DENORM = _F(1e-40)
# specials that do not trigger the saturation by themselves (they can stand in a calm region) / those that do
CALM_SPECIALS = [_F(65504.0), _F(-65504.0), JUST_UNDER_65520, -JUST_UNDER_65520, _F(0.0), _F(-0.0), DENORM, -DENORM, _F(1.4e-45),
                 _F(7.5), _F(7.75), np.nextafter(_F(8.0), _F(0.0)), _F(7.5 * 2.0 ** 12), _F(7.75 * 2.0 ** -9),
                 np.nextafter(_F(8.0 * 2.0 ** 5), _F(0.0)), NAN]
HOT_SPECIALS = [INF, -INF, _F(65520.0), _F(-65520.0), _F(1e30), _F(-1e30)]
EDGE_K = (-6, -1, 0, 3, 10)
_SPOTS = (0, 13, 31, 32, 50, 63, 64 + 0, 64 + 13, 64 + 31, 64 + 32, 64 + 50, 64 + 63)      # in a region: region / segment ends, mid-segment


def case_id(cs, dims, variant):
    return f"{cs[0]}+{cs[1]}@{dims[0]}x{dims[1]}x{dims[2]}/{variant}"


def region_kind(kb, pos):
    return (2 * kb + pos // REGION) % 4


def _plant(x, b, kb, base, specials):
    """x: [B][C][P]; special i of the list at spot i of the region starting at `base`, channel i % 15 of K block kb (never channel 15)."""
    for i, v in enumerate(specials):
        pos, ch = base + _SPOTS[i % len(_SPOTS)], 16 * kb + (i + i // len(_SPOTS)) % 15
        x[b, ch, max(pos - 2, base):min(pos + 3, base + REGION)] = 0.0
        x[b, ch, pos] = v


def raw_tensor(cin, dims, seed):
    """[B][cin][P] float32 of the "raw" variant."""
    D, H, W = dims
    P = D * H * W
    assert P % REGION == 0 and REGION % W == 0
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((B, cin, P)) * 1.5).astype(_F)
    for b in range(B):
        for kb in range(cin // 16):
            for r in range(P // REGION):
                base, kind = r * REGION, region_kind(kb, r * REGION)
                blk = x[b, 16 * kb:16 * kb + 16, base:base + REGION]
                if kind == 0:
                    _plant(x, b, kb, base, CALM_SPECIALS)
                elif kind == 1:
                    blk[15] = (rs.standard_normal(REGION) * 1e7).astype(_F)
                    _plant(x, b, kb, base, CALM_SPECIALS + HOT_SPECIALS)
                elif kind == 2:
                    blk[:] = 0.0
                    _plant(x, b, kb, base, [_F(-0.0), DENORM, -DENORM, _F(1.4e-45)])
                else:
                    blk[:] = 0.0
                    edges = [s * v for k in EDGE_K for v in (_F(7.5 * 2.0 ** k), _F(7.75 * 2.0 ** k), np.nextafter(_F(8.0 * 2.0 ** k), _F(0.0)))
                             for s in (_F(1.0), _F(-1.0))]
                    for i, v in enumerate(edges):      # 30 values, 4 positions apart
                        blk[(i + b + kb) % 16, 4 * i + 1] = v
    return x


def act_tensor(cin, dims, seed):
    D, H, W = dims
    P = D * H * W
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((B, cin, P)) * 1.5).astype(_F)
    # row end / row start, the end and the start of a wave's segment, mid-segment, tile end / start, the last position
    for pos, ch, v in ((31, 3, NAN), (32, 12, INF), (W - 1, 0, INF), (W, 9, -INF), (45, 7, _F(1e30)), (13, 14, -INF), (255, 21, -INF), (256, 17, NAN),
                       (P - 1, 5, NAN), (P - 2, 30, _F(-1e30))):
        for b in range(B):
            x[b, (ch + 16 * b) % cin, pos % P] = v
    return x


def to_f32b(x):
    """[B][C][P] -> F32B [B][C/8][P][8]."""
    b, c, p = x.shape
    return np.ascontiguousarray(x.reshape(b, c // 8, 8, p).transpose(0, 1, 3, 2))


def inputs(cs, dims, variant):
    """dict: parts (list of (F32B array, channels)), ac [B][C][2] or None, eq [C] or None, silu, nin_w [C][128], nin_bias [128]."""
    cin = sum(cs)
    seed = 7000 + 13 * cin + dims[2] + (1 if cs[1] else 0) + (100 if variant == "raw" else 0)
    x = raw_tensor(cin, dims, seed) if variant == "raw" else act_tensor(cin, dims, seed)
    rs = np.random.RandomState(seed + 1)
    ac = eq = None
    if variant == "act":
        ac = np.stack([0.5 + rs.rand(B, cin), rs.standard_normal((B, cin)) * 0.3], axis=2).astype(_F)
        eq = np.exp2(rs.randint(-3, 4, cin)).astype(_F)
    nin_w = (rs.standard_normal((cin, 128)) * 0.1).astype(_F)
    nin_bias = rs.standard_normal(128).astype(_F)
    parts, c0 = [], 0
    for c in cs:
        if c:
            parts.append((to_f32b(x[:, c0:c0 + c]), c))
            c0 += c
    return {"x": x, "parts": parts, "ac": ac, "eq": eq, "silu": variant == "act", "nin_w": nin_w, "nin_bias": nin_bias}


# ---- weights (md_wino_pack_weights_f6: md_split_f16f6 with the remainder first and the scale bias -11) ----
WEIGHT_SHAPE = (128, 32)      # the smallest the packer takes


def weight_inputs(with_eq):
    co, ci = WEIGHT_SHAPE
    rs = np.random.RandomState(4242 + with_eq)
    w = (rs.standard_normal((co, ci, 3, 3, 3)) * 0.05).astype(_F)
    w[3, 0:16] = 0.0                                       # all-zero blocks
    w[5, 16:32, 1] = 0.0
    for i, v in enumerate(CALM_SPECIALS + HOT_SPECIALS):      # one special per output row, both K blocks over the rows
        w[8 + 2 * i, (5 * i) % ci, i % 3, (i // 3) % 3, i % 3] = v
    w[60, 16:32] *= _F(2e6)                                 # a block whose every frequency saturates
    for i, k in enumerate(EDGE_K):
        w[70 + i, 0:16] = 0.0
        w[70 + i, i, 1, 1, 0] = _F(7.75 * 2.0 ** k)          # g0 alone: frequency 0 holds it as it is
    eq = np.exp2(rs.randint(-3, 4, ci)).astype(_F) if with_eq else None
    return w, eq


# ---- digests: a tensor too large for the golden file is recorded as one CRC-32 per slab ----
def slab_crcs(words, n_slabs):
    """words: a contiguous integer array whose size divides into n_slabs equal runs -> uint32 [n_slabs]."""
    flat = np.ascontiguousarray(words).reshape(n_slabs, -1)
    return np.array([zlib.crc32(r.tobytes()) for r in flat], dtype=np.uint32)


# ---- the host's view of the "raw" variant: which 16-channel blocks hold which special, and which waves saturate ----
def raw_block_values(x, dims):
    """t [B][C][P/2][4]: the F(2,3) input transform along w of x [B][C][P] with zero padding per row (md_wino_bt)."""
    D, H, W = dims
    b, c, p = x.shape
    rows = x.reshape(b, c, p // W, W)
    pad = np.zeros((b, c, p // W, W + 2), dtype=_F)
    pad[..., 1:-1] = rows
    d0, d1, d2, d3 = pad[..., 0:W:2], pad[..., 1:W + 1:2], pad[..., 2:W + 2:2], pad[..., 3:W + 3:2]
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], axis=-1)
    return t.reshape(b, c, p // 2, 4)


def raw_coverage(x, dims):
    """For every special: does it stand (bit for bit, or negated) in a block of a region where every wave takes the plain path, and in
    a block that itself asks for the saturation?  -> {name: (in_plain, in_saturating)}; also whether an all-zero block exists."""
    t = raw_block_values(x, dims)
    b, c, ph, _ = t.shape
    tb = t.reshape(b, c // 16, 16, ph, 4)
    with np.errstate(invalid="ignore"):
        a = np.abs(tb)
        trig_blk = (np.nan_to_num(a, nan=0.0, posinf=np.inf) >= 65520.0).any(axis=2)                     # [b][kb][ph][4]
    reg = trig_blk.reshape(b, c // 16, ph // (REGION // 2), REGION // 2, 4)
    calm_reg = ~reg.any(axis=(3, 4), keepdims=True) & np.ones_like(reg)
    calm_blk = calm_reg.reshape(trig_blk.shape)
    bits = tb.view(np.uint32)
    out = {}
    for v in CALM_SPECIALS + HOT_SPECIALS:
        if np.isnan(v):
            hit = np.isnan(tb).any(axis=2)
            name = "nan"
        else:
            w = np.array(v, dtype=_F).view(np.uint32)
            hit = ((bits == w) | (bits == (w ^ np.uint32(0x80000000)))).any(axis=2)
            name = repr(float(v))
        prev = out.get(name, (False, False))
        out[name] = (prev[0] or bool((hit & calm_blk).any()), prev[1] or bool((hit & trig_blk).any()))
    zero_block = bool((bits == 0).all(axis=2).any())
    return out, zero_block


# ---- running a case on the GPU (hip_ops is handed in: the test and the recording script share this) ----
def _device_inputs(ops, cs, dims, variant):
    import torch
    d = inputs(cs, dims, variant)
    parts = [(torch.from_numpy(x).cuda(), c) for x, c in d["parts"]]
    ac = torch.from_numpy(d["ac"]).cuda() if d["ac"] is not None else None
    eq = torch.from_numpy(d["eq"]).cuda() if d["eq"] is not None else None
    return d, parts, ac, eq


def run_plain(ops, cs, dims, variant):
    """md_wino_prep_f6 -> T as int16 (numpy)."""
    import torch
    d, parts, ac, eq = _device_inputs(ops, cs, dims, variant)
    t = ops.wino_prep(parts, ac, d["silu"], 0, B, None, f8="f6", eq=eq, dims=dims).view(torch.int16).clone()
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run_block(ops, cs, dims, variant, with_nin, n_cu):
    """md_wino_prep_f6_nin -> (T as int16, res as int32 or None)."""
    import torch
    d, parts, ac, eq = _device_inputs(ops, cs, dims, variant)
    pw = ops.PackedWeight(torch.from_numpy(d["nin_w"]).cuda(), "nin", ops.CFG_G1_128, "cuda") if with_nin else None
    bias = torch.from_numpy(d["nin_bias"]).cuda() if with_nin else None
    t, res = ops.wino_prep_nin(parts, ac, d["silu"], B, None, eq, pw, bias, dims=dims, n_cu=n_cu)
    t = t.view(torch.int16).clone()
    res = res.view(torch.int32).clone() if res is not None else None
    torch.cuda.synchronize()
    return t.cpu().numpy(), (res.cpu().numpy() if res is not None else None)


def run_weights(ops, with_eq):
    """md_wino_pack_weights_f6 -> the packed image as int32."""
    import torch
    w, eq = weight_inputs(with_eq)
    ww = ops.WinoWeightF8(torch.from_numpy(w), "cuda", fmt="f6", eq=torch.from_numpy(eq).cuda() if eq is not None else None)
    torch.cuda.synchronize()
    return ww.data.view(torch.int32).cpu().numpy()


def t_slabs(cs):
    return B * (sum(cs) // 8)          # one slab per (sample, channel group of 8): [f][plane][P/2] items of 16 bytes


RES_SLABS = B * 16                     # one slab per (sample, 8 output rows)
WPK_SLABS = 144                        # fragments of 128 x 32: 147456 words; the 64-word header is recorded whole
