"""Inputs on which the convolution kernels' arithmetic is EXACT, their float64 references and the proof obligations
(tests/test_gpu_conv_exact.py launches them on the GPU and demands torch.equal with the float64 result at every voxel;
tests/test_cpu_conv_cases.py proves on the CPU that every case is in the regime it claims).  Plain helper module: no
fixtures, no GPU, only torch.

Why exact.  Every product in these kernels is a product of split operands (bf16 hi / lo planes, or fp16 planes in the
f16f8 / f16f6 / fp16x2 arithmetics) accumulated in fp32.  When every operand and weight is a small integer (times a power
of two), every product is exact and every partial sum is an integer below 2^24 in units of the common lsb: the result
does not depend on the summation order, on the Winograd transforms or on split-K, and it equals the float64 convolution
bit for bit.  One wrong index, tap, stride, halo entry, plane or missing term changes at least one bit.

Classes (`cls`).  The kernels compute hi*hi + hi*lo + lo*hi and drop lo*lo, so a class may keep only ONE lo plane live:
    hi_only   operand and (transformed) weights <= 8 significant bits: both lo planes zero -- indexing, taps, tiles, halos, epilogue
    x_lo      operand 9 .. 11 bits (lo plane live), weights <= 5 bits               -- a dropped / misplaced lo*hi term
    w_lo      operand <= 4 bits, weights 9 .. 11 bits (lo live after G as well)     -- a dropped / misplaced hi*lo term
    f16       operand and transformed weights <= 11 bits (exact in ONE fp16, more than a bf16 hi plane holds): the fp16
              MFMA of md_conv3_wino_f8 / _f6 is exact and both cross terms vanish; only fed to those kernels
Values are hashed (torch.randint over the whole tensor from a seeded generator, not separable in the coordinates), so no
mis-indexing maps a tensor onto itself.  Weights are even integers (the G transform's /2 stays an integer or a half) and
SPARSE: `nnz` non-zero taps per output row on average, which bounds sum |term| whatever Cin is while every input voxel
still meets hundreds of weights.  The Winograd domain doubles the operand (d0 - d2) and can grow a tap by 1.5, so its sums
are about four times the direct ones; `exactness_margin` measures what is left to 2^24 in each domain.
"""
import torch
import torch.nn.functional as F

from attn_cases import split_bf16

LIMIT = float(2 ** 24)        # integers (in lsb units) up to here are exact in fp32

# xmax: |operand| <= xmax; wmax: |weight| <= wmax (even); nnz: mean number of non-zero taps per output row
CLASSES = {
    "hi_only": dict(xmax=127, wmax=30, nnz=500),
    "x_lo": dict(xmax=1023, wmax=14, nnz=250),
    "w_lo": dict(xmax=7, wmax=1022, nnz=250),
    "f16": dict(xmax=1023, wmax=126, nnz=48),
    # the twin of a case that checks GroupNorm sums exactly: the kernels add the squares of up to a whole (sample, channel) grid in
    # fp32 before the float64 atomic, so sum o^2 over the grid has to stay below 2^24 as well (`stats_margin`)
    "tiny": dict(xmax=3, wmax=2, nnz=16, emax=3),
}
EXTRA_MAX = 999               # |bias|, |residual| <= this (`emax` of a class overrides it)


def split_fp16(x):
    x = x.float()
    hi = x.half().float()
    lo = (x - hi).half().float()
    return hi, lo


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ---------------------------------------------------------------------------------------------------------------
# builder
# ---------------------------------------------------------------------------------------------------------------
def build(spec):
    """spec: dict(id, cls, B, parts=[c, ..], cout, dims=(D, H, W) of the OUTPUT, kshape=(3, 3, 3), stride=1, ups=0,
    bias / res = None | "sample" | "shared", ac=False (hand-made GroupNorm affine: power-of-two gains, integer offsets),
    dgrad=False (data-gradient orientation), seed, optional xmax / wmax / nnz overrides).  Returns the case:
      x_raw  list of fp32 [B, c, Din, Hin, Win] (what the kernel is given), ac fp32 [B, cin, 2] or None,
      x      fp32 [B, cin, Din, Hin, Win]: the conv's logical input (x_raw * a + c; exact),
      w      fp32 as the packer takes it ([cout, cin, k..]; dgrad: [cin, cout, 3, 3, 3]), w_eff [cout, cin, k..] the conv's taps,
      bias   fp32 [B or 1, cout] or None, res fp32 [B or 1, cout, D, H, W] or None."""
    p = dict(CLASSES[spec["cls"]])
    p.update({k: spec[k] for k in ("xmax", "wmax", "nnz") if k in spec})
    B, parts, cout = spec["B"], list(spec["parts"]), spec["cout"]
    D, H, W = spec["dims"]
    kshape, stride, ups = tuple(spec.get("kshape", (3, 3, 3))), spec.get("stride", 1), spec.get("ups", 0)
    assert not (ups and stride == 2)
    cin = sum(parts)
    din = (D * 2, H * 2, W * 2) if stride == 2 else ((D // 2, H // 2, W // 2) if ups else (D, H, W))
    g = torch.Generator().manual_seed(1000 + spec.get("seed", 0))
    xmax = p["xmax"]
    if spec.get("ac"):
        q = max(1, xmax // 4)
        raw = _randint(g, -q, q, (B, cin) + din)
        gain = torch.tensor([1.0, 2.0, -1.0, -2.0])[torch.randint(0, 4, (B, cin), generator=g)]
        off = _randint(g, 1, q, (B, cin)) * (2 * torch.randint(0, 2, (B, cin), generator=g).float() - 1)     # never 0: act(0) != 0
        ac = torch.stack([gain, off], -1).contiguous()
        x = raw * gain[:, :, None, None, None] + off[:, :, None, None, None]
    else:
        raw, ac = _randint(g, -xmax, xmax, (B, cin) + din), None
        x = raw
    x_raw = [t.contiguous() for t in torch.split(raw, parts, dim=1)]
    taps = kshape[0] * kshape[1] * kshape[2]
    half = p["wmax"] // 2
    w_eff = 2.0 * _randint(g, -half, half, (cout, cin) + kshape)
    density = min(1.0, p["nnz"] / float(cin * taps))
    w_eff = w_eff * (torch.rand((cout, cin) + kshape, generator=g) < density).float()
    if spec.get("dgrad"):
        assert kshape == (3, 3, 3)
        w = w_eff.transpose(0, 1).flip(2, 3, 4).contiguous()        # W[co' = cin][ci' = cout][26 - t]: w_eff is its data-gradient conv
    else:
        w = w_eff.contiguous()
    bias = res = None
    emax = p.get("emax", EXTRA_MAX)
    if spec.get("bias"):
        bias = _randint(g, -emax, emax, (B if spec["bias"] == "sample" else 1, cout))
    if spec.get("res"):
        res = _randint(g, -emax, emax, (B if spec["res"] == "sample" else 1, cout, D, H, W))
    return dict(spec=spec, x_raw=x_raw, ac=ac, x=x.contiguous(), w=w, w_eff=w_eff, bias=bias, res=res, B=B, cin=cin, cout=cout,
                dims=(D, H, W), din=din, kshape=kshape, stride=stride, ups=ups, rows=spec.get("ref_rows"))


# ---------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------
def conv_input(case, dtype=torch.float64):
    """The tensor the taps slide over (activated, nearest x2 for `ups`); zero padding happens in `_conv`."""
    x = case["x"].to(dtype)
    return F.interpolate(x, scale_factor=2, mode="nearest") if case["ups"] else x


def _conv(x, w, case):
    kd, kh, kw = w.shape[2:]
    if case["stride"] == 2:
        return F.conv3d(F.pad(x, (0, 1, 0, 1, 0, 1)), w, stride=2)
    return F.conv3d(x, w, padding=(kd // 2, kh // 2, kw // 2))


def _rows(case, t, dim):
    return t if case["rows"] is None else t.index_select(dim, torch.tensor(case["rows"]))


def _extras(case, dtype, absolute=False):
    """bias + residual of the checked rows, broadcastable to [B, rows, D, H, W]."""
    e = torch.zeros((1, 1, 1, 1, 1), dtype=dtype)
    for t, tail in ((case["bias"], (1, 1, 1)), (case["res"], ())):
        if t is not None:
            t = _rows(case, t, 1).to(dtype)
            e = e + (t.abs() if absolute else t).reshape(t.shape + tail)
    return e


def reference(case):
    """float64 [B, rows, D, H, W] from the tensors themselves (rows: all, or case['rows'])."""
    w = _rows(case, case["w_eff"], 0).double()
    return _conv(conv_input(case), w, case) + _extras(case, torch.float64)


def reference_stats(ref):
    """GroupNorm sums of the reference, [B, rows, 2] float64 (integers far below 2^53: exact)."""
    return torch.stack([ref.sum(dim=(2, 3, 4)), (ref * ref).sum(dim=(2, 3, 4))], dim=-1)


def stats_margin(ref):
    """Largest sum of o^2 (>= sum |o| for integers) over a (sample, channel) grid: below 2^24 every fp32 partial sum a kernel may
    form on the way to its float64 atomic -- a tile's (the epilogues) or the whole grid's (the split-K finish) -- is exact."""
    return float((ref * ref).sum(dim=(2, 3, 4)).max())


STATS_TILE = 256      # positions whose values and squares an epilogue adds in fp32 before its float64 atomic: one 4 x 8 x 8 tile per channel
                      # (conv3_main.hip, conv3_s2.hip, conv3_stem.hip, conv3_wino.hip: per-lane sums, a DPP row reduction, four waves)


def stats_tolerance(ref, whole_grid=False):
    """[B, rows, 2]: what fp32 partial sums may lose on ordinary magnitudes -- n additions and one rounding of every square, each
    2^-24 relative: (n + 1) 2^-24 sum |term|, n = the largest fp32 partial sum the kernel forms: a tile (STATS_TILE; the tile sums
    are then added in float64), or with `whole_grid` the (sample, channel) grid (md_splitk_reduce_stats_kernel: one block per 8
    channels adds all positions in fp32)."""
    n = ref.shape[2] * ref.shape[3] * ref.shape[4] if whole_grid else STATS_TILE
    return (n + 1) * 2.0 ** -24 * torch.stack([ref.abs().sum(dim=(2, 3, 4)), (ref * ref).sum(dim=(2, 3, 4))], dim=-1)


def stats_twin(spec):
    """The same launch on `tiny` values, or None where the case has no exact statistics check."""
    if not spec.get("stats") or spec.get("stats_exact") is False:
        return None
    twin = {k: v for k, v in spec.items() if k not in ("xmax", "wmax", "nnz")}
    twin.update(cls="tiny", id=spec["id"] + "/tiny")
    return twin


# ---------------------------------------------------------------------------------------------------------------
# Winograd F(2, 3) along w, as md_wino_prep / md_wino_pack_weights / md_conv3_wino define it
# ---------------------------------------------------------------------------------------------------------------
def wino_T(x):
    """[B, C, D, H, W] -> 4 x [B, C, D, H, W/2]: d0 - d2, d1 + d2, d2 - d1, d1 - d3 with d_k = x[2i - 1 + k], zero outside."""
    W = x.shape[-1]
    xp = F.pad(x, (1, 1))
    d = [xp[..., k:k + W:2] for k in range(4)]
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]


def wino_G(w):
    """[rows, K, 3, 3, 3] -> 4 x [rows, K, 3, 3, 1]: g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2 along kw."""
    g0, g1, g2 = w[..., 0:1], w[..., 1:2], w[..., 2:3]
    return [g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2]


def _interleave(y0, y1):
    return torch.stack([y0, y1], -1).reshape(y0.shape[:-1] + (2 * y0.shape[-1],))


# ---------------------------------------------------------------------------------------------------------------
# the proof obligations
# ---------------------------------------------------------------------------------------------------------------
def _pairs_zero(a_lo, b_lo, conv):
    """True when no product of the two lo planes that the convolution forms is non-zero."""
    if not bool(a_lo.any()) or not bool(b_lo.any()):
        return True
    return float(conv(a_lo.abs().double(), b_lo.abs().double()).max()) == 0.0


def exactness_margin(case, domain):
    """domain: "direct" (the operand as it is, all taps), "wino" (bf16 split of the T / G images), "wino_f16" (fp16 split of them).
    Returns dict(lolo_zero, split_exact, x_lo_live, w_lo_live, lsb, max_sum): max_sum[name] = max over outputs of sum |term| in lsb
    units, bias and residual included -- name "y" (direct) or "m0" .. "m3" (the frequency accumulators) and "y0" / "y1" (even / odd
    outputs after the inverse transform).  x_lo_live / w_lo_live: in the Winograd domains a list per frequency."""
    assert domain in ("direct", "wino", "wino_f16")
    split = split_fp16 if domain == "wino_f16" else split_bf16
    x = conv_input(case, torch.float32)
    w = _rows(case, case["w_eff"], 0)
    extra = _extras(case, torch.float64, absolute=True)
    if domain == "direct":
        xh, xl = split(x)
        wh, wl = split(w)
        conv = lambda a, b: _conv(a, b, case)
        s = conv((xh.abs() + xl.abs()).double(), (wh.abs() + wl.abs()).double()) + extra
        return dict(lolo_zero=_pairs_zero(xl, wl, conv), split_exact=bool(torch.equal(xh + xl, x) and torch.equal(wh + wl, w)),
                    x_lo_live=bool(xl.any()), w_lo_live=bool(wl.any()), lsb=1.0, max_sum={"y": float(s.max())})
    assert case["kshape"] == (3, 3, 3) and case["stride"] == 1
    lsb = 0.5                                                       # G of even integers: integers; of any integers: halves
    conv = lambda a, b: F.conv3d(a, b, padding=(1, 1, 0))
    out = dict(lolo_zero=True, split_exact=True, x_lo_live=[], w_lo_live=[], lsb=lsb, max_sum={})
    m = []
    for f, (t, gw) in enumerate(zip(wino_T(x), wino_G(w))):
        th, tl = split(t)
        gh, gl = split(gw)
        out["lolo_zero"] &= _pairs_zero(tl, gl, conv)
        out["split_exact"] &= bool(torch.equal(th + tl, t) and torch.equal(gh + gl, gw))
        out["x_lo_live"].append(bool(tl.any()))
        out["w_lo_live"].append(bool(gl.any()))
        m.append(conv((th.abs() + tl.abs()).double(), (gh.abs() + gl.abs()).double()))
        out["max_sum"][f"m{f}"] = float(m[-1].max()) / lsb
    e0, e1 = (extra[..., 0::2], extra[..., 1::2]) if extra.shape[-1] > 1 else (extra, extra)
    out["max_sum"]["y0"] = float((m[0] + m[1] + m[2] + e0).max()) / lsb
    out["max_sum"]["y1"] = float((m[1] + m[2] + m[3] + e1).max()) / lsb
    return out


def eval_fp32(case, domain, order):
    """The kernels' declared arithmetic in fp32 on the CPU: hi*hi + hi*lo + lo*hi with fp32 accumulation, in the direct or the
    Winograd form, in one of two summation orders (order 1: channels reversed and taken in blocks of 8 that are added one after
    the other, the three terms in the opposite order).  Returns fp32 [B, rows, D, H, W]."""
    split = split_fp16 if domain == "wino_f16" else split_bf16
    x = conv_input(case, torch.float32)
    w = _rows(case, case["w_eff"], 0)
    extra = _extras(case, torch.float32)

    def three(a, b, conv):
        ah, al = split(a)
        bh, bl = split(b)
        terms = [(ah, bh), (ah, bl), (al, bh)]
        if order == 0:
            return conv(terms[0][0], terms[0][1]) + conv(terms[1][0], terms[1][1]) + conv(terms[2][0], terms[2][1])
        acc = None
        for p, q in reversed(terms):
            p, q = p.flip(1), q.flip(1)
            for c0 in range(0, p.shape[1], 8):
                y = conv(p[:, c0:c0 + 8].contiguous(), q[:, c0:c0 + 8].contiguous())
                acc = y if acc is None else acc + y
        return acc

    if domain == "direct":
        return three(x, w, lambda a, b: _conv(a, b, case)) + extra
    conv = lambda a, b: F.conv3d(a, b, padding=(1, 1, 0))
    m = [three(t, gw, conv) for t, gw in zip(wino_T(x), wino_G(w))]
    y = _interleave(m[0] + m[1] + m[2], m[1] - m[2] - m[3]) if order == 0 else _interleave(m[2] + m[1] + m[0], (m[1] - m[3]) - m[2])
    return y + extra


def describe_mismatch(got, want, what, limit=6):
    """'' when equal; otherwise the number of differing elements and the coordinates / values of the first few."""
    if got.shape != want.shape:
        return f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if torch.equal(got, want):
        return ""
    bad = ~(got == want)
    idx = bad.nonzero()
    first = "; ".join(f"{tuple(i.tolist())}: got {got[tuple(i.tolist())].item()!r} want {want[tuple(i.tolist())].item()!r}" for i in idx[:limit])
    span = ", ".join(f"{int(idx[:, k].min())}..{int(idx[:, k].max())}" for k in range(idx.shape[1]))
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements differ (index ranges {span}); first: {first}"


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
CUBE_MIN, CUBE_TILES = (8, 8, 8), (16, 16, 16)
G_A, G_B, G_C, G_W24 = (4, 16, 8), (8, 24, 16), (12, 8, 32), (8, 16, 24)      # three different extents, in three orders; W = 24
L_MIN, L_A, L_B, L_C = (4, 4, 4), (4, 8, 12), (8, 4, 12), (12, 8, 4)          # the 4 x 4 x 4-tile configurations

SPECS = []


def _add(entry, cls, dims, parts, cout, B=1, **kw):
    """entry: which launcher of the GPU file takes the case; kw: builder options and launcher options (cfg, ksplit, stats, ...)."""
    kw.setdefault("domains", ["direct"])
    tag = "-".join(str(v) for v in (entry, kw.get("cfg", ""), cls, "x".join(map(str, dims)), "+".join(map(str, parts)), cout, f"B{B}",
                                    kw.get("tag", "")) if v != "")
    assert all(s["id"] != tag for s in SPECS), tag
    SPECS.append(dict(id=tag, entry=entry, cls=cls, dims=dims, parts=parts, cout=cout, B=B, seed=len(SPECS), **kw))


# ---- md_gemm_conv --------------------------------------------------------------------------------------------
for _cfg in ("CFG_C3_128", "CFG_C3_128_FAST"):
    _st = _cfg == "CFG_C3_128_FAST"                              # only the dedicated kernel writes GroupNorm sums without split-K
    _add("gemm", "hi_only", CUBE_MIN, [32], 128, B=2, cfg=_cfg, bias="sample", res="sample", stats=_st)
    _add("gemm", "hi_only", CUBE_TILES, [160], 256, cfg=_cfg, bias="shared", stats=_st)
    _add("gemm", "hi_only", G_A, [64], 128, B=2, cfg=_cfg, bias="sample", res="shared", stats=_st)
    _add("gemm", "x_lo", G_B, [64], 136, B=2, cfg=_cfg, bias="shared", res="sample", stats=_st)           # partial row tile
    _add("gemm", "w_lo", G_C, [96], 128, cfg=_cfg, bias="sample", stats=_st)
    _add("gemm", "hi_only", G_W24, [32], 128, cfg=_cfg, res="sample")
    _add("gemm", "x_lo", (8, 16, 32), [64], 128, B=2, cfg=_cfg, ups=1, bias="shared", tag="ups")
    _add("gemm", "x_lo", CUBE_MIN, [128], 136, B=2, cfg=_cfg, bias="sample", res="sample", ksplit=[2, 3, 4], stats=True, tag="splitk")
    _add("gemm", "w_lo", G_A, [128], 128, B=2, cfg=_cfg, bias="shared", res="shared", ksplit=[2, 4], stats=True, tag="splitk")
# MD_B_F32B_GN: fp32 parts, the affine and the split in the halo loader
_add("gemm", "x_lo", G_B, [64], 128, B=2, cfg="CFG_C3_128_FAST", b_f32=True, bias="shared", stats=True, tag="f32b")
_add("gemm", "hi_only", G_C, [96, 32], 128, B=2, cfg="CFG_C3_128_FAST", b_f32=True, ac=True, bias="sample", res="sample", stats=True, tag="f32b_ac")
_add("gemm", "x_lo", G_A, [32, 32], 136, B=2, cfg="CFG_C3_128_FAST", b_f32=True, ac=True, bias="shared", tag="f32b_ac")
_add("gemm", "w_lo", CUBE_MIN, [64], 128, B=2, cfg="CFG_C3_128_FAST", b_f32=True, ac=True, tag="f32b_ac")
_add("gemm", "x_lo", (8, 16, 32), [32], 128, cfg="CFG_C3_128_FAST", b_f32=True, ups=1, tag="f32b_ups")
_add("gemm", "hi_only", G_A, [64], 128, B=2, cfg="CFG_C3_128_FAST", prec="fp16x2", bias="sample", tag="fp16x2")
_add("gemm", "hi_only", L_MIN, [64], 128, B=2, cfg="CFG_C3_LOW", bias="sample", res="sample")
_add("gemm", "hi_only", L_A, [64], 136, B=2, cfg="CFG_C3_LOW", bias="shared", res="shared")
_add("gemm", "x_lo", L_B, [96], 128, cfg="CFG_C3_LOW", bias="sample")
_add("gemm", "w_lo", L_C, [64], 128, B=2, cfg="CFG_C3_LOW", res="sample")
_add("gemm", "x_lo", L_MIN, [128], 136, B=3, cfg="CFG_C3_LOW", bias="shared", res="sample", ksplit=[2, 3, 4], stats=True, tag="splitk")
_add("gemm", "hi_only", L_A, [64, 32], 128, B=3, cfg="CFG_C3_LOW", b_f32=True, ac=True, bias="shared", ksplit=[2], tag="f32b_ac")
_add("gemm", "x_lo", L_C, [64], 128, B=2, cfg="CFG_C3_LOW", b_f32=True, tag="f32b")
_add("gemm", "hi_only", L_MIN, [32], 64, B=2, cfg="CFG_C3_S2", stride=2, bias="shared")
_add("gemm", "hi_only", L_A, [64], 136, B=2, cfg="CFG_C3_S2", stride=2, bias="sample")
_add("gemm", "x_lo", L_B, [32], 128, cfg="CFG_C3_S2", stride=2, bias="shared")
_add("gemm", "w_lo", L_C, [64], 128, cfg="CFG_C3_S2", stride=2)
_add("gemm", "hi_only", CUBE_MIN, [64], 4, B=2, cfg="CFG_C3_32", out="ncdhw", bias="shared")
_add("gemm", "x_lo", G_A, [64], 4, B=2, cfg="CFG_C3_32", out="ncdhw", bias="shared")
_add("gemm", "w_lo", G_B, [32], 4, cfg="CFG_C3_32", out="ncdhw")
_add("gemm", "hi_only", G_C, [32], 4, cfg="CFG_C3_32", out="ncdhw", bias="shared")
_add("gemm", "hi_only", CUBE_MIN, [4], 128, B=2, cfg="CFG_C3_128_K16", bias="shared")
_add("gemm", "x_lo", G_C, [4], 136, B=2, cfg="CFG_C3_128_K16", res="shared")
_add("gemm", "w_lo", G_A, [4], 128, cfg="CFG_C3_128_K16", bias="sample")
_add("gemm", "hi_only", G_B, [4], 136, B=2, cfg="CFG_C3X_128_K16", bias="shared", res="shared", tag="xfold")
_add("gemm", "x_lo", G_W24, [4], 128, cfg="CFG_C3X_128_K16", tag="xfold")
_add("gemm", "w_lo", CUBE_MIN, [4], 128, B=2, cfg="CFG_C3X_128_K16", bias="shared", tag="xfold")
_add("gemm", "hi_only", G_A, [64], 4, B=2, cfg="CFG_C3X_32", bias="shared", tag="fold_dx")
_add("gemm", "x_lo", G_B, [32], 4, cfg="CFG_C3X_32", bias="shared", tag="fold_dx")
_add("gemm", "w_lo", CUBE_MIN, [64], 4, B=2, cfg="CFG_C3X_32", tag="fold_dx")
_add("gemm", "hi_only", G_C, [32], 4, cfg="CFG_C3X_32", bias="shared", tag="fold_dx")
_add("gemm", "hi_only", CUBE_MIN, [4], 128, B=2, cfg="CFG_C5_128_K16", kshape=(5, 5, 5), bias="shared")
_add("gemm", "x_lo", G_A, [4], 128, cfg="CFG_C5_128_K16", kshape=(5, 5, 5), bias="sample")
_add("gemm", "w_lo", G_B, [4], 136, cfg="CFG_C5_128_K16", kshape=(5, 5, 5))
_add("gemm", "hi_only", G_C, [4], 128, cfg="CFG_C5_128_K16", kshape=(5, 5, 5), res="shared")
_add("gemm", "hi_only", G_C, [64], 4, cfg="CFG_C5_32_K16", kshape=(5, 5, 5), out="ncdhw", bias="shared")
_add("gemm", "x_lo", CUBE_MIN, [32], 4, B=2, cfg="CFG_C5_32_K16", kshape=(5, 5, 5), out="ncdhw")
_add("gemm", "w_lo", G_A, [32], 4, B=2, cfg="CFG_C5_32_K16", kshape=(5, 5, 5), out="ncdhw", bias="shared")
# the dx-folded 5 x 5 x 5 forms the k = 5 model runs: stem K = 4 channels x 5 dx (padded to 32), head rows (co, dx) = 20 of 24 + md_fold_dx
_add("gemm", "hi_only", CUBE_MIN, [4], 128, B=2, cfg="CFG_C5X_128", kshape=(5, 5, 5), bias="shared", res="shared", tag="xfold")
_add("gemm", "x_lo", G_A, [4], 136, B=2, cfg="CFG_C5X_128", kshape=(5, 5, 5), bias="shared", tag="xfold")
_add("gemm", "w_lo", G_B, [4], 128, cfg="CFG_C5X_128", kshape=(5, 5, 5), res="shared", tag="xfold")
_add("gemm", "hi_only", G_C, [4], 128, cfg="CFG_C5X_128", kshape=(5, 5, 5), tag="xfold")
_add("gemm", "hi_only", CUBE_MIN, [64], 4, B=2, cfg="CFG_C5X_32_K16", kshape=(5, 5, 5), bias="shared", tag="fold_dx")
_add("gemm", "x_lo", G_A, [32], 4, B=2, cfg="CFG_C5X_32_K16", kshape=(5, 5, 5), bias="shared", tag="fold_dx")
_add("gemm", "w_lo", G_B, [64], 4, cfg="CFG_C5X_32_K16", kshape=(5, 5, 5), tag="fold_dx")
_add("gemm", "x_lo", G_C, [48], 4, cfg="CFG_C5X_32_K16", kshape=(5, 5, 5), bias="shared", tag="fold_dx")
for _cfg, _P, _co in (("CFG_G1_128", 768, 128), ("CFG_G1_128_N128", 384, 136), ("CFG_G1_128_LOW", 192, 128), ("CFG_G1_64_LOW", 192, 64)):
    _add("gemm", "hi_only", (1, 1, _P), [64], _co, B=2, cfg=_cfg, kshape=(1, 1, 1), bias="shared", res="sample")
    _add("gemm", "x_lo", (1, 1, _P), [96], _co, B=2, cfg=_cfg, kshape=(1, 1, 1), bias="sample")
    _add("gemm", "w_lo", (1, 1, _P), [160], _co, cfg=_cfg, kshape=(1, 1, 1), res="shared")
    # OUT_S16B: hi + lo of an integer of at most 16 bits is exact (smaller operands keep the outputs there)
    _add("gemm", "x_lo", (1, 1, _P), [64], _co, B=2, cfg=_cfg, kshape=(1, 1, 1), bias="shared", out="s16b", xmax=511, wmax=6, nnz=24, tag="s16b")
for _cfg in ("CFG_G1_128", "CFG_G1_128_N128"):
    _add("gemm", "x_lo", (1, 1, 512), [96, 32], 128, B=2, cfg=_cfg, kshape=(1, 1, 1), b_f32=True, bias="shared", tag="f32b")
# ---- the dedicated kernels -----------------------------------------------------------------------------------
_add("s2", "hi_only", CUBE_MIN, [32], 64, B=2, stride=2, bias="shared", stats=True)
_add("s2", "hi_only", CUBE_TILES, [64], 136, stride=2, bias="sample", stats=True)
_add("s2", "x_lo", G_A, [32], 128, B=2, stride=2, bias="sample", stats=True)
_add("s2", "w_lo", G_B, [64], 256, stride=2, bias="shared", stats=True)
_add("s2", "hi_only", G_C, [96], 128, B=2, stride=2, stats=True)
_add("s2", "x_lo", G_W24, [32], 136, stride=2, bias="shared", stats=True)
# Downsample of ddpm_res64 at the first level: 128 -> 128, 64^3 -> 32^3 (B = 1); reference for rows across the row tile only
_add("s2", "x_lo", (32, 32, 32), [128], 128, stride=2, bias="shared", ref_rows=[0, 37, 64, 127], tag="res64")
_add("stem", "hi_only", CUBE_MIN, [4], 128, B=2, bias="shared", res="shared", stats=True)
_add("stem", "hi_only", CUBE_TILES, [4], 136, B=3, bias="shared", res="shared", stats=True)
_add("stem", "x_lo", G_A, [4], 128, B=2, bias="shared", res="shared", stats=True)
_add("stem", "w_lo", G_B, [4], 136, B=2, bias="shared", stats=True)
_add("stem", "hi_only", G_C, [4], 128, res="shared", stats=True)
_add("stem", "x_lo", G_W24, [4], 128, B=2, bias="shared", res="shared", stats=True)
# the stem of ddpm_res64: 4 -> 128 at 64^3 (B = 1)
# (no `tiny` twin: sum o^2 over 2^18 positions cannot stay below 2^24; its sums are held to the tile bound of stats_tolerance)
_add("stem", "x_lo", (64, 64, 64), [4], 128, bias="shared", res="shared", stats=True, stats_exact=False, tag="res64")
for _i, _parts in enumerate(([128], [128, 128], [96, 32], [208, 48])):
    _cls = ("hi_only", "x_lo", "w_lo", "x_lo")[_i]
    _add("nin", _cls, (1, 1, 24576), _parts, 128, B=3, kshape=(1, 1, 1), bias="shared", tag="288tiles")     # more tiles than workgroups, ragged
    _add("nin", ("x_lo", "w_lo", "hi_only", "w_lo")[_i], (1, 1, 768), _parts, 128, B=3, kshape=(1, 1, 1), bias="shared", tag="9tiles")
# the shortcut NIN of an up-level ResnetBlock of ddpm_res64 on the concatenated input: cat(128, 128) -> 128 at 64^3 (B = 1); 8 rows checked
_add("nin", "x_lo", (1, 1, 64 ** 3), [128, 128], 128, kshape=(1, 1, 1), bias="shared", ref_rows=[0, 9, 31, 32, 70, 95, 96, 127], tag="res64")
# ---- Winograd, bf16x3 ----------------------------------------------------------------------------------------
_W = dict(domains=["wino"])
_add("wino", "hi_only", CUBE_MIN, [32], 128, B=2, bias="sample", res="sample", stats=True, **_W)                 # single K body
_add("wino", "hi_only", CUBE_TILES, [64], 256, bias="shared", stats=True, **_W)                                  # unrolled body, two row tiles
_add("wino", "x_lo", G_A, [128], 128, B=2, bias="sample", res="shared", stats=True, **_W)                        # second unrolled body
_add("wino", "w_lo", G_B, [256], 128, bias="shared", res="sample", stats=True, **_W)                             # the K loop
_add("wino", "hi_only", G_C, [96, 32], 128, B=2, ac=True, bias="sample", res="sample", stats=True, tag="ac", **_W)
_add("wino", "x_lo", G_B, [32, 32], 256, B=2, ac=True, bias="shared", tag="ac", **_W)
_add("wino", "w_lo", G_C, [64], 128, B=2, ac=True, res="shared", stats=True, tag="ac", **_W)
_add("wino", "hi_only", G_W24, [64], 128, B=2, bias="shared", res="sample", stats=True, **_W)                    # W = 24: md_wino_prep (one thread per pair)
_add("wino", "x_lo", G_W24, [32], 128, bias="sample", **_W)
_add("wino", "x_lo", (8, 16, 32), [64], 128, B=2, ups=1, bias="shared", stats=True, tag="ups", **_W)
_add("wino", "w_lo", (16, 8, 16), [32], 256, ups=1, tag="ups", **_W)
_add("wino", "w_lo", G_B, [160], 128, B=2, dgrad=True, tag="dgrad", **_W)
_add("wino", "x_lo", G_C, [128], 256, dgrad=True, tag="dgrad", **_W)
_add("wino", "hi_only", G_A, [256], 128, B=2, dgrad=True, tag="dgrad", **_W)
# ResnetBlock conv of ddpm_res64 at the first level: 128 -> 128 at 64^3 (B = 1); reference for rows across the four row tiles
_add("wino", "x_lo", (64, 64, 64), [128], 128, bias="sample", res="sample", ref_rows=[0, 33, 70, 127], tag="res64", **_W)
# ---- Winograd, f16f8 / f16f6 (fp16 products exact, cross terms zero) -----------------------------------------
_F = dict(domains=["wino_f16"])
for _fmt in ("f8", "f6"):
    _add("wino_" + _fmt, "f16", CUBE_MIN, [32], 128, B=2, bias="sample", res="sample", stats=True, **_F)
    _add("wino_" + _fmt, "hi_only", CUBE_TILES, [64], 256, bias="shared", stats=True, **_F)
    _add("wino_" + _fmt, "f16", G_A, [128], 128, B=2, bias="shared", res="shared", stats=True, eq=True, tag="eq", **_F)
    _add("wino_" + _fmt, "f16", G_B, [96, 32], 128, ac=True, bias="sample", stats=True, eq=True, tag="ac_eq", **_F)
    _add("wino_" + _fmt, "f16", G_C, [256], 256, res="sample", **_F)
    _add("wino_" + _fmt, "f16", (8, 16, 32), [64], 128, B=2, ups=1, bias="shared", tag="ups", **_F)
    # the ResnetBlock conv of ddpm_res64 at the first level in the inference arithmetic: 128 -> 128 at 64^3 (B = 1), 4 rows checked
    _add("wino_" + _fmt, "f16", (64, 64, 64), [128], 128, bias="sample", res="sample", ref_rows=[0, 33, 70, 127], tag="res64", **_F)
# the training data gradient: md_wino_prep_dual_f6 + flipped f16f6 fragments (fixed pre-scale 2^8: |G| 2^8 stays inside fp16) +
# md_conv3_wino_f6_scaled, with the lift from the tensor's own maximum and with a constant one
_add("wino_dgrad_f6", "f16", G_B, [160], 128, B=2, dgrad=True, lift="dyn", wmax=84, **_F)
_add("wino_dgrad_f6", "f16", G_C, [128], 256, dgrad=True, lift="const", wmax=84, **_F)
_add("wino_dgrad_f6", "hi_only", CUBE_TILES, [128], 128, B=2, dgrad=True, lift="dyn", **_F)

IDS = [s["id"] for s in SPECS]
LIFT_CONST = 16.0         # the constant lift the data-gradient launcher passes as `tscale` (and divides out as `out_scale`)


def equaliser(spec, cin):
    """The hand-made power-of-two equaliser of a case with `eq` (float [cin], entries 2^-1 .. 2^2), or None."""
    if not spec.get("eq"):
        return None
    pick = torch.randint(0, 4, (cin,), generator=torch.Generator().manual_seed(5))
    return torch.tensor([0.5, 1.0, 2.0, 4.0])[pick].contiguous()


def fp16_extremes(case):
    """(largest |operand|, largest |weight|) the fp16 planes of the f16f8 / f16f6 kernels hold for this case, from its tensors and the
    scales its launcher passes, restating the kernels' own scale choices:
      forward   operand T(act * eq); weights G 2^sw / eq with sw = 7 - ilogb(1.5 max |w|)   (md_pack.h md_wino_f8_wscale)
      dgrad     operand T(dy 2^k) with k = 4 - ilogb(max |dy|) (md_common.h md_dgrad_lift_log2) or 2^k = LIFT_CONST; weights G 2^8"""
    import math
    spec = case["spec"]
    x = conv_input(case, torch.float64)
    gmax_of = lambda w: max(float(v.abs().max()) for v in wino_G(w.double()))
    if spec["entry"] == "wino_dgrad_f6":
        lift = 2.0 ** (4 - math.frexp(float(x.abs().max()))[1] + 1) if spec["lift"] == "dyn" else LIFT_CONST
        return max(float(v.abs().max()) for v in wino_T(x * lift)), gmax_of(case["w_eff"]) * 2.0 ** 8
    eq = equaliser(spec, case["cin"])
    eq = torch.ones(case["cin"], dtype=torch.float64) if eq is None else eq.double()
    sw = 7 - (math.frexp(1.5 * float(case["w"].abs().max()))[1] - 1)
    t = max(float(v.abs().max()) for v in wino_T(x * eq[None, :, None, None, None]))
    return t, gmax_of(case["w_eff"] / eq.float()[None, :, None, None, None]) * 2.0 ** sw


def spec_of(case_id):
    return SPECS[IDS.index(case_id)]


# ---------------------------------------------------------------------------------------------------------------
# the loaders that cannot be exact: a transparent convolution in front of GroupNorm affine + SiLU
# ---------------------------------------------------------------------------------------------------------------
# Arbitrary affines and SiLU round, so the CONV is made transparent instead: every output row has ONE non-zero tap with a
# power-of-two value, rows use different input channels and all 27 taps, so out[co][p] = 2^k act[ci(co)][p + tap(co)] (zero
# where the tap leaves the grid) and the only error is the loader's, visible per element including the zero rim.
LOG2E_F32 = float(torch.tensor(-1.4426950408889634, dtype=torch.float32))     # the literal of the loaders, as fp32 holds it
U = 2.0 ** -24                                                                  # half an ulp of fp32, relative
SPLIT_ERR = 2.0 ** -17 + U                                                      # bf16 hi + lo of a value and its fp32 sum (see loader_bound)


def transparent_weights(cout, cin, seed, wset=0):
    """One tap per row: row co reads channel (5 co + 3 + 4 wset) % cin at tap (7 co + 1 + seed + 4 wset) % 27 with the value
    2^((co % 5) - 2).  With cout >= max(cin, 27) one set meets every channel and tap; the four rows of the head read channels
    3, 8, 13, 18 (+ 4 wset): one residue mod 4 each, so cin / 4 sets meet every channel, and 27 sets every tap
    (`transparent_sets`)."""
    w = torch.zeros((cout, cin, 27))
    co = torch.arange(cout)
    w[co, (5 * co + 3 + 4 * wset) % cin, (7 * co + 1 + seed + 4 * wset) % 27] = torch.exp2(((co % 5) - 2).float())
    return w.reshape(cout, cin, 3, 3, 3)


def transparent_sets(cout, cin):
    """Weight sets a launcher runs so that every input channel and every tap is observed."""
    if cout >= max(cin, 27):
        return 1
    assert cout == 4 and cin % 4 == 0
    return max(cin // 4, 27)


def transparent_case(B, parts, cout, dims, seed, zmax=12.0):
    """x, (a, c) and one-tap weights: z = a x + c uniform in [-zmax, zmax], |a| in [2^-6, 2^6), 0.25 <= |c| < 3, both signs."""
    g = torch.Generator().manual_seed(7000 + seed)
    cin = sum(parts)
    z = (torch.rand((B, cin) + tuple(dims), generator=g) * 2 - 1) * zmax
    sign = lambda shape: 2.0 * torch.randint(0, 2, shape, generator=g).float() - 1.0
    a = torch.exp2(torch.randint(-6, 6, (B, cin), generator=g).float()) * (1.0 + torch.rand((B, cin), generator=g)) * sign((B, cin))
    c = (0.25 + 2.75 * torch.rand((B, cin), generator=g)) * sign((B, cin))
    x = ((z - c[:, :, None, None, None]) / a[:, :, None, None, None]).float().contiguous()
    w = transparent_weights(cout, cin, seed)
    return dict(seed=seed, x=x, x_raw=[t.contiguous() for t in torch.split(x, list(parts), dim=1)], ac=torch.stack([a, c], -1).contiguous(), w=w, w_eff=w,
                B=B, cin=cin, cout=cout, dims=tuple(dims), stride=1, ups=0, rows=None, kshape=(3, 3, 3), bias=None, res=None)


def _azc(case):
    x = case["x"].double()
    a, c = (case["ac"][..., i].double()[:, :, None, None, None] for i in (0, 1))
    return a * x, a * x + c, c


def activation64(case):
    """silu(x a + c) in float64 from the fp32 x, a, c the kernel is given."""
    _, z, _ = _azc(case)
    return z * torch.sigmoid(z)


def loader_bound(case, split=True):
    """Per element of the ACTIVATED tensor: what the halo loaders (conv3_main.hip act_transform, gemm_conv.hip, conv3_head.hip,
    conv3_wino.hip / wino_prep2.hip phase 1) may lose against silu(z), z = a x + c, s = silu(z), derived from their instruction
    sequence  y = x * a + c;  s = y * rcp(1 + exp2(y * -log2 e));  hi = bf16(s);  lo = bf16(s - hi):
      y            one fma or a multiply and an add: |dy| <= 2^-24 |a x| + 2^-24 |y| <= 2^-23 (|a x| + |c|); through |silu'| <= 1.1:
                       1.1 * 2^-23 (|a x| + |c|)
      y * -log2 e  the fp32 constant (2^-25 relative) and one rounding (2^-24): the exponent moves by <= 1.5 * 2^-24 * 1.4427 |z|, the
                   exponential by ln 2 times that: <= 0.75 * 2^-23 |z| relative
      v_exp_f32    1 ulp = 2^-23 relative;  1 + e: 2^-24;  v_rcp_f32: 1 ulp = 2^-23;  y * r: 2^-24
                   (an error of e reaches sigma = 1 / (1 + e) with the factor e / (1 + e) < 1)
                       together <= (3 + 0.75 |z|) 2^-23 |s| <= (4 + |z|) 2^-23 |s|
      split        s in [2^e, 2^(e+1)): hi = RNE to 8 significant bits, |s - hi| <= 2^(e-8); the remainder lies in a binade
                   2^f <= |s - hi| with f <= e - 9 (or is the power of two 2^(e-8) itself: exact), so |(s - hi) - lo| <= 2^(f-8)
                   <= 2^(e-17) <= 2^-17 |s|, and the value is attained (RNE is deterministic: hardware and restatement agree).
                   [2^-18 |s|, i.e. 2^-9 relative per rounding, holds against the TOP of the binade only; the fp32 restatement
                   reaches 0.498 * 2^-16 |s|.]  The fp32 accumulator then holds 2^k hi + 2^k lo, which can span more than 24
                   bits:  + 2^-24 |s|
    split = False leaves the last line out (the Winograd path splits the TRANSFORMED value: `wino_transparent_bound`)."""
    ax, z, c = _azc(case)
    s = (z * torch.sigmoid(z)).abs()
    b = (4.0 + z.abs()) * 2.0 ** -23 * s + 1.1 * 2.0 ** -23 * (ax.abs() + c.abs())
    return b + SPLIT_ERR * s if split else b


def loader_fp32(case, split=True):
    """The loaders' formula restated in fp32 with a correctly rounded exp2 and reciprocal (fp32 tensor; with `split` the value
    hi + lo rounded to fp32, as the accumulator holds it)."""
    x = case["x"]
    a, c = (case["ac"][..., i][:, :, None, None, None] for i in (0, 1))
    y = x * a + c
    e = torch.exp2((y * LOG2E_F32).double()).float()
    r = (1.0 / (1.0 + e).double()).float()
    s = y * r
    if not split:
        return s
    hi, lo = split_bf16(s)
    return (hi.double() + lo.double()).float()


def _shift(t, dz, dy, dx):
    """out[.., z, y, x] = t[.., z + dz, y + dy, x + dx], zero where that leaves the grid."""
    out = torch.zeros_like(t)
    D, H, W = t.shape[-3:]
    z0, z1, y0, y1, x0, x1 = max(0, -dz), min(D, D - dz), max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    out[..., z0:z1, y0:y1, x0:x1] = t[..., z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def transparent_reference(case, w=None, act=None, bound=None):
    """float64 [B, cout, D, H, W]: the one-tap conv of the float64 activation, out[co] = 2^k shift(act[ci(co)], tap(co)) (a single
    term per output: exact), and the bound moved the same way.  w: another weight set of the case (act / bound: activation64 /
    loader_bound of the case, computed once by the caller)."""
    w = case["w_eff"] if w is None else w
    act = activation64(case) if act is None else act
    bound = loader_bound(case) if bound is None else bound
    ref, bnd = [], []
    for co in range(w.shape[0]):
        (ci, kd, kh, kw), = w[co].nonzero().tolist()
        v = float(w[co, ci, kd, kh, kw])
        ref.append(v * _shift(act[:, ci], kd - 1, kh - 1, kw - 1))
        bnd.append(abs(v) * _shift(bound[:, ci], kd - 1, kh - 1, kw - 1))
    return torch.stack(ref, 1), torch.stack(bnd, 1)


def _wino_abs_T(e):
    """sum_k |B[f][k]| e_k: the transform of error bounds."""
    W = e.shape[-1]
    ep = F.pad(e, (1, 1))
    d = [ep[..., k:k + W:2] for k in range(4)]
    return [d[0] + d[2], d[1] + d[2], d[2] + d[1], d[1] + d[3]]


def wino_transparent_bound(case, parts=False):
    """The same through md_wino_prep* (silu = 1) + md_conv3_wino.  The pass activates d_0 .. d_3 (loader_bound without the split),
    forms T_f = d_i -+ d_j in fp32 (2^-24 |T_f|) and splits THAT (2^-17 |T_f|); the kernel accumulates G_f (hi + lo) per frequency
    (G_f = 2^k or 2^(k - 1): exact; 2^-24 per accumulator) and adds three of them (2 x 2^-24 of the running sum):
        |err y| <= sum_f |A[y][f]| |G_f| (sum_k |B[f][k]| E(d_k) + (2^-17 + 2^-24) |T_f|)  +  3 * 2^-24 sum_f |A[y][f]| |G_f T_f|."""
    e_t = _wino_abs_T(loader_bound(case, split=False))
    t = wino_T(activation64(case))
    gw = [v.abs() for v in wino_G(case["w_eff"].double())]
    conv = lambda u, v: F.conv3d(u, v, padding=(1, 1, 0))
    m_err = [conv(e_t[f] + (2.0 ** -17 + U) * t[f].abs(), gw[f]) for f in range(4)]
    m_abs = [conv(t[f].abs(), gw[f]) for f in range(4)]
    y0 = m_err[0] + m_err[1] + m_err[2] + 3 * U * (m_abs[0] + m_abs[1] + m_abs[2])
    y1 = m_err[1] + m_err[2] + m_err[3] + 3 * U * (m_abs[1] + m_abs[2] + m_abs[3])
    if parts:       # the share of the deterministic roundings (transform, split, accumulation) alone
        return _interleave(y0, y1), (2.0 ** -17 + 5 * U) * _interleave(m_abs[0] + m_abs[1] + m_abs[2], m_abs[1] + m_abs[2] + m_abs[3])
    return _interleave(y0, y1)


def wino_loader_fp32(case):
    """fp32 restatement of the Winograd path on a transparent case: activate, transform in fp32, split, G (hi + lo) exactly, the
    three frequencies added in fp32."""
    t = wino_T(loader_fp32(case, split=False))
    gw = wino_G(case["w_eff"])
    conv = lambda u, v: F.conv3d(u, v, padding=(1, 1, 0))
    m = []
    for f in range(4):
        hi, lo = split_bf16(t[f])
        m.append(conv((hi.double() + lo.double()), gw[f].double()).float())
    return _interleave((m[1] + m[0]) + m[2], (m[1] - m[2]) - m[3])


# (name, B, parts, cout, dims, seed): what tests/test_gpu_conv_exact.py launches with SiLU on
TRANSPARENT = [
    ("fast-8x8x8", 2, [64], 128, CUBE_MIN, 0), ("fast-8x24x16", 1, [96, 32], 128, G_B, 1), ("fast-12x8x32", 2, [64], 136, G_C, 2),
    ("low-4x4x4", 2, [64], 128, L_MIN, 3), ("low-4x8x12", 2, [64, 32], 128, L_A, 4),
    ("wino-8x8x8", 2, [64], 128, CUBE_MIN, 5), ("wino-8x24x16", 1, [96, 32], 128, G_B, 6), ("wino-8x16x24", 2, [64], 128, G_W24, 7),
    ("head-8x8x8", 2, [64], 4, CUBE_MIN, 8), ("head-4x16x8", 2, [128], 4, G_A, 9), ("head-8x24x16", 1, [64], 4, G_B, 10),
    ("head-12x8x32", 1, [32], 4, G_C, 11),
    # the head of ddpm_res64: GroupNorm + SiLU + 128 -> 4 at 64^3 (B = 1)
    ("head-64x64x64", 1, [128], 4, (64, 64, 64), 12),
]
TRANSPARENT_IDS = [t[0] for t in TRANSPARENT]


def transparent_of(name):
    t = TRANSPARENT[TRANSPARENT_IDS.index(name)]
    return transparent_case(*t[1:])
