"""Inputs on which the weight-gradient kernels' arithmetic is EXACT, their float64 references and the proof obligations
(tests/test_gpu_wgrad_exact.py launches them on the GPU and demands torch.equal with the float64 result at every element of
dW; tests/test_cpu_wgrad_cases.py proves on the CPU that every case is in the regime it claims).  Plain helper module on the
pattern of tests/conv_cases.py: no fixtures, no GPU, only torch.

The kernels (csrc/wgrad.hip, csrc/wgrad_wino.hip) contract the output gradient dY with the activation A over (sample,
position) per tap:  dW[co][ci][tap] += sum dY[co][pos] A[ci][pos + off(tap)],  as hi*hi + hi*lo + lo*hi of bf16 planes with
fp32 accumulation (lo*lo is dropped).  On small integers every product and every partial sum below 2^24 is exact, so the
result does not depend on the summation order, the K split, the z-slab cut or the Winograd transforms and equals the float64
gradient bit for bit; one wrong tap offset, masked position, K range, plane or stride changes at least one integer.

Classes (`cls`): only ONE lo plane may be live
    hi_only   A and dY within 8 significant bits in the kernel's own domain (T = B^T d and U for md_wgrad_wino)
    a_lo      A 9 .. 11 bits (lo plane live, for Winograd in all four T), dY <= 5 bits     -- a dropped / misplaced hi*lo pass
    dy_lo     A <= 4 bits, dY 9 .. 11 bits (lo plane live, in all four U)                   -- a dropped / misplaced lo*hi pass
dY is EVEN (then every Winograd frequency sum is even and the reduce kernel's 0.5f (n1 +- n2) is an integer) and SPARSE: the
contraction is B * P long, so `nnz` non-zero positions per dY channel on average bound sum |term| whatever the grid is.
Values are hashed (torch.randint over the whole tensor from a seeded generator), and dW0, the integer the kernels accumulate
onto, is non-zero everywhere."""
import math

import torch
import torch.nn.functional as F

from attn_cases import split_bf16
from conv_cases import LIMIT, _randint, describe_mismatch, wino_T  # noqa: F401  (re-exported for the two test modules)

# amax: |A| <= amax; dymax: |dY| <= dymax (even); nnz: mean number of non-zero positions per dY channel over (sample, position),
# for the direct contraction and for the Winograd one (its operands are up to twice as large on both sides)
CLASSES = {
    "hi_only": dict(amax=127, dymax=30, nnz=2000, nnz_wino=800),
    "a_lo": dict(amax=1023, dymax=14, nnz=1000, nnz_wino=300),
    "dy_lo": dict(amax=7, dymax=1022, nnz=1000, nnz_wino=300),
}
DW0_MAX = 999
SENTINEL = 98765.5            # fills the buffer around the addressed elements of dW; no integer, so no element of dW equals it
MARGIN = 64                   # floats in front of and behind the addressed span


def zsplit_for(B, D):
    """backward.zsplit_for restated: 8 / gcd(B, 8) z-slabs per sample, halved until the depth divides."""
    zs = 8 // math.gcd(int(B), 8)
    while zs > 1 and D % zs:
        zs //= 2
    return zs


# ---------------------------------------------------------------------------------------------------------------
# builder
# ---------------------------------------------------------------------------------------------------------------
def strides_of(spec):
    """(s_row, s_k, s_tap) of the case's dW."""
    co, ci, taps = spec["co"], spec["ci"], spec["taps"]
    kind = spec.get("strides", "nin" if spec["entry"] == "nin" or taps == 1 else "conv")
    return {"conv": (ci * taps, taps, 1),                 # dW[co][ci][taps]
            "gap": ((ci + 5) * taps, taps, 1),            # the same inside rows of ci + 5 columns: unaddressed floats between the rows
            "tapfirst": (ci, 1, co * ci),                 # dW[taps][co][ci]
            "nin": (1, co, 0),                            # NIN: W[ci][co]
            "nin_gap": (1, co + 3, 0)}[kind]


def build(spec):
    """spec: dict(id, entry "pb" | "wino" | "nin", cls, B, co, ci, dims=(D, H, W) of the grid the taps slide over, taps,
    a_ch / b_ch (channels of the dY / A tensors, >= co / ci; the surplus is LIVE and must not reach dW), stuff / up, seed).
    Returns the case: a fp32 [B, b_ch, ..] and dy fp32 [B, a_ch, ..] as the operand passes are given them (`stuff`: dY on the
    coarse grid; `up`: A on the coarse grid), dw0 fp32 [co, ci, taps]."""
    p = CLASSES[spec["cls"]]
    B, co, ci, taps = spec["B"], spec["co"], spec["ci"], spec["taps"]
    a_ch, b_ch = spec.get("a_ch", co), spec.get("b_ch", ci)
    D, H, W = spec["dims"]
    half = tuple(s // 2 for s in (D, H, W))
    g = torch.Generator().manual_seed(4000 + spec["seed"])
    a = _randint(g, -p["amax"], p["amax"], (B, b_ch) + (half if spec.get("up") else (D, H, W)))
    dgrid = half if spec.get("stuff") else (D, H, W)
    dy = 2.0 * _randint(g, -(p["dymax"] // 2), p["dymax"] // 2, (B, a_ch) + dgrid)
    npos = B * dgrid[0] * dgrid[1] * dgrid[2]
    nnz = spec.get("nnz", p["nnz_wino"] if spec["entry"] == "wino" else p["nnz"])
    dy = dy * (torch.rand(dy.shape, generator=g) < min(1.0, nnz / float(npos))).float()
    dw0 = _randint(g, 1, DW0_MAX, (co, ci, taps)) * (2.0 * torch.randint(0, 2, (co, ci, taps), generator=g).float() - 1.0)
    return dict(spec=spec, a=a.contiguous(), dy=dy.contiguous(), dw0=dw0, B=B, co=co, ci=ci, a_ch=a_ch, b_ch=b_ch, dims=(D, H, W), taps=taps,
                ksz={1: 1, 27: 3, 125: 5}[taps], strides=strides_of(spec))


def act_full(case, dtype=torch.float64):
    """A on the grid the taps slide over, [B, ci, D, H, W] (nearest x2 for `up`); only the `ci` columns dW has."""
    a = case["a"][:, :case["ci"]].to(dtype)
    return F.interpolate(a, scale_factor=2, mode="nearest") if case["spec"].get("up") else a


def dy_full(case, dtype=torch.float64):
    """dY on the same grid, [B, co, D, H, W]; `stuff`: the coarse gradient at the odd positions, zeros elsewhere (the stride-2
    conv's weight gradient: out[o] = sum_t w[t] x[2 o + t] on F.pad(x, (0, 1) * 3), so dW[t] = sum_o dY[o] x[(2 o + 1) + (t - 1)])."""
    dy = case["dy"][:, :case["co"]].to(dtype)
    if not case["spec"].get("stuff"):
        return dy
    out = torch.zeros(dy.shape[:2] + case["dims"], dtype=dtype)
    out[:, :, 1::2, 1::2, 1::2] = dy
    return out


# ---------------------------------------------------------------------------------------------------------------
# the contraction as one matrix product per tap over shifted views
# ---------------------------------------------------------------------------------------------------------------
def _rows(t):
    """[B, C, ...] -> [C, B * positions]."""
    return t.transpose(0, 1).reshape(t.shape[1], -1)


def shifted(a, kd, kh, kw):
    """a [B, C, D, H, W] -> kd * kh * kw matrices [C, B * P]: a at position + (dz - kd // 2, dy - kh // 2, dx - kw // 2), zero outside."""
    D, H, W = a.shape[2:]
    ap = F.pad(a, (kw // 2, kw // 2, kh // 2, kh // 2, kd // 2, kd // 2))
    return [_rows(ap[:, :, z:z + D, y:y + H, x:x + W]) for z in range(kd) for y in range(kh) for x in range(kw)]


def contract(dym, mats, chunks=None):
    """sum over the columns of dym [R, N] x mats[t] [C, N] -> [R, C, len(mats)], the columns taken in the given chunks (list of
    (start, stop); the partial products are added in that order in the operands' dtype)."""
    N = dym.shape[1]
    chunks = [(0, N)] if chunks is None else chunks
    out = []
    for m in mats:
        acc = None
        for c0, c1 in chunks:
            if c1 > c0:
                y = dym[:, c0:c1] @ m[:, c0:c1].t()
                acc = y if acc is None else acc + y
        out.append(acc)
    return torch.stack(out, -1)


def reference(case):
    """float64 [co, ci, taps]: dW0 + the weight gradient (for NIN taps = 1; the launcher's strides place it as W[ci][co])."""
    k = case["ksz"]
    return case["dw0"].double() + contract(_rows(dy_full(case)), shifted(act_full(case), k, k, k))


def autograd_reference(case, rows, cols):
    """The same for a few rows and columns through float64 autograd of nn.Conv3d / the NIN einsum -- what `reference` must equal."""
    spec, k = case["spec"], case["ksz"]
    dy = case["dy"][:, rows].double()
    if spec.get("stuff"):
        x = F.pad(case["a"][:, cols].double(), (0, 1, 0, 1, 0, 1))
        g = torch.nn.grad.conv3d_weight(x, (len(rows), len(cols), 3, 3, 3), dy, stride=2)
    else:
        x = act_full(case)[:, cols]
        g = torch.nn.grad.conv3d_weight(x, (len(rows), len(cols), k, k, k), dy, padding=k // 2)
    return case["dw0"][rows][:, cols].double() + g.reshape(len(rows), len(cols), -1)


# ---------------------------------------------------------------------------------------------------------------
# Winograd F(2, 3) along w, as md_wino_prep / md_wino_prep_dual / md_wgrad_wino define it
# ---------------------------------------------------------------------------------------------------------------
def wino_U(dy):
    """[B, C, D, H, W] -> 4 x [B, C, D, H, W/2]: (v0, v0 + v1, v0 - v1, v1) of every output pair, md_wino_prep_dual's second output."""
    v0, v1 = dy[..., 0::2], dy[..., 1::2]
    return [v0, v0 + v1, v0 - v1, v1]


def wino_out(n, order=0):
    """The reduce kernel's output transform: 4 x [R, C, 9] -> [R, C, 27] (dg0 = n0 + (n1 + n2) / 2, dg1 = (n1 - n2) / 2,
    dg2 = (n1 + n2) / 2 - n3), in two algebraic orders."""
    if order == 0:
        h12 = 0.5 * (n[1] + n[2])
        g = [n[0] + h12, 0.5 * (n[1] - n[2]), h12 - n[3]]
    else:
        g = [(0.5 * n[2] + n[0]) + 0.5 * n[1], 0.5 * n[1] - 0.5 * n[2], (0.5 * n[2] - n[3]) + 0.5 * n[1]]
    return torch.stack(g, -1).reshape(n[0].shape[0], n[0].shape[1], 27)


# ---------------------------------------------------------------------------------------------------------------
# the proof obligations
# ---------------------------------------------------------------------------------------------------------------
def operands(case, domain, dtype=torch.float32):
    """The operand pairs the kernel contracts in `domain`: list of (dY-side [B, co, ..], A-side [B, ci, ..], (kd, kh, kw))
    -- one pair ("direct": md_wgrad, md_wgrad_nin) or the four frequencies ("wino": U_f, T_f, taps (3, 3, 1))."""
    a, dy = act_full(case, dtype), dy_full(case, dtype)
    if domain == "direct":
        k = case["ksz"]
        return [(dy, a, (k, k, k))]
    assert domain == "wino" and case["taps"] == 27
    return [(u, t, (3, 3, 1)) for u, t in zip(wino_U(dy), wino_T(a))]


def exactness_margin(case, domain):
    """dict(split_exact, lolo_zero, a_lo_live, dy_lo_live (a list per frequency for "wino"), dy_even, max_sum): max_sum[name] =
    the largest sum |term| an accumulator meets, dW0 included where it is added -- "tap" (direct: per (co, ci, tap)), or
    "n0" .. "n3" (the frequency accumulators), "n1+n2" (the reduce kernel's 0.5f (n1 +- n2)) and "dg0" .. "dg2" (Winograd)."""
    out = dict(split_exact=True, lolo_zero=True, a_lo_live=[], dy_lo_live=[], dy_even=True, max_sum={})
    sums = []
    for u, t, ks in operands(case, domain):
        uh, ul = split_bf16(u)
        th, tl = split_bf16(t)
        out["split_exact"] &= bool(torch.equal(uh + ul, u) and torch.equal(th + tl, t))
        out["dy_even"] &= bool(torch.equal((u * 0.5).round() * 2.0, u))
        out["a_lo_live"].append(bool(tl.any()))
        out["dy_lo_live"].append(bool(ul.any()))
        if bool(ul.any()) and bool(tl.any()):
            out["lolo_zero"] &= float(contract(_rows(ul.abs().double()), shifted(tl.abs().double(), *ks)).max()) == 0.0
        sums.append(contract(_rows((uh.abs() + ul.abs()).double()), shifted((th.abs() + tl.abs()).double(), *ks)))
    w0 = case["dw0"].abs().double()
    if domain == "direct":
        out["max_sum"]["tap"] = float((sums[0] + w0).max())
        return out
    for f in range(4):
        out["max_sum"][f"n{f}"] = float(sums[f].max())
    h = sums[1] + sums[2]
    out["max_sum"]["n1+n2"] = float(h.max())
    w0 = w0.reshape(case["co"], case["ci"], 9, 3)
    out["max_sum"]["dg0"] = float((w0[..., 0] + sums[0] + 0.5 * h).max())
    out["max_sum"]["dg1"] = float((w0[..., 1] + 0.5 * h).max())
    out["max_sum"]["dg2"] = float((w0[..., 2] + 0.5 * h + sums[3]).max())
    return out


def eval_fp32(case, domain, order):
    """The kernels' declared arithmetic in fp32 on the CPU: hi*hi + hi*lo + lo*hi with fp32 accumulation over K ranges, in one of
    two summation orders with two different K splits (order 0: lo*hi, hi*lo, hi*hi as the kernels issue them, two equal ranges;
    order 1: the terms reversed, three uneven ranges taken back to front), the Winograd form with the reduce kernel's output
    transform in two algebraic orders.  Returns fp32 [co, ci, taps] including dW0."""
    res = []
    for u, t, ks in operands(case, domain):
        uh, ul = split_bf16(u)
        th, tl = split_bf16(t)
        terms = [(ul, th), (uh, tl), (uh, th)]
        N = u.shape[0] * u[0, 0].numel()
        if order == 0:
            chunks = [(0, N // 2), (N // 2, N)]
        else:
            terms = terms[::-1]
            chunks = [(N - N // 7, N), (N // 3, N - N // 7), (0, N // 3)]
        acc = None
        for p, q in terms:
            y = contract(_rows(p), shifted(q, *ks), chunks)
            acc = y if acc is None else acc + y
        res.append(acc)
    g = res[0] if domain == "direct" else wino_out(res, order)
    return case["dw0"] + g if order == 0 else g + case["dw0"]


# ---------------------------------------------------------------------------------------------------------------
# the buffer dW lives in
# ---------------------------------------------------------------------------------------------------------------
def dw_index(case):
    """int64 [co, ci, taps]: the float each element of dW is addressed at, counted from the pointer the kernel is given."""
    s_row, s_k, s_tap = case["strides"]
    r, c, t = torch.arange(case["co"])[:, None, None], torch.arange(case["ci"])[None, :, None], torch.arange(case["taps"])[None, None, :]
    return r * s_row + c * s_k + t * s_tap


def dw_buffer(case, values):
    """The flat fp32 buffer around dW: SENTINEL everywhere (MARGIN floats in front, the gaps between the addressed elements, MARGIN
    behind), `values` [co, ci, taps] at the addressed ones.  The kernel is handed buffer[MARGIN:]."""
    idx = dw_index(case)
    buf = torch.full((int(idx.max()) + 1 + 2 * MARGIN,), SENTINEL, dtype=torch.float32)
    buf[idx.reshape(-1) + MARGIN] = values.reshape(-1).float()
    return buf


# ---------------------------------------------------------------------------------------------------------------
# md_to_pb16 + md_wgrad restated on the host: the z-slab layout and the slot -> tap map
# ---------------------------------------------------------------------------------------------------------------
def pb16_values(x, zs, pad, zhalo, guard):
    """x [B, C, D, H, W] (values, not planes) -> [ceil(B zs / 8) * 8 virtual samples, C, guard + (Dz + 2 pad)(H + 2 pad)(W + 2 pad)
    + guard]: sample b is cut into zs z-slabs of Dz = D / zs planes, virtual sample v = b * zs + slab; every slab is padded by
    `pad`; its z-halo planes hold the neighbouring slab's planes (zhalo = 1: activation) or zeros (zhalo = 0: dY); the grid's own
    halo, the guards and the virtual samples that fill the last block of 8 are zero."""
    B, C, D, H, W = x.shape
    Dz = D // zs
    full = F.pad(x, (pad,) * 6)
    VB = B * zs
    Pp = (Dz + 2 * pad) * (H + 2 * pad) * (W + 2 * pad)
    out = torch.zeros(((VB + 7) // 8 * 8, C, guard + Pp + guard), dtype=x.dtype)
    for v in range(VB):
        b, slab = divmod(v, zs)
        blk = full[b, :, slab * Dz:slab * Dz + Dz + 2 * pad].clone()
        if not zhalo:
            blk[:, :pad] = 0
            blk[:, pad + Dz:] = 0
        out[v, :, guard:guard + Pp] = blk.reshape(C, Pp)
    return out


def slot_taps(taps):
    """[(slot, tap or None, position offset in units of (plane, row, 1) = (dz, dy, dx))] of md_wgrad's accumulators: slot = group * NTAP
    + t.  taps 27: group = (dz, dy), t = dx.  taps 125: group = ((dz, dy), h), window h covers dx = 3 h + t - 2; h = 1, t = 2 would
    be dx = +3: computed and discarded (tap None).  taps 1: the one slot."""
    if taps == 1:
        return [(0, 0, (0, 0, 0))]
    if taps == 27:
        return [(g * 3 + t, g * 3 + t, (g // 3 - 1, g % 3 - 1, t - 1)) for g in range(9) for t in range(3)]
    out = []
    for g in range(50):
        zy, h = g >> 1, g & 1
        for t in range(3):
            dx = 3 * h + t
            out.append((g * 3 + t, zy * 5 + dx if dx < 5 else None, (zy // 5 - 2, zy % 5 - 2, dx - 2)))
    return out


def pb16_model(case):
    """float64 [co, ci, taps]: dW0 + the contraction as md_wgrad walks it -- over the interior positions of every virtual sample of
    the PB16 tensors (dY with zhalo = 0, A with zhalo = 1), one position offset per slot, the slots mapped to taps."""
    taps, (D, H, W) = case["taps"], case["dims"]
    assert H == W
    pad = 2 if taps == 125 else 1
    zs = zsplit_for(case["B"], D)
    Dz, sp = D // zs, H + 2 * pad
    guard = pad * (sp * sp + sp + 1) + 10
    dyp = pb16_values(dy_full(case), zs, pad, 0, guard)
    ap = pb16_values(act_full(case), zs, pad, 1, guard)
    z, y, x = torch.meshgrid(torch.arange(Dz), torch.arange(H), torch.arange(W), indexing="ij")
    pos = (guard + ((z + pad) * sp + (y + pad)) * sp + pad + x).reshape(-1)
    dym = dyp[:, :, pos].permute(1, 0, 2).reshape(case["co"], -1)
    out = torch.zeros((case["co"], case["ci"], taps), dtype=torch.float64)
    seen = set()
    for _, tap, (dz, dy_, dx) in slot_taps(taps):
        if tap is None:
            continue
        assert tap not in seen
        seen.add(tap)
        am = ap[:, :, pos + (dz * sp + dy_) * sp + dx].permute(1, 0, 2).reshape(case["ci"], -1)
        out[:, :, tap] = dym @ am.t()
    assert len(seen) == taps
    return case["dw0"].double() + out


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
C4, C8, C12, C16 = (4, 4, 4), (8, 8, 8), (12, 12, 12), (16, 16, 16)
SPECS = []


def _add(entry, cls, dims, co, ci, B, taps=27, **kw):
    """kw: builder options (a_ch, b_ch, stuff, up, strides, nnz) and launcher options -- ksplit: list of K-range counts, None = the
    wrapper's own choice, the first entry is the pass every other one must equal; prep: "v1" = md_wino_prep instead of _v2."""
    kw.setdefault("ksplit", [None])
    tag = "-".join(str(v) for v in (entry, taps, cls, "x".join(map(str, dims)), f"{co}x{ci}", f"B{B}", kw.get("tag", "")) if v != "")
    assert all(s["id"] != tag for s in SPECS), tag
    SPECS.append(dict(id=tag, entry=entry, cls=cls, dims=tuple(dims), co=co, ci=ci, B=B, taps=taps, seed=len(SPECS), **kw))


# ---- md_to_pb16 + md_wgrad, taps = 27 ------------------------------------------------------------------------------
# FULL (whole tiles, whole stages): 64 stages; 7 ranges do not divide them (10 .. 4), 48 ranges leave 16 of them empty
_add("pb", "hi_only", C8, 128, 128, 8, ksplit=[1, None, 7, 48], tag="full")
_add("pb", "a_lo", C8, 128, 128, 8, ksplit=[None, 1], tag="full")
_add("pb", "dy_lo", C8, 128, 128, 8, ksplit=[3, 1], tag="full")
_add("pb", "hi_only", C4, 256, 128, 8, ksplit=[1, None, 3])                     # S = 4: half a stage is masked
_add("pb", "a_lo", C4, 128, 256, 8, ksplit=[None, 16, 5])
_add("pb", "dy_lo", C8, 256, 256, 8, ksplit=[None, 8, 1], tag="remap")          # 8 x 36 units = 288 work items > 256: the XCD remap's second round
_add("pb", "hi_only", C8, 136, 128, 8, a_ch=136, strides="gap", ksplit=[None, 1], tag="rows136")
_add("pb", "a_lo", C8, 96, 128, 8, a_ch=128, strides="gap", tag="rows96of128")
_add("pb", "dy_lo", C8, 128, 96, 8, b_ch=96, strides="gap", tag="cols96")      # cols % 64 != 0: the generic reduce kernel
_add("pb", "hi_only", C8, 128, 4, 8, b_ch=8, strides="gap", ksplit=[None, 5], tag="stem")
_add("pb", "a_lo", C8, 4, 128, 8, a_ch=8, strides="gap", ksplit=[None, 5], tag="head")
_add("pb", "dy_lo", C4, 128, 128, 8, ksplit=[1, 16, 7])
_add("pb", "hi_only", C12, 128, 128, 8, ksplit=[None, 1, 11], tag="S12")       # S = 12: the second stage of a row has 4 positions
_add("pb", "dy_lo", C12, 128, 136, 2, b_ch=136, strides="gap", tag="S12")
_add("pb", "a_lo", C16, 128, 128, 2, ksplit=[None, 1], tag="S16")              # two whole stages per row
# z-slab virtual samples through the wrappers: zsplit 8, 8, 4, 8 (B = 11: 88 virtual samples), and Dz = 1 with a half-filled block
_add("pb", "hi_only", C8, 128, 128, 1, ksplit=[None, 1], tag="zslab")
_add("pb", "a_lo", C8, 128, 128, 3, ksplit=[None, 1, 5], tag="zslab")
_add("pb", "dy_lo", C8, 128, 128, 6, ksplit=[None, 1], tag="zslab")
_add("pb", "a_lo", C8, 128, 128, 11, ksplit=[None, 7], tag="zslab")
_add("pb", "hi_only", C4, 128, 128, 3, ksplit=[None, 1, 3], tag="zslab")       # zsplit 4, Dz = 1, 12 virtual samples: the second block half full
_add("pb", "dy_lo", C4, 136, 96, 3, a_ch=136, b_ch=96, strides="gap", tag="zslab")
# D != H
_add("pb", "hi_only", (4, 8, 8), 128, 128, 8, ksplit=[None, 1, 3])
_add("pb", "a_lo", (16, 8, 8), 128, 128, 2, ksplit=[None, 1])                   # zsplit 4, Dz = 4
_add("pb", "dy_lo", (4, 8, 8), 128, 128, 3, ksplit=[None, 1])                   # zsplit 4, Dz = 1
_add("pb", "hi_only", (2, 12, 12), 96, 128, 8, a_ch=96, strides="gap", ksplit=[None, 5])
# the stride-2 conv (dY zero-stuffed at the odd positions) and the Upsample conv (A nearest x2)
_add("pb", "a_lo", C8, 128, 128, 8, stuff=1, ksplit=[None, 1], tag="stuff")
_add("pb", "hi_only", C8, 128, 128, 3, stuff=1, tag="stuff")
_add("pb", "dy_lo", C8, 128, 128, 8, up=1, ksplit=[None, 1], tag="up")
_add("pb", "a_lo", C8, 128, 128, 6, up=1, tag="up")
# strides that are not the conv layout: dW[27][co][ci] (the generic reduce kernel on whole tiles)
_add("pb", "hi_only", C8, 128, 128, 8, strides="tapfirst", ksplit=[None, 1], tag="tapfirst")
_add("pb", "a_lo", C4, 136, 128, 8, a_ch=136, strides="tapfirst", tag="tapfirst")
# ---- taps = 125: the stem and the head of ddpm_res128, pad = 2 -----------------------------------------------------
_add("pb", "hi_only", C8, 128, 4, 8, taps=125, b_ch=8, ksplit=[None, 1, 3], tag="stem")
_add("pb", "a_lo", C8, 4, 128, 8, taps=125, a_ch=8, ksplit=[None, 1], tag="head")
_add("pb", "dy_lo", C12, 128, 4, 3, taps=125, b_ch=8, strides="gap", ksplit=[None, 1], tag="stem")
_add("pb", "hi_only", C12, 4, 128, 3, taps=125, a_ch=8, strides="gap", ksplit=[None, 5], tag="head")
_add("pb", "a_lo", C12, 128, 4, 8, taps=125, b_ch=8, tag="stem")
_add("pb", "dy_lo", C8, 4, 128, 6, taps=125, a_ch=8, tag="head")
# ---- taps = 1 ------------------------------------------------------------------------------------------------------
_add("pb", "hi_only", C8, 128, 128, 8, taps=1, ksplit=[None, 1, 7], tag="full")
_add("pb", "a_lo", C8, 256, 128, 8, taps=1, ksplit=[None, 1], tag="full")
_add("pb", "dy_lo", C8, 136, 40, 3, taps=1, a_ch=136, b_ch=40, strides="nin_gap", ksplit=[None, 1])
_add("pb", "hi_only", C4, 96, 128, 8, taps=1, a_ch=128, ksplit=[None, 3])
_add("pb", "a_lo", C12, 128, 96, 2, taps=1, b_ch=96, strides="nin_gap")
# ---- md_wino_prep_dual + md_wino_prep / _v2 + md_wgrad_wino --------------------------------------------------------
# the operand passes need W | 256 and D * H * W % 256 == 0, the kernel D, H >= 2 and W in {32, 64}: the smallest grids are
# (2, 4, 32) / (4, 2, 32) and (2, 2, 64); ksplit runs up to B (D - 1), where every range of kd != 1 owns exactly one plane
_add("wino", "hi_only", (2, 4, 32), 128, 128, 1, ksplit=[1])
_add("wino", "a_lo", (4, 2, 32), 128, 128, 2, ksplit=[1, 5, 6])
_add("wino", "dy_lo", (4, 8, 32), 128, 128, 3, ksplit=[1, None, 4, 9])
_add("wino", "hi_only", (8, 4, 32), 256, 128, 2, ksplit=[None, 1, 5, 14])
_add("wino", "a_lo", (8, 16, 32), 128, 256, 1, ksplit=[1, 3, 7])
_add("wino", "dy_lo", (8, 16, 32), 128, 128, 2, ksplit=[None, 14], prep="v1")
_add("wino", "dy_lo", (2, 2, 64), 128, 128, 3, ksplit=[1, 2, 3])
_add("wino", "hi_only", (4, 8, 64), 128, 128, 2, strides="tapfirst", ksplit=[1, 5, 6])
_add("wino", "a_lo", (8, 4, 64), 128, 128, 1, ksplit=[7, 1], prep="v1")
_add("wino", "dy_lo", (4, 8, 64), 256, 128, 1, strides="gap", ksplit=[None, 2])
_add("wino", "hi_only", (8, 4, 64), 128, 256, 3, ksplit=[None, 21, 4])
# ---- md_wgrad_nin: P = dims[2] positions; ksplit up to B P / 16 (one 16-position element per range) ------------------
_add("nin", "hi_only", (1, 1, 16), 128, 128, 1, taps=1, ksplit=[1])
_add("nin", "a_lo", (1, 1, 16), 128, 128, 3, taps=1, ksplit=[1, 2, 3])                   # one element per sample: every range boundary is a sample boundary or straddles one
_add("nin", "dy_lo", (1, 1, 48), 256, 128, 3, taps=1, ksplit=[1, 2, 4, 9])               # 3 elements per sample: 2 ranges 0-4 / 4-9, 4 ranges 0-2-4-6-9 straddle
_add("nin", "hi_only", (1, 1, 4096), 128, 256, 3, taps=1, ksplit=[None, 1, 5, 768])
_add("nin", "a_lo", (1, 1, 4096), 128, 128, 1, taps=1, ksplit=[None, 7, 256])
_add("nin", "dy_lo", (1, 1, 48), 128, 128, 1, taps=1, strides="nin_gap", ksplit=[None, 3])
# (appended, so that the seeds of the cases above stay what they are) zsplit 2: B = 4, two slabs of four planes
_add("pb", "dy_lo", C8, 128, 128, 4, ksplit=[None, 1, 7], tag="zslab")

IDS = [s["id"] for s in SPECS]


def spec_of(case_id):
    return SPECS[IDS.index(case_id)]


def domain_of(spec):
    return "wino" if spec["entry"] == "wino" else "direct"


# ---- md_wino_prep_dual alone: (B, c, dims) -- non-cubic grids at W = 8, 16, 32, 64; integers of up to 11 bits (lo planes live in T
#      and U); the channel sums stay far below 2^24
DUAL_CASES = [(3, 8, (4, 8, 8)), (3, 24, (2, 8, 16)), (3, 8, (4, 2, 32)), (3, 24, (2, 2, 64)), (3, 24, (8, 4, 16)), (3, 8, (4, 8, 32)),
              (3, 8, (2, 4, 64))]


def dual_input(B, c, dims, seed=0):
    g = torch.Generator().manual_seed(9000 + seed)
    return _randint(g, -1023, 1023, (B, c) + tuple(dims))


def t_layout(planes, B, c):
    """4 x (hi, lo) [B, c, D, H, W/2] fp32 -> int16 [B][c/8][4][2][D][H][W/2][8], the layout of T and U."""
    D, H, Wp = planes[0][0].shape[2:]
    out = torch.empty((B, c // 8, 4, 2, D, H, Wp, 8), dtype=torch.int16)
    for f, pair in enumerate(planes):
        for pl, v in enumerate(pair):
            out[:, :, f, pl] = v.to(torch.bfloat16).view(torch.int16).view(B, c // 8, 8, D, H, Wp).permute(0, 1, 3, 4, 5, 2)
    return out
