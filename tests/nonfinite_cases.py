"""Poisoned launches of the exact-input cases (tests/conv_cases.py, tests/wgrad_cases.py, tests/attn_cases.py) and of small
GroupNorm / softmax / loss inputs, their float64 references and the one check all of them share.  Plain helper module: no
fixtures, no GPU, only torch.  tests/test_gpu_nonfinite_kernels.py launches them on the GPU; tests/test_cpu_nonfinite_cases.py
proves on the CPU that every poisoned launch can fail (the reference has a non-finite set, most of the launch stays finite,
unpoisoned samples are finite).

The contract (rules R1 - R4 of tests/test_gpu_nonfinite.py, sharpened).  `ref` is the float64 reference of the poisoned
operands, "non-finite" = NaN or +-inf (not told apart):
    hidden    every non-finite position of `ref` is non-finite in the output                                   (R2)
    invented  every non-finite position of the output is non-finite in `ref_sub`                              (R1 / R3)
    the rest  torch.equal with ref.float() on exact cases; otherwise bit-identical to the clean launch where that computes
              the same value, or within the tolerance of the kernel's existing finite test
    R4        a sample (GroupNorm: a group) that holds no poison is bit-identical to the clean launch
`ref_sub` is the reference after +-inf in the poisoned operand is replaced by NaN: md_split maps inf to (hi = inf,
lo = inf - inf = NaN), so for a bf16x3 (or fp16x2) contraction an inf operand IS a NaN operand.  For the convolutions,
GroupNorm and the weight gradients both references have the same non-finite set (0 * inf is NaN in float64 as well, and the
exact cases multiply every reached voxel by a weight, zero or not); for an inf in K of attention they differ: a logit of
-inf keeps a query finite in float64 (p = 0), and the kernel cannot.  No dilation is allowed: none of these kernels reads a
neighbour of the poisoned voxel that the reference does not."""
import copy

import torch
import torch.nn.functional as F

import attn_cases as ac
import conv_cases as cc
import wgrad_cases as wc

NAN, INF = float("nan"), float("inf")


def bad(t):
    return ~torch.isfinite(t)


def nan_sub(t):
    """+-inf -> NaN (what md_split makes of an inf operand)."""
    return torch.where(torch.isinf(t), torch.full_like(t, NAN), t)


# ---------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------
def _first(mask, names):
    idx = mask.nonzero()[0].tolist()
    return "(" + ", ".join(names[:len(idx)]) + f") = {tuple(idx)}"


def check(out, ref, ref_sub, clean_out=None, clean_samples=(), what="", exact=True, tol=None, same_as_clean=None,
          names=("b", "row", "d", "h", "w")):
    """out: fp32 on the CPU, shaped like ref / ref_sub (float64).  clean_out: the clean launch of the same case;
    clean_samples: first-dimension indices that hold no poison (R4: bit-identical to clean_out).
    exact: finite values must be torch.equal to ref.float().  Otherwise `same_as_clean` (bool mask: positions where the
    clean launch computes the same value) must be bit-identical to clean_out, and what is left must lie within `tol`
    (max |out - ref| / max |ref| over the finite positions) -- the caller names the existing test `tol` is taken from.
    Prints and returns the sizes of the three sets (hidden, invented, compared); messages name the first offending position."""
    assert out.shape == ref.shape == ref_sub.shape, (what, out.shape, ref.shape, ref_sub.shape)
    out = out.detach().cpu()
    b_out, b_ref, b_sub = bad(out), bad(ref), bad(ref_sub)
    hidden, invented = b_ref & ~b_out, b_out & ~b_sub
    compared = ~b_out & ~b_ref
    n = (int(hidden.sum()), int(invented.sum()), int(compared.sum()))
    print(f"{what}: hidden {n[0]} of {int(b_ref.sum())} non-finite reference positions, invented {n[1]} of {int(b_out.sum())} "
          f"non-finite outputs, compared {n[2]} of {out.numel()}")
    assert n[0] == 0, f"{what}: {n[0]} hidden non-finites (R2), first at {_first(hidden, names)}: got {out[hidden][0].item()!r}"
    assert n[1] == 0, f"{what}: {n[1]} invented non-finites (R1 / R3), first at {_first(invented, names)}: reference {ref[invented][0].item()!r}"
    if exact:
        wrong = compared & (out != ref.float())
        assert not bool(wrong.any()), (f"{what}: {int(wrong.sum())} finite outputs differ from float64, first at {_first(wrong, names)}: "
                                       f"got {out[wrong][0].item()!r} want {ref[wrong][0].item()!r}")
    else:
        if same_as_clean is not None:
            wrong = same_as_clean & ~b_out & (out != clean_out)
            assert not bool((same_as_clean & b_out).any()), f"{what}: non-finite where the clean launch computes the same value"
            assert not bool(wrong.any()), (f"{what}: {int(wrong.sum())} outputs differ from the clean launch of the same values, first at "
                                           f"{_first(wrong, names)}: got {out[wrong][0].item()!r} clean {clean_out[wrong][0].item()!r}")
        if tol is not None and bool(compared.any()):
            scale = ref[compared].abs().max().clamp_min(1e-300)
            err = (out.double() - ref).abs()
            err[~compared] = 0
            assert float(err.max() / scale) <= tol, (f"{what}: finite outputs {float(err.max() / scale):.3e} beyond {tol:.1e}, worst at "
                                                     f"{_first(err == err.max(), names)}")
    for b in clean_samples:
        assert not bool(b_ref[b].any()), f"{what}: the reference of unpoisoned sample {b} is not finite"
        wrong = ~(out[b] == clean_out[b])
        assert not bool(wrong.any()), f"{what}: R4: unpoisoned sample {b} differs from the clean launch at {_first(wrong, names[1:])}"
    return n


def check_stats(stats, ref, clean_stats, what=""):
    """The fused GroupNorm sums [B, rows, 2] of a poisoned launch: a (sample, row) entry is non-finite iff the reference's is, and
    every other entry equals the clean launch's (such a row holds no poison at all)."""
    stats, clean_stats = stats.detach().cpu(), clean_stats.detach().cpu()
    want = bad(cc.reference_stats(ref))
    got = bad(stats)
    print(f"{what}: statistics: {int(want.sum())} non-finite entries in the reference, {int(got.sum())} in the output of {want.numel()}")
    assert torch.equal(got, want), f"{what}: statistics non-finite at {_first(got ^ want, ('b', 'row', 'which'))} differ from the reference's set"
    wrong = ~want & (stats != clean_stats)
    assert not bool(wrong.any()), f"{what}: finite statistics differ from the clean launch at {_first(wrong, ('b', 'row', 'which'))}"


# ---------------------------------------------------------------------------------------------------------------
# convolutions: the selected specs, the poison places, the launches
# ---------------------------------------------------------------------------------------------------------------
WINOGRAD = ("wino", "wino_f8", "wino_f6", "wino_dgrad_f6")


def _size(s):
    D, H, W = s["dims"]
    return s["B"] * sum(s["parts"]) * s["cout"] * D * H * W


def _select():
    """The smallest spec of every (entry, cfg) pair of conv_cases.SPECS other than the Winograd entries, B >= 2 preferred (a pair
    with B = 1 specs only gets the B = 2 twin of its smallest one); within a pair one spec per operand / output form as well
    (b_f32 with and without `ac`, fp16x2, ncdhw / s16b output, split-K, upsampling), so that every loader and epilogue is met."""
    groups = {}
    for s in cc.SPECS:
        if s["entry"] in WINOGRAD or s.get("ref_rows"):
            continue
        key = (s["entry"], s.get("cfg", ""), bool(s.get("b_f32")), bool(s.get("ac")), s.get("prec", ""), s.get("out", "f32b"),
               bool(s.get("ksplit")), bool(s.get("ups")))
        groups.setdefault(key, []).append(s)
    out = []
    for key, specs in groups.items():
        multi = [s for s in specs if s["B"] >= 2]
        if multi:
            out.append(min(multi, key=_size))
        else:
            twin = copy.deepcopy(min(specs, key=_size))
            twin.update(B=2, id=twin["id"].replace("-B1", "-B2") + "/twin")
            out.append(twin)
    return out


SPECS = _select()
IDS = [s["id"] for s in SPECS]
LAUNCHES = ("A", "B")           # A: NaN at `first` and +inf at `last`; B: -inf at `mid`; the clean launch is the built case itself


def spec_of(case_id):
    return SPECS[IDS.index(case_id)]


def places(case):
    """{name: (channel of the concatenated input, (z, y, x) on the INPUT grid)}, always in sample 0."""
    D, H, W = case["din"]
    return {"first": (0, (0, 0, 0)), "last": (case["cin"] - 1, (D - 1, H - 1, W - 1)), "mid": (case["cin"] // 2, (D // 2, H // 2, W // 2))}


def _set_input(case, ch, vox, value, b=0):
    """Writes `value` into the raw tensor the kernel is given and rebuilds the logical input (raw * gain + offset)."""
    raw = torch.cat(case["x_raw"], 1)
    raw[(b, ch) + tuple(vox)] = value
    parts = [t.shape[1] for t in case["x_raw"]]
    case["x_raw"] = [t.contiguous() for t in torch.split(raw, parts, dim=1)]
    if case["ac"] is not None:
        case["x"] = (raw * case["ac"][:, :, 0, None, None, None] + case["ac"][:, :, 1, None, None, None]).contiguous()
    else:
        case["x"] = raw.contiguous()


def _clone(case):
    out = dict(case)
    for k in ("x", "w", "w_eff", "bias", "res", "ac"):
        out[k] = None if case[k] is None else case[k].clone()
    out["x_raw"] = [t.clone() for t in case["x_raw"]]
    return out


def poison(case, launch):
    """The poisoned copy of a built conv case.  launch: "A" | "B", or ("bias", b, row) | ("res", b, row, (z, y, x)) |
    ("w", co, ci, (kd, kh, kw)) for a NaN in the epilogue operands or in the weights."""
    out = _clone(case)
    pl = places(case)
    if launch == "A":
        _set_input(out, *pl["first"], NAN)
        _set_input(out, *pl["last"], INF)
    elif launch == "B":
        _set_input(out, *pl["mid"], -INF)
    elif launch[0] == "bias":
        out["bias"][launch[1], launch[2]] = NAN
    elif launch[0] == "res":
        out["res"][(launch[1], launch[2]) + tuple(launch[3])] = NAN
    elif launch[0] == "w":
        _, co, ci, tap = launch
        assert not case["spec"].get("dgrad")
        assert case["stride"] == 1 and not case["ups"]
        out["w_clean"], out["w_poison"] = case["w_eff"], (co, tuple(tap))
        out["w_eff"][(co, ci) + tuple(tap)] = NAN
        out["w"] = out["w_eff"].clone()
    else:
        raise ValueError(launch)
    return out


def references(case):
    """(ref, ref_sub) of a poisoned case: conv_cases.reference / wgrad_cases.reference on the poisoned tensors, and on them with
    +-inf replaced by NaN.
    A poisoned WEIGHT tap: where the tap leaves the grid the answer depends on whether padding is a multiplied zero (0 * NaN = NaN,
    what F.conv3d computes) or an absent term (the clean value), and neither is wrong: `ref` takes the absent term there and
    `ref_sub` the multiplied zero, so that row is non-finite wherever the tap reaches the grid, may be either at that rim, and a
    finite value there must be the clean one."""
    sub = dict(case)
    if "w_eff" in case:
        sub.update(x=nan_sub(case["x"]), w_eff=nan_sub(case["w_eff"]))
        ref, ref_sub = cc.reference(case), cc.reference(sub)
        if "w_poison" in case:
            co, (kd, kh, kw) = case["w_poison"]
            reach = cc._shift(torch.ones(case["dims"]), kd - 1, kh - 1, kw - 1) != 0
            clean = cc.reference(dict(case, w_eff=case["w_clean"]))
            ref[:, co] = torch.where(reach, ref[:, co], clean[:, co])
        return ref, ref_sub
    sub.update(a=nan_sub(case["a"]), dy=nan_sub(case["dy"]))
    return wc.reference(case), wc.reference(sub)


def own_position(case, vox):
    """The output voxel that reads input voxel `vox` through the centre (stride 2: a) tap."""
    if case["stride"] == 2:
        return tuple(v // 2 for v in vox)
    return tuple(2 * v for v in vox) if case["ups"] else tuple(vox)


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm forward
# ---------------------------------------------------------------------------------------------------------------
GN_C, GN_GROUPS, GN_EPS = 64, 32, 1e-6
GN_GRIDS = ((4, 4, 4), (3, 5, 7))
GN_VALUES = {"nan": NAN, "pinf": INF, "ninf": -INF, "1e30": 1e30}


def gn_case(grid, two_parts, seed=0):
    """x [2, 64, grid] (channels 48.. are the second part when `two_parts`), gamma, beta; the poisoned channel c0 lies in the
    second part of a two-part input."""
    g = torch.Generator().manual_seed(300 + seed)
    x = torch.randn((2, GN_C) + tuple(grid), generator=g) * 1.5 + 0.3
    gamma = 1 + 0.2 * torch.randn(GN_C, generator=g)
    beta = 0.1 * torch.randn(GN_C, generator=g)
    parts = [48, 16] if two_parts else [GN_C]
    return dict(x=x, gamma=gamma, beta=beta, parts=parts, grid=tuple(grid), c0=53 if two_parts else 21)


def gn_poison(case, value, last):
    x = case["x"].clone()
    D, H, W = case["grid"]
    vox = (D - 1, H - 1, W - 1) if last else (0, 0, 0)
    x[(0, case["c0"]) + vox] = value
    return dict(case, x=x, vox=vox)


def gn_reference(case, silu=True):
    y = F.group_norm(case["x"].double(), GN_GROUPS, case["gamma"].double(), case["beta"].double(), eps=GN_EPS)
    return F.silu(y) if silu else y


def gn_group_mask(case):
    """bool like x: the (sample 0, group of c0) block."""
    m = torch.zeros_like(case["x"], dtype=torch.bool)
    cpg = GN_C // GN_GROUPS
    g0 = case["c0"] // cpg
    m[0, g0 * cpg:(g0 + 1) * cpg] = True
    return m


# ---------------------------------------------------------------------------------------------------------------
# softmax over keys on raw fp32 logits
# ---------------------------------------------------------------------------------------------------------------
SOFTMAX_SHAPES = ((8, 32, 1), (40, 32, 2), (264, 32, 1))          # (n_keys, n_q, B) of test_softmax_keys_uneven_key_slices


def softmax_logits(nk, nq, B):
    g = torch.Generator().manual_seed(nk)
    return (torch.randn(B, nk, nq, generator=g, dtype=torch.float64) * 6).float()


def softmax_poisons(nk, nq):
    """[(name, [(key, query, value), ..])] in sample 0.  md_softmax_keys gives key block kb (8 keys) to key slice kb % 4 and the
    keys 4 half .. 4 half + 3 of a block to lane `half` of the query's lane pair: key 0 lies in the first slice and half 0, key
    `last` in the last slice that has keys and half 1."""
    first, last = 0, (min(nk // 8, 4) - 1) * 8 + 7
    return [
        ("some_ninf", [(first, 3, -INF), (last, 3, -INF), (nk - 1, 19, -INF)]),
        ("all_ninf", [(k, 5, -INF) for k in range(nk)] + [(k, 21, -INF) for k in range(nk)]),
        ("one_pinf", [(first, 7, INF), (last, 23, INF)]),
        ("one_nan", [(last, 9, NAN), (first, 25, NAN)]),
    ]


def softmax_apply(s, items):
    s = s.clone()
    for k, q, v in items:
        s[0, k, q] = v
    return s


# ---------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------
ATTN_CASES = {"dominant-N128-B3": lambda: ac.dominant_key(128, 3), "plateau_spike-N128-B2": lambda: ac.plateau_spike(128, 2, double=False),
              "rising-N1024-B3": lambda: ac.rising_staircase(1024, 3)}


def attn_poisons(N):
    """[(name, operand, (channel, position), value)]: key0 in the first and in the last tile, i0 in lane half 0 (in-tile offset 3)
    and in half 1 (offset 30), as attn_cases.plateau_spike places its spikes."""
    first, last = 5, N - ac.AT_TK + 30
    i_h0, i_h1 = ac.AT_QW + 3, N - ac.AT_QW + 30
    out = []
    for tag, key0, i0 in (("first", first, i_h0), ("last", last, i_h1)):
        out += [(f"q_nan_{tag}", "q", (17, i0), NAN), (f"v_nan_{tag}", "v", (40, key0), NAN), (f"k_nan_{tag}", "k", (2, key0), NAN),
                (f"k_pinf_{tag}", "k", (2, key0), INF), (f"k_ninf_{tag}", "k", (2, key0), -INF)]
    return out


def attn_apply(case, operand, where, value):
    out = dict(case)
    out[operand] = case[operand].clone()
    out[operand][(0,) + tuple(where)] = value
    return out


def attn_reference(case):
    """float64 [B, C, N] from q, k, v, bias as they are (the exact cases' operands are bf16-exact: the kernels read the same)."""
    return torch.stack([ac.attention64(ac.logits64(case["q"][b], case["k"][b]), case["v"][b], case["bias"])[0] for b in range(case["B"])])


def attn_references(case):
    sub = dict(case, q=nan_sub(case["q"]), k=nan_sub(case["k"]), v=nan_sub(case["v"]))
    return attn_reference(case), attn_reference(sub)


def attn_expected(case, operand, where):
    """bool [B, C, N]: the set a NaN at `where` of `operand` (sample 0) must make non-finite."""
    m = torch.zeros((case["B"], ac.AT_C, case["N"]), dtype=torch.bool)
    if operand == "q":
        m[0, :, where[1]] = True
    elif operand == "v":
        m[0, where[0], :] = True
    else:
        m[0] = True
    return m


# ---------------------------------------------------------------------------------------------------------------
# masked squared error (the training loss)
# ---------------------------------------------------------------------------------------------------------------
def loss_case():
    """The shape of test_perturb_bit_exact_and_masked_loss: B = 3, 4 channels, 8^3, a 30 % mask."""
    r = lambda seed: torch.randn((3, 4, 8, 8, 8), generator=torch.Generator().manual_seed(seed))
    mask = (torch.rand(1, 1, 8, 8, 8, generator=torch.Generator().manual_seed(4)) < 0.3).float()
    return dict(eh=r(3), noise=r(2), mask=mask, gscale=0.5)


def loss_poison(case, masked_in):
    """NaN in eps_hat of sample 0, channel 2, at the first voxel whose mask is 1 (`masked_in`) or 0."""
    vox = (case["mask"][0, 0] == (1.0 if masked_in else 0.0)).nonzero()[0].tolist()
    eh = case["eh"].clone()
    eh[(0, 2) + tuple(vox)] = NAN
    return dict(case, eh=eh, vox=tuple(vox))


def loss_reference(case):
    """The float64 expression of oracle/unet_oracle.py's loss, sum((eps_hat - noise)^2 * mask) per sample, and its gradient."""
    eh, noise, mask = case["eh"].double(), case["noise"].double(), case["mask"].double()
    sums = (torch.square(eh - noise) * mask).reshape(eh.shape[0], -1).sum(-1)
    return sums, case["gscale"] * 2 * (eh - noise) * mask


# ---------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------
def wgrad_spec(entry):
    """The smallest spec of wgrad_cases.SPECS for md_wgrad with 27 taps ("pb"), md_wgrad_wino ("wino") or md_wgrad_nin ("nin") that has
    B >= 2, the plain dW layout and (27 taps) a grid with an interior voxel."""
    specs = [s for s in wc.SPECS if s["entry"] == entry and s["taps"] == (1 if entry == "nin" else 27) and not s.get("stuff") and not s.get("up")
             and s["B"] >= 2 and "strides" not in s and (entry == "nin" or min(s["dims"]) >= 3)]
    return min(specs, key=lambda s: s["B"] * s["co"] * s["ci"] * s["dims"][0] * s["dims"][1] * s["dims"][2])


def wgrad_poison(case, which):
    """which = "dy": NaN in dy[0, co0, interior voxel] (at least one voxel from every face where the grid allows it: at a face the
    answer depends on whether padding is a multiplied zero or an absent term, and neither is wrong) -> dW[co0, :, :];
    which = "act": NaN in act[0, ci0, corner voxel] -> dW[:, ci0, the taps that reach it];
    which = "act_row_end": the same at the last voxel of the first row, (0, 0, W - 1)."""
    out = dict(case, a=case["a"].clone(), dy=case["dy"].clone())
    D, H, W = case["dims"]
    if which == "dy":
        vox = (min(1, D - 1), min(1, H - 1), W // 2)
        out["dy"][(0, 5) + vox] = NAN
    elif which == "act":
        out["a"][0, 9, 0, 0, 0] = NAN
    else:
        assert which == "act_row_end"
        out["a"][0, 9, 0, 0, W - 1] = NAN
    return out
