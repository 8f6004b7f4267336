"""Every poisoned launch of tests/nonfinite_cases.py can fail: conditions on the float64 references alone, no GPU.
    - the reference's non-finite set is non-empty
    - at least half of the launch's outputs are finite in the reference (else "everything else is exact" would be vacuous)
    - unpoisoned samples are entirely finite
    - convolutions: at the poisoned voxel's own output position EVERY output row is non-finite (the sparse weights of the exact
      cases still give 0 * NaN = NaN in float64)
    - convolutions, GroupNorm, weight gradients: `ref` and `ref_sub` (inf -> NaN in the operand) have identical sets"""
import pytest
import torch

import attn_cases as ac
import conv_cases as cc
import nonfinite_cases as nf
import wgrad_cases as wc


def _conditions(ref, ref_sub, clean_samples, what, same_sets=True):
    b = nf.bad(ref)
    assert bool(b.any()), f"{what}: the reference has no non-finite"
    assert int(b.sum()) * 2 <= b.numel(), f"{what}: {int(b.sum())} of {b.numel()} reference values are non-finite"
    for s in clean_samples:
        assert not bool(b[s].any()) and not bool(nf.bad(ref_sub[s]).any()), f"{what}: unpoisoned sample {s} is not finite"
    if same_sets:
        assert torch.equal(b, nf.bad(ref_sub)), f"{what}: ref and ref_sub differ in their non-finite sets"


def test_selection_covers_every_direct_entry_and_form():
    pairs = {(s["entry"], s.get("cfg", "")) for s in cc.SPECS if s["entry"] not in nf.WINOGRAD}
    assert pairs == {(s["entry"], s.get("cfg", "")) for s in nf.SPECS}
    assert all(s["B"] >= 2 for s in nf.SPECS)
    assert any(s.get("prec") == "fp16x2" for s in nf.SPECS)
    assert any(s.get("b_f32") and s.get("ac") for s in nf.SPECS) and any(s.get("b_f32") and not s.get("ac") for s in nf.SPECS)
    assert {"ncdhw", "s16b"} <= {s.get("out") for s in nf.SPECS}
    assert any(s.get("ksplit") for s in nf.SPECS) and any(s.get("stats") for s in nf.SPECS)
    assert len(set(nf.IDS)) == len(nf.IDS) and all("/twin" in i for i in set(nf.IDS) - set(cc.IDS))


@pytest.mark.parametrize("case_id", nf.IDS)
def test_conv_launches_can_fail(case_id):
    case = cc.build(nf.spec_of(case_id))
    assert not bool(nf.bad(cc.reference(case)).any())
    pl = nf.places(case)
    for launch, names in (("A", ("first", "last")), ("B", ("mid",))):
        p = nf.poison(case, launch)
        assert int(nf.bad(torch.cat(p["x_raw"], 1)).sum()) == len(names) and not bool(nf.bad(p["x"][1:]).any())
        ref, ref_sub = nf.references(p)
        _conditions(ref, ref_sub, range(1, case["B"]), f"{case_id} launch {launch}")
        for n in names:
            z, y, x = nf.own_position(case, pl[n][1])
            assert bool(nf.bad(ref[0, :, z, y, x]).all()), f"{case_id} launch {launch}: a row is finite at the output position of `{n}`"
        if case["spec"].get("stats"):
            st = nf.bad(cc.reference_stats(ref))
            assert bool(st[0].all()) and not bool(st[1:].any())


def _epilogue_specs():
    bias = next(s for s in nf.SPECS if s.get("bias") == "sample")
    res = next(s for s in nf.SPECS if s.get("res") == "sample")
    return bias, res


def test_conv_epilogue_and_weight_poisons_can_fail():
    sb, sr = _epilogue_specs()
    case = cc.build(sb)
    ref, ref_sub = nf.references(nf.poison(case, ("bias", 1, 3)))
    want = torch.zeros_like(ref, dtype=torch.bool)
    want[1, 3] = True
    assert torch.equal(nf.bad(ref), want) and torch.equal(nf.bad(ref_sub), want)
    case = cc.build(sr)
    ref, _ = nf.references(nf.poison(case, ("res", 1, 3, (0, 1, 2))))
    want = torch.zeros_like(ref, dtype=torch.bool)
    want[1, 3, 0, 1, 2] = True
    assert torch.equal(nf.bad(ref), want)
    spec = next(s for s in nf.SPECS if s.get("prec") == "fp16x2")
    case = cc.build(spec)
    ref, ref_sub = nf.references(nf.poison(case, ("w", 7, 11, (0, 1, 2))))
    b = nf.bad(ref)
    bs = nf.bad(ref_sub)
    assert bool(b[:, 7].any()) and not bool(bs[:, :7].any()) and not bool(bs[:, 8:].any()) and bool(bs[:, 7].all())
    # the tap (0, 1, 2) leaves the grid at the z = 0 and x = W - 1 faces: `ref` is finite there (an absent term), `ref_sub` is not
    assert not bool(b[:, 7, 0].any()) and not bool(b[:, 7, :, :, -1].any()) and bool(b[:, 7, 1:, :, :-1].all())
    assert int(bs.sum()) * 2 <= bs.numel()


@pytest.mark.parametrize("grid", nf.GN_GRIDS)
@pytest.mark.parametrize("two_parts", [False, True])
def test_groupnorm_launches_can_fail(grid, two_parts):
    case = nf.gn_case(grid, two_parts)
    assert case["c0"] >= (case["parts"][0] if two_parts else 0)
    for name, value in nf.GN_VALUES.items():
        for last in (False, True):
            p = nf.gn_poison(case, value, last)
            ref = nf.gn_reference(p)
            if name == "1e30":
                assert not bool(nf.bad(ref).any())
                continue
            ref_sub = nf.gn_reference(dict(p, x=nf.nan_sub(p["x"])))
            _conditions(ref, ref_sub, [1], f"GroupNorm {grid} {name}")
            assert torch.equal(nf.bad(ref), nf.gn_group_mask(p)), "one non-finite voxel poisons exactly its (sample, group)"


@pytest.mark.parametrize("nk,nq,B", nf.SOFTMAX_SHAPES)
def test_softmax_launches_can_fail(nk, nq, B):
    s = nf.softmax_logits(nk, nq, B)
    for name, items in nf.softmax_poisons(nk, nq):
        ref = torch.softmax(nf.softmax_apply(s, items).double(), dim=1)
        cols = sorted({q for _, q, _ in items})
        b = nf.bad(ref)
        if name == "some_ninf":
            assert not bool(b.any())
            for k, q, _ in items:
                assert float(ref[0, k, q]) == 0.0
        else:
            want = torch.zeros_like(b)
            want[0, :, cols] = True
            assert torch.equal(b, want), name
            assert int(b.sum()) * 2 <= b.numel()


@pytest.mark.parametrize("name", list(nf.ATTN_CASES))
def test_attention_launches_can_fail(name):
    case = nf.ATTN_CASES[name]()
    assert ac.bf16_exact(case["q"]) and ac.bf16_exact(case["k"]) and ac.bf16_exact(case["v"])
    for pname, operand, where, value in nf.attn_poisons(case["N"]):
        ref, ref_sub = nf.attn_references(nf.attn_apply(case, operand, where, value))
        what = f"{name} {pname}"
        assert not bool(nf.bad(ref[1:]).any()) and not bool(nf.bad(ref_sub[1:]).any()), what
        assert torch.equal(nf.bad(ref_sub), nf.attn_expected(case, operand, where)), what
        assert bool(nf.bad(ref_sub).any()) and int(nf.bad(ref_sub).sum()) * 2 <= ref.numel(), what
        if value != value:
            assert torch.equal(nf.bad(ref), nf.bad(ref_sub)), what
        else:
            assert not bool((nf.bad(ref) & ~nf.bad(ref_sub)).any()), what          # ref's set lies inside ref_sub's


def test_loss_launches_can_fail():
    case = nf.loss_case()
    for masked_in in (True, False):
        p = nf.loss_poison(case, masked_in)
        assert float(p["mask"][(0, 0) + p["vox"]]) == (1.0 if masked_in else 0.0)
        sums, grad = nf.loss_reference(p)
        assert bool(nf.bad(sums[0])) and not bool(nf.bad(sums[1:]).any())          # 0 * NaN = NaN: the mask is a factor, not a select
        want = torch.zeros_like(grad, dtype=torch.bool)
        want[(0, 2) + p["vox"]] = True
        assert torch.equal(nf.bad(grad), want)


@pytest.mark.parametrize("entry", ["pb", "wino", "nin"])
def test_wgrad_launches_can_fail(entry):
    case = wc.build(nf.wgrad_spec(entry))
    assert case["B"] >= 2
    p = nf.wgrad_poison(case, "dy")
    ref, ref_sub = nf.references(p)
    want = torch.zeros_like(ref, dtype=torch.bool)
    want[5] = True
    assert torch.equal(nf.bad(ref), want) and torch.equal(nf.bad(ref_sub), want)
    p = nf.wgrad_poison(case, "act")
    ref, ref_sub = nf.references(p)
    b = nf.bad(ref)
    assert torch.equal(b, nf.bad(ref_sub)) and bool(b[:, 9].any()) and not bool(b[:, :9].any()) and not bool(b[:, 10:].any())
    reach = b[0, 9]
    assert bool((b[:, 9] == reach[None]).all()) and int(reach.sum()) == (1 if case["taps"] == 1 else 8)
    assert int(b.sum()) * 2 <= b.numel()
    if entry == "pb":
        ref, ref_sub = nf.references(nf.wgrad_poison(case, "act_row_end"))
        b = nf.bad(ref)
        assert torch.equal(b, nf.bad(ref_sub)) and int(b[0, 9].sum()) == 8 and not bool(b[0, 9].reshape(3, 3, 3)[:, :, 0].any())     # dx = -1 never reaches x = W - 1
