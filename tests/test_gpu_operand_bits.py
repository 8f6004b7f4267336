"""The f16f6 operand passes and the f16f6 weight packer, bit for bit against RECORDED words (tests/golden/operand_bits.npz, written
by tools/gen_operand_bits_golden.py on the commit before md_split_f16f6 took its wave-uniform saturation branch and the block pass
its DPP neighbours): T as int16, the shortcut `res` and the packed weights as int32, through md_wino_prep_f6, md_wino_prep_f6_nin
(with and without the NIN weights, n_cu 0 and 3) and md_wino_pack_weights_f6.  Shapes, values and the coverage of the split's two
paths: tests/operand_bits_cases.py.  Tensors recorded as slab CRCs are compared as such; a failure names the (sample, channel
group) slabs that differ."""
import os

import numpy as np
import pytest
import torch

import operand_bits_cases as oc


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from meshdiffusion_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, "operand_bits.npz"))


def _check_crcs(words, ref, n_slabs, what):
    assert words.size % n_slabs == 0 and ref.shape == (n_slabs,), f"{what}: {words.size} words, {ref.shape} recorded slabs"
    got = oc.slab_crcs(words, n_slabs)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {n_slabs} slabs differ from the recorded words, first slabs {bad[:8].tolist()}"


_ID = lambda c: f"{c[0][0]}+{c[0][1]}@{'x'.join(map(str, c[1]))}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", oc.VARIANTS)
@pytest.mark.parametrize("case", oc.PLAIN_CASES, ids=_ID)
def test_plain_pass_writes_the_recorded_words(ops, gold, case, variant):
    cs, dims = case
    cid = oc.case_id(cs, dims, variant)
    t = oc.run_plain(ops, cs, dims, variant)
    if "plain_T/" + cid in gold.files:
        ref = gold["plain_T/" + cid]
        assert t.shape == ref.shape
        bad = np.nonzero(t != ref)[0]
        assert bad.size == 0, f"{cid}: {bad.size} of {t.size} int16 words of T differ, first at {bad[:8].tolist()}"
    _check_crcs(t, gold["plain_T_crc/" + cid], oc.t_slabs(cs), f"md_wino_prep_f6 {cid}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", oc.VARIANTS)
@pytest.mark.parametrize("case", oc.BLOCK_CASES, ids=_ID)
def test_plain_pass_on_the_block_shapes(ops, gold, case, variant):
    """md_wino_prep_f6 on the block pass's shapes: the parent wrote the same T through either kernel, so one record serves both."""
    cs, dims = case
    cid = oc.case_id(cs, dims, variant)
    _check_crcs(oc.run_plain(ops, cs, dims, variant), gold["block_T_crc/" + cid], oc.t_slabs(cs), f"md_wino_prep_f6 {cid}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_cu", [0, 3])
@pytest.mark.parametrize("with_nin", [True, False], ids=["nin", "operand-only"])
@pytest.mark.parametrize("variant", oc.VARIANTS)
@pytest.mark.parametrize("case", oc.BLOCK_CASES, ids=_ID)
def test_block_pass_writes_the_recorded_words(ops, gold, case, variant, with_nin, n_cu):
    cs, dims = case
    cid = oc.case_id(cs, dims, variant)
    t, res = oc.run_block(ops, cs, dims, variant, with_nin, n_cu)
    what = f"md_wino_prep_f6_nin {cid} {'with' if with_nin else 'without'} weights, n_cu {n_cu}"
    _check_crcs(t, gold["block_T_crc/" + cid], oc.t_slabs(cs), what + ": T")
    if with_nin:
        _check_crcs(res, gold["block_res_crc/" + cid], oc.RES_SLABS, what + ": res")
    else:
        assert res is None


@pytest.mark.gpu
@pytest.mark.parametrize("with_eq", [False, True], ids=["noeq", "eq"])
def test_weight_packer_writes_the_recorded_words(ops, gold, with_eq):
    key = "eq" if with_eq else "noeq"
    wpk = oc.run_weights(ops, with_eq)
    assert np.array_equal(wpk[-64:], gold["wpk_header/" + key]), "the packed weights' header differs"
    _check_crcs(wpk[:-64], gold["wpk_crc/" + key], oc.WPK_SLABS, f"md_wino_pack_weights_f6 ({key})")


def test_every_special_stands_on_both_paths_of_the_split():
    """Host only: in the "raw" inputs every special value stands in a 16-channel block that asks for the fp16 saturation and -- unless
    the value asks for it itself -- in a block of a region none of whose waves saturates; and there is an all-zero block."""
    hot = {repr(float(v)) for v in oc.HOT_SPECIALS}
    for cs, dims in oc.BLOCK_CASES + oc.PLAIN_CASES:
        cov, zero = oc.raw_coverage(oc.inputs(cs, dims, "raw")["x"], dims)
        assert zero, f"{cs} {dims}: no all-zero block"
        for name, (plain, sat) in cov.items():
            assert sat, f"{cs} {dims}: {name} stands in no saturating block"
            assert plain or name in hot, f"{cs} {dims}: {name} stands in no block of a calm region"
