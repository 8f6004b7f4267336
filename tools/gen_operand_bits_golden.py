"""Records tests/golden/operand_bits.npz: the words the f16f6 operand passes and the f16f6 weight packer write for the inputs of
tests/operand_bits_cases.py, from the library that is built when this runs.

    python tools/gen_operand_bits_golden.py [--out tests/golden/operand_bits.npz]

Run it on the commit whose bits are the reference (the parent of a change to md_split_f16f6 or to the passes), on the GPU.  Tensors
above ~150 KB are recorded as one CRC-32 per slab (operand_bits_cases.slab_crcs); the two smallest operands and the packed
weights' header are recorded whole.  The script also checks, on the host, that every special value of the "raw" variant stands in a
block of a wave that saturates and (where the value does not itself ask for the saturation) in one that does not."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import operand_bits_cases as oc  # noqa: E402
from meshdiffusion_amd import hip_ops as ops  # noqa: E402

WHOLE = [((16, 16), (4, 8, 8))]      # operands small enough to be recorded whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "operand_bits.npz"))
    out = ap.parse_args().out
    gold = {}
    hot = {repr(float(v)) for v in oc.HOT_SPECIALS}
    for cs, dims in oc.BLOCK_CASES + oc.PLAIN_CASES:
        cov, zero = oc.raw_coverage(oc.inputs(cs, dims, "raw")["x"], dims)
        bad = [k for k, (plain, sat) in cov.items() if not sat or (not plain and k not in hot)]
        assert zero and not bad, f"{cs} {dims}: specials not covered on both paths: {bad}, all-zero block: {zero}"
    for variant in oc.VARIANTS:
        for cs, dims in oc.PLAIN_CASES:
            t = oc.run_plain(ops, cs, dims, variant)
            cid = oc.case_id(cs, dims, variant)
            gold["plain_T_crc/" + cid] = oc.slab_crcs(t, oc.t_slabs(cs))
            if (cs, dims) in WHOLE:
                gold["plain_T/" + cid] = t
        for cs, dims in oc.BLOCK_CASES:
            cid = oc.case_id(cs, dims, variant)
            t, res = oc.run_block(ops, cs, dims, variant, True, 0)
            gold["block_T_crc/" + cid] = oc.slab_crcs(t, oc.t_slabs(cs))
            gold["block_res_crc/" + cid] = oc.slab_crcs(res, oc.RES_SLABS)
            # the parent's two forms agree (tests/test_gpu_block_pass.py); a golden that they disagree on would be no reference
            t3, res3 = oc.run_block(ops, cs, dims, variant, True, 3)
            tp = oc.run_plain(ops, cs, dims, variant)
            assert np.array_equal(t, t3) and np.array_equal(res, res3) and np.array_equal(t, tp), cid
            print(cid, "T words", t.size, "res words", res.size, flush=True)
    for with_eq in (False, True):
        wpk = oc.run_weights(ops, with_eq)
        key = "eq" if with_eq else "noeq"
        gold["wpk_crc/" + key] = oc.slab_crcs(wpk[:-64], oc.WPK_SLABS)
        gold["wpk_header/" + key] = wpk[-64:]
    np.savez_compressed(out, **gold)
    print(f"wrote {out}: {len(gold)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
