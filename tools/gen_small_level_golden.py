"""Records tests/golden/small_level_bits.npz: the words md_gemm_conv writes for the cases of tests/small_level_cases.py (the 4^3-level
conv with the GroupNorm loader and split-K, the MD_CFG_G1_128 GEMM with F32B output), from the library that is built when this runs.

    python tools/gen_small_level_golden.py [--out tests/golden/small_level_bits.npz]

Run it on the GPU, on a commit whose md_gemm_conv serves these launches with the generic tile alone: the file is the reference the
dedicated small-level kernels are held to, so the script refuses a library that contains them.  Every output is recorded as one
CRC-32 per (sample, 8-channel group) slab; the smallest outputs are recorded whole as well."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import small_level_cases as sc  # noqa: E402
from meshdiffusion_amd import _lib, hip_ops as ops  # noqa: E402

NEW_KERNELS = (b"md_conv3_low_kernel", b"md_gemm_stream_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "small_level_bits.npz"))
    out = ap.parse_args().out
    _lib.load()
    blob = open(_lib.LIB_PATH, "rb").read()
    found = [n.decode() for n in NEW_KERNELS if n in blob]
    assert not found, f"{_lib.LIB_PATH} contains {found}: record the golden on the commit before the dedicated kernels"
    gold = {}
    for cid, case in sc.CASES.items():
        host = sc.build(case)
        words = sc.run(ops, case, host)
        again = sc.run(ops, case, host)
        assert np.array_equal(words, again), f"{cid}: the same launch twice differs"
        assert not np.isnan(words.view(np.float32)).any(), f"{cid}: an output word was not written"
        gold["crc/" + cid] = sc.slab_crcs(words)
        if words.nbytes <= sc.WHOLE_BYTES:
            gold["whole/" + cid] = words
        print(cid, "words", words.size, flush=True)
    np.savez_compressed(out, **gold)
    print(f"wrote {out}: {len(gold)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
