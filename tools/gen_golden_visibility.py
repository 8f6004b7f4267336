"""Generate tests/golden/visibility.npz (build host only, CPU, seeded):
    python tools/gen_golden_visibility.py

  init/<case>/unsure_share    per case of tests/visibility_cases.py INIT_CASES: the share of grid vertices whose decision in
                      `init_with_gt_surface` is ill-conditioned in fp32 (two centres tie within NN_GAP and decide differently, or the
                      distance to the face's plane or the flip of its normal is below DOT_GAP), from the float64 restatement alone.
                      The GPU test leaves these vertices out; each share must stay at most raster_cases.EXCLUDE_CAP (0.5 %), checked
                      here.
  init/<case>/outside_share   the share of vertices the float64 restatement sets to 1.0 (a case where all or none are set tests
                      nothing).
  init/<case>/fp32_differs    the number of vertices outside the ill-conditioned set where the fp32 torch restatement decides
                      differently from float64: the bar of the GPU test is 0, and the restatement in fp32 meets it here.
  init/nn_gap, init/dot_gap   the gaps.
The file holds only such numbers.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raster_cases as rc  # noqa: E402
import visibility_cases as vc  # noqa: E402


def main():
    out = {"init/nn_gap": np.float64(vc.NN_GAP), "init/dot_gap": np.float64(vc.DOT_GAP)}
    for name in vc.INIT_CASES:
        v_pos, gt_verts, faces, campos = vc.init_case(name)
        r64 = vc.init_with_gt_surface_restated(v_pos, gt_verts, faces, campos, torch.float64)
        r32 = vc.init_with_gt_surface_restated(v_pos, gt_verts, faces, campos, torch.float32)
        N = v_pos.shape[0]
        share = float(r64["unsure"].sum()) / N
        differs = int(((r32["outside"] != r64["outside"]) & ~r64["unsure"]).sum())
        out[f"init/{name}/unsure_share"] = np.float64(share)
        out[f"init/{name}/outside_share"] = np.float64(float(r64["outside"].sum()) / N)
        out[f"init/{name}/fp32_differs"] = np.int64(differs)
        print(f"[visibility] init {name}: N {N} visible faces {faces.shape[0]} set to 1.0 {int(r64['outside'].sum())} ill-conditioned "
              f"{int(r64['unsure'].sum())} ({share:.5f}) fp32 restatement differs on {int((r32['outside'] != r64['outside']).sum())}, "
              f"outside the ill-conditioned set on {differs}")
        assert share <= rc.EXCLUDE_CAP, (name, share)
        assert differs == 0, (name, differs)
    path = os.path.join(rc.GOLD, "visibility.npz")
    np.savez_compressed(path, **out)
    print(f"[visibility] wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
