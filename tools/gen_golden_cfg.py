"""Writes tests/golden/cfg.npz on the CPU: the bars of the guidance-rescale test of tests/test_gpu_cfg.py -- for every case of
tests/cfg_cases.py the distance of the float32 restatement of the per-sample factor from its float64 restatement, times
cfg_cases.BAR_MARGIN -- and the state-dict keys / parameter names of the small class-less U-Net (synth.small_config) as they were
before class conditioning existed.  The name lists are kept from the existing file when there is one: they pin what
model.num_classes = 0 must go on producing, so they are not re-derived from the code they check.

    python tools/gen_golden_cfg.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cfg_cases as cc  # noqa: E402


def small_unet_names():
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    cfg = synth.small_config()
    cfg.device = torch.device("cpu")
    cfg.model.num_classes = 0
    m = mutils.create_model(cfg, use_parallel=False)
    return list(m.state_dict().keys()), [n for n, _ in m.named_parameters()]


def main():
    path = os.path.join(ROOT, "tests", "golden", "cfg.npz")
    out = {}
    if os.path.exists(path):
        old = np.load(path)
        out.update({k: old[k] for k in ("unet_small_keys", "unet_small_params") if k in old})
    if "unet_small_keys" not in out:
        keys, params = small_unet_names()
        out["unet_small_keys"], out["unet_small_params"] = np.array(keys), np.array(params)
    for B in cc.BATCHES:
        for n in cc.SIZES + cc.SIZES_UNALIGNED:
            ec, eu, w = cc.combine_inputs(B, n)
            o = cc.combine_restated(ec, eu, w).astype(np.float32)
            for phi in cc.PHIS:
                bar = cc.rescale_bar(ec, o, phi)
                out[f"rescale/{cc.case_id(B, n)}/phi{phi}/bar"] = np.float64(bar)
                print(f"rescale {cc.case_id(B, n)} phi {phi}: w {w.tolist()} bar {bar:.3e}")
    np.savez(path, **out)
    print(f"wrote {path}: {len(out)} entries, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
