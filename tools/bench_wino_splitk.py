#!/usr/bin/env python
"""Per-launch A/B of the 8^3-level 3x3x3 convs: the direct kernel with split-K (md_gemm_conv: fused GroupNorm loader, finish kernel)
against the K-sliced Winograd route (md_wino_prep_f6 + md_conv3_wino_splitk: operand pass, conv, finish) -- both through
layers.run_conv3, so each timing covers everything the route launches for one conv, statistics included.

One process, HIP events, the two routes alternating; median [min, max] of --reps measurements each (one measurement = --inner
convs queued back to back, divided by their number), after --warmup untimed pairs.
Shapes: the four Cin -> 512 convs of the bench's 8^3 level at B = 8, with and without a residual operand.

    python tools/bench_wino_splitk.py [--batch 8] [--reps 20] [--warmup 5]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshdiffusion_amd import hip_ops as ops                       # noqa: E402
from meshdiffusion_amd.lib.diffusion.models import layers          # noqa: E402

SHAPES = [(512, 512, True), (512, 512, False), (1024, 512, False), (768, 512, False), (256, 512, False)]      # (cin, cout, residual)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


class Pair(layers.HipLayer):
    def __init__(self, cin, cout):
        super().__init__()
        self.gn = torch.nn.GroupNorm(32, cin, eps=1e-6)
        self.conv = torch.nn.Conv3d(cin, cout, 3, padding=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8, help="convs queued back to back between one pair of events (the host's launch "
                    "overhead of a single conv is of the order of its GPU time: with several queued the GPU never waits for the host)")
    a = ap.parse_args()
    B, S = a.batch, 8
    P = S ** 3
    print(f"# {torch.cuda.get_device_name(0)}; B = {B}, 8^3; us per conv (all launches of the route), median [min, max] of {a.reps} x {a.inner}")
    for cin, cout, with_res in SHAPES:
        pair = Pair(cin, cout)
        with torch.no_grad():
            pair.conv.weight.copy_(_rand((cout, cin, 3, 3, 3), cin, 0.02))
            pair.gn.weight.copy_(1.0 + 0.2 * _rand((cin,), cin + 1)); pair.gn.bias.copy_(0.3 * _rand((cin,), cin + 2))
        pair = pair.cuda().eval()
        parts = [(ops.ncdhw_to_f32b((_rand((B, cin, S, S, S), cin + 3) * 1.5 + 0.2).cuda()), cin)]
        _, ac = ops.gn_params(parts, pair.gn.weight, pair.gn.bias, B, P, want_ac=True)
        bias = _rand((B, cout), cin + 4).cuda()
        res = ops.ncdhw_to_f32b(_rand((B, cout, S, S, S), cin + 5).cuda()) if with_res else None
        pw = layers.conv3_packed(pair, "w", pair.conv, ops.conv_cfg_for(S))
        wino = layers.conv3_wino_packed(pair, "w", pair.conv, gn=pair.gn)
        out = ops.f32b_empty(B, cout, P, "cuda")

        def run(split):
            ops.WINO_SPLITK = split
            with ops.precision_scope("f16f6"), torch.no_grad():
                return layers.run_conv3(pw, None, B, S, bias=bias, bias_bstride=cout, residual=res, want_stats=True, out=out,
                                        b_f32=ops.F32Operand(parts, ac, silu=True), wino=wino)

        keep = ops.WINO_SPLITK
        try:
            plans = {}
            for split in (False, True):
                ops.WINO_SPLITK = split
                with ops.precision_scope("f16f6"):
                    plans[split] = layers.plan_conv3(pw, ops.F32Operand(parts, ac, silu=True), B, S, ups=0, out_mode=ops.OUT_F32B,
                                                     rows_alloc=cout, want_stats=True, wino=wino)
            for _ in range(a.warmup):
                run(False); run(True)
            y = {s: run(s).clone() for s in (False, True)}
            diff = float((y[True].double() - y[False].double()).norm() / y[False].double().norm())
            times = {False: [], True: []}
            for _ in range(a.reps):
                for split in (False, True):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.inner):
                        run(split)
                    e1.record()
                    e1.synchronize()
                    times[split].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        finally:
            ops.WINO_SPLITK = keep
        fmt = lambda v: f"{statistics.median(v):7.1f} [{min(v):7.1f}, {max(v):7.1f}]"
        print(f"{cin:5d} -> {cout}{'/res' if with_res else '    '}  direct ks{plans[False].ksplit} ({plans[False].path}): {fmt(times[False])}   "
              f"wino ks{plans[True].ksplit} ({plans[True].path}/{plans[True].fmt}): {fmt(times[True])}   "
              f"delta {statistics.median(times[True]) - statistics.median(times[False]):+7.1f} us   rel-L2 between the routes {diff:.2e}")


if __name__ == "__main__":
    main()
