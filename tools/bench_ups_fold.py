"""Per-launch A/B of an f16f6 Upsample conv: the 9-tap route on the compact operand (md_conv3_wino_upsdh) against the fold
(md_conv3_wino_upsfold), same operand, same equaliser, one process, HIP events, launches alternating, median [min, max] of 20.

    python tools/bench_ups_fold.py [out.txt] [sweep]

The three Upsample shapes of the res64 workload at B = 8; with `sweep` also Cin = 32 .. 256 at 128 rows on 64^3, which separates a
launch's fixed cost (prologue, epilogue) from its cost per 32 input channels (the main loop)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshdiffusion_amd import hip_ops as ops  # noqa: E402
from meshdiffusion_amd.lib.diffusion.models.layers import fold_upsample_weight  # noqa: E402

REPS = 20
lines = []


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def measure(Cin, Cout, S, B):
    x = rnd((B, Cin, S // 2, S // 2, S // 2), 1)
    w = rnd((Cout, Cin, 3, 3, 3), 2, 0.05)
    bias = rnd((Cout,), 3).cuda()
    parts = [(ops.ncdhw_to_f32b(x.cuda()), Cin)]
    ms = ops.wino_operand_ms(parts, None, False, B, (S // 2) ** 3)
    eq = ops.wino_equaliser(None, None, w.cuda(), a2m=ms)
    ww = ops.WinoWeightF8(w.cuda(), "cuda", "f6", eq=eq)
    wf = ops.WinoWeightF8(fold_upsample_weight(w).cuda(), "cuda", "f6", eq=eq)
    out = ops.f32b_empty(B, Cout, S ** 3, torch.device("cuda"))
    times = {"old": [], "fold": []}

    def launch(route):      # the operand pass in front of every conv, as in a step; only the conv is timed
        t = ops.wino_prep(parts, None, False, True, B, S, f8="f6", eq=eq, compact=True)
        st = ops.stats_zeros(B, Cout, torch.device("cuda"))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if route == "old":
            ops.conv3_wino(ww, t, B, S, bias=bias, stats=st, out=out)
        else:
            ops.conv3_wino_upsfold(wf, t, B, S, bias=bias, stats=st, out=out)
        e1.record()
        return e0, e1

    for _ in range(3):
        launch("old"); launch("fold")
    torch.cuda.synchronize()
    evs = [(r, launch(r)) for _ in range(REPS) for r in ("old", "fold")]
    torch.cuda.synchronize()
    for r, (e0, e1) in evs:
        times[r].append(e0.elapsed_time(e1))
    f = lambda v: f"{statistics.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]"
    line = (f"  {Cin}->{Cout}@{S}^3 B={B} f16f6: 9-tap route {f(times['old'])} ms | fold {f(times['fold'])} ms | "
            f"ratio {statistics.median(times['fold']) / statistics.median(times['old']):.3f}")
    print(line, flush=True)
    lines.append(line)
    del x, w, parts, out
    ops.release_scratch()
    torch.cuda.empty_cache()


def main():
    for (C, S, B) in [(128, 64, 8), (256, 32, 8), (512, 16, 8)]:
        measure(C, C, S, B)
    if "sweep" in sys.argv[1:]:
        for cin in (32, 64, 128, 256):
            measure(cin, 128, 64, 8)
    outs = [a for a in sys.argv[1:] if a != "sweep"]
    if outs:
        with open(outs[0], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
