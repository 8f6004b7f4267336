"""Per-launch timing of md_wino_prep_f6_nin (csrc/block_pass.hip) against the two kernels it replaces.

    python tools/bench_block_pass.py CIN,S,NIN [...]        e.g.  256,64,1 256,32,1 128,64,0 256,64,0
NIN = 1: the fused launch against md_wino_prep_f6 + md_nin_f32; NIN = 0: the operand-only mode (wpk = NULL) against md_wino_prep_f6.
B = 8, HIP events, 20 interleaved repetitions: median [min, max] per launch and the fused launch's algorithmic GB/s."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshdiffusion_amd import hip_ops as ops

B, REPS = 8, 20


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fn):
    a, b = ev(), ev()
    a.record(); fn(); b.record()
    return a, b


def run(cin, S, nin=True):
    P = S ** 3
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((B, cin // 8, P, 8), device="cuda", generator=g)
    parts = [(x[:, :cin // 16].contiguous(), cin // 2), (x[:, cin // 16:].contiguous(), cin // 2)]
    del x
    ac = torch.stack([0.5 + torch.rand((B, cin), device="cuda"), torch.randn((B, cin), device="cuda") * 0.3], 2).contiguous()
    eq = torch.exp2(torch.randint(-3, 4, (cin,), device="cuda").float())
    pw = ops.PackedWeight(torch.randn((cin, 128), device="cuda") * 0.1, "nin", ops.CFG_G1_128, "cuda")
    bias = torch.randn(128, device="cuda")
    out = ops.f32b_empty(B, 128, P, "cuda")
    f_prep = lambda: ops.wino_prep(parts, ac, True, 0, B, S, f8="f6", eq=eq)
    f_nin = lambda: ops.nin_f32(parts, pw, bias, B, P, out=out)
    f_fused = lambda: ops.wino_prep_nin(parts, ac, True, B, S, eq, pw if nin else None, bias if nin else None)
    for _ in range(3):
        f_prep(); f_nin(); f_fused()
    torch.cuda.synchronize()
    rec = {"prep": [], "nin": [], "fused": []}
    for _ in range(REPS):
        rec["prep"].append(timed(f_prep))
        if nin:
            rec["nin"].append(timed(f_nin))
        rec["fused"].append(timed(f_fused))
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in rec.items() if v}
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (min(v), max(v)) for k, v in ms.items()}
    nbytes = 4.0 * B * cin * P + 8.0 * B * cin * P + (4.0 * B * 128 * P if nin else 0.0)
    line = f"{cin}@{S}^3 B={B} {'fused prep+nin' if nin else 'operand only'}: " + "  ".join(
        f"{k} {med[k]:.4f} ms [{spread[k][0]:.4f}, {spread[k][1]:.4f}]" for k in med)
    if nin:
        line += f"  prep+nin {med['prep'] + med['nin']:.4f} ms"
    line += f"  fused {nbytes / med['fused'] / 1e6:.0f} GB/s"
    print(line, flush=True)
    ops.release_scratch()


for a in sys.argv[1:]:
    cin, S, nin = a.split(",")
    run(int(cin), int(S), nin == "1")
