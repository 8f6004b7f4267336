"""Per-launch A/B of the f16f6 operand passes between two builds of the library, in ONE process.

    python tools/bench_operand_ab.py --parent /path/to/parent/libmeshdiffusion_hip.so [--also name=/path/to/another.so ...] [--launches N]
                                     [block:256,64 block:256,32 plain:128,64 plain:256,64]

block:CIN,S = md_wino_prep_f6_nin (two parts of CIN / 2 channels, NIN weights: the launch of a shortcut block); plain:CIN,S =
md_wino_prep_f6.  B = 8, GroupNorm affine + SiLU + equaliser, HIP events, 20 repetitions with the two libraries alternating launch by
launch: median [min, max] per launch for each, and whether the two wrote the same words.  --also: further builds in the same
rotation (one item of a change alone).  --launches N: a repetition times N back-to-back launches of one library and reports their mean
(N = 1 alternates after every launch, and every launch then starts behind another kernel's tail)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshdiffusion_amd import _lib, hip_ops as ops  # noqa: E402

B, REPS = 8, 20


def bind(path):
    lib = C.CDLL(path)
    for name in ("md_wino_prep_f6", "md_wino_prep_f6_nin"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--also", action="append", default=[])
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("cases", nargs="*", default=["block:256,64", "block:256,32", "plain:128,64", "plain:256,64"])
    a = ap.parse_args()
    _lib.load()
    libs = {"parent": bind(a.parent)}
    for spec in a.also:
        name, path = spec.split("=", 1)
        libs[name] = bind(path)
    libs["change"] = bind(_lib.LIB_PATH)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for case in a.cases:
        kind, shape = case.split(":")
        cin, S = map(int, shape.split(","))
        P = S ** 3
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((B, cin // 8, P, 8), device="cuda", generator=g)
        x1, x2 = x[:, :cin // 16].contiguous(), x[:, cin // 16:].contiguous()
        del x
        ac = torch.stack([0.5 + torch.rand((B, cin), device="cuda", generator=g), torch.randn((B, cin), device="cuda", generator=g) * 0.3], 2).contiguous()
        eq = torch.exp2(torch.randint(-3, 4, (cin,), device="cuda", generator=g).float())
        pw = ops.PackedWeight(torch.randn((cin, 128), device="cuda", generator=g) * 0.1, "nin", ops.CFG_G1_128, "cuda")
        bias = torch.randn(128, device="cuda", generator=g)
        nbytes = _lib.load().md_wino_operand_bytes(B, cin, S, S, S)
        T = {k: torch.empty(nbytes // 2, dtype=torch.int16, device="cuda") for k in libs}
        res = {k: ops.f32b_empty(B, 128, P, "cuda") for k in libs}

        def launch(k):
            if kind == "block":
                rc = libs[k].md_wino_prep_f6_nin(p(x1), p(x2), cin // 2, cin // 2, p(ac), 1, p(eq), p(T[k]), p(pw.data), p(bias), p(res[k]), B, S, S, S, 0, st)
            else:
                rc = libs[k].md_wino_prep_f6(p(x1), p(x2), cin // 2, cin // 2, p(ac), 1, 0, p(eq), p(T[k]), B, S, S, S, st)
            assert rc == 0, (k, rc)

        for _ in range(3):
            for k in libs:
                launch(k)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(T["parent"], T[k])) and (kind != "block" or bool(torch.equal(res["parent"].view(torch.int32), res[k].view(torch.int32))))
                   for k in libs)
        rec = {k: [] for k in libs}
        for _ in range(REPS):
            for k in libs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    launch(k)
                e1.record()
                rec[k].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: [e0.elapsed_time(e1) / a.launches for e0, e1 in v] for k, v in rec.items()}
        line = f"{kind} {cin}@{S}^3 B={B}: " + "  ".join(f"{k} {statistics.median(v):.4f} ms [{min(v):.4f}, {max(v):.4f}]" for k, v in ms.items())
        d = "  ".join(f"{k} {statistics.median(ms['parent']) - statistics.median(ms[k]):+.4f}" for k in libs if k != "parent")
        print(line + f"  gain (ms) {d}; parent spread {max(ms['parent']) - min(ms['parent']):.4f} ms; same words: {same}", flush=True)
        del T, res, x1, x2
        ops.release_scratch()


if __name__ == "__main__":
    main()
