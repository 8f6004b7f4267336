"""Per-launch A/B of the small-level launches of md_gemm_conv between two builds of the library, in ONE process.

    python tools/bench_small_level_ab.py --parent /path/to/parent/libmeshdiffusion_hip.so [--launches N] [conv:512,512,8 gemm:256,512,4096,8 ...]

conv:CIN,COUT,B = a ResnetBlock conv at the 4^3 level: MD_CFG_C3_LOW, fp32 parts with GroupNorm affine + SiLU in the loader, the
split-K factor hip_ops.ksplit_for picks, GroupNorm sums in the finish kernel (md_gemm_conv = the conv kernel + md_splitk_reduce_stats,
timed together: that is what a step pays).  gemm:K,COUT,P,B[,res][,f32] = a 1x1x1 launch of MD_CFG_G1_128 with bias, F32B output,
optionally a residual, the operand S16B or (f32) one fp32 part split by the loader.  HIP events, 20 repetitions with the two libraries
alternating launch by launch: median [min, max] per launch for each, whether the two wrote the same words, and what the launch reaches
of the floors: distinct bytes per second (packed weights for the conv; operand + output + residual + weights for the GEMM) and issued
bf16x3 FLOP/s (3 MFMA products per multiply-add).  --launches N: a repetition times N back-to-back launches of one library and reports
their mean (N = 1 alternates after every launch, and every launch then starts behind another kernel's tail)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshdiffusion_amd import _lib, hip_ops as ops  # noqa: E402

REPS = 20
DEFAULT = ["conv:512,512,8", "conv:1024,512,8", "conv:512,512,1", "conv:1024,512,1",
           "gemm:256,512,4096,8", "gemm:256,256,4096,8,res", "gemm:768,256,4096,8", "gemm:1024,512,512,8"]


def bind(path):
    lib = C.CDLL(path)
    fn = lib.md_gemm_conv
    fn.restype, fn.argtypes = _lib.SIGNATURES["md_gemm_conv"]
    return lib


def conv_case(spec, g):
    cin, cout, B = map(int, spec.split(","))
    P = 64
    x = torch.randn((B, cin // 8, P, 8), device="cuda", generator=g)
    ac = torch.stack([0.5 + torch.rand((B, cin), device="cuda", generator=g), torch.randn((B, cin), device="cuda", generator=g) * 0.3], 2).contiguous()
    pw = ops.PackedWeight(torch.randn((cout, cin, 3, 3, 3), device="cuda", generator=g) * (27 * cin) ** -0.5, "conv", ops.CFG_C3_LOW, "cuda")
    bias = torch.randn(cout, device="cuda", generator=g)
    ks = ops.ksplit_for(ops.CFG_C3_LOW, B, cout, cin, 4)
    keep = [x, ac, pw, bias]

    def fill(r, out):
        part = torch.empty(ks * B * cout * P, dtype=torch.float32, device="cuda")
        stats = torch.zeros((B, cout, 2), dtype=torch.float64, device="cuda")
        keep.extend([part, stats])
        r.a, r.b, r.out, r.bias = pw.data.data_ptr(), x.data_ptr(), out.data_ptr(), bias.data_ptr()
        r.alpha, r.cfg, r.batch, r.rows, r.rows_alloc, r.kdim = 1.0, ops.CFG_C3_LOW, B, cout, cout, cin
        r.D = r.H = r.W = 4
        r.b_bstride, r.b_split, r.b_ac, r.b_silu, r.b_mode = cin * P, cin, ac.data_ptr(), 1, _lib.B_F32B_GN
        r.ksplit, r.partial, r.stats = ks, part.data_ptr(), stats.data_ptr()

    nbytes = pw.data.numel() * pw.data.element_size()
    return f"conv {cin}->{cout}@4^3 B={B} ksplit={ks}", B, cout, P, fill, nbytes, 3 * 2.0 * B * cout * cin * 27 * P, keep


def gemm_case(spec, g):
    f = spec.split(",")
    K, cout, P, B = map(int, f[:4])
    res, f32 = "res" in f[4:], "f32" in f[4:]
    x = torch.randn((B, K // 8, P, 8), device="cuda", generator=g)
    xs = None if f32 else ops.gn_apply([(x, K)], None, B, P, norm=False, silu=False)      # S16B split of the same values
    pw = ops.PackedWeight(torch.randn((K, cout), device="cuda", generator=g) * K ** -0.5, "nin", ops.CFG_G1_128, "cuda")
    bias = torch.randn(cout, device="cuda", generator=g)
    r0 = torch.randn((B, cout // 8, P, 8), device="cuda", generator=g) if res else None
    keep = [x, xs, pw, bias, r0]

    def fill(r, out):
        r.a, r.out, r.bias = pw.data.data_ptr(), out.data_ptr(), bias.data_ptr()
        r.alpha, r.cfg, r.batch, r.rows, r.rows_alloc, r.kdim = 1.0, ops.CFG_G1_128, B, cout, cout, K
        r.D, r.H, r.W = 1, 1, P
        if f32:
            r.b, r.b_bstride, r.b_split, r.b_mode = x.data_ptr(), K * P, K, _lib.B_F32B_GN
        else:
            r.b, r.b_bstride = xs.data_ptr(), (K // 8) * 2 * P * 8
        if res:
            r.residual, r.res_bstride = r0.data_ptr(), cout * P

    nbytes = (8 if f32 else 4) * B * K * P // (2 if f32 else 1) + 4 * B * cout * P * (2 if res else 1) + pw.data.numel() * pw.data.element_size()
    tag = f"gemm {K}->{cout}@P={P} B={B}" + ("/res" if res else "") + ("/f32" if f32 else "")
    return tag, B, cout, P, fill, nbytes, 3 * 2.0 * B * cout * K * P, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("cases", nargs="*", default=DEFAULT)
    a = ap.parse_args()
    _lib.load()
    libs = {"parent": bind(a.parent), "change": bind(_lib.LIB_PATH)}
    st = torch.cuda.current_stream().cuda_stream
    for case in a.cases:
        kind, spec = case.split(":")
        g = torch.Generator(device="cuda").manual_seed(1)
        tag, B, cout, P, fill, nbytes, flop, keep = (conv_case if kind == "conv" else gemm_case)(spec, g)
        out = {k: ops.f32b_empty(B, cout, P, "cuda") for k in libs}
        args = {}
        for k in libs:
            args[k] = _lib.MdGemmConvArgs()
            fill(args[k], out[k])

        def launch(k):
            rc = libs[k].md_gemm_conv(C.byref(args[k]), st)
            assert rc == 0, (k, rc)

        for _ in range(3):
            for k in libs:
                launch(k)
        torch.cuda.synchronize()
        same = bool(torch.equal(out["parent"].view(torch.int32), out["change"].view(torch.int32)))
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
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = f"{tag}: " + "  ".join(f"{k} {med[k]:.4f} ms [{min(v):.4f}, {max(v):.4f}]" for k, v in ms.items())
        reach = "  ".join(f"{k}: {nbytes / med[k] / 1e9:.2f} TB/s, issued {flop / med[k] / 1e9:.0f} TF/s" for k in libs)
        print(line + f"  gain {med['parent'] - med['change']:+.4f} ms; parent spread {max(ms['parent']) - min(ms['parent']):.4f} ms; "
              f"same words: {same}; {reach}", flush=True)
        del keep, out, args


if __name__ == "__main__":
    main()
