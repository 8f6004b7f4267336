"""Cost of the all-pairs earth mover's distance matrix behind MMD / COV / 1-NNA (EMD), one process: the union matrix of T clouds
of 2048 points -- T (T - 1) / 2 assignment problems of 2048 x 2048, one workgroup each (`metrics.emd_matrix(x)`, md_emd_matrix).
Half the clouds are surface samples of spheres, half of tori (the generators of tests/shape_metrics_cases.py), normalised to
their bounding boxes like tools/eval_shapes.py does.  Device events after one warm-up call, the median over --reps calls.
Reports seconds, pairs per second, the minimum / median / maximum of the bidding rounds per pair, and as context the host's time
for scipy.optimize.linear_sum_assignment on ONE of those pairs (float64 distances), whose value the kernel's is checked against.
    python tools/bench_emd.py [--clouds 32] [--all] [--reps 3] [--out profiles/emd_bench.txt]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

POINTS = 2048


def clouds(T):
    import shape_metrics_cases as sm
    from meshdiffusion_amd.metrics import clouds_from_meshes, normalize_clouds
    half = T // 2
    meshes = [sm.sphere_mesh(0.3 + 0.2 * k / half) for k in range(half)]
    meshes += [sm.torus_mesh(0.3 + 0.2 * k / (T - half), 0.1, 0.0) for k in range(T - half)]
    gen = torch.Generator(device="cuda").manual_seed(1234)
    return normalize_clouds(clouds_from_meshes(meshes, POINTS, generator=gen)[0], "bbox")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, nargs="+", default=[32])
    ap.add_argument("--all", action="store_true", help="T = 32 and 64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emd_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_emd.py needs a GPU: the HIP path has no CPU fallback")
    import emd_cases as ec
    from meshdiffusion_amd.metrics import emd_matrix, emd_quantum

    lines = [f"union EMD matrix of T clouds x {POINTS} points (spheres and tori, bbox-normalised); device events, median of {a.reps} calls"]
    print(lines[0], flush=True)
    for T in ([32, 64] if a.all else a.clouds):
        x = clouds(T)
        quantum = emd_quantum(x)
        out, info = emd_matrix(x, quantum=quantum, return_info=True)              # warm-up, and the round counts
        assert int(info["status"].abs().max()) == 0 and torch.equal(out, out.t()) and not bool(out.diagonal().any())
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            again = emd_matrix(x, quantum=quantum)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            assert torch.equal(again, out)
        sec = sorted(ms)[len(ms) // 2] * 1e-3
        pairs = T * (T - 1) // 2
        r = info["rounds"][torch.triu(torch.ones(T, T, dtype=torch.bool, device=x.device), 1)].to(torch.float64)
        line = (f"T={T}: {pairs} pairs in {sec:.4f} s (calls {', '.join(f'{v * 1e-3:.4f}' for v in ms)}) = {pairs / sec:.0f} pairs/s, "
                f"{sec / pairs * 1e3:.3f} ms per pair of the launch; rounds per pair min {int(r.min())} median {int(r.median())} max "
                f"{int(r.max())} = {r.max() / POINTS:.1f} p (cap {ec.default_max_rounds(POINTS)}); quantum 2^{int(torch.log2(torch.tensor(quantum)))}")
        print(line, flush=True)
        lines.append(line)
        if T == (32 if a.all else a.clouds[0]):
            one, one_info = emd_matrix(x[:1], x[T - 1:].clone(), quantum=quantum, return_info=True)      # one pair alone: one CU
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            emd_matrix(x[:1], x[T - 1:].clone(), quantum=quantum)
            e1.record()
            torch.cuda.synchronize()
            t0 = time.time()
            e64 = ec.emd_float64(x[0].cpu().numpy(), x[T - 1].cpu().numpy())
            host = time.time() - t0
            assert abs(float(one[0, 0]) - e64) <= ec.value_bar(e64, quantum) and float(one[0, 0]) == float(out[0, T - 1])
            line = (f"one pair (cloud 0, cloud {T - 1}) alone: {e0.elapsed_time(e1):.2f} ms on one CU, {int(one_info['rounds'][0, 0])} rounds; "
                    f"scipy linear_sum_assignment on the host, float64: {host:.2f} s; EMD {float(one[0, 0]):.7f} against {e64:.7f}")
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
