"""Cost of the all-pairs chamfer matrix behind MMD / COV / 1-NNA, one process: the union matrix of T clouds of 2048 points by
  (a) `metrics.chamfer_matrix(x)`: one launch of md_sided_mean_matrix plus S + S^T;
  (b) the route the tree offered before that kernel: `pointcloud.sided_distance` on EXPANDED pair batches ([rows * T, 2048, 3]
      copies of both sides, chunked so that a chunk's operands, workspace and outputs stay under --chunk_bytes and its batch
      under the launch limit), float64 means, S + S^T.
Device events after warm-up; the two alternate round by round and each figure is the median over rounds.  Reports point-to-point
distances per second and the implied share of the fp32 vector peak at FLOP_PER_DISTANCE (3 subtractions, 1 multiply, 2
multiply-adds: the minimum is not counted), and how far the two routes' matrices are apart (the same fp32 minima, float64 sums in
another order: last-bit differences at the most).
    python tools/bench_shape_metrics.py [--clouds 256] [--all] [--rounds 5] [--reps 3] [--out profiles/shape_metrics_bench.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pc import interleaved  # noqa: E402

FLOP_PER_DISTANCE = 8
PEAK_FP32 = 157.3e12
POINTS = 2048
PAIR_BYTES = 2 * POINTS * 12 + POINTS * (8 + 4 + 8)      # both operands, one 64-bit key per query per chunk of q, dist, idx


def expanded_route(x, chunk_bytes):
    """The union chamfer matrix of x [T,P,3] through pointcloud.sided_distance on expanded pair batches."""
    from meshdiffusion_amd.pointcloud import sided_distance
    T, P = x.shape[0], x.shape[1]
    rows = max(1, min(65535 // T, chunk_bytes // (PAIR_BYTES * T)))
    s = torch.empty((T, T), dtype=torch.float32, device=x.device)
    for i0 in range(0, T, rows):
        n = min(rows, T - i0)
        p = x[i0:i0 + n, None].expand(n, T, P, 3).reshape(n * T, P, 3)
        q = x[None].expand(n, T, P, 3).reshape(n * T, P, 3)
        d, _ = sided_distance(p, q)
        s[i0:i0 + n] = d.mean(dim=1, dtype=torch.float64).reshape(n, T).to(torch.float32)
    return s + s.t()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, nargs="+", default=[256])
    ap.add_argument("--all", action="store_true", help="T = 64, 256 and 1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk_bytes", type=int, default=2 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape_metrics_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shape_metrics.py needs a GPU: the HIP path has no CPU fallback")
    import pointcloud_cases as pc
    import shape_metrics_cases as sm
    from meshdiffusion_amd.metrics import chamfer_matrix

    lines = [f"union chamfer matrix of T clouds x {POINTS} points; device events, {a.rounds} interleaved rounds x {a.reps} calls (1 above T = 256), medians;"
             f" {FLOP_PER_DISTANCE} FLOP per distance against {PEAK_FP32 / 1e12:.1f} TF fp32 vector peak"]
    print(lines[0], flush=True)
    for T in ([64, 256, 1024] if a.all else a.clouds):
        x = torch.stack([pc.sphere_cloud(POINTS, 0.3 + 0.2 * k / T, (0.0, 0.0, 0.0), 100 + k) for k in range(T)]).cuda()
        new, old = chamfer_matrix(x), expanded_route(x, a.chunk_bytes)
        apart = float(((new.double() - old.double()).abs() / old.double().clamp_min(1e-300)).max())
        assert torch.equal(new, new.t()) and not bool(torch.diagonal(new).any())
        ok, worst = sm.within_bar(new[:4, :4], sm.chamfer_float64(x[:4]), sm.VALUE_BAR + 2.0 ** -24)      # a corner against float64
        assert ok, worst
        reps = a.reps if T <= 256 else 1
        for _ in range(2):
            chamfer_matrix(x); expanded_route(x, a.chunk_bytes)
        torch.cuda.synchronize()
        med, raw = interleaved({"new": lambda: chamfer_matrix(x), "expanded": lambda: expanded_route(x, a.chunk_bytes)}, a.rounds, reps)
        dist = float(T) * T * POINTS * POINTS
        rate = dist / (med["new"] * 1e-3)
        line = (f"T={T}: md_sided_mean_matrix {med['new']:.3f} ms (rounds {', '.join(f'{v:.3f}' for v in raw['new'])}) | expanded "
                f"sided_distance batches {med['expanded']:.3f} ms (rounds {', '.join(f'{v:.3f}' for v in raw['expanded'])}) | x"
                f"{med['expanded'] / med['new']:.2f} | {rate / 1e12:.3f} T distances/s = {rate * FLOP_PER_DISTANCE / PEAK_FP32 * 100:.1f} % "
                f"of the fp32 vector peak | expanded route {dist / (med['expanded'] * 1e-3) / 1e12:.3f} T distances/s | matrices apart by "
                f"{apart:.2e} relative at the most")
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
