"""What the light-field distance costs, one process (meshdiffusion_amd/lfd.py, csrc/lfd.hip):
  * the three stages for the 32 meshes of one marching-tetrahedra launch on the shipped 64 grid (sign grids of ellipsoids and tori) at 256 x 256, 10 light fields of 10
    views: `silhouettes` (the rasteriser and the torch glue around it, mesh by mesh), `describe` (md_lfd_describe on the 3200
    masks) and `lfd_matrix` (md_lfd_matrix, the triangular union of the 32 models), each timed on its own, and the share of the
    rasteriser stage in their sum;
  * `describe` against a plain-torch statement of the same formulas (fp32 on the device, one mesh = 100 masks per call: masked
    sums of R_nm(rho) cos / sin(m theta), scatter-max signature, a 64-point transform);
  * `lfd_matrix` for a union of T = 64 and 256 models of random bytes (integer work: its time does not depend on the bytes) against
    a torch broadcast version (per x model: |x - y| summed over the 48 bytes for every (la, lb, v, u), a gather per rotation, a
    minimum), whose result must be equal.
Device events after a warm-up call, medians over rounds with the variants alternating.  No pass / fail bar on time.
    python tools/bench_lfd.py [--meshes 32] [--res 256] [--fields 10] [--models 64 256] [--rounds 3] [--out profiles/lfd_bench.txt]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pc import interleaved  # noqa: E402


def torch_describe(masks, nm, coefs):
    """float32 [n,45]: the contract's formulas as torch ops on masks uint8 [n,R,R] (non-empty)."""
    n, R, _ = masks.shape
    m = masks.reshape(n, -1) != 0
    w = m.to(torch.float32)
    idx = torch.arange(R * R, device=masks.device)
    x, y = (idx % R).to(torch.float32), torch.div(idx, R, rounding_mode="floor").to(torch.float32)
    count = w.sum(dim=1, keepdim=True)
    dx, dy = x[None] - (w * x).sum(dim=1, keepdim=True) / count, y[None] - (w * y).sum(dim=1, keepdim=True) / count
    r = torch.sqrt(dx * dx + dy * dy) * w
    rho = r / r.max(dim=1, keepdim=True).values.clamp_min(0.5)
    theta = torch.atan2(dy, dx)
    out = torch.empty((n, 45), dtype=torch.float32, device=masks.device)
    power = {0: torch.ones_like(rho)}
    for k in range(1, 11):
        power[k] = power[k - 1] * rho
    for j, ((nn, mm), cs) in enumerate(zip(nm, coefs)):
        Rnm = sum(c * power[k] for c, k in cs) * w
        re, im = (Rnm * torch.cos(mm * theta)).sum(dim=1), (Rnm * torch.sin(mm * theta)).sum(dim=1)
        out[:, j] = 512 * torch.sqrt(re * re + im * im) / count[:, 0]
    b = torch.floor(theta * (64 / (2 * math.pi)) + 0.5).to(torch.int64) % 64
    sig = torch.zeros((n, 64), dtype=torch.float32, device=masks.device).scatter_reduce(1, b, rho * w, "amax", include_self=True)
    f = torch.fft.fft(sig, dim=1)[:, 1:11].abs() / sig.sum(dim=1, keepdim=True).clamp_min(1e-30)
    out[:, 35:] = 512 * f
    return out


def torch_matrix(x, perms):
    """int32 [T,T] of x uint8 [T,L,10,48] against itself: the contract's minimum by broadcasting, one x model at a time."""
    T = x.shape[0]
    xs = x.to(torch.int16)
    v = torch.arange(10, device=x.device)
    out = torch.empty((T, T), dtype=torch.int32, device=x.device)
    for i in range(T):
        tab = (xs[i][None, :, None, :, None, :] - xs[:, None, :, None, :, :]).abs().sum(dim=-1, dtype=torch.int32)      # [T,la,lb,v,u]
        out[i] = tab[:, :, :, v[None], perms].sum(dim=-1).reshape(T, -1).min(dim=1).values                                  # [T,la,lb,G]
    return out


def sign_grids(M, R=64):
    """[M,4,R,R,R] float32 for GridMesher: channel 0 the sign of an ellipsoid (even m) or a torus (odd m) whose proportions change
    with m, no deformation."""
    k = (torch.arange(R, dtype=torch.float32) + 0.5) / R - 0.5
    z, y, x = torch.meshgrid(k, k, k, indexing="ij")
    out = torch.zeros(M, 4, R, R, R)
    for m in range(M):
        t = m / max(M - 1, 1)
        if m % 2 == 0:
            sdf = torch.sqrt((x / 0.4) ** 2 + (y / (0.15 + 0.25 * t)) ** 2 + (z / (0.4 - 0.2 * t)) ** 2) - 1.0
        else:
            sdf = torch.sqrt((torch.sqrt(x * x + y * y) - (0.2 + 0.1 * t)) ** 2 + z * z) - (0.12 - 0.06 * t)
        out[m, 0] = torch.sign(sdf)
    return out.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--fields", type=int, default=10)
    ap.add_argument("--models", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfd_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lfd.py needs a GPU: the HIP path has no CPU fallback")
    import lfd_cases as lc
    import raster_cases as rc
    from meshdiffusion_amd import lfd
    from meshdiffusion_amd.dmtet import GridMesher

    tv, ti = rc.tet_grid()
    meshes = [(v.detach().clone(), f.clone()) for v, f, _ in GridMesher(tv, ti, 64)(torch.from_numpy(sign_grids(a.meshes)))]
    faces = sum(int(f.shape[0]) for _, f in meshes)
    L, R, views = a.fields, a.res, a.fields * lfd.VIEWS
    lines = [f"{a.meshes} marching-tets meshes ({faces} faces in all), {L} light fields x {lfd.VIEWS} views at {R} x {R}: {a.meshes * views} silhouettes"]

    def stage_silhouettes():
        return [lfd.silhouettes(v, f, R, L) for v, f in meshes]

    masks = torch.cat(stage_silhouettes())
    desc, coef, status = lfd.describe(masks, return_info=True)
    models = desc.reshape(a.meshes, L, lfd.VIEWS, lfd.DESC_BYTES)
    nm = lc.NM
    coefs = [lc.radial_coefficients(n, m) for n, m in nm]
    full = status == 0
    want = torch.cat([torch_describe(masks[k:k + views], nm, coefs) for k in range(0, masks.shape[0], views)])
    gap = float((coef[full] - want[full]).abs().max())
    filled = float(masks.to(torch.float32).mean())
    stages = {"silhouettes": stage_silhouettes, "describe": lambda: lfd.describe(masks), "matrix": lambda: lfd.lfd_matrix(models),
              "torch_describe": lambda: [torch_describe(masks[k:k + views], nm, coefs) for k in range(0, masks.shape[0], views)]}
    for fn in stages.values():
        fn()
    med, _ = interleaved(stages, a.rounds, 1)
    total = med["silhouettes"] + med["describe"] + med["matrix"]
    lines += [f"silhouettes {med['silhouettes']:.2f} ms | describe {med['describe']:.3f} ms | lfd_matrix (triangular, {a.meshes} models) "
              f"{med['matrix']:.3f} ms | the rasteriser stage is {100 * med['silhouettes'] / total:.1f} % of their sum {total:.2f} ms; "
              f"{100 * filled:.1f} % of the pixels are set, {int((~full).sum())} empty masks",
              f"describe, {masks.shape[0]} masks: HIP {med['describe']:.3f} ms ({med['describe'] * 1e3 / masks.shape[0]:.2f} us per mask) | plain torch, "
              f"100 masks per call {med['torch_describe']:.2f} ms | x{med['torch_describe'] / med['describe']:.1f}; largest |512 z| difference {gap:.2e} "
              f"(torch sums in fp32)"]
    perms = torch.from_numpy(lfd.rotation_perms().astype(np.int64)).cuda()
    for T in a.models:
        x = torch.randint(0, 256, (T, L, lfd.VIEWS, lfd.DESC_BYTES), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(T))
        got = lfd.lfd_matrix(x)
        equal = torch.equal(got, torch_matrix(x, perms))
        m2, _ = interleaved({"hip": lambda: lfd.lfd_matrix(x), "torch": lambda: torch_matrix(x, perms)}, a.rounds, 1)
        pairs = T * (T - 1) // 2
        lines.append(f"lfd_matrix, union of T={T} models ({pairs} pairs, {L}^2 field pairs x 60 rotations each): HIP {m2['hip']:.3f} ms = "
                     f"{m2['hip'] * 1e3 / pairs:.2f} us per pair | torch broadcast {m2['torch']:.1f} ms | x{m2['torch'] / m2['hip']:.1f}; equal: {equal}")
    lines.append(f"medians of {a.rounds} rounds, variants alternating; device events after a warm-up call")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
