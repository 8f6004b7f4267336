"""Case definitions, restatements and derived bars for the earth mover's distance (csrc/emd.hip, metrics.emd_matrix):

    EMD(a, b) = (1/p) * min over permutations pi of sum_i |a_i - b_pi(i)|          (Euclidean distance, not its square)

No implementation was consulted: the oracle is scipy.optimize.linear_sum_assignment, once on float64 distances (`emd_float64`)
and once on the kernel's own integer matrix restated in numpy (`emd_quantised`).  `auction_restated` is the kernel's solver
written a second time in numpy -- for the round counts below, never as something the kernel's rounds must match.  Shared by
tests/test_cpu_emd_host.py, tests/test_gpu_emd.py and tools/bench_emd.py.

THE VALUE BAR   |out - emd_float64| <= VALUE_C * quantum + 2^-23 * emd_float64,   VALUE_C = 0.75,
for a quantum of `emd_quantum(..., bits=20)` (quantum * 2^20 >= the diagonal of the bounding box of all clouds >= any distance d).
  1. The fp32 distance.  u = 2^-24.  dx = fl(ax - bx) carries (1 + u); its square (1 + u)^3; the two additions put at most
     (1 + u)^2 on every term: the sum of squares is s (1 + t) with |t| <= 5u / (1 - 5u).  A correctly rounded square root
     gives d (1 + t)^(1/2) (1 + u): a relative error of at most 3.5 u + O(u^2), so
         |d_fp32 - d| <= 3.5 * 2^-24 * d <= 3.5 * 2^-24 * 2^20 quanta = 0.21875 quanta.
     (A square that underflows is off by less than 2^-149, nothing against a quantum; md_emd_matrix refuses quanta below 2^-126.)
  2. The integer.  q = rint(d_fp32 / quantum), the division exact: |q * quantum - d_fp32| <= 0.5 quanta.
  3. Every entry of the integer matrix is therefore within 0.71875 quanta of the float64 distance, so is the cost of every
     assignment per matched pair, and so are the two minima: |total * quantum / p - emd_float64| <= 0.71875 quanta.
  4. out = (float)((double)total * quantum / p): the product is exact (total < 2^53, a power of two), the division rounds by
     2^-53 and the conversion by 2^-24, relative to a value below emd_float64 + 0.72 quanta.
  0.71875 + 2^-24 * 0.72 rounds up to VALUE_C = 0.75; 2^-24 (1 + 2^-29) to 2^-23.  test_cpu_emd_host.py shows scipy on the
  integer matrix inside the bar on every finite case and prints the share it uses.

THE FLIP BAR   |total_gpu - emd_quantised| <= p quanta on general cases: an fp32 distance that differs from numpy's in its last
bit (there is none with a correctly rounded square root and no contraction, but the bar does not assume that) moves rint by at
most one quantum per matched pair.  On the exact-lattice cases every square and sum is exact in fp32, both sides take the
square root of the same number, and the test demands total_gpu == emd_quantised.

ROUNDS (auction_restated: theta = 4, eps0 = max(1, C / 2) with C the largest scaled cost, every phase restarts unassigned with the
prices kept).  Measured with this file, `python tests/emd_cases.py` (theta = 8, 16, 32 were tried: no better):
    random / sphere clouds p = 63 ... 257       2.5 - 8.4 p rounds        (p257: 1.5 k rounds, 10 k bids)
    sphere clouds p = 2048                      "p2048": 27.6 k rounds = 13.5 p, 137 k bids: 5 bidders per round on average
    clusters p = 256                            3.7 k = 14.6 p
    exact lattices                              7.6 - 10.8 p
    one point against another p = 64            2.9 k = 44.8 p, the worst rounds / p of all cases here
The default max_rounds of metrics.emd_matrix is 256 p + 4096: at p = 64 that is 20480 = 7.1 x the 2867 rounds of that worst case
(4 x them would be 11468: the default stays); at p = 2048 it is 528384 = 10 x the largest count the kernel has shown on 2048-point
sphere and torus samples (52336 = 25.6 p, tools/bench_emd.py, profiles/emd_bench.txt).  The kernel words the same solver, so its counts should be these; the tests print them and do not demand it.
"""
import math

import numpy as np
import torch

import pointcloud_cases as pc

VALUE_C = 0.75
BITS = 20
THETA = 4                               # the kernel's eps divisor (EMD_THETA in csrc/emd.hip)
MAX_P = 2048


def value_bar(emd64, quantum):
    return VALUE_C * quantum + 2.0 ** -23 * emd64


def flip_bar(p):
    return p


def default_max_rounds(p):
    return 256 * p + 4096


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _lattice3(p, seed):
    return (torch.randint(-32, 33, (p, 3), generator=_gen(seed)).to(torch.float32) / 8)[None]


def _clusters():
    g = _gen(8301)
    c0, c1 = torch.zeros(3), torch.tensor([1.0, 0.0, 0.0])
    a = torch.cat([c0 + 0.01 * torch.randn(128, 3, generator=g), c1 + 0.01 * torch.randn(128, 3, generator=g)])
    b = torch.cat([c0 + 0.01 * torch.randn(64, 3, generator=g), c1 + 0.01 * torch.randn(192, 3, generator=g)])
    return a[None], b[None]


EXACT_CASES = ("lat65", "lat256", "lat1d")
FINITE_CASES = ("p1", "p2", "p3", "p63", "p64", "p65", "p257", "p2048", "clusters", "permuted", "same_point", "two_points", "rect",
                "union")


def case(name):
    """(x float32 [Nx,P,3], y float32 [Ny,P,3]) on the CPU; for "union" y IS x."""
    if name in ("p1", "p2", "p3", "p63", "p64", "p65"):
        p = int(name[1:])
        return torch.rand(2, p, 3, generator=_gen(8100 + p)) - 0.5, torch.rand(2, p, 3, generator=_gen(8200 + p)) - 0.5
    if name == "p257":
        return pc.sphere_cloud(257, 0.5, (0.0, 0.0, 0.0), 8110)[None], pc.sphere_cloud(257, 0.45, (0.02, 0.0, 0.0), 8111)[None]
    if name == "p2048":                                     # the LDS limit
        return pc.sphere_cloud(2048, 0.5, (0.0, 0.0, 0.0), 8120)[None], pc.sphere_cloud(2048, 0.45, (0.02, 0.0, 0.0), 8121)[None]
    if name == "clusters":                                  # the price war that needs eps-scaling
        return _clusters()
    if name == "permuted":
        a = torch.rand(1, 200, 3, generator=_gen(8130)) - 0.5
        return a, a[:, torch.randperm(200, generator=_gen(8131))].contiguous()
    if name == "same_point":
        a = torch.tensor([0.25, -0.125, 0.375]).repeat(1, 50, 1)
        return a, a.clone()
    if name == "two_points":                                # every cost equal
        return torch.tensor([0.25, -0.125, 0.375]).repeat(1, 64, 1), torch.tensor([-0.3, 0.2, 0.1]).repeat(1, 64, 1)
    if name == "rect":
        return torch.rand(3, 33, 3, generator=_gen(8140)) - 0.5, torch.rand(5, 33, 3, generator=_gen(8141)) - 0.5
    if name == "union":
        x = torch.stack([pc.sphere_cloud(96, 0.3 + 0.03 * k, (0.0, 0.0, 0.0), 8150 + k) for k in range(7)])
        return x, x
    if name == "lat65":                                     # multiples of 1/8 in [-4, 4]: many repeated distances
        return _lattice3(65, 8160), _lattice3(65, 8161)
    if name == "lat256":
        return _lattice3(256, 8162), _lattice3(256, 8163)
    if name == "lat1d":                                     # every site of a 1-D lattice twice, b = a + (0.5, 0, 0): EMD exactly 0.5
        a = torch.zeros(1, 100, 3)
        a[0, :, 0] = -4 + torch.arange(100).div(2, rounding_mode="floor") / 8
        a = a[:, torch.randperm(100, generator=_gen(8164))].contiguous()
        return a, a + torch.tensor([0.5, 0.0, 0.0])
    raise KeyError(name)


def quantum_restated(*clouds, bits=BITS):
    """2^(ceil(log2 diag) - bits), diag the diagonal of the bounding box of all clouds in float64; 2^-bits for a zero diagonal."""
    pts = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds])
    diag = float(np.sqrt(((pts.max(axis=0) - pts.min(axis=0)) ** 2).sum()))
    if diag == 0:
        return 2.0 ** -bits
    m, e = math.frexp(diag)                                 # diag = m 2^e, 0.5 <= m < 1
    return 2.0 ** ((e - 1 if m == 0.5 else e) - bits)


# ---- restatements ---------------------------------------------------------------------------------------------------------
def _assignment(cost):
    from scipy.optimize import linear_sum_assignment
    return linear_sum_assignment(cost)


def emd_float64(a, b):
    """scipy on float64 Euclidean distances of the fp32 points a, b [P,3]."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))
    r, c = _assignment(d)
    return float(d[r, c].sum() / a.shape[0])


def quantised(a, b, quantum):
    """The kernel's integer matrix int64 [P,P]: fp32, direct form, numpy's correctly rounded square root, rint(d / quantum)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    dx, dy, dz = (a[:, None, k] - b[None, :, k] for k in range(3))
    d = np.sqrt(dz * dz + (dy * dy + dx * dx))
    assert d.dtype == np.float32
    return np.rint(d / np.float32(quantum)).astype(np.int64)


def emd_quantised(a, b, quantum):
    """scipy on the integer matrix: the optimal integer cost."""
    q = quantised(a, b, quantum)
    r, c = _assignment(q)
    return int(q[r, c].sum())


def emd_float64_matrix(x, y):
    return torch.tensor([[emd_float64(a, b) for b in y] for a in x], dtype=torch.float64)


def out_from_total(total, quantum, p):
    return (np.asarray(total, dtype=np.float64) * np.float64(quantum) / np.float64(p)).astype(np.float32)


def auction_restated(q, theta=THETA):
    """Forward Jacobi auction with eps-scaling on the integer matrix q [P,P] scaled by P + 1, as csrc/emd.hip words it.
    Returns (total, perm, rounds, bids)."""
    p = q.shape[0]
    cost = q.astype(np.int64) * (p + 1)
    price = np.zeros(p, dtype=np.int64)
    eps = max(1, int(cost.max()) // 2)
    rounds = bids = 0
    while True:
        owner = np.full(p, -1, dtype=np.int64)              # object -> person
        asg = np.full(p, -1, dtype=np.int64)                # person -> object
        while True:
            who = np.nonzero(asg < 0)[0]
            if who.size == 0:
                break
            rounds += 1
            bids += who.size
            w = cost[who] + price[None, :]
            best = w.argmin(axis=1)                         # the lowest index among ties
            w1 = w[np.arange(who.size), best]
            if p > 1:
                w[np.arange(who.size), best] = np.iinfo(np.int64).max
                gamma = w.min(axis=1) - w1
            else:
                gamma = np.zeros(1, dtype=np.int64)
            bid = price[best] + gamma + eps
            for j in np.unique(best):
                m = best == j
                top = bid[m].max()
                i = who[m][bid[m] == top].min()             # the highest bid, ties to the lowest bidder
                if owner[j] >= 0:
                    asg[owner[j]] = -1
                owner[j], asg[i], price[j] = i, j, top
        if eps == 1:
            break
        eps = max(1, eps // theta)
    return int(q[np.arange(p), asg].sum()), asg, rounds, bids


if __name__ == "__main__":
    for name in EXACT_CASES + FINITE_CASES:
        x, y = case(name)
        quantum = quantum_restated(x, y)
        a, b = x[0].numpy(), y[-1].numpy()
        q = quantised(a, b, quantum)
        total, perm, rounds, bids = auction_restated(q)
        want = emd_quantised(a, b, quantum)
        print(f"{name}: p {q.shape[0]} rounds {rounds} ({rounds / q.shape[0]:.1f} p) bids {bids} total {total} scipy {want}"
              f" {'ok' if total == want else 'DIFFERENT'}", flush=True)
