"""THE LFD CONTRACT (csrc/lfd.hip, include/meshdiffusion_hip.h) restated in plain numpy: the descriptor in float64 from the formulas
(`describe_float64`), the kernel's per-pixel fp32 scheme (`describe_fp32`), the matrix as integer loops (`matrix_numpy`), the
masks the tests run on (`CASES`) and the error bar of the descriptor (`DESC_BAR`, `COEF_BAR`), derived below from the scheme and
from nothing else.  No GPU here.

THE BAR.  u = 2^-24 is the unit roundoff of fp32; every line is to first order in u, and the factor 1.001 at the end pays for
the rest (the largest relative term below is about 70 u = 4e-6, its square 2e-11).

  * Nx, Ny, q = Nx^2 + Ny^2, Q and Qe are exact integers (Qe = max(Q, count^2 / 4) exact in float64).  inv = fp32(1/sqrt(Qe)) and
    inv2 = fp32(1/Qe) are correctly rounded float64 results rounded once more: relative error u each.
  * w = (fp32(Nx) inv, -fp32(Ny) inv): a conversion (u), inv (u) and a product (u): each component has relative error 3u, so
    |w^ - w| <= 3u |w|, |w| = rho <= 1.
  * t = fp32(q) inv2: again 3u relative, t = rho^2 <= 1.
  * W_m = W_{m-1} w, a complex product without fused operations: each component is a sum of two rounded products, rounded:
    error <= 2u (|ar br| + |ai bi|) <= 2u |a| |b| per component, hence <= 2 sqrt(2) u |a| |b| < 3u |a| |b| in modulus.  By
    induction |W_m^ - w^m| <= (3m + 3(m - 1)) u rho^m = (6m - 3) u for m >= 1, and W_0 = 1 is exact.
  * P_nm(t) = sum_j c_j t^j of degree k = (n - m) / 2 with S = sum_j |c_j| (the coefficients of R_nm), by Horner with a rounded
    multiply and a rounded add per step: |P^(t^) - P(t^)| <= 2k u S (Higham, Accuracy and Stability, section 5.1, with t <= 1), and
    the rounded argument moves the value by sum_j |c_j| |t^^j - t^j| <= sum_j |c_j| 3 j u <= 3k u S.  |P| <= S.
  * term = P W_m, one more rounding per component: u |P| |W_m| <= u S.  Together, in modulus,
        |term^ - term| <= u S (5k + max(0, 6m - 3) + 1).
  * Each component times 2^32 is rounded to an integer: at most 2^-33 per component, below 2^-32 in modulus.  The integer sum is
    exact.  The mean of the terms is therefore off by at most the bound of one term, and | . | is 1-Lipschitz.
  * The float64 tail (|sum| / count, times 512) contributes 1e-13; the single rounding to fp32 of 512 z <= 512 at most 512 u.

        DESC_BAR[n, m] = 512 (1.001 u S_nm (5 (n - m)/2 + max(0, 6m - 3) + 1) + 2^-32) + 512 u             in units of 512 z

It runs from 2e-4 (n = m) to 1.34 at (10, 0), where S = 1683: the power form pays for its cancellation, and a byte whose bar
exceeds one half is never required to be equal (the tests then ask for |difference| <= 1 and the coefficient within the bar).

The Fourier values: the maximum of a bin is the exact integer max q, sig, the 64-point transform and the normalisation are
float64 (1e-13), and 512 f <= 512 is rounded once: FOURIER_BAR = 2 * 512 u, PROVIDED every pixel falls into the bin float64 gives
it.  The kernel's bin is floorf(atan2f(fp32(Ny), fp32(Nx)) * fp32(64 / 2 pi) + 0.5f): the conversions move the angle by at most u
rad, atan2f by 2 ulp of a value below pi (2 * 2^-22 = 4.8e-7 rad; times 64 / 2 pi: 5.5e-6 bins with the conversions), the rounded constant, product and sum by 3 half-ulps of
a value below 33 (5.8e-6 bins): 1.13e-5 bins in all, below the 2^-16 = 1.5e-5 bins that `bin_clearance` of every case exceeds
(tests/test_cpu_lfd_host.py).
"""
import math

import numpy as np

U = 2.0 ** -24
MAX_N = 10
NM = [(n, m) for n in range(1, MAX_N + 1) for m in range(n & 1, n + 1, 2)]      # the order of the 35 Zernike values
N_FOURIER, BINS, COEFS, DESC_BYTES, VIEWS = 10, 64, 45, 48, 10
assert len(NM) == 35


def radial_coefficients(n, m):
    """[(coefficient, power of rho)] of R_nm, highest power first: (-1)^s (n-s)! / (s! ((n+m)/2-s)! ((n-m)/2-s)!) rho^(n-2s)."""
    f = math.factorial
    return [((-1) ** s * f(n - s) // (f(s) * f((n + m) // 2 - s) * f((n - m) // 2 - s)), n - 2 * s) for s in range((n - m) // 2 + 1)]


DESC_BAR = {}
for _n, _m in NM:
    _S = sum(abs(c) for c, _ in radial_coefficients(_n, _m))
    DESC_BAR[_n, _m] = 512 * (1.001 * U * _S * (5 * ((_n - _m) // 2) + max(0, 6 * _m - 3) + 1) + 2.0 ** -32) + 512 * U
FOURIER_BAR = 2 * 512 * U
COEF_BAR = np.array([DESC_BAR[nm] for nm in NM] + [FOURIER_BAR] * N_FOURIER)      # per coefficient, in the order of `coef`


# ---- the descriptor, float64, from the formulas ------------------------------------------------------------------------------------
def _pixels(mask):
    ys, xs = np.nonzero(np.asarray(mask))
    return xs.astype(np.int64), ys.astype(np.int64)


def _fourier(sig):
    tot = sig.sum()
    if tot == 0:
        return np.zeros(N_FOURIER)
    b = np.arange(BINS)
    return np.array([abs((sig * np.exp(-2j * np.pi * k * b / BINS)).sum()) / tot for k in range(1, N_FOURIER + 1)])


def describe_float64(mask):
    """(coef float64 [45] = 512 z, 512 f unrounded; bytes uint8 [48]; status) of one mask [R,R]."""
    xs, ys = _pixels(mask)
    count = xs.size
    if count == 0:
        return np.zeros(COEFS), np.zeros(DESC_BYTES, dtype=np.uint8), 1
    dx, dy = xs - xs.sum() / count, ys - ys.sum() / count
    r = np.hypot(dx, dy)
    rmax = max(0.5, r.max())
    rho, theta = r / rmax, np.arctan2(dy, dx)
    z = []
    for n, m in NM:
        R = sum(c * rho ** k for c, k in radial_coefficients(n, m))
        z.append(abs((R * np.exp(-1j * m * theta)).sum()) / count)
    b = np.floor(BINS * theta / (2 * np.pi) + 0.5).astype(np.int64) % BINS
    sig = np.zeros(BINS)
    np.maximum.at(sig, b, rho)
    coef = 512 * np.concatenate([np.array(z), _fourier(sig)])
    return coef, to_bytes(coef), 0


def to_bytes(coef):
    out = np.zeros(DESC_BYTES, dtype=np.uint8)
    out[:COEFS] = np.minimum(255, np.rint(coef)).astype(np.uint8)
    return out


def bin_clearance(mask):
    """The smallest distance, in bins, of a set pixel's 64 theta / 2 pi from a bin boundary (float64); the pixel AT the centroid,
    whose rho is 0 in whatever bin, is left out.  inf for an empty mask."""
    xs, ys = _pixels(mask)
    if xs.size == 0:
        return math.inf
    nx, ny = xs * xs.size - xs.sum(), ys * ys.size - ys.sum()
    keep = (nx != 0) | (ny != 0)
    if not keep.any():
        return math.inf
    pos = BINS * np.arctan2(ny[keep].astype(np.float64), nx[keep].astype(np.float64)) / (2 * np.pi) + 0.5
    return float(np.abs(pos - np.rint(pos)).min())


def near_half(coef, bar=COEF_BAR):
    """bool [45]: the float64 value lies within the bar of a half-integer, so fp32 may round it to the other byte."""
    return np.abs(coef - (np.floor(coef) + 0.5)) <= bar


# ---- the descriptor, the kernel's fp32 scheme ----------------------------------------------------------------------------------------
def describe_fp32(mask):
    """coef float32 [45] of one non-empty mask by the evaluation scheme of the contract: exact integers, fp32 per pixel without
    fused operations, exact integer sums of the terms scaled by 2^32, a float64 tail."""
    f32 = np.float32
    xs, ys = _pixels(mask)
    count = xs.size
    nx, ny = xs * count - xs.sum(), ys * count - ys.sum()
    q = nx * nx + ny * ny
    Qe = max(float(q.max()), 0.25 * count * count)
    inv, inv2 = f32(1.0 / math.sqrt(Qe)), f32(1.0 / Qe)
    wr, wi = nx.astype(f32) * inv, -(ny.astype(f32) * inv)
    t = q.astype(np.uint64).astype(f32) * inv2
    Wr, Wi = [np.ones_like(wr), wr], [np.zeros_like(wr), wi]
    for k in range(2, MAX_N + 1):
        Wr.append(Wr[k - 1] * wr - Wi[k - 1] * wi)
        Wi.append(Wr[k - 1] * wi + Wi[k - 1] * wr)
    coef = np.zeros(COEFS, dtype=f32)
    for idx, (n, m) in enumerate(NM):
        cs = [c for c, _ in radial_coefficients(n, m)]
        P = np.full_like(t, f32(cs[0]))
        for c in cs[1:]:
            P = P * t + f32(c)
        re = int(np.rint((P * Wr[m]).astype(np.float64) * 2.0 ** 32).astype(np.int64).sum())
        im = int(np.rint((P * Wi[m]).astype(np.float64) * 2.0 ** 32).astype(np.int64).sum()) if m else 0
        coef[idx] = f32(512.0 * (math.sqrt(float(re) * float(re) + float(im) * float(im)) / 2.0 ** 32 / count))
    ang = np.arctan2(ny.astype(f32), nx.astype(f32))
    b = np.floor(ang * f32(10.18591636) + f32(0.5)).astype(np.int64) % BINS
    qb = np.zeros(BINS, dtype=np.int64)
    np.maximum.at(qb, b[q > 0], q[q > 0])
    coef[35:] = (512.0 * _fourier(np.sqrt(qb / Qe))).astype(f32)
    return coef


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def _grid(R):
    y, x = np.mgrid[0:R, 0:R]
    return x.astype(np.float64), y.astype(np.float64)


def _ellipse(R, cx, cy, a, b, angle):
    x, y = _grid(R)
    c, s = math.cos(angle), math.sin(angle)
    u, v = (x - cx) * c + (y - cy) * s, -(x - cx) * s + (y - cy) * c
    return ((u / a) ** 2 + (v / b) ** 2 <= 1).astype(np.uint8)


def _rect(R, x0, y0, w, h):
    m = np.zeros((R, R), dtype=np.uint8)
    m[y0:y0 + h, x0:x0 + w] = 1
    return m


def _ring(R, cx, cy, r0, r1):
    x, y = _grid(R)
    d = np.hypot(x - cx, y - cy)
    return ((d > r0) & (d <= r1)).astype(np.uint8)


def _build_cases():
    c = {}
    c["empty16"] = np.zeros((16, 16), dtype=np.uint8)
    c["pixel16"] = _rect(16, 5, 9, 1, 1)                                      # rmax floor: Q = 0
    c["pair16"] = _rect(16, 7, 7, 2, 1)                                       # rmax = 0.5 exactly at the floor
    c["full16"] = np.full((16, 16), 255, dtype=np.uint8)                      # the whole frame; centroid between pixels
    c["bar16"] = _rect(16, 2, 8, 12, 1)                                       # a thin bar: most bins stay empty
    c["two16"] = _rect(16, 1, 2, 4, 3) | _rect(16, 10, 9, 3, 5)               # two components
    c["disc33"] = _ellipse(33, 16, 16, 11.3, 11.3, 0.0)
    c["ring33"] = _ring(33, 16, 16, 6.2, 13.1)
    c["border33"] = _rect(33, 0, 20, 13, 13) | _rect(33, 0, 0, 33, 2)         # touches three borders
    c["between33"] = _rect(33, 9, 11, 4, 7)                                   # centroid at (10.5, 14): between pixels in x
    c["L33"] = _rect(33, 5, 4, 6, 24) | _rect(33, 5, 22, 20, 6)
    c["ellipse64"] = _ellipse(64, 31.3, 32.2, 27.0, 9.0, 0.0)
    c["ellipse64_rot"] = _ellipse(64, 31.3, 32.2, 27.0, 9.0, 0.6)
    c["square64"] = _rect(64, 12, 15, 37, 37)
    c["two64"] = _ellipse(64, 16, 20, 9, 6, 0.3) | _rect(64, 35, 38, 20, 11)
    c["ellipse256"] = _ellipse(256, 127.3, 130.4, 102.0, 34.0, 0.0)
    c["ellipse256_rot"] = _ellipse(256, 127.3, 130.4, 102.0, 34.0, 0.6)
    c["disc256"] = _ellipse(256, 128, 128, 90.5, 90.5, 0.0)
    c["square256"] = _rect(256, 40, 50, 150, 150)
    c["ring256"] = _ring(256, 128, 128, 60.3, 100.7)
    c["L256"] = _rect(256, 30, 20, 50, 200) | _rect(256, 30, 170, 180, 50)
    c["bar256"] = _rect(256, 28, 120, 200, 3)
    c["block256"] = _rect(256, 100, 77, 3, 3)
    return c


CASES = _build_cases()
# what tests/test_gpu_lfd.py runs on the GPU, batched per resolution; the 256^2 masks beyond the first serve the host tests only
GPU_CASES = [k for k in CASES if CASES[k].shape[0] < 256] + ["ellipse256_rot"]
_REF = {}


def reference(name):
    """describe_float64 of a case, computed once."""
    if name not in _REF:
        _REF[name] = describe_float64(CASES[name])
    return _REF[name]


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
def matrix_numpy(x, y, perm):
    """int64 [nx,ny] of x uint8 [nx,L,10,48], y uint8 [ny,L,10,48], perm [G,10]: the contract's minimum, every term formed."""
    x, y, perm = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64), np.asarray(perm, dtype=np.int64)
    out = np.zeros((x.shape[0], y.shape[0]), dtype=np.int64)
    v = np.arange(VIEWS)
    for i in range(x.shape[0]):
        for j in range(y.shape[0]):
            tab = np.abs(x[i][:, None, :, None, :] - y[j][None, :, None, :, :]).sum(axis=-1)      # [la, lb, v, u]
            out[i, j] = min(int(tab[:, :, v, perm[g]].sum(axis=-1).min()) for g in range(perm.shape[0]))
    return out


def random_models(n, L, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, L, VIEWS, DESC_BYTES), dtype=np.uint8)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def box_mesh(sx, sy, sz):
    """(verts float64 [8,3], faces int64 [12,3]) of the box [-sx/2, sx/2] x [-sy/2, sy/2] x [-sz/2, sz/2]."""
    v = np.array([[x, y, z] for x in (-sx / 2, sx / 2) for y in (-sy / 2, sy / 2) for z in (-sz / 2, sz / 2)], dtype=np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], dtype=np.int64)
    return v, f
