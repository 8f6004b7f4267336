"""Cases and restatements of classifier-free guidance (md_cfg_combine / md_cfg_rescale, class dropout), shared by
tests/test_cpu_cfg_host.py, tests/test_gpu_cfg.py and tools/gen_golden_cfg.py.  numpy / torch on the CPU only.

The combine contract is out = fmaf(w, ec - eu, eu) in float32.  Its float64 restatement keeps the contract's float32 subtraction
and forms w*d + eu in double (the product of two floats is exact there, the sum is rounded once to 53 bits); rounding that to
float32 is a second rounding, so it can differ from the fused float32 result by one ulp, and by no more.
"""
import numpy as np
import torch

BATCHES = (1, 3)
SIZES = (1, 500, 4 * 16 ** 3)            # one value; fewer values than one workgroup moves; a small grid, several workgroups
SIZES_UNALIGNED = (499, 1027)            # n % 4 != 0: rows that are not 16-byte aligned, the one-value-at-a-time path with a tail
W_VALUES = (0.0, 1.0, 3.0, -0.5, 7.5)
PHIS = (0.7, 1.0)
BAR_MARGIN = 4.0                         # the rescale bar is BAR_MARGIN x the float32 restatement's distance from float64


def case_id(B, n):
    return f"B{B}_n{n}"


def combine_inputs(B, n, seed=0):
    """(ec, eu float32 [B, n], w float32 [B]) of a case: unit normal halves that share most of their signal (as the two halves of a
    guided evaluation do), w cycling through W_VALUES from a per-case offset so that every value meets every shape."""
    g = torch.Generator().manual_seed(1000 * B + n + 7919 * seed)
    common = torch.randn((B, n), generator=g)
    ec = (common + 0.3 * torch.randn((B, n), generator=g)).numpy().astype(np.float32)
    eu = (common + 0.3 * torch.randn((B, n), generator=g)).numpy().astype(np.float32)
    off = (B + n + seed) % len(W_VALUES)
    w = np.array([W_VALUES[(off + b) % len(W_VALUES)] for b in range(B)], dtype=np.float32)
    return ec, eu, w


def combine_restated(ec, eu, w):
    """float64 [B, n]: w*d + eu in double with d = ec - eu taken in float32, as the contract takes it."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (ec.astype(np.float32) - eu.astype(np.float32)).astype(np.float64)
        return w.astype(np.float64)[:, None] * d + eu.astype(np.float64)


def ulp_distance(a, b):
    """Units in the last place between two float32 arrays, elementwise (int64); both must be finite."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def rescale_factor_restated(ec, out, phi, dtype=np.float64):
    """[B] factors phi*std(ec)/std(out) + (1 - phi) in `dtype`, population std over all n values of a sample; 1 where std(out) is 0
    or a statistic is not finite (the sample stays unscaled)."""
    ec, out = ec.astype(dtype), out.astype(dtype)
    f = np.ones(ec.shape[0], dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(ec.shape[0]):
            sc, so = ec[b].std(dtype=dtype), out[b].std(dtype=dtype)
            v = dtype(phi) * sc / so + (dtype(1) - dtype(phi))
            if so > 0 and np.isfinite(v):
                f[b] = v
    return f


def rescale_bar(ec, out, phi):
    """The bar of the per-sample factor for these operands: BAR_MARGIN x the largest relative distance of the float32 restatement
    from the float64 one."""
    f64 = rescale_factor_restated(ec, out, phi, np.float64)
    f32 = rescale_factor_restated(ec, out, phi, np.float32).astype(np.float64)
    return BAR_MARGIN * float(np.max(np.abs(f32 - f64) / np.abs(f64)))


def draw_order_restated(shape, N, class_dropout, y, null_class, generator):
    """The draws of one training loss evaluation on a CPU generator, in the contract's order: timesteps, noise, and only with class
    ids and class_dropout > 0 one uniform per sample; returns (labels, noise, y after dropout or None)."""
    labels = torch.randint(0, N, (shape[0],), generator=generator)
    noise = torch.randn(shape, generator=generator)
    if y is None or class_dropout <= 0:
        return labels, noise, y
    u = torch.rand(shape[0], generator=generator)
    return labels, noise, torch.where(u < class_dropout, torch.full_like(y, null_class), y)
