"""The training dropout mask restated on the host, from the comment in csrc/md_common.h ("Counter-based dropout mask") -- plain
numpy, no GPU, no hip_ops.  The GPU tests (tests/test_gpu_dropout.py) tie every kernel that regenerates the mask to THIS file bit
for bit, so a changed constant, field order or quad index can no longer pass by changing in all five users at once.

The contract:
  thr16 = (uint32)(p * 65536 + 0.5) in fp32, clamped to [0, 65535]; thr16 == 0 means "no dropout at all" (identity) in every user
  element (b, channel, pos) of a tensor with c_total channels (`channel` counts inside the concatenated tensor: c_off + c):
      n     = b * c_total + channel
      q     = (n >> 2) * P + pos                                   one 64-bit word per 4 consecutive channels of one position
      word  = SplitMix64 finaliser of  seed + (q + 1) * 0x9E3779B97F4A7C15   (all mod 2^64)
      field = (word >> 16 * (n & 3)) & 0xFFFF                       channel-in-quad 0 sits in the LOW 16 bits
      kept  = field >= thr16
  kept values are multiplied by scale = 1 / (1 - p) in fp32 (one division, one multiply per value), dropped ones are exactly 0.

Also here: the case tables of tests/test_cpu_dropout.py and tests/test_gpu_dropout.py.
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB
M64 = (1 << 64) - 1
U64_MAX = M64


def thr16(p):
    """md_drop_thr16: the fp32 expression p * 65536 + 0.5, truncated, clamped to [0, 65535]."""
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    if t <= np.float32(0.0):
        return 0
    if t >= np.float32(65535.0):
        return 65535
    return int(t)


def scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def hash_word_int(seed, q):
    """The hash word with Python integers (the form the pinned literals of test_cpu_dropout.py were computed with)."""
    z = (seed + (q + 1) * GOLDEN) & M64
    z = ((z ^ (z >> 30)) * MIX1) & M64
    z = ((z ^ (z >> 27)) * MIX2) & M64
    return z ^ (z >> 31)


def hash_words(seed, q):
    """The same for a uint64 array of quad indices."""
    q = np.asarray(q, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + (q + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        return z ^ (z >> np.uint64(31))


def fields(seed, B, c_total, c_off, C, P):
    """The 16-bit uniform of every element: uint32 [B, C, P]."""
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    ch = np.arange(c_off, c_off + C, dtype=np.uint64)[None, :, None]
    pos = np.arange(P, dtype=np.uint64)[None, None, :]
    n = b * np.uint64(c_total) + ch
    q = (n >> np.uint64(2)) * np.uint64(P) + pos
    w = hash_words(seed, q)
    return ((w >> (np.uint64(16) * (n & np.uint64(3)))) & np.uint64(0xFFFF)).astype(np.uint32)


def keep(seed, p, B, c_total, c_off, C, P):
    """bool [B, C, P]: the elements the mask keeps.  All true where thr16(p) == 0."""
    t = thr16(p)
    if t == 0:
        return np.ones((B, C, P), dtype=bool)
    return fields(seed, B, c_total, c_off, C, P) >= np.uint32(t)


def factor(seed, p, B, c_total, c_off, C, P):
    """float32 [B, C, P] (NCDHW order): scale(p) where kept, 0 where dropped; all ones where thr16(p) == 0."""
    k = keep(seed, p, B, c_total, c_off, C, P)
    s = scale(p) if thr16(p) else np.float32(1)
    return np.where(k, s, np.float32(0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------
THR16_TABLE = ((0.1, 6554), (0.3, 19661), (0.5, 32768), (2.0 ** -17, 1), (1e-6, 0), (0.99999, 65535))

# statistical properties of the restatement (test_cpu_dropout.py)
STAT_SHAPE = dict(B=4, c_total=32, c_off=0, C=32, P=4096)
STAT_SEEDS = (0, 1, 2, 3, 77, 99, 2 ** 62 - 2, 2 ** 62 - 1, 2 ** 64 - 1, 0x1234567890ABCDE)
STAT_PS = (0.1, 0.3, 0.5)
STAT_Z = 5.0

# md_dropout_scale against factor(): (B, C, P, c_total, c_off)
SCALE_SHAPES = ((3, 16, 210, 24, 8),        # P = 5*6*7, not a multiple of 64; the part starts mid-tensor
                (1, 8, 64, 8, 0),
                (2, 8, 4096, 40, 32))
GPU_SEEDS = (0, 1, 2 ** 62 - 1, U64_MAX)    # the last: the largest value a uint64_t argument takes
SCALE_PS = (2.0 ** -17, 0.1, 0.3, 0.5, 0.99999)
P_IDENTITY = 1e-6                           # thr16 == 0


def phi_z(a, b):
    """phi coefficient of two equally shaped bool arrays times sqrt(n): ~N(0, 1) for independent ones."""
    a, b = np.asarray(a, dtype=bool).ravel(), np.asarray(b, dtype=bool).ravel()
    n = a.size
    n11 = float(np.count_nonzero(a & b))
    n1_, n_1 = float(np.count_nonzero(a)), float(np.count_nonzero(b))
    den = np.sqrt(n1_ * (n - n1_) * n_1 * (n - n_1))
    return (n * n11 - n1_ * n_1) / den * np.sqrt(n)


def rate_z(k, t16):
    """The keep rate of a bool array against 1 - thr16 / 65536, in binomial sigmas."""
    q = 1.0 - t16 / 65536.0
    n = k.size
    return (np.count_nonzero(k) / n - q) / np.sqrt(q * (1.0 - q) / n)


def stat_pairs(seed, p):
    """name -> (a, b): the pairs of masks whose correlation the CPU test bounds, on STAT_SHAPE."""
    k = keep(seed, p, **STAT_SHAPE)
    k1 = keep((seed + 1) & M64, p, **STAT_SHAPE)
    return k, {
        "channels 2k / 2k+1": (k[:, 0::2], k[:, 1::2]),
        "neighbouring positions": (k[:, :, :-1], k[:, :, 1:]),
        "neighbouring quads": (k[:, :-4], k[:, 4:]),
        "neighbouring samples": (k[:-1], k[1:]),
        "seed / seed+1": (k, k1),
    }
