"""Inputs, float64 references, rounding-count bounds and fp32 emulations for the direct tests of the streaming kernels:
csrc/norm.hip (GroupNorm), csrc/train.hip (the training step) and the small kernels of csrc/elementwise.hip.
tests/test_gpu_stream_f64.py runs the cases on the GPU; tests/test_cpu_stream_cases.py proves on the CPU that the emulation of
every kernel lies inside its bound, that one-line mutations of it land far outside, and that every case is in the regime its name
claims.  Plain helper module: no fixtures, no GPU, only torch.

Conventions
  * inputs are fp32 tensors from seeded generators; every reference is float64 arithmetic on those fp32 values and on the host
    scalars the reference program (torch.optim.Adam, models/ema.py, nn.GroupNorm, layers.get_timestep_embedding) would use;
  * u = 2^-24 is the unit roundoff of fp32 (half an ulp): one fp32 operation is off by at most u times its result;
  * every bound is a function next to its case whose docstring counts the roundings of the kernel source it covers.  A bound is
    first order in u; the (1 + 2^-10) factor `SECOND_ORDER` pays for the products of two error terms.
"""
import math

import torch

U = 2.0 ** -24
D53 = 2.0 ** -53
SECOND_ORDER = 1.0 + 2.0 ** -10
F32 = torch.float32
F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(x):
    """The fp32 value of a Python scalar, as a Python float (what a `float` parameter of the C ABI or a torch scalar cast holds)."""
    return float(torch.tensor(x, dtype=F32))


def split_bf16(x):
    """md_split on the host: hi = bf16(x) (RNE), lo = bf16(x - hi)."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def to_f32b(x):
    """[B][C][P] -> F32B [B][C/8][P][8]."""
    B, C, P = x.shape
    return x.reshape(B, C // 8, 8, P).permute(0, 1, 3, 2).contiguous()


def from_s16b(t):
    """S16B [B][C/8][2][P][8] bf16 -> (hi, lo) as [B][C][P] bf16."""
    B, G, _, P, _ = t.shape
    hi = t[:, :, 0].permute(0, 1, 3, 2).reshape(B, G * 8, P)
    lo = t[:, :, 1].permute(0, 1, 3, 2).reshape(B, G * 8, P)
    return hi, lo


def ulp_distance(a, b):
    """Largest distance in units of the last place between two fp32 tensors of finite values."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a.float()) - key(b.float())).abs().max()) if a.numel() else 0


def butterfly(x, bits):
    """The `v += __shfl_xor(v, o)` ladder over the last axis, in the dtype of x: every lane ends with the same tree sum."""
    idx = torch.arange(x.shape[-1])
    for b in bits:
        x = x + x[..., idx ^ b]
    return x


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm: md_gn_stats -> md_gn_finalize -> md_gn_apply
# ---------------------------------------------------------------------------------------------------------------
GN_GROUPS = 32
GN_EPS = 1e-6
GN_CHUNK = 2048      # positions per workgroup   (norm.hip GN_CHUNK)
GN_STRIDE = 128      # positions per unrolled item: 256 threads, two lanes (the halves of 8 channels) per position
GN_ITEMS = 16        # items per thread          (norm.hip GN_ITEMS)
# The largest group |mean| / std any GroupNorm input reaches in the small res64 / res128 nets (sensitised and trained-like weights,
# synthetic inputs; test_cpu_stream_cases.test_network_groupnorm_offsets measures it with the oracle) is 1.59.  Twice that, because
# trained weights drift, rounded up to a power of two, is the ratio at which GroupNorm still has to meet the project's 1e-5.
GN_NETWORK_RATIO = 1.59
GN_SERVED_RATIO = 4
GN_SERVED_TOL = 1e-5
GN_KS, GN_KQ = 12, 13   # the caps on the fp32 roundings of a sum / a sum of squares that the bound grants (see gn_bound)


def _gn_case(name, B, parts, grid, seed, ratio=0.0, spread=0.0, const_group=None, owns=""):
    P = grid[0] * grid[1] * grid[2]
    C = sum(parts)
    cpg = C // GN_GROUPS
    g = _gen(seed)
    x = torch.randn(B, C, P, generator=g)
    if spread:      # channel means that differ inside a group: +-spread, alternating with the channel index inside its group
        sign = ((torch.arange(C) % cpg) % 2).float() * 2 - 1
        x = x + spread * sign[None, :, None]
    if ratio:       # every group standardised, then one offset: mean / std = ratio in every group
        xg = x.double().reshape(B, GN_GROUPS, -1)
        xg = (xg - xg.mean(-1, keepdim=True)) / xg.var(-1, unbiased=False, keepdim=True).sqrt()
        x = (xg + float(ratio)).float().reshape(B, C, P)
    if const_group is not None:
        x[:, const_group * cpg:(const_group + 1) * cpg] = 3.25     # 3.25 k and 3.25^2 k are exact in fp32 for every k that occurs
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    return dict(name=name, B=B, parts=tuple(parts), grid=tuple(grid), P=P, C=C, cpg=cpg, x=x.contiguous(), gamma=gamma, beta=beta,
                ratio=float(ratio), spread=float(spread), const_group=const_group, owns=owns)


def gn_cases():
    cs = [
        _gn_case("cpg1-P64", 1, (32,), (4, 4, 4), 1, owns="cpg = 1, one block"),
        _gn_case("concat40+56-P45", 2, (40, 56), (3, 3, 5), 3, owns="part boundary inside group 13; per-part c_off"),
        _gn_case("chunk-P2047", 1, (64,), (1, 23, 89), 4, owns="one position short of the chunk"),
        _gn_case("chunk-P2048", 1, (64,), (8, 16, 16), 5, owns="exactly one chunk"),
        _gn_case("chunk-P2049", 1, (64,), (1, 3, 683), 6, owns="one position into the second block"),
        _gn_case("cpg65-P8", 1, (2080,), (2, 2, 2), 7, owns="cpg = 65: finalize's strided loop"),
    ]
    for tag, B, parts, grid, seed in (("P210", 3, (96,), (5, 6, 7), 10), ("P4100", 1, (32,), (4, 25, 41), 20)):
        cs.append(_gn_case(f"{tag}-ratio0", B, parts, grid, seed, owns="cpg = 3 straddles 8-channel blocks, odd P, odd batch"
                           if tag == "P210" else "three blocks adding onto one double"))
        cs.append(_gn_case(f"{tag}-ratio4", B, parts, grid, seed + 3, ratio=GN_SERVED_RATIO))
        cs.append(_gn_case(f"{tag}-ratio8", B, parts, grid, seed + 1, ratio=8))
        cs.append(_gn_case(f"{tag}-ratio64", B, parts, grid, seed + 2, ratio=64))
        cs.append(_gn_case(f"{tag}-const", B, parts, grid, seed + 4, const_group=5))
    cs.append(_gn_case("P210-chanmeans", 3, (96,), (5, 6, 7), 13, spread=2.0))   # cpg = 1 at (32,): only the 210 row has channels to differ
    return cs


def gn_group_stats(case):
    """float64 (mean, var, n, S1 = sum |x|, S2 = sum x^2) per (b, group)."""
    B, C, P, cpg = case["B"], case["C"], case["P"], case["cpg"]
    xg = case["x"].double().reshape(B, GN_GROUPS, cpg * P)
    n = cpg * P
    mean = xg.sum(-1) / n
    var = ((xg - mean[..., None]) ** 2).sum(-1) / n          # two-pass: no cancellation in the reference
    if case["const_group"] is not None:
        assert float(var[:, case["const_group"]].abs().max()) == 0.0
    return mean, var, n, xg.abs().sum(-1), (xg * xg).sum(-1)


def gn_reference(case, silu, norm=True):
    """float64 GroupNorm(32, C, eps) (+ SiLU) of the case, and the per-channel quantities the kernels store."""
    B, C, P, cpg = case["B"], case["C"], case["P"], case["cpg"]
    x = case["x"].double()
    mean, var, n, S1, S2 = gn_group_stats(case)
    eps = f32(GN_EPS)                                         # md_gn_finalize receives eps as a float
    rstd = 1.0 / torch.sqrt(var + eps)
    mean_c = mean.repeat_interleave(cpg, 1)                   # [B][C]
    rstd_c = rstd.repeat_interleave(cpg, 1)
    a = rstd_c * case["gamma"].double()[None]
    beta = case["beta"].double()[None].expand(B, C)
    y = (x - mean_c[..., None]) * a[..., None] + beta[..., None] if norm else x
    out = y / (1.0 + torch.exp(-y)) if silu else y
    return dict(mean=mean_c, rstd=rstd_c, a=a, beta=beta, c=beta - mean_c * a, y=y, out=out)


def gn_stat_roundings(P):
    """(fp32 roundings a sum passes through, the same for a sum of squares) in md_gn_stats_kernel, for P positions.

    A thread owns 4 channels of one position per item and GN_ITEMS = 16 items, 128 positions apart: min(16, ceil(P'/128)) values
    per accumulator (P' = min(P, 2048)), i.e. that many minus one sequential fp32 adds (the first lands on 0 and is exact).  Then
    5 `__shfl_xor` levels (32 .. 2) in fp32.  The square adds one rounding (none where the compiler contracts it into an fma).
    Everything after that -- the 4 waves, the blocks (atomicAdd), md_gn_finalize -- is double.

    The count is 15 + 5 = 20 (sums) and 21 (squares) for a full chunk.  The bound does NOT grant that much: it caps the counts at
    GN_KS = 12 and GN_KQ = 13, the worst case the tests were specified with (which assumed 8 values per accumulator).  Below the
    cap the count is a true worst case; at the cap it is a demand: 20 roundings of a random sum do not line up, their root sum
    square is sqrt(20) u, and a kernel that needs more than 12 u has lost accuracy somewhere."""
    seq = min(GN_ITEMS, -(-min(P, GN_CHUNK) // GN_STRIDE)) - 1
    return min(seq + 5, GN_KS), min(seq + 6, GN_KQ)


def gn_param_bounds(case):
    """Bounds on what md_gn_finalize stores, per (b, channel): dict(mean, rstd, a, c) of |stored fp32 - float64|.

    md_gn_stats: |ds| <= Ks u S1, |dq| <= Kq u S2 per group (gn_stat_roundings; S1 = sum |x|, S2 = sum x^2 = n (var + mean^2)).
    Double part: 4 waves + one atomicAdd per block + ceil(cpg/64) + 6 adds in finalize + the 5 operations of mean / var: `dbl`.
      mean = s / n                   |dmean| <= (Ks u + dbl) S1 / n                         (+ u |mean| once stored as a float)
      var  = q / n - mean^2          |dvar|  <= (Kq u + dbl) (var + eps) (1 + mean^2 / (var + eps)) + 2 |mean| |dmean| + dmean^2
                                     -- the offset factor 1 + mean^2 / var: the cancellation of q/n against mean^2
      rstd = (float)(1/sqrt(var+eps)) exact interval over var +- dvar (clamped at 0 like the kernel), + u rstd for the cast
      a    = rstd * gamma            one fp32 product: + u |a|
      c    = (float)(beta - mean a)  double arithmetic on the stored a: |a| |dmean| + |mean| |da| + u |c|."""
    B, C, P, cpg = case["B"], case["C"], case["P"], case["cpg"]
    mean, var, n, S1, S2 = gn_group_stats(case)
    ks, kq = gn_stat_roundings(P)
    nblk = -(-P // GN_CHUNK)
    dbl = (4 + nblk + -(-cpg // 64) + 6 + 5) * D53
    eps = f32(GN_EPS)
    dmean = (ks * U + dbl) * S1 / n
    offset = 1.0 + mean * mean / (var + eps)
    dvar = (kq * U + dbl) * (var + eps) * offset + 2 * mean.abs() * dmean + dmean * dmean
    r = 1.0 / torch.sqrt(var + eps)
    rlo = 1.0 / torch.sqrt(var + dvar + eps)
    rhi = 1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + eps)
    drstd = torch.maximum(rhi - r, r - rlo) + U * rhi
    rep = lambda t: t.repeat_interleave(cpg, 1)
    gam = case["gamma"].double().abs()[None]
    mean_c, dmean_c, r_c, rhi_c, drstd_c = rep(mean), rep(dmean), rep(r), rep(rhi), rep(drstd)
    da = gam * drstd_c + U * gam * rhi_c
    a = gam * r_c
    cref = (case["beta"].double()[None] - mean_c * r_c * case["gamma"].double()[None]).abs()
    dc = a * dmean_c + mean_c.abs() * da + dmean_c * da + U * (cref + a * dmean_c + mean_c.abs() * da)
    return dict(mean=(dmean_c + U * mean_c.abs()) * SECOND_ORDER, rstd=drstd_c * SECOND_ORDER, a=da * SECOND_ORDER,
                c=dc * SECOND_ORDER, dmean=dmean_c, offset=offset)


def gn_bound(case, silu, norm=True):
    """Elementwise bound on |hi + lo - float64| of md_gn_apply's output.

    y = (x - mean) * a + beta in fp32 from the stored (mean, a, beta):
      stored parameters     |a| dmean + |x - mean| da                            (gn_param_bounds)
      x - mean              1 rounding, carried through the product: u |x - mean| |a|
      * a, + beta           2 roundings (1 where contracted into an fma): u |x - mean| |a| + u |y|
    SiLU y / (1 + expf(-y)):  |silu'| <= 1.1 carries dy; expf is within 1 ulp = 2 u, the add and the division 1 u each: 4 u |out|.
    bf16 split: hi = bf16(v), lo = bf16(v - hi): bf16 keeps 8 significant bits (unit roundoff 2^-8), v - hi is exact in fp32, so
    |v - (hi + lo)| <= 2^-8 |v - hi| <= 2^-16 |v| -- the floor of the operand format, 256 u; it dominates wherever the group mean
    is small against its spread, which is why the stored parameters are checked on their own (gn_param_bounds).
    norm = False leaves the floor (and SiLU) only."""
    ref = gn_reference(case, silu, norm)
    if norm:
        pb = gn_param_bounds(case)
        d = (case["x"].double() - ref["mean"][..., None]).abs()
        A = ref["a"].abs()[..., None]
        dy = A * pb["mean"][..., None] + d * pb["a"][..., None] + pb["mean"][..., None] * pb["a"][..., None] \
            + U * (2 * d * A + ref["y"].abs())
    else:
        dy = torch.zeros_like(ref["y"])
    dout = 1.1 * dy + 4 * U * ref["out"].abs() if silu else dy
    return (dout + 2.0 ** -16 * (ref["out"].abs() + dout)) * SECOND_ORDER


def emulate_gn_stats(x, mut=None):
    """md_gn_stats in torch: [B][C][P] fp32 -> double (sum, sumsq) [B][C].  The summation tree of the kernel: per 2048-position
    block, 128 accumulators take positions j, j + 128, ... in order (fp32), the 32 accumulators of a wave meet in a 5-level xor
    butterfly (fp32), waves and blocks add in double.  mut = 'drop_tail': the last position is not read."""
    B, C, P = x.shape
    if mut == "drop_tail":
        x = x.clone()
        x[..., P - 1] = 0.0
    nblk = -(-P // GN_CHUNK)
    xp = torch.zeros(B, C, nblk * GN_CHUNK, dtype=F32)
    xp[..., :P] = x
    xp = xp.reshape(B, C, nblk, GN_ITEMS, GN_STRIDE)
    s = torch.zeros(B, C, nblk, GN_STRIDE, dtype=F32)
    q = torch.zeros(B, C, nblk, GN_STRIDE, dtype=F32)
    for i in range(GN_ITEMS):
        v = xp[..., i, :]
        s = s + v
        q = q + v * v
    s = butterfly(s.reshape(B, C, nblk, 4, 32), (16, 8, 4, 2, 1))[..., 0]
    q = butterfly(q.reshape(B, C, nblk, 4, 32), (16, 8, 4, 2, 1))[..., 0]
    return s.double().sum((-1, -2)), q.double().sum((-1, -2))


def emulate_gn(case, silu, mut=None):
    """The three kernels in torch with their arithmetic order.  Returns dict(mean, a, beta, rstd, c: fp32 [B][C]; hi, lo: bf16).
    Mutations (one at a time): 'drop_tail', 'padded_n' (n counts the padded chunk), 'neighbour_part' (the group at the concat
    boundary reads one channel of the neighbouring part instead of its own), 'swap_pair' (mean and rstd*gamma swapped between
    the two channels of a group)."""
    B, C, P, cpg = case["B"], case["C"], case["P"], case["cpg"]
    x = case["x"]
    s, q = emulate_gn_stats(x, mut)
    if mut == "neighbour_part":
        edge = case["parts"][0]                      # first channel of part 2; its group starts below it
        lo_ch = (edge // cpg) * cpg
        assert lo_ch < edge < lo_ch + cpg
        s, q = s.clone(), q.clone()
        s[:, lo_ch:lo_ch + cpg] = s[:, lo_ch - 1:lo_ch + cpg - 1].clone()
        q[:, lo_ch:lo_ch + cpg] = q[:, lo_ch - 1:lo_ch + cpg - 1].clone()
    n = float(cpg) * float(P if mut != "padded_n" else -(-P // GN_CHUNK) * GN_CHUNK)
    sg = s.reshape(B, GN_GROUPS, cpg).sum(-1)
    qg = q.reshape(B, GN_GROUPS, cpg).sum(-1)
    mean = sg / n
    var = (qg / n - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(var + f32(GN_EPS))).float()
    mean_c, rstd_c = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    a = rstd_c * case["gamma"][None]
    beta = case["beta"][None].expand(B, C)
    c = (beta.double() - mean_c * a.double()).float()
    mean_f = mean_c.float()
    if mut == "swap_pair":
        assert cpg == 2
        perm = torch.arange(C) ^ 1
        mean_f, a = mean_f[:, perm], a[:, perm]
    y = (x - mean_f[..., None]) * a[..., None] + beta[..., None]
    if silu:
        y = y / (1.0 + torch.exp(-y))
    hi, lo = split_bf16(y)
    return dict(mean=mean_f, a=a, beta=beta, rstd=rstd_c, c=c, hi=hi, lo=lo)


def gn_measure(got64, ref64, bound):
    """(per-sample max |got - ref| / max |ref|, max of |got - ref| / bound over the elements)."""
    err = (got64 - ref64).abs()
    B = ref64.shape[0]
    rel = (err.reshape(B, -1).amax(1) / ref64.abs().reshape(B, -1).amax(1).clamp_min(1e-300)).max()
    return float(rel), float((err / bound.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------
# md_linear, md_timestep_embedding, md_ncdhw_to_s16b
# ---------------------------------------------------------------------------------------------------------------
def linear_cases():
    cs = []
    k = 0
    for in_dim in (1, 63, 64, 65, 512):
        for batch in (1, 8, 9, 19):
            out_dim = (5, 510, 512)[k % 3]
            bias, silu = k % 2 == 0, (k // 2) % 2 == 0
            g = _gen(500 + k)
            cs.append(dict(name=f"b{batch}-in{in_dim}-out{out_dim}-{'bias' if bias else 'nobias'}-{'silu' if silu else 'id'}",
                           x=torch.randn(batch, in_dim, generator=g), w=torch.randn(out_dim, in_dim, generator=g) / math.sqrt(in_dim),
                           bias=torch.randn(out_dim, generator=g) if bias else None, silu=silu))
            k += 1
    return cs


def linear_reference(case):
    x = case["x"].double()
    act = x / (1.0 + torch.exp(-x)) if case["silu"] else x
    y = act @ case["w"].double().T
    mag = act.abs() @ case["w"].double().abs().T
    if case["bias"] is not None:
        y = y + case["bias"].double()[None]
        mag = mag + case["bias"].double().abs()[None]
    return y, mag


def linear_bound(case):
    """md_linear_kernel: lane l owns inputs l, l + 64, ...: ceil(in_dim/64) products (1 rounding each, none as an fma) added in
    order (ceil(in_dim/64) roundings, the first onto 0 exact), then 6 `__shfl_xor` levels, then + bias: every product passes
    through at most ceil(in_dim/64) + 1 + 6 + 1 roundings; SiLU on the input adds its 4 u (gn_bound).  Relative to
    sum |act(x) w| + |bias|."""
    _, mag = linear_reference(case)
    k = -(-case["x"].shape[1] // 64) + 1 + 6 + 1 + (4 if case["silu"] else 0)
    return k * U * mag * SECOND_ORDER


def emulate_linear(case):
    x, w = case["x"], case["w"]
    B, I = x.shape
    act = x / (1.0 + torch.exp(-x)) if case["silu"] else x
    seq = -(-I // 64)
    prod = torch.zeros(B, w.shape[0], seq * 64, dtype=F32)
    prod[..., :I] = act[:, None, :] * w[None]
    prod = prod.reshape(B, w.shape[0], seq, 64)
    acc = torch.zeros(B, w.shape[0], 64, dtype=F32)
    for i in range(seq):
        acc = acc + prod[:, :, i]
    y = butterfly(acc, (32, 16, 8, 4, 2, 1))[..., 0]
    return y + case["bias"][None] if case["bias"] is not None else y


TEMB_T = (0.0, 0.999, 500.3, 999.0)
TEMB_DIMS = (4, 7, 128, 129)


def temb_reference(dim):
    """float64 embedding of TEMB_T.  The exponent (float)j * (float)(-ln(1e4)/(half-1)) is an fp32 product in the reference
    program as well (layers.get_timestep_embedding), so it is taken as given; exp, the product with t and sin / cos are float64."""
    half = dim // 2
    neg = torch.tensor(-(math.log(10000.0) / (half - 1)), dtype=F64).float()
    arg = (torch.arange(half, dtype=F32) * neg).double()
    tf = torch.tensor(TEMB_T, dtype=F32).double()[:, None] * torch.exp(arg)[None]
    ref = torch.zeros(len(TEMB_T), dim, dtype=F64)
    ref[:, :half], ref[:, half:2 * half] = torch.sin(tf), torch.cos(tf)
    bound = torch.zeros_like(ref)
    bound[:, :half] = bound[:, half:2 * half] = temb_bound(tf)
    return ref, bound


def temb_bound(tf):
    """expf within 1 ulp (2 u on f), the product t * f 1 u: 3 u |t f| on the argument, which sin and cos pass on with slope <= 1;
    sinf / cosf themselves within 1 ulp of a value <= 1: 2 u.  The odd tail is a stored 0: bound 0."""
    return 3 * U * tf.abs() + 2 * U


def emulate_temb(dim):
    half = dim // 2
    neg = torch.tensor(-(math.log(10000.0) / (half - 1)), dtype=F64).float()
    arg = torch.tensor(TEMB_T, dtype=F32)[:, None] * torch.exp(torch.arange(half, dtype=F32) * neg)[None]
    out = torch.zeros(len(TEMB_T), dim, dtype=F32)
    out[:, :half], out[:, half:2 * half] = torch.sin(arg), torch.cos(arg)
    return out


S16B_CASES = ((3, 8), (4, 8), (13, 16), (3, 16))      # (C, c_pad); P = 210, B = 2


# ---------------------------------------------------------------------------------------------------------------
# md_masked_sq_err, md_grad_sqnorm
# ---------------------------------------------------------------------------------------------------------------
def sq_err_case(name, B, C, grid, seed, mask="random", init=False):
    P = grid[0] * grid[1] * grid[2]
    g = _gen(seed)
    noise = torch.randn(B, C, *grid, generator=g)
    eh = noise + 1e-6 * torch.randn(B, C, *grid, generator=g)         # eps_hat = noise + 1e-6 r: the difference is 10 ulps of noise
    if mask == "random":
        m = (torch.rand(P, generator=g) < 0.3).float()
    elif mask == "zero":
        m = torch.zeros(P)
    else:
        m = None
    sums0 = 1.0 + torch.rand(B, generator=g).double() if init else torch.zeros(B, dtype=F64)
    return dict(name=name, B=B, C=C, grid=grid, P=P, eps_hat=eh, noise=noise, mask=m, sums0=sums0, gscale=0.37)


def sq_err_cases():
    return [sq_err_case("B3-C5-6x10x14", 3, 5, (6, 10, 14), 31),
            sq_err_case("nomask", 2, 1, (6, 10, 14), 32, mask=None),
            sq_err_case("onto-nonzero", 3, 4, (6, 10, 14), 33, init=True),
            sq_err_case("zero-mask", 2, 4, (6, 10, 14), 34, mask="zero"),
            sq_err_case("wrap-C4-40x40x44", 1, 4, (40, 40, 44), 35)]           # C P = 281 600 > 256 * 256 * 4: second trip


def sq_err_reference(case):
    """(sums float64 [B] including sums0, bound [B], grad fp32 = ((gscale * 2) * d) * m as the kernel orders it)."""
    B, P = case["B"], case["P"]
    d64 = case["eps_hat"].double() - case["noise"].double()
    m64 = case["mask"].double().reshape(1, 1, *case["grid"]) if case["mask"] is not None else 1.0
    terms = (d64 * d64 * m64).reshape(B, -1).sum(1)
    d32 = case["eps_hat"] - case["noise"]
    gs = torch.tensor(case["gscale"], dtype=F32) * 2.0
    grad = gs * d32
    if case["mask"] is not None:
        grad = grad * case["mask"].reshape(1, 1, *case["grid"])
    return terms + case["sums0"], sq_err_bound(terms, case["sums0"], case["C"] * P), grad


def sq_err_bound(terms, sums0, count):
    """md_masked_sq_err_kernel, per group of 4 elements in fp32: d = e - n (1 rounding, felt twice by d^2), d * d (1), * mask (1;
    exact for a 0/1 mask), and up to 3 adds into `part`: 7 u on a term at most.  Then double: one add per group per thread, 6
    shuffle levels, 4 waves, one atomicAdd per block onto sums[b]."""
    return (7 * U * terms + (count / 4 + 16) * D53 * (terms + sums0.abs())) * SECOND_ORDER


def emulate_sq_err(case, mut=None):
    """fp32 per group of four, double after.  mut = 'skip_second_trip': elements past 256 blocks x 256 threads x 4 are not read."""
    B, P = case["B"], case["P"]
    d = case["eps_hat"] - case["noise"]
    t = d * d
    if case["mask"] is not None:
        t = t * case["mask"].reshape(1, 1, *case["grid"])
    t = t.reshape(B, -1, 4)
    part = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]
    if mut == "skip_second_trip":
        part = part[:, :256 * 256]
    return part.double().sum(1) + case["sums0"]


SQNORM_N = (1, 2, 3, 4, 5, 7, 1023, 1048576 + 3, 1048576 + 1201)     # the last one takes a second trip (n/4 > 1024 * 256)
SQNORM_SCALES = (1e-12, 1.0, 1e12)


def sqnorm_params():
    """(n, scale, mixed) of every case: the small sizes at three magnitudes, the large ones once, two with mixed magnitudes."""
    cs = [(n, s, False) for n in SQNORM_N[:7] for s in SQNORM_SCALES] + [(n, 1.0, False) for n in SQNORM_N[7:]]
    return cs + [(1023, 1.0, True), (SQNORM_N[7], 1.0, True)]


def sqnorm_case(n, scale, seed=40, mixed=False):
    g = _gen(seed + n % 1000)
    x = torch.randn(n, generator=g)
    if mixed:
        x = x * 10.0 ** (24 * torch.rand(n, generator=g) - 12)       # magnitudes 1e-12 .. 1e12 in one vector
    else:
        x = x * scale
    out0 = float((x.double() ** 2).sum()) * 0.75                     # accumulation onto a non-zero *out
    return dict(n=n, g=x, out0=out0)


def sqnorm_reference(case):
    ref = (case["g"].double() ** 2).sum()
    return float(ref + case["out0"]), sqnorm_bound(float(ref), case["out0"], case["n"])


def sqnorm_bound(ref, out0, n):
    """md_grad_sqnorm_kernel: v0 v0 + v1 v1 in fp32 (1 rounding per square, 1 for the add: 2 u on a term), pairs and everything
    after them in double; the n % 4 tail is squared in double."""
    return (2 * U * ref + (n / 4 + 16) * D53 * (ref + abs(out0))) * SECOND_ORDER


def emulate_sqnorm(case, mut=None):
    """mut = 'skip_tail': the n % 4 tail is not added; 'skip_second_trip': float4 items past 1024 x 256 are not read."""
    x, n = case["g"], case["n"]
    n4 = n // 4
    v = x[:n4 * 4].reshape(n4, 4)
    if mut == "skip_second_trip":
        v = v[:1024 * 256]
    sq = v * v
    acc = ((sq[:, 0] + sq[:, 1]).double() + (sq[:, 2] + sq[:, 3]).double()).sum()
    if mut != "skip_tail":
        acc = acc + (x[n4 * 4:].double() ** 2).sum()
    return float(acc + case["out0"])


# ---------------------------------------------------------------------------------------------------------------
# md_adam_ema_step
# ---------------------------------------------------------------------------------------------------------------
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
ADAM_MAX_NORM = 1.0


def ema_decay(decay, num_updates):
    """models/ema.py: d = min(decay, (1 + n) / (10 + n)) after n updates (n counts this one)."""
    return min(decay, (1 + num_updates) / (10 + num_updates))


def adam_case(name, n, step, wd=0.0, clip="off", d=0.9999, ema=True, seed=70):
    """Parameters 1e-3 randn with lr = 1e-3 and a shadow 1e-5 randn drawn on its own: one step moves a parameter by about its own
    size, the shadow by (1 - d) |p|, so the roundings of p and ema themselves (u |p|, u |ema|) stay under the error a wrong update
    or a wrong rate makes.  clip: 'off' (max_norm < 0), 'nosq' (max_norm set, no norm given: no clip), 'under' / 'over' (the
    gradient norm 1 % under / over max_norm)."""
    g = _gen(seed + n % 997 + step % 13)
    p = 1e-3 * torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g)
    if clip in ("under", "over"):
        target = ADAM_MAX_NORM * (0.99 if clip == "under" else 1.01)
        grad = grad * (target / float(grad.double().norm()))
    m = 0.1 * torch.randn(n, generator=g) * (0.0 if step == 1 else 1.0) * float(grad.double().abs().mean())
    v = (0.5 + torch.rand(n, generator=g)) * (0.0 if step == 1 else 1.0) * float((grad.double() ** 2).mean())
    s = 1e-5 * torch.randn(n, generator=g) if ema else None
    return dict(name=name, n=n, step=step, wd=wd, clip=clip, d=d, p=p, g=grad, m=m, v=v, ema=s, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2,
                eps=ADAM_EPS, max_norm=-1.0 if clip == "off" else ADAM_MAX_NORM,
                sq=None if clip in ("off", "nosq") else float((grad.double() ** 2).sum()))


def adam_cases():
    cs = []
    for i, n in enumerate((1, 3, 255, 257, 524288 + 5)):
        cs.append(adam_case(f"n{n}", n, (1, 2, 1000, 10 ** 6, 2)[i], d=(2 / 11, 0.999, 0.9999, 0.9999, 0.9999)[i],
                            clip=("off", "over", "under", "nosq", "over")[i], wd=(0.0, 0.01, 0.0, 0.01, 0.01)[i]))
    for step in (1, 2, 1000, 10 ** 6):
        cs.append(adam_case(f"step{step}", 257, step, clip="over", d=0.9999))
    for clip in ("off", "nosq", "under", "over"):
        for wd in (0.0, 0.01):
            cs.append(adam_case(f"clip-{clip}-wd{wd}", 255, 1000, wd=wd, clip=clip, d=0.9999))
    for d in (2 / 11, 0.999, 0.9999):
        cs.append(adam_case(f"d{d:.4f}", 257, 2, d=d))
    cs.append(adam_case("no-ema", 257, 2, ema=False, clip="over"))
    return cs


def adam_scalars(case):
    """The fp32 scalars of one step as the reference program forms them, as Python floats: torch.optim.Adam casts 1 - beta1
    (lerp weight), beta2, 1 - beta2, eps, weight_decay, lr / bc1 and sqrt(bc2) from doubles; models/ema.py casts 1.0 - d."""
    b1, b2, step = case["b1"], case["b2"], case["step"]
    return dict(w1=f32(1.0 - b1), b2=f32(b2), w2=f32(1.0 - b2), eps=f32(case["eps"]), wd=f32(case["wd"]),
                step_size=f32(case["lr"] / (1.0 - b1 ** step)), bc2s=f32(math.sqrt(1.0 - b2 ** step)),
                rate=f32(1.0 - case["d"]), max_norm=f32(case["max_norm"]))


def adam_clip(case, sc):
    if case["sq"] is None or sc["max_norm"] < 0:
        return 1.0
    return min(1.0, sc["max_norm"] / (math.sqrt(case["sq"]) + 1e-6))


def adam_reference(case, sq_rel_err=0.0):
    """float64 step and its running error bound.  Returns dict(m, v, dp, p, dema, ema: float64; e_m, e_v, e_dp, e_dema: bounds).

    Every line of the kernel is one fp32 operation, off by u times its result, plus what its inputs carry (SECOND_ORDER at the end):
      clip = min(1, max_norm / ((float)sqrt(sq) + 1e-6f))   cast, add, divide: 3 u (+ sq_rel_err / 2 where md_grad_sqnorm made sq)
      g' = g clip                                           1      (clip = 1.f: exact)
      g' = g' + wd p                                        2      (only where wd != 0)
      m  = m + (g' - m) w1                                  3
      v  = v b2 + (w2 g') g'                                4      and twice the error of g'
      den = sqrtf(v) / bc2s + eps                           3      sqrt halves the relative error of v
      dp = step_size (m / den)                              2
      p  = p - dp                                           1      the only one relative to p itself: u |p|
    18 operations in all between g and p: with nothing cancelling |p_gpu - p64| <= u |p64| + 18 u |dp64| (less: the sqrt halves
    its 11).  Where m + (g' - m) w1 cancels the bound is larger than that form in |dp64| and still right, because each rounding is
    charged on the result it rounds.  ema = ema - rate (ema - p): 3 operations; dema carries 2 u |dema| + rate |dp - dp64| and
    ema itself u |ema|.  m and v come out bounded in their own ulps: e_m ~ (3 + 7 w1) u, e_v ~ 16 u |v| at most."""
    sc = adam_scalars(case)
    p, g, m, v = (case[k].double() for k in ("p", "g", "m", "v"))
    clip = adam_clip(case, sc)
    gc = g * clip
    clipped = case["sq"] is not None and sc["max_norm"] >= 0
    e_g = (((3 * U + sq_rel_err / 2) if clipped else 0.0) + (U if clip != 1.0 else 0.0)) * gc.abs()
    if sc["wd"] != 0.0:
        t = sc["wd"] * p
        gc, e_g = gc + t, e_g + U * t.abs() + U * (gc + t).abs()
    d = gc - m
    e_d = e_g + U * d.abs()
    t2 = d * sc["w1"]
    e_t2 = sc["w1"] * e_d + U * t2.abs()
    m1 = m + t2
    e_m = e_t2 + U * m1.abs()
    v1 = v * sc["b2"]
    q = (sc["w2"] * gc) * gc
    e_q = 2 * (sc["w2"] * gc).abs() * e_g + 2 * U * q
    v2 = v1 + q
    e_v = U * v1 + e_q + U * v2
    r = torch.sqrt(v2)
    e_r = e_v / (2 * r.clamp_min(1e-300)) + U * r
    h = r / sc["bc2s"]
    e_h = e_r / sc["bc2s"] + U * h
    den = h + sc["eps"]
    e_den = e_h + U * den
    z = m1 / den
    e_z = e_m / den + z.abs() * e_den / den + U * z.abs()
    dp = -sc["step_size"] * z
    e_dp = sc["step_size"] * e_z + U * dp.abs()
    p1 = p + dp
    e_p = e_dp + U * p1.abs()
    out = dict(m=m1, v=v2, dp=dp, p=p1, e_m=e_m * SECOND_ORDER, e_v=e_v * SECOND_ORDER, e_dp=e_p * SECOND_ORDER, clip=clip, sc=sc)
    if case["ema"] is not None:
        s = case["ema"].double()
        x = s - p1
        e_x = e_p + U * x.abs()
        y = sc["rate"] * x
        e_y = sc["rate"] * e_x + U * y.abs()
        s1 = s - y
        out.update(dema=-y, ema=s1, e_dema=(e_y + U * s1.abs()) * SECOND_ORDER)
    return out


def emulate_adam(case, mut=None):
    """md_adam_ema_kernel in fp32 torch, line for line.  Returns (p, m, v, ema) fp32.  Mutations: 'no_clip', 'bc_step_minus_1',
    'mul_bc2', 'ema_rate_f32' (rate = 1.f - (float)d: the kernel before this suite), 'no_wd', 'betas_f32' (1.f - (float)beta and
    the bias corrections formed from betas that went through a float: the kernel before this suite as well), 'skip_second_trip'
    (elements past 2048 blocks x 256 threads keep their old state)."""
    sc = adam_scalars(case)
    T = lambda x: torch.tensor(x, dtype=F32)
    step = case["step"] - (1 if mut == "bc_step_minus_1" else 0)
    b1, b2, w1, w2 = case["b1"], case["b2"], T(sc["w1"]), T(sc["w2"])
    if mut == "betas_f32":
        b1, b2 = f32(b1), f32(b2)
        w1, w2 = T(1.0) - T(b1), T(1.0) - T(b2)
    step_size = T(case["lr"] / (1.0 - b1 ** step)) if step > 0 else T(float("inf"))
    bc2s = T(math.sqrt(1.0 - b2 ** step)) if step > 0 else T(0.0)
    p, g, m, v = case["p"], case["g"], case["m"], case["v"]
    clip = T(1.0)
    if case["sq"] is not None and sc["max_norm"] >= 0 and mut != "no_clip":
        c = T(sc["max_norm"]) / (T(math.sqrt(case["sq"])) + T(1e-6))
        clip = c if c < 1 else T(1.0)
    gi = g * clip
    if sc["wd"] != 0.0 and mut != "no_wd":
        gi = gi + T(sc["wd"]) * p
    mi = m + (gi - m) * w1
    vi = v * T(sc["b2"]) + w2 * gi * gi
    denom = (torch.sqrt(vi) * bc2s if mut == "mul_bc2" else torch.sqrt(vi) / bc2s) + T(sc["eps"])
    pi = p - step_size * (mi / denom)
    s = case["ema"]
    if s is not None:
        rate = T(1.0) - T(case["d"]) if mut == "ema_rate_f32" else T(sc["rate"])
        s = s - rate * (s - pi)
    if mut == "skip_second_trip":
        k = 2048 * 256
        keep = lambda new, old: torch.cat([new[:k], old[k:]]) if old is not None else None
        pi, mi, vi, s = keep(pi, p), keep(mi, m), keep(vi, v), keep(s, case["ema"])
    return pi, mi, vi, s


def adam_worst(got, case, ref):
    """max over the elements of |got - ref| / bound for (m, v, dp, dema); got = (p, m, v, ema) fp32 after the step."""
    p1, m1, v1, s1 = got
    tiny = 1e-300
    out = dict(m=float(((m1.double() - ref["m"]).abs() / ref["e_m"].clamp_min(tiny)).max()),
               v=float(((v1.double() - ref["v"]).abs() / ref["e_v"].clamp_min(tiny)).max()),
               dp=float((((p1.double() - case["p"].double()) - ref["dp"]).abs() / ref["e_dp"].clamp_min(tiny)).max()))
    if case["ema"] is not None:
        out["dema"] = float((((s1.double() - case["ema"].double()) - ref["dema"]).abs() / ref["e_dema"].clamp_min(tiny)).max())
    return out
