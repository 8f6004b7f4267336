"""Inputs, float64 references and the schedule replay for the direct tests of the attention kernels
(tests/test_gpu_attention.py runs them on the GPU, tests/test_cpu_attention_cases.py proves on the CPU that every
case is in the regime it claims).  Plain helper module: no fixtures, no GPU, only torch.

The fused kernel (csrc/attention.hip) keeps a running maximum `m_run` per query in the log2 domain and multiplies
its output accumulators and denominator by corr = 2^(m_run - m_new) only when some query of the WAVE sees a
32-key tile whose maximum exceeds `m_run` by more than 8.  `replay` restates that schedule; its three constants
mirror AT_QW, AT_TK and the literal in the kernel's ballot -- if the kernel changes them, change them here.

Exact cases.  Query i of sample b has type (i + b) % T; type t owns channels 16t .. 16t + 15:
    k[16t + j][key] = level_t[key],   q[16t + j][i] = gain_t (type of i is t) or 0,   scale = 1/16
so the logit of (key, query i) is exactly gain_t * level_t[key] (natural-log units; x 1.4427 for the kernel's
log2 domain).  Levels and gains carry at most 8 significant bits, so the bf16 hi plane holds them, lo = 0, and every
product and sum is exact in fp32: the kernel sees the reference's logits.  Levels END at 0 (lower levels negative), so
the one fp32 rounding of tv = s * scale * log2(e) (6e-8 relative to |tv|) vanishes for the keys that carry mass.
v[c][key] = small integers that depend on the tile index, the key and the channel; bias_v is non-zero.
"""
import math

import torch

AT_C = 256          # head dim of md_attn_fwd
AT_QW = 32          # queries per wave            (attention.hip AT_QW)
AT_TK = 32          # keys per tile               (attention.hip AT_TK)
AT_THRESHOLD = 8.0  # lazy-rescale threshold, log2 (attention.hip: `mloc > m_run + 8.0f`)
AT_M0 = -1e30       # initial running maximum     (attention.hip: `m_run = -1e30f`)
LOG2E = 1.4426950408889634
SCALE = AT_C ** -0.5

# Two spike heights in natural-log units with 7 significant bits: 8.025 and 16.05 in the log2 domain, so the second
# step clears m_run + 8 by 0.025 (fp32 resolves 1e-6 there) while e^-L1 = 1/260 keeps old keys visible.
L1 = 5.5625
L2 = 11.125


def bf16_exact(x):
    return bool(torch.equal(x.to(torch.bfloat16).to(x.dtype), x))


def split_bf16(x):
    """md_split on the host: hi = bf16(x) (RNE), lo = bf16(x - hi); fp32 in, two fp32 tensors out."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


# ---------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------
def _values(N, seed=0):
    t = torch.arange(N)
    c = torch.arange(AT_C)[:, None]
    v = ((t // AT_TK)[None] * 37 + c * 11 + (t % AT_TK)[None] * 5 + seed * 3) % 129 - 64
    return v.float()                                                   # [C][N], integers in [-64, 64]


def _bias(seed):
    return 0.5 * torch.randn(AT_C, generator=torch.Generator().manual_seed(1000 + seed)) + 0.25


def _exact_case(name, N, B, types, **meta):
    """types: list of (level[N] tensor, gain); T = len(types) must divide 32 and be <= 16."""
    T = len(types)
    assert 32 % T == 0 and T <= AT_C // 16 and N % 128 == 0
    q = torch.zeros(B, AT_C, N)
    k = torch.zeros(B, AT_C, N)
    qtype = torch.empty(B, N, dtype=torch.long)
    for b in range(B):
        qtype[b] = (torch.arange(N) + b) % T
        for t, (level, gain) in enumerate(types):
            k[b, 16 * t:16 * t + 16] = level.float()[None]
            q[b, 16 * t:16 * t + 16, qtype[b] == t] = float(gain)
    v = torch.stack([_values(N, b) for b in range(B)])
    return dict(name=name, N=N, B=B, q=q, k=k, v=v, bias=_bias(N + B), exact=True, qtype=qtype, T=T, **meta)


def _flat(N, value=0.0):
    return torch.full((N,), float(value))


def plateau_spike(N, B, double=True):
    """Types 0/1/2: one key L1 above a plateau, in the first / middle / last third (the last one in the LAST tile);
    type 3 (double): plateau, then 1 key at +L1 two thirds in, then 1 key at +L2 in the last tile -- two rescales with
    >= 1 % of the final mass in front of each (needs N >= ~700: n0 >= 0.01 * e^L2 keys; so double = False at small N)."""
    nt = N // AT_TK
    tiles = [max(1, nt // 6), nt // 2, nt - 1]
    types = []
    for i, t in enumerate(tiles):
        lv = _flat(N, -L1)
        lv[t * AT_TK + (3, 5, 30)[i]] = 0.0          # in-tile offsets 3 / 5 / 30: lane half h = 0 / 1 / 1 holds the spike
        types.append((lv, 1.0))
    if double:
        lv = _flat(N, -L2)
        lv[(nt - 2) * AT_TK + 9] = L1 - L2
        lv[(nt - 1) * AT_TK + 20] = 0.0
    else:
        lv = _flat(N, -L1)
        lv[1 * AT_TK + 12] = 0.0
    types.append((lv, 1.0))
    return _exact_case(f"plateau_spike-N{N}-B{B}", N, B, types, kind="plateau_spike", double=double)


def rising_staircase(N, B):
    """Every tile is 6 (8.66 log2) above the previous one: every tile after the first rescales live accumulators."""
    assert N <= 1024
    nt = N // AT_TK
    lv = -6.0 * (nt - 1 - torch.arange(N) // AT_TK).float()
    return _exact_case(f"rising-N{N}-B{B}", N, B, [(lv, 1.0)], kind="rising")


def lazy_staircase(N, B):
    """Steps of 1 (1.44 log2) per tile: m_run stays for 5 tiles while p grows to 2^7.2, then one rescale."""
    nt = N // AT_TK
    lv = -1.0 * (nt - 1 - torch.arange(N) // AT_TK).float()
    lv2 = -0.5 * (nt - 1 - torch.arange(N) // AT_TK).float()          # steps of 0.72: 11 tiles per rescale
    return _exact_case(f"lazy-N{N}-B{B}", N, B, [(lv, 1.0), (lv2, 1.0)], kind="lazy")


def falling_staircase(N, B):
    """Maximum in the first tile, 6 less per tile: no rescale after tile 0, later tiles underflow to p = 0."""
    lv = -6.0 * (torch.arange(N) // AT_TK).float()
    lv2 = -0.25 * (torch.arange(N) // AT_TK).float()
    return _exact_case(f"falling-N{N}-B{B}", N, B, [(lv, 1.0), (lv2, 1.0)], kind="falling")


def dominant_key(N, B):
    """One key 16 above all others (softmax weight > 0.99) at position 0, 31, 32 or N - 1."""
    types = []
    for pos in (0, 31, 32, N - 1):
        lv = _flat(N, -16.0)
        lv[pos] = 0.0
        types.append((lv, 1.0))
    return _exact_case(f"dominant-N{N}-B{B}", N, B, types, kind="dominant", positions=(0, 31, 32, N - 1))


def mixed_gains(N, B):
    """One level structure (plateau, one key L1 higher in the middle, one more in the last tile at the same height)
    read with gains 1, 2, 0.5, -1, and a second structure with the spike in the other lane half: on one firing the
    lanes of a wave get corr = 2^-8.03 (gain 1), 2^-16.05 (gain 2), 2^-4.01 (gain 0.5: no rescale of its own, it follows the
    wave's) and exactly 1 (gain -1: the plateau IS the maximum)."""
    nt = N // AT_TK
    lv = _flat(N, -L1)
    lv[(nt // 2) * AT_TK + 2] = 0.0           # lane half h = 0
    lv[(nt - 1) * AT_TK + 17] = 0.0
    lw = _flat(N, -L1)
    lw[(nt // 2) * AT_TK + 6] = 0.0           # lane half h = 1
    types = [(lv, 1.0), (lv, 2.0), (lv, 0.5), (lv, -1.0), (lw, 1.0), (lw, 2.0), (lw, 0.5), (lw, -1.0)]
    return _exact_case(f"mixed-N{N}-B{B}", N, B, types, kind="mixed")


def uniform(N, B):
    """All logits of a query equal (3 * gain): the control."""
    return _exact_case(f"uniform-N{N}-B{B}", N, B, [(_flat(N, 3.0), 1.0), (_flat(N, 3.0), -2.0)], kind="uniform")


def randn_case(N=4096, B=2, sigma2=3.5, seed=7):
    """Ordinary operands: q, k ~ N(0, sigma2) per entry, so logits ~ N(0, sigma2^2) and a query's spread over 4096 keys is
    about 2 * 3.7 * sigma2 * log2(e) = 37 log2 units (the block tests: 13 .. 16)."""
    g = torch.Generator().manual_seed(seed)
    s = math.sqrt(sigma2)
    q = torch.randn(B, AT_C, N, generator=g) * s
    k = torch.randn(B, AT_C, N, generator=g) * s
    v = torch.randn(B, AT_C, N, generator=g)
    return dict(name=f"randn-N{N}-B{B}", N=N, B=B, q=q, k=k, v=v, bias=_bias(seed), exact=False, kind="randn")


EXACT_CASES = [
    lambda: plateau_spike(128, 1, double=False),
    lambda: plateau_spike(1024, 3),
    lambda: plateau_spike(4096, 3),
    lambda: rising_staircase(128, 1),
    lambda: rising_staircase(1024, 3),
    lambda: lazy_staircase(512, 1),
    lambda: lazy_staircase(4096, 1),
    lambda: falling_staircase(512, 1),
    lambda: dominant_key(128, 3),
    lambda: dominant_key(1024, 1),
    lambda: mixed_gains(512, 1),
    lambda: mixed_gains(1024, 3),
    lambda: uniform(128, 1),
    lambda: uniform(1024, 1),
]
EXACT_IDS = ["plateau_spike-N128-B1", "plateau_spike-N1024-B3", "plateau_spike-N4096-B3", "rising-N128-B1", "rising-N1024-B3",
             "lazy-N512-B1", "lazy-N4096-B1", "falling-N512-B1", "dominant-N128-B3", "dominant-N1024-B1", "mixed-N512-B1",
             "mixed-N1024-B3", "uniform-N128-B1", "uniform-N1024-B1"]
# the unfused path runs every case with N <= 1024 and this one N = 4096 case
UNFUSED_IDS = [i for i in EXACT_IDS if "N4096" not in i] + ["lazy-N4096-B1"]


def exact_case(case_id):
    return EXACT_CASES[EXACT_IDS.index(case_id)]()


# ---------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------
def logits64(q, k, scale=SCALE):
    """[key][query] natural-log logits of one sample from (de-quantised) q, k [C][N], exact float64."""
    return (k.double().t() @ q.double()) * scale


def logits64_bf16x3(qhi, qlo, khi, klo, scale=SCALE):
    """The kernel's declared arithmetic: hi*hi + hi*lo + lo*hi, the lo*lo term dropped; float64 otherwise."""
    qh, ql, kh, kl = (t.double() for t in (qhi, qlo, khi, klo))
    return (kh.t() @ qh + kh.t() @ ql + kl.t() @ qh) * scale


def attention64(logits, v, bias):
    """o[c][query] = sum_key v[c][key] softmax_key(logits)[key][query] + bias[c]; returns (o, P)."""
    p = torch.softmax(logits.double(), dim=0)
    return v.double() @ p + bias.double()[:, None], p


def elementwise_err(got, ref):
    """per sample max |got - ref| / max |ref| (first dimension = samples); returns the largest."""
    got, ref = got.double(), ref.double()
    B = ref.shape[0]
    d = (got - ref).reshape(B, -1).abs().amax(1)
    return float((d / ref.reshape(B, -1).abs().amax(1).clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------
# the kernel's rescale schedule, replayed from the reference's logits
# ---------------------------------------------------------------------------------------------------------------
def replay(logits, p=None):
    """logits: [key][query] float64, natural-log units (one sample); p: its softmax (computed when None).
    Returns a dict of [ntiles][N] tensors:
      fired   bool    the query's wave rescales at this tile (wave-uniform)
      corr    float64 the factor this query's lanes apply (1 where not fired or unmoved)
      before  float64 share of the query's final softmax mass held by the keys of earlier tiles
      pmax    float64 log2 of the largest p = 2^(tv - m_run) the query forms at this tile (after a possible rescale)
    and `visible` = fired & (0 < corr < 1) & (before >= 0.01) & (tile > 0)."""
    tv = logits.double() * LOG2E
    N = tv.shape[1]
    nt = tv.shape[0] // AT_TK
    tmax = tv.view(nt, AT_TK, N).amax(1)                                # [tile][query]
    if p is None:
        p = torch.softmax(logits.double(), dim=0)
    tmass = p.view(nt, AT_TK, N).sum(1)
    before = torch.cumsum(tmass, 0) - tmass
    m_run = torch.full((N,), AT_M0, dtype=torch.float64)
    fired = torch.zeros(nt, N, dtype=torch.bool)
    corr = torch.ones(nt, N, dtype=torch.float64)
    pmax = torch.empty(nt, N, dtype=torch.float64)
    for t in range(nt):
        want = tmax[t] > m_run + AT_THRESHOLD
        wave = want.view(-1, AT_QW).any(1).repeat_interleave(AT_QW)    # the ballot
        m_new = torch.where(wave, torch.maximum(m_run, tmax[t]), m_run)
        fired[t] = wave
        corr[t] = torch.exp2(m_run - m_new)
        m_run = m_new
        pmax[t] = tmax[t] - m_run
    live = fired & (corr > 0) & (corr < 1)
    live[0] = False
    return dict(fired=fired, corr=corr, before=before, pmax=pmax, live=live, visible=live & (before >= 0.01))


def check_precondition(case, b, rep):
    """Asserts that sample b of `case` is in the regime its kind claims (conditions on the inputs only)."""
    kind, N = case["kind"], case["N"]
    nt = N // AT_TK
    vis, live, fired = rep["visible"], rep["live"], rep["fired"]
    per_wave = lambda m: m.view(-1, N // AT_QW, AT_QW).any(2)          # [..][wave]
    if kind == "plateau_spike":
        third = torch.arange(nt) * 3 // nt                             # 0 / 1 / 2 by key range
        for s in range(3):
            assert bool(per_wave(vis[third == s].any(0)).all()), f"{case['name']}: a wave has no visible firing in third {s}"
        if case["double"]:
            assert int((vis.sum(0) >= 2).sum()) >= N // 4, f"{case['name']}: no query with two visible firings"
    elif kind == "rising":
        assert bool(live[1:].all()), f"{case['name']}: a tile after the first does not rescale"
    elif kind == "lazy":
        quiet = ~fired & (rep["pmax"] > 7.0)
        assert bool(per_wave(quiet.any(0)).all()), f"{case['name']}: p never exceeds 2^7 without a rescale"
        assert bool(per_wave(vis.any(0)).all())
    elif kind == "falling":
        assert not bool(fired[1:].any()), f"{case['name']}: a rescale after tile 0"
    elif kind == "dominant":
        pm = torch.softmax(rep["logits"], 0).amax(0) if "logits" in rep else None
        assert pm is None or bool((pm > 0.99).all())
    elif kind == "mixed":
        c = rep["corr"].view(nt, N // AT_QW, AT_QW)
        f = fired.view(nt, N // AT_QW, AT_QW)[:, :, 0]
        both = f & ((c > 0) & (c < 1)).any(2) & (c == 1).any(2)
        both[0] = False
        assert bool(both.any(0).all()), f"{case['name']}: no firing with corr < 1 and corr == 1 in one wave"
        assert bool(per_wave(vis.any(0)).all())
    elif kind == "uniform":
        assert not bool(fired[1:].any())
    elif kind == "randn":
        assert int(live.any(1).sum()) >= 1 and int(per_wave(live.any(0)).sum()) >= (N // AT_QW) // 2, \
            f"{case['name']}: fewer than half of the waves rescale after tile 0"
    else:
        raise AssertionError(kind)


def analyse(case, b, logits=None):
    """float64 logits, softmax, output and replay of sample b from the operands as given (exact cases: these ARE the
    kernel's operands; inexact ones: pass the logits of the de-quantised operands)."""
    if logits is None:
        logits = logits64(case["q"][b], case["k"][b])
    out, p = attention64(logits, case["v"][b], case["bias"])
    rep = replay(logits, p)
    rep["logits"] = logits
    return out, p, rep


# ---------------------------------------------------------------------------------------------------------------
# float64 emulation of the kernel's loop (used by the CPU tests to show that the cases bite)
# ---------------------------------------------------------------------------------------------------------------
def emulate_kernel(logits, v, bias, skip_oacc=False, skip_l=False, never_after0=False, dtype=torch.float64):
    """The online-softmax loop of md_attn_fwd with its schedule, in float64 (or fp32: `dtype`); the three flags are the
    mutations the GPU tests are meant to catch (oacc *= corr removed, l_run *= corr removed, no rescale after tile 0).
    The third one is exact in real arithmetic: it shows only where p = 2^(tv - m_run) leaves the fp32 range (> 2^128)."""
    tv = (logits.double() * LOG2E).to(dtype)
    N = tv.shape[1]
    nt = tv.shape[0] // AT_TK
    v = v.to(dtype)
    m_run = torch.full((N,), AT_M0, dtype=dtype)
    l_run = torch.zeros(N, dtype=dtype)
    oacc = torch.zeros(v.shape[0], N, dtype=dtype)
    for t in range(nt):
        tile = tv[t * AT_TK:(t + 1) * AT_TK]
        mloc = tile.amax(0)
        thr = 1e30 if (never_after0 and t > 0) else AT_THRESHOLD
        wave = (mloc > m_run + thr).view(-1, AT_QW).any(1).repeat_interleave(AT_QW)
        m_new = torch.where(wave, torch.maximum(m_run, mloc), m_run)
        corr = torch.exp2(m_run - m_new)
        m_run = m_new
        if not skip_l:
            l_run = l_run * corr
        if not skip_oacc:
            oacc = oacc * corr
        pt = torch.exp2(tile - m_run)
        l_run = l_run + pt.sum(0)
        oacc = oacc + v[:, t * AT_TK:(t + 1) * AT_TK] @ pt
    return (oacc / l_run).double() + bias.double()[:, None]


# ---------------------------------------------------------------------------------------------------------------
# layouts (host side)
# ---------------------------------------------------------------------------------------------------------------
def block_keys(s):
    """[B][keys][queries] -> [B][keys/8][queries][8] (the layout md_softmax_keys reads and md_softmax_keys_bwd's dP)."""
    B, nk, nq = s.shape
    return s.reshape(B, nk // 8, 8, nq).permute(0, 1, 3, 2).contiguous()


def unblock_keys(sb):
    B, nkb, nq, _ = sb.shape
    return sb.permute(0, 1, 3, 2).reshape(B, nkb * 8, nq)


def s16b_planes(t):
    """S16B bf16 tensor [B][R/8][2][Cn][8] -> (hi, lo) as fp32 [B][R][Cn]."""
    t = t.float().cpu()
    B, rb, _, cn, _ = t.shape
    hi = t[:, :, 0].permute(0, 1, 3, 2).reshape(B, rb * 8, cn)
    lo = t[:, :, 1].permute(0, 1, 3, 2).reshape(B, rb * 8, cn)
    return hi, lo


# ---------------------------------------------------------------------------------------------------------------
# the sharp AttnBlock
# ---------------------------------------------------------------------------------------------------------------
SHARP_GAIN = 3.0      # NIN_0.W and NIN_1.W of the sensitised state are multiplied by this (logits by its square)


def sharpen(sd, gain=SHARP_GAIN):
    sd = {k: v.clone() for k, v in sd.items()}
    sd["NIN_0.W"] = sd["NIN_0.W"] * gain
    sd["NIN_1.W"] = sd["NIN_1.W"] * gain
    return sd


def oracle_max_weight(sd, x):
    """Largest softmax weight of every query, from the oracle's own formulation in float64: [B][N]."""
    from oracle import unet_oracle as uo
    sd = {k: v.double() for k, v in sd.items()}
    x = x.double()
    B, C = x.shape[:2]
    h = uo.group_norm(x, sd["GroupNorm_0.weight"], sd["GroupNorm_0.bias"])
    q = uo.nin(h, sd["NIN_0.W"], sd["NIN_0.b"]).reshape(B, C, -1)
    k = uo.nin(h, sd["NIN_1.W"], sd["NIN_1.b"]).reshape(B, C, -1)
    w = torch.einsum("bcq,bck->bqk", q, k) * (int(C) ** (-0.5))
    return torch.softmax(w, dim=-1).amax(-1)
