"""Inputs and launchers of the small-level bit tests (tests/test_gpu_small_level_bits.py, tools/gen_small_level_golden.py):
the 4^3-level 3x3x3 convolution (MD_CFG_C3_LOW, fp32 parts with the GroupNorm loader, split-K) and the 1x1x1 GEMM (MD_CFG_G1_128,
F32B output) through hip_ops.gemm_conv.  Plain helper module: no fixtures; numpy + torch, the GPU only inside `run`.

Every tensor is made from numpy's MT19937 integers (the same on every machine and library version) scaled by powers of two or one
fp32 multiplication, so the words a build writes for a case depend on the kernels alone.  The golden file holds one CRC-32 per
(sample, 8-channel group) slab of the F32B output, and the whole output of the cases below WHOLE_BYTES."""
import zlib

import numpy as np
import torch

WHOLE_BYTES = 40 * 1024


def _ints(seed, shape, lo, hi):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float32)


# ---- the cases ---------------------------------------------------------------------------------------------------
# conv: B samples, `parts` input channels (their concatenation), cout rows (rows_alloc = cout rounded up to 8), ksplit
CONV = [
    dict(id="c64-128-ks2-B1", B=1, parts=[64], cout=128, ksplit=2, bias="shared", res=True),
    dict(id="c64-128-ks2-B3", B=3, parts=[64], cout=128, ksplit=2, bias="sample", res=False),
    dict(id="c64-128-ks2-B8", B=8, parts=[64], cout=128, ksplit=2, bias="shared", res=True),
    dict(id="c512-512-ks8-B1", B=1, parts=[512], cout=512, ksplit=8, bias="sample", res=True),
    dict(id="c512-512-ks8-B3", B=3, parts=[256, 256], cout=512, ksplit=8, bias="shared", res=True),
    dict(id="c512-512-ks8-B8", B=8, parts=[512], cout=512, ksplit=8, bias="sample", res=False),
    dict(id="c72+184-128-ks8-B5", B=5, parts=[72, 184], cout=128, ksplit=8, bias="shared", res=True),      # part boundary inside a chunk
    dict(id="c64-100of104-ks2-B2", B=2, parts=[64], cout=100, ksplit=2, bias="sample", res=False),        # rows_alloc > rows
    dict(id="c1024-512-ks8-B8", B=8, parts=[512, 512], cout=512, ksplit=8, bias="shared", res=False),
]
# gemm: P positions per sample, K input channels, cout rows; f32 = None (S16B operand) or the fp32 parts (split-only loader)
GEMM = [
    dict(id="g-P256-K32-128-B1-s16", B=1, P=256, K=32, cout=128, f32=None, bias="shared", res=True),
    dict(id="g-P256-K256-512-B8-s16", B=8, P=256, K=256, cout=512, f32=None, bias=None, res=False),
    dict(id="g-P256-K768-128-B8-f32", B=8, P=256, K=768, cout=128, f32=[384, 384], bias="sample", res=True),
    dict(id="g-P256-K768-512-B1-f32", B=1, P=256, K=768, cout=512, f32=[512, 256], bias=None, res=False),
    dict(id="g-P4096-K32-512-B1-f32", B=1, P=4096, K=32, cout=512, f32=[32], bias="shared", res=False),
    dict(id="g-P4096-K256-128-B8-s16", B=8, P=4096, K=256, cout=128, f32=None, bias="shared", res=True),
    dict(id="g-P4096-K768-512-B1-s16", B=1, P=4096, K=768, cout=512, f32=None, bias="sample", res=False),
    dict(id="g-P4096-K256-512-B8-f32", B=8, P=4096, K=256, cout=512, f32=[128, 128], bias="shared", res=True),
    dict(id="g-P512-K1024-512-B8-s16", B=8, P=512, K=1024, cout=512, f32=None, bias="shared", res=True),
]
CASES = {c["id"]: dict(c, kind="conv") for c in CONV}
CASES.update({c["id"]: dict(c, kind="gemm") for c in GEMM})
CONV_IDS, GEMM_IDS = [c["id"] for c in CONV], [c["id"] for c in GEMM]


def _seed(case):
    return zlib.crc32(case["id"].encode()) & 0x7fffffff


def build(case):
    """The host tensors of a case: x [B, K, D, H, W] fp32, ac [B, K, 2] or None, w ([cout, K, 3, 3, 3] or NIN [K, cout]),
    bias [B or 1, cout] or None, res [B, rows_alloc, D, H, W] or None."""
    s = _seed(case)
    B, cout = case["B"], case["cout"]
    rows_alloc = (cout + 7) // 8 * 8
    if case["kind"] == "conv":
        K, dims = sum(case["parts"]), (4, 4, 4)
        x = _ints(s, (B, K, 4, 4, 4), -4096, 4096) * np.float32(2.0 ** -10)
        # +-large values on a hashed eighth of the face voxels (56 of the 64 positions lie on a face): a halo entry read from the
        # wrong side, or padding that is not zero after the transform, moves the sums by far more than a rounding
        big = (_ints(s + 1, x.shape, 0, 7) == 0)
        big[:, :, 1:3, 1:3, 1:3] = False
        x = np.where(big, x * np.float32(64.0), x)
        # GroupNorm constants with a 2^6 spread of the gains, both signs; offsets that never vanish (act(0) != 0 at the rim)
        gain = np.exp2(_ints(s + 2, (B, K), -3, 3)) * (1.0 + _ints(s + 3, (B, K), 0, 255) * np.float32(2.0 ** -8))
        gain = gain * (2.0 * _ints(s + 4, (B, K), 0, 1) - 1.0)
        off = (_ints(s + 5, (B, K), 64, 512) * np.float32(2.0 ** -9)) * (2.0 * _ints(s + 6, (B, K), 0, 1) - 1.0)
        ac = np.stack([gain, off], -1).astype(np.float32)
        w = _ints(s + 7, (cout, K, 3, 3, 3), -1024, 1024) * np.float32(2.0 ** -10 / np.sqrt(27.0 * K))
    else:
        K, dims = case["K"], (1, 1, case["P"])
        x = _ints(s, (B, K, 1, 1, case["P"]), -4096, 4096) * np.float32(2.0 ** -10)
        ac = None
        w = _ints(s + 7, (K, cout), -1024, 1024) * np.float32(2.0 ** -10 / np.sqrt(float(K)))
    bias = res = None
    if case["bias"]:
        bias = _ints(s + 8, (B if case["bias"] == "sample" else 1, cout), -2048, 2048) * np.float32(2.0 ** -10)
    if case["res"]:
        res = _ints(s + 9, (B, rows_alloc) + dims, -4096, 4096) * np.float32(2.0 ** -10)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(case=case, x=t(x), ac=t(ac), w=t(w), bias=t(bias), res=t(res), dims=dims, K=K, rows_alloc=rows_alloc)


def run(ops, case, host=None):
    """The launch of a case on the library `ops` has loaded; returns the F32B output [B, rows_alloc / 8, P, 8] as int32 words (numpy)."""
    h = host or build(case)
    B, cout, rows_alloc, dims, K = case["B"], case["cout"], h["rows_alloc"], h["dims"], h["K"]
    P = dims[0] * dims[1] * dims[2]
    x = h["x"].cuda()
    kw = dict(batch=B, rows=cout, rows_alloc=rows_alloc, dims=dims, out=torch.full((B, rows_alloc // 8, P, 8), float("nan"), device="cuda"))
    if h["bias"] is not None:
        kw.update(bias=h["bias"].cuda(), bias_bstride=cout if h["bias"].shape[0] > 1 else 0)
    if h["res"] is not None:
        kw.update(residual=ops.ncdhw_to_f32b(h["res"].cuda()), res_bstride=rows_alloc * P)
    if case["kind"] == "conv":
        pw = ops.PackedWeight(h["w"].cuda(), "conv", ops.CFG_C3_LOW, "cuda")
        parts = [(ops.ncdhw_to_f32b(t.contiguous()), t.shape[1]) for t in torch.split(x, case["parts"], dim=1)]
        stats = torch.zeros((B, rows_alloc, 2), dtype=torch.float64, device="cuda")
        out = ops.gemm_conv(cfg=ops.CFG_C3_LOW, a=pw.data, b=None, kdim=pw.kdim, ksplit=case["ksplit"], stats=stats,
                            b_f32=ops.F32Operand(parts, h["ac"].cuda(), silu=True), **kw)
    else:
        pw = ops.PackedWeight(h["w"].cuda(), "nin", ops.CFG_G1_128, "cuda")
        if case["f32"]:
            parts = [(ops.ncdhw_to_f32b(t.contiguous()), t.shape[1]) for t in torch.split(x, case["f32"], dim=1)]
            out = ops.gemm_conv(cfg=ops.CFG_G1_128, a=pw.data, b=None, kdim=pw.kdim, b_f32=ops.F32Operand(parts), **kw)
        else:
            out = ops.gemm_conv(cfg=ops.CFG_G1_128, a=pw.data, b=ops.ncdhw_to_s16b(x, pw.kdim), kdim=pw.kdim, **kw)
    torch.cuda.synchronize()
    return out.view(torch.int32).cpu().numpy()


def slab_crcs(words):
    """[B, G, P, 8] int32 -> uint32 [B, G]: CRC-32 of each (sample, 8-channel group) slab."""
    B, G = words.shape[:2]
    return np.array([[zlib.crc32(np.ascontiguousarray(words[b, g]).tobytes()) for g in range(G)] for b in range(B)], dtype=np.uint32)


def describe(got, want):
    """'' when the slab CRCs agree, else which (sample, channel group) slabs differ."""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    if not len(bad):
        return ""
    return f"{len(bad)} of {got.size} (sample, channel group) slabs differ; first: {bad[:8].tolist()}"


# ---- exact cases (tests/conv_cases.py: small integers, the float64 convolution bit for bit) -----------------------------
# 4^3 conv through the fp32-parts loader with a hand-made power-of-two affine, two parts whose boundary falls inside a chunk, a
# partial row tile, B = 5 (one whole sample block of four and a remainder), split-K 4; and the GEMM on split-only fp32 parts and on S16B
EXACT = [
    dict(id="small-conv-exact", entry="gemm", cls="hi_only", dims=(4, 4, 4), parts=[72, 56], cout=136, B=5, cfg="CFG_C3_LOW", b_f32=True,
         ac=True, bias="sample", ksplit=4, seed=901),
    dict(id="small-gemm-exact-f32", entry="gemm", cls="x_lo", dims=(1, 1, 512), parts=[96, 32], cout=256, B=2, cfg="CFG_G1_128", b_f32=True,
         kshape=(1, 1, 1), bias="shared", res="sample", seed=902),
    dict(id="small-gemm-exact-s16", entry="gemm", cls="w_lo", dims=(1, 1, 256), parts=[288], cout=128, B=3, cfg="CFG_G1_128",
         kshape=(1, 1, 1), bias="sample", res="sample", seed=903),
]
