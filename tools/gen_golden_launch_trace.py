"""Records tests/golden/launch_trace.json.gz: which exports of libmeshdiffusion_hip.so the U-Net's host path calls, in which order and
with which scalar arguments, for a set of small scenarios on both sides of every dispatch boundary of the 3x3x3 convolutions.

    python tools/gen_golden_launch_trace.py [--out tests/golden/launch_trace.json.gz]

Run it on the GPU, on the commit whose dispatch is the reference (the PARENT of a change to layers.run_conv3 / hip_ops that must not
move a launch).  tests/test_gpu_launch_trace.py replays the same scenario functions and compares element for element: routes that
are bit-identical by construction (block pass vs. prep + NIN, compact vs. full upsampled operand, prep v2 vs. v1) cannot be told
apart by any numerical test.

How: `meshdiffusion_amd._lib.load` is replaced by a proxy around the real library handle (every module calls `_lib.load()` per
launch).  Per call the proxy records the export name, every integer argument exactly, every float as its repr and of every pointer
only whether it is null; of md_gemm_conv the scalar fields and pointer null-ness of its MdGemmConvArgs; of md_pack_batch the scalar
fields of its job table (taken from the host copy hip_ops uploads: torch.frombuffer is watched while recording).  No addresses, no
events, no timings.  The scenarios drive public entry points only (create_model(cfg)(x, labels), forward_train / backward,
layer.forward_blocked / backward_blocked, precision_scope), so this file runs unmodified before and after such a change."""
import argparse
import contextlib
import ctypes as C
import gc
import gzip
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from meshdiffusion_amd import _lib, hip_ops as ops, synth  # noqa: E402
from meshdiffusion_amd.config import get_config_res64  # noqa: E402
from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, layers, utils as mutils  # noqa: E402,F401

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.json.gz")
_JOB_SCALARS = [n for n, t in _lib.MdPackJob._fields_ if t is not C.c_void_p]


def _scalar(ctype, v):
    if ctype in (C.c_float, C.c_double):
        return "f:" + repr(float(v))
    if ctype in (C.c_int, C.c_int32, C.c_int64, C.c_uint64):
        return int(v)
    if isinstance(v, C.c_void_p):          # a pointer: null or not, never the address
        v = v.value
    return "null" if not v else "ptr"


class _Recorder:
    """Stands in for the ctypes library handle: same attributes, every call of a declared export noted in `trace`."""

    def __init__(self, lib):
        self._lib, self.trace, self.table = lib, [], None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        sig = _lib.SIGNATURES.get(name)
        if sig is None:
            return fn

        def call(*args):
            assert len(args) == len(sig[1]), name
            rec = [name]
            for ctype, a in zip(sig[1], args):
                if ctype == C.POINTER(_lib.MdGemmConvArgs):
                    rec.append({f: _scalar(t, getattr(a._obj, f)) for f, t in _lib.MdGemmConvArgs._fields_})
                else:
                    rec.append(_scalar(ctype, a))
            if name == "md_pack_batch":    # the job table lives on the device: its scalars from the host copy that was uploaded
                n = int(args[1])
                assert self.table is not None and len(self.table) == n * C.sizeof(_lib.MdPackJob), "md_pack_batch: host table not seen"
                jobs = (_lib.MdPackJob * n).from_buffer_copy(self.table)
                rec.append([[int(getattr(j, f)) for f in _JOB_SCALARS] for j in jobs])
            self.trace.append(rec)
            return fn(*args)
        return call


@contextlib.contextmanager
def recording():
    """with recording() as trace: every library call made inside is appended to `trace`."""
    real_load, real_frombuffer = _lib.load, torch.frombuffer
    rec = _Recorder(real_load())

    def frombuffer(buf, *a, **kw):
        rec.table = bytes(buf)
        return real_frombuffer(buf, *a, **kw)
    _lib.load, torch.frombuffer = (lambda: rec), frombuffer
    try:
        yield rec.trace
    finally:
        _lib.load, torch.frombuffer = real_load, real_frombuffer


def record(scenario):
    """The trace of one scenario function, from a clean host state: no packing job or pack-use note left by earlier work in this
    process (both would add launches in an order that depends on object addresses), dropout seeds pinned."""
    gc.collect()
    ops.prewarm_packs()
    torch.manual_seed(0)
    with recording() as trace, torch.no_grad():
        scenario()
    torch.cuda.synchronize()
    return json.loads(json.dumps(trace))       # what the golden holds after a round trip (lists, not tuples)


# ---------------------------------------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------------------------------------
def _f32b(B, Cc, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, Cc // 8, S ** 3, 8), generator=g).cuda()


def _loaded(layer, seed=3):
    layer.load_state_dict(synth.sensitised_state_dict(layer.state_dict(), seed=seed))
    return layer.cuda().eval()


def _model(cfg):
    cfg.device = torch.device("cuda")
    model = mutils.create_model(cfg)
    R = cfg.data.image_size
    model.module.load_state_dict(synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R)),
                                 strict=True)
    return model.eval(), R


def small_eval_then_train():
    """a: every direct / generic route, stem, head, unfused attention, split-K with statistics."""
    model, R = _model(synth.small_config())
    x, labels = synth.synthetic_inputs(2, 4, R).cuda(), torch.tensor([100.0, 700.0]).cuda()
    model(x, labels)
    net = model.module.train()
    out, ctx = net.forward_train(x, labels)
    net.backward(ctx, torch.ones_like(out))


def _resblock(cin, cout, S, B, scope, split=None, sites=None, dropout=0.0):
    def run():
        blk = _loaded(layers.ResnetBlockDDPM(act=torch.nn.SiLU(), in_ch=cin, out_ch=cout, temb_dim=128, dropout=dropout))
        if sites is not None:
            blk.md_bf16x3_sites = sites
        parts = [(_f32b(B, c, S, 10 + i), c) for i, c in enumerate(split or (cin,))]
        temb = torch.randn((B, 128), generator=torch.Generator().manual_seed(2)).cuda()
        with ops.precision_scope(scope):
            blk.forward_blocked(parts, B, S ** 3, temb)
    return run


def _resblock_train(S, B):
    def run():
        blk = _loaded(layers.ResnetBlockDDPM(act=torch.nn.SiLU(), in_ch=128, out_ch=128, temb_dim=128, dropout=0.1)).train()
        temb = torch.randn((B, 128), generator=torch.Generator().manual_seed(2)).cuda()
        tape = []
        with ops.precision_scope(None, training=True):
            blk.forward_blocked([(_f32b(B, 128, S, 10), 128)], B, S ** 3, temb, tape=tape)
            blk.backward_blocked(tape[0], _f32b(B, 128, S, 11))
    return run


def _upsample(S_in, measured=False):
    def run():
        up = _loaded(layers.Upsample(128, with_conv=True))
        if measured:
            up._md_act_ms = {"w": torch.ones(128, dtype=torch.float32, device="cuda")}
        with ops.precision_scope("f16f6"):
            up.forward_blocked(_f32b(8, 128, S_in, 12), 128, 8, S_in ** 3)
    return run


def _downsample(S_in):
    def run():
        down = _loaded(layers.Downsample(128, with_conv=True))
        with ops.precision_scope("bf16x3"):
            down.forward_blocked(_f32b(1, 128, S_in, 13), 128, 1, S_in ** 3)
    return run


def _attn(taped):
    def run():
        blk = _loaded(layers.AttnBlock(256))
        with ops.precision_scope("bf16x3"):
            blk.forward_blocked(_f32b(1, 256, 8, 14), 1, 512, tape=[] if taped else None)
    return run


def res64_eval():
    """h: the registered res64 configuration in its own precision, B = 1."""
    model, R = _model(get_config_res64())
    model(synth.synthetic_inputs(1, 4, R).cuda(), torch.tensor([500.0]).cuda())


SCENARIOS = {
    "a_small_eval_then_train": small_eval_then_train,
    "b_res128_s32_f16f6": _resblock(128, 128, 32, 1, "f16f6"),            # wino_ok at exactly 128 workgroups, f6
    "b_res128_s16_f16f6": _resblock(128, 128, 16, 1, "f16f6"),            # below the floor: fused-loader direct kernel
    "b_res128_s32_bf16x3": _resblock(128, 128, 32, 1, "bf16x3"),
    "b_res128_s32_f16f8": _resblock(128, 128, 32, 1, "f16f8"),
    "c_nin_s32_block_pass": _resblock(256, 128, 32, 1, "f16f6"),          # P = 32768: the block pass's lower bound
    "c_nin_s16_b8": _resblock(256, 128, 16, 8, "f16f6"),                  # Winograd, shortcut by the GEMM on fp32 parts
    "c_nin_s32_parts_72_184": _resblock(256, 128, 32, 1, "f16f6", split=(72, 184)),   # f8, no block pass
    "c_nin_s32_demoted_w0": _resblock(256, 128, 32, 1, "f16f6", sites={"w0"}),
    "d_ups_8_uncalibrated": _upsample(8),                                  # compact operand, raw stream -> bf16x3
    "d_ups_8_measured": _upsample(8, measured=True),                       # measured equaliser -> f6, compact
    "d_ups_4": _upsample(4),                                               # neither compact nor Winograd
    "e_down_64": _downsample(64),                                          # md_conv3_s2 at 128 workgroups
    "e_down_32": _downsample(32),                                          # generic stride-2 tile
    "f_attn_fused": _attn(False),
    "f_attn_unfused": _attn(True),
    "g_train_s32_b2": _resblock_train(32, 2),                              # kept T, dual f6 operand, md_wgrad_wino, dynamic lift
    "g_train_s32_b1": _resblock_train(32, 1),                              # S16B activations, md_wgrad
    "h_res64_eval_b1": res64_eval,
}


def first_difference(got, want):
    """None when the traces are equal, else a sentence naming the first differing launch."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g == w:
            continue
        if g[0] != w[0]:
            return f"launch {i}: export {g[0]} where the golden has {w[0]}"
        for k, (ga, wa) in enumerate(zip(g[1:], w[1:])):
            if ga != wa:
                if isinstance(ga, dict) and isinstance(wa, dict):      # MdGemmConvArgs: only the fields that differ
                    fields = [f for f in ga if ga[f] != wa.get(f)]
                    ga, wa = {f: ga[f] for f in fields}, {f: wa.get(f) for f in fields}
                return f"launch {i}: {g[0]} argument {k}: {ga} where the golden has {wa}"
        return f"launch {i}: {g[0]} with {len(g) - 1} arguments where the golden has {len(w) - 1}"
    if len(got) != len(want):
        longer = got if len(got) > len(want) else want
        return f"{len(got)} launches where the golden has {len(want)}; first unmatched: {longer[min(len(got), len(want))][0]}"
    return None


def load_golden(path=GOLDEN):
    with gzip.open(path, "rt") as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--commit", default="", help="hash of the commit this runs on (stored in the file)")
    a = ap.parse_args()
    gold = {"commit": a.commit, "scenarios": {}}
    for name, fn in SCENARIOS.items():
        gold["scenarios"][name] = record(fn)
        print(f"{name}: {len(gold['scenarios'][name])} calls", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with gzip.GzipFile(a.out, "wb", mtime=0) as f:
        f.write(json.dumps(gold, separators=(",", ":")).encode())
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
