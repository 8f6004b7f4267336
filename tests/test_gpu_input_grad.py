"""The U-Net's input gradient on the HIP path: md_conv3_stem_dgrad against a float64 conv (bit for bit on exact inputs), the
whole-net d eps_hat / dx against torch autograd through the oracle, and the data-gradient-only backward (param_grads=False): no
weight-gradient work, no `.grad`, same data gradients."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _randint(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _stem_dgrad_weight(ops, w):
    """W [co][ci][3][3][3] -> the packed rows (ci, kw) of the flipped, transposed weight (include/meshdiffusion_hip.h)."""
    wt = w.flip(2, 3, 4).transpose(0, 1)                                  # W'[ci][co][kd][kh][kw]
    w2 = wt.permute(0, 4, 1, 2, 3).reshape(wt.shape[0] * 3, wt.shape[1], 3, 3, 1).contiguous()
    return ops.PackedWeight(w2.cuda(), "conv", ops.CFG_HEAD_PACK, torch.device("cuda", 0))


def _stem_dgrad(ops, w, g0, dims):
    B, ci = g0.shape[0], w.shape[1]
    y = ops.conv3_stem_dgrad(_stem_dgrad_weight(ops, w), ops.ncdhw_to_f32b(g0.cuda()), B, None, 16, dims=dims)
    return ops.fold_dx(y, None, B, ci, 3, 16, None, dims=dims).cpu()


def _conv_input_f64(w, g0, dims):
    k = w.shape[-1]
    return torch.nn.grad.conv3d_input((g0.shape[0], w.shape[1]) + tuple(dims), w.double(), g0.double(), padding=k // 2)


@pytest.mark.parametrize("nf", [32, 128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dims", [(4, 8, 8), (8, 8, 16), (16, 16, 16)])
def test_stem_dgrad_kernel(hip_lib, dims, B, nf):
    """(4, 8, 8): one tile, every position at a border; (8, 8, 16): several tiles along z and x; 16^3: along all three."""
    from meshdiffusion_amd import hip_ops as ops
    assert ops.conv3_stem_dgrad_ok(nf, *dims)
    # small integers: bf16x3 holds them exactly and every partial sum (<= 27 * 128 * 8 * 4 < 2^24) is exact in fp32
    w, g0 = _randint((nf, 4, 3, 3, 3), -4, 4, 1), _randint((B, nf) + dims, -8, 8, 2)
    out, ref = _stem_dgrad(ops, w, g0, dims), _conv_input_f64(w, g0, dims)
    assert out.shape == ref.shape and torch.equal(out.double(), ref), float((out.double() - ref).abs().max())
    w, g0 = _randn((nf, 4, 3, 3, 3), 3), _randn((B, nf) + dims, 4)
    out, ref = _stem_dgrad(ops, w, g0, dims), _conv_input_f64(w, g0, dims)
    err = rel_l2(out, ref)
    print(f"md_conv3_stem_dgrad nf={nf} B={B} {dims}: rel-L2 {err:.2e}")
    assert err < 2e-4
    assert torch.equal(out, _stem_dgrad(ops, w, g0, dims))              # the same bits on a second launch


def _model(cfg_fn, centered=True, train=False):
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, ddpm_res128, utils as mutils  # noqa: F401
    cfg = cfg_fn()
    cfg.device = torch.device("cuda", 0)
    cfg.data.centered = centered
    R = cfg.data.image_size
    model = mutils.create_model(cfg)
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    model.train(train)
    return cfg, model, sd


@pytest.mark.parametrize("k", [3, 5])
def test_stem_dgrad_routes_of_the_model(hip_lib, k):
    """The 5x5x5 stem (ddpm_res128) goes through the generic dx-folded tile; so does the 3x3x3 one where the kernel does not
    apply.  Both against the same float64 reference; the factor 2 of a non-centered input is in the result."""
    from meshdiffusion_amd import hip_ops as ops, synth
    cfg, model, sd = _model(synth.small_config if k == 3 else synth.small_config_res128, centered=(k == 5))
    net, R, B = model.module, cfg.data.image_size, 2
    stem = net.all_modules[2]
    assert stem.weight.shape[-1] == k
    g0 = _randn((B, net.nf, R, R, R), 5)
    ref = _conv_input_f64(stem.weight.detach().cpu(), g0, (R, R, R)) * (1.0 if k == 5 else 2.0)

    def run():
        ops.PROFILE = []
        try:
            with torch.no_grad(), ops.precision_scope(None, training=True):
                out = net._stem_dgrad(stem, ops.ncdhw_to_f32b(g0.cuda()), B, R).cpu()
            return out, [r[0] for r in ops.PROFILE]
        finally:
            ops.PROFILE = None
    out, tags = run()
    assert ("stem_dgrad" in tags) == (k == 3)
    err = rel_l2(out, ref)
    print(f"stem data gradient k={k}: rel-L2 {err:.2e} ({tags})")
    assert err < 2e-4
    if k == 3:
        ok = ops.conv3_stem_dgrad_ok
        ops.conv3_stem_dgrad_ok = lambda *a: False
        try:
            out2, tags2 = run()
        finally:
            ops.conv3_stem_dgrad_ok = ok
        assert "stem_dgrad" not in tags2 and rel_l2(out2, ref) < 2e-4


def _oracle_input_grad(sd, cfg, x, labels, cot, centered=True):
    from meshdiffusion_amd import synth
    from oracle import unet_oracle as uo
    xr = x.clone().requires_grad_(True)
    e = uo.unet_res64_forward(sd, synth.oracle_cfg(cfg), xr if centered else 2 * xr - 1.0, labels)
    return e.detach(), torch.autograd.grad(e, xr, cot)[0]


def _forbid_param_work(monkeypatch):
    from meshdiffusion_amd import hip_ops as ops
    from meshdiffusion_amd.lib.diffusion.models import backward as bw

    def forbidden(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called by a data-gradient-only backward")
        return f
    for name in ("wgrad", "to_pb16", "wgrad_nin", "channel_sums", "_grad_of"):
        monkeypatch.setattr(bw, name, forbidden(name))
    for name in ("wgrad_wino", "wgrad_nin", "bump_param_epoch"):
        monkeypatch.setattr(ops, name, forbidden(name))


@pytest.mark.parametrize("arch,B,centered", [("res64", 2, True), ("res64", 3, True), ("res128", 1, True), ("res64", 2, False)])
def test_whole_net_input_gradient(hip_lib, monkeypatch, arch, B, centered):
    """Eval mode, x.requires_grad: x.grad against autograd through the oracle (2e-3 rel-L2, the whole-net gradient bar of
    test_gpu_train.py); no parameter gets a `.grad`, no weight-gradient kernel is launched."""
    from meshdiffusion_amd import hip_ops as ops, synth
    cfg, model, sd = _model(synth.small_config if arch == "res64" else synth.small_config_res128, centered=centered)
    R = cfg.data.image_size
    x = _randn((B, 4, R, R, R), 11) * 0.7 + (0.0 if centered else 0.5)
    labels = torch.tensor([37.0, 611.5, 998.0][:B])
    cot = _randn((B, 4, R, R, R), 12)
    e_ref, g_ref = _oracle_input_grad(sd, cfg, x, labels, cot, centered)
    hook_calls = []
    model.module.__dict__["_grad_ready_hook"] = lambda ps: hook_calls.append(len(ps))
    _forbid_param_work(monkeypatch)
    xg = x.cuda().requires_grad_(True)
    ops.PROFILE = []
    try:
        out = model(xg, labels.cuda())
        out.backward(cot.cuda())
        tags = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert xg.grad is not None and xg.grad.shape == x.shape and xg.grad.dtype == torch.float32
    err_f, err_g = rel_l2(out.detach(), e_ref), rel_l2(xg.grad, g_ref)
    print(f"{arch} B={B} centered={centered}: forward rel-L2 {err_f:.2e}, input gradient rel-L2 {err_g:.2e}")
    assert err_f < 1e-4 and err_g < 2e-3
    assert all(p.grad is None for p in model.parameters()) and not hook_calls
    assert not [t for t in tags if "wgrad" in str(t)] and ("stem_dgrad" in tags) == (arch == "res64")
    with pytest.raises(RuntimeError):            # differentiable once: the tape is gone
        out.backward(cot.cuda())
    # under no_grad, or without x.requires_grad, the inference path runs as before
    with torch.no_grad():
        out2 = model(x.cuda(), labels.cuda())
    assert not out2.requires_grad and rel_l2(out2, e_ref) < 1e-4
    assert not model(x.cuda(), labels.cuda()).requires_grad


def test_training_mode_hands_back_the_same_input_gradient(hip_lib):
    """Training mode with x.requires_grad: the same x.grad as in eval mode (dropout 0), and parameter gradients bit-identical to
    a training backward that was not asked for the input gradient -- for every gradient that IS reproducible: two identical
    training backwards differ in the gradients that are accumulated with float atomics (bias and FiLM channel sums, the timestep
    MLP behind them: 48 of the 176 tensors of this net, measured).  Those are named by category, everything else must be
    bit-identical, and each of them is held on its own to the spread of three identical backwards that did not ask for x.grad."""
    from meshdiffusion_amd import synth
    cfg, model, sd = _model(synth.small_config, train=True)
    R, B = cfg.data.image_size, 2
    x, labels, cot = _randn((B, 4, R, R, R), 11) * 0.7, torch.tensor([37.0, 611.5]), _randn((B, 4, R, R, R), 12)

    def run(want_dx, train=True):
        model.train(train)
        for p in model.parameters():
            p.grad = None
        xg = x.cuda().requires_grad_(want_dx)
        model(xg, labels.cuda()).backward(cot.cuda())
        return xg.grad, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    dx0, g0 = run(False)
    base = [g0, run(False)[1], run(False)[1]]
    dx1, g1 = run(True)
    dx2, g2 = run(True, train=False)
    assert dx0 is None and g0 and not g2 and all(set(g) == set(g1) for g in base)

    def atomic(n):
        """Gradients that end in float atomics (csrc/backward.hip: md_channel_sums, the ch_sums of md_gn_bwd_apply) or are derived
        from such sums: conv / NIN / Linear biases, the FiLM table (Dense_0) and the timestep MLP behind it."""
        leaf = n.split(".")[-1]
        return ((leaf in ("bias", "b") and "GroupNorm" not in n) or n.endswith("Dense_0.weight")
                or n.endswith(("all_modules.0.weight", "all_modules.1.weight")))
    exact = [n for n in g0 if not atomic(n)]
    loose = [n for n in g0 if atomic(n)]
    assert len(exact) > len(loose) > 0
    differ = [n for n in exact if not torch.equal(g0[n], g1[n])]
    assert not differ, differ

    def dist(a, b):
        return float(torch.linalg.vector_norm(a.double() - b.double()))
    worst = ("", 0.0)
    for n in loose:          # each tensor on its own: within three times the spread of three identical backwards without x.grad
        spread = max(dist(base[i][n], base[k][n]) for i in range(3) for k in range(i))
        got = max(dist(g1[n], b[n]) for b in base)
        floor = 4 * torch.finfo(torch.float32).eps * float(torch.linalg.vector_norm(g0[n].double()))
        ratio = got / max(spread, floor, 1e-300)
        worst = max(worst, (n, ratio), key=lambda v: v[1])
        assert got <= 3 * spread + floor, (n, got, spread)
    print(f"{len(exact)} gradients bit-identical; {len(loose)} atomic sums, worst distance / run-to-run spread {worst[1]:.2f} ({worst[0]})")
    _, g_ref = _oracle_input_grad(sd, cfg, x, labels, cot)
    print(f"training-mode input gradient rel-L2 {rel_l2(dx1, g_ref):.2e}; against eval mode {rel_l2(dx1, dx2):.2e}")
    assert rel_l2(dx1, g_ref) < 2e-3 and rel_l2(dx1, dx2) < 5e-5


def test_golden_input_gradient(hip_lib, gold_dir):
    """The input gradient stored with tests/golden/likelihood.npz (oracle, fixed cotangent, t = 0.5)."""
    import os
    import numpy as np
    import likelihood_cases as lc
    from meshdiffusion_amd import synth
    gold = np.load(os.path.join(gold_dir, "likelihood.npz"))
    cfg, model, sd = _model(synth.small_config)
    _, gm, x0 = lc.golden_setup()
    R = cfg.data.image_size
    xg = x0.cuda().requires_grad_(True)
    model(xg, torch.full((2,), 0.5 * 999).cuda()).backward(synth.synthetic_inputs(2, 4, R, seed=9).cuda())
    err = rel_l2(xg.grad, torch.from_numpy(gold["input_grad"]))
    print(f"golden input gradient rel-L2 {err:.2e}")
    assert err < 2e-3


@pytest.mark.parametrize("B,cin_parts,cout,S,wgrad_tag", [(16, (128, 128), 128, 16, "wgrad_nin"), (2, (128,), 128, 32, "wgrad_wino")])
def test_resnet_block_data_gradients_only_through_winograd_path(hip_lib, monkeypatch, B, cin_parts, cout, S, wgrad_tag):
    """The block of test_resnet_block_training_through_winograd_path, and one at 32^3 whose full backward takes the dual operand
    pass + md_wgrad_wino (+ the f16f6 data-gradient conv), with param_grads=False: the single operand pass + the bf16x3 Winograd
    conv per data gradient, no weight-gradient launch, no `.grad`; the data gradients are the full backward's (5e-5, that test's
    bar for two routes of one gradient) and bit-equal to the full backward's bf16x3 route, whose kernels these are."""
    from meshdiffusion_amd import hip_ops as ops, synth
    from meshdiffusion_amd.lib.diffusion.models import layers
    p = 0.1
    cin, P = sum(cin_parts), S ** 3
    assert ops.wino_ok(cout, cin, S, B) and ops.WINO and ops.WINO_TRAIN_FWD
    blk = layers.ResnetBlockDDPM(act=torch.nn.SiLU(), in_ch=cin, out_ch=cout, temb_dim=128, dropout=p)
    blk.load_state_dict(synth.sensitised_state_dict(blk.state_dict(), seed=5))
    blk = blk.cuda().train()
    parts = [(ops.ncdhw_to_f32b(_randn((B, c, S, S, S), 20 + i).cuda()), c) for i, c in enumerate(cin_parts)]
    temb, dy = _randn((B, 128), 22).cuda(), ops.ncdhw_to_f32b(_randn((B, cout, S, S, S), 23).cuda())
    tape = []
    with torch.no_grad():
        blk.forward_blocked(parts, B, P, temb, tape=tape)

        def run(**kw):
            ops.PROFILE = []
            try:
                dparts, dbias0 = blk.backward_blocked(tape[0], dy, **kw)
                return [d.clone() for d in dparts], dbias0, [e[0] for e in ops.PROFILE]
            finally:
                ops.PROFILE = None
        full, db_full, tags_full = run()
        assert wgrad_tag in tags_full and db_full is not None
        f6 = ops.DGRAD_F6
        ops.DGRAD_F6 = False
        try:
            full3, _, _ = run()
        finally:
            ops.DGRAD_F6 = f6
        for q in blk.parameters():
            q.grad = None
        _forbid_param_work(monkeypatch)
        only, db_only, tags = run(param_grads=False)
    assert db_only is None and all(q.grad is None for q in blk.parameters())
    assert tags.count("wino") == 2 and tags.count("wino_prep") == 2 and not [t for t in tags if "wgrad" in str(t)], tags
    for a, b, c in zip(only, full, full3):
        print(f"data gradient: vs full backward {rel_l2(a, b):.2e}, vs its bf16x3 route {rel_l2(a, c):.2e}")
        assert rel_l2(a, b) < 5e-5
        assert torch.equal(a, c)
