"""Class conditioning and classifier-free guidance on the GPU: md_cfg_combine / md_cfg_rescale against the restatements of
tests/cfg_cases.py, the conditional U-Net against the oracle (whose timestep-MLP bias takes the class row: algebraically the same
network), its class-embedding gradient, sampling.ClassifierFreeModel under the DDIM and ancestral samplers, and a training step
with class dropout and a checkpoint round trip.

Bars: one U-Net evaluation 1e-4 and a few sampler steps 1e-3 (tests/test_gpu_unet.py TOL_EVAL / TOL_SAMPLE, tests/test_gpu_ddim.py),
gradients 2e-3 per tensor and 5e-4 of the global norm (tests/test_gpu_train.py); the combine is held to one float32 ulp of the
float64 restatement, the rescale factor to the bar recorded in tests/golden/cfg.npz (tools/gen_golden_cfg.py)."""
import os

import numpy as np
import pytest
import torch

import cfg_cases as cc
from conftest import GOLD, rel_l2

pytestmark = pytest.mark.gpu

TOL_EVAL = 1e-4          # tests/test_gpu_unet.py
TOL_SAMPLE = 1e-3        # tests/test_gpu_unet.py, tests/test_gpu_ddim.py
NC = 3                   # classes of the small conditional model; NC is the null id


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from meshdiffusion_amd import hip_ops
    return hip_ops


def _small(num_classes=NC, precision=None, seed=1234):
    """(cfg, model in eval mode, state dict): tests/test_gpu_unet.py::_small_model with model.num_classes set."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    cfg = synth.small_config(); cfg.device = torch.device("cuda")
    cfg.model.num_classes = num_classes
    if precision is not None:
        cfg.model.hip_precision = precision
    model = mutils.create_model(cfg)
    R = cfg.data.image_size
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=seed, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    return cfg, model.eval(), sd


def _oracle_sd(sd, class_id):
    """The class-less state dict that is the same network under `class_id`: all_modules.1.bias takes the class row."""
    out = {k: v for k, v in sd.items() if k != "class_emb.weight"}
    out["all_modules.1.bias"] = sd["all_modules.1.bias"] + sd["class_emb.weight"][class_id]
    return out


@pytest.fixture(scope="module")
def net(ops):
    from meshdiffusion_amd import synth
    from oracle import unet_oracle as uo
    cfg, model, sd = _small()
    return dict(cfg=cfg, model=model, sd=sd, synth=synth, uo=uo, R=cfg.data.image_size)


# ---- 1. the combine kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cc.SIZES + cc.SIZES_UNALIGNED)
@pytest.mark.parametrize("B", cc.BATCHES)
def test_combine_within_one_ulp_of_float64_and_reproducible(ops, B, n):
    ec, eu, w = cc.combine_inputs(B, n)
    eps2 = torch.from_numpy(np.concatenate([ec, eu])).cuda()
    wt = torch.from_numpy(w).cuda()
    out, slabs, factor = ops.cfg_combine(eps2, wt, stats=True)
    plain = ops.cfg_combine(eps2, wt)                                    # without slabs: another grid, the same values
    want = cc.combine_restated(ec, eu, w).astype(np.float32)
    got = out.cpu().numpy()
    worst = int(cc.ulp_distance(got, want).max())
    print(f"combine {cc.case_id(B, n)} w {w.tolist()}: worst distance from the float64 restatement {worst} ulp")
    assert got.shape == (B, n) and worst <= 1
    assert torch.equal(plain, out) and factor.tolist() == [1.0] * B
    for b in range(B):
        if w[b] == 0.0:
            assert np.array_equal(got[b], eu[b])                         # exactly the null-class half
    # the slab sums: {ec, ec^2, out, out^2} in double, summing to the float64 sums of the tensors the kernel read and wrote
    s = slabs.sum(1).cpu().numpy()
    ref = np.stack([ec.astype(np.float64).sum(1), (ec.astype(np.float64) ** 2).sum(1), got.astype(np.float64).sum(1),
                    (got.astype(np.float64) ** 2).sum(1)], axis=1)
    scale = np.stack([np.abs(ec).astype(np.float64).sum(1), ref[:, 1], np.abs(got).astype(np.float64).sum(1), ref[:, 3]], axis=1)
    assert np.all(np.abs(s - ref) <= 1e-12 * scale)                      # double sums of n <= 16384 terms: n * 2^-53 at the worst
    # two runs: equal bits, slab sums included
    out2, slabs2, _ = ops.cfg_combine(eps2, wt, stats=True)
    assert torch.equal(out2, out) and torch.equal(slabs2, slabs)
    # a float for every sample is the per-sample vector of that float
    assert torch.equal(ops.cfg_combine(eps2, 3.0), ops.cfg_combine(eps2, torch.full((B,), 3.0, device="cuda")))


@pytest.mark.parametrize("B,n", [(1, 500), (3, 4 * 16 ** 3), (3, 499)])
def test_combine_propagates_nan_and_inf_in_place(ops, B, n):
    ec, eu, w = cc.combine_inputs(B, n, seed=1)
    w[:] = np.resize(np.array(cc.W_VALUES, np.float32), B)               # w = 0 among them: 0 * inf is NaN, not a finite value
    g = np.random.RandomState(3)
    pos = g.choice(B * n, size=12, replace=False)
    for k, p in enumerate(pos):
        half = (ec, eu)[k % 2]
        half.reshape(-1)[p] = (np.nan, np.inf, -np.inf)[k % 3]
    eps2 = torch.from_numpy(np.concatenate([ec, eu])).cuda()
    out, slabs, _ = ops.cfg_combine(eps2, torch.from_numpy(w).cuda(), stats=True)
    got = out.cpu().numpy()
    bad_in = ~(np.isfinite(ec) & np.isfinite(eu))
    assert bad_in.sum() == 12 and np.array_equal(~np.isfinite(got), bad_in)          # the same positions, no others
    assert np.array_equal(np.isnan(got), np.isnan(cc.combine_restated(ec, eu, w).astype(np.float32)))
    ok = ~bad_in
    assert int(cc.ulp_distance(got[ok], cc.combine_restated(ec, eu, w).astype(np.float32)[ok]).max()) <= 1
    # a sample with a non-finite value has non-finite sums and is left unscaled by the rescale; the others are scaled as ever
    res, _, f = ops.cfg_combine(eps2, torch.from_numpy(w).cuda(), rescale=0.7, stats=True)
    touched = bad_in.any(1)
    f = f.cpu().numpy()
    assert np.all(f[touched] == 1.0)
    for b in range(B):
        if touched[b]:
            assert np.array_equal(res[b].cpu().numpy(), got[b], equal_nan=True)


def test_combine_refuses_bad_arguments(ops):
    from meshdiffusion_amd import _lib
    eps2 = torch.zeros(4, 8, device="cuda")
    w = torch.ones(2, device="cuda")
    with pytest.raises(_lib.MeshDiffusionHipError):                      # out may alias neither half
        ops.call("md_cfg_combine", eps2, w, 2, 8, eps2[2:], None)
    with pytest.raises(_lib.MeshDiffusionHipError):
        ops.call("md_cfg_combine", eps2, w, 2, 8, eps2[:2], None)
    with pytest.raises(_lib.MeshDiffusionHipError):
        ops.call("md_cfg_combine", eps2, w, 0, 8, torch.zeros(2, 8, device="cuda"), None)
    with pytest.raises(_lib.MeshDiffusionHipError):                      # rescale needs the slabs; phi in [0, 1]
        ops.call("md_cfg_rescale", torch.zeros(2, 8, device="cuda"), None, 0.5, None, 2, 8)
    slabs = torch.zeros(2, 64, 4, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.MeshDiffusionHipError):
        ops.call("md_cfg_rescale", torch.zeros(2, 8, device="cuda"), slabs, 1.5, None, 2, 8)
    with pytest.raises(ValueError):
        ops.cfg_combine(eps2, w, rescale=-0.1)
    with pytest.raises(AssertionError):
        ops.cfg_combine(torch.zeros(3, 8, device="cuda"), w)


# ---- 2. guidance rescale -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", cc.PHIS)
@pytest.mark.parametrize("n", cc.SIZES + cc.SIZES_UNALIGNED)
@pytest.mark.parametrize("B", cc.BATCHES)
def test_rescale_factor_within_the_recorded_bar(ops, B, n, phi):
    gold = np.load(os.path.join(GOLD, "cfg.npz"))
    bar = float(gold[f"rescale/{cc.case_id(B, n)}/phi{phi}/bar"])
    ec, eu, w = cc.combine_inputs(B, n)
    eps2 = torch.from_numpy(np.concatenate([ec, eu])).cuda()
    wt = torch.from_numpy(w).cuda()
    plain = ops.cfg_combine(eps2, wt).cpu().numpy()
    res, slabs, f = ops.cfg_combine(eps2, wt, rescale=phi, stats=True)
    f = f.cpu().numpy()
    want = cc.rescale_factor_restated(ec, plain, phi)                    # float64, of the tensors the kernel read and wrote
    err = float(np.max(np.abs(f - want) / np.abs(want)))
    print(f"rescale {cc.case_id(B, n)} phi {phi}: factors {f.tolist()} worst relative distance from float64 {err:.2e}, bar {bar:.2e}")
    assert err <= bar
    # the values: one float32 product with the factor rounded to float32
    assert np.array_equal(res.cpu().numpy(), plain * f.astype(np.float32)[:, None])
    # without stats the same tensor; two runs the same bits
    again = ops.cfg_combine(eps2, wt, rescale=phi)
    assert torch.equal(again, res)


def test_rescale_leaves_a_constant_sample_unscaled(ops):
    n = 4 * 16 ** 3
    ec, eu, _ = cc.combine_inputs(3, n, seed=2)
    ec[1, :] = 0.3
    eu[1, :] = 0.3                                                       # out is 0.3 everywhere whatever w: std(out) = 0
    ec[2, :] = 0.0
    eu[2, :] = 0.0                                                       # and all zeros
    w = np.array([3.0, 3.0, 7.5], np.float32)
    eps2 = torch.from_numpy(np.concatenate([ec, eu])).cuda()
    plain = ops.cfg_combine(eps2, torch.from_numpy(w).cuda())
    res, _, f = ops.cfg_combine(eps2, torch.from_numpy(w).cuda(), rescale=1.0, stats=True)
    f = f.cpu().numpy()
    assert f[1] == 1.0 and f[2] == 1.0 and torch.equal(res[1:], plain[1:])
    assert np.all(plain[1].cpu().numpy() == np.float32(0.3)) and np.all(plain[2].cpu().numpy() == 0.0)
    want = cc.rescale_factor_restated(ec, plain.cpu().numpy(), 1.0)
    assert want[1] == 1.0 and want[2] == 1.0 and 0.0 < want[0] < 1.0 and abs(f[0] - want[0]) <= 1e-12 * want[0]       # double sums


# ---- 3. the conditional forward against the oracle --------------------------------------------------------------------------------
def test_conditional_forward_vs_oracle_with_the_class_row_in_the_bias(net):
    cfg, model, sd, synth, uo, R = (net[k] for k in ("cfg", "model", "sd", "synth", "uo", "R"))
    x1 = synth.synthetic_inputs(1, 4, R, seed=42)
    x = x1.expand(2, -1, -1, -1, -1).contiguous()                        # the same grid twice: the two rows differ by their class only
    labels = torch.tensor([417.0, 417.0])
    y = torch.tensor([1, NC])
    with torch.no_grad():
        out = model(x.cuda(), labels.cuda(), y=y).cpu()
        none = model(x.cuda(), labels.cuda()).cpu()                      # y=None: the null class for every sample
        ref = torch.cat([uo.unet_res64_forward(_oracle_sd(sd, int(c)), synth.oracle_cfg(cfg), x[b:b + 1], labels[b:b + 1])
                         for b, c in enumerate(y)])
    errs = [rel_l2(out[b], ref[b]) for b in range(2)]
    apart = rel_l2(out[0], out[1])
    print(f"conditional forward vs oracle: rel-L2 {errs[0]:.2e} (class 1) {errs[1]:.2e} (null); the two rows differ by {apart:.2e}")
    assert max(errs) < TOL_EVAL
    assert apart > 100 * TOL_EVAL                                         # a hundred bars: nothing the arithmetic could produce by itself
    assert torch.equal(none[1], out[1]) and rel_l2(none[0], ref[1]) < TOL_EVAL
    # ids are checked on the host, before any launch; a class-less model takes none
    for bad in ([1, NC + 1], [-1, 0], [1]):
        with pytest.raises(ValueError):
            model(x.cuda(), labels.cuda(), y=torch.tensor(bad))
    cfg0, model0, _ = _small(num_classes=0)
    with pytest.raises(ValueError, match="no classes"):
        model0(x.cuda(), labels.cuda(), y=torch.tensor([0, 0]))


# ---- 4. the same network with the row folded into the bias, on the device ------------------------------------------------------------
def test_conditional_model_equals_classless_model_with_the_row_in_its_bias():
    from meshdiffusion_amd import synth
    c = 2
    cfg, model, sd = _small(precision="bf16x3")
    cfg0, model0, _ = _small(num_classes=0, precision="bf16x3")
    model0.module.load_state_dict(_oracle_sd(sd, c), strict=True)
    x = synth.synthetic_inputs(1, 4, cfg.data.image_size, seed=43).cuda()
    labels = torch.tensor([850.0]).cuda()
    with torch.no_grad():
        a = model(x, labels, y=torch.tensor([c]))
        b = model0(x, labels)
        null = model(x, labels)
    e = rel_l2(a.cpu(), b.cpu())
    print(f"conditional model at y = {c} vs the class-less model with the row in all_modules.1.bias (bf16x3): rel-L2 {e:.2e}; "
          f"vs its own null class {rel_l2(a.cpu(), null.cpu()):.2e}")
    assert e < TOL_EVAL and rel_l2(a.cpu(), null.cpu()) > 100 * TOL_EVAL


# ---- 5. the gradient ---------------------------------------------------------------------------------------------------------------
def _train_backward(model, x, labels, y, cot):
    for p in model.parameters():
        p.grad = None
    model.train()
    try:
        model(x, labels, y=y).backward(cot)
    finally:
        model.eval()
    return {n: p.grad.detach().cpu().clone() for n, p in model.module.named_parameters() if p.grad is not None}


def test_class_embedding_gradient_vs_oracle_autograd(net):
    """One training-mode forward and backward at B = 2 with y = (2, 2).  The second run: md_channel_sums and the operand passes add
    the bias / FiLM gradients with float atomics (tests/test_gpu_dropout.py::_atomic_sums lists what derives from them), d_temb is
    such a sum, and d class_emb is a fixed-order sum of d_temb's rows: it repeats bit for bit exactly when d_temb does, which is
    what is asserted (row 2 against all_modules.1.bias.grad, the same two rows added once more); every gradient that derives
    from no atomic sum repeats bit for bit unconditionally."""
    from test_gpu_dropout import _atomic_sums
    cfg, model, sd, synth, uo, R = (net[k] for k in ("cfg", "model", "sd", "synth", "uo", "R"))
    B = 2
    mask = synth.synthetic_grid_mask(R).view(1, 1, R, R, R)
    x = synth.synthetic_inputs(B, 4, R, seed=8) * mask
    labels = torch.tensor([120.0, 733.0])
    y = torch.tensor([2, 2])
    cot = synth.synthetic_inputs(B, 4, R, seed=9) * mask / float(mask.sum())
    grads = _train_backward(model, x.cuda(), labels.cuda(), y, cot.cuda())
    # ---- torch autograd through the oracle, sample by sample, the class row substituted into the bias ----
    sdr = {k: v.clone().requires_grad_(v.dtype == torch.float32 and k not in ("coords", "mask")) for k, v in sd.items()}
    biases, outs = [], []
    for b in range(B):
        one = {k: v for k, v in sdr.items() if k != "class_emb.weight"}
        one["all_modules.1.bias"] = sdr["all_modules.1.bias"] + sdr["class_emb.weight"][int(y[b])]
        one["all_modules.1.bias"].retain_grad()
        biases.append(one["all_modules.1.bias"])
        outs.append(uo.unet_res64_forward(one, synth.oracle_cfg(cfg), x[b:b + 1], labels[b:b + 1]))
    (torch.cat(outs) * cot).sum().backward()
    assert set(grads) == {n for n, v in sdr.items() if v.grad is not None}
    gnorm = torch.sqrt(sum((sdr[n].grad.double() ** 2).sum() for n in grads))
    worst = ("", 0.0)
    for n, g in grads.items():
        r = sdr[n].grad
        err = float((g.double() - r.double()).norm() / gnorm)
        worst = max(worst, (n, err), key=lambda t: t[1])
        if float(r.norm()) > 1e-3 * float(gnorm):
            assert rel_l2(g, r) < 2e-3, n
    ce = grads["class_emb.weight"]
    per_sample = biases[0].grad + biases[1].grad
    e_row = rel_l2(ce[2], per_sample)
    print(f"d class_emb[2] vs the sum of the two per-sample bias gradients: rel-L2 {e_row:.2e} (|row| / |grad| = "
          f"{float(per_sample.norm() / gnorm):.2e}); worst tensor relative to the global gradient norm: {worst}")
    assert worst[1] < 5e-4
    assert e_row < 2e-3 and float(per_sample.norm()) > 0
    assert torch.equal(ce[[0, 1, 3]], torch.zeros(3, ce.shape[1]))       # absent classes and the null class: exactly zero
    assert torch.equal(ce[2], grads["all_modules.1.bias"])               # both samples in class 2: the batch sum of d_temb, same bits
    # ---- a second run ----
    grads2 = _train_backward(model, x.cuda(), labels.cuda(), y, cot.cuda())
    atomic = _atomic_sums(model.module) | {"class_emb.weight"}
    differ = [n for n in grads if n not in atomic and not torch.equal(grads[n], grads2[n])]
    temb_same = torch.equal(grads["all_modules.1.bias"], grads2["all_modules.1.bias"])
    ce_same = torch.equal(ce, grads2["class_emb.weight"])
    print(f"second run: {len(grads) - len(atomic & set(grads))} gradients without atomic sums, {len(differ)} differ; d_temb repeats bit for "
          f"bit: {temb_same}; d class_emb repeats bit for bit: {ce_same}")
    assert not differ
    assert ce_same == temb_same and torch.equal(grads2["class_emb.weight"][2], grads2["all_modules.1.bias"])
    assert torch.equal(grads2["class_emb.weight"][[0, 1, 3]], torch.zeros(3, ce.shape[1]))
    spread = float((grads2["class_emb.weight"].double() - ce.double()).norm() / gnorm)
    assert spread < 1e-5                                                  # tests/test_gpu_dropout.py: what the order of fp32 additions can cost


def test_class_row_sums_repeat_bit_for_bit_with_repeated_classes(net):
    """The reduction by itself, on one d_temb: 48 samples over 3 of 5 classes, twice -- equal bits, the float64 sums to float32
    rounding, exact zeros for the absent classes."""
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    cfg = net["synth"].small_config(); cfg.device = torch.device("cuda"); cfg.model.num_classes = 5
    m = mutils.create_model(cfg).module
    g = torch.Generator().manual_seed(4)
    d = torch.randn((48, 4 * m.nf), generator=g)
    ids = torch.tensor([0, 3, 5])[torch.randint(0, 3, (48,), generator=g)]
    a = m.class_row_sums(ids.cuda(), d.cuda())
    b = m.class_row_sums(ids.cuda(), d.cuda())
    assert torch.equal(a, b) and tuple(a.shape) == (6, 4 * m.nf)
    want = torch.zeros(6, 4 * m.nf, dtype=torch.float64).index_add_(0, ids, d.double())
    assert torch.equal(a[[1, 2, 4]].cpu(), torch.zeros(3, 4 * m.nf))
    absd = torch.zeros(6, 4 * m.nf, dtype=torch.float64).index_add_(0, ids, d.double().abs())
    assert bool(((a.cpu().double() - want).abs() <= 48 * 2.0 ** -24 * absd).all())      # at most 47 float32 additions per value


# ---- 6. the samplers take the wrapper as they take the U-Net ------------------------------------------------------------------------
class _WithY(torch.nn.Module):
    """The model called with `y` directly."""

    def __init__(self, model, y):
        super().__init__()
        self.model, self.y = model, y

    def forward(self, x, labels):
        return self.model(x, labels) if self.y is None else self.model(x, labels, y=self.y)


class _HostCFG(torch.nn.Module):
    """Both halves evaluated separately at batch B, combined on the host with the float64 restatement."""

    def __init__(self, model, y, w):
        super().__init__()
        self.model, self.y, self.w = model, y, np.asarray(w, np.float32)

    def forward(self, x, labels):
        ec = self.model(x, labels, y=self.y).cpu().numpy()
        eu = self.model(x, labels).cpu().numpy()
        B = ec.shape[0]
        out = cc.combine_restated(ec.reshape(B, -1), eu.reshape(B, -1), self.w).astype(np.float32)
        return torch.from_numpy(out.reshape(ec.shape)).to(x.device)


@pytest.mark.parametrize("method", ["ddim", "pc"])
def test_samplers_take_the_classifier_free_model(net, method):
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    cfg, model, synth, R = net["cfg"], net["model"], net["synth"], net["R"]
    cfg = cfg.copy_and_resolve()
    cfg.sampling.method, cfg.sampling.noise_removal = method, False
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, R, R, R)
    B = 2
    fn = sampling.get_sampling_fn(cfg, sde, (B, 4, R, R, R), lambda v: v, 1e-3, grid_mask=mask.cuda())
    y = torch.tensor([1, NC])                                             # a class and, per sample, the null id
    x_init = synth.synthetic_inputs(B, 4, R, seed=77)

    def run(m):
        torch.manual_seed(5)                                              # the ancestral prior and per-step noise; DDIM starts from x_init
        kw = dict(x0=x_init.cuda()) if method == "ddim" else {}
        out = fn(m, n_iters=3, **kw)[0]
        assert bool(torch.isfinite(out).all())
        return out

    CFM = sampling.ClassifierFreeModel
    direct, null = run(_WithY(model, y)), run(_WithY(model, None))
    assert torch.equal(run(CFM(model, y, scale=1.0)), direct)             # one evaluation with y: bit for bit
    assert torch.equal(run(CFM(model, y, scale=0.0)), null)               # one evaluation with the null class: bit for bit
    assert not torch.equal(direct, null)
    guided, host = run(CFM(model, y, scale=3.0)), run(_HostCFG(model, y, [3.0, 3.0]))
    e = rel_l2(guided.cpu(), host.cpu())
    moved = rel_l2(guided.cpu(), direct.cpu())
    print(f"{method}, 3 steps, cfg_scale 3: doubled evaluation + md_cfg_combine vs the host loop rel-L2 {e:.2e}; vs scale 1: {moved:.2e}")
    assert e < TOL_SAMPLE
    assert rel_l2(guided[1].cpu(), direct[1].cpu()) < TOL_SAMPLE          # sample 1 carries the null id: both halves are the null class
    per = run(CFM(model, torch.tensor([1, 2]), scale=[3.0, 0.0]))                    # a scale per sample
    assert rel_l2(per[0].cpu(), guided[0].cpu()) < TOL_SAMPLE and rel_l2(per[1].cpu(), null[1].cpu()) < TOL_SAMPLE      # w = 0: the null class
    resc = run(CFM(model, y, scale=3.0, rescale=0.7))
    assert not torch.equal(resc[0], guided[0]) and float((resc.cpu() * (1 - mask)).abs().max()) == 0.0
    # the out-of-scope list
    part = torch.zeros(1, 1, R, R, R).cuda()
    pm = (mask.view(1, 1, R, R, R) * 0.5 > 0.25).float().cuda()
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        fn(CFM(model, y, scale=3.0), partial=part, partial_mask=pm, guidance_scale=1.0)
    if method == "ddim":
        with pytest.raises(NotImplementedError, match="encode=True"):
            fn(CFM(model, y, scale=3.0), x0=x_init.cuda(), encode=True)


def test_graphed_stepper_takes_the_classifier_free_model(net):
    """The captured step replays the doubled evaluation and the combine: against the eager stepper on the same noise."""
    from meshdiffusion_amd.lib.diffusion import sampling, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import utils as mutils
    cfg, model, synth, R = net["cfg"], net["model"], net["synth"], net["R"]
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, R, R, R)
    st = sampling.AncestralStepper(sde, (2, 4, R, R, R), device="cuda", grid_mask=mask.cuda())
    wrapped = sampling.ClassifierFreeModel(model, torch.tensor([0, 2]), scale=2.0, rescale=0.5)
    fn = mutils.get_model_fn(wrapped)
    zs = [synth.synthetic_inputs(2, 4, R, seed=100 + i).cuda() for i in range(3)]
    x0 = (synth.synthetic_inputs(2, 4, R, seed=99) * mask).cuda()
    with torch.no_grad():
        xe = x0
        for i in range(3):
            xe, xme = st.step(fn, xe, i, draw=lambda t, i=i: zs[i])
        gs = sampling.GraphedStepper(st, fn, warmup=1)
        xg = x0
        for i in range(3):
            xg, xmg = gs.step(xg, i, draw=lambda t, i=i: zs[i])
    assert gs.graph is not None
    assert rel_l2(xmg.cpu(), xme.cpu()) < 1e-5 and bool(torch.isfinite(xmg).all())     # tests/test_gpu_unet.py: graphed vs eager


# ---- 7. a training step with class dropout, the checkpoint -----------------------------------------------------------------------------
def _train_state(cfg, model):
    from meshdiffusion_amd.lib.diffusion import losses
    from meshdiffusion_amd.lib.diffusion.models.ema import ExponentialMovingAverage
    ema = ExponentialMovingAverage(model.parameters(), decay=0.999)
    opt = losses.get_optimizer(cfg, model.parameters())
    return dict(model=model, ema=ema, optimizer=opt, step=1)


def test_train_steps_with_class_dropout_and_checkpoint_round_trip(tmp_path):
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    from meshdiffusion_amd.lib.diffusion.utils import restore_checkpoint, save_checkpoint
    cfg, model, _ = _small()
    cfg.optim.warmup = 2                                                  # a learning rate above 0 from state["step"] = 1 on
    R, B = cfg.data.image_size, 4
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, 1, R, R, R).cuda()
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), mask=mask, class_dropout=0.5)
    batch = (synth.synthetic_inputs(B, 4, R, seed=8) * mask.cpu()).cuda()
    y = torch.tensor([0, 1, 1, 0])                                        # class 2 is never seen
    state = _train_state(cfg, model)
    before = model.module.class_emb.weight.detach().cpu().clone()
    seen = set()
    for seed in (321, 322):
        torch.manual_seed(seed)
        loss = float(step_fn(state, (batch, y))["loss"].detach())
        torch.manual_seed(seed)                                           # the step's draws once more: timesteps, noise, then the class draw
        torch.randint(0, 1000, (B,), device="cuda")
        torch.randn_like(batch)
        dropped = (torch.rand(B, device="cuda") < 0.5).cpu()
        seen |= set(torch.where(dropped, torch.full_like(y, NC), y).tolist())
        print(f"train step (seed {seed}): loss {loss:.5f}, dropped {dropped.tolist()}")
        assert np.isfinite(loss)
        g = model.module.class_emb.weight.grad.detach().cpu()
        present = set(torch.where(dropped, torch.full_like(y, NC), y).tolist())
        for c in range(NC + 1):
            assert bool((g[c] != 0).any()) == (c in present), (c, present)
    after = model.module.class_emb.weight.detach().cpu()
    moved = {c for c in range(NC + 1) if not torch.equal(after[c], before[c])}
    print(f"classes seen over the two steps {sorted(seen)}, rows that moved {sorted(moved)}")
    assert moved == seen and 2 not in moved and {0, 1} & moved
    assert state["step"] == 3 and state["ema"].num_updates == 2
    ema_row = state["ema"].shadow_params[-1].detach().cpu().clone()
    assert ema_row.shape == after.shape and not torch.equal(ema_row, before) and not torch.equal(ema_row, after)
    # ---- checkpoint round trip into fresh objects ----
    path = str(tmp_path / "checkpoint.pth")
    save_checkpoint(path, state)
    cfg2, model2, _ = _small(seed=99)
    state2 = _train_state(cfg2, model2)
    assert not torch.equal(model2.module.class_emb.weight.detach().cpu(), after)
    state2 = restore_checkpoint(path, state2, device="cuda")
    assert torch.equal(model2.module.class_emb.weight.detach().cpu(), after)
    assert torch.equal(state2["ema"].shadow_params[-1].detach().cpu(), ema_row) and state2["step"] == 3
    assert "module.class_emb.weight" in torch.load(path, map_location="cpu", weights_only=False)["model"]
    # the restored model evaluates as the trained one
    x = batch[:2]
    lab = torch.tensor([500.0, 20.0]).cuda()
    with torch.no_grad():
        assert torch.equal(model2.eval()(x, lab, y=torch.tensor([0, 1])), model.eval()(x, lab, y=torch.tensor([0, 1])))
    # ids are checked before anything is drawn; a class-less model takes no ids
    with pytest.raises(ValueError):
        step_fn(state, (batch, torch.tensor([0, 1, 1, NC + 1])))
    cfg0, model0, _ = _small(num_classes=0)
    with pytest.raises(ValueError, match="no classes"):
        step_fn(_train_state(cfg0, model0), (batch, y))


def test_classless_train_step_ignores_class_dropout():
    """With a class-less model the step draws what it drew before class conditioning existed, whatever class_dropout says: the same
    loss and the same updated weights, bit for bit where no float atomic sum is involved (the loss is one such value)."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    R = 16
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, 1, R, R, R).cuda()
    batch = (synth.synthetic_inputs(2, 4, R, seed=8) * mask.cpu()).cuda()
    got = []
    for p in (0.1, 0.9):
        cfg, model, _ = _small(num_classes=0)
        cfg.optim.warmup = 2
        step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), mask=mask, class_dropout=p)
        torch.manual_seed(11)
        loss = step_fn(_train_state(cfg, model), batch)["loss"].detach().cpu()
        got.append((loss, torch.rand(4, device="cuda").cpu()))            # and the device generator stands where it stood
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
