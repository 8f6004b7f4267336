"""Training-step pieces on the HIP path (csrc/train.hip) vs their PyTorch definitions."""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def test_perturb_bit_exact_and_masked_loss(hip_lib):
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    B, Cc, S = 3, 4, 8
    x0, noise, eh = _rand((B, Cc, S, S, S), 1), _rand((B, Cc, S, S, S), 2), _rand((B, Cc, S, S, S), 3)
    mask = (torch.rand(1, 1, S, S, S, generator=torch.Generator().manual_seed(4)) < 0.3).float()
    labels = torch.tensor([0, 417, 999])
    xt = losses.ddpm_perturb(sde, x0.cuda(), labels.cuda(), noise.cuda(), mask.reshape(-1).cuda()).cpu()
    sa, s1 = sde.sqrt_alphas_cumprod.cpu(), sde.sqrt_1m_alphas_cumprod.cpu()
    ref = (sa[labels, None, None, None, None] * x0 + s1[labels, None, None, None, None] * noise) * mask
    assert torch.equal(xt, ref)
    sums, grad = losses.masked_sq_err(eh.cuda(), noise.cuda(), mask.reshape(-1).cuda(), want_grad=True, gscale=0.5)
    ref_l = (torch.square(eh - noise) * mask).double().reshape(B, -1).sum(-1)
    assert rel_l2(sums.cpu(), ref_l) < 1e-7
    assert rel_l2(grad.cpu(), 0.5 * 2 * (eh - noise) * mask) < 1e-7


def test_fused_clip_adam_ema_matches_torch(hip_lib):
    """FusedAdamEMA against torch's clip_grad_norm_ + Adam + EMA, four steps from one state, twice: through the EMA's warm-up
    (d = 2/11, 3/12, ...) and late in training (d = 0.9999).  Parameters are 1e-3 randn with lr = 1e-3 and the shadow starts at an
    independent 1e-5 randn, so that one step moves both by amounts fp32 resolves: besides the parameters and the shadow themselves,
    the INCREMENTS of every step are compared -- with float64 under the rounding-count bounds of tests/stream_cases.py, and with
    torch's own increments under the sum of both sides' bounds (each side's float64 step taken from its own fp32 state, and from
    the norm it clipped with)."""
    import stream_cases as sc
    from meshdiffusion_amd.lib.diffusion.losses import FusedAdamEMA
    from meshdiffusion_amd.lib.diffusion.models.ema import ExponentialMovingAverage
    shapes = [(64, 32, 3, 3, 3), (64,), (257, 5), (1000,)]
    lr0 = 1e-3
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu()
    for updates0 in (0, 10 ** 6):
        ref_p = [torch.nn.Parameter(1e-3 * _rand(s, 10 + i).cuda()) for i, s in enumerate(shapes)]
        my_p = [torch.nn.Parameter(p.detach().clone()) for p in ref_p]
        opt = torch.optim.Adam(ref_p, lr=lr0, betas=(0.9, 0.999), eps=1e-8)
        ema = ExponentialMovingAverage(ref_p, decay=0.9999)
        fused = FusedAdamEMA(my_p, lr=lr0, grad_clip=1.0, warmup=5)
        for i, (s, mine) in enumerate(zip(ema.shadow_params, fused.ema_shadow_params())):
            s.copy_(1e-5 * _rand(shapes[i], 50 + i).cuda())
            mine.copy_(s)
        ema.num_updates = fused.ema_updates = updates0
        for step in range(1, 5):
            grads = [_rand(s, 100 * step + i).cuda() * (3.0 if step == 2 else 0.01) for i, s in enumerate(shapes)]
            for p, q, g in zip(ref_p, my_p, grads):
                p.grad = g.clone()
                q.grad.copy_(g)
            lr = float(lr0 * np.minimum(step / 5, 1.0))
            for gr in opt.param_groups:
                gr["lr"] = lr
            zeros = [torch.zeros_like(p) for p in ref_p]
            before_t = dict(p=flat(ref_p), m=flat([opt.state[p]["exp_avg"] for p in ref_p] if step > 1 else zeros),
                            v=flat([opt.state[p]["exp_avg_sq"] for p in ref_p] if step > 1 else zeros), ema=flat(ema.shadow_params))
            before_f = dict(p=fused.flat.cpu(), m=fused.m.cpu(), v=fused.v.cpu(), ema=fused.ema.cpu())
            g_flat = flat(grads)
            total_norm = torch.nn.utils.clip_grad_norm_(ref_p, max_norm=1.0)
            opt.step()
            ema.update(ref_p)
            fused.step(step)
            for p, q, s in zip(ref_p, my_p, ema.shadow_params):
                assert rel_l2(q.detach().cpu(), p.detach().cpu()) < 1e-6
            for mine, s in zip(fused.ema_shadow_params(), ema.shadow_params):
                assert rel_l2(mine.cpu(), s.cpu()) < 1e-6
            assert rel_l2(fused.m.cpu(), flat([opt.state[p]["exp_avg"] for p in ref_p])) < 1e-6
            assert rel_l2(fused.v.cpu(), flat([opt.state[p]["exp_avg_sq"] for p in ref_p])) < 1e-6
            # the increments of this step
            common = dict(n=g_flat.numel(), step=step, wd=0.0, g=g_flat, lr=lr, b1=0.9, b2=0.999, eps=1e-8, max_norm=1.0,
                          d=sc.ema_decay(0.9999, updates0 + step), clip="norm")
            assert ema.num_updates == fused.ema_updates == updates0 + step
            ref_f = sc.adam_reference(dict(common, sq=float((g_flat.double() ** 2).sum()), **before_f), sq_rel_err=2 * sc.U)
            ref_t = sc.adam_reference(dict(common, sq=float(total_norm.double()) ** 2, **before_t))
            got_f = (fused.flat.cpu(), fused.m.cpu(), fused.v.cpu(), fused.ema.cpu())
            w = sc.adam_worst(got_f, dict(common, **before_f), ref_f)
            print(f"fused adam updates0={updates0} step {step} (d = {common['d']:.6f}): worst err/bound vs float64 "
                  + ", ".join(f"{k} {x:.3f}" for k, x in w.items()))
            assert max(w.values()) <= 1.0, w
            for key, new_f, new_t, e in (("p", fused.flat.cpu(), flat(ref_p), "e_dp"), ("ema", fused.ema.cpu(), flat(ema.shadow_params), "e_dema")):
                inc_f = new_f.double() - before_f[key].double()
                inc_t = new_t.double() - before_t[key].double()
                r = "dp" if key == "p" else "dema"
                allowed = ref_f[e] + ref_t[e] + (ref_f[r] - ref_t[r]).abs()
                worst = float(((inc_f - inc_t).abs() / allowed).max())
                print(f"    increment of {key} vs torch: worst difference/allowed {worst:.3f}")
                assert worst <= 1.0


def test_eval_step_fn_matches_oracle_loss(hip_lib):
    """get_step_fn(train=False): loss under EMA weights, end to end on the HIP path, vs the oracle."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    from meshdiffusion_amd.lib.diffusion.models.ema import ExponentialMovingAverage
    from oracle import unet_oracle as uo
    cfg = synth.small_config(); cfg.device = torch.device("cuda")
    model = mutils.create_model(cfg)
    R = cfg.data.image_size
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    ema = ExponentialMovingAverage(model.parameters(), decay=0.999)
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, 1, R, R, R).cuda()
    step_fn = losses.get_step_fn(sde, train=False, mask=mask)
    batch = (synth.synthetic_inputs(2, 4, R, seed=8) * mask.cpu()).cuda()
    torch.manual_seed(123)
    loss = float(step_fn(dict(model=model, ema=ema, step=0), batch)["loss"])
    # oracle: same RNG stream (labels, noise drawn on the device in the same order)
    torch.manual_seed(123)
    labels = torch.randint(0, 1000, (2,), device="cuda")
    noise = torch.randn_like(batch)
    b, n, m, lb = batch.cpu(), noise.cpu(), mask.cpu(), labels.cpu()
    _, sa, s1 = uo.vpsde_tables()
    xt = (sa[lb, None, None, None, None] * b + s1[lb, None, None, None, None] * n) * m
    with torch.no_grad():
        e = uo.unet_res64_forward(sd, synth.oracle_cfg(cfg), xt, lb)
    ls = (torch.square(e - n) * m).reshape(2, -1).mean(-1)
    ref = float(ls.mean() / m.sum() * m.numel())
    assert abs(loss - ref) / abs(ref) < 1e-4


@pytest.mark.parametrize("arch,B", [("ddpm_res64", 8), ("ddpm_res128", 8), ("ddpm_res128", 1), ("ddpm_res64", 3)])
def test_whole_unet_backward_and_train_step_vs_oracle_autograd(hip_lib, arch, B):
    """get_step_fn(train=True) on the HIP path (forward, loss, backward, reference optimize_fn) vs the same step
    computed with torch autograd through the oracle on the CPU: every parameter gradient and the updated weights.
    ddpm_res128: 5x5x5 stem / mask_layer / head, no coords, 2 blocks at level 0; B = 1 is its per-GPU batch in the
    reference config (8 over 8 GPUs), B = 3: a batch that is not a multiple of the 8-sample wgrad block."""
    import copy
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, ddpm_res128, utils as mutils  # noqa: F401
    from meshdiffusion_amd.lib.diffusion.models.ema import ExponentialMovingAverage
    from oracle import unet_oracle as uo
    cfg = synth.small_config() if arch == "ddpm_res64" else synth.small_config_res128()
    cfg.device = torch.device("cuda")
    cfg.optim.warmup = 2
    cfg.optim.grad_clip = -1.0        # keep p.grad unscaled so it can be compared with autograd's gradient
    model = mutils.create_model(cfg)
    R = cfg.data.image_size
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    params = [p for p in model.parameters()]
    ema = ExponentialMovingAverage(model.parameters(), decay=0.999)
    opt = losses.get_optimizer(cfg, model.parameters())
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, 1, R, R, R).cuda()
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), mask=mask)
    batch = (synth.synthetic_inputs(B, 4, R, seed=8) * mask.cpu()).cuda()
    state = dict(model=model, ema=ema, optimizer=opt, step=1)
    torch.manual_seed(321)
    w_before = {n: p.detach().cpu().clone() for n, p in model.module.named_parameters()}
    loss = float(step_fn(state, batch)["loss"].detach())
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.module.named_parameters() if p.grad is not None}
    # ---- reference: autograd through the oracle, same labels/noise stream ----
    torch.manual_seed(321)
    labels = torch.randint(0, 1000, (B,), device="cuda").cpu()
    noise = torch.randn_like(batch).cpu()
    b, m = batch.cpu(), mask.cpu()
    _, sa, s1 = uo.vpsde_tables()
    xt = (sa[labels, None, None, None, None] * b + s1[labels, None, None, None, None] * noise) * m
    sdr = {k: v.clone().requires_grad_(v.dtype == torch.float32 and k not in ("coords", "mask")) for k, v in sd.items()}
    e = uo.unet_res64_forward(sdr, synth.oracle_cfg(cfg), xt, labels)
    ls = (torch.square(e - noise) * m).reshape(B, -1).mean(-1)
    ref_loss = ls.mean() / m.sum() * m.numel()
    ref_loss.backward()
    assert abs(loss - float(ref_loss)) / float(ref_loss) < 1e-4
    worst = ("", 0.0)
    gnorm = torch.sqrt(sum((sdr[n].grad.double() ** 2).sum() for n in grads))
    for n, g in grads.items():
        r = sdr[n].grad
        err = float((g.double() - r.double()).norm() / gnorm)     # error relative to the whole gradient
        if err > worst[1]:
            worst = (n, err)
        if float(r.norm()) > 1e-3 * float(gnorm):
            assert rel_l2(g, r) < 2e-3, n
    print("worst per-tensor error relative to the global grad norm:", worst)
    assert worst[1] < 5e-4
    assert set(grads) == {n for n, v in sdr.items() if v.grad is not None}
    # the optimizer really stepped (reference optimize_fn: warm-up lr 2e-5 * 1/2, Adam) and the EMA moved
    moved = [n for n, p in model.module.named_parameters() if p.requires_grad and not torch.equal(p.detach().cpu(), w_before[n])]
    assert len(moved) == len(grads) and state["step"] == 2 and ema.num_updates == 1


@pytest.mark.parametrize("case", ["small_res64", "small_res128", "res64", "res64_b2", "res64_trained", "res64_b2_drop"])
def test_loss_and_gradients_vs_reference_golden(hip_lib, case):
    """The UNMODIFIED reference loss function run on the CPU by oracle/gen_golden.py (train mode, dropout 0, fixed
    labels/noise) pins loss and every parameter gradient of the HIP path -- `res64` is the real 364 M-parameter
    network at B = 1 (the autograd reference takes 40 s on the build host; here only its recorded norms/samples);
    `res64_b2` (train_grads_b2.npz) the same at B = 2, where the 32^3 levels run through the Winograd forward /
    data-gradient kernels as well (hip_ops.wino_ok), so those are pinned to the reference's autograd at two grid sizes;
    `res64_trained` (train_grads_trained.npz) the real network at B = 1 on the adversarial trained-like weights of round 5 (heavy tails,
    2^U(-3,3) GroupNorm gammas): training runs bf16x3, which has no block scale to upset.
    `res64_b2_drop` (train_grads_drop.npz) is `res64_b2` with dropout 0.1, the setting both shipped configurations train with and
    bench.py times: the reference ran with every block's Dropout_0 replaced by the seeded mask of tests/dropout_cases.py, and the
    HIP path pops the stored seeds, one per ResnetBlock in forward order, through a patched hip_ops.next_dropout_seed.  The mask
    inside the kept Winograd operand, md_wgrad_wino and the f16f6 data gradients are on the reference's autograd here."""
    import os
    from conftest import GOLD
    from oracle.gen_golden import fixed_draws, train_step_inputs
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.config import get_config_res64
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, ddpm_res128, utils as mutils  # noqa: F401
    gfile = {"res64_b2": "train_grads_b2.npz", "res64_trained": "train_grads_trained.npz",
             "res64_b2_drop": "train_grads_drop.npz"}.get(case, "train_grads.npz")
    if not os.path.exists(os.path.join(GOLD, gfile)):
        pytest.skip(f"{gfile} not generated")
    gold = np.load(os.path.join(GOLD, gfile))
    cfg = {"small_res64": synth.small_config, "small_res128": synth.small_config_res128, "res64": get_config_res64,
           "res64_b2": get_config_res64, "res64_trained": get_config_res64, "res64_b2_drop": get_config_res64}[case]()
    cfg.device = torch.device("cuda")
    drop_seeds = [int(s) for s in gold[f"{case}_seeds"]] if case == "res64_b2_drop" else None
    cfg.model.dropout = float(gold[f"{case}_p"]) if drop_seeds else 0.0
    assert not drop_seeds or cfg.model.dropout == 0.1
    R, B = cfg.data.image_size, int(gold[f"{case}_B"])
    model = mutils.create_model(cfg)
    make = synth.trained_like_state_dict if case.endswith("_trained") else synth.sensitised_state_dict
    sd = make(model.module.state_dict(), seed=int(gold[f"{case}_sd_seed"]), grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    del sd
    batch, labels, noise, mask = train_step_inputs(B, R, seed=2024)
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cuda")
    loss_fn = losses.get_ddpm_loss_fn(sde, train=True, mask=mask.cuda())
    from meshdiffusion_amd import hip_ops
    wino_launches = []
    real_wino = hip_ops.conv3_wino
    hip_ops.conv3_wino = lambda ww, t, B_, S_, **kw: (wino_launches.append(S_), real_wino(ww, t, B_, S_, **kw))[1]
    wgrad_launches = []
    real_wgrad, real_seed = hip_ops.wgrad_wino, hip_ops.next_dropout_seed
    hip_ops.wgrad_wino = lambda u, t, B_, co, ci, S_, dw, **kw: (wgrad_launches.append(S_), real_wgrad(u, t, B_, co, ci, S_, dw, **kw))[1]
    if drop_seeds:
        left = list(drop_seeds)
        hip_ops.next_dropout_seed = lambda: left.pop(0)       # IndexError if the net asks for more masks than the reference had blocks
    try:
        with fixed_draws(labels.cuda(), noise.cuda()):
            loss = loss_fn(model, batch.cuda())
        loss.backward()
    finally:
        hip_ops.conv3_wino, hip_ops.wgrad_wino, hip_ops.next_dropout_seed = real_wino, real_wgrad, real_seed
    if case in ("res64_b2", "res64_b2_drop"):      # the point of these cases: Winograd launches (forward and data gradient) at both grid sizes
        assert hip_ops.WINO and wino_launches.count(64) >= 20 and wino_launches.count(32) >= 20, sorted(set(wino_launches))
    if drop_seeds:
        assert not left, f"{len(left)} of {len(drop_seeds)} stored seeds were not drawn"
        print(f"{case}: md_wgrad_wino launches at 64^3: {wgrad_launches.count(64)}, at 32^3: {wgrad_launches.count(32)}")
        assert wgrad_launches.count(64) > 0 and wgrad_launches.count(32) > 0, wgrad_launches
    ref_loss = float(gold[f"{case}_loss"])
    assert abs(float(loss.detach()) - ref_loss) / ref_loss < 2e-5
    gnorm = float(gold[f"{case}_gnorm"])
    worst, n_checked, sq = ("", 0.0), 0, 0.0
    for n, p in model.module.named_parameters():
        key = f"{case}/{n}/norm"
        if key not in gold.files:
            assert p.grad is None or not p.requires_grad, n
            continue
        g = p.grad.detach().flatten()
        sq += float(g.double().square().sum())
        stride = max(1, g.numel() // 256)
        smp, ref = g[::stride][:256].cpu().double(), torch.from_numpy(gold[f"{case}/{n}/sample"]).double()
        rn = float(gold[key])
        assert abs(float(g.double().norm()) - rn) <= 2e-3 * rn + 1e-5 * gnorm, n
        # sampled entries: error measured against the RMS entry of this tensor (and the global norm for tiny tensors)
        scale = max(rn / g.numel() ** 0.5, 1e-4 * gnorm / g.numel() ** 0.5)
        err = float((smp - ref).abs().max()) / scale
        if err > worst[1]:
            worst = (n, err)
        n_checked += 1
    print(f"{case}: {n_checked} tensors, worst sampled-entry error / RMS entry = {worst}")
    assert n_checked > 100 and worst[1] < 2e-3
    assert abs(sq ** 0.5 - gnorm) / gnorm < 1e-4


def test_fused_optimizer_under_reference_objects_matches_torch_path(hip_lib, tmp_path):
    """get_step_fn runs clip + Adam + EMA as md_grad_sqnorm + md_adam_ema_step over flat buffers while the caller keeps
    torch.optim.Adam / ExponentialMovingAverage objects: parameters, Adam moments, EMA shadow params after 3 steps must
    equal the torch-kernel path (MD_FUSED_OPT off), and a reference-format checkpoint written in between must restore
    into fresh objects and continue identically."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    from meshdiffusion_amd.lib.diffusion.models.ema import ExponentialMovingAverage
    from meshdiffusion_amd.lib.diffusion.utils import restore_checkpoint, save_checkpoint

    def fresh():
        cfg = synth.small_config(); cfg.device = torch.device("cuda")
        cfg.optim.warmup, cfg.optim.lr, cfg.optim.grad_clip = 4, 1e-3, 1.0
        model = mutils.create_model(cfg)
        R = cfg.data.image_size
        sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
        model.module.load_state_dict(sd, strict=True)
        ema = ExponentialMovingAverage(model.parameters(), decay=0.999)
        opt = losses.get_optimizer(cfg, model.parameters())
        sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
        mask = synth.synthetic_grid_mask(R).view(1, 1, R, R, R).cuda()
        step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), mask=mask)
        batch = (synth.synthetic_inputs(4, 4, R, seed=8) * mask.cpu()).cuda()
        return dict(model=model, ema=ema, optimizer=opt, step=1), step_fn, batch

    def run(fused, n, state=None, step_fn=None, batch=None, first=0):
        old, losses.FUSED_OPT = losses.FUSED_OPT, fused
        try:
            if state is None:
                state, step_fn, batch = fresh()
            for k in range(first, first + n):
                torch.manual_seed(100 + k)
                step_fn(state, batch)
        finally:
            losses.FUSED_OPT = old
        return state, step_fn, batch

    def snapshot(state):
        ps = [p.detach().cpu().clone() for p in state["model"].parameters() if p.requires_grad]
        es = [s.detach().cpu().clone() for s in state["ema"].shadow_params]
        osd = state["optimizer"].state_dict()["state"]
        ms = [osd[i]["exp_avg"].detach().cpu().clone() for i in sorted(osd)]
        return ps, es, ms

    def rel(xs, ys):
        num = sum(float((a.double() - b.double()).pow(2).sum()) for a, b in zip(xs, ys))
        return (num / max(sum(float(b.double().pow(2).sum()) for b in ys), 1e-300)) ** 0.5

    st_f, fn_f, batch = run(True, 2)
    assert st_f["model"].module.__dict__.get("_md_flat_opt") is not None, "the fused path did not engage"
    ck = str(tmp_path / "ck.pth")
    save_checkpoint(ck, st_f)
    st_f, _, _ = run(True, 1, st_f, fn_f, batch, first=2)
    st_t, _, _ = run(False, 3)
    assert st_t["model"].module.__dict__.get("_md_flat_opt") is None
    a, b = snapshot(st_f), snapshot(st_t)
    errs = [rel(x, y) for x, y in zip(a, b)]
    print("fused vs torch optimizer path after 3 steps: params / ema / exp_avg rel", errs)
    assert max(errs) < 2e-5 and st_f["step"] == st_t["step"] == 4 and st_f["ema"].num_updates == st_t["ema"].num_updates == 3
    # checkpoint written after step 2 by the fused path -> fresh objects -> step 3 == the uninterrupted run
    st_r, fn_r, _ = fresh()
    st_r = restore_checkpoint(ck, st_r, torch.device("cuda"))
    assert st_r["step"] == 3
    st_r, _, _ = run(True, 1, st_r, fn_r, batch, first=2)
    c = snapshot(st_r)
    errs = [rel(x, y) for x, y in zip(c, a)]
    print("restored-from-checkpoint continuation vs uninterrupted:", errs)
    assert max(errs) < 2e-6
    # the same fused-written checkpoint resumed through the TORCH optimizer (MD_FUSED_OPT off = the reference's
    # torch.optim.Adam): every parameter's Adam `step` must advance by exactly 1 per optimizer.step() (a `step` tensor shared
    # by all entries would advance once per parameter) and the result must equal the uninterrupted torch-path run
    st_q, fn_q, _ = fresh()
    st_q = restore_checkpoint(ck, st_q, torch.device("cuda"))
    steps0 = {float(e["step"]) for e in st_q["optimizer"].state_dict()["state"].values()}
    assert steps0 == {2.0}
    ptrs = {e["step"].data_ptr() for e in st_q["optimizer"].state.values()}
    assert len(ptrs) == len(st_q["optimizer"].state), "Adam step tensors alias each other after the restore"
    st_q, _, _ = run(False, 1, st_q, fn_q, batch, first=2)
    steps1 = {float(e["step"]) for e in st_q["optimizer"].state_dict()["state"].values()}
    assert steps1 == {3.0}, steps1
    errs = [rel(x, y) for x, y in zip(snapshot(st_q), b)]
    print("fused-written checkpoint continued by torch.optim.Adam vs the all-torch run:", errs)
    assert max(errs) < 2e-5


def test_flat_optimizer_state_follows_replaced_parameter_storage(hip_lib):
    """parameters whose storage is replaced after the first fused step (p.data = ..., model.float(), ...) no
    longer alias the flat buffer: the flat state must be rebuilt from the live parameters instead of updating an orphan."""
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    from meshdiffusion_amd.lib.diffusion.models.ema import ExponentialMovingAverage
    cfg = synth.small_config(); cfg.device = torch.device("cuda")
    cfg.optim.warmup, cfg.optim.lr, cfg.optim.grad_clip = 0, 1e-3, 1.0
    model = mutils.create_model(cfg)
    R = cfg.data.image_size
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    ema = ExponentialMovingAverage(model.parameters(), decay=0.999)
    opt = losses.get_optimizer(cfg, model.parameters())
    sde = sde_lib.VPSDE(0.1, 20.0, 1000, device="cuda")
    mask = synth.synthetic_grid_mask(R).view(1, 1, R, R, R).cuda()
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), mask=mask)
    batch = (synth.synthetic_inputs(2, 4, R, seed=8) * mask.cpu()).cuda()
    state = dict(model=model, ema=ema, optimizer=opt, step=1)
    torch.manual_seed(1); step_fn(state, batch)
    fs0 = model.module.__dict__.get("_md_flat_opt")
    assert fs0 is not None and fs0.params_alias_flat()
    for p in model.parameters():                       # what model.float() / a manual reassignment does
        p.data = p.data.clone()
    assert not fs0.params_alias_flat()
    before = [p.detach().clone() for p in model.parameters() if p.requires_grad]
    torch.manual_seed(2); step_fn(state, batch)
    fs1 = model.module.__dict__.get("_md_flat_opt")
    assert fs1 is not fs0 and fs1.params_alias_flat()
    moved = sum(float((p.detach() - q).abs().sum()) for p, q in zip((p for p in model.parameters() if p.requires_grad), before))
    assert moved > 0, "the live parameters did not train after their storage was replaced"
    assert fs1.opt_steps == 2                          # Adam state (incl. the step count) carried over


def test_res64_batch8_training_gradients_winograd_vs_direct_kernels(hip_lib):
    """the whole res64 loss + backward at the bench / training batch (B = 8), with the Winograd
    forward and data-gradient convs (64^3, 32^3 AND 16^3 levels at this batch) and once with the direct kernels
    (MD_WINO=0, the build pinned to the reference's autograd by `res64` / `res64_b2` above): loss and all 494 parameter
    gradients must agree to 5e-5 in the same arithmetic (bf16x3 data gradients: hip_ops.DGRAD_F6 off).  Round 6: the shipped
    configuration runs the data-gradient convs of the Winograd layers in f16f6 (1.7e-5 per conv, accumulating along the ~20
    convs between the loss and the stem): all gradients together stay under 5e-5, the worst single tensor under 1e-4."""
    from oracle.gen_golden import fixed_draws, train_step_inputs
    from meshdiffusion_amd import hip_ops, synth
    from meshdiffusion_amd.config import get_config_res64
    from meshdiffusion_amd.lib.diffusion import losses, sde_lib
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, utils as mutils  # noqa: F401
    cfg = get_config_res64(); cfg.device = torch.device("cuda")
    cfg.model.dropout = 0.0
    R, B = 64, 8
    model = mutils.create_model(cfg)
    sd = synth.sensitised_state_dict(model.module.state_dict(), seed=1234, grid_mask=synth.synthetic_grid_mask(R))
    model.module.load_state_dict(sd, strict=True)
    del sd
    batch, labels, noise, mask = train_step_inputs(B, R, seed=2024)
    sde = sde_lib.VPSDE(cfg.model.beta_min, cfg.model.beta_max, cfg.model.num_scales, device="cuda")
    loss_fn = losses.get_ddpm_loss_fn(sde, train=True, mask=mask.cuda())
    runs = {}
    keep, keep_f6 = hip_ops.WINO, hip_ops.DGRAD_F6
    try:
        for key, wino, f6 in (("wino_f6", True, True), ("wino", True, False), ("direct", False, False)):
            hip_ops.WINO, hip_ops.DGRAD_F6 = wino, f6
            seen, seen_f6 = [], []
            real = hip_ops.conv3_wino

            def spy(ww, t, B_, S_, **kw):
                seen.append(S_)
                if isinstance(ww, hip_ops.WinoWeightF6Dgrad):
                    seen_f6.append(S_)
                return real(ww, t, B_, S_, **kw)
            hip_ops.conv3_wino = spy
            try:
                for p in model.parameters():
                    p.grad = None
                with fixed_draws(labels.cuda(), noise.cuda()):
                    loss = loss_fn(model, batch.cuda())
                loss.backward()
            finally:
                hip_ops.conv3_wino = real
            runs[key] = (float(loss.detach()), {n: p.grad.detach().cpu().clone() for n, p in model.module.named_parameters()
                                                if p.grad is not None}, sorted(set(seen)), len(seen_f6))
    finally:
        hip_ops.WINO, hip_ops.DGRAD_F6 = keep, keep_f6
    (l0, g0, s0, n0) = runs["direct"]
    assert s0 == [] and n0 == 0
    assert len(g0) == 494
    gsq = sum(float(g.double().square().sum()) for g in g0.values())
    ntot = sum(g.numel() for g in g0.values())
    for key, bar_all, bar_worst in (("wino", 5e-5, 5e-5), ("wino_f6", 5e-5, 1e-4)):
        l1, g1, s1, n1 = runs[key]
        assert s1 == [16, 32, 64], s1
        assert (n1 >= 20) if key == "wino_f6" else (n1 == 0), n1          # the f16f6 data-gradient launches really ran / really did not
        assert abs(l1 - l0) <= 2e-6 * abs(l0), (l1, l0)
        assert g1.keys() == g0.keys()
        num, worst = 0.0, ("", 0.0)
        for n in g0:
            d = float((g1[n].double() - g0[n].double()).square().sum())
            num += d
            # per tensor: relative to its own norm, floored at the norm an average-sized entry would give this tensor
            floor = (gsq / ntot * g0[n].numel()) ** 0.5 * 1e-2
            e = d ** 0.5 / max(float(g0[n].double().norm()), floor)
            if e > worst[1]:
                worst = (n, e)
        print(f"res64 B=8 training gradients, Winograd ({'f16f6' if key == 'wino_f6' else 'bf16x3'} data gradients) vs direct kernels: loss "
              f"{l1:.6f} / {l0:.6f}, all gradients rel-L2 {(num / gsq) ** 0.5:.3e}, worst tensor {worst}")
        assert (num / gsq) ** 0.5 < bar_all and worst[1] < bar_worst
