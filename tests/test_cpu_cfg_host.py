"""Class conditioning and classifier-free guidance, the host side (no GPU): what model.num_classes adds to the state dict and
what it leaves alone, the restatements of tests/cfg_cases.py on hand-computed values, the labelled dataset, the order of the
training step's draws, and the configuration plumbing of the generation drivers."""
import json
import os

import numpy as np
import pytest
import torch

import cfg_cases as cc
from conftest import GOLD


def _small(num_classes=None):
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res64, ddpm_res128, utils as mutils  # noqa: F401
    cfg = synth.small_config()
    cfg.device = torch.device("cpu")
    if num_classes is not None:
        cfg.model.num_classes = num_classes
    return cfg, mutils.create_model(cfg, use_parallel=False)


# ---- model: keys, order, checks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_classes", [None, 0])
def test_classless_model_keeps_its_keys_and_parameter_order(num_classes):
    gold = np.load(os.path.join(GOLD, "cfg.npz"))
    cfg, m = _small(num_classes)
    assert cfg.model.num_classes == 0 and m.num_classes == 0 and not hasattr(m, "class_emb")
    assert list(m.state_dict().keys()) == gold["unet_small_keys"].tolist()
    assert [n for n, _ in m.named_parameters()] == gold["unet_small_params"].tolist()


def test_conditional_model_adds_one_key_last():
    gold = np.load(os.path.join(GOLD, "cfg.npz"))
    _, m = _small(3)
    keys, params = list(m.state_dict().keys()), [n for n, _ in m.named_parameters()]
    assert keys == gold["unet_small_keys"].tolist() + ["class_emb.weight"]
    assert params == gold["unet_small_params"].tolist() + ["class_emb.weight"]
    w = m.state_dict()["class_emb.weight"]
    assert tuple(w.shape) == (4, 4 * m.nf) and w.dtype == torch.float32 and m.null_class == 3
    assert 0.01 < float(w.std()) < 0.04                                      # N(0, 0.02)
    order = m.grad_completion_order()
    assert order[-1] is m.class_emb.weight and sum(p is m.class_emb.weight for p in order) == 1
    # the class-less parameters come in the order they have without classes
    names = {id(p): n for n, p in m.named_parameters()}
    _, m0 = _small(0)
    names0 = {id(p): n for n, p in m0.named_parameters()}
    assert [names[id(p)] for p in order[:-1]] == [names0[id(p)] for p in m0.grad_completion_order()]


def test_res128_takes_classes_too():
    from meshdiffusion_amd import synth
    from meshdiffusion_amd.lib.diffusion.models import ddpm_res128, utils as mutils  # noqa: F401
    cfg = synth.small_config_res128()
    cfg.device = torch.device("cpu")
    k0 = list(mutils.create_model(cfg, use_parallel=False).state_dict().keys())
    cfg.model.num_classes = 5
    m = mutils.create_model(cfg, use_parallel=False)
    assert list(m.state_dict().keys()) == k0 + ["class_emb.weight"] and tuple(m.class_emb.weight.shape) == (6, 4 * m.nf)


def test_class_ids_are_checked_on_the_host():
    _, m = _small(3)
    _, m0 = _small(0)
    assert m.class_ids(None, 2, "cpu").tolist() == [3, 3]                     # None: the null class for every sample
    ids = m.class_ids(torch.tensor([1, 3]), 2, "cpu")
    assert ids.tolist() == [1, 3] and ids.dtype == torch.int64 and m.class_ids(ids, 2, "cpu") is ids
    assert m.class_ids([0, 2], 2, "cpu").tolist() == [0, 2]
    for bad in ([1, 4], [-1, 0], [1], [[1, 2]], torch.tensor([0.0, 1.0])):
        with pytest.raises(ValueError):
            m.class_ids(bad, 2, "cpu")
    assert m0.class_ids(None, 2, "cpu") is None
    with pytest.raises(ValueError, match="no classes"):
        m0.class_ids([0, 0], 2, "cpu")
    with pytest.raises(ValueError):
        cfg, _ = _small(0)
        cfg.model.num_classes = -1
        from meshdiffusion_amd.lib.diffusion.models import utils as mutils
        mutils.create_model(cfg, use_parallel=False)


# ---- the restatements on hand-computed values --------------------------------------------------------------------------------
def test_combine_restatement_on_hand_values():
    ec = np.array([[3.0, 1.0, -2.0, 0.5]], np.float32)
    eu = np.array([[1.0, 1.0, 2.0, 0.25]], np.float32)
    for w, want in ((2.0, [5.0, 1.0, -6.0, 0.75]), (0.0, [1.0, 1.0, 2.0, 0.25]), (1.0, [3.0, 1.0, -2.0, 0.5]), (-0.5, [0.0, 1.0, 4.0, 0.125]),
                    (7.5, [16.0, 1.0, -28.0, 2.125])):
        got = cc.combine_restated(ec, eu, np.array([w], np.float32))
        assert got.dtype == np.float64 and got.tolist() == [want], (w, got)
    # the subtraction is the contract's float32 one: 1 - 2^-30 is 1 in float32, so d = 0 although the operands differ in double
    got = cc.combine_restated(np.array([[1.0]], np.float32), np.array([[2.0 ** -30]], np.float32), np.array([4.0], np.float32))
    assert got.tolist() == [[4.0 + 2.0 ** -30]]
    # per-sample w
    got = cc.combine_restated(np.array([[2.0], [2.0]], np.float32), np.array([[1.0], [1.0]], np.float32), np.array([0.0, 3.0], np.float32))
    assert got.tolist() == [[1.0], [4.0]]
    # non-finite values propagate
    got = cc.combine_restated(np.array([[np.inf, np.nan, 1.0]], np.float32), np.array([[1.0, 1.0, -np.inf]], np.float32), np.array([3.0], np.float32))
    assert np.isposinf(got[0, 0]) and np.isnan(got[0, 1]) and np.isnan(got[0, 2])      # 3*(1 + inf) - inf: inf - inf


def test_ulp_distance_on_hand_values():
    one = np.float32(1.0)
    nxt = np.nextafter(one, np.float32(2.0))
    tiny = np.float32(1e-45)                                            # the smallest subnormal
    a = np.array([one, one, np.float32(0.0), -tiny, np.float32(-1.0)], np.float32)
    b = np.array([one, nxt, np.float32(-0.0), tiny, np.nextafter(np.float32(-1.0), np.float32(-2.0))], np.float32)
    assert cc.ulp_distance(a, b).tolist() == [0, 1, 0, 2, 1]


def test_rescale_restatement_on_hand_values():
    ec = np.array([[3.0, 1.0], [3.0, 1.0], [2.0, 2.0]], np.float32)          # std 1, 1, 0
    out = np.array([[5.0, 1.0], [4.0, 4.0], [1.0, 3.0]], np.float32)         # std 2, 0, 1
    assert cc.rescale_factor_restated(ec, out, 0.5).tolist() == [0.75, 1.0, 0.5]          # 0.5*1/2 + 0.5 ; constant: unscaled ; 0.5*0 + 0.5
    assert cc.rescale_factor_restated(ec, out, 1.0).tolist() == [0.5, 1.0, 0.0]
    assert cc.rescale_factor_restated(ec, out, 0.0).tolist() == [1.0, 1.0, 1.0]
    bad = out.copy()
    bad[0, 0] = np.nan
    assert cc.rescale_factor_restated(ec, bad, 0.5).tolist() == [1.0, 1.0, 0.5]           # a non-finite statistic: unscaled
    assert cc.rescale_factor_restated(ec, out, 0.5, np.float32).dtype == np.float32
    assert cc.rescale_bar(ec, out, 0.5) == 0.0                                              # exact in both formats


def test_recorded_rescale_bars_cover_the_cases():
    gold = np.load(os.path.join(GOLD, "cfg.npz"))
    for B in cc.BATCHES:
        for n in cc.SIZES + cc.SIZES_UNALIGNED:
            ec, eu, w = cc.combine_inputs(B, n)
            assert ec.shape == eu.shape == (B, n) and set(w.tolist()) <= set(cc.W_VALUES)
            for phi in cc.PHIS:
                bar = float(gold[f"rescale/{cc.case_id(B, n)}/phi{phi}/bar"])
                assert 0.0 <= bar < 4e-6                  # a few float32 roundings, times the margin: never a loose bar
                assert (bar == 0.0) == (n == 1)           # one value has no spread: the factor is exactly 1 in both formats
    ws = set()
    for B in cc.BATCHES:
        for n in cc.SIZES:
            ws |= set(cc.combine_inputs(B, n)[2].tolist())
    assert ws == set(cc.W_VALUES)                         # every guidance scale of the list is met by the cases


# ---- dataset -----------------------------------------------------------------------------------------------------------------
def _write_grids(tmp_path, n=4, r=8):
    g = torch.Generator().manual_seed(5)
    paths = []
    for i in range(n):
        p = str(tmp_path / f"grid_{i}.npy")
        np.save(p, torch.randn((4, r, r, r), generator=g).numpy())
        paths.append(p)
    meta = str(tmp_path / "meta.json")
    with open(meta, "w") as f:
        json.dump(paths, f)
    return paths, meta


def test_dataset_with_and_without_class_meta(tmp_path):
    from meshdiffusion_amd.lib.dataset.shapenet_dmtet_dataset import ShapeNetDMTetDataset
    paths, meta = _write_grids(tmp_path)
    mask = torch.ones(1, 1, 8, 8, 8)
    plain = ShapeNetDMTetDataset(meta, mask, extension="npy")
    items = [plain[i] for i in range(len(plain))]
    for p, item in zip(paths, items):                      # today's item: the grid with the sign of its first depth slab
        want = torch.from_numpy(np.load(p)).clone()
        sign = torch.sign(want[:, :1])
        sign[sign == 0] = 1.0
        want[:, :1] = sign
        assert torch.is_tensor(item) and torch.equal(item, want)
    classes = {p: c for p, c in zip(paths, (2, 0, 1, 2))}
    cm = str(tmp_path / "classes.json")
    with open(cm, "w") as f:
        json.dump(dict(classes, **{"some/other/grid_99.npy": 7}), f)          # entries of grids that are not listed do not matter
    labelled = ShapeNetDMTetDataset(meta, mask, extension="npy", class_meta_path=cm)
    assert len(labelled) == len(plain) and labelled.labels == [2, 0, 1, 2]
    for i, item in enumerate(items):
        grid, y = labelled[i]
        assert torch.equal(grid, item) and y.dtype == torch.int64 and y.dim() == 0 and int(y) == classes[paths[i]]
    xb, yb = next(iter(torch.utils.data.DataLoader(labelled, batch_size=4)))             # the default collate: (grids [B,...], y [B])
    assert tuple(xb.shape) == (4, 4, 8, 8, 8) and yb.tolist() == [2, 0, 1, 2] and yb.dtype == torch.int64
    # the filter applies first: labels follow the filtered list
    filt = str(tmp_path / "keep.json")
    with open(filt, "w") as f:
        json.dump([1, 3], f)
    kept = ShapeNetDMTetDataset(meta, mask, extension="npy", filter_meta_path=filt, class_meta_path=cm)
    assert kept.labels == [0, 2]
    # a grid without a class, a class that is no id: refused at construction
    with open(cm, "w") as f:
        json.dump({p: 0 for p in paths[:-1]}, f)
    with pytest.raises(KeyError, match="grid_3"):
        ShapeNetDMTetDataset(meta, mask, extension="npy", class_meta_path=cm)
    with open(cm, "w") as f:
        json.dump({p: -1 for p in paths}, f)
    with pytest.raises(ValueError):
        ShapeNetDMTetDataset(meta, mask, extension="npy", class_meta_path=cm)


# ---- the training step's draws -----------------------------------------------------------------------------------------------
def test_draw_order_timesteps_noise_then_class_dropout():
    from meshdiffusion_amd.lib.diffusion import losses
    batch = torch.zeros(6, 4, 4, 4, 4)
    y = torch.tensor([0, 1, 2, 0, 1, 2])

    def before(seed):
        """the draws as they were before class conditioning: timesteps, then noise, nothing else"""
        torch.manual_seed(seed)
        labels = torch.randint(0, 1000, (batch.shape[0],), device=batch.device)
        noise = torch.randn_like(batch)
        return labels, noise, torch.rand(3)                # and what the generator gives next

    for seed in (0, 11):
        l0, n0, next0 = before(seed)
        # no class ids: class_dropout, whatever its value, draws nothing -- the stream of a class-less run is what it was
        for p in (0.0, 0.1, 1.0):
            torch.manual_seed(seed)
            l1, n1, y1 = losses.draw_step_randoms(batch, 1000, None, p, None)
            assert y1 is None and torch.equal(l1, l0) and torch.equal(n1, n0) and torch.equal(torch.rand(3), next0)
        # class ids without dropout: nothing more drawn either
        torch.manual_seed(seed)
        l1, n1, y1 = losses.draw_step_randoms(batch, 1000, y, 0.0, 3)
        assert y1 is y and torch.equal(l1, l0) and torch.equal(n1, n0) and torch.equal(torch.rand(3), next0)
        # class ids with dropout: the same timesteps and noise, then one uniform per sample -- the restated order, on a generator
        torch.manual_seed(seed)
        l2, n2, y2 = losses.draw_step_randoms(batch, 1000, y, 0.5, 3)
        gen = torch.Generator().manual_seed(seed)
        lr, nr, yr = cc.draw_order_restated(tuple(batch.shape), 1000, 0.5, y, 3, gen)
        assert torch.equal(l2, l0) and torch.equal(n2, n0) and torch.equal(l2, lr) and torch.equal(n2, nr) and torch.equal(y2, yr)
        assert set(y2.tolist()) <= {0, 1, 2, 3} and torch.equal(y2[y2 != 3], y[y2 != 3])
        assert not torch.equal(torch.rand(3), next0)       # the generator moved on by the class draw
    torch.manual_seed(3)
    assert losses.draw_step_randoms(batch, 1000, y, 1.0, 3)[2].tolist() == [3] * 6          # p = 1: every id is the null class
    with pytest.raises(ValueError):
        losses.get_ddpm_loss_fn(__import__("meshdiffusion_amd.lib.diffusion.sde_lib", fromlist=["VPSDE"]).VPSDE(0.1, 20.0, 1000), True,
                                class_dropout=1.5)


# ---- configuration and drivers -----------------------------------------------------------------------------------------------
def test_config_defaults_are_inert():
    from meshdiffusion_amd.config import get_config_res64, get_config_res128
    for cfg in (get_config_res64(), get_config_res128()):
        assert cfg.model.num_classes == 0 and cfg.data.class_meta_path is None and cfg.training.class_dropout == 0.1
        assert cfg.eval.class_id is None and cfg.eval.cfg_scale == 1.0 and cfg.eval.cfg_rescale == 0.0


def test_eval_class_id_is_sliced_with_the_batch_and_refused_without_classes():
    from meshdiffusion_amd.config import get_config_res64
    from meshdiffusion_amd.lib.diffusion import evaler, parallel
    cfg = get_config_res64()
    assert evaler.class_ids_of(cfg, 5) is None
    cfg.eval.class_id = 2
    assert evaler.class_ids_of(cfg, 5) == [2] * 5 and evaler.class_ids_of(cfg, 5, 3, 2) == [2, 2]
    cfg.eval.class_id = [0, 1, 2, 3, 4]
    sizes = parallel.shard_sizes(5, 2)                      # ranks 0 and 1 of a sharded run take 3 and 2 samples
    got = [evaler.class_ids_of(cfg, 5, sum(sizes[:r]), sizes[r]) for r in range(2)]
    assert got == [[0, 1, 2], [3, 4]]
    for bad in ([0, 1], "chair", [0, 1, 2, 3, 4.5], True):
        cfg.eval.class_id = bad
        with pytest.raises(ValueError, match="eval.class_id"):
            evaler.class_ids_of(cfg, 5)
    cfg.eval.class_id = 1                                   # a class-less model: refused with the way out, before a checkpoint is read
    with pytest.raises(ValueError, match="model.num_classes"):
        evaler.check_class_config(cfg)
    with pytest.raises(ValueError, match="model.num_classes"):
        evaler.uncond_gen(cfg)
    cfg.model.num_classes = 3
    evaler.check_class_config(cfg)
    cfg.eval.guidance_scale = 1.0                           # the out-of-scope list: refused before any file is read
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        evaler.cond_gen(cfg)
    with pytest.raises(NotImplementedError, match="likelihood"):
        evaler.likelihood(cfg)


def test_classifier_free_model_checks_its_arguments():
    from meshdiffusion_amd.lib.diffusion import sampling
    _, m = _small(3)
    _, m0 = _small(0)
    with pytest.raises(ValueError, match="no classes"):
        sampling.ClassifierFreeModel(m0, [0, 1])
    for kw in (dict(y=[0, 4]), dict(y=[0, -1]), dict(y=[]), dict(y=[0, 1], scale=[1.0, 2.0, 3.0]), dict(y=[0, 1], scale=float("nan")),
               dict(y=[0, 1], rescale=1.5), dict(y=[0, 1], rescale=-0.1)):
        with pytest.raises(ValueError):
            sampling.ClassifierFreeModel(m, **kw)
    assert [sampling.ClassifierFreeModel(m, [0, 3], scale=s).mode for s in (1.0, 0.0, 3.0, [1.0, 1.0], [1.0, 2.0])] == \
        ["cond", "null", "both", "cond", "both"]
    w = sampling.ClassifierFreeModel(m, [0, 3], scale=3.0, rescale=0.7)
    ids, wt = w._operands("cpu")
    assert ids.tolist() == [0, 3, 3, 3] and wt.tolist() == [3.0, 3.0] and w.B == 2
    assert list(w.state_dict().keys()) == ["model." + k for k in m.state_dict().keys()]
    with pytest.raises(ValueError, match="2 class ids"):
        w(torch.zeros(3, 4, 16, 16, 16), torch.zeros(3))
    # the refusals of the out-of-scope list that need no GPU
    from meshdiffusion_amd.lib.diffusion import likelihood, sde_lib
    sde = sde_lib.VPSDE(0.1, 20.0, 1000)
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        sampling._check_guidance(1.0, torch.zeros(1), model=w)
    assert sampling._check_guidance(0.0, None, model=w) is False
    fn = likelihood.get_likelihood_fn(sde, lambda x: x)
    with pytest.raises(NotImplementedError, match="likelihood"):
        fn(w, torch.zeros(2, 4, 16, 16, 16))
    shape = (2, 4, 16, 16, 16)
    ddim = sampling.get_ddim_sampler(sde, shape, sampling.get_predictor("ddim"), lambda x: x, device="cpu")
    ode = sampling.get_ode_sampler(sde, shape, lambda x: x, device="cpu")
    for fn in (ddim, ode):
        with pytest.raises(NotImplementedError, match="encode=True"):
            fn(w, x0=torch.zeros(shape), encode=True)
