"""Generation drivers -- mirror of the reference's lib/diffusion/evaler.py
(`uncond_gen` :14-60, `cond_gen` :134-211, `slerp` + `uncond_gen_interp` :63-131 repaired as `interp`).  Same behaviour and file outputs
(`{eval_dir}/{idx}.npy`, float32 [B,4,R,R,R]); the grid mask is read from
`./data/grid_mask_{R}.pt` relative to the cwd like the reference, with `map_location` so that the
CUDA-saved tensor loads on any host.

Multi-GPU (replaces the reference's `torch.nn.DataParallel` inside `create_model`, models/utils.py:88-96, that
evaler.py:29 relies on): under `torchrun --nproc-per-node N main_diffusion.py --mode=uncond_gen|cond_gen` every rank
builds a static replica on `cuda:LOCAL_RANK`, samples its shard of `config.eval.batch_size` (parallel.shard_sizes) with
the global RNG seeded `config.seed + rank`, and rank 0 gathers the shards (the only collective: 4.2 MB per sample) and
writes ONE `{idx}.npy` holding the full batch in rank order.  Parity under sharding is per shard: rank r's
rows equal a single-process run with batch `sizes[r]` after `torch.manual_seed(config.seed + r)`; the reference
itself draws a whole batch from one unseeded generator, so no stronger statement exists.  A single process behaves
exactly as before (no seeding, the caller's RNG state decides the draw).
"""
import os

import numpy as np
import torch

from . import losses, parallel, sampling, sde_lib
from .models import ddpm_res64, ddpm_res128  # noqa: F401  (registers the models, like trainer.py:7 in the reference)
from .models import utils as mutils
from .models.ema import ExponentialMovingAverage
from .utils import restore_checkpoint


def _load_model(config):
    """The score model of `config.eval.ckpt_path` with its EMA weights, and the SDE."""
    ckpt_path = config.eval.ckpt_path
    os.makedirs(config.eval.eval_dir, exist_ok=True)
    score_model = mutils.create_model(config)
    optimizer = losses.get_optimizer(config, score_model.parameters())
    ema = ExponentialMovingAverage(score_model.parameters(), decay=config.model.ema_rate)
    state = dict(optimizer=optimizer, model=score_model, ema=ema, step=0)
    sde = sde_lib.VPSDE(beta_min=config.model.beta_min, beta_max=config.model.beta_max,
                        N=config.model.num_scales, device=config.device)
    assert os.path.exists(ckpt_path), ckpt_path
    print("ckpt path:", ckpt_path)
    state = restore_checkpoint(ckpt_path, state, device=config.device)
    ema.copy_to(score_model.parameters())
    print(f"loaded model is trained till iter {state['step'] // config.training.iter_size}")
    return score_model, sde


def class_ids_of(config, total, start=0, count=None):
    """config.eval.class_id as the class ids of samples start .. start+count-1 of a batch of `total`: an int (every sample) or a
    list of length `total`, sliced together with the batch when it is sharded over ranks.  None when the field is unset."""
    cid = getattr(config.eval, "class_id", None)
    if cid is None:
        return None
    count = total - start if count is None else count
    if isinstance(cid, (int, np.integer)) and not isinstance(cid, bool):
        return [int(cid)] * count
    if not isinstance(cid, (list, tuple)) or len(cid) != total or not all(isinstance(c, (int, np.integer)) for c in cid):
        raise ValueError(f"eval.class_id must be an int or a list of {total} ints (one per sample of the batch), got {cid!r}")
    return [int(c) for c in cid[start:start + count]]


def check_class_config(config):
    """eval.class_id with a class-less model is refused with the way out, before a checkpoint is read."""
    if getattr(config.eval, "class_id", None) is not None and int(getattr(config.model, "num_classes", 0) or 0) <= 0:
        raise ValueError("eval.class_id is set, but the model has no classes (model.num_classes = 0): train a class-conditional "
                         "model (model.num_classes > 0 with data.class_meta_path), or drop eval.class_id")


def with_classes(config, score_model, ids):
    """The model the samplers are given: `score_model` itself without eval.class_id (a class-conditional model then runs under its
    null class), else sampling.ClassifierFreeModel over it with eval.cfg_scale (default 1.0) and eval.cfg_rescale (default 0.0)."""
    if ids is None:
        return score_model
    check_class_config(config)
    return sampling.ClassifierFreeModel(score_model, ids, scale=getattr(config.eval, "cfg_scale", 1.0),
                                        rescale=getattr(config.eval, "cfg_rescale", 0.0))


def _grid_mask(config, shape):
    R = config.data.image_size
    mask_path = getattr(config.eval, "grid_mask_path", None) or f"./data/grid_mask_{R}.pt"
    return torch.load(mask_path, map_location=config.device).view(*shape).to(config.device)


def _setup(config, mask_shape, local_batch=None):
    eval_dir = config.eval.eval_dir
    score_model, sde = _load_model(config)
    R = config.data.image_size
    grid_mask = _grid_mask(config, mask_shape(R))
    shape = (config.eval.batch_size if local_batch is None else local_batch, config.data.num_channels, R, R, R)
    sampling_fn = sampling.get_sampling_fn(config, sde, shape, lambda x: x, 1e-3, grid_mask=grid_mask)
    # the checkpoint's weights meet the reduced-precision conv formats here for the first time: measure every conv's operand on a
    # few noise batches, rebuild the equalisers from the measurement, audit each conv against its bf16x3 form and demote the ones
    # above the bar (models/utils.calibrate_model; config.eval.calibrate = False skips it)
    _calibrate(score_model, config, shape[0])
    return score_model, sampling_fn, eval_dir


def _calibrate(score_model, config, batch):
    if getattr(config.eval, "calibrate", True) and torch.device(config.device).type == "cuda":
        rep = mutils.calibrate_model(score_model, config, batch=batch)      # at the sampling batch: which convs take the Winograd path depends on it
        if rep is not None:
            print(f"calibrated the {score_model.module.hip_precision} convs: {rep['measured']} measured, worst kept {rep['worst']:.2e}, "
                  f"demoted to bf16x3: {rep['demoted']}")


def _ranks(config):
    """(rank, world) of this process; under torchrun (WORLD_SIZE > 1) joins the process group and moves the run to this
    rank's GPU."""
    rank, world, local_rank = parallel.init_distributed()
    if world > 1 and torch.device(config.device).type == "cuda":
        torch.cuda.set_device(local_rank)
        config.device = torch.device("cuda", local_rank)
    return rank, world


def _generate(config, mask_shape, fname, run):
    """Shard `config.eval.batch_size` over the ranks, run `run(model, sampling_fn) -> samples` on each shard, gather to
    rank 0 and write `{eval_dir}/{fname}.npy` once.  Returns the full batch on rank 0 (None elsewhere)."""
    rank, world = _ranks(config)
    total = int(config.eval.batch_size)

    start = sum(parallel.shard_sizes(total, world)[:rank])
    check_class_config(config)
    class_ids_of(config, total)                         # a malformed eval.class_id: refused before the checkpoint is read

    def shard(local_batch, seed):
        if world > 1:
            torch.manual_seed(seed)                     # CPU generator (prior) and this rank's device generator (per-step noise)
        model, sampling_fn, _ = _setup(config, mask_shape, local_batch=local_batch)
        return run(with_classes(config, model, class_ids_of(config, total, start, local_batch)), sampling_fn)

    with torch.no_grad():
        samples = parallel.sharded_sample(shard, total, int(getattr(config, "seed", 0)))
    if rank == 0:
        os.makedirs(config.eval.eval_dir, exist_ok=True)
        np.save(os.path.join(config.eval.eval_dir, f"{fname}.npy"), samples.cpu().numpy())
    if world > 1:
        parallel.barrier()                              # nobody leaves (and tears the group down) before the file exists
    ops_release()
    return samples


def ops_release():
    from ... import hip_ops as ops
    ops.release_scratch()                               # the Winograd operand buffer (GBs at 64^3) is not needed after a run


def uncond_gen(config, idx=0):
    """Unconditional generation: N-1 ancestral steps from the masked prior, saves {idx}.npy."""
    return _generate(config, lambda R: (1, R, R, R), idx, lambda model, sampling_fn: sampling_fn(model)[0])


def interp_plan(config, source_rows=None, fields=True):
    """What an interpolation run of `config` does, decided before any GPU work: (pairs Np, points per pair K, sampling method,
    encoded).  Reads config.eval.interp_sources / interp_pairs / interp_points, all optional; source_rows: the rows of the
    interp_sources file (needed when the field is set); fields off: the three fields are not read.  Raises ValueError on a count
    out of range and NotImplementedError on a sampler that cannot run it."""
    from ..._lib import SLERP_MAX_K
    ev = config.eval if fields else {}
    method = str(getattr(config.sampling, "method", "pc")).lower()
    encoded = bool(getattr(ev, "interp_sources", None))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("interp runs in a single process: sharding pairs over ranks is not implemented")
    if encoded:
        if method not in ("ddim", "ode"):
            raise NotImplementedError(f"interp_sources are encoded by the inverse of the configured sampler: sampling.method must be "
                                      f"'ddim' (DDIM inversion) or 'ode' (ODE inversion), got {method!r}")
        if source_rows is None or source_rows < 2 or source_rows % 2:
            raise ValueError(f"interp_sources must hold 2*Np grids (rows 2p and 2p+1 form pair p), got {source_rows} rows")
    elif method == "dpmpp" and int(getattr(config.sampling, "dpmpp_tau", 0)) != 0:
        raise NotImplementedError("interp needs a deterministic sampler: 'dpmpp' runs it with sampling.dpmpp_tau = 0 only")
    elif method not in ("ddim", "dpmpp", "ode"):
        raise NotImplementedError(f"interp needs a sampler that starts from a given latent (x0=): sampling.method 'ddim', 'dpmpp' "
                                  f"with dpmpp_tau = 0, or 'ode', got {method!r}")
    pairs = getattr(ev, "interp_pairs", None)
    pairs = int(pairs) if pairs is not None else (source_rows // 2 if encoded else 1)
    if pairs < 1 or (encoded and 2 * pairs > source_rows):
        raise ValueError(f"interp_pairs = {pairs}: at least 1" + (f", and interp_sources holds {source_rows // 2} pairs" if encoded else ""))
    points = getattr(ev, "interp_points", None)
    points = int(points) if points is not None else int(config.eval.batch_size) // pairs
    if not 2 <= points <= SLERP_MAX_K:
        raise ValueError(f"interp_points = {points}: between 2 (both ends) and {SLERP_MAX_K} per pair")
    return pairs, points, method, encoded


def _interp(config, fname, plan, sources=None):
    from ... import hip_ops as ops
    pairs, K, method, encoded = plan
    dev, R, C = config.device, config.data.image_size, config.data.num_channels
    check_class_config(config)
    if encoded and class_ids_of(config, K) is not None:
        raise NotImplementedError("interp_sources (encode=True inversions) under classifier-free guidance is not implemented: "
                                  "drop eval.class_id or the sources")
    with torch.no_grad():
        score_model, sde = _load_model(config)
        grid_mask = _grid_mask(config, (1, R, R, R))
        fn_for = lambda batch: sampling.get_sampling_fn(config, sde, (batch, C, R, R, R), lambda x: x, 1e-3, grid_mask=grid_mask)   # noqa: E731
        decode = fn_for(K)
        _calibrate(score_model, config, K)
        score_model = with_classes(config, score_model, class_ids_of(config, K))   # eval.class_id: an int, or one id per point of a walk
        if encoded:
            encode = fn_for(2)
            ends = torch.cat([encode(score_model, x0=sources[2 * p:2 * p + 2].to(dev), encode=True)[0].float() for p in range(pairs)])
        else:
            ends = sde.prior_sampling((2 * pairs, C, R, R, R)).to(dev)
        alpha = np.arange(K, dtype=np.float64) / float(K - 1)                    # evaler.py:127
        mix, theta = ops.slerp(ends[0::2], ends[1::2], torch.from_numpy(alpha), grid_mask.reshape(-1).float().contiguous())
        samples = torch.cat([decode(score_model, x0=mix[p])[0].float().cpu() for p in range(pairs)])
    os.makedirs(config.eval.eval_dir, exist_ok=True)
    np.save(os.path.join(config.eval.eval_dir, f"{fname}.npy"), samples.numpy())
    np.savez(os.path.join(config.eval.eval_dir, f"{fname}_meta.npz"), theta=theta.cpu().numpy(), alpha=alpha, method=method,
             encoded=encoded)
    ops_release()
    return samples


def interp(config, save_fname="interp"):
    """Walks between pairs of shapes (`--mode=interp`; the reference's `slerp` + `uncond_gen_interp`, evaler.py:63-131, which reads
    undefined names and cannot run): K latents on the great circle between the two endpoints of every pair (hip_ops.slerp), each
    decoded by the configured deterministic sampler.  Optional config.eval fields:
        interp_sources  unset: the endpoints are prior draws on the grid mask.  Set: a .npy [2*Np, C, R, R, R] of data grids; rows
                        2p, 2p+1 form pair p and are encoded first, by the inverse of the configured sampler (sampling.method
                        'ddim': DDIM inversion, first order; 'ode': ODE inversion, to the solver's tolerance)
        interp_pairs    Np (default 1; with sources: rows / 2)
        interp_points   K per pair, both ends included (default eval.batch_size // Np); alpha_k = k/(K-1)
    The checkpoint is loaded once and calibrated once at batch K; encoding runs at batch 2, decoding pair by pair at batch K.
    Writes {eval_dir}/{save_fname}.npy, float32 [Np*K, C, R, R, R] pair-major (mesh_export input as it stands), and
    {save_fname}_meta.npz: theta [Np], alpha [K], method, encoded.  Single process."""
    path = getattr(config.eval, "interp_sources", None)
    sources = torch.from_numpy(np.load(path)).float() if path else None
    if sources is not None:
        R, C = config.data.image_size, config.data.num_channels
        if sources.dim() != 5 or tuple(sources.shape[1:]) != (C, R, R, R):
            raise ValueError(f"interp_sources must be [2*Np, {C}, {R}, {R}, {R}], got {tuple(sources.shape)}")
    return _interp(config, save_fname, interp_plan(config, None if sources is None else sources.shape[0]), sources)


def uncond_gen_interp(config, idx=0):
    """The reference's entry point (evaler.py:73-131) as it was meant: one pair of prior draws, K = config.eval.batch_size points,
    whatever the interp_* fields say; saves {idx}.npy (and {idx}_meta.npz)."""
    return _interp(config, idx, interp_plan(config, fields=False))


def tet_vertices_to_grid_index(vertices):
    """Map tet-grid vertex positions to integer cubic-grid coordinates (evaler.py:187-195)."""
    uniq = vertices[:].unique()
    dx = uniq[1] - uniq[0]
    return torch.round((vertices - vertices.min()) / dx).long()


def cond_gen(config, save_fname="0"):
    """Conditional generation from a partial DMTet (2.5D view) scattered into the cubic grid."""
    R = config.data.image_size
    scale = float(getattr(config.eval, "guidance_scale", 0.0) or 0.0)
    if scale > 0 and getattr(config.eval, "class_id", None) is not None:
        raise NotImplementedError("eval.class_id (classifier-free guidance) together with eval.guidance_scale > 0 is not implemented: "
                                  "reconstruction guidance needs the Jacobian of the combined output")
    partial = torch.load(config.eval.partial_dmtet_path, map_location="cpu", weights_only=False)
    tet = np.load(config.eval.tet_path)
    idx = tet_vertices_to_grid_index(torch.tensor(tet["vertices"]))
    sdf_grid = torch.zeros((1, 1, R, R, R))
    sdf_grid[0, 0, idx[:, 0], idx[:, 1], idx[:, 2]] = partial["sdf"].cpu().float()
    vis_grid = torch.zeros((1, 1, R, R, R))
    vis_grid[0, 0, idx[:, 0], idx[:, 1], idx[:, 2]] = partial["vis"].cpu().float()

    # reconstruction guidance (sampling.guidance_terms): optional config.eval fields guidance_scale (unset or 0: none, the call
    # below is the unguided one), guidance_replace (True: the replacement of the known voxels stays), guidance_chunk (samples per
    # taped forward).  The load-time calibration still runs; the taped forward of a guided step is bf16x3 and does not read it.
    method = str(getattr(getattr(config, "sampling", None), "method", "pc")).lower()
    kw = {} if method == "dpmpp" else dict(freeze_iters=config.eval.freeze_iters)      # DPM-Solver++ has its own time grid
    if scale > 0:
        if method == "ddim":
            kw = {}                                     # the DDIM sampler visits its own sub-sequence: no freeze_iters
        kw.update(guidance_scale=scale, guidance_replace=bool(getattr(config.eval, "guidance_replace", True)),
                  guidance_chunk=getattr(config.eval, "guidance_chunk", None))

    def run(model, sampling_fn):
        return sampling_fn(model, partial=sdf_grid.to(config.device), partial_mask=vis_grid.to(config.device), **kw)[0]

    return _generate(config, lambda R: (1, 1, R, R, R), save_fname, run)


def likelihood(config):
    """Held-out log-likelihood of the grids of `config.data.meta_path` through the probability-flow ODE
    (likelihood.get_likelihood_fn on the grid mask; the reference ships the function, lib/diffusion/likelihood.py, but no driver
    that reaches it).  Restores the checkpoint, applies the EMA, no calibration: every evaluation is the bf16x3 taped forward and
    the data-gradient-only backward.  `config.eval.batch_size` grids per batch, read as the trainer reads them but without
    augmentation; optional config.eval fields: ode_rtol / ode_atol (1e-5), ode_eps (1e-5), num_batches (all), hutchinson
    ('Rademacher').  Writes {eval_dir}/likelihood.npz: bpd, logp, delta_logp (nats), nfe per batch, the dataset indices.
    Single process."""
    from ..dataset.shapenet_dmtet_dataset import ShapeNetDMTetDataset
    from . import likelihood as lk
    ev = config.eval
    if getattr(ev, "class_id", None) is not None:
        raise NotImplementedError("--mode=likelihood under classifier-free guidance (eval.class_id) is not implemented: the "
                                  "divergence needs the Jacobian of the combined output")
    R = config.data.image_size
    score_model, sde = _load_model(config)
    score_model.eval()
    mask = _grid_mask(config, (1, 1, R, R, R))
    dataset = ShapeNetDMTetDataset(config.data.meta_path, deform_scale=config.model.deform_scale, aug=False, grid_mask=mask,
                                   filter_meta_path=config.data.filter_meta_path, normalize_sdf=config.data.normalize_sdf,
                                   extension=config.data.extension)
    gen = torch.Generator(device=config.device).manual_seed(int(getattr(config, "seed", 0)))
    fn = lk.get_likelihood_fn(sde, lambda x: x, hutchinson_type=getattr(ev, "hutchinson", "Rademacher"),
                              rtol=float(getattr(ev, "ode_rtol", 1e-5)), atol=float(getattr(ev, "ode_atol", 1e-5)),
                              eps=float(getattr(ev, "ode_eps", 1e-5)), grid_mask=mask, generator=gen)
    B, n = int(ev.batch_size), len(dataset)
    starts = list(range(0, n, B))
    if getattr(ev, "num_batches", None):
        starts = starts[:int(ev.num_batches)]
    out = dict(bpd=[], logp=[], delta_logp=[], nfe=[], index=[])
    for s in starts:
        idx = list(range(s, min(s + B, n)))
        batch = (torch.stack([dataset[i] for i in idx]).float().to(config.device) * mask).contiguous()
        bpd, _, nfe, delta_logp, prior_logp = fn(score_model, batch, return_parts=True)
        out["bpd"].append(bpd.cpu().numpy())
        out["logp"].append((prior_logp + delta_logp).cpu().numpy())
        out["delta_logp"].append(delta_logp.cpu().numpy())
        out["nfe"].append(nfe)
        out["index"].append(np.array(idx, dtype=np.int64))
        print(f"grids {idx[0]}..{idx[-1]}: bits/dim {out['bpd'][-1]}, nfe {nfe}")
    res = {k: (np.array(v, dtype=np.int64) if k == "nfe" else np.concatenate(v)) for k, v in out.items()}
    np.savez(os.path.join(ev.eval_dir, "likelihood.npz"), **res)
    ops_release()
    return res
