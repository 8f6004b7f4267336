"""Generation drivers -- mirror of the reference's lib/diffusion/evaler.py
(`uncond_gen` :14-60, `cond_gen` :134-211).  Same behaviour and file outputs
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
    if getattr(config.eval, "calibrate", True) and torch.device(config.device).type == "cuda":
        rep = mutils.calibrate_model(score_model, config, batch=shape[0])      # at the sampling batch: which convs take the Winograd path depends on it
        if rep is not None:
            print(f"calibrated the {score_model.module.hip_precision} convs: {rep['measured']} measured, worst kept {rep['worst']:.2e}, "
                  f"demoted to bf16x3: {rep['demoted']}")
    return score_model, sampling_fn, eval_dir


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

    def shard(local_batch, seed):
        if world > 1:
            torch.manual_seed(seed)                     # CPU generator (prior) and this rank's device generator (per-step noise)
        model, sampling_fn, _ = _setup(config, mask_shape, local_batch=local_batch)
        return run(model, sampling_fn)

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


def tet_vertices_to_grid_index(vertices):
    """Map tet-grid vertex positions to integer cubic-grid coordinates (evaler.py:187-195)."""
    uniq = vertices[:].unique()
    dx = uniq[1] - uniq[0]
    return torch.round((vertices - vertices.min()) / dx).long()


def cond_gen(config, save_fname="0"):
    """Conditional generation from a partial DMTet (2.5D view) scattered into the cubic grid."""
    R = config.data.image_size
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
    scale = float(getattr(config.eval, "guidance_scale", 0.0) or 0.0)
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
