"""CLI drop-in for the reference's main_diffusion.py:13-25 without absl/ml_collections:

    python main_diffusion.py --config=configs/res64.py --mode=uncond_gen \\
        --config.eval.eval_dir=out --config.eval.ckpt_path=ckpt.pth [--config.eval.batch_size=8]

`--config` may be a reference-style python config file (get_config()) or one of the built-in
names `res64` / `res128`.  `--mode=train` runs one rank per GPU under torchrun.
`--mode=likelihood` writes {eval_dir}/likelihood.npz: bits/dim of the grids of `--config.data.meta_path` through the
probability-flow ODE (`--config.eval.ode_rtol=1e-5 --config.eval.ode_atol=1e-5 --config.eval.num_batches=N` optional).
`--mode=cond_gen --config.eval.guidance_scale=1.0 [--config.eval.guidance_replace=False]` adds reconstruction guidance to the
conditional samplers (`--config.sampling.method=ddim` is the form to run: 99 guided evaluations instead of 1000).
`--config.sampling.method=dpmpp [--config.sampling.dpmpp_steps=20 --config.sampling.dpmpp_order=2 --config.sampling.dpmpp_tau=0]`
samples with DPM-Solver++ in 20 evaluations, in uncond_gen and cond_gen (with or without guidance), under torchrun as well.
`--mode=interp --config.sampling.method=ddim|dpmpp|ode [--config.eval.interp_points=K --config.eval.interp_pairs=Np]` writes
{eval_dir}/interp.npy: K shapes per pair on the walk between two latents; `--config.eval.interp_sources=grids.npy` walks between
given grids instead of prior draws, encoded by DDIM (method ddim) or ODE (method ode) inversion.
`--config.model.num_classes=K --config.data.class_meta_path=classes.json [--config.training.class_dropout=0.1]` trains one
class-conditional model; `--config.eval.class_id=C [--config.eval.cfg_scale=3.0 --config.eval.cfg_rescale=0.7]` then steers
uncond_gen, cond_gen and interp with classifier-free guidance under every sampler (not with guidance_scale > 0, likelihood or
interp_sources).
"""
import sys

from meshdiffusion_amd import config as mdconfig


def parse(argv):
    cfg_path, mode, rest = None, None, []
    i = 0
    while i < len(argv):
        a = argv[i]
        for key in ("--config", "--mode"):
            if a == key or a.startswith(key + "="):
                val = a.split("=", 1)[1] if "=" in a else argv[i + 1]
                i += 0 if "=" in a else 1
                if key == "--config":
                    cfg_path = val
                else:
                    mode = val
                break
        else:
            rest.append(a)
        i += 1
    if cfg_path is None or mode is None:
        raise SystemExit("flags --config and --mode are required")
    if mode not in ("train", "uncond_gen", "cond_gen", "likelihood", "interp"):
        raise SystemExit(f"--mode must be one of train|uncond_gen|cond_gen|likelihood|interp, got {mode}")
    if cfg_path in ("res64", "res128"):
        config = getattr(mdconfig, f"get_config_{cfg_path}")()
    else:
        config = mdconfig.load_config_file(cfg_path)
    left = mdconfig.apply_overrides(config, rest)
    if left:
        raise SystemExit(f"unknown flags: {left}")
    return config, mode


def main(argv=None):
    config, mode = parse(sys.argv[1:] if argv is None else argv)
    from meshdiffusion_amd.lib.diffusion import evaler
    if mode == "uncond_gen":
        evaler.uncond_gen(config)
    elif mode == "cond_gen":
        evaler.cond_gen(config)
    elif mode == "likelihood":
        evaler.likelihood(config)
    elif mode == "interp":
        try:
            evaler.interp(config)
        except (ValueError, NotImplementedError) as e:      # a run this mode refuses: the message names what it takes
            raise SystemExit(f"--mode=interp: {e}") from e
    else:
        from meshdiffusion_amd.lib.diffusion import trainer
        trainer.train(config)


if __name__ == "__main__":
    main()
