"""Predictor-corrector and DDIM samplers with grid-mask and partial-grid inpainting.

Host-side mirror of the reference's lib/diffusion/sampling.py: `get_sampling_fn` :83-117, predictors
`EulerMaruyamaPredictor` :185-196, `ReverseDiffusionPredictor` :199-210, `AncestralSamplingPredictor` :213-237,
correctors `LangevinCorrector` :259-286, `AnnealedLangevinDynamics` :289-321, `NoneCorrector` :324-332,
`get_pc_sampler`/`pc_sampler` :357-487 (unconditional loop :471-481, inpainting :429-467), `DDIMPredictor` :249-257,
`get_ddim_sampler`/`ddim_sampler` :500-570 (with sde_lib.py:113-140 `discretize_ddim`).

Same call surface:
    fn = get_sampling_fn(config, sde, shape, inverse_scaler, eps, grid_mask=None)
    samples, nfe = fn(model, partial=None, partial_mask=None, partial_channel=0, freeze_iters=None)
The per-step arithmetic (score scaling, x_mean, re-noising, masking) is ONE HIP kernel per predictor step
(md_ancestral_step, md_sde_step) and two per corrector step (md_langevin_norms + md_langevin_step); the noise still comes from torch's global generator (CPU generator for the
prior, device generator per step) so that, on the same device and seed, the stream of random
numbers is the reference's.  Two optional keyword extensions used by tests/bench:
    n_iters  -- run only the first n iterations of the N-step schedule
    noise_fn -- callable(x) -> z replacing torch.randn_like (to replay recorded noise)
Reconstruction guidance of the conditional samplers (not in the reference; `guidance_terms`): pc_sampler and ddim_sampler take
    guidance_scale, guidance_replace, guidance_chunk -- each step also descends zeta * grad_x ||pm (x0_hat[ch] - partial)||
"""
import numpy as np
import torch

from . import sde_lib
from .models import utils as mutils
from ... import hip_ops as ops

_PREDICTORS = {}
_CORRECTORS = {}


def _registrar(table):
    def register(cls=None, *, name=None):
        def _do(c):
            key = c.__name__ if name is None else name
            if key in table:
                raise ValueError(f"Already registered model with name: {key}")
            table[key] = c
            return c

        return _do if cls is None else _do(cls)

    return register


register_predictor = _registrar(_PREDICTORS)
register_corrector = _registrar(_CORRECTORS)


def get_predictor(name):
    return _PREDICTORS[name]


def get_corrector(name):
    return _CORRECTORS[name]


class Predictor:
    def __init__(self, sde, score_fn, probability_flow=False):
        self.sde, self.score_fn = sde, score_fn


class Corrector:
    def __init__(self, sde, score_fn, snr, n_steps):
        self.sde, self.score_fn, self.snr, self.n_steps = sde, score_fn, snr, n_steps


@register_predictor(name="ancestral_sampling")
class AncestralSamplingPredictor(Predictor):
    """x_mean = (x + beta*score)/sqrt(1-beta), x = x_mean + sqrt(beta)*z, score = -eps_hat/sigma."""

    def __init__(self, sde, score_fn, probability_flow=False):
        super().__init__(sde, score_fn, probability_flow)
        if not isinstance(sde, sde_lib.VPSDE):
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
        assert not probability_flow, "Probability flow not supported by ancestral sampling"

    def update_fn(self, x, t, model=None, noise=None, mask=None):
        """Stand-alone update (same semantics as the reference's vpsde_update_fn)."""
        sde = self.sde
        k = (t * (sde.N - 1) / sde.T).long()
        eps_hat = mutils.get_model_fn(model, train=False)(x, t * (sde.N - 1))
        beta = sde.discrete_betas.to(t.device)[k]
        sigma = sde.sqrt_1m_alphas_cumprod.to(t.device)[k]
        coef = torch.stack([beta, sigma, torch.sqrt(1.0 - beta), torch.sqrt(beta)], dim=1).contiguous()
        z = torch.randn_like(x) if noise is None else noise
        return ops.ancestral_step(x, eps_hat, z, mask, coef)


@register_predictor(name="reverse_diffusion")
class ReverseDiffusionPredictor(Predictor):
    """f = sqrt(alpha)*x - x, rev_f = f - G^2*score*h, x_mean = x - rev_f, x = x_mean + G'*z (VPSDE.discretize and the
    reverse SDE, sde_lib.py:106-111; h = 0.5 and G' = 0 under probability flow).  One md_sde_step launch."""
    kind = "reverse_diffusion"


@register_predictor(name="euler_maruyama")
class EulerMaruyamaPredictor(Predictor):
    """drift = -0.5*beta(t)*x - diffusion^2*score, x_mean = x + drift*dt, x = x_mean + diffusion*sqrt(-dt)*z with
    dt = -1/N (sampling.py:190-196, VPSDE.sde).  One md_sde_step launch."""
    kind = "euler_maruyama"


@register_predictor(name="ddim")
class DDIMPredictor(Predictor):
    """Deterministic DDIM update between two (not necessarily adjacent) time levels; state in float64 like the
    reference's `discretize_ddim` (sde_lib.py:113-140): one U-Net evaluation + one md_ddim_step launch."""

    def coefficients(self, t, tprev):
        """[B,4] float64 rows {a1, a2, a1_prev/a1, a2_prev/a2} for batch time vectors t, tprev (sde_lib.py:115-127)."""
        sde = self.sde
        k = (t * (sde.N - 1) / sde.T).long()
        kp = (tprev * (sde.N - 1) / sde.T).long()
        sa, s1 = sde.sqrt_alphas_cumprod.to(t.device), sde.sqrt_1m_alphas_cumprod.to(t.device)
        a1, a2 = sa[k].double(), s1[k].double()
        return torch.stack([a1, a2, sa[kp].double() / a1, s1[kp].double() / a2], dim=1).contiguous()

    def update_fn(self, x, t, tprev=None, model=None, mask=None, partial=None, pmask=None, ch=0):
        eps_hat = mutils.get_model_fn(model, train=False)(x.float(), t.float() * (self.sde.N - 1))
        xn, x0p, _ = ops.ddim_step(x.double(), eps_hat, mask, self.coefficients(t, tprev), partial, pmask, ch)
        return xn, x0p


@register_predictor(name="none")
class NonePredictor(Predictor):
    def update_fn(self, x, t, **_):
        return x, x


@register_corrector(name="langevin")
class LangevinCorrector(Corrector):
    """step = (snr * mean|z| / mean|score|)^2 * 2 * alpha over the batch, x_mean = x + step*score,
    x = x_mean + sqrt(2*step)*z (sampling.py:270-286).  md_langevin_norms + md_langevin_step per step."""
    mode = "langevin"


@register_corrector(name="ald")
class AnnealedLangevinDynamics(Corrector):
    """The same update with step = (snr*std(t))^2 * 2 * alpha, std of VPSDE.marginal_prob (sampling.py:300-321)."""
    mode = "ald"


@register_corrector(name="none")
class NoneCorrector(Corrector):
    def __init__(self, sde=None, score_fn=None, snr=None, n_steps=None):
        pass

    def update_fn(self, x, t, **_):
        return x, x


def get_sampling_fn(config, sde, shape, inverse_scaler, eps, grid_mask=None, return_traj=False):
    name = config.sampling.method.lower()
    if name == "ddim":
        return get_ddim_sampler(sde=sde, shape=shape, predictor=get_predictor("ddim"), inverse_scaler=inverse_scaler,
                                n_steps=config.sampling.n_steps_each, denoise=config.sampling.noise_removal, eps=eps,
                                device=config.device, grid_mask=grid_mask)
    if name == "ode":
        return get_ode_sampler(sde=sde, shape=shape, inverse_scaler=inverse_scaler, eps=eps, device=config.device,
                               rtol=float(getattr(config.sampling, "ode_rtol", 1e-5)),
                               atol=float(getattr(config.sampling, "ode_atol", 1e-5)), grid_mask=grid_mask)
    if name != "pc":
        raise ValueError(f"Sampler name {config.sampling.method} unknown.")
    return get_pc_sampler(sde=sde, shape=shape,
                          predictor=get_predictor(config.sampling.predictor.lower()),
                          corrector=get_corrector(config.sampling.corrector.lower()),
                          inverse_scaler=inverse_scaler, snr=config.sampling.snr,
                          n_steps=config.sampling.n_steps_each,
                          probability_flow=config.sampling.probability_flow,
                          continuous=config.training.continuous, denoise=config.sampling.noise_removal,
                          eps=eps, device=config.device, grid_mask=grid_mask, return_traj=return_traj)


class AncestralStepper:
    """Per-iteration state of the N-step ancestral loop: label / coefficient tables built once with the
    reference's float32 ops (sampling.py:406, :224-226; models/utils.py:193-195), then one U-Net call and
    one md_ancestral_step launch per iteration.  Used by pc_sampler and by bench.py."""

    def __init__(self, sde, shape, eps=1e-3, device="cuda", grid_mask=None):
        if not isinstance(sde, sde_lib.VPSDE):
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
        dev = torch.device(device)
        self.sde, self.shape, self.dev = sde, tuple(shape), dev
        self.B = shape[0]
        self.P = int(shape[2] * shape[3] * shape[4])
        self.timesteps = torch.linspace(sde.T, eps, sde.N, device=dev)
        labels_all = self.timesteps * (sde.N - 1)                      # fractional float labels
        k_all = (self.timesteps * (sde.N - 1) / sde.T).long()
        betas = sde.discrete_betas.to(dev)[k_all]
        sigmas = sde.sqrt_1m_alphas_cumprod.to(dev)[k_all]
        coef_all = torch.stack([betas, sigmas, torch.sqrt(1.0 - betas), torch.sqrt(betas)], dim=1)
        # per-iteration rows pre-expanded over the batch: no host-side tensor math inside the loop
        self.labels = labels_all[:, None].expand(sde.N, self.B).contiguous()
        self.coef = coef_all[:, None, :].expand(sde.N, self.B, 4).contiguous()
        self.gm, self.gm_flat = None, None
        if grid_mask is not None:
            self.gm = grid_mask.to(dev)
            self.gm_flat = self.gm.reshape(-1).to(torch.float32).contiguous()
            assert self.gm_flat.numel() == self.P, "grid_mask must broadcast over batch and channels"
            # a 0/1 mask makes the reference's pre-predictor `x * grid_mask` (sampling.py:476) an exact
            # no-op on the already masked state, so one masked store per step suffices
            assert bool(((self.gm_flat == 0) | (self.gm_flat == 1)).all()), "grid_mask must be binary"

    def prior(self):
        """Initial sample: CPU generator like the reference (sde_lib.py:216-217), then masked."""
        x = self.sde.prior_sampling(self.shape).to(self.dev)
        if self.gm is not None:
            x = x * self.gm
        return x.contiguous()

    def step(self, model_fn, x, i, draw=torch.randn_like):
        eps_hat = model_fn(x, self.labels[i])
        z = draw(x)
        return ops.ancestral_step(x, eps_hat, z, self.gm_flat, self.coef[i])


class GraphedStepper:
    """One denoise step (U-Net evaluation + ancestral update) captured in a hipGraph and replayed.

    ~700 kernel launches per step go through ctypes; at small batch (B=1: 23 ms/step) their host cost is a
    visible fraction of the step.  The graph is captured on a side stream with static input buffers
    (x, labels, coef, z); the per-step noise is still drawn eagerly by `torch.randn_like` (one tiny launch)
    so the random stream is exactly the eager sampler's.  Weight packing / caches are warmed by eager steps
    before capture.
    """

    def __init__(self, stepper, model_fn, warmup=2):
        self.st, self.model_fn = stepper, model_fn
        dev = stepper.dev
        self.x = torch.zeros(stepper.shape, dtype=torch.float32, device=dev)
        self.labels = torch.zeros(stepper.B, dtype=torch.float32, device=dev)
        self.coef = torch.zeros((stepper.B, 4), dtype=torch.float32, device=dev)
        self.z = torch.zeros(stepper.shape, dtype=torch.float32, device=dev)
        self.graph = None
        self._warm = warmup

    def _body(self):
        eps_hat = self.model_fn(self.x, self.labels)
        return ops.ancestral_step(self.x, eps_hat, self.z, self.st.gm_flat, self.coef)

    def step(self, x, i, draw=torch.randn_like):
        self.x.copy_(x)
        self.labels.copy_(self.st.labels[i])
        self.coef.copy_(self.st.coef[i])
        self.z.copy_(draw(x))
        if self.graph is None:
            if self._warm > 0:           # eager warm-up: packs weights, fills allocator pools
                self._warm -= 1
                return self._body()
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._body()             # one more eager pass on the capture stream
            torch.cuda.current_stream().wait_stream(side)
            with torch.cuda.graph(g):
                self.out = self._body()
            self.graph = g
        self.graph.replay()
        return self.out[0].clone(), self.out[1].clone()


def _pc_tables(sde, timesteps, B, predictor, corrector, snr, probability_flow):
    """Per-iteration coefficient rows of md_sde_step ([N,B,5]) and md_langevin_step ([N,B,3]), built once with the
    reference's float32 expressions (sampling.py:190-196, :270-321; sde_lib.py:93-111, :198-232; score scaling
    models/utils.py:191-198) and pre-expanded over the batch: no host-side tensor math inside the loop."""
    dev = timesteps.device
    k = (timesteps * (sde.N - 1) / sde.T).long()
    sigma = sde.sqrt_1m_alphas_cumprod.to(dev)[k]
    pcoef = ccoef = None
    if predictor is ReverseDiffusionPredictor:
        beta, alpha = sde.discrete_betas.to(dev)[k], sde.alphas.to(dev)[k]
        G = torch.sqrt(beta)
        rows = [sigma, torch.sqrt(alpha), G ** 2, torch.full_like(G, 0.5 if probability_flow else 1.0),
                torch.zeros_like(G) if probability_flow else G]
        pcoef = torch.stack(rows, dim=1)
    elif predictor is EulerMaruyamaPredictor:
        beta_t = sde.beta_0 + timesteps * (sde.beta_1 - sde.beta_0)
        diffusion = torch.sqrt(beta_t)
        dt = -1.0 / sde.N
        rows = [sigma, -0.5 * beta_t, diffusion ** 2, torch.full_like(beta_t, dt), diffusion * np.sqrt(-dt)]
        pcoef = torch.stack(rows, dim=1)
    if corrector is not NoneCorrector:
        alpha = sde.alphas.to(dev)[k]
        _, std = sde.marginal_prob(torch.zeros((len(timesteps), 1, 1, 1, 1), device=dev), timesteps)
        ccoef = torch.stack([sigma, alpha, (snr * std) ** 2 * 2 * alpha], dim=1)
    expand = (lambda t: None if t is None else t[:, None, :].expand(t.shape[0], B, t.shape[1]).contiguous())
    return expand(pcoef), expand(ccoef)


def _check_pc_pair(sde, predictor, corrector, n_steps, probability_flow, continuous, return_traj):
    """Refuse, before any GPU work, what the reference itself cannot run (or what this path does not implement)."""
    supported = (AncestralSamplingPredictor, ReverseDiffusionPredictor, EulerMaruyamaPredictor, NonePredictor)
    if predictor not in supported:
        raise NotImplementedError(f"predictor {predictor.__name__} does not run in the PC loop (the reference calls "
                                  "DDIMPredictor.update_fn without tprev); use config.sampling.method = 'ddim'")
    if corrector not in (LangevinCorrector, AnnealedLangevinDynamics, NoneCorrector):
        raise NotImplementedError(f"corrector {corrector.__name__} is not implemented")
    if not isinstance(sde, sde_lib.VPSDE):
        raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
    if continuous:
        raise NotImplementedError("continuous=True: the reference's get_score_fn asserts it away (models/utils.py:183)")
    if probability_flow and predictor is AncestralSamplingPredictor:
        raise NotImplementedError("probability flow is not supported by ancestral sampling (reference sampling.py:219)")
    if probability_flow and predictor is EulerMaruyamaPredictor:
        raise NotImplementedError("euler_maruyama with probability_flow: the reference's reverse ODE returns the float "
                                  "diffusion 0. and EulerMaruyamaPredictor indexes it (sde_lib.py:100, sampling.py:195)")
    if corrector is not NoneCorrector and n_steps < 1:
        raise NotImplementedError("a corrector needs n_steps_each >= 1 (the reference returns an unbound x_mean)")
    if return_traj:
        raise NotImplementedError("return_traj is only used by the reference's unreachable uncond_gen_interp")


def _check_guidance(guidance_scale, partial, predictor=None, corrector=None, probability_flow=False):
    """Refuse, before any GPU work, the guided runs that are not implemented.  Returns whether the run is guided."""
    scale = float(guidance_scale)
    if scale == 0.0:
        return False
    if not scale > 0.0:
        raise ValueError(f"guidance_scale must be >= 0, got {guidance_scale}")
    if partial is None:
        raise NotImplementedError("guidance_scale > 0 needs `partial`: the guidance descends the error against the partial grid")
    if probability_flow:
        raise NotImplementedError("guidance under probability flow is not implemented")
    if predictor is not None and predictor is not AncestralSamplingPredictor:
        raise NotImplementedError(f"guidance runs with the ancestral predictor (or method 'ddim'), not {predictor.__name__}")
    if corrector is not None and corrector is not NoneCorrector:
        raise NotImplementedError(f"guidance with a corrector ({corrector.__name__}) is not implemented")
    return True


def guidance_terms(model, sde_or_coef, x, labels, alpha, sigma, src, pm_flat, gm_flat, ch, chunk=None):
    """What one step of reconstruction guidance needs, at the state `x` [B,C,D,H,W] (fp32, on the GPU) the step starts from:
        eps_hat = model(x, labels)                       one evaluation, the one the step itself uses
        cot     = pm*gm*(x0_hat[ch] - src) in channel ch, 0 elsewhere, x0_hat = (x - sigma*eps_hat)/alpha    (md_guide_residual)
        g       = J^T cot                                the vector-Jacobian product of eps_hat with respect to x
        slabs   [B, 64] float64, summing to ||cot_b||^2
    Returns (eps_hat, cot, g, slabs), none of them attached to a graph.  A DDPMUNet3D runs its taped eval-mode forward and the
    data-gradient-only HIP backward (no weight-gradient work, every parameter's `.grad` stays None); any other callable goes
    through plain torch autograd.  Grad mode is switched on here: the samplers run under no_grad.
    sde_or_coef: the [B,2] float64 rows (alpha, sigma) as md_guide_residual takes them (then `alpha` / `sigma` are not read), or
    the SDE (or None): the rows are built from `alpha` and `sigma`, floats or [B] tensors.
    src: the partial grid, one shared by the batch (P values) or one per sample (B*P); pm_flat / gm_flat: [P] fp32, gm_flat may
    be None.  chunk: samples per forward and backward (default: the whole batch); exact per sample up to the forward's own
    batch dependence."""
    B = x.shape[0]
    P = x[0, 0].numel()
    if torch.is_tensor(sde_or_coef):
        coef = sde_or_coef
    else:
        rows = [torch.as_tensor(v, dtype=torch.float64, device=x.device).expand(B) for v in (alpha, sigma)]
        coef = torch.stack(rows, dim=1).contiguous()
    eps_fn = mutils.get_model_fn(model, train=False) if isinstance(model, torch.nn.Module) else model
    per_sample = src.numel() == B * P and B > 1
    src = src.reshape(B, P) if per_sample else src.reshape(P)
    step = B if not chunk else max(1, min(int(chunk), B))
    parts = []
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        with torch.enable_grad():
            xr = x[b0:b1].detach().requires_grad_(True)
            eps_hat = eps_fn(xr, labels[b0:b1])
            e = eps_hat.detach().contiguous()
            cot, slabs = ops.guide_residual(xr.detach(), e, src[b0:b1] if per_sample else src, pm_flat, gm_flat, coef[b0:b1], ch,
                                            src_bstride=P if per_sample else 0)
            g, = torch.autograd.grad(eps_hat, xr, cot)
        parts.append((e, cot, g.contiguous(), slabs))
    if len(parts) == 1:
        return parts[0]
    return tuple(torch.cat(p) for p in zip(*parts))


def get_pc_sampler(sde, shape, predictor, corrector, inverse_scaler, snr, n_steps=1, probability_flow=False,
                   continuous=False, denoise=True, eps=1e-3, device="cuda", grid_mask=None, return_traj=False):
    """Each iteration runs the reference's order (sampling.py:443-481): corrector x n_steps (one U-Net evaluation and
    one draw each), mask, predictor, mask, then the inpainting blend / re-noise of the conditional branch.  The masks
    are applied inside the kernels.  The Langevin step size is a mean over the batch this sampler sees (one shard
    per rank under torchrun).  The ancestral predictor is AncestralStepper.step, unchanged."""
    predictor = NonePredictor if predictor is None else predictor
    corrector = NoneCorrector if corrector is None else corrector
    _check_pc_pair(sde, predictor, corrector, n_steps, probability_flow, continuous, return_traj)
    B = shape[0]
    P = int(shape[2] * shape[3] * shape[4])
    n_corr = 0 if corrector is NoneCorrector else int(n_steps)

    def pc_sampler(model, partial=None, partial_mask=None, partial_channel=0, freeze_iters=None,
                   n_iters=None, noise_fn=None, guidance_scale=0.0, guidance_replace=True, guidance_chunk=None):
        """guidance_scale > 0 (reconstruction guidance; needs `partial`, the ancestral predictor, no corrector): each iteration
        is guidance_terms at the state it starts from, md_ancestral_step with that eps_hat, md_guide_apply_f32 on (x, x_mean),
        then the blend and re-noise below unless guidance_replace is off.  guidance_chunk: samples per taped forward."""
        guided = _check_guidance(guidance_scale, partial, predictor, corrector, probability_flow)
        with torch.no_grad():
            if freeze_iters is None:
                freeze_iters = sde.N + 10
            st = AncestralStepper(sde, shape, eps=eps, device=device, grid_mask=grid_mask)
            dev, timesteps, gm_flat = st.dev, st.timesteps, st.gm_flat
            pcoef, ccoef = _pc_tables(sde, timesteps, B, predictor, corrector, snr, probability_flow)
            model_fn = mutils.get_model_fn(model, train=False)
            draw = torch.randn_like if noise_fn is None else noise_fn
            x = st.prior()

            cond = partial is not None
            replace = cond and (guidance_replace or not guided)
            if cond:
                assert st.gm is not None and partial.dim() == 5 and partial_mask is not None
                ch = partial_channel
                pm_flat = partial_mask[0, ch].reshape(-1).to(dev, torch.float32).contiguous()
                src = (partial[:, ch].to(dev, torch.float32)).contiguous()
                src_bstride = 0 if src.shape[0] == 1 else P
            if guided:
                # (alpha, sigma, zeta) of every iteration's level, from the float32 tables the step's own coefficients come from
                k_all = (timesteps * (sde.N - 1) / sde.T).long()
                a_all, s_all = sde.sqrt_alphas_cumprod.to(dev)[k_all].double(), sde.sqrt_1m_alphas_cumprod.to(dev)[k_all].double()
                gcoef = torch.stack([a_all, s_all, torch.full_like(a_all, float(guidance_scale))], dim=1)
                gcoef = gcoef[:, None, :].expand(sde.N, B, 3).contiguous()
                rcoef = gcoef[:, :, :2].contiguous()
            if replace:
                # ---- initial conditioning (sampling.py:429-440), including its broadcasting quirk:
                # `sampled_update` is [B,B,R,R,R] there and `[:, partial_channel]` indexes its SECOND batch
                # axis, so every sample receives batch element `ch`'s mean and noise, scaled by its own std.
                vec_t = torch.ones(B, device=dev) * timesteps[0]
                x[:, ch] = src * gm_flat.view(1, *shape[2:])
                mean, std = sde.marginal_prob(x, vec_t)
                z0 = draw(mean[:, ch])
                upd = (mean[ch, ch][None] + std[:, None, None, None] * z0[ch][None]).contiguous()
                ops.inpaint_blend_(x, upd, pm_flat, gm_flat, ch, src_bstride=P)

            total = sde.N if cond else sde.N - 1
            if n_iters is not None:
                total = min(total, int(n_iters))
            x_mean = x
            for i in range(total):
                for j in range(n_corr):   # the reference masks once, after all n_steps corrector steps (:449-450)
                    eps_hat = model_fn(x, st.labels[i])
                    z = draw(x)
                    x, x_mean, _ = ops.langevin_step(x, eps_hat, z, gm_flat if j == n_corr - 1 else None, ccoef[i], snr,
                                                     corrector.mode)
                if guided:
                    eps_hat, cot, g, slabs = guidance_terms(model, rcoef[i], x, st.labels[i], None, None, src, pm_flat, gm_flat, ch,
                                                            chunk=guidance_chunk)
                    z = draw(x)
                    x, x_mean = ops.ancestral_step(x, eps_hat, z, gm_flat, st.coef[i])
                    ops.guide_apply_(x, x_mean, cot, g, gm_flat, gcoef[i], slabs)
                elif predictor is AncestralSamplingPredictor:
                    x, x_mean = st.step(model_fn, x, i, draw)
                elif predictor is not NonePredictor:
                    eps_hat = model_fn(x, st.labels[i])
                    z = draw(x)
                    x, x_mean = ops.sde_step(x, eps_hat, z, gm_flat, pcoef[i], predictor.kind)
                else:   # the reference's predictor returns (x, x) and masks them into two tensors
                    x_mean = x.clone() if cond else x
                if replace and i != sde.N - 1 and i < freeze_iters:
                    ops.inpaint_blend_(x, src, pm_flat, gm_flat, ch, src_bstride=src_bstride)
                    ops.inpaint_blend_(x_mean, src, pm_flat, gm_flat, ch, src_bstride=src_bstride)
                    t_i = timesteps[i]
                    lmc = -0.25 * t_i ** 2 * (sde.beta_1 - sde.beta_0) - 0.5 * t_i * sde.beta_0
                    rc = torch.stack([torch.exp(lmc), torch.sqrt(1.0 - torch.exp(2.0 * lmc))]).expand(B, 2).contiguous()
                    z2 = draw(x[:, ch]).contiguous()
                    ops.inpaint_renoise_(x, x_mean, z2, pm_flat, gm_flat, rc, ch)
            return inverse_scaler(x_mean if denoise else x), sde.N * (n_steps + 1)

    return pc_sampler


def ddim_schedule(N, schedule="quad", num_steps=100):
    """The sub-sequence of the N levels visited by the DDIM sampler (sampling.py:545-557), as fractional times seq/N.
    'quad' is hard-wired to 100 points in the reference (`num_steps` only drives 'uniform'); kept."""
    if schedule == "uniform":
        seq = list(range(0, N, N // num_steps))
    elif schedule == "quad":
        seq = [int(v) for v in list(np.linspace(0, np.sqrt(N * 0.8), 100) ** 2)]
    else:
        raise ValueError(f"unknown DDIM schedule {schedule!r}")
    return torch.tensor(seq) / N


def get_ddim_sampler(sde, shape, predictor, inverse_scaler, n_steps=1, denoise=False, eps=1e-3, device="cuda",
                     grid_mask=None):
    """Deterministic DDIM sampler on a sub-sequence of the N levels (100-point quadratic schedule by default: 99 U-Net
    evaluations instead of 999).  Mirrors `get_ddim_sampler` (sampling.py:500-570) with one repair: the reference's
    return statement reads an undefined name (`encode`, sampling.py:569), so it raises NameError whenever
    `config.sampling.noise_removal` is true; here `encode` is taken as False, i.e. noise_removal=True returns the last
    x0 prediction and noise_removal=False returns the last state (the path the unmodified reference can run, pinned by
    tests/golden/ddim.npz).  The state is float64 from the first update on, as in the reference."""
    if predictor is not DDIMPredictor:
        raise NotImplementedError("the DDIM sampler runs with the 'ddim' predictor")
    B = shape[0]
    P = int(shape[2] * shape[3] * shape[4])
    dev = torch.device(device)

    def ddim_sampler(model, schedule="quad", num_steps=100, x0=None, partial=None, partial_mask=None, partial_channel=0,
                     n_iters=None, guidance_scale=0.0, guidance_replace=True, guidance_chunk=None):
        """guidance_scale > 0 (reconstruction guidance; needs `partial`): each update is guidance_terms at the float32 state the
        U-Net sees, md_ddim_step with that eps_hat, then md_guide_apply_f64 on the float64 state and its float32 copy; x0_pred stays
        the step's own prediction.  guidance_replace off: no replacement of the known voxels, at the start or in the steps."""
        guided = _check_guidance(guidance_scale, partial)
        with torch.no_grad():
            gm = grid_mask.to(dev) if grid_mask is not None else None
            gm_flat = None
            if gm is not None:
                gm_flat = gm.reshape(-1).to(torch.float32).contiguous()
                assert gm_flat.numel() == P, "grid_mask must broadcast over batch and channels"
            x = (x0.to(dev) if x0 is not None else sde.prior_sampling(shape).to(dev))
            if gm is not None:
                x = x * gm
            part = pm = None
            ch = partial_channel
            if partial is not None:
                part = partial.to(dev, torch.float32).reshape(-1).contiguous()
                pm = partial_mask.to(dev, torch.float32).reshape(-1).contiguous()
                assert part.numel() == P and pm.numel() == P, "partial / partial_mask: one grid shared by the batch"
                if guidance_replace or not guided:
                    x[:, ch] = x[:, ch] * (1 - pm.view(shape[2:])) + part.view(shape[2:]) * pm.view(shape[2:])
            timesteps = ddim_schedule(sde.N, schedule, num_steps)
            pred = predictor(sde, None)
            model_fn = mutils.get_model_fn(model, train=False)
            x64, x32, x0_pred = x.double(), x.float().contiguous(), x.double()
            order = list(reversed(range(1, len(timesteps))))
            if n_iters is not None:
                order = order[:int(n_iters)]
            for i in order:
                vec_t = torch.ones(B, device=dev) * timesteps[i]
                vec_tprev = torch.ones(B, device=dev) * timesteps[i - 1]
                if guided:
                    coef = pred.coefficients(vec_t, vec_tprev)
                    gcoef = torch.cat([coef[:, :2], torch.full_like(coef[:, :1], float(guidance_scale))], dim=1).contiguous()
                    eps_hat, cot, g, slabs = guidance_terms(model, gcoef[:, :2].contiguous(), x32, vec_t.float() * (sde.N - 1), None,
                                                            None, part, pm, gm_flat, ch, chunk=guidance_chunk)
                    rep = (part, pm) if guidance_replace else (None, None)
                    x64, x0_pred, x32 = ops.ddim_step(x64, eps_hat, gm_flat, coef, rep[0], rep[1], ch)
                    ops.guide_apply64_(x64, x32, cot, g, gm_flat, gcoef, slabs)
                else:
                    eps_hat = model_fn(x32, vec_t.float() * (sde.N - 1))
                    x64, x0_pred, x32 = ops.ddim_step(x64, eps_hat, gm_flat, pred.coefficients(vec_t, vec_tprev), part, pm, ch)
            out = x0_pred if denoise else x64
            if gm is not None:
                out = out * gm
            return inverse_scaler(out), sde.N * (n_steps + 1)

    return ddim_sampler


def get_ode_sampler(sde, shape, inverse_scaler, rtol=1e-5, atol=1e-5, eps=1e-3, device="cuda", grid_mask=None):
    """Probability-flow ODE sampler (the reference's likelihood.py ODE run backwards, T -> eps; `config.sampling.method = 'ode'`):
    the ODE of likelihood.get_likelihood_fn without the log-density entries, so no divergence and no backward -- the model's
    inference path, one md_pf_ode_rhs launch per evaluation, likelihood.rk45 as the integrator (float64 state on the device).
    ode_sampler(model, x0=None) -> (samples, nfe); x0: the latent to start from (likelihood_fn's z decodes back to its data)
    instead of a prior draw.  get_sampling_fn reads rtol / atol from config.sampling.ode_rtol / ode_atol (default 1e-5)."""
    from . import likelihood
    shape = tuple(shape)
    dev = torch.device(device)

    def ode_sampler(model, x0=None, partial=None, **unknown):
        if partial is not None or unknown:
            raise NotImplementedError(f"the ODE sampler takes no conditioning or other options ({['partial'] * (partial is not None) + sorted(unknown)})")
        with torch.no_grad():
            x = (x0 if x0 is not None else sde.prior_sampling(shape)).to(dev)
            if x.dtype not in (torch.float32, torch.float64):
                x = x.float()
            if grid_mask is not None:
                x = x * grid_mask.to(dev).reshape((1, 1) + shape[2:]).to(x.dtype)
            fun = likelihood.get_ode_rhs(sde, model, shape, x, grid_mask=grid_mask)
            y, nfe, _ = likelihood.rk45(fun, (sde.T, eps), x.double().reshape(-1), rtol=rtol, atol=atol)
            return inverse_scaler(y.view(shape).to(x.dtype)), nfe

    return ode_sampler
