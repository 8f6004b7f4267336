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
DPM-Solver++ (not in the reference; `get_dpmpp_sampler`, config.sampling.method = 'dpmpp'): 15-25 evaluations, each followed by one
md_multistep_step launch; its schedule, time grid and coefficient rows are the float64 host functions vp_lambda ... dpmpp_tables.
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
    if name == "dpmpp":
        s = config.sampling
        return get_dpmpp_sampler(sde=sde, shape=shape, inverse_scaler=inverse_scaler, steps=int(getattr(s, "dpmpp_steps", 20)),
                                 order=int(getattr(s, "dpmpp_order", 2)), variant=getattr(s, "dpmpp_variant", "taylor"),
                                 tau=int(getattr(s, "dpmpp_tau", 0)), schedule=getattr(s, "dpmpp_schedule", "logsnr"),
                                 lower_order_final=bool(getattr(s, "dpmpp_lower_order_final", True)),
                                 denoise=config.sampling.noise_removal, eps=eps, device=config.device, grid_mask=grid_mask)
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


def _grid_mask_operands(grid_mask, dev, P):
    """(gm, gm_flat): the grid mask on `dev` as given, and as the contiguous float32 [P] the kernels read; both None without one."""
    if grid_mask is None:
        return None, None
    gm = grid_mask.to(dev)
    gm_flat = gm.reshape(-1).to(torch.float32).contiguous()
    assert gm_flat.numel() == P, "grid_mask must broadcast over batch and channels"
    return gm, gm_flat


def prepare_run(sde, shape, dev, grid_mask=None, x0=None, partial=None, partial_mask=None, ch=0, replace=False):
    """The operands of a DDIM / DPM-Solver++ run: (x, gm, gm_flat, part, pm).  x: x0 or a prior draw, on `dev`, times the grid
    mask, always a fresh tensor (never the caller's x0); part / pm: `partial` / `partial_mask` as float32 [P], None without a
    partial.  replace: channel `ch` of x starts as x*(1-pm) + part*pm."""
    P = int(shape[2] * shape[3] * shape[4])
    gm, gm_flat = _grid_mask_operands(grid_mask, dev, P)
    x = (x0.to(dev) if x0 is not None else sde.prior_sampling(shape).to(dev))
    x = x * gm if gm is not None else x.clone()
    part = pm = None
    if partial is not None:
        part = partial.to(dev, torch.float32).reshape(-1).contiguous()
        pm = partial_mask.to(dev, torch.float32).reshape(-1).contiguous()
        assert part.numel() == P and pm.numel() == P, "partial / partial_mask: one grid shared by the batch"
        if replace:
            x[:, ch] = x[:, ch] * (1 - pm.view(shape[2:])) + part.view(shape[2:]) * pm.view(shape[2:])
    return x, gm, gm_flat, part, pm


def guidance_rows(alpha, sigma, scale):
    """(alpha, sigma, zeta) rows [...,3] of md_guide_apply and their (alpha, sigma) prefix [...,2] of md_guide_residual, both
    contiguous, in the dtype of `alpha` (float64 in every sampler)."""
    gcoef = torch.stack([alpha, sigma, torch.full_like(alpha, float(scale))], dim=-1).contiguous()
    return gcoef, gcoef[..., :2].contiguous()


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
        self.gm, self.gm_flat = _grid_mask_operands(grid_mask, dev, self.P)
        # a 0/1 mask makes the reference's pre-predictor `x * grid_mask` (sampling.py:476) an exact
        # no-op on the already masked state, so one masked store per step suffices
        assert self.gm is None or bool(((self.gm_flat == 0) | (self.gm_flat == 1)).all()), "grid_mask must be binary"

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
        raise NotImplementedError("return_traj (sampling trajectories) is not implemented; latent interpolation does not need "
                                  "it: evaler.interp / --mode=interp")


class ClassifierFreeModel(torch.nn.Module):
    """A class-conditional U-Net (model.num_classes > 0) with its class ids and classifier-free guidance folded in: called as
    (x, labels) -> eps_hat like the U-Net itself, so get_model_fn, the steppers, the PC loop, DDIM, DPM-Solver++ and the ODE sampler
    take it as they take the U-Net.
        y       int64 [B] class ids (a sequence or tensor), checked here on the host, once; the null id (num_classes) is allowed
                per sample
        scale   the guidance scale w, one float or B of them: eps_hat = eps_null + w (eps_y - eps_null)
        rescale phi in [0, 1]: eps_hat times phi std(eps_y)/std(eps_hat) + (1 - phi) per sample (hip_ops.cfg_combine)
    scale == 1 for every sample: one evaluation at batch B with y, no doubling and no combine; scale == 0: one evaluation with
    the null class; otherwise one evaluation at batch 2B (x twice, y then the null class) and one md_cfg_combine launch.
    Not implemented (NotImplementedError): reconstruction guidance (guidance_scale > 0: it needs the Jacobian of the combined
    output), the likelihood and `encode=True` inversions."""

    def __init__(self, model, y, scale=1.0, rescale=0.0):
        super().__init__()
        self.model = model
        net = self.net
        if int(getattr(net, "num_classes", 0) or 0) <= 0:
            raise ValueError("classifier-free guidance needs a class-conditional model (model.num_classes > 0); this one has no classes")
        y = torch.as_tensor(y)
        if y.dim() != 1 or y.numel() < 1:
            raise ValueError(f"y must hold one class id per sample, got shape {tuple(y.shape)}")
        self.B = int(y.numel())
        self._y = net.class_ids(y, self.B, "cpu")                  # the host check: ValueError on an id out of range
        w = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
        if w.numel() not in (1, self.B) or not bool(torch.isfinite(w).all()):
            raise ValueError(f"scale must be one finite number or one per sample ({self.B}), got {scale}")
        self._w = w.expand(self.B).contiguous()
        self.rescale = float(rescale)
        if not 0.0 <= self.rescale <= 1.0:
            raise ValueError(f"rescale must lie in [0, 1], got {rescale}")
        self.mode = "cond" if bool((w == 1).all()) else ("null" if bool((w == 0).all()) else "both")
        self._dev = {}

    @property
    def net(self):
        return self.model.module if hasattr(self.model, "module") else self.model

    def _operands(self, device):
        """(class ids of the evaluation, w [B] or None) on `device`, built once per device."""
        key = str(device)
        if key not in self._dev:
            net, null = self.net, torch.full_like(self._y, self.net.null_class)
            ids = {"cond": self._y, "null": null, "both": torch.cat([self._y, null])}[self.mode]
            self._dev[key] = (net.class_ids(ids, ids.numel(), device), self._w.to(device) if self.mode == "both" else None)
        return self._dev[key]

    def forward(self, x, labels):
        if x.shape[0] != self.B:
            raise ValueError(f"this ClassifierFreeModel holds {self.B} class ids; the batch has {x.shape[0]} samples")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("classifier-free guidance under a gradient with respect to x (reconstruction guidance, "
                                      "likelihood) is not implemented: it needs the Jacobian of the combined output")
        ids, w = self._operands(x.device)
        if self.mode != "both":
            return self.model(x, labels, y=ids)
        eps2 = self.model(torch.cat([x, x]), torch.cat([labels, labels]), y=ids)
        return ops.cfg_combine(eps2, w, rescale=self.rescale)


def _refuse_cfg(model, what):
    if isinstance(model, ClassifierFreeModel):
        raise NotImplementedError(f"classifier-free guidance with {what} is not implemented")


def _check_guidance(guidance_scale, partial, predictor=None, corrector=None, probability_flow=False, model=None):
    """Refuse, before any GPU work, the guided runs that are not implemented.  Returns whether the run is guided."""
    scale = float(guidance_scale)
    if scale == 0.0:
        return False
    _refuse_cfg(model, "reconstruction guidance (guidance_scale > 0: it needs the Jacobian of the combined output)")
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
        guided = _check_guidance(guidance_scale, partial, predictor, corrector, probability_flow, model=model)
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
                gcoef, rcoef = guidance_rows(a_all[:, None].expand(sde.N, B), s_all[:, None].expand(sde.N, B), guidance_scale)
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
    dev = torch.device(device)

    def ddim_sampler(model, schedule="quad", num_steps=100, x0=None, partial=None, partial_mask=None, partial_channel=0,
                     n_iters=None, guidance_scale=0.0, guidance_replace=True, guidance_chunk=None, encode=False):
        """guidance_scale > 0 (reconstruction guidance; needs `partial`): each update is guidance_terms at the float32 state the
        U-Net sees, md_ddim_step with that eps_hat, then md_guide_apply_f64 on the float64 state and its float32 copy; x0_pred stays
        the step's own prediction.  guidance_replace off: no replacement of the known voxels, at the start or in the steps.
        encode (DDIM inversion; the meaning given to the name the reference reads at sampling.py:569 and never defines): x0 holds
        data grids, and the same schedule is walked upward, i = 1 .. len-1: the U-Net is evaluated at the current level
        timesteps[i-1] and md_ddim_step moves the state to timesteps[i] with coefficients(current, next), whose row works in either
        direction of time.  n_iters limits the upward steps.  Returns the float64 state at the top level -- what
        ddim_sampler(x0=latent) starts from -- whatever `denoise` says, without the inverse scaler: a latent is no data grid."""
        if encode:
            _refuse_cfg(model, "DDIM inversion (encode=True)")
            if x0 is None:
                raise ValueError("encode=True needs x0: the data grids to invert")
            if partial is not None or float(guidance_scale) != 0.0:
                raise NotImplementedError("DDIM inversion (encode=True) of a partial grid or under guidance is not implemented")
        guided = _check_guidance(guidance_scale, partial, model=model)
        with torch.no_grad():
            if encode:
                x, gm, gm_flat, _, _ = prepare_run(sde, shape, dev, grid_mask, x0)
                timesteps = ddim_schedule(sde.N, schedule, num_steps)
                pred = predictor(sde, None)
                model_fn = mutils.get_model_fn(model, train=False)
                x64, x32 = x.double(), x.float().contiguous()
                order = list(range(1, len(timesteps)))
                if n_iters is not None:
                    order = order[:int(n_iters)]
                for i in order:
                    vec_t = torch.ones(B, device=dev) * timesteps[i - 1]
                    vec_tnext = torch.ones(B, device=dev) * timesteps[i]
                    eps_hat = model_fn(x32, vec_t.float() * (sde.N - 1))
                    x64, _, x32 = ops.ddim_step(x64, eps_hat, gm_flat, pred.coefficients(vec_t, vec_tnext))
                return x64, sde.N * (n_steps + 1)
            ch = partial_channel
            x, gm, gm_flat, part, pm = prepare_run(sde, shape, dev, grid_mask, x0, partial, partial_mask, ch,
                                                   replace=guidance_replace or not guided)
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
                    gcoef, rcoef = guidance_rows(coef[:, 0], coef[:, 1], guidance_scale)
                    eps_hat, cot, g, slabs = guidance_terms(model, rcoef, x32, vec_t.float() * (sde.N - 1), None, None, part, pm,
                                                            gm_flat, ch, chunk=guidance_chunk)
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


# ---- DPM-Solver++ (Lu et al. 2022): multistep exponential integrator in the data prediction, orders 1-3, ODE and SDE variants ----
# Host side, all float64 numpy: the continuous VP schedule the re-noise lines above and likelihood.vp_coefficients use, its
# inverse in the half-log-SNR lambda, the time grid and the coefficient rows of md_multistep_step.
def vp_log_alpha_sigma(sde, t):
    """(log alpha, sigma) of the continuous VP schedule at t (float or array): lmc = -t^2 (b1-b0)/4 - t b0/2, alpha = exp(lmc),
    sigma = sqrt(-expm1(2 lmc))."""
    t = np.asarray(t, np.float64)
    lmc = -0.25 * t ** 2 * (sde.beta_1 - sde.beta_0) - 0.5 * t * sde.beta_0
    return lmc, np.sqrt(-np.expm1(2.0 * lmc))


def vp_lambda(sde, t):
    """Half-log-SNR lambda(t) = log alpha - log sigma."""
    lmc, sigma = vp_log_alpha_sigma(sde, t)
    return lmc - np.log(sigma)


def vp_t_of_lambda(sde, lam):
    """The inverse of vp_lambda in closed form: log alpha = -logaddexp(0, -2 lambda)/2 =: -L/2, and the positive root of
    (b1-b0) t^2 + 2 b0 t - 2 L = 0 written without cancellation."""
    L = np.logaddexp(0.0, -2.0 * np.asarray(lam, np.float64))
    a, b0 = float(sde.beta_1 - sde.beta_0), float(sde.beta_0)
    return 2.0 * L / (b0 + np.sqrt(b0 * b0 + 2.0 * a * L))


def dpmpp_schedule(sde, steps, kind="logsnr", eps=1e-3):
    """steps+1 times from sde.T down to eps, float64: 'logsnr' uniform in lambda, 'uniform' in t, 'quad' in sqrt(t)."""
    steps, T, eps = int(steps), float(sde.T), float(eps)
    if steps < 1 or not 0.0 < eps < T:
        raise ValueError(f"dpmpp_schedule: steps >= 1 and 0 < eps < T, got steps={steps} eps={eps}")
    if kind == "logsnr":
        t = vp_t_of_lambda(sde, np.linspace(vp_lambda(sde, T), vp_lambda(sde, eps), steps + 1))
    elif kind == "uniform":
        t = np.linspace(T, eps, steps + 1)
    elif kind == "quad":
        t = np.linspace(np.sqrt(T), np.sqrt(eps), steps + 1) ** 2
    else:
        raise ValueError(f"unknown DPM-Solver++ schedule {kind!r}")
    t[0], t[-1] = T, eps
    return torch.from_numpy(t)


_DPMPP_SERIES_BELOW = 0.5


def dpmpp_moments(g, k_max=2):
    """I_k(g) = g * int_0^1 exp(-g (1-u)) u^k du for k = 0..k_max and g > 0: I_0 = -expm1(-g), I_k = 1 - k I_{k-1} / g.  The
    recursion subtracts nearly equal numbers for small g (4e-10 off in I_2 at g = 1e-3), so below _DPMPP_SERIES_BELOW the series
    I_k = k! sum_n (-1)^n g^(n+1) / (n+k+1)! is summed instead: its terms fall by more than g/(k+2) each, 30 of them are exact
    to the last bit there."""
    g = float(g)
    if g < _DPMPP_SERIES_BELOW:
        out = []
        for k in range(k_max + 1):
            term, total = g / (k + 1), 0.0                 # n = 0: g k! / (k+1)!
            for n in range(30):
                total += term
                term *= -g / (n + k + 2)
            out.append(total)
        return out
    out = [-float(np.expm1(-g))]
    for k in range(1, k_max + 1):
        out.append(1.0 - k * out[-1] / g)
    return out


def dpmpp_weights(h, rs=(), order=1, variant="taylor", tau=0):
    """w_j, j = 0..order-1, of x_t = c_x x_s + alpha_t sum_j w_j x0_j: w_j = g int_0^1 exp(-g (1-u)) l_j(u) du with g = h (tau = 0)
    or 2 h (tau = 1), l_j the Lagrange polynomials in u = (lambda - lambda_s)/h on the nodes 0, -r_1, -r_1-r_2 (rs: the earlier step
    lengths over h, newest first).  variant 'midpoint' (order 2): w_0 = I_0 (1 + 1/(2r)), w_1 = -I_0/(2r), the 2M update as published."""
    order, rs = int(order), [float(r) for r in rs]
    if order not in (1, 2, 3) or len(rs) < order - 1 or tau not in (0, 1) or variant not in ("taylor", "midpoint"):
        raise ValueError(f"dpmpp_weights: order {order} with {len(rs)} earlier steps, variant {variant!r}, tau {tau}")
    g = float(h) * (2.0 if tau else 1.0)
    mom = dpmpp_moments(g, order - 1)
    if order == 2 and variant == "midpoint":
        return [mom[0] * (1.0 + 0.5 / rs[0]), -mom[0] * 0.5 / rs[0]]
    nodes = [0.0, -rs[0] if order > 1 else 0.0, -(rs[0] + rs[1]) if order > 2 else 0.0][:order]
    w = []
    for j in range(order):
        others = [n for i, n in enumerate(nodes) if i != j]
        poly = np.poly(others) if others else np.array([1.0])         # highest power first
        den = float(np.prod([nodes[j] - n for n in others])) if others else 1.0
        w.append(float(sum(c * mom[len(poly) - 1 - i] for i, c in enumerate(poly)) / den))
    return w


def dpmpp_orders(steps, order, lower_order_final=True):
    """The order of every step: capped by the history available, and with lower_order_final and fewer than 15 steps also by the
    steps that remain (order 3 over 10 steps: 1, 2, 3, ..., 3, 2, 1)."""
    steps, order = int(steps), int(order)
    tail = lower_order_final and steps < 15
    return [min(order, i + 1, steps - i) if tail else min(order, i + 1) for i in range(steps)]


def dpmpp_tables(sde, times, order=2, variant="taylor", tau=0, lower_order_final=True):
    """Rows of md_multistep_step for the steps times[i] -> times[i+1]: ([steps, 8] float64 = {alpha_s, sigma_s, c_x, c_0, c_1,
    c_2, c_z, 0}, labels [steps] float64 = t_s (N-1)).  With h = lambda_t - lambda_s:
        tau = 0: c_x = sigma_t/sigma_s,           c_j = alpha_t w_j(h),   c_z = 0
        tau = 1: c_x = sigma_t/sigma_s exp(-h),   c_j = alpha_t w_j(2h),  c_z = sigma_t sqrt(1 - exp(-2h))     (SDE-DPM-Solver++)
    Order 1 with tau = 0 is DDIM on the continuous schedule."""
    if int(order) not in (1, 2, 3) or variant not in ("taylor", "midpoint") or tau not in (0, 1):
        raise ValueError(f"dpmpp_tables: order 1-3, variant 'taylor' | 'midpoint', tau 0 | 1; got {order}, {variant!r}, {tau}")
    t = np.asarray(times, np.float64)
    steps = len(t) - 1
    lmc, sigma = vp_log_alpha_sigma(sde, t)
    alpha, lam = np.exp(lmc), lmc - np.log(sigma)
    hs = np.diff(lam)
    if steps < 1 or not np.all(hs > 0):
        raise ValueError("dpmpp_tables: the times must decrease")
    rows = np.zeros((steps, 8))
    for i, k in enumerate(dpmpp_orders(steps, order, lower_order_final)):
        h = hs[i]
        w = dpmpp_weights(h, [hs[i - 1 - j] / h for j in range(k - 1)], k, variant, tau)
        rows[i, 0], rows[i, 1] = alpha[i], sigma[i]
        rows[i, 2] = sigma[i + 1] / sigma[i] * (np.exp(-h) if tau else 1.0)
        rows[i, 3:3 + k] = alpha[i + 1] * np.asarray(w)
        rows[i, 6] = sigma[i + 1] * np.sqrt(-np.expm1(-2.0 * h)) if tau else 0.0
    return torch.from_numpy(rows), torch.from_numpy(t[:-1] * (sde.N - 1))


def get_dpmpp_sampler(sde, shape, inverse_scaler, steps=20, order=2, variant="taylor", tau=0, schedule="logsnr",
                      lower_order_final=True, denoise=False, eps=1e-3, device="cuda", grid_mask=None):
    """DPM-Solver++ sampler (`config.sampling.method = 'dpmpp'`): `steps` U-Net evaluations instead of DDIM's 99, each followed by
    one md_multistep_step launch on the float64 state.  Set up like ddim_sampler (prepare_run: masked prior draw or x0, replacement of
    the known voxels at the start), then the same loop: replacement in every step, guidance_terms + md_guide_apply_f64 under guidance.  tau = 1: the SDE variant, one
    float32 draw(x_f32) per step taken before the launch.  denoise: return the last clean-grid prediction.  Returns (samples,
    number of evaluations)."""
    if not isinstance(sde, sde_lib.VPSDE):
        raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
    B = shape[0]
    dev = torch.device(device)
    times = dpmpp_schedule(sde, steps, schedule, eps)
    rows, labels = dpmpp_tables(sde, times, order, variant, tau, lower_order_final)
    orders = dpmpp_orders(steps, order, lower_order_final)

    def dpmpp_sampler(model, x0=None, partial=None, partial_mask=None, partial_channel=0, n_iters=None, guidance_scale=0.0,
                      guidance_replace=True, guidance_chunk=None, draw=torch.randn_like):
        guided = _check_guidance(guidance_scale, partial, model=model)
        with torch.no_grad():
            ch = partial_channel
            replace = partial is not None and (guidance_replace or not guided)
            x, gm, gm_flat, part, pm = prepare_run(sde, shape, dev, grid_mask, x0, partial, partial_mask, ch, replace)
            rep = (part, pm) if replace else (None, None)
            # per-step rows pre-expanded over the batch: no host-side tensor math inside the loop
            coef = rows.to(dev)[:, None, :].expand(steps, B, 8).contiguous()
            lab = labels.to(dev, torch.float32)[:, None].expand(steps, B).contiguous()
            if guided:
                gcoef, rcoef = guidance_rows(coef[:, :, 0], coef[:, :, 1], guidance_scale)
            model_fn = mutils.get_model_fn(model, train=False)
            # the sampler's own buffers, rotated: two float64 states, a ring of three clean-grid predictions, the U-Net input
            xa, x32 = x.double().contiguous(), x.float().contiguous()
            xb, ring = torch.empty_like(xa), [torch.empty_like(xa) for _ in range(3)]
            x0_pred = xa
            total = steps if n_iters is None else min(steps, int(n_iters))
            for i in range(total):
                if guided:
                    eps_hat, cot, g, slabs = guidance_terms(model, rcoef[i], x32, lab[i], None, None, part, pm, gm_flat, ch,
                                                            chunk=guidance_chunk)
                else:
                    eps_hat = model_fn(x32, lab[i])
                z = draw(x32) if tau else None
                hist = [ring[(i - 1 - j) % 3] for j in range(orders[i] - 1)]
                x0_pred = ring[i % 3]
                ops.multistep_step(xa, eps_hat, hist, z, gm_flat, coef[i], rep[0], rep[1], ch, out=(xb, x0_pred, x32))
                xa, xb = xb, xa
                if guided:
                    ops.guide_apply64_(xa, x32, cot, g, gm_flat, gcoef[i], slabs)
            out = x0_pred if denoise else xa
            if gm is not None:
                out = out * gm
            return inverse_scaler(out), total

    return dpmpp_sampler


def get_ode_sampler(sde, shape, inverse_scaler, rtol=1e-5, atol=1e-5, eps=1e-3, device="cuda", grid_mask=None):
    """Probability-flow ODE sampler (the reference's likelihood.py ODE run backwards, T -> eps; `config.sampling.method = 'ode'`):
    the ODE of likelihood.get_likelihood_fn without the log-density entries, so no divergence and no backward -- the model's
    inference path, one md_pf_ode_rhs launch per evaluation, likelihood.rk45 as the integrator (float64 state on the device).
    ode_sampler(model, x0=None) -> (samples, nfe); x0: the latent to start from (likelihood_fn's z decodes back to its data)
    instead of a prior draw.  get_sampling_fn reads rtol / atol from config.sampling.ode_rtol / ode_atol (default 1e-5).
    ode_sampler(model, x0=grids, encode=True) -> (latent, nfe): the same drift integrated upward, eps -> T (ODE inversion; no
    divergence, no backward), from data grids; the latent is returned as it is, without the inverse scaler."""
    from . import likelihood
    shape = tuple(shape)
    dev = torch.device(device)

    def ode_sampler(model, x0=None, partial=None, encode=False, **unknown):
        if partial is not None or unknown:
            raise NotImplementedError(f"the ODE sampler takes no conditioning or other options ({['partial'] * (partial is not None) + sorted(unknown)})")
        if encode:
            _refuse_cfg(model, "ODE inversion (encode=True)")
        if encode and x0 is None:
            raise ValueError("encode=True needs x0: the data grids to invert")
        with torch.no_grad():
            x = (x0 if x0 is not None else sde.prior_sampling(shape)).to(dev)
            if x.dtype not in (torch.float32, torch.float64):
                x = x.float()
            if grid_mask is not None:
                x = x * grid_mask.to(dev).reshape((1, 1) + shape[2:]).to(x.dtype)
            fun = likelihood.get_ode_rhs(sde, model, shape, x, grid_mask=grid_mask)
            span = (eps, sde.T) if encode else (sde.T, eps)
            y, nfe, _ = likelihood.rk45(fun, span, x.double().reshape(-1), rtol=rtol, atol=atol)
            y = y.view(shape).to(x.dtype)
            return (y if encode else inverse_scaler(y)), nfe

    return ode_sampler
