"""Unconditional predictor-corrector sampling.

Mirrors ``get_sampling_fn`` (sampling/unconditional.py:13-75) and ``get_pc_sampler`` (:161-228):
``pc_sampler(model, show_evolution=False) -> (samples, {'times', 'steps'[, 'evolution']})``.
``sampling.method='ode'`` gives the probability-flow ODE sampler (:93-158): scipy's black-box RK45 on the host, every drift
evaluation = one network evaluation + one HIP axpby; with ``device_loop=True`` (``config.sampling.csd_device_loop``) the same RK45
with the float64 state in device memory (ode_solver.py, csrc/ode_rk45.hip) and one 8-byte read per step.  ``get_inpainting_fn`` /
``get_pc_inpainter`` (:78-91, :230-345): the PC loop with the known pixels re-imposed after every update (masked blend on csd_axpby /
csd_mul), or - ``device_loop=True`` - the same sampler on the fused device loop (csd_pc_inpaint_sample: one library call, on-device
noise, no host synchronisation).
"""
import functools

import torch

from ..models import utils as mutils
from . import fused
from .correctors import NoneCorrector, get_corrector
from .predictors import NonePredictor, get_predictor


def get_sampling_fn(config, sde, shape, eps, predictor='default', corrector='default', p_steps='default',
                    c_steps='default', snr='default', denoise='default'):
    predictor = get_predictor((config.sampling.predictor if predictor == 'default' else predictor).lower())
    corrector = get_corrector((config.sampling.corrector if corrector == 'default' else corrector).lower())
    if p_steps == 'default':
        p_steps = config.model.num_scales
    if c_steps == 'default':
        c_steps = config.sampling.n_steps_each
    if snr == 'default':
        snr = config.sampling.snr
    if denoise == 'default':
        denoise = config.sampling.noise_removal
    method = config.sampling.method.lower()
    if method == 'ode':
        return get_ode_sampler(sde=sde, shape=shape, denoise=denoise, eps=eps,
                               device_loop=config.sampling.get('csd_device_loop', False))
    if method != 'pc':
        raise ValueError(f"Sampler name {config.sampling.method} unknown.")
    return get_pc_sampler(sde=sde, shape=shape, predictor=predictor, corrector=corrector, snr=snr,
                          p_steps=p_steps, c_steps=c_steps, probability_flow=config.sampling.probability_flow,
                          continuous=config.training.continuous, denoise=denoise, eps=eps)


def get_ode_sampler(sde, shape, denoise=False, rtol=1e-5, atol=1e-5, method='RK45', eps=1e-3, device_loop=False):
    """Probability-flow ODE sampler with a black-box solver (sampling/unconditional.py:93-158):
    ``ode_sampler(model, z=None) -> (samples, nfe)``.  The drift of the reverse-time ODE, f(x, t) - g(t)^2 score / 2
    (sde_lib.py:123-133), is linear in x for every SDE of sde_lib, so an evaluation is the score network plus one
    ``csd_axpby`` with host scalars; the state crosses to the host per evaluation exactly as in the reference.

    ``device_loop=True`` integrates with ``ode_solver.solve`` instead: the same step-size controller, the float64 state and the stage
    derivatives in device memory.  An evaluation is the inference forward on the fp32 input that the stage combination wrote
    (``csd_ode_combine``) and one fp64 drift pass (``csd_ode_drift``: a x + c h, c = -g^2 / (2 std)); per evaluation the host
    uploads the coefficients and labels (20 B bytes) and per attempted step it reads one double.  RK45, a HipUNet on the GPU and a
    VESDE / VPSDE / subVPSDE only: anything else raises NotImplementedError naming the reason, never the host loop."""
    from scipy import integrate

    from .. import ops
    from .predictors import ReverseDiffusionPredictor, _linear_sde_coeffs

    def denoise_update_fn(model, x):
        score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
        predictor_obj = ReverseDiffusionPredictor(sde, score_fn, probability_flow=False)
        vec_eps = torch.ones(x.shape[0], device=x.device) * eps
        _, x = predictor_obj.update_fn(x, vec_eps)
        return x

    def drift_fn(model, x, t):
        score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)
        phi, g = _linear_sde_coeffs(sde, t)
        return ops.axpby(x, score_fn(x, t), alpha=phi, beta=-0.5 * g * g)

    def device_solve(model, x):
        """the final state (float64, flat) and nfe of the device-resident integration from sde.T to eps"""
        import ctypes

        from .. import likelihood, ode_solver
        from .._lib import check, current_stream, lib, ptr
        why = likelihood.why_not_device_loop(model, sde, False, method)
        if why is not None:
            raise NotImplementedError('get_ode_sampler(device_loop=True): ' + why)
        dev, B, S = model.device, shape[0], model.image_size
        D, net_stride = model.x_channels * S * S, model.out_channels * S * S
        if tuple(x.shape) != (B, model.x_channels, S, S):
            raise RuntimeError('the initial sample has shape %s, expected %s' % (tuple(x.shape), (B, model.x_channels, S, S)))
        probe = likelihood._Probe(model)
        score = mutils.get_score_fn(sde, probe, conditional=False, train=False, continuous=True)
        model.eval()
        model._ensure_packed()
        ws = model._workspace(B)
        x32 = torch.empty(B * D, dtype=torch.float32, device=dev)
        out = torch.empty(B * net_stride, dtype=torch.float32, device=dev)
        ring = ode_solver.CoefficientRing(B, dev)
        p_a, p_c = ctypes.c_void_p(ring.a.data_ptr()), ctypes.c_void_p(ring.c.data_ptr())
        stream = current_stream(dev)

        def rhs(t, y, x32_, k_out):
            ring.upload(*likelihood._row_coefficients(sde, score, probe, t, B, False))
            check(lib().csd_unet_forward(model._h, ptr(model._packed), ptr(ws), ws.numel(), ptr(x32_), None, ptr(ring.labels), ptr(out),
                                         B, None, 0.0, stream), 'unet_forward')
            check(lib().csd_ode_drift(ptr(y), ptr(out), net_stride, p_a, p_c, ptr(k_out), B, D, stream), 'ode_drift')

        be = ode_solver.DeviceBackend(x.to(device=dev).reshape(-1).double(), x32=x32)
        res = ode_solver.solve(rhs, be, sde.T, eps, rtol, atol)
        return res.y, res.nfev

    def ode_sampler(model, z=None):
        with torch.no_grad():
            x = sde.prior_sampling(shape).to(model.device) if z is None else z
            if device_loop:
                xf, nfe = device_solve(model, x)
                x = xf.reshape(shape).type(torch.float32)
                if denoise:
                    x = denoise_update_fn(model, x)
                return x, nfe

            def ode_func(t, xf):
                xt = mutils.from_flattened_numpy(xf, shape).to(model.device).type(torch.float32)
                vec_t = torch.ones(shape[0], device=xt.device) * t
                return mutils.to_flattened_numpy(drift_fn(model, xt, vec_t))

            solution = integrate.solve_ivp(ode_func, (sde.T, eps), mutils.to_flattened_numpy(x), rtol=rtol, atol=atol,
                                           method=method)
            nfe = solution.nfev
            x = torch.tensor(solution.y[:, -1]).reshape(shape).to(model.device).type(torch.float32)
            if denoise:
                x = denoise_update_fn(model, x)
            return x, nfe

    return ode_sampler


def get_inpainting_fn(config, sde, eps, n_steps_each=1):
    """sampling/unconditional.py:78-91."""
    return get_pc_inpainter(sde=sde, predictor=get_predictor(config.sampling.predictor.lower()),
                            corrector=get_corrector(config.sampling.corrector.lower()), snr=config.sampling.snr,
                            n_steps=n_steps_each, probability_flow=config.sampling.probability_flow,
                            continuous=config.training.continuous, denoise=config.sampling.noise_removal, eps=eps,
                            device_loop=config.sampling.get('csd_device_loop', False))


def get_pc_inpainter(sde, predictor, corrector, snr, n_steps=1, probability_flow=False, continuous=False, denoise=True, eps=1e-5,
                     device_loop=False):
    """Image inpainting with an unconditional model (sampling/unconditional.py:230-345):
    ``pc_inpainter(model, data, mask, show_evolution=False, noise_tape=None, seed=None, global_norm=None) -> (x, info)``; ``mask`` is
    1 on known pixels.  After every corrector / predictor update the known region is replaced by the data perturbed to the current
    noise level.

    ``device_loop=False`` (the default) is the step-by-step loop, exactly as it has always run: two update objects per step, the
    blend on csd_axpby / csd_mul, noise from torch's generator (``torch.randn`` / ``torch.randn_like``, which is what a caller who
    patches or seeds them relies on).  That path is not touched by ``device_loop`` and takes none of the three keywords: it raises
    NotImplementedError for them, like ``pc_sampler`` off the fused loop.

    ``device_loop=True`` runs the whole sampler (``sde.N`` steps) as one call of the fused device loop (``fused.run(...,
    inpaint=(data, mask))``) with the re-imposition as one kernel per phase: Philox noise on the device (``seed=``; None = a fresh
    key), ``noise_tape=`` in the draw order prior | per step [z_corrector] z_blend [z_predictor] z_blend, ``global_norm=(reduce_fn,
    global_batch)`` for a batch that is one shard of a larger one, NonFiniteError instead of NaN images.  ``mask`` may broadcast to
    ``data``.  A (model, sde, predictor, corrector, n_steps) combination the loop does not cover raises NotImplementedError naming the
    reason - there is no silent fall-back to the step-by-step loop."""
    from .. import ops
    from ..losses import _bstd

    def blend(a, b, mask):
        """a*(1 - mask) + b*mask = a + (b - a)*mask on the device"""
        from ..grad_ops import _mul
        return ops.axpby(a, _mul(ops.axpby(b, a, 1.0, -1.0), mask))

    def inpaint_update(data, mask, x, vec_t):
        m, std = _bstd(sde, data, vec_t)                       # mean scale / std of p_t(x | data): [B] host scalars
        mean = data if bool(torch.all(m == 1)) else ops.scale_rows(data, m.to(data.device))
        masked = ops.axpby(mean, ops.scale_rows(torch.randn_like(x), std.to(data.device)))
        x = blend(x, masked, mask)
        x_mean = blend(x, mean, mask)
        return x, x_mean

    run = _constrained_pc_sampler('get_pc_inpainter', 'inpainting', sde, predictor, corrector, snr, n_steps, probability_flow, continuous,
                                  denoise, eps, device_loop)

    def pc_inpainter(model, data, mask, show_evolution=False, noise_tape=None, seed=None, global_norm=None):
        def start(timesteps):
            d, m = data.contiguous().float(), mask.contiguous().float()
            x = blend(sde.prior_sampling(d.shape).to(d.device), d, m)
            return x, lambda x, i, vec_t: inpaint_update(d, m, x, vec_t)

        return run(model, data, {'inpaint': (data, mask)}, start, show_evolution, noise_tape, seed, global_norm)

    return pc_inpainter


def get_colorization_fn(config, sde, eps, n_steps_each=1):
    """The colorizer of a config, read like ``get_inpainting_fn`` reads it (``config.sampling.csd_device_loop``: the device loop)."""
    return get_pc_colorizer(sde=sde, predictor=get_predictor(config.sampling.predictor.lower()),
                            corrector=get_corrector(config.sampling.corrector.lower()), snr=config.sampling.snr,
                            n_steps=n_steps_each, probability_flow=config.sampling.probability_flow,
                            continuous=config.training.continuous, denoise=config.sampling.noise_removal, eps=eps,
                            device_loop=config.sampling.get('csd_device_loop', False))


def get_pc_colorizer(sde, predictor, corrector, snr, n_steps=1, probability_flow=False, continuous=False, denoise=True, eps=1e-5,
                     device_loop=False):
    """Image colorization with an unconditional 3-channel model (controllable_generation.py:95-191 of the reference, without its
    ``inverse_scaler``): ``pc_colorizer(model, gray_scale_img, show_evolution=False, noise_tape=None, seed=None, global_norm=None) ->
    (x, info)``; ``gray_scale_img`` is [B, 3, H, W] with equal channels.  A fixed orthonormal 3 x 3 matrix rotates the channels so that
    channel 0 is the gray one; after every corrector / predictor update that channel is replaced by the gray image perturbed to the
    current noise level (``ops.colorize_blend``, one kernel) and the state rotated back.

    ``device_loop=False`` (the default) is the step-by-step loop: two update objects per step, the prior and the draws from torch's
    generator (``sde.prior_sampling`` / ``torch.randn_like``), the re-imposition through ``ops.colorize_blend`` with that draw.  It
    takes none of the three keywords and raises NotImplementedError for them.

    ``device_loop=True`` runs the whole sampler (``sde.N`` steps) as one call of the fused device loop (``fused.run(...,
    colorize=gray_scale_img)``): Philox noise on the device (``seed=``; None = a fresh key), ``noise_tape=`` in the draw order prior |
    per step [z_corrector] z_colorize [z_predictor] z_colorize (full-size draws), ``global_norm=(reduce_fn, global_batch)``,
    NonFiniteError instead of NaN images.  A (model, sde, predictor, corrector, n_steps) combination the loop does not cover raises
    NotImplementedError naming the reason - there is no silent fall-back to the step-by-step loop."""
    from .. import ops

    def three_channels(model):
        if getattr(model, 'x_channels', 3) != 3:
            return 'colorization needs a 3-channel state, this network has %d channels' % model.x_channels
        return None

    run = _constrained_pc_sampler('get_pc_colorizer', 'colorization', sde, predictor, corrector, snr, n_steps, probability_flow, continuous,
                                  denoise, eps, device_loop, extra_check=three_channels)

    def pc_colorizer(model, gray_scale_img, show_evolution=False, noise_tape=None, seed=None, global_norm=None):
        def start(timesteps):
            gray = gray_scale_img.contiguous().float()
            gray0 = ops.colorize_gray0(gray)                                  # once per call
            mean_scale, std = fused.inpaint_tables(sde, timesteps)            # p_t(x | gray) per step: host scalars
            x = ops.colorize_start(sde.prior_sampling(gray.shape).to(gray.device).float().contiguous(), gray0)
            return x, lambda x, i, vec_t: ops.colorize_blend(x.contiguous(), gray0, torch.randn_like(x), float(mean_scale[i]),
                                                             float(std[i]))

        return run(model, gray_scale_img, {'colorize': gray_scale_img}, start, show_evolution, noise_tape, seed, global_norm)

    return pc_colorizer


def _constrained_pc_sampler(name, noun, sde, predictor, corrector, snr, n_steps, probability_flow, continuous, denoise, eps, device_loop,
                            extra_check=lambda model: None):
    """The PC sampler behind ``get_pc_inpainter`` / ``get_pc_colorizer`` (``name``; ``noun``: what its refusals call the constraint):
    ``run(model, like, constraint, start, show_evolution, noise_tape, seed, global_norm) -> (x, info)``.  ``like``: the tensor whose
    shape and device the state takes.  ``constraint``: the keyword ``fused.run`` takes for it on the device loop.  ``start(timesteps)
    -> (x0, reimpose)``: the step-by-step loop's initial state and its ``reimpose(x, i, vec_t) -> (x, x_mean)`` behind every update of
    step ``i``, both with the getter's own draws.  ``extra_check(model)``: one more reason the device loop does not cover the model."""
    pred_fn = functools.partial(shared_predictor_update_fn, sde=sde, predictor=predictor, probability_flow=probability_flow,
                                continuous=continuous)
    corr_fn = functools.partial(shared_corrector_update_fn, sde=sde, corrector=corrector, continuous=continuous, snr=snr,
                                n_steps=n_steps)
    pred = NonePredictor if predictor is None else predictor
    corr = NoneCorrector if corrector is None else corrector

    def why_not_fused(model):
        """None when the device loop covers this sampler, else the reason"""
        from ..models.ddpm import HipUNet
        if not isinstance(model, HipUNet):
            return 'the model is a %s, not a HipUNet' % type(model).__name__
        if getattr(model, 'y_channels', 0) > 0:
            return '%s uses an unconditional network, this one takes a %d-channel condition' % (noun, model.y_channels)
        why = extra_check(model)
        if why is not None:
            return why
        if n_steps != 1:
            return 'n_steps = %d corrector steps per update (the device loop runs 1)' % n_steps
        if isinstance(sde, dict):
            return 'a single SDE is needed, not an {x, y} pair'
        if not fused.fusable(model, sde, pred, corr, n_steps, probability_flow, continuous):
            return 'the device loop does not implement (%s, %s, %s, probability_flow=%s, continuous=%s)' % (
                type(sde).__name__, pred.__name__, corr.__name__, probability_flow, continuous)
        if model.device.type != 'cuda':
            return 'the model is on %s, the device loop runs on the GPU' % model.device
        return None

    def run(model, like, constraint, start, show_evolution, noise_tape, seed, global_norm):
        if device_loop:
            why = why_not_fused(model)
            if why is not None:
                raise NotImplementedError('%s(device_loop=True): %s' % (name, why))
            x, rec, _ = fused.run(model, sde, tuple(like.shape), None, sde.N, snr, eps, denoise, noise_tape=noise_tape, seed=seed,
                                  record=show_evolution, unconditional_label=fused.unconditional_label(model), global_norm=global_norm,
                                  predictor=pred, corrector=corr, probability_flow=probability_flow, continuous=continuous, **constraint)
            return x, ({'evolution': rec.cpu()} if show_evolution else {})
        for kw, value in (('noise_tape', noise_tape), ('seed', seed), ('global_norm', global_norm)):
            if value is not None:
                raise NotImplementedError('%s is only available on the device loop: %s(..., device_loop=True)' % (kw, name))
        with torch.no_grad():
            timesteps = torch.linspace(sde.T, eps, sde.N)
            x, reimpose = start(timesteps)
            evolution = [x.cpu()] if show_evolution else None
            x_mean = x
            for i in range(sde.N):
                vec_t = torch.ones(like.shape[0], device=like.device) * timesteps[i]
                for update_fn in (corr_fn, pred_fn):
                    x, _ = update_fn(x, vec_t, model=model)
                    x, x_mean = reimpose(x, i, vec_t)
                if show_evolution:
                    evolution.append(x.cpu())
            info = {'evolution': torch.stack(evolution)} if show_evolution else {}
            return (x_mean if denoise else x), info

    return run


def shared_predictor_update_fn(x, t, sde, model, predictor, probability_flow, continuous):
    score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=continuous)
    obj = (NonePredictor if predictor is None else predictor)(sde, score_fn, probability_flow)
    return obj.update_fn(x, t)


def shared_corrector_update_fn(x, t, sde, model, corrector, continuous, snr, n_steps):
    score_fn = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=continuous)
    obj = (NoneCorrector if corrector is None else corrector)(sde, score_fn, snr, n_steps)
    return obj.update_fn(x, t)


def get_pc_sampler(sde, shape, predictor, corrector, snr, p_steps, c_steps, probability_flow=False,
                   continuous=False, denoise=True, eps=1e-3):
    pred_fn = functools.partial(shared_predictor_update_fn, sde=sde, predictor=predictor,
                                probability_flow=probability_flow, continuous=continuous)
    corr_fn = functools.partial(shared_corrector_update_fn, sde=sde, corrector=corrector, continuous=continuous,
                                snr=snr, n_steps=c_steps)

    def pc_sampler(model, show_evolution=False, noise_tape=None, seed=None, global_norm=None):
        steps = p_steps * (c_steps + 1)
        if fused.fusable(model, sde, predictor, corrector, c_steps, probability_flow, continuous):
            # the network's label: sigma(t) or log sigma(t) for the VE SDEs; VP / sub-VP take t*(N-1) whatever is passed here
            x, rec, ts = fused.run(model, sde, shape, None, p_steps, snr, eps, denoise, noise_tape=noise_tape, seed=seed,
                                   record=show_evolution, unconditional_label=fused.unconditional_label(model), global_norm=global_norm,
                                   predictor=predictor, corrector=corrector, probability_flow=probability_flow,
                                   continuous=continuous)
            info = {'times': ts, 'steps': steps}
            if show_evolution:
                info['evolution'] = rec.cpu()
            return x, info
        if noise_tape is not None:
            raise NotImplementedError('noise_tape is only available on the fused path')
        if global_norm is not None:       # (the step-by-step fallback would use per-shard norms: refuse instead; 'langevin_global' exists)
            raise NotImplementedError('global-norm sharded sampling runs on the fused device loop only; this (model, sde, predictor, '
                                      'corrector, c_steps) combination falls back to the step-by-step loop')
        with torch.no_grad():
            x = sde.prior_sampling(shape).to(model.device).type(torch.float32)
            timesteps = torch.linspace(sde.T, eps, p_steps, device=model.device)
            evolution = []
            x_mean = x
            for i in range(p_steps):
                vec_t = torch.ones(shape[0], device=model.device) * timesteps[i]
                x, x_mean = corr_fn(x, vec_t, model=model)
                x, x_mean = pred_fn(x, vec_t, model=model)
                if show_evolution:
                    evolution.append(x.cpu())
            info = {'times': timesteps, 'steps': steps}
            if show_evolution:
                info['evolution'] = torch.stack(evolution)
            return (x_mean if denoise else x), info

    return pc_sampler
