"""Score-matching losses with the reference's factories (losses.py:55-232): evaluation value and training loss.

``get_sde_loss_fn`` / ``get_general_sde_loss_fn`` return ``loss_fn(model, batch) -> scalar tensor`` with the reference's
argument meaning: per-sample ``t ~ U(eps, T)``, perturbation ``x_t = mean + std * z``, score evaluation, and the
(likelihood-)weighted denoising score-matching residual, reduced per sample (mean or 0.5*sum) and averaged over the
batch.  Every pixel-sized operation runs on the HIP kernels (perturbation: csd_scale_rows + csd_axpby; residual:
csd_scale_rows + csd_axpby; per-sample squared norms: csd_row_norms); the remaining arithmetic is on B scalars.

``train=False`` (the reference's eval step) evaluates the network on the planned graph executor and returns a plain value.
``train=True`` puts the model in training mode: the network runs on the differentiable HIP operators (grad_ops: forward and
backward kernels of csrc/backward.hip, dropout on), the residual / per-sample reduction are differentiable HIP operators too,
and the returned scalar is autograd-connected - ``loss.backward()`` fills ``param.grad`` of every network parameter
(SURVEY.md 8 rows a19/a20).  The last reduction over the B per-sample values is torch arithmetic on a [B] tensor.

``fused=True`` on either factory (opt-in; ``config.training.csd_fused_loss`` for the Trainer) returns
``loss_fn(model, batch, noise=None, t=None, seed=None)``: the same objective as csd_dsm_perturb -> the planned network ->
csd_dsm_residual, with Philox noise keyed by (seed, forward call index) instead of torch's generator (see the fused route below).
"""
import torch

from . import grad_ops, ops, sde_lib
from .models import utils as mutils
from .optim import get_optimizer, optimization_manager  # noqa: F401  (losses.py:26-53: same names, same module as the reference)


def _bstd(sde, ref, t):
    """(mean-scale, std) of p_t(x|x0) as [B] fp32 host tensors: every SDE of sde_lib has mean = m(t)*x0."""
    t = t.detach().cpu().float()
    mean, std = sde.marginal_prob(torch.ones(t.shape[0], 1, 1, 1), t)
    return mean.flatten(), std.flatten().float()


def _perturb(x, z, m, std):
    """x_t = m_b * x + std_b * z on the device."""
    dev = x.device
    xm = x if bool(torch.all(m == 1)) else ops.scale_rows(x, m.to(dev))
    return ops.axpby(xm, ops.scale_rows(z, std.to(dev)))


def _residual_sumsq(score, z, std, weighting):
    """per-sample sum of squares of (score*std + z) [weighting False] or (score + z/std) [True] -> [B] host tensor."""
    dev = score.device
    if score.requires_grad:            # training: differentiable operators, [B] device tensor
        if weighting:
            d = grad_ops.axpby(score, ops.scale_rows(z, std.to(dev), divide=True))
        else:
            d = grad_ops.axpby(grad_ops.scale_rows(score, std.to(dev)), z)
        return grad_ops.sumsq_rows(d)
    if weighting:
        d = ops.axpby(score, ops.scale_rows(z, std.to(dev), divide=True))
    else:
        d = ops.axpby(ops.scale_rows(score, std.to(dev)), z)
    n = ops.row_norms(d).cpu().double()
    return n * n


def _reduce(sumsq, numel, reduce_mean):
    return sumsq / numel if reduce_mean else 0.5 * sumsq


def _g2(sde, t):
    t = t.detach().cpu().float()
    return (sde.sde(torch.zeros(t.shape[0], 1, 1, 1), t)[1].flatten().double()) ** 2


def get_sde_loss_fn(sde, train, reduce_mean=True, continuous=True, likelihood_weighting=True, eps=1e-5, fused=False, seed=None):
    """losses.py:55-97 (unconditional).  ``fused=True``: the fused route (``_fused_loss_fn`` below), ``seed`` its default Philox key."""
    if fused:
        return _fused_loss_fn(sde, train, False, reduce_mean, continuous, likelihood_weighting, eps, seed)

    def loss_fn(model, batch):
        score_fn = mutils.get_score_fn(sde, model, train=train, continuous=continuous)
        t = torch.rand(batch.shape[0]) * (sde.T - eps) + eps
        z = torch.randn_like(batch)
        m, std = _bstd(sde, batch, t)
        score = score_fn(_perturb(batch, z, m, std), t.to(batch.device))
        per = batch[0].numel()
        losses = _reduce(_residual_sumsq(score, z, std, likelihood_weighting), per, reduce_mean)
        if likelihood_weighting:
            losses = losses * _g2(sde, t).to(losses)
        return losses.mean().float()

    return loss_fn


def get_general_sde_loss_fn(sde, train, conditional=False, reduce_mean=True, continuous=True, likelihood_weighting=True,
                            eps=1e-5, fused=False, seed=None):
    """losses.py:99-232: unconditional, SR3 (one conditional SDE, clean y) and the two-SDE CMDE / VS-CMDE branch.
    ``fused=True``: the fused route (``_fused_loss_fn`` below), ``seed`` its default Philox key."""
    if not conditional:
        return get_sde_loss_fn(sde, train, reduce_mean, continuous, likelihood_weighting, eps, fused, seed)
    if isinstance(sde, dict):
        if len(sde) != 2:
            raise NotImplementedError('multi-speed losses with >= 3 SDEs (losses.py:148-183) are not provided')
        assert likelihood_weighting, 'For the variance reduction technique in inverse problems, we only support likelihood weighting for the time being.'
    if fused:
        return _fused_loss_fn(sde, train, True, reduce_mean, continuous, likelihood_weighting, eps, seed)
    if isinstance(sde, dict):

        def loss_fn(model, batch):
            y, x = batch
            score_fn = mutils.get_score_fn(sde, model, conditional=True, train=train, continuous=continuous)
            t = torch.rand(x.shape[0]) * (sde['x'].T - eps) + eps
            z_y = torch.randn_like(y)
            m_y, std_y = _bstd(sde['y'], y, t)
            z_x = torch.randn_like(x)
            m_x, std_x = _bstd(sde['x'], x, t)
            score = score_fn({'x': _perturb(x, z_x, m_x, std_x), 'y': _perturb(y, z_y, m_y, std_y)}, t.to(x.device))
            sx = _residual_sumsq(score['x'].contiguous(), z_x, std_x, True)
            sx = sx * _g2(sde['x'], t).to(sx)
            sy = _residual_sumsq(score['y'].contiguous(), z_y, std_y, True)
            sy = sy * _g2(sde['y'], t).to(sy)
            numel = x[0].numel() + y[0].numel()          # the reference concatenates both residuals before reducing
            return _reduce(sx + sy, numel, reduce_mean).mean().float()

        return loss_fn

    def loss_fn(model, batch):          # SR3 estimator (losses.py:185-205)
        y, x = batch
        score_fn = mutils.get_score_fn(sde, model, conditional=True, train=train, continuous=continuous)
        t = torch.rand(x.shape[0]) * (sde.T - eps) + eps
        z = torch.randn_like(x)
        m, std = _bstd(sde, x, t)
        score = score_fn({'x': _perturb(x, z, m, std), 'y': y}, t.to(x.device))
        losses = _reduce(_residual_sumsq(score, z, std, likelihood_weighting), x[0].numel(), reduce_mean)
        if likelihood_weighting:
            losses = losses * _g2(sde, t).to(losses)
        return losses.mean().float()

    return loss_fn


# ------------------------------------------------------------------------------------------------------------------
# fused route (``fused=True``): the objective as two HIP passes around the planned network (csrc/dsm_loss.hip)
#
# Every score function of models/utils.py is score = s_b * h with a per-sample factor, so every variant above is
#     loss = sum_b sum_segments w_b * sum_i (a_b * h[b, i] + b_b * z[b, i])^2
# over the x block (and, with two SDEs, the y block) of the network's flat per-sample output row.  The per-sample numbers are taken
# from the SAME functions the default route calls - the score function evaluated on a likelihood._Probe gives s_b and the labels,
# _bstd the perturbation's (m, std), _g2 the likelihood weight - and no formula is restated per SDE:
#     likelihood_weighting   a = s,        b = 1 / std,   w = g^2 * r / B
#     otherwise              a = s * std,  b = 1,         w = r / B            r = 1 / numel (reduce_mean) or 1 / 2
# They are written on the host and uploaded in ONE asynchronous copy per step; the step never waits for the device.
#
# Noise.  ``noise`` is an explicit tape in the order of the default route's randn_like calls ([z] or [z_y, z_x]).  Without one, z is
# never stored: csd_dsm_perturb and csd_dsm_residual both make element b * D + i of the Philox fill of (seed, stream) in registers.
# seed defaults to model.dropout_seed; with ``call`` the index the forward is about to take (model._train_calls + 1)
#     stream = 2^63 + 2 * call + k,   k = 0 for x, 1 for y            (eval mode: 2^63 + 2^62 + 2 * model._train_calls + k)
# The dropout masks of that forward use (seed, (call << 16) + j): below 2^63 for every call < 2^47, so the two families of
# (seed, stream) pairs are disjoint for every call, and distinct calls get distinct noise streams.  z is thus a function of
# (seed, call) alone: a run resumed from Trainer.state_dict() (which keeps _train_calls) repeats it without any torch RNG state.
# ------------------------------------------------------------------------------------------------------------------
_NOISE_STREAM = 1 << 63
_EVAL_STREAM = 1 << 62
# How keyed noise reaches the two passes: 'registers' (each pass makes its normals itself) or 'fill' (one csd_randn fill per segment,
# read by both).  The values are bitwise the same; 'registers' measured 12 % faster at the SR3-160 shape, B = 64 (tools/bench_train.py
# --fused-loss, profiles/train_fused_loss.json: noise_forms).
FUSED_NOISE_FORM = 'registers'


def _dsm_tables(sde, t, numels, embedding_type='positional', conditional=False, reduce_mean=True, continuous=True,
                likelihood_weighting=True):
    """Host side of the fused route: ``(labels [B] float32, {'x': {...}[, 'y': {...}]})`` with float64 ``a, b, w`` and the float32
    ``m, std`` of the perturbation per segment, at the per-sample times ``t``.  ``numels``: floats per sample of each segment
    ({'x': ..} or, with two SDEs, {'x': .., 'y': ..})."""
    import types
    from . import likelihood
    pair = isinstance(sde, dict)
    t = t.detach().cpu().float()
    B = t.shape[0]

    class _PairProbe(likelihood._Probe):
        def __call__(self, x, labels):
            self.labels = labels
            return {k: torch.ones_like(v) for k, v in x.items()}

    probe = (_PairProbe if pair else likelihood._Probe)(types.SimpleNamespace(embedding_type=embedding_type))
    one = torch.ones(B, 1, 1, 1)
    s = mutils.get_score_fn(sde, probe, conditional=conditional, train=False, continuous=continuous)(
        {'x': one, 'y': one.clone()} if conditional else one, t)
    total = sum(int(n) for n in numels.values())
    r = (1.0 / total if reduce_mean else 0.5) / B
    tables = {}
    for k in (('x', 'y') if pair else ('x',)):
        sde_k = sde[k] if pair else sde
        m, std = _bstd(sde_k, None, t)
        s_k = (s[k] if pair else s).reshape(B).double()
        if likelihood_weighting:
            a, b, w = s_k, 1.0 / std.double(), _g2(sde_k, t) * r
        else:
            a, b, w = s_k * std.double(), torch.ones(B, dtype=torch.float64), torch.full((B,), r, dtype=torch.float64)
        tables[k] = {'m': m.float(), 'std': std, 'a': a, 'b': b, 'w': w}
    return probe.labels.reshape(B).float(), tables


class _CoefficientUpload:
    """Pinned staging of a step's per-sample coefficients (the ode_solver.CoefficientRing pattern): the rows are written into a slot
    and leave in ONE asynchronous copy to a fresh device tensor.  A slot is rewritten 8 uploads later, after the event recorded behind
    its copy - long past by then, so the host does not wait."""
    SLOTS = 8

    def __init__(self):
        self.host, self.events, self.k = None, [None] * self.SLOTS, 0

    def __call__(self, rows, dev):
        B = rows[0].shape[0]
        n = len(rows) * B
        if self.host is None or self.host.shape[1] < n:
            self.host, self.events = torch.empty(self.SLOTS, n, dtype=torch.float32).pin_memory(), [None] * self.SLOTS
        if self.events[self.k] is not None:
            self.events[self.k].synchronize()
        slot = self.host[self.k, :n]
        for i, row in enumerate(rows):
            slot[i * B:(i + 1) * B].copy_(row)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        out.copy_(slot, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self.events[self.k] = ev
        self.k = (self.k + 1) % self.SLOTS
        return [out[i * B:(i + 1) * B] for i in range(len(rows))]


class _DsmResidual(torch.autograd.Function):
    """loss = sum_b sum_seg w sum (a h + b z)^2 as ONE node: the forward writes d loss / d h beside the value (csd_dsm_residual),
    the backward scales it by the incoming scalar (csd_scale_rows)."""

    @staticmethod
    def forward(ctx, out, segments, seed):
        loss, _, d_out = ops.dsm_residual(out, segments, seed)
        ctx.d_out = d_out
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d_out = ctx.d_out
        scale = g.detach().to(device=d_out.device, dtype=torch.float32).reshape(1).expand(d_out.shape[0]).contiguous()
        return ops.scale_rows(d_out, scale), None, None


def _require_fused(model, tensors, sde):
    from .models.ddpm import HipUNet
    if isinstance(sde, dict) and len(sde) != 2:
        raise NotImplementedError('the fused loss takes one SDE or the {x, y} pair, not %d SDEs' % len(sde))
    if getattr(model, 'arch', None) == 2 or model.__class__.__name__.startswith('DDPM3D'):
        if not getattr(model, 'planned_train', False):
            raise NotImplementedError('the fused loss is not provided for the 3-D classes (%s) without the planned training graph '
                                      '(planned_train=True, config.model.csd_planned_train or CSD_PLANNED_TRAIN=1)'
                                      % model.__class__.__name__)
    elif not (isinstance(model, HipUNet) and model.arch == 0 and model.train_executor == 'planned' and model.train_layout == 'nhwc'):
        raise NotImplementedError('the fused loss needs a HipUNet on the planned training executor (DDPM family, '
                                  'CSD_TRAIN_EXECUTOR=planned, CSD_TRAIN_LAYOUT=nhwc), got %s' % model.__class__.__name__)
    for name, v in tensors:
        if not (isinstance(v, torch.Tensor) and v.is_cuda):
            raise NotImplementedError('the fused loss runs on GPU tensors only: %s is on %s' % (name, getattr(v, 'device', type(v))))


def _fused_loss_fn(sde, train, conditional, reduce_mean, continuous, likelihood_weighting, eps, seed0):
    """``loss_fn(model, batch, noise=None, t=None, seed=None)``: the objectives above on csd_dsm_perturb -> the planned network ->
    csd_dsm_residual.  ``t``: per-sample times (default: the default route's torch.rand draw); ``noise``: the tape; ``seed``: the
    Philox key (default: the factory's ``seed``, else model.dropout_seed).  Training mode returns an autograd-connected device scalar
    behind the unchanged ``_PlannedNet`` node; eval mode runs the planned inference forward and writes no gradient."""
    pair = isinstance(sde, dict)
    if pair and len(sde) != 2:
        raise NotImplementedError('the fused loss takes one SDE or the {x, y} pair, not %d SDEs' % len(sde))
    upload = _CoefficientUpload()

    def loss_fn(model, batch, noise=None, t=None, seed=None):
        y, x = batch if conditional else (None, batch)
        _require_fused(model, [('x', x)] + ([('y', y)] if conditional else []), sde)
        B, dev = x.shape[0], x.device
        if t is None:
            t = torch.rand(B) * ((sde['x'] if pair else sde).T - eps) + eps
        numels = {'x': x[0].numel(), 'y': y[0].numel()} if pair else {'x': x[0].numel()}
        labels, tab = _dsm_tables(sde, t, numels, getattr(model, 'embedding_type', 'positional'), conditional, reduce_mean,
                                  continuous, likelihood_weighting)
        keys = ('x', 'y') if pair else ('x',)
        rows = upload([labels] + [tab[k][c] for k in keys for c in ('m', 'std', 'a', 'b', 'w')], dev)
        labels_d, coef = rows[0], {k: dict(zip(('m', 'std', 'a', 'b', 'w'), rows[1 + 5 * i:6 + 5 * i])) for i, k in enumerate(keys)}
        if seed is None:
            seed = seed0 if seed0 is not None else model.dropout_seed
        base = _NOISE_STREAM + 2 * (model._train_calls + 1) if train else _NOISE_STREAM + _EVAL_STREAM + 2 * model._train_calls
        stream = {'x': base, 'y': base + 1}
        z = {}
        if noise is not None:
            tape = [noise] if isinstance(noise, torch.Tensor) else list(noise)
            if len(tape) != len(keys):
                raise ValueError('the noise tape holds %d tensors, this objective draws %d' % (len(tape), len(keys)))
            z = dict(zip(('y', 'x') if pair else ('x',), [v.to(device=dev, dtype=torch.float32).contiguous() for v in tape]))
        elif FUSED_NOISE_FORM == 'fill':
            z = {k: ops.randn(tuple(v.shape), seed, stream[k], dev) for k, v in (('x', x), ('y', y)) if k in keys}
        data = {'x': x, 'y': y}
        pert = {k: ops.dsm_perturb(data[k], coef[k]['std'], None if bool(torch.all(tab[k]['m'] == 1)) else coef[k]['m'], z.get(k),
                                   seed, stream[k]) for k in keys}
        model.train() if train else model.eval()
        if train:
            out = model._run(pert['x'], pert['y'] if pair else y, labels_d)
        else:
            with torch.no_grad():
                out = model._run(pert['x'], pert['y'] if pair else y, labels_d)
        segments, off = [], 0
        for k in keys:
            n = numels[k]
            segments.append({'offset': off, 'length': n, 'a': coef[k]['a'], 'b': coef[k]['b'], 'w': coef[k]['w'],
                             'z': z.get(k), 'stream_id': stream[k]})
            off += n
        if out.requires_grad:
            return _DsmResidual.apply(out, segments, seed)
        return ops.dsm_residual(out, segments, seed, want_d_out=False)[0].reshape(())

    return loss_fn


# ------------------------------------------------------------------------------------------------------------------
# discrete-time ("legacy") objectives and the one-step function - losses.py:236-407
# ------------------------------------------------------------------------------------------------------------------
def _diff_sumsq(a, b):
    """per-sample sum of squares of (a - b): differentiable in ``a`` when it carries a graph"""
    if a.requires_grad:
        return grad_ops.sumsq_rows(grad_ops.axpby(a, b, 1.0, -1.0))
    n = ops.row_norms(ops.axpby(a, b, 1.0, -1.0)).cpu().double()
    return n * n


def get_smld_loss_fn(vesde, train, reduce_mean=False, likelihood_weighting=False):
    """losses.py:236-265 (SMLD / NCSN objective on the discrete sigma ladder).  (score + z/sigma)^2 sigma^2 = (score sigma + z)^2:
    both weightings of the reference reduce to the same per-sample value."""
    assert isinstance(vesde, sde_lib.VESDE), "SMLD training only works for VESDEs."

    def loss_fn(model, batch):
        score_fn = mutils.get_score_fn(vesde, model, train=train)
        labels = torch.randint(0, vesde.N, (batch.shape[0],))
        sigmas = vesde.discrete_sigmas[labels].float()
        z = torch.randn_like(batch)
        perturbed = ops.axpby(batch, ops.scale_rows(z, sigmas.to(batch.device)))
        score = score_fn(perturbed, (labels / (vesde.N - 1)).to(batch.device))
        losses = _reduce(_residual_sumsq(score, z, sigmas, False), batch[0].numel(), reduce_mean)
        return losses.mean().float()

    return loss_fn


def get_inverse_problem_smld_loss_fn(sde, train, reduce_mean=False, likelihood_weighting=True):
    """losses.py:267-318: SMLD objective for the {'x', 'y'} pair of VE SDEs on a shared label."""
    def loss_fn(model, batch):
        y, x = batch
        score_fn = mutils.get_score_fn(sde, model, train=train)
        labels = torch.randint(0, sde['x'].N, (x.shape[0],))
        sig_y, sig_x = sde['y'].discrete_sigmas[labels].float(), sde['x'].discrete_sigmas[labels].float()
        z_y = torch.randn_like(y)
        z_x = torch.randn_like(x)
        pert = {'x': ops.axpby(x, ops.scale_rows(z_x, sig_x.to(x.device))), 'y': ops.axpby(y, ops.scale_rows(z_y, sig_y.to(y.device)))}
        score = score_fn(pert, (labels / (sde['x'].N - 1)).to(x.device))
        numel = x[0].numel() + y[0].numel()
        if likelihood_weighting:      # (s + z/sigma)^2 sigma^2 per domain, concatenated, reduced
            sx = _residual_sumsq(score['x'].contiguous(), z_x, sig_x, False)
            sy = _residual_sumsq(score['y'].contiguous(), z_y, sig_y, False)
            return _reduce(sx + sy, numel, reduce_mean).mean().float()
        sx = _residual_sumsq(score['x'].contiguous(), z_x, sig_x, True)      # (s + z/sigma)^2
        sy = _residual_sumsq(score['y'].contiguous(), z_y, sig_y, True)
        w = (sig_x.double() ** 2 * sig_y.double() ** 2) / (sig_x.double() ** 2 + sig_y.double() ** 2)
        tot = sx + sy
        return (_reduce(tot, numel, reduce_mean) * w.to(tot)).mean().float()

    return loss_fn


def get_ddpm_loss_fn(vpsde, train, reduce_mean=True):
    """losses.py:320-340 (DDPM noise-prediction objective)."""
    assert isinstance(vpsde, sde_lib.VPSDE), "DDPM training only works for VPSDEs."

    def loss_fn(model, batch):
        model_fn = mutils.get_model_fn(model, train=train)
        labels = torch.randint(0, vpsde.N, (batch.shape[0],))
        a = vpsde.sqrt_alphas_cumprod[labels].float()
        b = vpsde.sqrt_1m_alphas_cumprod[labels].float()
        z = torch.randn_like(batch)
        perturbed = ops.axpby(ops.scale_rows(batch, a.to(batch.device)), ops.scale_rows(z, b.to(batch.device)))
        out = model_fn(perturbed, labels.to(batch.device))
        return _reduce(_diff_sumsq(out, z), batch[0].numel(), reduce_mean).mean().float()

    return loss_fn


def get_inverse_problem_ddpm_loss_fn(vpsdes, train, reduce_mean=True):
    """losses.py:342-343: not implemented upstream either (the reference returns the NotImplementedError class)."""
    raise NotImplementedError('discrete DDPM training of inverse problems is not implemented in the reference')


def get_step_fn(sde, train, optimize_fn=None, reduce_mean=False, continuous=True, likelihood_weighting=False):
    """losses.py:345-407: ``step_fn(state, batch) -> loss`` with state = {'model', 'optimizer', 'ema', 'step'}."""
    if continuous:
        loss_fn = get_sde_loss_fn(sde, train, reduce_mean=reduce_mean, continuous=True, likelihood_weighting=likelihood_weighting)
    elif isinstance(sde, dict):
        if isinstance(sde['y'], sde_lib.VESDE) and isinstance(sde['x'], sde_lib.cVESDE) and len(sde) == 2:
            loss_fn = get_inverse_problem_smld_loss_fn(sde, train, reduce_mean=reduce_mean, likelihood_weighting=likelihood_weighting)
        else:
            raise NotImplementedError('This combination of sdes is not supported for discrete training yet.')
    elif isinstance(sde, sde_lib.VESDE):
        loss_fn = get_smld_loss_fn(sde, train, reduce_mean=reduce_mean)
    elif isinstance(sde, sde_lib.VPSDE):
        loss_fn = get_ddpm_loss_fn(sde, train, reduce_mean=reduce_mean)
    else:
        raise ValueError(f"Discrete training for {sde.__class__.__name__} is not recommended.")

    def step_fn(state, batch):
        model = state['model']
        if train:
            optimizer = state['optimizer']
            optimizer.zero_grad()
            loss = loss_fn(model, batch)
            loss.backward()
            optimize_fn(optimizer, model.parameters(), step=state['step'])
            state['step'] += 1
            state['ema'].update(model.parameters())
        else:
            with torch.no_grad():
                ema = state['ema']
                ema.store(model.parameters())
                ema.copy_to(model.parameters())
                loss = loss_fn(model, batch)
                ema.restore(model.parameters())
        return loss

    return step_fn
