"""Host driver of the fused device-resident PC loop (csd_pc_sample).

Computes the per-step scalars on the CPU in fp32 with the SAME torch expressions the reference
evaluates per step (timesteps: sampling/conditional.py:202; labels: models/utils.py:198,213,234; sigma(t):
sde_lib.py:390-395; G_i: sde_lib.py:410-418; the VP / sub-VP std, drift and G: sde_lib.py:49-63,170-195,268-287),
then launches ONE library call that runs the whole
loop on the device: 2 network evaluations + 2 update kernels per step, no per-step Python objects,
no host synchronisation.
"""
import ctypes

import torch

from .. import _lib, ops, sde_lib
from .._lib import check, current_stream, lib, ptr


def _rule_ids(predictor, corrector):
    """(predictor id, corrector id) of csd_pc_params, or None for classes the device loop does not implement.
    0 = the reverse-diffusion / Langevin pair, 1 = an affine rule with a per-step coefficient table, 2 = none."""
    from . import correctors as C, predictors as P
    if predictor in (P.ReverseDiffusionPredictor, P.conditionalReverseDiffusionPredictor):
        pid = 0
    elif predictor in (P.EulerMaruyamaPredictor, P.conditionalEulerMaruyamaPredictor, P.AncestralSamplingPredictor,
                       P.conditionalAncestralSamplingPredictor):
        pid = 1
    elif predictor in (P.NonePredictor, P.conditionalNonePredictor):
        pid = 2
    else:
        return None
    if corrector in (C.LangevinCorrector, C.conditionalLangevinCorrector):
        cid = 0
    elif corrector in (C.AnnealedLangevinDynamics, C.conditionalAnnealedLangevinDynamics):
        cid = 1
    elif corrector in (C.NoneCorrector, C.conditionalNoneCorrector):
        cid = 2
    else:
        return None
    return pid, cid


_VE = (sde_lib.VESDE, sde_lib.cVESDE)
_VP = (sde_lib.VPSDE, sde_lib.cVPSDE)             # (the classes with the DDPM tables: discrete_betas, alphas, ...)
_VP_FAMILY = _VP + (sde_lib.subVPSDE,)


def fusable(model, sde, predictor, corrector, c_steps, probability_flow, continuous, use_path=False):
    """True when (model, sde, predictor, corrector) runs on the fused device loop: a VE SDE (or the two-SDE VE pair), a VPSDE, cVPSDE
    or subVPSDE with any registered predictor (reverse diffusion, Euler-Maruyama, ancestral sampling, none) and corrector (Langevin,
    annealed Langevin dynamics, none) that the SDE's class supports in the step-by-step classes.  The model is a HipUNet or a planned
    3-D network (models/ddpm3d.py with ``csd_planned``): both own a csd_unet handle that the loop evaluates."""
    from ..models.ddpm import HipUNet
    from ..models.ddpm3d import DDPM3D
    from . import predictors as P
    c_sde = sde['x'] if isinstance(sde, dict) else sde
    if isinstance(sde, dict):                   # the two-SDE setting: VE members only (models/utils.py:171-188 refuses the others)
        ok_sde = isinstance(c_sde, _VE) and isinstance(sde.get('y'), sde_lib.VESDE) and len(sde) == 2
    else:
        ok_sde = isinstance(c_sde, _VE + _VP_FAMILY)
    ids = _rule_ids(predictor, corrector)
    if ids is None or ids == (2, 2):
        return False
    ancestral = predictor in (P.AncestralSamplingPredictor, P.conditionalAncestralSamplingPredictor)
    # the probability flow: reverse diffusion and Euler-Maruyama (ancestral sampling refuses it)
    ok_pf = (not probability_flow) or (ids[0] != 2 and not ancestral)
    if isinstance(c_sde, sde_lib.subVPSDE):
        # no DDPM tables: the Langevin / ALD step size (alphas[timestep]) and ancestral sampling (discrete_betas) raise for it
        ok_sde = ok_sde and ids[1] == 2 and not ancestral
    # discrete-time score functions: the VP classes index sqrt_1m_alphas_cumprod with the truncated label; the VE ones are not provided
    ok_time = continuous or isinstance(c_sde, _VP_FAMILY)
    # use_path (the bridge for y_t): two-SDE setting only
    ok_path = (not use_path) or isinstance(sde, dict)
    ok_model = isinstance(model, HipUNet) or (isinstance(model, DDPM3D) and model.planned)
    return (ok_model and ok_sde and c_steps == 1 and ok_pf and ok_time and ok_path)


def _index(c_sde, t1):
    return int((t1 * (c_sde.N - 1) / c_sde.T).long()[0])


def rule_tables(c_sde, ts, predictor, corrector, snr, probability_flow):
    """Per-step (p, a, b) tables of the affine rules, evaluated exactly like the per-step classes evaluate their scalars
    (sampling/predictors.py: _euler_maruyama, _ancestral; sampling/correctors.py: _ald): fp32 SDE quantities, python-float
    arithmetic, one rounding to fp32 at the library boundary."""
    from . import predictors as P
    pid, cid = _rule_ids(predictor, corrector)
    n = ts.numel()
    pred = corr = None
    if pid == 1:
        pred = torch.empty(n, 3, dtype=torch.float32)
        for i in range(n):
            t1 = ts[i:i + 1].to(torch.float32)
            if predictor in (P.EulerMaruyamaPredictor, P.conditionalEulerMaruyamaPredictor):
                drift, diffusion = c_sde.sde(torch.ones(1, 1, 1, 1), t1)
                phi, g = float(drift.flatten()[0]), float(diffusion.flatten()[0])
                dt = -1.0 / c_sde.N
                kappa = 0.5 if probability_flow else 1.0
                co = (1.0 + phi * dt, -kappa * g * g * dt, 0.0 if probability_flow else g * (-dt) ** 0.5)
            elif isinstance(c_sde, _VP):
                beta = float(c_sde.discrete_betas.to(torch.float32)[_index(c_sde, t1)])
                r = (1.0 - beta) ** 0.5
                co = (1.0 / r, beta / r, beta ** 0.5)
            else:
                k = int((t1 * (c_sde.N - 1) / c_sde.T).long()[0])
                sig = c_sde.discrete_sigmas.to(torch.float32)
                s2 = float(sig[k]) ** 2
                a2 = float(sig[k - 1]) ** 2 if k > 0 else 0.0
                co = (1.0, s2 - a2, (a2 * (s2 - a2) / s2) ** 0.5)
            pred[i] = torch.tensor(co, dtype=torch.float64).to(torch.float32)
    if cid == 1:
        corr = torch.empty(n, 3, dtype=torch.float32)
        for i in range(n):
            t1 = ts[i:i + 1].to(torch.float32)
            std = float(c_sde.marginal_prob(torch.zeros(1, 1, 1, 1), t1)[1].flatten()[0])
            alpha = float(c_sde.alphas.to(torch.float32)[_index(c_sde, t1)]) if isinstance(c_sde, _VP_FAMILY) else 1.0
            step = (snr * std) ** 2 * 2 * alpha
            corr[i] = torch.tensor((1.0, step, (2 * step) ** 0.5), dtype=torch.float64).to(torch.float32)
    return pid, cid, pred, corr


def reverse_diffusion_table(c_sde, ts):
    """(rd_drift [n][2] fp32 or None, rd_sub_x) of csd_pc_params: the reverse-diffusion predictor's forward drift per step, from the
    same host evaluation the per-step class makes (sampling/predictors.py:reverse_diffusion_drift); None for the VE SDEs (f = 0)."""
    from .predictors import reverse_diffusion_drift
    rows = [reverse_diffusion_drift(c_sde, ts[i:i + 1].to(torch.float32)) for i in range(ts.numel())]
    if rows[0] is None:
        return None, 0
    tab = torch.tensor([r[:2] for r in rows], dtype=torch.float64).to(torch.float32).contiguous()
    return tab, int(rows[0][2])


def langevin_alphas(c_sde, ts):
    """corr_alpha of csd_pc_params: alphas[timestep_i] (sampling/correctors.py:63-65,94-96) for the VP classes, None (= 1) for VE;
    subVPSDE has no ``alphas`` and raises AttributeError as the per-step corrector (and the reference) does."""
    if not isinstance(c_sde, _VP_FAMILY):
        return None
    return torch.stack([c_sde.alphas[_index(c_sde, ts[i:i + 1])] for i in range(ts.numel())]).to(torch.float32).contiguous()


def step_scalars(sde, p_steps, eps, unconditional_label=None, continuous=True):
    """fp32 per-step arrays (labels, std_x, G, std_y|None) + the timesteps tensor."""
    c_sde = sde['x'] if isinstance(sde, dict) else sde
    ts = torch.linspace(c_sde.T, eps, p_steps)
    if isinstance(c_sde, _VP_FAMILY):
        # one evaluation per step at a one-element time, like the per-step classes (models/utils.py:get_score_fn, predictors.py);
        # the label is t*(N-1), unrounded, for the conditional and the unconditional score function alike
        labels = (ts * (c_sde.N - 1)).float()
        std_x, G = torch.empty(p_steps), torch.empty(p_steps)
        for i in range(p_steps):
            t1 = ts[i:i + 1]
            if continuous or isinstance(c_sde, sde_lib.subVPSDE):
                std_x[i] = c_sde.marginal_prob(torch.zeros(1, 1), t1)[1][0]        # (sub-VP: 1 - exp(2*lmc), no square root)
            else:
                std_x[i] = c_sde.sqrt_1m_alphas_cumprod.type_as(labels)[labels[i:i + 1].long()][0]
            G[i] = c_sde.discretize(torch.zeros(1, 1), t1)[1][0]
        return ts, labels.contiguous(), std_x, G, None
    dummy = torch.zeros(p_steps, 1)
    std_x = c_sde.marginal_prob(dummy, ts)[1].float()
    G = c_sde.discretize(dummy, ts)[1].float()
    if unconditional_label is None:
        labels = (ts * (c_sde.N - 1)).float()
    else:   # unconditional continuous VE: the network sees sigma(t) or log sigma(t) (models/utils.py:246-253)
        labels = torch.log(std_x) if unconditional_label == 'fourier' else std_x.clone()
    std_y = sde['y'].marginal_prob(dummy, ts)[1].float() if isinstance(sde, dict) else None
    return ts, labels.contiguous(), std_x.contiguous(), G.contiguous(), (std_y.contiguous() if std_y is not None else None)


def inpaint_tables(sde, ts):
    """(mean_scale, std) of csd_pc_inpaint_params, [n] fp32 each: p_t(x | data) = N(mean_scale*data, std^2) per step, from one
    ``sde.marginal_prob`` evaluation at a one-element time like ``step_scalars`` (sampling/unconditional.py:268 evaluates it on the
    data at the step's time).  The marginal std in discrete time as well: the inpainter perturbs the data with the SDE's marginal,
    whatever std the score function divides by.  mean_scale is exactly 1 for the VE SDEs."""
    n = ts.numel()
    mean_scale, std = torch.empty(n, dtype=torch.float32), torch.empty(n, dtype=torch.float32)
    one = torch.ones(1, 1, 1, 1)
    for i in range(n):
        m, sd = sde.marginal_prob(one, ts[i:i + 1].to(torch.float32))
        mean_scale[i], std[i] = m.flatten()[0], sd.flatten()[0]
    return mean_scale.contiguous(), std.contiguous()


DRAW_KINDS = ('z_y0', 'z_y', 'zy', 'z', 'z_blend', 'z_colorize')      # csd_pc_noise_draws (include/csd.h): kind ids
DRAW_PHASES = ('corrector', 'predictor', 'none')        # ... and phase ids


def noise_draws(handle, B, predictor, corrector, std_y=False, use_path=False, inpaint=False, n_steps=1, colorize=False):
    """The draws behind the prior of a fused loop, in the order it consumes them, as the library lists them (csd_pc_noise_draws; no
    GPU): rows ``(step, kind, phase, elems, tape_offset, philox_stream)`` with step -1 in front of the loop, kind / phase indexing
    DRAW_KINDS / DRAW_PHASES.  ``predictor`` / ``corrector``: the rule ids of csd_pc_params.  ``colorize``: the schedule of a
    csd_pc_colorize_* call (the library's ``inpaint`` argument is then 2).  A combination the loop refuses raises RuntimeError with the
    library's message."""
    if inpaint and colorize:
        raise NotImplementedError('inpaint and colorize exclude each other: one re-imposition per loop')
    return _noise_draws(handle, B, predictor, corrector, std_y, use_path, 2 if colorize else int(bool(inpaint)), n_steps)


def _noise_draws(handle, B, predictor, corrector, std_y, use_path, blend, n_steps):
    """``noise_draws`` with the library's own ``inpaint`` integer: 0 none, 1 inpainting, 2 colorization (``_Constraint.draws``)"""
    args = (handle, int(B), int(predictor), int(corrector), int(bool(std_y)), int(bool(use_path)), int(blend), int(n_steps))
    n = lib().csd_pc_noise_draws(*args, None, 0)
    if n < 0:
        check(int(n), 'pc_noise_draws')
    rows = (ctypes.c_int64 * (6 * n))()
    lib().csd_pc_noise_draws(*args, rows, n)
    return [tuple(rows[6 * k:6 * k + 6]) for k in range(n)]


def check_tape(draws, tape, nx, ny):
    """``tape``: the tensors after the prior; ``draws``: the rows of ``noise_draws``.  The loop finds each draw by the sizes of the ones
    before it, so the tape must hold that many draws and that many elements."""
    if len(tape) != len(draws):
        raise RuntimeError('noise tape holds %d draws after the prior, the loop needs %d' % (len(tape), len(draws)))
    have, floats = sum(int(t.numel()) for t in tape), sum(r[3] for r in draws)
    if have != floats:
        raise RuntimeError('noise tape holds %d elements after the prior, the loop needs %d (x draws of %d, y draws of %d)'
                           % (have, floats, nx, ny))


def inpaint_tape_length(p_steps, has_corrector, has_predictor):
    """draws of an inpainting run in the order of the step-by-step inpainter's randn_like calls: the prior, then per step
    [z_corrector] z_blend [z_predictor] z_blend - a 'none' phase draws no update noise but its blend does draw"""
    return 1 + (int(bool(has_corrector)) + int(bool(has_predictor)) + 2) * p_steps


def _fp(t):
    return t.data_ptr() and ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def fresh_seed():
    """A Philox key drawn from torch's global CPU generator: successive calls get different noise (as the reference's
    torch.randn calls do, sampling/conditional.py:198) and torch.manual_seed still makes a run reproducible."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def path_tables(sy, ts):
    """use_path: per-step bridge coefficients (w0, w1, std) of p(y_t | y_0, y_{t+tau}) and sigma_y(T + tau), evaluated in fp32 with the
    torch expressions of sde_lib.compute_backward_kernel / marginal_prob (sampling/conditional.py:143-160)"""
    tau = ts[0] - ts[1] if len(ts) > 1 else ts[0] * 0
    one, zero = torch.ones(1, 1, 1, 1), torch.zeros(1, 1, 1, 1)
    std0 = float(sy.marginal_prob(zero, (ts[0] + tau).reshape(1))[1].flatten()[0])
    rows = []
    for i in range(len(ts)):
        t1 = ts[i].reshape(1)
        m0, sd = sy.compute_backward_kernel(one, zero, t1, tau.reshape(1))
        m1, _ = sy.compute_backward_kernel(zero, one, t1, tau.reshape(1))
        rows.append([float(m0.flatten()[0]), float(m1.flatten()[0]), float(sd.flatten()[0])])
    return torch.tensor(rows, dtype=torch.float32).contiguous(), std0


def unconditional_label(model):
    """the ``unconditional_label`` of an unconditional run on ``model``: the network sees log sigma(t) behind a Fourier embedding and
    sigma(t) otherwise (the VE SDEs; VP / sub-VP take t*(N-1) whatever is passed)"""
    return 'fourier' if getattr(model, 'embedding_type', 'positional') == 'fourier' else 'sigma'


class _Constraint:
    """What one loop re-imposes behind every phase, as ``prepare`` resolves ``inpaint=`` / ``colorize=``: everything that differs
    between the constrained entry families.  A kind sets ``family`` (its entries are csd_<family>_sample / _step_begin / _step_end),
    ``noun`` (what its refusals call it) and ``draws`` (the ``inpaint`` integer of csd_pc_noise_draws), checks its own argument
    against the state's shape (``check_shape``), fills its ctypes ``struct`` and the tensors ``keep`` that the struct points into
    (``fill``) and turns the prior into the initial state (``start``).  ``scratch_bytes`` names the entry that sizes the loop's scratch:
    the plain one unless the family exports its own.  The constructor makes every refusal, on the host."""
    scratch_bytes = 'csd_pc_scratch_bytes'

    def __init__(self, arg, model, shape, y, sde, use_path):
        who = (self.noun, self.family)
        if len(shape) == 5:
            raise NotImplementedError('%s on the device loop is not provided for the 3-D networks (csd_%s_* refuse them)' % who)
        if getattr(model, 'y_scale', 0):
            raise NotImplementedError('%s on the device loop is not provided for %s (the Kx super-resolution networks, ddpm_KxSR / '
                                      'ncsnpp_KxSR, are conditional; csd_%s_* refuse y_scale)' % (who[0], type(model).__name__, who[1]))
        if y is not None or isinstance(sde, dict) or use_path:
            raise NotImplementedError('%s on the device loop runs unconditional networks on a single SDE' % who[0])
        self.check_shape(arg, tuple(shape))
        self.arg = arg


class _Inpaint(_Constraint):
    """``inpaint=(data, mask)``: the known pixels (csd_pc_inpaint_params).  ``blend=False``: the initial state stays the bare prior"""
    family, noun, draws, blend = 'pc_inpaint', 'inpainting', 1, True
    scratch_bytes = 'csd_pc_inpaint_scratch_bytes'

    def check_shape(self, arg, shape):
        if tuple(arg[0].shape) != shape:
            raise ValueError('inpaint: data has shape %s, the sampler runs %s' % (tuple(arg[0].shape), shape))

    def fill(self, dev, c_sde, ts):
        data, mask = self.arg
        self.data = data.to(dev, torch.float32).contiguous()
        self.mask = mask.to(dev, torch.float32).expand_as(self.data).contiguous()
        mean, std = inpaint_tables(c_sde, ts)
        self.struct = _lib.PCInpaintParams()
        self.struct.data, self.struct.mask = self.data.data_ptr(), self.mask.data_ptr()
        self.struct.mean_scale, self.struct.std = _fp(mean), _fp(std)
        self.keep = (mean, std, self.data, self.mask)

    def start(self, x, record):
        if self.blend:
            ops.inpaint_blend(x, self.data, self.mask, x_mean=False)      # prior*(1 - mask) + data*mask
        elif record:
            raise NotImplementedError('record needs the initial state, which blend=False leaves to the caller')


class _Colorize(_Constraint):
    """``colorize=gray``: the gray channel of the decoupled channel space (csd_pc_colorize_params)"""
    family, noun, draws = 'pc_colorize', 'colorization', 2

    def check_shape(self, gray, shape):
        if tuple(gray.shape) != shape or len(shape) != 4 or shape[1] != 3:
            raise ValueError('colorize: the gray-scale image has shape %s, the sampler runs %s; colorization needs [B, 3, H, W]'
                             % (tuple(gray.shape), shape))

    def fill(self, dev, c_sde, ts):
        self.gray0 = ops.colorize_gray0(self.arg.to(dev, torch.float32).contiguous())      # once per call
        mean, std = inpaint_tables(c_sde, ts)
        self.struct = _lib.PCColorizeParams()
        self.struct.gray0 = self.gray0.data_ptr()
        self.struct.mean_scale, self.struct.std = _fp(mean), _fp(std)                 # (matrix / inv_matrix NULL: the library's default)
        self.keep = (mean, std, self.gray0)

    def start(self, x, record):
        ops.colorize_start(x, self.gray0)               # couple(decouple(gray)*mask + decouple(prior*(1 - mask)))


def _resolve(inpaint, colorize, blend, *run):
    """the ``_Constraint`` of ``prepare``'s ``inpaint=`` / ``colorize=`` (None: neither); ``run``: what the refusals look at"""
    if inpaint is not None and colorize is not None:
        raise NotImplementedError('inpaint= and colorize= exclude each other: the device loop re-imposes one constraint per run')
    if inpaint is not None:
        con = _Inpaint(inpaint, *run)
        con.blend = blend
        return con
    return _Colorize(colorize, *run) if colorize is not None else None


class Prepared:
    """One fused loop ready to be enqueued (``prepare``): the state ``x`` (prior in, result out), the condition ``y``, the filled
    csd_pc_params ``p``, the ``constraint`` (a ``_Constraint`` with its filled ``struct``; None: a plain run), the record tensor
    ``rec`` and the timesteps ``ts``.  ``keep`` holds every host array and device tensor the two structs point into: the object must
    stay alive until the library call that reads them has returned."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def prepare(model, sde, shape, y, p_steps, snr, eps, denoise, noise_tape=None, seed=None, record=False,
            unconditional_label=None, global_norm=None, predictor=None, corrector=None, probability_flow=False, use_path=False,
            corr_alpha=None, continuous=True, inpaint=None, blend=True, colorize=None):
    """Everything ``run`` does before it calls the library - argument checks, per-step tables, prior, tape, record buffer, the two
    parameter structs - as a ``Prepared``; ``run`` is ``launch(prepare(...))``.  sampling/cascade.py prepares every stage this way and
    hands them to ONE csd_pc_cascade_sample.  ``blend=False`` (inpainting): the initial state stays the bare prior and ``data`` is
    used as it is - the cascade's link writes the data and blends on the device."""
    if seed is None:
        seed = fresh_seed()
    con = _resolve(inpaint, colorize, blend, model, shape, y, sde, use_path)      # (every refusal of a constraint: host only)
    c_sde = sde['x'] if isinstance(sde, dict) else sde
    dev = model.device
    if dev.type != 'cuda':
        raise RuntimeError('the fused PC sampler runs on the MI355X only (model is on %s)' % dev)
    B = shape[0]
    if y is not None and getattr(model, 'y_scale', 0) and tuple(y.shape) != model._y_shape(B):
        # (with seed= nothing else looks at y: a full-resolution y would be read as the first y_channels (S / K)^2 floats of each sample)
        raise RuntimeError('y has shape %s, %s takes the low-resolution %s' % (tuple(y.shape), type(model).__name__, model._y_shape(B)))
    ve = isinstance(c_sde, _VE)
    if not ve and isinstance(sde, dict):
        raise NotImplementedError('This combination of SDEs is not supported for conditional SDEs yet.')
    if ve and not continuous:
        raise NotImplementedError('the fused loop runs the VE SDEs in continuous time only')
    ts, labels, std_x, G, std_y = step_scalars(sde, p_steps, eps, unconditional_label, continuous)
    pid = cid = 0
    pred_tab = corr_tab = None
    if predictor is not None or corrector is not None:
        from . import correctors as C_, predictors as P_
        predictor = predictor or P_.ReverseDiffusionPredictor
        corrector = corrector or C_.LangevinCorrector
        pid, cid, pred_tab, corr_tab = rule_tables(c_sde, ts, predictor, corrector, float(snr), probability_flow)
    rd_tab, rd_sub_x = reverse_diffusion_table(c_sde, ts) if pid == 0 else (None, 0)
    if cid == 0 and corr_alpha is None:
        corr_alpha = langevin_alphas(c_sde, ts)
    path_tab, path_std0 = None, 0.0
    if con is not None:
        con.fill(dev, c_sde, ts)
    if use_path:
        if not isinstance(sde, dict):
            raise NotImplementedError('use_path needs the two-SDE (CMDE / VS-CMDE) setting: sde = {"x": ..., "y": ...}')
        if global_norm is not None:
            raise NotImplementedError('use_path is not provided in the global-norm sharded mode')
        path_tab, path_std0 = path_tables(sde['y'], ts)
        std_y = None                            # y_t comes from the bridge, not from the marginal
    # prior: VE N(0, sigma_max^2) (+ data mean) - drawn on the host like the reference (sde_lib.py:397-403); VP / sub-VP N(0, I) (:177-178)
    if noise_tape is not None:
        tape = [t.float() for t in noise_tape]
        x = (tape[0] * c_sde.sigma_max) if ve else tape[0]
        if ve and c_sde.diffused_mean is not None:
            x = x + c_sde.diffused_mean.unsqueeze(0)
        x = x.to(dev).contiguous()
        flat = torch.cat([t.reshape(-1) for t in tape[1:]]).to(dev).contiguous() if len(tape) > 1 else None
        # draws and elements: an x draw has the state's size, a y draw that of y (the low-resolution y of a y_scale network)
        check_tape(_noise_draws(model._h, B, pid, cid, std_y is not None, use_path, con.draws if con is not None else 0, p_steps),
                   tape[1:], int(x.numel()), int(y.numel()) if y is not None else 0)
    else:
        x = ops.randn(tuple(shape), seed, 0, dev)
        if ve:
            x = ops.scale_rows(x, torch.full((B,), float(c_sde.sigma_max), device=dev))
        if ve and c_sde.diffused_mean is not None:
            raise NotImplementedError('data-mean prior with on-device noise is not provided yet')
        flat = None
    model.eval()
    model._ensure_packed()
    n_rec = p_steps + (1 if con is not None else 0)          # a constrained run records its initial state in front of the steps
    rec = ops._out((n_rec,) + tuple(x.shape), torch.float32, dev) if record else None
    rec_steps = rec
    if con is not None:
        con.start(x, record)
        if record:
            rec[0].copy_(x)
            rec_steps = rec[1:]
    p = _lib.PCParams()
    p.n_steps = p_steps
    p.labels, p.std_x, p.G = _fp(labels), _fp(std_x), _fp(G)
    p.std_y = _fp(std_y) if std_y is not None else None
    p.snr = float(snr)
    p.denoise = int(bool(denoise))
    p.noise_tape = flat.data_ptr() if flat is not None else None
    p.seed = int(seed)
    p.record = rec_steps.data_ptr() if rec is not None else None
    p.predictor, p.corrector = pid, cid
    p.pred_coef = _fp(pred_tab) if pred_tab is not None else None
    p.corr_coef = _fp(corr_tab) if corr_tab is not None else None
    p.path_coef = _fp(path_tab) if path_tab is not None else None
    p.path_std0 = float(path_std0)
    if corr_alpha is not None:
        corr_alpha = torch.as_tensor(corr_alpha, dtype=torch.float32).contiguous()
        if corr_alpha.numel() != p_steps:
            raise ValueError('corr_alpha needs one factor per step (%d), got %d' % (p_steps, corr_alpha.numel()))
    p.corr_alpha = _fp(corr_alpha) if corr_alpha is not None else None
    p.rd_drift = _fp(rd_tab) if rd_tab is not None else None
    p.rd_sub_x = rd_sub_x
    p.probability_flow = int(bool(probability_flow)) if pid == 0 else 0      # (an affine table carries the flow in its coefficients)
    if global_norm is not None and cid != 0:
        global_norm = None                      # only the Langevin corrector couples the samples of a batch
    yy = y.contiguous() if y is not None else None
    keep = (labels, std_x, G, std_y, pred_tab, corr_tab, path_tab, corr_alpha, rd_tab, flat, rec)
    if con is not None:
        keep += con.keep
    return Prepared(model=model, dev=dev, B=B, x=x, y=yy, p=p, constraint=con, rec=rec, ts=ts, p_steps=p_steps, global_norm=global_norm,
                    keep=keep)


def launch(prep):
    """Enqueue a ``Prepared`` loop through its single-stage entry (csd_pc_sample / csd_pc_inpaint_sample / csd_pc_colorize_sample, or
    the two step calls per PC step under ``global_norm``); returns ``(samples, record_or_None, timesteps)``."""
    model, dev, B, x, p, con = prep.model, prep.dev, prep.B, prep.x, prep.p, prep.constraint
    ws = model._workspace(B)
    family, scratch_bytes = (con.family, con.scratch_bytes) if con is not None else ('pc', _Constraint.scratch_bytes)
    scratch = ops._scratch(getattr(lib(), scratch_bytes)(model._h, B), dev)
    sample, begin, end = (getattr(lib(), 'csd_%s_%s' % (family, f)) for f in ('sample', 'step_begin', 'step_end'))
    args = (model._h, ptr(model._packed), ptr(ws), ws.numel(), ptr(scratch), scratch.numel(), ptr(x), ptr(prep.y), B, ctypes.byref(p))
    if con is not None:
        args += (ctypes.byref(con.struct),)                 # (prepare refused a y: the constrained families run unconditional networks)
    if prep.global_norm is None:
        check(sample(*args, current_stream(dev)), family + '_sample')
    else:
        reduce_fn, global_batch = prep.global_norm
        sums = torch.zeros(2, dtype=torch.float32, device=dev)
        for i in range(prep.p_steps):
            check(begin(*args, i, ptr(sums), current_stream(dev)), family + '_step_begin')
            reduce_fn(sums)
            check(end(*args, i, ptr(sums), int(global_batch), current_stream(dev)), family + '_step_end')
    # (prep.keep held the host arrays until the enqueue returned: they are read at enqueue time only)
    return x, prep.rec, prep.ts


def run(model, sde, shape, y, p_steps, snr, eps, denoise, noise_tape=None, seed=None, record=False,
        unconditional_label=None, global_norm=None, predictor=None, corrector=None, probability_flow=False, use_path=False,
        corr_alpha=None, continuous=True, inpaint=None, colorize=None):
    """Run the fused loop; returns (samples, record_or_None, timesteps).  ``seed=None``: a fresh key per call (fresh_seed).

    ``predictor`` / ``corrector``: the registered classes (default: the reverse-diffusion / Langevin pair); see ``fusable``.

    ``corr_alpha``: optional [p_steps] fp32 factors of the Langevin step size (csd_pc_params.corr_alpha); None = alphas[timestep] for
    the VP classes (sampling/correctors.py:63-65,94-96) and 1 for the VE SDEs.

    ``continuous``: False selects the discrete-time std of the VP classes (sqrt_1m_alphas_cumprod at the truncated label,
    models/utils.py:201-205,237-241); the VE SDEs run continuous only.

    Prior: N(0, sigma_max^2) (+ data mean) for the VE SDEs, N(0, I) for VP / sub-VP; ``noise_tape[0]`` is the standard-normal draw.

    ``inpaint``: ``(data, mask)`` - inpainting with an unconditional network (csd_pc_inpaint_sample; sampling/unconditional.py:230-345):
    the loop starts from prior*(1 - mask) + data*mask and re-imposes the known pixels (mask = 1) at every step's noise level after
    each phase.  ``mask`` broadcasts to ``data`` (the Haar multi-scale model passes [1, C, 1, 1]).  Draw order / tape layout: prior,
    then the rows of ``noise_draws`` (per step [z_corrector] z_blend [z_predictor] z_blend); without a tape the prior is
    ``ops.randn`` stream 0.  ``record`` then returns [p_steps + 1, ...]: the initial state followed by every step.

    ``colorize``: the gray-scale image [B, 3, H, W] - colorization with an unconditional 3-channel network (csd_pc_colorize_sample;
    controllable_generation.py:95-191 of the reference): the loop starts from couple(decouple(gray)*mask + decouple(prior*(1 - mask)))
    and re-imposes the gray channel of the decoupled space at every step's noise level after each phase (``ops.colorize_blend``).  Draw
    order, tape layout, ``record`` and the refusals are those of ``inpaint``, with a full-size z_colorize draw (channel 0 used) where
    inpainting has its z_blend; ``inpaint`` and ``colorize`` together are refused.

    ``global_norm``: None = the Langevin step size uses the batch means of THIS call's batch (the reference run on this batch;
    one library call enqueues the whole loop).  Otherwise ``(reduce_fn, global_batch)``: the batch is one shard of a larger one
    and the step size must use the means over the GLOBAL batch (identical to one reference process holding all of it,
    sampling/correctors.py:100-106): every PC step is enqueued as csd_pc_step_begin -> ``reduce_fn(sums)`` -> csd_pc_step_end,
    where ``sums`` is a 2-float device tensor and ``reduce_fn`` adds the other shards' sums into it in place (an 8-byte
    ``torch.distributed.all_reduce``) - no host synchronisation anywhere."""
    return launch(prepare(model, sde, shape, y, p_steps, snr, eps, denoise, noise_tape=noise_tape, seed=seed, record=record,
                          unconditional_label=unconditional_label, global_norm=global_norm, predictor=predictor, corrector=corrector,
                          probability_flow=probability_flow, use_path=use_path, corr_alpha=corr_alpha, continuous=continuous,
                          inpaint=inpaint, colorize=colorize))
