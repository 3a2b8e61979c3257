"""Likelihood of the data under the probability-flow ODE (reference likelihood.py:21-103), in bits/dim.

``get_div_fn`` and ``get_likelihood_fn`` keep the reference's names and signatures; ``likelihood_fn(model, data)`` returns
``(bpd, z, nfe)``.  The ODE

    dx/dt = f(x, t) - g(t)^2 score(x, t) / 2,     d log p / dt = div_x of that drift (Hutchinson-Skilling estimate)

is integrated by scipy's ``solve_ivp`` from ``eps`` to ``sde.T`` on the host, exactly as in the reference, so ``nfe`` means the same.

Two paths compute the right-hand side:

* **fused** (a HIP network - DDPM family or planned NCSN++ - and a VE, VP or sub-VP SDE): per evaluation one host-to-device copy of the
  float64 state (with the per-row SDE coefficients and labels), ``csd_pf_ode_state`` (the fp32 operands of the network),
  ``csd_unet_train_forward`` (dropout 0), ``csd_unet_backward_ex`` (input gradient only, seeded with the Hutchinson noise),
  ``csd_pf_ode_rhs`` (drift and divergence in fp64) and one device-to-host copy.  Every SDE of sde_lib has a drift linear in x,
  f = a x, and the score is s h for the raw network output h, so the drift is a x + c h with c = -g^2 s / 2, and the divergence
  estimate is a eps.eps + c eps.(dh/dx)^T eps.
* **generic** (any other model or SDE): the reference algorithm over torch autograd (``get_div_fn``); HIP networks take part through
  their eval-mode input gradient.

``get_conditional_likelihood_fn`` gives the conditional NLL of x given a clean y under a single conditional SDE (cVESDE / cVPSDE: the
CDE / SR3 estimator).  The CMDE / VS-CMDE pair diffuses y as well and is not provided.

``device_loop=True`` (both getters; the default False is the path above, unchanged) keeps the fused right-hand side and replaces scipy by
``ode_solver.solve``: the same RK45 controller with the float64 state and the stage derivatives in device memory.  The per-evaluation
upload shrinks to the 20 B bytes of coefficients and labels, the download to one double per attempted step; the network's fp32 input is
written by the stage combination itself (``csd_ode_combine``), so ``csd_pf_ode_state`` is not run.  A combination it does not cover
raises NotImplementedError; it never falls back to the host loop.
"""
import ctypes

import numpy as np
import torch
from scipy import integrate

from . import ops, sde_lib
from ._lib import check, current_stream, lib, ptr
from .models import utils as mutils


def get_div_fn(fn):
    """Create the divergence function of `fn` using the Hutchinson-Skilling trace estimator."""

    def div_fn(x, t, eps):
        with torch.enable_grad():
            x.requires_grad_(True)
            fn_eps = torch.sum(fn(x, t) * eps)
            grad_fn_eps = torch.autograd.grad(fn_eps, x)[0]
        x.requires_grad_(False)
        return torch.sum(grad_fn_eps * eps, dim=tuple(range(1, len(x.shape))))

    return div_fn


def _hutchinson_noise(hutchinson_type, data):
    if hutchinson_type == 'Gaussian':
        return torch.randn_like(data)
    if hutchinson_type == 'Rademacher':
        return torch.randint_like(data, low=0, high=2).float() * 2 - 1.
    raise NotImplementedError(f"Hutchinson type {hutchinson_type} unknown.")


def _bpd(sde, inverse_scaler, z, delta_logp, shape):
    prior_logp = sde.prior_logp(z)
    bpd = -(prior_logp + delta_logp) / np.log(2)
    N = np.prod(shape[1:])
    bpd = bpd / N
    # A hack to convert log-likelihoods to bits/dim
    offset = 7. - inverse_scaler(-1.)
    return bpd + offset


class _Probe:
    """Stands in for the network inside ``mutils.get_score_fn``: records the labels the score function feeds it and returns ones, so
    the score function's value is the per-row factor s_b of score = s_b * h.  The fused path thus takes labels and scaling from the
    same code as the generic one."""

    def __init__(self, model):
        self.embedding_type = getattr(model, 'embedding_type', 'positional')
        self.labels = None

    def train(self, mode=True):
        return self

    def eval(self):
        return self

    def __call__(self, x, labels):
        self.labels = labels
        return torch.ones_like(x['x'] if isinstance(x, dict) else x)


def _row_coefficients(sde, probe_score_fn, probe, t, B, conditional):
    """(a, c, labels) float64 [B] each at the uniform time t: f = a x, drift = a x + c h."""
    vec_t = torch.ones(B) * t
    one = torch.ones(B, 1, 1, 1)
    s = probe_score_fn({'x': one, 'y': one} if conditional else one, vec_t)
    drift, g = sde.sde(one, vec_t)
    a = drift.reshape(B).double()
    g = torch.as_tensor(g).reshape(-1).expand(B).double()
    c = -0.5 * g * g * s.reshape(B).double()
    return a, c, probe.labels.reshape(B).double()


def _fused_supported(model, sde, conditional):
    from .models.ddpm import HipUNet
    if not isinstance(model, HipUNet) or model.device.type != 'cuda':
        return False
    if conditional:
        return isinstance(sde, (sde_lib.cVESDE, sde_lib.cVPSDE)) and model.y_channels > 0
    return isinstance(sde, (sde_lib.VESDE, sde_lib.VPSDE, sde_lib.subVPSDE)) and model.y_channels == 0


class _FusedRHS:
    """The probability-flow right-hand side of one likelihood call on the HIP network (buffers allocated once per call)."""

    def __init__(self, model, sde, x, y, epsilon, conditional, host_state=True):
        self.model, self.sde, self.conditional = model, sde, conditional
        dev = x.device
        B, cx, S = x.shape[0], model.x_channels, model.image_size
        if tuple(x.shape) != (B, cx, S, S):
            raise RuntimeError('data has shape %s, expected %s' % (tuple(x.shape), (B, cx, S, S)))
        self.B, self.D, self.dev = B, cx * S * S, dev
        oc = model.out_channels
        self.net_stride = oc * S * S
        self.probe = _Probe(model)
        self.score = mutils.get_score_fn(sde, self.probe, conditional=conditional, train=False, continuous=True)
        self.params = model._train_params()
        self.table = (ctypes.c_void_p * len(self.params))(*[p.data_ptr() for p in self.params])
        need = lib().csd_unet_train_workspace_bytes(model._h, B, 0.0)
        if need == 0:
            raise RuntimeError('libcsd_hip: cannot plan the likelihood graph at batch %d: %s' % (B, lib().csd_last_error().decode()))
        self.ws = ops._scratch(need, dev)
        n = B * self.D
        self.n = n
        if host_state:              # (the state lives with scipy; host_state=False: with ode_solver on the device, see device_rhs)
            # upload: [x (B*D) | log p (B) | a (B) | c (B) | labels (B)] float64 - ONE copy per evaluation
            self.host = torch.empty(n + 4 * B, dtype=torch.float64).pin_memory()
            self.up = torch.empty(n + 4 * B, dtype=torch.float64, device=dev)
            self.res = torch.empty(n + B, dtype=torch.float64, device=dev)
            self.res_host = torch.empty(n + B, dtype=torch.float64).pin_memory()
        self.x32 = torch.empty(B, cx, S, S, dtype=torch.float32, device=dev)
        self.lab32 = torch.empty(B, dtype=torch.float32, device=dev)
        self.out = torch.empty(B, oc, S, S, dtype=torch.float32, device=dev)
        self.v = torch.empty(B, cx, S, S, dtype=torch.float32, device=dev)
        self.dout = torch.zeros(B, oc, S, S, dtype=torch.float32, device=dev)     # d_out = eps on the x channels
        self.dout[:, :cx].copy_(epsilon)
        self.y = y.to(device=dev, dtype=torch.float32).contiguous() if model.y_channels else None
        self.scratch = ops._scratch(lib().csd_pf_ode_scratch_bytes(B, self.D), dev)
        self.stream = current_stream(dev)
        if host_state:
            base = self.up.data_ptr()
            self.p_a, self.p_c, self.p_lab = (ctypes.c_void_p(base + 8 * (n + k * B)) for k in (1, 2, 3))

    def _evaluate(self, state, lab32, p_a, p_c, res):
        """forward, input-only backward and csd_pf_ode_rhs at the fp32 operands self.x32 / lab32; state, res: float64 [n + B]"""
        model, B = self.model, self.B
        model._xgrad_calls = getattr(model, '_xgrad_calls', 0) + 1
        call = model._xgrad_calls
        check(lib().csd_unet_train_forward(model._h, self.table, ptr(self.ws), self.ws.numel(), ptr(self.x32), ptr(self.y),
                                           ptr(lab32), ptr(self.out), B, 0.0, model.dropout_seed, call, self.stream),
              'unet_train_forward')
        check(lib().csd_unet_backward_ex(model._h, self.table, None, ptr(self.v), ptr(self.ws), self.ws.numel(), ptr(self.dout), B,
                                         call, self.stream), 'unet_backward_ex')
        check(lib().csd_pf_ode_rhs(ptr(state), ptr(self.out), ptr(self.v), ptr(self.dout), self.net_stride, p_a, p_c,
                                   ptr(res), B, self.D, ptr(self.scratch), self.stream), 'pf_ode_rhs')

    def __call__(self, t, state):
        B, n = self.B, self.n
        a, c, labels = _row_coefficients(self.sde, self.score, self.probe, t, B, self.conditional)
        h = self.host.numpy()
        h[:n + B] = state
        h[n + B:n + 2 * B] = a.numpy()
        h[n + 2 * B:n + 3 * B] = c.numpy()
        h[n + 3 * B:] = labels.numpy()
        self.up.copy_(self.host, non_blocking=True)
        check(lib().csd_pf_ode_state(ptr(self.up), self.p_lab, ptr(self.x32), ptr(self.lab32), B, self.D, self.stream), 'pf_ode_state')
        self._evaluate(self.up, self.lab32, self.p_a, self.p_c, self.res)
        self.res_host.copy_(self.res, non_blocking=True)
        torch.cuda.current_stream(self.dev).synchronize()
        return self.res_host.numpy().copy()

    def device_rhs(self):
        """The same evaluation as an ``ode_solver`` right-hand side ``rhs(t, y, x32, k_out)``: the state ``y`` and the derivative
        ``k_out`` (float64 [n + B]) stay on the device, ``x32`` is self.x32 (the solver's combine pass keeps it equal to float(y_x));
        what is uploaded per evaluation is [a | c | labels] through a pinned ring."""
        from .ode_solver import CoefficientRing
        ring = CoefficientRing(self.B, self.dev)
        p_a, p_c = ctypes.c_void_p(ring.a.data_ptr()), ctypes.c_void_p(ring.c.data_ptr())

        def rhs(t, y, x32, k_out):
            ring.upload(*_row_coefficients(self.sde, self.score, self.probe, t, self.B, self.conditional))
            self._evaluate(y, ring.labels, p_a, p_c, k_out)

        return rhs

    def close(self):
        lib().csd_unet_train_release(self.model._h, ptr(self.ws))


def _solve(ode_func, data, sde, rtol, atol, method, eps):
    shape = data.shape
    init = np.concatenate([mutils.to_flattened_numpy(data), np.zeros((shape[0],))], axis=0)
    solution = integrate.solve_ivp(ode_func, (eps, sde.T), init, rtol=rtol, atol=atol, method=method)
    nfe = solution.nfev
    zp = solution.y[:, -1]
    z = mutils.from_flattened_numpy(zp[:-shape[0]], shape).to(data.device).type(torch.float32)
    delta_logp = mutils.from_flattened_numpy(zp[-shape[0]:], (shape[0],)).to(data.device).type(torch.float32)
    return z, delta_logp, nfe


def why_not_device_loop(model, sde, conditional, method):
    """None when (model, sde, method) runs on the device-resident RK45 loop, else the reason as text."""
    from .models.ddpm import HipUNet
    if method != 'RK45':
        return "the device loop integrates with RK45 only, not method = '%s'" % method
    if not isinstance(model, HipUNet):
        return 'the model is a %s, not a HipUNet' % type(model).__name__
    if model.device.type != 'cuda':
        return 'the model is on %s, the device loop runs on the GPU' % model.device
    if not _fused_supported(model, sde, conditional):
        want = 'cVESDE / cVPSDE with a network that takes a condition' if conditional else \
            'VESDE / VPSDE / subVPSDE with an unconditional network'
        return 'the fused right-hand side covers %s, not %s with a %d-channel condition' % (
            want, type(sde).__name__, getattr(model, 'y_channels', 0))
    return None


def _solve_on_device(rhs, data, sde, rtol, atol, eps):
    """_solve with the state [x | log p] and the stage derivatives in device memory (ode_solver.solve)"""
    from . import ode_solver
    B = data.shape[0]
    init = torch.cat([data.reshape(-1).double(), torch.zeros(B, dtype=torch.float64, device=data.device)])
    be = ode_solver.DeviceBackend(init, x32=rhs.x32)
    res = ode_solver.solve(rhs.device_rhs(), be, eps, sde.T, rtol, atol)
    z = res.y[:-B].reshape(data.shape).type(torch.float32)
    delta_logp = res.y[-B:].type(torch.float32)
    return z, delta_logp, res.nfev


def _run(model, sde, inverse_scaler, data, y, hutchinson_type, epsilon, rtol, atol, method, eps, conditional, drift_fn,
         device_loop=False):
    if (getattr(model, 'planned', False) or getattr(model, 'planned_train', False)) and data.dim() == 5:
        raise NotImplementedError('likelihood: the probability-flow right-hand side (csd_pf_ode_rhs) is not wired to the planned '
                                  'training graph of the 3-D networks')
    with torch.no_grad():
        shape = data.shape
        epsilon = _hutchinson_noise(hutchinson_type, data) if epsilon is None else \
            epsilon.to(device=data.device, dtype=torch.float32).reshape(shape)
        if device_loop:
            why = why_not_device_loop(model, sde, conditional, method)
            if why is not None:
                raise NotImplementedError('likelihood (device_loop=True): ' + why)
            rhs = _FusedRHS(model, sde, data, y, epsilon, conditional, host_state=False)
            try:
                z, delta_logp, nfe = _solve_on_device(rhs, data, sde, rtol, atol, eps)
            finally:
                rhs.close()
        elif _fused_supported(model, sde, conditional):
            rhs = _FusedRHS(model, sde, data, y, epsilon, conditional)
            try:
                z, delta_logp, nfe = _solve(rhs, data, sde, rtol, atol, method, eps)
            finally:
                rhs.close()
        else:
            div_fn = get_div_fn(drift_fn)

            def ode_func(t, x):
                sample = mutils.from_flattened_numpy(x[:-shape[0]], shape).to(data.device).type(torch.float32)
                vec_t = torch.ones(sample.shape[0], device=sample.device) * t
                drift = mutils.to_flattened_numpy(drift_fn(sample, vec_t))
                logp_grad = mutils.to_flattened_numpy(div_fn(sample, vec_t, epsilon))
                return np.concatenate([drift, logp_grad], axis=0)

            z, delta_logp, nfe = _solve(ode_func, data, sde, rtol, atol, method, eps)
        return _bpd(sde, inverse_scaler, z, delta_logp, shape), z, nfe


def get_likelihood_fn(sde, inverse_scaler, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45', eps=1e-5,
                      device_loop=False):
    """Create a function to compute the unbiased log-likelihood estimate of a given data point (reference likelihood.py:40-103).

    Returns ``likelihood_fn(model, data, epsilon=None) -> (bpd, z, nfe)``: bits/dim [B], the latent code, the number of function
    evaluations of the black-box solver.  ``epsilon`` (shape of ``data``) pins the Hutchinson noise; by default it is drawn once per
    call as in the reference.  ``device_loop=True``: the same fused right-hand side under the device-resident RK45 of ``ode_solver``
    instead of scipy on the host (module docstring); NotImplementedError where it does not apply."""

    def likelihood_fn(model, data, epsilon=None):
        def drift_fn(x, t):
            score_fn = mutils.get_score_fn(sde, model, train=False, continuous=True)
            # Probability flow ODE is a special case of Reverse SDE
            rsde = sde.reverse(score_fn, probability_flow=True)
            return rsde.sde(x, t)[0]

        return _run(model, sde, inverse_scaler, data, None, hutchinson_type, epsilon, rtol, atol, method, eps, False, drift_fn,
                    device_loop)

    return likelihood_fn


def get_conditional_likelihood_fn(sde, inverse_scaler, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45', eps=1e-5,
                                  device_loop=False):
    """Conditional NLL of x given y in bits/dim under the CDE / SR3 estimator: a single ``cVESDE`` / ``cVPSDE`` on x, the score network
    ``get_score_fn(..., conditional=True)`` sees the clean condition y.  Returns ``likelihood_fn(model, x, y, epsilon=None) ->
    (bpd, z, nfe)``; bits/dim are per dimension of x.  ``device_loop`` as in ``get_likelihood_fn``."""
    if isinstance(sde, dict):
        raise NotImplementedError('the conditional likelihood is provided for a single conditional SDE (CDE / SR3); the CMDE / VS-CMDE '
                                  'pair diffuses y as well')
    if not isinstance(sde, (sde_lib.cVESDE, sde_lib.cVPSDE)):
        raise NotImplementedError(f"SDE class {sde.__class__.__name__} is not a conditional SDE (cVESDE / cVPSDE).")

    def likelihood_fn(model, x, y, epsilon=None):
        if getattr(model, 'y_scale', 0):
            raise NotImplementedError('the conditional likelihood is not provided for %s (the Kx super-resolution networks, '
                                      'ddpm_KxSR / ncsnpp_KxSR)' % type(model).__name__)

        def drift_fn(xx, t):
            score_fn = mutils.get_score_fn(sde, model, conditional=True, train=False, continuous=True)
            rsde = sde.reverse(mutils.get_conditional_score_fn(score_fn, 'x'), probability_flow=True)
            return rsde.sde(xx, y, t)[0]

        return _run(model, sde, inverse_scaler, x, y, hutchinson_type, epsilon, rtol, atol, method, eps, True, drift_fn, device_loop)

    return likelihood_fn
