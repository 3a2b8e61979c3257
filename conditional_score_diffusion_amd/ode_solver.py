"""Adaptive Dormand-Prince 5(4) integration whose state never leaves the device.

The black-box ODE entry points (``get_ode_sampler``, ``get_likelihood_fn``) follow the reference in handing the state to scipy's
``solve_ivp`` on the host: two copies of the whole batch and a stream synchronisation per network evaluation, and all of RK45's
vector arithmetic in numpy.  ``solve`` is the same algorithm - the step-size controller of scipy's ``RK45`` (Hairer, Norsett, Wanner,
Solving Ordinary Differential Equations I, II.4 and II.5), restated over the published tableau - with the vectors kept where the
network is: the state, the stage argument and the seven stage derivatives live in the backend's memory, and the host sees one double
per attempted step (the squared error norm), from which it accepts or rejects the step and chooses the next ``h``.  That 8-byte read
is the loop's only synchronisation.

A backend holds the vectors and does three things with them:

* ``combine(y, flip, s, coef, h, out)``: ``out = y + h * sum_{j<s} coef[j] * K[j]``, and the network's fp32 copy of ``out``;
* ``error_sumsq(y, ynew, flip, E, h, rtol, atol)``: ``sum ((h * sum_j E[j] K[j]) / (atol + rtol * max(|y|, |ynew|)))**2``;
* ``scaled_sumsq(alpha, u, beta, w, y, rtol, atol)``: ``sum ((alpha u + beta w) / (atol + rtol |y|))**2`` (``w`` may be None),

both sums returned as Python floats.  Its attributes are ``n``, the three state vectors ``y`` (holds y0 on entry), ``ynew``, ``ytmp``,
the fp32 network input ``x32`` (holds float(y0) on entry) and ``krow(flip, j)``, stage derivative j.  The stage store is 7 rows;
``flip`` says from which end they are counted, so that the last stage of an accepted step is the first of the next (FSAL) by
toggling it - no copy.  ``DeviceBackend`` runs on csrc/ode_rk45.hip; the tests keep a numpy one.

The right-hand side is ``rhs(t, y, x32, k_out)``: it reads the state ``y`` (and its fp32 copy ``x32``), writes the derivative to
``k_out``, launches on the current stream and returns nothing.

No dense output, no events, RK45 only.  A span of zero length returns y0 without evaluating the right-hand side (``nfev = 0``).
"""
import collections
import ctypes
import math

from ._lib import NonFiniteError

# Dormand, Prince: A family of embedded Runge-Kutta formulae, J. Comp. Appl. Math. 6 (1980), the 5(4) pair with FSAL.
C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0)
A = ((),
     (1 / 5,),
     (3 / 40, 9 / 40),
     (44 / 45, -56 / 15, 32 / 9),
     (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
     (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656))
B = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84)
# B - B_hat (B_hat = 5179/57600, 0, 7571/16695, 393/640, -92097/339200, 187/2100, 1/40: the embedded 4th-order weights)
E = (71 / 57600, 0.0, -71 / 16695, 71 / 1920, -17253 / 339200, 22 / 525, -1 / 40)

SAFETY, MIN_FACTOR, MAX_FACTOR = 0.9, 0.2, 10.0
ERROR_EXPONENT = -1 / 5            # (the error estimate is of order 4)

Result = collections.namedtuple('Result', 't y nfev n_accepted n_rejected')


def _norm(sumsq, n, what, t):
    if not math.isfinite(sumsq):
        raise NonFiniteError('RK45: the %s at t = %r is not finite (%r): the right-hand side or the state left the finite range'
                             % (what, t, sumsq))
    return math.sqrt(sumsq) / n ** 0.5


def _initial_step(rhs, be, t0, t1, direction, rtol, atol):
    """Hairer, Norsett, Wanner II.4 (the starting step size); K[0] holds f0.  One more evaluation, left in K[1]."""
    n, y = be.n, be.y
    interval = abs(t1 - t0)
    f0, f1 = be.krow(False, 0), be.krow(False, 1)
    d0 = _norm(be.scaled_sumsq(1.0, y, 0.0, None, y, rtol, atol), n, 'norm of the initial state', t0)
    d1 = _norm(be.scaled_sumsq(1.0, f0, 0.0, None, y, rtol, atol), n, 'norm of the initial derivative', t0)
    h0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
    h0 = min(h0, interval)
    be.combine(y, False, 1, (1.0,), h0 * direction, be.ytmp)
    rhs(t0 + h0 * direction, be.ytmp, be.x32, f1)
    d2 = _norm(be.scaled_sumsq(1.0, f1, -1.0, f0, y, rtol, atol), n, 'norm of the derivative change', t0) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1 / 5)
    return min(100 * h0, h1, interval)


def solve(rhs, be, t0, t1, rtol, atol, first_step=None):
    """Integrate dy/dt = rhs from t0 to t1 (either direction) on the backend ``be``; -> Result(t, y, nfev, n_accepted, n_rejected)
    with ``y`` the backend vector that holds the final state (``be.x32`` holds its fp32 copy).  ``nfev`` counts every right-hand
    side, as scipy does: f0, the probe of the initial-step selection, and six per attempted step."""
    t0, t1, rtol, atol = float(t0), float(t1), float(rtol), float(atol)
    n = be.n
    if t1 == t0:
        return Result(t0, be.y, 0, 0, 0)
    direction = 1.0 if t1 > t0 else -1.0
    y, ynew, flip = be.y, be.ynew, False
    rhs(t0, y, be.x32, be.krow(flip, 0))
    nfev = 1
    if first_step is None:
        h_abs = _initial_step(rhs, be, t0, t1, direction, rtol, atol)
        nfev += 1
    else:
        h_abs = float(first_step)
        if not 0 < h_abs <= abs(t1 - t0):
            raise ValueError('first_step must be positive and no longer than the span')
    t, accepted, rejected = t0, 0, 0
    while t != t1:
        min_step = 10 * abs(math.nextafter(t, direction * math.inf) - t)
        h_abs = max(h_abs, min_step)
        step_rejected = False
        while True:
            if h_abs < min_step:
                raise RuntimeError('RK45: the step size fell below the spacing of floating-point numbers at t = %r' % t)
            h = h_abs * direction
            t_new = t + h
            if direction * (t_new - t1) > 0:
                t_new = t1
            h = t_new - t
            h_abs = abs(h)
            for s in range(1, 6):
                be.combine(y, flip, s, A[s], h, be.ytmp)
                rhs(t + C[s] * h, be.ytmp, be.x32, be.krow(flip, s))
            be.combine(y, flip, 6, B, h, ynew)
            rhs(t + h, ynew, be.x32, be.krow(flip, 6))
            nfev += 6
            err = _norm(be.error_sumsq(y, ynew, flip, E, h, rtol, atol), n, 'error norm of the step', t)
            if err < 1:
                factor = MAX_FACTOR if err == 0 else min(MAX_FACTOR, SAFETY * err ** ERROR_EXPONENT)
                if step_rejected:
                    factor = min(1.0, factor)
                h_abs *= factor
                break
            h_abs *= max(MIN_FACTOR, SAFETY * err ** ERROR_EXPONENT)
            step_rejected = True
            rejected += 1
        accepted += 1
        t, y, ynew, flip = t_new, ynew, y, not flip          # FSAL: K[6] is the next step's K[0]
    return Result(t, y, nfev, accepted, rejected)


class DeviceBackend:
    """The solver's vectors in device memory, its arithmetic on csrc/ode_rk45.hip (csd_ode_combine, csd_ode_error_sumsq,
    csd_ode_scaled_sumsq).  ``y0``: float64 [n] on the GPU (copied); ``x32``: the float32 buffer the right-hand side's network reads,
    its ``nx <= n`` elements are kept equal to float(state[:nx]) by the combine pass itself."""

    def __init__(self, y0, x32=None):
        import torch

        from . import ops
        from ._lib import current_stream, lib
        if not (y0.is_cuda and y0.dtype == torch.float64 and y0.dim() == 1):
            raise RuntimeError('DeviceBackend needs a flat float64 state on the GPU')
        dev = y0.device
        self.n = n = y0.numel()
        self.dev, self.lib, self.torch = dev, lib(), torch
        self.stream = current_stream(dev)
        self.stride = (n + 1) // 2 * 2                     # (even: every K row is 16-byte aligned)
        self.y = y0.clone()
        self.ynew, self.ytmp = torch.empty_like(self.y), torch.empty_like(self.y)
        self.K = torch.empty(7 * self.stride, dtype=torch.float64, device=dev)
        self.x32 = torch.empty(0, dtype=torch.float32, device=dev) if x32 is None else x32.view(-1)
        if self.x32.numel() > n or (self.x32.numel() and not (self.x32.is_cuda and self.x32.dtype == torch.float32)):
            raise RuntimeError('x32 must be a float32 GPU buffer of at most n elements')
        self.nx = self.x32.numel()
        if self.nx:
            self.x32.copy_(self.y[:self.nx])
        self.scratch = ops._scratch(self.lib.csd_ode_scratch_bytes(n), dev)
        self.res = torch.empty(2, dtype=torch.float64, device=dev)
        self.res_host = torch.empty(2, dtype=torch.float64).pin_memory()
        self._rows = [self.K[j * self.stride:j * self.stride + n] for j in range(7)]

    def krow(self, flip, j):
        return self._rows[6 - j if flip else j]

    def _k(self, flip):
        """(address of stage 0, signed row stride)"""
        return ctypes.c_void_p(self._rows[6 if flip else 0].data_ptr()), (-self.stride if flip else self.stride)

    def _read(self):
        self.res_host.copy_(self.res, non_blocking=True)
        self.torch.cuda.current_stream(self.dev).synchronize()
        return float(self.res_host[0])

    def combine(self, y, flip, s, coef, h, out):
        from ._lib import OdeCoef, check, ptr
        k0, stride = self._k(flip)
        c = OdeCoef((ctypes.c_double * 7)(*coef[:s]))
        check(self.lib.csd_ode_combine(ptr(y), k0, stride, s, c, h, ptr(out), ptr(self.x32) if self.nx else None, self.nx, self.n,
                                       self.stream), 'ode_combine')

    def error_sumsq(self, y, ynew, flip, E, h, rtol, atol):
        from ._lib import OdeCoef, check, ptr
        k0, stride = self._k(flip)
        c = OdeCoef((ctypes.c_double * 7)(*E))
        check(self.lib.csd_ode_error_sumsq(ptr(y), ptr(ynew), k0, stride, c, h, atol, rtol, self.n, ptr(self.res), ptr(self.scratch),
                                           self.stream), 'ode_error_sumsq')
        return self._read()

    def scaled_sumsq(self, alpha, u, beta, w, y, rtol, atol):
        from ._lib import check, ptr
        check(self.lib.csd_ode_scaled_sumsq(ptr(u), ptr(w), alpha, beta, ptr(y), atol, rtol, self.n, ptr(self.res), ptr(self.scratch),
                                            self.stream), 'ode_scaled_sumsq')
        return self._read()


class CoefficientRing:
    """Pinned staging for the per-evaluation coefficients of a right-hand side ([a | c] float64 and the labels float32, B each).  An
    upload is an asynchronous copy out of a slot; a slot is rewritten only ``slots`` uploads later, and the solver synchronises at
    least once per 6 evaluations (the error norm of every attempted step), so a copy never reads a slot that is being rewritten."""
    SLOTS = 8

    def __init__(self, B, dev):
        import torch
        self.B = B
        self.slot_bytes = (20 * B + 255) // 256 * 256
        self.host = torch.empty(self.SLOTS * self.slot_bytes, dtype=torch.uint8).pin_memory()
        self.device = torch.empty(self.slot_bytes, dtype=torch.uint8, device=dev)
        self.a = self.device[:8 * B].view(torch.float64)
        self.c = self.device[8 * B:16 * B].view(torch.float64)
        self.labels = self.device[16 * B:20 * B].view(torch.float32)
        self.k = 0

    def upload(self, a, c, labels):
        import torch
        B = self.B
        slot = self.host[self.k * self.slot_bytes:(self.k + 1) * self.slot_bytes]
        self.k = (self.k + 1) % self.SLOTS
        slot[:8 * B].view(torch.float64).copy_(a)
        slot[8 * B:16 * B].view(torch.float64).copy_(c)
        slot[16 * B:20 * B].view(torch.float32).copy_(labels)          # (float64 -> float32, as csd_pf_ode_state rounds them)
        self.device.copy_(slot, non_blocking=True)
