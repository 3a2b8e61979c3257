"""The RK45 step-size controller of ode_solver.py over a numpy backend against scipy.integrate.solve_ivp(method='RK45'): the same
number of right-hand sides, the same number of accepted steps, the same final state to rounding.  No GPU.

The test problem is contracting in both directions of time (the factor d = sign(t1 - t0)), so rounding differences between the two
implementations are damped instead of amplified and the step sequences stay identical."""
import math

import numpy as np
import pytest
from scipy import integrate

from conditional_score_diffusion_amd import ode_solver
from conditional_score_diffusion_amd._lib import NonFiniteError


def _sum(v):
    """a sum whose order differs from numpy's pairwise one: 7 chunks, last chunk first, each chunk back to front, sequentially"""
    total = 0.0
    for chunk in reversed(np.array_split(v, 7)):
        total += float(np.add.reduce(chunk[::-1].copy()))
    return total


class NumpyBackend:
    """the backend interface of ode_solver.solve on float64 numpy vectors (the stage store is 7 rows, `flip` counts them from the
    far end)"""

    def __init__(self, y0):
        self.n = y0.size
        self.y, self.ynew, self.ytmp = y0.astype(np.float64).copy(), np.empty(y0.size), np.empty(y0.size)
        self.K = np.full((7, y0.size + 3), np.nan)
        self.x32 = np.empty(y0.size, dtype=np.float32)
        self.x32[:] = self.y

    def krow(self, flip, j):
        return self.K[6 - j if flip else j, :self.n]

    def combine(self, y, flip, s, coef, h, out):
        acc = np.zeros(self.n)
        for j in range(s):
            acc += coef[j] * self.krow(flip, j)
        out[:] = y + h * acc
        self.x32[:] = out

    def error_sumsq(self, y, ynew, flip, E, h, rtol, atol):
        acc = np.zeros(self.n)
        for j in range(7):
            acc += E[j] * self.krow(flip, j)
        return _sum((h * acc / (atol + rtol * np.maximum(np.abs(y), np.abs(ynew)))) ** 2)

    def scaled_sumsq(self, alpha, u, beta, w, y, rtol, atol):
        v = alpha * u if w is None else alpha * u + beta * w
        return _sum((v / (atol + rtol * np.abs(y))) ** 2)


def problem(n):
    """f(t, y) = d (-lam y + 5 sin(w t) + 0.3 roll(y, 1)^2 / (1 + y^2)), d = sign(t1 - t0); -> (make_f(d), y0)"""
    rs = np.random.RandomState(3)
    lam = rs.uniform(0.1, 3.0, size=n)
    w = rs.uniform(0.0, 20.0, size=n)
    y0 = 3.0 * rs.standard_normal(n)

    def make_f(d):
        return lambda t, y: d * (-lam * y + 5.0 * np.sin(w * t) + 0.3 * np.roll(y, 1) ** 2 / (1.0 + y * y))

    return make_f, y0


def scipy_reference(n, t0, t1, tol):
    make_f, y0 = problem(n)
    f = make_f(math.copysign(1.0, t1 - t0))
    sol = integrate.solve_ivp(f, (t0, t1), y0, rtol=tol, atol=tol, method='RK45')
    assert sol.status == 0
    return sol.y[:, -1], sol.nfev, sol.t.size - 1


SPANS = [(1.0, 1e-3), (1e-5, 1.0)]


@pytest.mark.parametrize('tol', [1e-5, 1e-6])
@pytest.mark.parametrize('span', SPANS)
@pytest.mark.parametrize('n', [75, 1001, 1538])
def test_controller_matches_scipy_rk45(n, span, tol):
    t0, t1 = span
    want_y, want_nfev, want_steps = scipy_reference(n, t0, t1, tol)
    make_f, y0 = problem(n)
    f = make_f(math.copysign(1.0, t1 - t0))
    be = NumpyBackend(y0)

    def rhs(t, y, x32, k_out):
        k_out[:] = f(t, y)

    res = ode_solver.solve(rhs, be, t0, t1, tol, tol)
    diff = np.abs(res.y - want_y).max() / np.abs(want_y).max()
    print('n %d span %r tol %g: nfev %d (scipy %d), steps %d (scipy %d), rejected %d, rel diff %.3g'
          % (n, span, tol, res.nfev, want_nfev, res.n_accepted, want_steps, res.n_rejected, diff))
    assert res.t == t1
    assert res.nfev == want_nfev
    assert res.n_accepted == want_steps
    assert res.nfev == 2 + 6 * (res.n_accepted + res.n_rejected)
    assert diff <= 1e-12
    assert np.array_equal(be.x32, res.y.astype(np.float32))          # the fp32 copy follows the state


def test_tableau_is_dormand_prince():
    """the order conditions the published tableau satisfies: rows of A sum to C, B is a 5th-order and B - E a 4th-order quadrature"""
    A, B, C, E = ode_solver.A, ode_solver.B, ode_solver.C, ode_solver.E
    for s in range(1, 6):
        assert len(A[s]) == s and abs(sum(A[s]) - C[s]) < 1e-15
    c7 = np.array(C + (1.0,))
    b7, e7 = np.array(B + (0.0,)), np.array(E)
    for k in range(5):
        assert abs(np.dot(b7, c7 ** k) - 1 / (k + 1)) < 1e-15
    for k in range(4):
        assert abs(np.dot(b7 - e7, c7 ** k) - 1 / (k + 1)) < 1e-15
    assert abs(np.dot(b7 - e7, c7 ** 4) - 1 / 5) > 1e-4               # (the embedded formula is of order 4 only)
    assert E[6] == -1 / 40 and abs(sum(E)) < 1e-16


def test_nan_right_hand_side_raises_nonfinite():
    be = NumpyBackend(np.ones(10))

    def rhs(t, y, x32, k_out):
        k_out[:] = np.nan if t > 0.05 else -y

    with pytest.raises(NonFiniteError):
        ode_solver.solve(rhs, be, 0.0, 1.0, 1e-5, 1e-5)
    with pytest.raises(NonFiniteError):                                # from the first evaluation on
        ode_solver.solve(lambda t, y, x32, k: k.fill(np.nan), NumpyBackend(np.ones(10)), 0.0, 1.0, 1e-5, 1e-5)


def test_zero_length_span_returns_y0_without_an_evaluation():
    """the controller notices the empty span before it evaluates f0: nfev = 0 (scipy reports 1)"""
    y0 = np.arange(5.0)
    calls = []
    res = ode_solver.solve(lambda t, y, x32, k: calls.append(t), NumpyBackend(y0), 0.3, 0.3, 1e-5, 1e-5)
    assert res.nfev == 0 and calls == [] and res.n_accepted == 0 and res.t == 0.3
    assert np.array_equal(res.y, y0)


def test_step_below_float_spacing_raises_runtime_error_naming_t():
    """an error estimate that never drops below 1 shrinks the step until it falls below 10 ulp of t"""
    class Stubborn(NumpyBackend):
        def error_sumsq(self, *a):
            return 4.0 * self.n

    with pytest.raises(RuntimeError, match=r't = 1\.0') as info:
        ode_solver.solve(lambda t, y, x32, k: k.fill(1.0), Stubborn(np.ones(4)), 1.0, 2.0, 1e-5, 1e-5)
    assert not isinstance(info.value, NonFiniteError)
