"""The device-resident RK45 on the MI355X: the kernels of csrc/ode_rk45.hip against float64 numpy, ode_solver.solve on the device
against scipy on an analytic problem, and get_ode_sampler / get_likelihood_fn / get_conditional_likelihood_fn with device_loop=True
against the reference's sample and against the host loop."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases
import score_oracle as so

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _coef(row):
    from conditional_score_diffusion_amd._lib import OdeCoef
    return OdeCoef((ctypes.c_double * 7)(*row))


def _kptr(K, stride, flip):
    """(address of stage 0, signed stride): flip counts the 7 rows from the far end, as the solver does after an accepted step"""
    return ctypes.c_void_p(K.data_ptr() + (6 * stride * 8 if flip else 0)), (-stride if flip else stride)


def _rows(Kh, stride, n, flip):
    return [Kh[(6 - j if flip else j) * stride:(6 - j if flip else j) * stride + n] for j in range(7)]


# ---- 1. kernels against float64 numpy ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 75, 1001, 1538, 300001])
def test_combine_vs_float64(n):
    """every s with the tableau's own rows and a random one; nx = 0, n - 2 (the end of the image rows inside a 16-byte step), n; an
    even stride (16-byte rows), an odd one (8-byte accesses) and the rows counted backwards"""
    from conditional_score_diffusion_amd import ode_solver as osv
    from conditional_score_diffusion_amd._lib import check, current_stream, lib, ptr
    rs = np.random.RandomState(n)
    y = rs.standard_normal(n) * 3.0
    rows = [(s, osv.A[s]) for s in range(1, 6)] + [(6, osv.B), (7, osv.E), (7, tuple(rs.standard_normal(7)))]
    yd = _T(y)
    for stride, flip in [((n + 1) // 2 * 2 + 4, False), (n + 3 + (n % 2), False), ((n + 1) // 2 * 2, True)]:
        Kh = rs.standard_normal(7 * stride) * 10.0
        Kd = _T(Kh)
        k0, ks = _kptr(Kd, stride, flip)
        kr = _rows(Kh, stride, n, flip)
        for s, row in rows:
            h = float(rs.uniform(-0.3, 0.3))
            want = y + h * sum(row[j] * kr[j] for j in range(s))
            for nx in sorted({0, max(n - 2, 0), n}):
                out = torch.full((n,), float('nan'), dtype=torch.float64, device=DEV)
                x32 = torch.full((n + 4,), float('nan'), dtype=torch.float32, device=DEV)
                check(lib().csd_ode_combine(ptr(yd), k0, ks, s, _coef(row[:s]), h, ptr(out), ptr(x32) if nx else None, nx, n,
                                            current_stream(DEV)), 'ode_combine')
                assert torch.allclose(out.cpu(), torch.from_numpy(want), rtol=1e-14, atol=1e-12), (stride, flip, s, nx)
                assert torch.equal(x32[:nx], out[:nx].float()), (stride, flip, s, nx)
                assert torch.isnan(x32[nx:]).all(), (stride, flip, s, nx)            # nothing written past nx


@pytest.mark.parametrize('n', [1, 75, 1001, 1538, 300001])
def test_sums_vs_float64(n):
    from conditional_score_diffusion_amd import ode_solver as osv
    from conditional_score_diffusion_amd._lib import check, current_stream, lib, ptr
    rs = np.random.RandomState(100 + n)
    y, yn, u, w = (rs.standard_normal(n) * 3.0 for _ in range(4))
    yd, ynd, ud, wd = _T(y), _T(yn), _T(u), _T(w)
    rtol, atol, h = 1e-5, 1e-6, 0.0123
    sc = torch.empty(lib().csd_ode_scratch_bytes(n), dtype=torch.uint8, device=DEV)
    res = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
    st = current_stream(DEV)

    def twice(call):
        got = []
        for _ in range(2):
            res.fill_(float('nan'))
            check(call(), 'ode sum')
            got.append(res.clone())
        assert torch.equal(got[0], got[1])           # fixed-order reduction: the same bits every run
        return got[0].item()

    for stride, flip in [((n + 1) // 2 * 2 + 4, False), (n + 3 + (n % 2), False), ((n + 1) // 2 * 2, True)]:
        Kh = rs.standard_normal(7 * stride) * 1e-3
        Kd = _T(Kh)
        k0, ks = _kptr(Kd, stride, flip)
        kr = _rows(Kh, stride, n, flip)
        want = math.fsum((h * sum(osv.E[j] * kr[j] for j in range(7)) / (atol + rtol * np.maximum(np.abs(y), np.abs(yn)))) ** 2)
        got = twice(lambda: lib().csd_ode_error_sumsq(ptr(yd), ptr(ynd), k0, ks, _coef(osv.E), h, atol, rtol, n, ptr(res), ptr(sc), st))
        assert abs(got - want) <= 1e-12 * abs(want), (stride, flip, got, want)
    for alpha, beta, wdev, whost in [(1.0, 0.0, None, None), (1.0, -1.0, wd, w), (0.7, 2.5, wd, w)]:
        v = alpha * u if whost is None else alpha * u + beta * whost
        want = math.fsum((v / (atol + rtol * np.abs(y))) ** 2)
        got = twice(lambda: lib().csd_ode_scaled_sumsq(ptr(ud), ptr(wdev), alpha, beta, ptr(yd), atol, rtol, n, ptr(res), ptr(sc), st))
        assert abs(got - want) <= 1e-12 * abs(want), (alpha, beta, got, want)
    if n > 1:                                        # operands that start 8 bytes off a 16-byte boundary: the 8-byte path
        want = math.fsum(((u[1:] - w[1:]) / (atol + rtol * np.abs(y[1:]))) ** 2)
        got = twice(lambda: lib().csd_ode_scaled_sumsq(ptr(ud[1:]), ptr(wd[1:]), 1.0, -1.0, ptr(yd[1:]), atol, rtol, n - 1, ptr(res),
                                                       ptr(sc), st))
        assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize('B,D,extra', [(1, 1, 0), (3, 75, 0), (2, 1001, 7), (3, 3 * 20 * 20, 3 * 20 * 20), (5, 3 * 160 * 160, 0)])
def test_drift_vs_float64(B, D, extra):
    from conditional_score_diffusion_amd._lib import check, current_stream, lib, ptr
    rs = np.random.RandomState(B * 7 + D)
    ns = D + extra
    y = rs.standard_normal(B * D) * 3.0
    h = rs.standard_normal((B, ns)).astype(np.float32)
    a, c = rs.standard_normal(B), rs.standard_normal(B) * 10
    out = torch.full((B * D,), float('nan'), dtype=torch.float64, device=DEV)
    yd, hd, ad, cd = _T(y), _T(h, torch.float32), _T(a), _T(c)
    check(lib().csd_ode_drift(ptr(yd), ptr(hd), ns, ptr(ad), ptr(cd), ptr(out), B, D, current_stream(DEV)), 'ode_drift')
    want = a[:, None] * y.reshape(B, D) + c[:, None] * h[:, :D].astype(np.float64)
    assert torch.allclose(out.cpu(), torch.from_numpy(want.reshape(-1)), rtol=1e-14, atol=1e-12)


def test_bad_arguments_return_an_error_and_launch_nothing():
    from conditional_score_diffusion_amd import ode_solver as osv
    from conditional_score_diffusion_amd._lib import current_stream, lib, ptr
    n = 64
    y = torch.ones(n, dtype=torch.float64, device=DEV)
    K = torch.ones(7 * n, dtype=torch.float64, device=DEV)
    out = torch.full((n,), float('nan'), dtype=torch.float64, device=DEV)
    x32 = torch.full((n,), float('nan'), dtype=torch.float32, device=DEV)
    st = current_stream(DEV)
    c = _coef(osv.B)
    bad = [lib().csd_ode_combine(ptr(y), ptr(K), n, 0, c, 0.1, ptr(out), ptr(x32), n, n, st),          # s = 0
           lib().csd_ode_combine(ptr(y), ptr(K), n, 8, c, 0.1, ptr(out), ptr(x32), n, n, st),          # s = 8
           lib().csd_ode_combine(ptr(y), ptr(K), n, 6, c, 0.1, ptr(out), ptr(x32), n + 1, n, st),      # nx > n
           lib().csd_ode_combine(ptr(y), ptr(K), n, 6, c, 0.1, ptr(y), ptr(x32), n, n, st),            # out aliases y
           lib().csd_ode_combine(ptr(y), ptr(K), n, 6, c, 0.1, ptr(K[5 * n:6 * n]), ptr(x32), n, n, st),   # out aliases a K row
           lib().csd_ode_combine(ptr(y), ptr(K), n - 2, 6, c, 0.1, ptr(out), ptr(x32), n, n, st)]     # rows overlap
    assert all(rc != 0 for rc in bad), bad
    assert b'ode_combine' in lib().csd_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(x32).all()
    assert torch.equal(y, torch.ones_like(y)) and torch.equal(K, torch.ones_like(K))


# ---- 2. the device solver on the analytic problem ---------------------------------------------------------------------------------

@pytest.mark.parametrize('span', [(1.0, 1e-3), (1e-5, 1.0)])
@pytest.mark.parametrize('n', [1001, 1538])
def test_device_solver_matches_scipy(n, span):
    from conditional_score_diffusion_amd import ode_solver as osv
    from test_ode_solver_host import scipy_reference
    t0, t1 = span
    tol = 1e-6
    want_y, want_nfev, want_steps = scipy_reference(n, t0, t1, tol)
    rs = np.random.RandomState(3)                     # the draws of test_ode_solver_host.problem
    lam, w, y0 = _T(rs.uniform(0.1, 3.0, size=n)), _T(rs.uniform(0.0, 20.0, size=n)), _T(3.0 * rs.standard_normal(n))
    d = math.copysign(1.0, t1 - t0)

    def rhs(t, y, x32, k_out):
        k_out.copy_(d * (-lam * y + 5.0 * torch.sin(w * t) + 0.3 * torch.roll(y, 1) ** 2 / (1.0 + y * y)))

    res = osv.solve(rhs, osv.DeviceBackend(y0), t0, t1, tol, tol)
    diff = np.abs(res.y.cpu().numpy() - want_y).max() / np.abs(want_y).max()
    print('n %d span %r: nfev %d (scipy %d), steps %d (scipy %d), rel diff %.3g' % (n, span, res.nfev, want_nfev, res.n_accepted,
                                                                                   want_steps, diff))
    assert res.nfev == want_nfev and res.n_accepted == want_steps
    assert diff <= 1e-12


# ---- 3. the ODE sampler -----------------------------------------------------------------------------------------------------------

def test_ode_sampler_device_loop_vs_reference_and_host_loop(golden_dir):
    from conditional_score_diffusion_amd.sampling.unconditional import get_sampling_fn
    from test_gpu_network import build, sdes_for
    g = np.load(os.path.join(golden_dir, 'ode.npz'))
    cfg, nc, p, model = build('uncond_tiny')
    sde = sdes_for(cfg)
    cfg.sampling.method = 'ode'
    B = cases.case_config('uncond_tiny')[1]
    shape = (B,) + tuple(cfg.data.shape_x)
    z = cases.tape([shape], 17)[0] * float(cfg.model.sigma_max_x)
    host, nfe_host = get_sampling_fn(cfg, sde, shape, 1e-5)(model, z=z.to(DEV))
    cfg.sampling.csd_device_loop = True
    x, nfe = get_sampling_fn(cfg, sde, shape, 1e-5)(model, z=z.to(DEV))
    assert x.dtype == torch.float32 and tuple(x.shape) == shape
    for name, ref, ref_nfe in (('reference', g['x'], int(g['nfe'])), ('host loop', host.cpu().numpy(), nfe_host)):
        err = np.abs(x.cpu().numpy() - ref).max() / np.abs(ref).max()
        print('device loop against the %s: nfe %d / %d, relative error %.3g' % (name, nfe, ref_nfe, err))
        assert abs(nfe - ref_nfe) <= 6
        assert err <= 1e-3


# ---- 4. the likelihoods -----------------------------------------------------------------------------------------------------------

TOL = dict(rtol=1e-6, atol=1e-6, eps=1e-3)    # (tests/test_gpu_likelihood.py)


def _agree(r1, r2):
    (b1, z1, n1), (b2, z2, n2) = r1, r2
    assert (b1.cpu().double() - b2.cpu().double()).abs().max().item() <= 1e-3, (b1, b2)
    zr = (z1.cpu().double() - z2.cpu().double()).abs().max().item() / z2.cpu().double().abs().max().item()
    assert zr <= 1e-3, zr
    assert abs(n1 - n2) <= max(12, 0.02 * n2), (n1, n2)     # (two RK45 steps)


def _same(r1, r2):
    return torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and r1[2] == r2[2]


def _uncond():
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = cases.case_config('uncond_tiny')
    cfg.model.csd_precision = 'fp32'
    nc = so.NetCfg.from_config(cfg)
    model = mutils.create_model(cfg)
    model.load_state_dict(so.synth_params(so.ddpm_param_shapes(nc), 0))
    rs = np.random.RandomState(17)
    x = torch.from_numpy(rs.uniform(0, 1, size=(B,) + tuple(cfg.data.shape_x)).astype(np.float32))
    e = torch.from_numpy((rs.randint(0, 2, size=x.shape) * 2 - 1).astype(np.float32))
    return cfg, model, x, e


def _sde(name):
    from conditional_score_diffusion_amd import sde_lib
    return {'ve': lambda: sde_lib.VESDE(0.01, 5.0, 1000), 'vp': lambda: sde_lib.VPSDE(0.1, 20., 1000),
            'subvp': lambda: sde_lib.subVPSDE(0.1, 20., 1000)}[name]()


@pytest.mark.parametrize('sde_name', ['ve', 'vp', 'subvp'])
def test_likelihood_device_loop_matches_host_loop(sde_name):
    from conditional_score_diffusion_amd import likelihood
    cfg, model, x, e = _uncond()
    model = model.to(DEV).eval()
    sde = _sde(sde_name)
    host = likelihood.get_likelihood_fn(sde, lambda v: v, **TOL)(model, x.to(DEV), epsilon=e.to(DEV))
    fn = likelihood.get_likelihood_fn(sde, lambda v: v, device_loop=True, **TOL)
    got = fn(model, x.to(DEV), epsilon=e.to(DEV))
    print('%s: bpd %s / %s, nfe %d / %d' % (sde_name, got[0].tolist(), host[0].tolist(), got[2], host[2]))
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32 and got[1].shape == x.shape and got[1].device.type == 'cuda'
    assert np.isfinite(got[0].cpu().numpy()).all()
    _agree(got, host)
    assert _same(got, fn(model, x.to(DEV), epsilon=e.to(DEV)))


def test_conditional_likelihood_device_loop_matches_host_loop():
    from conditional_score_diffusion_amd import likelihood, sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = cases.case_config('sr3_tiny')
    cfg.model.csd_precision = 'fp32'
    nc = so.NetCfg.from_config(cfg)
    model = mutils.create_model(cfg)
    model.load_state_dict(so.synth_params(so.ddpm_param_shapes(nc), 0))
    model = model.to(DEV).eval()
    rs = np.random.RandomState(19)
    x = torch.from_numpy(rs.uniform(0, 1, size=(B,) + tuple(cfg.data.shape_x)).astype(np.float32))
    y = cases.case_y('sr3_tiny')
    e = torch.from_numpy((rs.randint(0, 2, size=x.shape) * 2 - 1).astype(np.float32))
    sde = sde_lib.cVESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, cfg.model.num_scales)
    host = likelihood.get_conditional_likelihood_fn(sde, lambda v: v, **TOL)(model, x.to(DEV), y.to(DEV), epsilon=e.to(DEV))
    fn = likelihood.get_conditional_likelihood_fn(sde, lambda v: v, device_loop=True, **TOL)
    got = fn(model, x.to(DEV), y.to(DEV), epsilon=e.to(DEV))
    print('sr3: bpd %s / %s, nfe %d / %d' % (got[0].tolist(), host[0].tolist(), got[2], host[2]))
    _agree(got, host)
    assert _same(got, fn(model, x.to(DEV), y.to(DEV), epsilon=e.to(DEV)))


# ---- 5. guard rails ---------------------------------------------------------------------------------------------------------------

class Generic(nn.Module):
    """hides a HIP network from the fused dispatch"""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.embedding_type = getattr(net, 'embedding_type', 'positional')

    @property
    def device(self):
        return self.net.device

    def forward(self, x, labels):
        return self.net(x, labels)


def test_device_loop_refuses_what_it_does_not_cover():
    from conditional_score_diffusion_amd import likelihood
    from conditional_score_diffusion_amd.sampling.unconditional import get_ode_sampler
    cfg, cpu_model, x, e = _uncond()
    sde = _sde('ve')
    shape = tuple(x.shape)
    with pytest.raises(NotImplementedError, match='on cpu'):
        likelihood.get_likelihood_fn(sde, lambda v: v, device_loop=True, **TOL)(cpu_model, x, epsilon=e)
    with pytest.raises(NotImplementedError, match='on cpu'):
        get_ode_sampler(sde, shape, device_loop=True)(cpu_model, z=x)
    model = _uncond()[1].to(DEV).eval()
    xd, ed = x.to(DEV), e.to(DEV)
    with pytest.raises(NotImplementedError, match='RK45 only.*RK23'):
        likelihood.get_likelihood_fn(sde, lambda v: v, method='RK23', device_loop=True, **TOL)(model, xd, epsilon=ed)
    with pytest.raises(NotImplementedError, match='RK45 only.*RK23'):
        get_ode_sampler(sde, shape, method='RK23', device_loop=True)(model, z=xd)
    with pytest.raises(NotImplementedError, match='Generic, not a HipUNet'):
        likelihood.get_likelihood_fn(sde, lambda v: v, device_loop=True, **TOL)(Generic(model), xd, epsilon=ed)
    with pytest.raises(NotImplementedError, match='Generic, not a HipUNet'):
        get_ode_sampler(sde, shape, device_loop=True)(Generic(model), z=xd)
    with pytest.raises(NotImplementedError, match='cVESDE'):
        from conditional_score_diffusion_amd import sde_lib
        get_ode_sampler(sde_lib.cVESDE(0.01, 5.0, 1000), shape, device_loop=True)(model, z=xd)


def test_device_loop_false_is_the_default_path():
    from conditional_score_diffusion_amd import likelihood
    from conditional_score_diffusion_amd.sampling.unconditional import get_ode_sampler
    cfg, model, x, e = _uncond()
    model = model.to(DEV).eval()
    sde = _sde('ve')
    xd, ed = x.to(DEV), e.to(DEV)
    a = likelihood.get_likelihood_fn(sde, lambda v: v, **TOL)(model, xd, epsilon=ed)
    b = likelihood.get_likelihood_fn(sde, lambda v: v, device_loop=False, **TOL)(model, xd, epsilon=ed)
    assert _same(a, b)
    z = (torch.from_numpy(np.random.RandomState(5).standard_normal(x.shape).astype(np.float32)) * 5.0).to(DEV)
    xa, na = get_ode_sampler(sde, tuple(x.shape), eps=1e-3)(model, z=z)
    xb, nb = get_ode_sampler(sde, tuple(x.shape), eps=1e-3, device_loop=False)(model, z=z)
    assert torch.equal(xa, xb) and na == nb
