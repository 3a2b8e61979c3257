"""Probability-flow likelihood on the MI355X: the csd_pf_ode_rhs kernel against a float64 restatement, and the fused likelihood path
against the generic autograd path and an oracle-driven scipy run."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases
import score_oracle as so


def _rhs(y, h, v, e, ns, a, c, B, D):
    from conditional_score_diffusion_amd._lib import check, current_stream, lib, ptr
    dev = y.device
    out = torch.full((B * D + B,), float('nan'), dtype=torch.float64, device=dev)
    sc = torch.empty(lib().csd_pf_ode_scratch_bytes(B, D), dtype=torch.uint8, device=dev)
    check(lib().csd_pf_ode_rhs(ptr(y), ptr(h), ptr(v), ptr(e), ns, ptr(a), ptr(c), ptr(out), B, D, ptr(sc), current_stream(dev)),
          'pf_ode_rhs')
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 3, 64])
@pytest.mark.parametrize('D,extra', [(3 * 16 * 16, 0), (75, 0), (3 * 20 * 20, 3 * 20 * 20), (1001, 7), (3 * 160 * 160, 0)])
@pytest.mark.parametrize('kind', ['Rademacher', 'Gaussian'])
def test_pf_ode_rhs_vs_float64(B, D, extra, kind):
    if B == 64 and D == 3 * 160 * 160 and kind == 'Gaussian':
        pytest.skip('one SR3-160-sized case per noise type is enough')
    rs = np.random.RandomState(B * 7 + D)
    ns = D + extra
    dev = torch.device('cuda:0')
    x = rs.standard_normal(B * D) * 3.0
    y = np.concatenate([x, rs.standard_normal(B)])
    h = rs.standard_normal((B, ns)).astype(np.float32)
    v = rs.standard_normal((B, D)).astype(np.float32)
    e = (rs.randint(0, 2, size=(B, ns)) * 2 - 1).astype(np.float32) if kind == 'Rademacher' else \
        rs.standard_normal((B, ns)).astype(np.float32)
    a = rs.standard_normal(B)
    c = rs.standard_normal(B) * 10
    T = lambda z, dt: torch.from_numpy(np.ascontiguousarray(z)).to(device=dev, dtype=dt)     # noqa: E731
    args = (T(y, torch.float64), T(h, torch.float32), T(v, torch.float32), T(e, torch.float32), ns, T(a, torch.float64),
            T(c, torch.float64), B, D)
    got = _rhs(*args)
    h64, v64, e64 = (torch.from_numpy(z).double() for z in (h[:, :D], v, e[:, :D]))
    a64, c64 = torch.from_numpy(a)[:, None], torch.from_numpy(c)[:, None]
    drift = a64 * torch.from_numpy(x).reshape(B, D) + c64 * h64
    logp = a64[:, 0] * (e64 * e64).sum(1) + c64[:, 0] * (v64 * e64).sum(1)
    assert torch.allclose(got[:B * D], drift.reshape(-1), rtol=1e-14, atol=1e-12)
    assert torch.allclose(got[B * D:], logp, rtol=1e-12, atol=1e-9)
    again = _rhs(*args)
    assert torch.equal(got, again)          # fixed-order reductions: the same bits every run


@pytest.mark.gpu
def test_pf_ode_state_converts():
    from conditional_score_diffusion_amd._lib import check, current_stream, lib, ptr
    dev = torch.device('cuda:0')
    B, D = 3, 77
    y = torch.from_numpy(np.random.RandomState(1).standard_normal(B * D + 4 * B)).to(dev)
    x32 = torch.empty(B * D, device=dev)
    l32 = torch.empty(B, device=dev)
    lab = y[B * D + 3 * B:]
    check(lib().csd_pf_ode_state(ptr(y), ctypes.c_void_p(lab.data_ptr()), ptr(x32), ptr(l32), B, D, current_stream(dev)), 'state')
    assert torch.equal(x32, y[:B * D].float()) and torch.equal(l32, lab.float())


class Generic(nn.Module):
    """hides a HIP network from the fused dispatch: the generic (autograd) likelihood path runs on it"""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.embedding_type = getattr(net, 'embedding_type', 'positional')

    def forward(self, x, labels):
        return self.net(x, labels)


class Oracle(nn.Module):
    """the CPU oracle as a score network (fp32 autograd)"""

    def __init__(self, fwd):
        super().__init__()
        self.fwd = fwd

    def forward(self, x, labels):
        return self.fwd(x, labels)


def _uncond():
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = cases.case_config('uncond_tiny')
    cfg.model.csd_precision = 'fp32'
    nc = so.NetCfg.from_config(cfg)
    p = so.synth_params(so.ddpm_param_shapes(nc), 0)
    model = mutils.create_model(cfg)
    model.load_state_dict(p)
    rs = np.random.RandomState(17)
    x = torch.from_numpy(rs.uniform(0, 1, size=(B,) + tuple(cfg.data.shape_x)).astype(np.float32))
    e = torch.from_numpy((rs.randint(0, 2, size=x.shape) * 2 - 1).astype(np.float32))
    return cfg, model.to('cuda:0').eval(), Oracle(lambda xx, ll: so.ddpm_forward(p, nc, xx, ll)), x, e


TOL = dict(rtol=1e-6, atol=1e-6, eps=1e-3)    # (tight enough that the solver's own error is far below the 1e-3 comparisons)


def _agree(r1, r2):
    (b1, z1, n1), (b2, z2, n2) = r1, r2
    assert (b1.cpu().double() - b2.cpu().double()).abs().max().item() <= 1e-3, (b1, b2)
    zr = (z1.cpu().double() - z2.cpu().double()).abs().max().item() / z2.cpu().double().abs().max().item()
    assert zr <= 1e-3, zr
    assert abs(n1 - n2) <= max(12, 0.02 * n2), (n1, n2)     # (two RK45 steps)


@pytest.mark.gpu
@pytest.mark.parametrize('sde_name', ['ve', 'vp', 'subvp'])
def test_fused_likelihood_matches_generic_and_oracle(sde_name):
    from conditional_score_diffusion_amd import likelihood, sde_lib
    cfg, model, oracle, x, e = _uncond()
    sde = {'ve': lambda: sde_lib.VESDE(0.01, 5.0, 1000), 'vp': lambda: sde_lib.VPSDE(0.1, 20., 1000),
           'subvp': lambda: sde_lib.subVPSDE(0.1, 20., 1000)}[sde_name]()
    fn = likelihood.get_likelihood_fn(sde, lambda v: v, **TOL)
    dev = torch.device('cuda:0')
    fused = fn(model, x.to(dev), epsilon=e.to(dev))
    generic = fn(Generic(model), x.to(dev), epsilon=e.to(dev))
    assert np.isfinite(fused[0].cpu().numpy()).all()
    _agree(fused, generic)
    if sde_name == 've':
        _agree(fused, fn(oracle, x, epsilon=e))


@pytest.mark.gpu
def test_conditional_likelihood_sr3():
    from conditional_score_diffusion_amd import likelihood, sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = cases.case_config('sr3_tiny')
    cfg.model.csd_precision = 'fp32'
    nc = so.NetCfg.from_config(cfg)
    p = so.synth_params(so.ddpm_param_shapes(nc), 0)
    model = mutils.create_model(cfg)
    model.load_state_dict(p)
    model = model.to('cuda:0').eval()
    rs = np.random.RandomState(19)
    x = torch.from_numpy(rs.uniform(0, 1, size=(B,) + tuple(cfg.data.shape_x)).astype(np.float32))
    y = cases.case_y('sr3_tiny')
    e = torch.from_numpy((rs.randint(0, 2, size=x.shape) * 2 - 1).astype(np.float32))
    sde = sde_lib.cVESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, cfg.model.num_scales)
    fn = likelihood.get_conditional_likelihood_fn(sde, lambda v: v, **TOL)
    dev = torch.device('cuda:0')
    fused = fn(model, x.to(dev), y.to(dev), epsilon=e.to(dev))

    class GenericPaired(nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, d, labels):
            return self.net(d, labels)

    generic = fn(GenericPaired(model), x.to(dev), y.to(dev), epsilon=e.to(dev))
    oracle = Oracle(lambda d, ll: so.paired_forward(p, nc, d['x'], d['y'], ll, sr3=True))
    ref = fn(oracle, x, y, epsilon=e)
    _agree(fused, generic)
    _agree(fused, ref)
