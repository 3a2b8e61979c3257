"""Host side of the fused denoising score-matching loss (no GPU): the per-sample tables (a, b, w) that losses._dsm_tables takes from the
score function through likelihood._Probe against closed forms, a float64 numpy restatement of  w * sum (a h + b z)^2  with those
tables against the reference's loss values (tests/golden/losses.npz) on the oracle's network output, and the refusals of the library
entries and of the Python route.

Exchanging a and b: in continuous time every score function of models/utils.py divides by exactly the std the perturbation uses, so
a == b (both 1 / std with likelihood weighting, both 1 without) and the exchange cannot change a value; it is observable in discrete
time only, where a comes from the sigma ladder and b from sigma(t) - test_exchanging_a_and_b_shows_in_discrete_time_only pins both
halves of that statement.  The other two mutations (g^2 dropped, the y segment given the x coefficients) are checked on every key of
losses.npz whose tables they change."""
import os
import types

import numpy as np
import pytest
import torch

import cases
import score_oracle as so

T = torch.tensor([0.83, 0.21, 0.5])
SMIN, SMAX, N, BMIN, BMAX = 0.01, 50.0, 1000, 0.1, 20.0


def _sde(name):
    from conditional_score_diffusion_amd import sde_lib
    return {'vesde': lambda: sde_lib.VESDE(SMIN, SMAX, N), 'vpsde': lambda: sde_lib.VPSDE(BMIN, BMAX, N),
            'subvpsde': lambda: sde_lib.subVPSDE(BMIN, BMAX, N), 'cvesde': lambda: sde_lib.cVESDE(SMIN, SMAX, N),
            'pair': lambda: {'x': sde_lib.cVESDE(SMIN, SMAX, N), 'y': sde_lib.VESDE(SMIN, 1.0, N)}}[name]()


def _closed(name, t, continuous, smax=SMAX):
    """(m, std of the perturbation, std the score function divides by, g^2) in float64"""
    t = t.double().numpy()
    if name in ('vesde', 'cvesde'):
        std = SMIN * (smax / SMIN) ** t
        g2 = std ** 2 * 2 * np.log(smax / SMIN)
        ladder = np.exp(np.linspace(np.log(SMIN), np.log(smax), N))
        return np.ones_like(t), std, std if continuous else ladder[np.round(t.astype(np.float32) * (N - 1)).astype(int)], g2
    lmc = -0.25 * t ** 2 * (BMAX - BMIN) - 0.5 * t * BMIN
    beta = BMIN + t * (BMAX - BMIN)
    if name == 'vpsde':
        std = np.sqrt(1 - np.exp(2 * lmc))
        betas = np.linspace(BMIN / N, BMAX / N, N)
        disc = np.sqrt(1 - np.cumprod(1 - betas))[(t.astype(np.float32) * (N - 1)).astype(int)]
        return np.exp(lmc), std, std if continuous else disc, beta
    std = 1 - np.exp(2 * lmc)          # subVPSDE: its score function takes the continuous std in both modes
    return np.exp(lmc), std, std, beta * (1 - np.exp(-2 * BMIN * t - (BMAX - BMIN) * t ** 2))


# (the two-SDE objective is likelihood-weighted only: an assertion of the factory)
@pytest.mark.parametrize('continuous', [True, False])
@pytest.mark.parametrize('reduce_mean', [True, False])
@pytest.mark.parametrize('name,lw', [(n, lw) for n in ['vesde', 'vpsde', 'subvpsde', 'cvesde', 'pair'] for lw in (True, False)
                                     if lw or n != 'pair'])
def test_tables_match_closed_forms(name, lw, reduce_mean, continuous):
    from conditional_score_diffusion_amd import losses
    B, numels = T.shape[0], ({'x': 75, 'y': 25} if name == 'pair' else {'x': 75})
    labels, tab = losses._dsm_tables(_sde(name), T, numels, 'positional', name in ('cvesde', 'pair'), reduce_mean, continuous, lw)
    r = (1.0 / sum(numels.values()) if reduce_mean else 0.5) / B
    for k in tab:
        m, std, sdiv, g2 = _closed('vesde' if name == 'pair' else name, T, continuous, 1.0 if k == 'y' else SMAX)
        np.testing.assert_allclose(tab[k]['m'].numpy(), m, rtol=2e-6)
        np.testing.assert_allclose(tab[k]['std'].numpy(), std, rtol=2e-5)
        a, b, w = (1 / sdiv, 1 / std, g2 * r) if lw else (std / sdiv, np.ones(B), np.full(B, r))
        np.testing.assert_allclose(tab[k]['a'].numpy(), a, rtol=3e-5)
        np.testing.assert_allclose(tab[k]['b'].numpy(), b, rtol=3e-5)
        np.testing.assert_allclose(tab[k]['w'].numpy(), w, rtol=3e-5)
    t = T.double().numpy()
    if name == 'vesde':          # the unconditional VE network is labelled by sigma
        want = _closed(name, T, continuous)[2]
    else:
        want = np.round(t.astype(np.float32) * (N - 1)) if (not continuous and name in ('cvesde', 'pair')) else t * (N - 1)
    np.testing.assert_allclose(labels.numpy(), want, rtol=2e-5)
    assert labels.dtype == torch.float32 and labels.shape == (B,)


def _oracle_case(case):
    """inputs of tests/golden/losses.npz (oracle/make_goldens.py:gen_losses) and the oracle's network forward"""
    cfg, B = cases.case_config(case)
    nc = so.NetCfg.from_config(cfg)
    p = so.synth_params(so.ddpm_param_shapes(nc), 0)
    rs = np.random.RandomState(11)
    xs, ys = (B,) + tuple(cfg.data.shape_x), (B,) + tuple(cfg.data.shape_y)
    x = torch.from_numpy(rs.uniform(0, 1, size=xs).astype(np.float32))
    y = cases.case_y(case)
    name = cfg.model.name
    tape = cases.tape([ys, xs] if name == 'ddpm_paired' else [xs], 3)
    z = {'y': tape[0], 'x': tape[1]} if name == 'ddpm_paired' else {'x': tape[0]}
    return cfg, nc, p, B, x, y, z


_NET = {}


def _network_output(case):
    """the oracle's flat per-sample output rows h on the perturbed input, once per case (it does not depend on lw / rm)"""
    if case not in _NET:
        from conditional_score_diffusion_amd import losses
        from test_gpu_network import sdes_for
        cfg, nc, p, B, x, y, z = _oracle_case(case)
        sde = sdes_for(cfg)
        t = torch.tensor([0.83, 0.21][:B]) * (1 - 1e-5) + 1e-5          # losses.py:124,190,217: t = rand * (T - eps) + eps
        pair = isinstance(sde, dict)
        numels = {'x': x[0].numel(), 'y': y[0].numel()} if pair else {'x': x[0].numel()}
        labels, tab = losses._dsm_tables(sde, t, numels, 'positional', cfg.model.name != 'ddpm', True, True, True)
        pert = lambda v, k: v * tab[k]['m'][:, None, None, None] + tab[k]['std'][:, None, None, None] * z[k]
        with torch.no_grad():
            if cfg.model.name == 'ddpm':
                h = {'x': so.ddpm_forward(p, nc, pert(x, 'x'), labels)}
            elif pair:
                h = so.paired_forward(p, nc, pert(x, 'x'), pert(y, 'y'), labels, sr3=False)
            else:
                h = {'x': so.paired_forward(p, nc, pert(x, 'x'), y, labels, sr3=True)}
        _NET[case] = (sde, t, numels, {k: v.reshape(B, -1).double().numpy() for k, v in h.items()},
                      {k: v.reshape(B, -1).double().numpy() for k, v in z.items()}, cfg.model.name != 'ddpm')
    return _NET[case]


def _restate(tab, h, z):
    """float64 numpy: sum_b sum_seg w_b sum_i (a_b h + b_b z)^2"""
    tot = 0.0
    for k in tab:
        a, b, w = (tab[k][c].double().numpy()[:, None] for c in 'abw')
        tot += float((w * (a * h[k] + b * z[k]) ** 2).sum())
    return tot


def _keys(case, sde):
    return [(lw, rm) for lw in (True, False) for rm in (True, False) if lw or not isinstance(sde, dict)]


@pytest.mark.parametrize('case', list(cases.CASES))
def test_restatement_reproduces_reference_losses(golden_dir, case):
    from conditional_score_diffusion_amd import losses
    g = np.load(os.path.join(golden_dir, 'losses.npz'))
    sde, t, numels, h, z, cond = _network_output(case)
    for lw, rm in _keys(case, sde):
        _, tab = losses._dsm_tables(sde, t, numels, 'positional', cond, rm, True, lw)
        ref = float(g['%s_lw%d_rm%d' % (case, lw, rm)])
        v = _restate(tab, h, z)
        print(case, lw, rm, v, ref)
        assert abs(v - ref) <= 2e-5 * abs(ref), (case, lw, rm, v, ref)


@pytest.mark.parametrize('case', list(cases.CASES))
def test_wrong_tables_miss_reference_losses(golden_dir, case):
    """g^2 dropped (every likelihood-weighted key) and the y segment given the x coefficients (every two-SDE key) miss the reference
    value by more than 10 x the 2e-5 the right tables meet"""
    from conditional_score_diffusion_amd import losses
    g = np.load(os.path.join(golden_dir, 'losses.npz'))
    sde, t, numels, h, z, cond = _network_output(case)
    checked = 0
    for lw, rm in _keys(case, sde):
        _, tab = losses._dsm_tables(sde, t, numels, 'positional', cond, rm, True, lw)
        ref = float(g['%s_lw%d_rm%d' % (case, lw, rm)])
        if lw:
            no_g2 = {k: dict(tab[k], w=torch.full_like(tab[k]['w'], float((1.0 / sum(numels.values()) if rm else 0.5) / t.shape[0])))
                     for k in tab}
            v = _restate(no_g2, h, z)
            assert abs(v - ref) > 10 * 2e-5 * abs(ref), ('g2 dropped', case, lw, rm, v, ref)
            checked += 1
        if isinstance(sde, dict):
            v = _restate({'x': tab['x'], 'y': tab['x']}, h, z)
            assert abs(v - ref) > 10 * 2e-5 * abs(ref), ('y <- x coefficients', case, lw, rm, v, ref)
            checked += 1
    assert checked >= 2


def test_exchanging_a_and_b_shows_in_discrete_time_only():
    from conditional_score_diffusion_amd import losses
    rs = np.random.RandomState(5)
    h, z = {'x': rs.standard_normal((3, 75))}, {'x': rs.standard_normal((3, 75))}
    for continuous in (True, False):
        _, tab = losses._dsm_tables(_sde('vesde'), T, {'x': 75}, 'positional', False, True, continuous, True)
        v = _restate(tab, h, z)
        sw = _restate({'x': dict(tab['x'], a=tab['x']['b'], b=tab['x']['a'])}, h, z)
        if continuous:
            assert abs(sw - v) <= 1e-6 * abs(v)
        else:
            assert abs(sw - v) > 10 * 2e-5 * abs(v)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _residual(segs, n_seg=None, net=0x1000, net_stride=100, d_out=0x2000, partials=0x3000, rows=0x4000, loss=0x5000, B=2):
    from conditional_score_diffusion_amd import _lib
    arr = (_lib.DsmSegment * max(len(segs), 1))()
    for i, s in enumerate(segs):
        arr[i].offset, arr[i].length = s.get('offset', 0), s.get('length', 10)
        arr[i].a, arr[i].b, arr[i].w, arr[i].z = s.get('a', 0x6000), s.get('b', 0x7000), s.get('w', 0x8000), s.get('z', None)
    l = _lib.lib()
    rc = l.csd_dsm_residual(net, net_stride, arr if segs else None, len(segs) if n_seg is None else n_seg, d_out, partials, rows, loss, B, 0,
                            None)
    return rc, l.csd_last_error().decode()


def test_library_refusals_name_the_cause():
    """every refusal comes before the device is touched (this machine may have none): the addresses are never dereferenced"""
    from conditional_score_diffusion_amd import _lib
    for kw, word in [(dict(segs=[{}], B=0), 'B'), (dict(segs=[{}], n_seg=0), 'n_seg'), (dict(segs=[{}, {}], n_seg=3), 'n_seg'),
                     (dict(segs=[{}], net=None), 'null'), (dict(segs=[{}], partials=None), 'null'), (dict(segs=[{}], loss=None), 'null'),
                     (dict(segs=[], n_seg=1), 'null'), (dict(segs=[{'a': None}]), 'null'),
                     (dict(segs=[{}], net=0x1002), 'misaligned'), (dict(segs=[{}], rows=0x4004), 'misaligned'),
                     (dict(segs=[{'w': 0x8001}]), 'misaligned'), (dict(segs=[{'z': 0x9002}]), 'misaligned'),
                     (dict(segs=[{'offset': 95, 'length': 10}]), 'beyond net_stride'), (dict(segs=[{'length': 0}]), 'beyond net_stride'),
                     (dict(segs=[{'offset': -4}]), 'beyond net_stride'),
                     (dict(segs=[{'offset': 0, 'length': 60}, {'offset': 50, 'length': 50}]), 'overlapping'),
                     (dict(segs=[{'offset': 50, 'length': 50}, {'offset': 0, 'length': 51}]), 'overlapping')]:
        rc, msg = _residual(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    l = _lib.lib()
    for args, word in [((0x1000, 0x2000, None, 0x3000, None, 0, 10), 'B'), ((None, 0x2000, None, 0x3000, None, 2, 10), 'null'),
                       ((0x1000, 0x2000, None, None, None, 2, 10), 'null'), ((0x1000, 0x2002, None, 0x3000, None, 2, 10), 'misaligned'),
                       ((0x1000, 0x2000, 0x2801, 0x3000, None, 2, 10), 'misaligned'), ((0x1000, 0x2000, None, 0x3000, None, 2, 0), 'per_sample')]:
        rc = l.csd_dsm_perturb(*args, 0, 0, None)
        assert rc == -1 and word in l.csd_last_error().decode(), (args, rc, l.csd_last_error())
    assert _lib.DSM_PARTS == int(__import__('re').search(r'#define CSD_DSM_PARTS (\d+)', open(os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'csd.h')).read()).group(1))


def test_python_refusals():
    from conditional_score_diffusion_amd import losses, sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    ve = sde_lib.VESDE(SMIN, SMAX, N)
    with pytest.raises(NotImplementedError, match='3 SDEs'):
        losses.get_general_sde_loss_fn({'x': ve, 'y': ve, 'z': ve}, True, conditional=True, fused=True)
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(NotImplementedError, match='planned training executor'):
        losses.get_sde_loss_fn(ve, True, fused=True)(torch.nn.Linear(1, 1), x)
    with pytest.raises(NotImplementedError, match='3-D classes'):
        losses.get_sde_loss_fn(ve, True, fused=True)(types.SimpleNamespace(arch=2), x)
    cfg, _ = cases.case_config('uncond_tiny')
    model = mutils.create_model(cfg)
    with pytest.raises(NotImplementedError, match='GPU tensors only'):
        losses.get_sde_loss_fn(ve, True, fused=True)(model, x)
    model.train_executor = 'operators'
    with pytest.raises(NotImplementedError, match='planned training executor'):
        losses.get_sde_loss_fn(ve, True, fused=True)(model, x)
    # the default route is untouched by the keyword
    assert losses.get_sde_loss_fn(ve, True).__code__.co_varnames[:2] == ('model', 'batch')
