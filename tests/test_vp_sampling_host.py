"""VP / sub-VP predictor-corrector sampling on the fused device loop, host side: the per-step tables the loop is handed against the
reference's own per-step fp32 scalars (tests/golden/vp_sampling.npz part (c), tools/make_vp_goldens.py) and the dispatch."""
import os

import numpy as np
import pytest
import torch

import cases

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'vp_sampling.npz')
P_STEPS, EPS, SNR = 6, 1e-3, 0.075
ULP = 1.2e-7        # both sides evaluate the same fp32 torch expressions: only the float -> Python -> fp32 hand-over can differ


def _close(got, ref, what, bound=ULP):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref) / np.abs(ref)
    assert err.max() <= bound, (what, err.max())


def _sde(key):
    from conditional_score_diffusion_amd import sde_lib
    cls = {'vp_c': sde_lib.VPSDE, 'vp_d': sde_lib.VPSDE, 'subvp': sde_lib.subVPSDE, 'cvp_c': sde_lib.cVPSDE}[key]
    return cls(beta_min=0.1, beta_max=20., N=1000), key != 'vp_d'


@pytest.mark.parametrize('key', ['vp_c', 'vp_d', 'subvp', 'cvp_c'])
def test_step_tables_match_the_reference_scalars(key):
    from conditional_score_diffusion_amd.sampling import correctors as C, fused, predictors as P
    g = np.load(GOLD)
    ref = {k: g['sc_%s_%s' % (key, k)] for k in ('t', 'label', 'std', 'drift', 'G', 'alpha', 'beta', 'phi', 'g')}
    sde, continuous = _sde(key)
    ts, labels, std_x, G, std_y = fused.step_scalars(sde, P_STEPS, EPS, 'sigma', continuous)
    assert std_y is None and labels.dtype == std_x.dtype == G.dtype == torch.float32
    assert np.array_equal(ts.numpy(), ref['t'])
    _close(labels, ref['label'], 'label')           # t*(N-1), not sigma(t) and not rounded in discrete time either
    _close(std_x, ref['std'], 'std')
    _close(G, ref['G'], 'G')
    tab, sub_x = fused.reverse_diffusion_table(sde, ts)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (P_STEPS, 2)
    _close(tab[:, 0], ref['drift'], 'drift')
    if key == 'subvp':
        assert sub_x == 0 and bool((tab[:, 1] == np.float32(1.0 / sde.N)).all())
        with pytest.raises(AttributeError):         # no `alphas`: the Langevin / ALD step size raises, as the reference's does
            fused.langevin_alphas(sde, ts)
        with pytest.raises(AttributeError):
            fused.rule_tables(sde, ts, P.NonePredictor, C.AnnealedLangevinDynamics, SNR, False)
    else:
        assert sub_x == 1 and bool((tab[:, 1] == 1.0).all())
        _close(fused.langevin_alphas(sde, ts), ref['alpha'], 'alpha')
        beta = ref['beta'].astype(np.float64)
        anc = np.stack([1.0 / np.sqrt(1.0 - beta), beta / np.sqrt(1.0 - beta), np.sqrt(beta)], 1)
        pa, ca = (P.conditionalAncestralSamplingPredictor, C.conditionalAnnealedLangevinDynamics) if key == 'cvp_c' else \
                 (P.AncestralSamplingPredictor, C.AnnealedLangevinDynamics)
        pid, cid, pred, corr = fused.rule_tables(sde, ts, pa, ca, SNR, False)
        assert (pid, cid) == (1, 1)
        _close(pred, anc, 'ancestral table')
        m_std = np.array([float(sde.marginal_prob(torch.zeros(1, 1), ts[i:i + 1])[1][0]) for i in range(P_STEPS)])
        if continuous:
            _close(m_std, ref['std'], 'marginal std')
        step = (SNR * m_std) ** 2 * 2 * ref['alpha'].astype(np.float64)
        _close(corr, np.stack([np.ones(P_STEPS), step, np.sqrt(2 * step)], 1), 'ald table')
    # Euler-Maruyama: 1 + phi*dt, g^2*dt (half of it and no noise for the probability flow), g*sqrt(dt)
    phi, gg, dt = ref['phi'].astype(np.float64), ref['g'].astype(np.float64), 1.0 / sde.N
    pe = P.conditionalEulerMaruyamaPredictor if key == 'cvp_c' else P.EulerMaruyamaPredictor
    for pf in (False, True):
        _, _, pred, _ = fused.rule_tables(sde, ts, pe, C.NoneCorrector, SNR, pf)
        em = np.stack([1.0 - phi * dt, (0.5 if pf else 1.0) * gg * gg * dt, gg * np.sqrt(dt)], 1)
        _close(pred[:, 0], em[:, 0], 'em drift')
        # g = sqrt(beta(t)) is a sqrt evaluated on THIS host: fp32 torch.sqrt differs by one ulp between CPUs (measured: two AVX512
        # hosts), g*g doubles that and the hand-over adds half an ulp -> 3 ulp for the two columns built from g
        _close(pred[:, 1], em[:, 1], 'em score', 3 * ULP)
        if pf:
            assert float(pred[:, 2].abs().max()) == 0.0
        else:
            _close(pred[:, 2], em[:, 2], 'em noise', 3 * ULP)


def test_reverse_diffusion_drift_is_exact_for_vp():
    """sqrt(alpha_i) comes back bit-exact from the one evaluation of discretize at x = 1 (the difference to 1 is exact in fp32)"""
    from conditional_score_diffusion_amd.sampling.predictors import reverse_diffusion_drift
    sde, _ = _sde('vp_c')
    for tv in (1.0, 0.73, 0.31, 1e-3, 1e-4):
        t1 = torch.tensor([tv])
        a, b, sub_x = reverse_diffusion_drift(sde, t1)
        i = int((t1 * (sde.N - 1) / sde.T).long()[0])
        assert np.float32(a) == torch.sqrt(sde.alphas[i]).numpy() and a == float(np.float32(a)) and b == 1.0 and sub_x
    from conditional_score_diffusion_amd import sde_lib
    assert reverse_diffusion_drift(sde_lib.VESDE(0.01, 50., 1000), torch.tensor([0.5])) is None


def test_fusable_truth_table():
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector as gc
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor as gp
    un = mutils.create_model(cases.case_config('uncond_tiny')[0])
    sr3 = mutils.create_model(cases.case_config('sr3_tiny')[0])
    cmde = mutils.create_model(cases.case_config('cmde_tiny')[0])
    vp, sub, cvp = sde_lib.VPSDE(0.1, 20., 1000), sde_lib.subVPSDE(0.1, 20., 1000), sde_lib.cVPSDE(0.1, 20., 1000)
    ve, cve = sde_lib.VESDE(0.01, 50., 1000), sde_lib.cVESDE(0.01, 50., 1000)

    def f(model, sde, pred, corr, c_steps=1, pf=False, continuous=True, **kw):
        return fused.fusable(model, sde, gp(pred), gc(corr), c_steps, pf, continuous, **kw)

    # VPSDE: every predictor, continuous and discrete, with langevin / ald / none
    for pred in ('reverse_diffusion', 'euler_maruyama', 'ancestral_sampling', 'none'):
        for corr in ('langevin', 'ald', 'none'):
            for continuous in (True, False):
                assert f(un, vp, pred, corr, continuous=continuous) == ((pred, corr) != ('none', 'none')), (pred, corr)
    assert f(un, vp, 'reverse_diffusion', 'none', pf=True) and f(un, vp, 'euler_maruyama', 'langevin', pf=True)
    # cVPSDE
    for pred in ('conditional_reverse_diffusion', 'conditional_euler_maruyama'):
        for corr in ('conditional_langevin', 'conditional_ald', 'conditional_none'):
            assert f(sr3, cvp, pred, corr) and f(sr3, cvp, pred, corr, continuous=False)
    assert f(sr3, cvp, 'conditional_reverse_diffusion', 'conditional_langevin', pf=True)
    # subVPSDE: reverse diffusion and Euler-Maruyama without a corrector
    for pred in ('reverse_diffusion', 'euler_maruyama'):
        assert f(un, sub, pred, 'none') and f(un, sub, pred, 'none', pf=True) and f(un, sub, pred, 'none', continuous=False)
        assert not f(un, sub, pred, 'langevin') and not f(un, sub, pred, 'ald')          # no `alphas`
    assert not f(un, sub, 'ancestral_sampling', 'none')
    assert not f(un, sub, 'none', 'langevin')
    # refused for everyone
    assert not f(un, vp, 'reverse_diffusion', 'langevin', c_steps=2)
    assert not f(un, vp, 'ancestral_sampling', 'none', pf=True)
    assert not f(sr3, cvp, 'conditional_ancestral_sampling', 'conditional_none', pf=True)
    assert not f(un, vp, 'reverse_diffusion', 'langevin', use_path=True)
    # {'x', 'y'} dicts with VP members: the reference refuses them (models/utils.py:171-188)
    assert not f(cmde, {'x': cvp, 'y': ve}, 'conditional_reverse_diffusion', 'conditional_langevin')
    assert not f(cmde, {'x': cve, 'y': vp}, 'conditional_reverse_diffusion', 'conditional_langevin')
    assert not f(cmde, {'x': cvp, 'y': vp}, 'conditional_reverse_diffusion', 'conditional_langevin')
    # VE: as before, continuous only, and now with the probability flow of the reverse-diffusion predictor
    assert f(un, ve, 'reverse_diffusion', 'langevin') and not f(un, ve, 'reverse_diffusion', 'langevin', continuous=False)
    assert f(cmde, {'x': cve, 'y': ve}, 'conditional_reverse_diffusion', 'conditional_langevin', pf=True)
    assert f(sr3, cve, 'conditional_euler_maruyama', 'conditional_none', pf=True)
    assert not f(sr3, cve, 'conditional_ancestral_sampling', 'conditional_ald', pf=True)
    assert not f(torch.nn.Identity(), vp, 'reverse_diffusion', 'langevin')


def test_zero_initialised_params_mean_the_ve_pair():
    """bench.py and the sharded test fill a fresh PCParams with the old fields only: the appended ones must default to 'absent'"""
    from conditional_score_diffusion_amd import _lib
    p = _lib.PCParams()
    assert not p.rd_drift and p.rd_sub_x == 0 and p.probability_flow == 0
    names = [n for n, _ in _lib.PCParams._fields_]
    assert names[-3:] == ['rd_drift', 'rd_sub_x', 'probability_flow'] and names[-4] == 'corr_alpha'      # appended, nothing moved
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'csd.h')).read()
    body = hdr[hdr.index('typedef struct csd_pc_params {'):hdr.index('} csd_pc_params;')]
    import re
    assert re.findall(r'^\s+(?:const )?[a-z0-9_]+\*? ([a-z0-9_A-Z]+);', body, flags=re.M) == names
