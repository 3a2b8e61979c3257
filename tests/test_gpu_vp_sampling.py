"""-m gpu: VP / sub-VP predictor-corrector sampling.  The reverse-diffusion update with a forward drift and the probability flow
against single updates of the reference classes, the fused device loop against the same classes driven step by step and against
the reference's own 6-step runs on the tiny networks (tests/golden/vp_sampling.npz, tools/make_vp_goldens.py), the step-wise
global-norm form, and the on-device noise."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from test_gpu_network import build, dev, rel  # noqa: E402
from test_gpu_steps import _Tape, step_score  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'vp_sampling.npz')
VP_KW = dict(beta_min=0.1, beta_max=20., N=1000)
VE_KW = dict(sigma_min=0.01, sigma_max=50., N=1000)
EPS, SNR = 1e-3, 0.075

_MODELS = {}


def model_for(case, precision='fp32'):
    if (case, precision) not in _MODELS:
        _MODELS[case, precision] = build(case, precision)
    return _MODELS[case, precision]


def vp_sde(scls):
    from conditional_score_diffusion_amd import sde_lib
    return getattr(sde_lib, scls)(**VP_KW)


# ---- 1. single updates against the reference classes ------------------------------------------------------------------------
STEP_CASES = [      # tools/make_vp_goldens.py:STEP_CASES
    ('vp_rd', 'VPSDE', VP_KW, 'reverse_diffusion', False, False),
    ('vp_rd_pf', 'VPSDE', VP_KW, 'reverse_diffusion', True, False),
    ('subvp_rd', 'subVPSDE', VP_KW, 'reverse_diffusion', False, False),
    ('subvp_rd_pf', 'subVPSDE', VP_KW, 'reverse_diffusion', True, False),
    ('cvp_crd', 'cVPSDE', VP_KW, 'conditional_reverse_diffusion', False, True),
    ('cvp_crd_pf', 'cVPSDE', VP_KW, 'conditional_reverse_diffusion', True, True),
    ('ve_rd_pf', 'VESDE', VE_KW, 'reverse_diffusion', True, False),
]


@pytest.mark.parametrize('name,scls,skw,reg,pf,cond', STEP_CASES)
def test_reverse_diffusion_step_vs_reference(name, scls, skw, reg, pf, cond):
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import predictors
    g = np.load(GOLD)
    x0, y0 = torch.from_numpy(g['x0']).to(dev()), torch.from_numpy(g['y0']).to(dev())
    z0 = torch.from_numpy(g['z0'])
    sde = getattr(sde_lib, scls)(**skw)
    for ti, tv in enumerate(g['times']):
        t = torch.full((x0.shape[0],), float(tv), device=dev())
        score_fn = (lambda x, y, t: step_score(x, t, y)) if cond else (lambda x, t: step_score(x, t))
        with _Tape([z0[0], z0[1]]) as tp:
            obj = predictors.get_predictor(reg)(sde, score_fn, pf)
            x, xm = obj.update_fn(x0.clone(), y0, t) if cond else obj.update_fn(x0.clone(), t)
            assert tp.i == 1                          # the probability flow consumes its draw as well
        if pf:
            assert torch.equal(x, xm)
        for got, key in ((x, 'x'), (xm, 'xmean')):
            ref = torch.from_numpy(g['%s_t%d_%s' % (name, ti, key)])
            err = (got.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)
            print('%s t%d %s: %.3e' % (name, ti, key, err))
            assert err < 5e-6, (name, ti, key, err)      # fp32 elementwise; coefficients rounded once on the host


def test_per_sample_times_are_refused():
    from conditional_score_diffusion_amd.sampling import predictors
    x0 = torch.zeros(2, 3, 8, 8, device=dev())
    obj = predictors.get_predictor('reverse_diffusion')(vp_sde('VPSDE'), lambda x, t: step_score(x, t), False)
    with pytest.raises(NotImplementedError):
        obj.update_fn(x0, torch.tensor([0.7, 0.2], device=dev()))


# ---- 2. the fused loop against the same classes driven step by step ---------------------------------------------------------------
LOOP_CASES = [      # network, SDE class, predictor, corrector, continuous, probability_flow
    ('uncond_tiny', 'VPSDE', 'reverse_diffusion', 'langevin', True, False),
    ('uncond_tiny', 'VPSDE', 'reverse_diffusion', 'none', True, True),
    ('uncond_tiny', 'VPSDE', 'ancestral_sampling', 'none', False, False),
    ('uncond_tiny', 'VPSDE', 'euler_maruyama', 'ald', True, False),
    ('uncond_tiny', 'subVPSDE', 'reverse_diffusion', 'none', True, False),
    ('uncond_tiny', 'subVPSDE', 'euler_maruyama', 'none', True, False),
    ('sr3_tiny', 'cVPSDE', 'conditional_reverse_diffusion', 'conditional_langevin', True, False),
    ('sr3_tiny', 'cVPSDE', 'conditional_euler_maruyama', 'conditional_none', True, False),
    # a VE pair that reaches the new kernel on a row-strided network output ([score_x | score_y] per sample)
    ('cmde_tiny', 'VE', 'conditional_reverse_diffusion', 'conditional_langevin', True, True),
]


@pytest.mark.parametrize('case,scls,pred_name,corr_name,continuous,pf', LOOP_CASES)
def test_fused_loop_matches_the_step_by_step_classes(case, scls, pred_name, corr_name, continuous, pf):
    from conditional_score_diffusion_amd import ops
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    n = 4
    cfg, nc, p, model = model_for(case)
    if scls == 'VE':
        from test_gpu_network import sdes_for
        sde = sdes_for(cfg)
    else:
        sde = vp_sde(scls)
    c_sde = sde['x'] if isinstance(sde, dict) else sde
    B = cases.CASES[case][1]
    cond = case != 'uncond_tiny'
    y = cases.case_y(case).to(dev()) if cond else None
    xs, ys = (B,) + tuple(cfg.data.shape_x), (B,) + tuple(cfg.data.shape_y)
    P, C = get_predictor(pred_name), get_corrector(corr_name)
    assert fused.fusable(model, sde, P, C, 1, pf, continuous)
    phases = (not pred_name.endswith('none')) + (not corr_name.endswith('none'))
    per_phase = [ys, xs] if isinstance(sde, dict) else [xs]
    tape = cases.tape([xs] + per_phase * (phases * n), 17)
    x_f, _, _ = fused.run(model, sde, xs, y, n, SNR, EPS, True, noise_tape=tape, predictor=P, corrector=C, probability_flow=pf,
                          continuous=continuous)
    sfn = mutils.get_score_fn(sde, model, conditional=cond, continuous=continuous)
    if cond:
        sfn = mutils.get_conditional_score_fn(sfn, 'x')
    with _Tape(tape[1:]) as tp:
        pred, corr = P(c_sde, sfn, pf), C(c_sde, sfn, SNR, 1)
        x = (tape[0] * (c_sde.sigma_max if scls == 'VE' else 1.0)).to(dev())
        ts = torch.linspace(c_sde.T, EPS, n)
        for i in range(n):
            vt = torch.ones(B, device=dev()) * ts[i]
            for obj in (corr, pred):
                if not cond:
                    x, xm = obj.update_fn(x, vt)
                    continue
                y_in = y
                if isinstance(sde, dict) and type(obj).__name__ not in ('conditionalNonePredictor', 'conditionalNoneCorrector'):
                    # the two-SDE loop redraws y_t for every update (sampling/conditional.py:104-116)
                    y_in = y + ops.scale_rows(torch.randn_like(y), sde['y'].marginal_prob(y, vt)[1])
                x, xm = obj.update_fn(x, y_in, vt)
        assert tp.i == len(tape) - 1                       # both paths consumed the same number of draws
    assert torch.isfinite(x_f).all()
    err = rel(xm.cpu().numpy(), x_f.cpu().numpy(), floor=1.0)
    print('%s %s %s/%s: fused vs step by step %.3e' % (case, scls, pred_name, corr_name, err))
    assert err < 1e-5


# ---- 3. the fused loop (through the samplers) against the reference's 6-step runs -------------------------------------------------
RUNS = [            # tools/make_vp_goldens.py:RUNS
    ('vp_rd_lang_c', 'uncond_tiny', 'VPSDE', 'reverse_diffusion', 'langevin', True, False),
    ('vp_rd_lang_d', 'uncond_tiny', 'VPSDE', 'reverse_diffusion', 'langevin', False, False),
    ('vp_rd_none_c', 'uncond_tiny', 'VPSDE', 'reverse_diffusion', 'none', True, False),
    ('vp_rd_none_d', 'uncond_tiny', 'VPSDE', 'reverse_diffusion', 'none', False, False),
    ('vp_rd_none_pf', 'uncond_tiny', 'VPSDE', 'reverse_diffusion', 'none', True, True),
    ('vp_anc_none_d', 'uncond_tiny', 'VPSDE', 'ancestral_sampling', 'none', False, False),
    ('vp_em_none_c', 'uncond_tiny', 'VPSDE', 'euler_maruyama', 'none', True, False),
    ('subvp_rd_none', 'uncond_tiny', 'subVPSDE', 'reverse_diffusion', 'none', True, False),
    ('cvp_crd_clang', 'sr3_tiny', 'cVPSDE', 'conditional_reverse_diffusion', 'conditional_langevin', True, False),
    ('cvp_crd_cnone', 'sr3_tiny', 'cVPSDE', 'conditional_reverse_diffusion', 'conditional_none', True, False),
    ('cvp_cem_cnone', 'sr3_tiny', 'cVPSDE', 'conditional_euler_maruyama', 'conditional_none', True, False),
]


def _sampler(cfg, case, sde, pred, corr, continuous, pf, p_steps):
    from conditional_score_diffusion_amd.sampling import conditional, unconditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    xs = (cases.CASES[case][1],) + tuple(cfg.data.shape_x)
    kw = dict(snr=SNR, p_steps=p_steps, c_steps=1, probability_flow=pf, continuous=continuous, denoise=True, eps=EPS)
    if case == 'uncond_tiny':
        fn = unconditional.get_pc_sampler(sde, xs, get_predictor(pred), get_corrector(corr), **kw)
        return xs, lambda model, **k: fn(model, **k)
    fn = conditional.get_pc_conditional_sampler(sde, xs, get_predictor(pred), get_corrector(corr), **kw)
    y = cases.case_y(case).to(dev())
    return xs, lambda model, **k: fn(model, y, **k)


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('name,case,scls,pred,corr,continuous,pf', RUNS)
def test_fused_loop_vs_reference_runs(name, case, scls, pred, corr, continuous, pf, precision):
    """error relative to max(|ref|max, 1); measured on the MI355X over the eleven runs: fp32 1.1e-7 .. 3.4e-7, fp16x3 6.1e-8 .. 2.5e-7"""
    g = np.load(GOLD)
    cfg, nc, p, model = model_for(case, precision)
    xs, sample = _sampler(cfg, case, vp_sde(scls), pred, corr, continuous, pf, 6)
    phases = (not pred.endswith('none')) + (not corr.endswith('none'))
    out, _ = sample(model, noise_tape=cases.tape([xs] * (1 + phases * 6)))
    err = rel(out.cpu().numpy(), g['run_' + name], floor=1.0)
    print('%s %s: fused vs the reference run %.3e' % (name, precision, err))
    assert err < 1e-3                                  # the project's contract
    if precision == 'fp32':
        assert err < 2e-4                              # what test_gpu_network.py holds its fp32 tiny trajectories to


# ---- 4. the step-wise global-norm form --------------------------------------------------------------------------------------------
def test_step_begin_end_reproduce_pc_sample_for_vp_langevin():
    """csd_pc_step_begin / csd_pc_step_end with global_batch == B and no exchange ARE csd_pc_sample (the bound of the VE assertion in
    test_gpu_sharded.py: 1e-6 of the prior's scale, which is 1 here)"""
    case = 'uncond_tiny'
    cfg, nc, p, model = model_for(case)
    B = cases.CASES[case][1]
    xs, sample = _sampler(cfg, case, vp_sde('VPSDE'), 'reverse_diffusion', 'langevin', True, False, 6)
    tape = cases.tape([xs] * 13, seed=91)
    a, _ = sample(model, noise_tape=tape)
    b, _ = sample(model, noise_tape=tape, global_norm=(lambda s: None, B))
    err = np.abs(a.cpu().numpy() - b.cpu().numpy()).max() / 1.0
    print('step_begin/step_end vs pc_sample (VP): %.3e' % err)
    assert torch.isfinite(a).all() and err < 1e-6


# ---- 5. on-device noise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,scls,pred,corr', [('uncond_tiny', 'VPSDE', 'reverse_diffusion', 'langevin'),
                                                 ('uncond_tiny', 'subVPSDE', 'reverse_diffusion', 'none'),
                                                 ('sr3_tiny', 'cVPSDE', 'conditional_euler_maruyama', 'conditional_langevin')])
def test_philox_path_is_reproducible(case, scls, pred, corr):
    cfg, nc, p, model = model_for(case)
    xs, sample = _sampler(cfg, case, vp_sde(scls), pred, corr, True, False, 6)
    a, _ = sample(model, seed=5)
    b, _ = sample(model, seed=5)
    c, _ = sample(model, seed=6)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert (a - c).abs().max().item() > 1e-2           # another key, another N(0, I) prior and other noise
