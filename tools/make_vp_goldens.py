"""Build-container tool: run the IMPORTED REFERENCE on the VP / sub-VP sampling cases and write tests/golden/vp_sampling.npz.

    python tools/make_vp_goldens.py

Uses oracle/ref_import.py, oracle/cases.py and the helpers of oracle/make_goldens.py by import.  The fixture holds inputs by seed,
reference OUTPUTS and the reference's per-step fp32 scalars - no reference source text.

  (a) single reverse-diffusion updates of the reference classes (closed-form score, noise tape; the recipe of gen_steps):
      <name>_t<i>_x / _xmean
  (b) 6-step PC runs of the reference on the tiny networks (eps = 1e-3, snr = 0.075, denoise, the tape of cases.tape): run_<name>
  (c) the per-step scalars of each schedule, evaluated per step at a [B] time vector like the reference's loop: sc_<schedule>_<what>

Not pinned, because the reference raises there:
  subVPSDE with the langevin / ald corrector: the class has no `alphas` (AttributeError, sampling/correctors.py:63-65,128-130)
  conditional_ancestral_sampling: update_fn(self, x, t) is called with (x, y, t) (TypeError, sampling/predictors.py:175-179)
  probability-flow Euler-Maruyama: indexes a Python float (TypeError, sampling/predictors.py:62)
  ancestral sampling on subVPSDE / with a probability flow: refused by the constructor (sampling/predictors.py:111-113)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
import cases  # noqa: E402
import make_goldens as mg  # noqa: E402
import ref_import  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'vp_sampling.npz')
VP_KW = dict(beta_min=0.1, beta_max=20., N=1000)
VE_KW = dict(sigma_min=0.01, sigma_max=50., N=1000)

STEP_CASES = [      # name, SDE class, kwargs, registry name, probability_flow, conditional
    ('vp_rd', 'VPSDE', VP_KW, 'reverse_diffusion', False, False),
    ('vp_rd_pf', 'VPSDE', VP_KW, 'reverse_diffusion', True, False),
    ('subvp_rd', 'subVPSDE', VP_KW, 'reverse_diffusion', False, False),
    ('subvp_rd_pf', 'subVPSDE', VP_KW, 'reverse_diffusion', True, False),
    ('cvp_crd', 'cVPSDE', VP_KW, 'conditional_reverse_diffusion', False, True),
    ('cvp_crd_pf', 'cVPSDE', VP_KW, 'conditional_reverse_diffusion', True, True),
    ('ve_rd_pf', 'VESDE', VE_KW, 'reverse_diffusion', True, False),
]

P_STEPS, EPS, SNR = 6, 1e-3, 0.075
RUNS = [            # name, tiny network, SDE class, predictor, corrector, continuous, probability_flow
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
SCHEDULES = [('vp_c', 'VPSDE', True), ('vp_d', 'VPSDE', False), ('subvp', 'subVPSDE', True), ('cvp_c', 'cVPSDE', True)]


def gen_single_steps(ref, out):
    sl, pr = ref['sde_lib'], ref['sampling.predictors']
    g = torch.Generator().manual_seed(77)               # (the input recipe of make_goldens.gen_steps)
    B, C, S = 3, 3, 8
    x0 = torch.randn(B, C, S, S, generator=g) * 2.0
    y0 = torch.rand(B, C, S, S, generator=g)
    z0 = torch.randn(2, B, C, S, S, generator=g)
    out.update(x0=x0.numpy(), y0=y0.numpy(), z0=z0.numpy(), times=np.array(mg.STEP_TIMES, np.float32))
    for name, scls, skw, reg, pf, cond in STEP_CASES:
        sde = getattr(sl, scls)(**skw)
        for ti, tv in enumerate(mg.STEP_TIMES):
            t = torch.full((B,), tv)
            score_fn = (lambda x, y, t: mg.step_score(x, t, y)) if cond else (lambda x, t: mg.step_score(x, t))
            with ref_import.TapeRandn([z0[0], z0[1]]) as tr:
                obj = pr.get_predictor(reg)(sde, score_fn, pf)
                x, xm = obj.update_fn(x0.clone(), y0, t) if cond else obj.update_fn(x0.clone(), t)
                assert tr.i == 1                        # (a probability-flow predictor still consumes its draw)
            out['%s_t%d_x' % (name, ti)] = x.numpy()
            out['%s_t%d_xmean' % (name, ti)] = xm.numpy()


def gen_runs(ref, out):
    sl, pr, co = ref['sde_lib'], ref['sampling.predictors'], ref['sampling.correctors']
    models = {}
    for name, case, scls, pred, corr, continuous, pf in RUNS:
        cfg, B = cases.case_config(case)
        if case not in models:
            models[case] = mg.build_ref_model(ref, cfg)[0]
        model = models[case]
        sde = getattr(sl, scls)(VP_KW['beta_min'], VP_KW['beta_max'], cfg.model.num_scales)
        xs = (B,) + tuple(cfg.data.shape_x)
        phases = (not pred.endswith('none')) + (not corr.endswith('none'))
        tp = cases.tape([xs] * (1 + phases * P_STEPS))
        with ref_import.TapeRandn(tp) as tr, torch.no_grad():
            if case == 'uncond_tiny':
                fn = ref['sampling.unconditional'].get_pc_sampler(sde, xs, pr.get_predictor(pred), co.get_corrector(corr), snr=SNR,
                                                                  p_steps=P_STEPS, c_steps=1, probability_flow=pf,
                                                                  continuous=continuous, denoise=True, eps=EPS)
                res, _ = fn(model)
            else:
                fn = ref['sampling.conditional'].get_pc_conditional_sampler(sde, xs, pr.get_predictor(pred), co.get_corrector(corr),
                                                                            snr=SNR, p_steps=P_STEPS, c_steps=1,
                                                                            probability_flow=pf, continuous=continuous,
                                                                            denoise=True, use_path=False, eps=EPS)
                res, _ = fn(model, cases.case_y(case))
            assert tr.i == len(tp), (name, tr.i, len(tp))
        assert torch.isfinite(res).all(), name
        out['run_' + name] = res.numpy()
        print(name, 'max |x|', float(res.abs().max()))


def gen_scalars(ref, out):
    """what the reference's loop evaluates per step (sampling/unconditional.py:207-213) for a batch of 2"""
    sl = ref['sde_lib']
    for key, scls, continuous in SCHEDULES:
        sde = getattr(sl, scls)(**VP_KW)
        ts = torch.linspace(sde.T, EPS, P_STEPS)
        rows = {k: [] for k in ('label', 'std', 'drift', 'G', 'alpha', 'beta', 'phi', 'g')}
        one, zero = torch.ones(2, 1, 1, 1), torch.zeros(2, 1, 1, 1)
        for i in range(P_STEPS):
            t = torch.ones(2) * ts[i]
            labels = t * (sde.N - 1)                                      # models/utils.py:198,234
            timestep = (t * (sde.N - 1) / sde.T).long()
            if continuous or scls == 'subVPSDE':
                std = sde.marginal_prob(zero, t)[1]
            else:
                std = sde.sqrt_1m_alphas_cumprod.type_as(labels)[labels.long()]
            phi, g = sde.sde(one, t)
            if scls == 'subVPSDE':          # Euler default discretisation: f = (phi*x)*dt; no DDPM tables
                drift, alpha, beta = phi.flatten(), torch.full((2,), float('nan')), torch.full((2,), float('nan'))
            else:                           # f = sqrt(alpha_i)*x - x
                alpha, beta = sde.alphas[timestep], sde.discrete_betas[timestep]
                drift = torch.sqrt(alpha)
            G = sde.discretize(zero, t)[1]
            for k, v in (('label', labels), ('std', std), ('drift', drift), ('G', G), ('alpha', alpha), ('beta', beta),
                         ('phi', phi.flatten()), ('g', g)):
                assert v.dtype == torch.float32 and bool((v == v[0]).all() or torch.isnan(v).all()), (key, k)
                rows[k].append(float(v[0]))
        out['sc_%s_t' % key] = ts.numpy()
        for k, v in rows.items():
            out['sc_%s_%s' % (key, k)] = np.array(v, np.float64).astype(np.float32)


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    out = {}
    gen_single_steps(ref, out)
    gen_runs(ref, out)
    gen_scalars(ref, out)
    np.savez_compressed(OUT, **out)
    print('vp_sampling.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
