"""Build-container tool: run the IMPORTED REFERENCE's inpainter on the tiny unconditional network and write
tests/golden/inpaint_runs.npz.

    python tools/make_inpaint_goldens.py

Uses oracle/ref_import.py, oracle/cases.py and the helpers of oracle/make_goldens.py by import.  The fixture holds reference OUTPUTS
only (run_<name>): the network's parameters, the data, the masks and the noise tape are regenerated from seeds on either side.

Every run is the reference's get_pc_inpainter (sampling/unconditional.py:230-345) on `uncond_tiny` with an SDE of N = 6 steps,
eps = 1e-3, snr = 0.075, denoise, the data and the half-image mask of cases.inpaint_case() and the tape
cases.tape([shape] * (1 + (phases + 2) * 6)): the prior, then per step [z_corrector] z_blend [z_predictor] z_blend.

The VP / sub-VP SDEs run with beta_min = 0.1, beta_max = 5: the inpainter takes sde.N steps, and the discrete betas beta_max / N of
the usual beta_max = 20 exceed 1 at N = 6 (alphas < 0, the reverse-diffusion drift sqrt(alpha) is NaN).

`ve_rd_lang_chmask` has the Haar multi-scale model's mask: [1, 3, 1, 1] with the values (1, 0, 0) - the first channel is known.

Not pinned, because the reference raises there:
  subVPSDE with the langevin / ald corrector: the class has no `alphas` (AttributeError, sampling/correctors.py:63-65,128-130)
  ancestral sampling on subVPSDE: refused by the constructor (sampling/predictors.py:111-113)
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

OUT = os.path.join(ROOT, 'tests', 'golden', 'inpaint_runs.npz')
N, EPS, SNR = 6, 1e-3, 0.075
VP_KW = dict(beta_min=0.1, beta_max=5.)
RUNS = [            # name, SDE class, predictor, corrector, continuous, channel mask
    ('vp_rd_lang_c', 'VPSDE', 'reverse_diffusion', 'langevin', True, False),
    ('vp_rd_lang_d', 'VPSDE', 'reverse_diffusion', 'langevin', False, False),
    ('vp_anc_none_d', 'VPSDE', 'ancestral_sampling', 'none', False, False),
    ('subvp_rd_none', 'subVPSDE', 'reverse_diffusion', 'none', True, False),
    ('ve_rd_none', 'VESDE', 'reverse_diffusion', 'none', True, False),
    ('ve_rd_lang_chmask', 'VESDE', 'reverse_diffusion', 'langevin', True, True),
]


def make_sde(sl, scls, cfg):
    if scls == 'VESDE':
        return sl.VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, N)
    return getattr(sl, scls)(VP_KW['beta_min'], VP_KW['beta_max'], N)


def channel_mask():
    return torch.tensor([1., 0., 0.]).reshape(1, 3, 1, 1)


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    sl, pr, co = ref['sde_lib'], ref['sampling.predictors'], ref['sampling.correctors']
    cfg, B, data, mask, _ = cases.inpaint_case()
    model, _ = mg.build_ref_model(ref, cfg)
    model.embedding_type = 'positional'
    out = {}
    for name, scls, pred, corr, continuous, chmask in RUNS:
        sde = make_sde(sl, scls, cfg)
        phases = (pred != 'none') + (corr != 'none')
        tp = cases.tape([tuple(data.shape)] * (1 + (phases + 2) * N))
        m = channel_mask() if chmask else mask
        fn = ref['sampling.unconditional'].get_pc_inpainter(sde, pr.get_predictor(pred), co.get_corrector(corr), snr=SNR, n_steps=1,
                                                            probability_flow=False, continuous=continuous, denoise=True, eps=EPS)
        with ref_import.TapeRandn(tp) as tr:
            res, _ = fn(model, data.clone(), m.clone())
            assert tr.i == len(tp), (name, tr.i, len(tp))
        assert torch.isfinite(res).all(), name
        out['run_' + name] = res.numpy()
        print(name, 'max |x|', float(res.abs().max()))
    np.savez_compressed(OUT, **out)
    print('inpaint_runs.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
