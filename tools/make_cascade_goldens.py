"""Build-container tool: run the IMPORTED REFERENCE's samplers stage by stage on the seeded cascade cases of tests/cascade_cases.py and
write tests/golden/cascade.npz.

    python tools/make_cascade_goldens.py

Uses oracle/ref_import.py, oracle/make_goldens.py (build_ref_model) and tests/cascade_cases.py by import.  Per flow and stage the
reference's own sampler runs on the stage's seeded tape (ref_import.TapeRandn), exactly as tools/make_sr_goldens.py and
tools/make_wide_goldens.py run one stage:

  bicubic       sampling.conditional.get_pc_conditional_sampler on DDPM_2xSR (R1, then R2 on R1's result)
  haar          the same sampler on ddpm_paired 9 + 3; the next low band is haar_backward(cat(dc, hf))
  haar_inpaint  sampling.unconditional.get_pc_inpainter on ddpm with 12 bands, data = (dc | zeros), mask [1, 12, 1, 1]

THE MERGE BETWEEN HAAR STAGES IS A RESTATEMENT, NOT THE REFERENCE: the reference's transform layer (iunets' InvertibleDownsampling2D)
cannot be imported here, so ``cascade_cases.merge64`` (float64 conv_transpose2d with the orthonormal Haar matrix, band-major channels)
stands in for ``haar_backward``; its result is rounded to float32 before it becomes the next stage's condition, which is what the
reference's fp32 layer would hand on.  The fixture holds every stage's image: ``<flow>_s<k>``, float32.

It also prints each stage's distance to the float64 restatement ``cascade_cases.cascade64`` and to its two wrong restatements, in units
of the stage's sigma_max_x (tests/test_cascade_host.py asserts them).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]
import cascade_cases as cc  # noqa: E402
import make_goldens as mg  # noqa: E402
import ref_import  # noqa: E402


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    sl, pr, co = ref['sde_lib'], ref['sampling.predictors'], ref['sampling.correctors']
    out = {}
    for flow in cc.FLOWS:
        cur = cc.lr_input(flow)
        for k in range(cc.N_STAGES):
            cfg = cc.stage_config(flow, k)
            m = cfg.model
            model, _ = mg.build_ref_model(ref, cfg)
            tp = cc.tape(flow, k)
            with ref_import.TapeRandn(tp) as tr, torch.no_grad():
                if flow == 'haar_inpaint':
                    model.embedding_type = 'positional'
                    sde = sl.VESDE(m.sigma_min_x, m.sigma_max_x, cc.P_STEPS)
                    fn = ref['sampling.unconditional'].get_pc_inpainter(sde, pr.get_predictor(cfg.sampling.predictor),
                                                                      co.get_corrector(cfg.sampling.corrector), snr=cfg.sampling.snr, n_steps=1,
                                                                      probability_flow=False, continuous=True, denoise=True, eps=cc.EPS)
                    data = torch.cat([cur, torch.zeros(cc.B, 9, cur.shape[2], cur.shape[3])], dim=1)
                    mask = torch.zeros(1, 12, 1, 1)
                    mask[:, :3] = 1.
                    bands, _ = fn(model, data, mask)
                    assert tuple(bands.shape) == cc.state_shape(flow, k)
                    cur = cc.merge64(data[:, :3], bands[:, 3:]).float()
                else:
                    sde = {'x': sl.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sl.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
                    fn = ref['sampling.conditional'].get_pc_conditional_sampler(
                        sde, cc.state_shape(flow, k), pr.get_predictor(cfg.sampling.predictor), co.get_corrector(cfg.sampling.corrector),
                        snr=cfg.sampling.snr, p_steps=cc.P_STEPS, c_steps=1, probability_flow=False, continuous=True, denoise=True,
                        use_path=False, eps=cc.EPS)
                    x, _ = fn(model, cur)
                    assert tuple(x.shape) == cc.state_shape(flow, k)
                    cur = x if flow == 'bicubic' else cc.merge64(cur, x).float()
                assert tr.i == len(tp), (flow, k, tr.i, len(tp))
            assert torch.isfinite(cur).all() and tuple(cur.shape) == cc.image_shape(flow, k), (flow, k, tuple(cur.shape))
            out['%s_s%d' % (flow, k)] = cur.numpy().astype(np.float32)
        with torch.no_grad():
            for mangle in (None, 'squeeze' if flow == 'bicubic' else 'bands'):
                images = cc.cascade64(flow, mangle)
                d = [float((torch.from_numpy(out['%s_s%d' % (flow, k)]).double() - images[k]).abs().max()) / cc.sigma_max(flow, k)
                     for k in range(cc.N_STAGES)]
                print('%s: reference vs float64 restatement%s, per stage in units of sigma_max_x: %s; max |image| %s'
                      % (flow, ' (%s exchanged)' % mangle if mangle else '', ', '.join('%.3e' % v for v in d),
                         ', '.join('%.2f' % float(np.abs(out['%s_s%d' % (flow, k)]).max()) for k in range(cc.N_STAGES))))
    np.savez_compressed(cc.GOLDEN, **out)
    print('cascade.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(cc.GOLDEN)))


if __name__ == '__main__':
    main()
