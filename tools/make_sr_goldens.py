"""Build-container tool: run the IMPORTED REFERENCE's DDPM_2xSR (models/ddpm.py:39-52,300-314), its conditional PC sampler and autograd
on the seeded cases of tests/sr_cases.py and write tests/golden/sr2x.npz.

    python tools/make_sr_goldens.py

Uses oracle/ref_import.py (SqueezeBlock is plain torch: it imports like the rest of models/ddpm.py), oracle/cases.py,
oracle/score_oracle.py and oracle/make_goldens.py (build_ref_model) by import.  The fixture holds reference OUTPUTS only; parameters
(score_oracle.synth_params(shapes, 0)), inputs, labels and noise tapes are regenerated from seeds on either side:

  <case>_x<j>, <case>_y<j>   the network's two outputs ([B, c, 2S, 2S] and [B, cy, S, S]) at t = sr_cases.FORWARD_TIMES[j]
  <case>_pc                  get_pc_conditional_sampler on the pair {'x': cVESDE, 'y': VESDE}: conditional reverse diffusion +
                             conditional Langevin, P_STEPS steps, continuous, denoise (SAMPLER_CASES)
  <case>_path                the same with use_path = True (PATH_CASE)
  <case>_loss / _names / _norms / _samples
                             the training loss (losses.get_general_sde_loss_fn, train = True, dropout 0) and per parameter the
                             gradient's L2 norm and its values at cases.grad_sample_index - the layout of tests/golden/grads.npz

It also checks the float64 restatement sr_cases.forward64 against the reference's fp32 output and prints the distance.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]
import cases  # noqa: E402
import make_goldens as mg  # noqa: E402
import ref_import  # noqa: E402
import sr_cases as sc  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def sdes_for(ref, cfg):
    sl, m = ref['sde_lib'], cfg.model
    return {'x': sl.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sl.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    L, pr, co = ref['losses'], ref['sampling.predictors'], ref['sampling.correctors']
    out = {}
    for case in sc.CASES:
        cfg = sc.make_config(case)
        model, p = mg.build_ref_model(ref, cfg)
        assert type(model).__name__ == 'DDPM_2xSR'
        sde = sdes_for(ref, cfg)
        y = sc.case_y(case)
        with torch.no_grad():
            for j, (x, t) in enumerate(sc.forward_inputs(case)):
                labels = sc.labels_of(cfg, t)
                net = model({'x': x, 'y': y}, labels)
                wx, wy = sc.forward64(p, case, x, y, labels)
                e = max(rel(net['x'], wx), rel(net['y'], wy))
                assert torch.isfinite(net['x']).all() and torch.isfinite(net['y']).all() and e < 1e-5, (case, j, e)
                out['%s_x%d' % (case, j)], out['%s_y%d' % (case, j)] = net['x'].numpy(), net['y'].numpy()
            print('case %s: out %s | %s, fp32 reference vs float64 restatement %.2e' % (case, tuple(net['x'].shape), tuple(net['y'].shape), e))
            xs = sc.shapes(case)[0]
            for key, use_path, tp in (('_pc', False, sc.pc_tape(case) if case in sc.SAMPLER_CASES else None),
                                      ('_path', True, sc.path_tape(case) if case == sc.PATH_CASE else None)):
                if tp is None:
                    continue
                fn = ref['sampling.conditional'].get_pc_conditional_sampler(
                    sde, xs, pr.get_predictor(cfg.sampling.predictor), co.get_corrector(cfg.sampling.corrector), snr=cfg.sampling.snr,
                    p_steps=sc.P_STEPS, c_steps=1, probability_flow=False, continuous=True, denoise=True, use_path=use_path, eps=1e-5)
                with ref_import.TapeRandn(tp) as tr:
                    res, _ = fn(model, y)
                    assert tr.i == len(tp), (case, key, tr.i, len(tp))
                assert torch.isfinite(res).all() and tuple(res.shape) == xs
                out[case + key] = res.numpy()
                print('case %s%s: %d-step PC sample, max |x| %.3f' % (case, key, sc.P_STEPS, float(res.abs().max())))
        if case == sc.TRAIN_CASE:
            gcfg, x, gy, tvals, tape = sc.grad_inputs(case)
            gm, _ = mg.build_ref_model(ref, gcfg)
            gm.train()
            fn = L.get_general_sde_loss_fn(sdes_for(ref, gcfg), True, True, True, True, True)
            orig = torch.rand
            torch.rand = lambda *a, **k: tvals.clone()
            try:
                with ref_import.TapeRandn(tape) as tr:
                    loss = fn(gm, (gy, x))
                    assert tr.i == len(tape)
            finally:
                torch.rand = orig
            loss.backward()
            names, norms, samples = [], [], []
            for k, prm in gm.named_parameters():
                g = prm.grad.detach().reshape(-1).double().numpy()
                idx = cases.grad_sample_index(k, g.size)
                sm = np.zeros(48)
                sm[:idx.size] = g[idx]
                names.append(k); norms.append(np.sqrt((g * g).sum())); samples.append(sm)
            out[case + '_loss'] = np.float64(loss.item())
            out[case + '_names'], out[case + '_norms'], out[case + '_samples'] = np.array(names), np.array(norms), np.array(samples)
            print('case %s: loss %.6f, %d gradients' % (case, loss.item(), len(names)))
    np.savez_compressed(sc.GOLDEN, **out)
    print('sr2x.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(sc.GOLDEN)))


if __name__ == '__main__':
    main()
