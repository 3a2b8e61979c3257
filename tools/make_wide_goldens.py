"""Build-container tool: run the IMPORTED REFERENCE's DDPM family (models/ddpm.py), its samplers, get_pc_inpainter and autograd on the
seeded more-than-8-channel cases of tests/wide_cases.py and write tests/golden/wide_channels.npz.

    python tools/make_wide_goldens.py

Uses oracle/ref_import.py, oracle/cases.py, oracle/score_oracle.py and oracle/make_goldens.py (build_ref_model, sdes_for) by import.  The
fixture holds reference OUTPUTS only; parameters (score_oracle.synth_params(shapes, 0)), inputs, labels and noise tapes are regenerated
from seeds on either side:

  <case>_net<j>, <case>_score<j>   network output (the paired network's halves concatenated back) and score of the x domain at
                                   t = wide_cases.FORWARD_TIMES[j] (ONE_TIME_CASES: the output at j = 0 only)
  <case>_pc                        get_pc_conditional_sampler, conditional reverse diffusion + conditional Langevin, P_STEPS steps,
                                   continuous, denoise (W1: the pair {'x': cVESDE, 'y': VESDE}, two extra z_y draws per step; W3: cVESDE)
  W2_inpaint                       get_pc_inpainter on W2, VESDE with INPAINT_N steps, the Haar channel mask [1, 12, 1, 1]
  <case>_loss / _names / _norms / _samples
                                   the training loss (losses.get_general_sde_loss_fn, train = True, dropout 0) and per parameter the
                                   gradient's L2 norm and its values at cases.grad_sample_index - the layout of tests/golden/grads.npz
  <case>_dx                        d (out * w).sum() / d x of the eval-mode network (wide_cases.dx_inputs)

It also checks the float64 restatement wide_cases.forward64 against the reference's fp32 output and prints the distance.
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
import wide_cases as wc  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    mu, L = ref['models.utils'], ref['losses']
    pr, co = ref['sampling.predictors'], ref['sampling.correctors']
    out = {}
    for case in wc.CASES:
        cfg = wc.make_config(case)
        model, p = mg.build_ref_model(ref, cfg)
        model.embedding_type = 'positional'          # (DDPM has no such attribute; the unconditional VESDE score_fn reads it)
        sde = mg.sdes_for(ref, cfg)
        y = wc.case_y(case)
        name = cfg.model.name
        with torch.no_grad():
            for j, (x, t) in enumerate(wc.forward_inputs(case)):
                if j and case in wc.ONE_TIME_CASES:
                    break
                if name == 'ddpm':
                    labels = sde.marginal_prob(x, t)[1]
                    score = mu.get_score_fn(sde, model, conditional=False, train=False, continuous=True)(x, t)
                else:
                    labels = t * (cfg.model.num_scales - 1)
                    sfn = mu.get_score_fn(sde, model, conditional=True, train=False, continuous=True)
                    score = mu.get_conditional_score_fn(sfn, target_domain='x')(x, y, t)
                net = wc.call(model, cfg, x, y, labels)
                e = rel(net, wc.forward64(p, cfg, x, y, labels))
                assert torch.isfinite(net).all() and e < 1e-5, (case, j, e)
                out['%s_net%d' % (case, j)] = net.numpy()
                if case not in wc.ONE_TIME_CASES:
                    out['%s_score%d' % (case, j)] = score.numpy()
            print('case %s: out %s, fp32 reference vs float64 restatement %.2e' % (case, tuple(net.shape), e))
            if case in wc.SAMPLER_CASES:
                xs = (wc.B,) + tuple(cfg.data.shape_x)
                tp = wc.pc_tape(case)
                fn = ref['sampling.conditional'].get_pc_conditional_sampler(
                    sde, xs, pr.get_predictor(cfg.sampling.predictor), co.get_corrector(cfg.sampling.corrector), snr=cfg.sampling.snr,
                    p_steps=wc.P_STEPS, c_steps=1, probability_flow=False, continuous=True, denoise=True, use_path=False, eps=1e-5)
                with ref_import.TapeRandn(tp) as tr:
                    res, _ = fn(model, y)
                    assert tr.i == len(tp), (case, tr.i, len(tp))
                assert torch.isfinite(res).all()
                out[case + '_pc'] = res.numpy()
                print('case %s: %d-step PC sample, max |x| %.3f' % (case, wc.P_STEPS, float(res.abs().max())))
        if case in wc.TRAIN_CASES:
            gcfg, x, gy, tvals, tape = wc.grad_inputs(case)
            gm, _ = mg.build_ref_model(ref, gcfg)
            gm.train()
            fn = L.get_general_sde_loss_fn(mg.sdes_for(ref, gcfg), True, True, True, True, True)
            orig = torch.rand
            torch.rand = lambda *a, **k: tvals.clone()
            try:
                with ref_import.TapeRandn(tape):
                    loss = fn(gm, (gy, x))
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
            dcfg, x, dy, labels, w = wc.dx_inputs(case)
            xg = x.clone().requires_grad_(True)
            gx, = torch.autograd.grad((wc.call(model, dcfg, xg, dy, labels) * w).sum(), xg)
            out[case + '_dx'] = gx.numpy()
            print('case %s: loss %.6f, %d gradients, |d_x| max %.3e' % (case, float(loss), len(names), float(gx.abs().max())))
    cfg, data, mask, tape = wc.inpaint_inputs()
    model, _ = mg.build_ref_model(ref, cfg)
    model.embedding_type = 'positional'
    sde = ref['sde_lib'].VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, wc.INPAINT_N)
    fn = ref['sampling.unconditional'].get_pc_inpainter(sde, pr.get_predictor('reverse_diffusion'), co.get_corrector('langevin'), snr=0.15,
                                                      n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-5)
    with ref_import.TapeRandn(tape) as tr, torch.no_grad():
        xi, _ = fn(model, data, mask)
        assert tr.i == len(tape), (tr.i, len(tape))
    out['W2_inpaint'] = xi.numpy()
    print('inpaint W2: max |x| %.3f, known channels err %.2e' % (float(xi.abs().max()), float(((xi - data) * mask).abs().max())))
    np.savez_compressed(wc.GOLDEN, **out)
    print('wide_channels.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(wc.GOLDEN)))


if __name__ == '__main__':
    main()
