"""Build-container tool: run the IMPORTED REFERENCE's NCSN++ family (models/ncsnpp.py: NCSNpp, NCSNpp_paired, NCSNpp_2xSR), its
samplers and autograd on the seeded more-than-8-channel cases of tests/ncsnpp_wide_cases.py and write
tests/golden/ncsnpp_wide.npz.

    python tools/make_ncsnpp_wide_goldens.py

Uses oracle/ref_import.py, oracle/cases.py, oracle/score_oracle.py and oracle/make_goldens.py by import.  The fixture holds reference
OUTPUTS only; parameters (cases.ncsnpp_params(shapes, 5)), inputs, labels and noise tapes are regenerated from seeds on either side:

  <case>_net<j>                    network output (the paired halves concatenated back; N5: the x block in the squeezed layout) at
                                   t = FORWARD_TIMES[j] (ONE_TIME_CASES: j = 0 only).  The reference's SCORE of the x domain is not
                                   stored (the file has to stay below 1 MiB): it is net_x / sigma_x(t) (models/utils.py
                                   divide_by_sigmas), which this tool asserts against the reference's score function to 1e-6 and
                                   ncsnpp_wide_cases.score_of restates for the tests
  N5_keys                          the state_dict of NCSNpp_2xSR, 'name|shape' in order
  <case>_pc                        get_pc_conditional_sampler on the pair {'x': cVESDE, 'y': VESDE}, conditional reverse diffusion +
                                   conditional Langevin, P_STEPS steps, continuous, denoise (SAMPLER_CASES)
  <case>_loss / _names / _norms / _samples
                                   the training loss (losses.get_general_sde_loss_fn, train = True, dropout 0) and per trained
                                   parameter the gradient's L2 norm and its values at cases.grad_sample_index, rounded to float32 (TRAIN_CASES)
  N2_dx                            d (out * w).sum() / d x of the eval-mode network (ncsnpp_wide_cases.dx_inputs)
  bicubic_s<k>                     the two ncsnpp_2xSR stages of the 'bicubic' cascade, the reference's sampler chained on the stage tapes

It also checks oracle/score_oracle.py's ncsnpp_forward against the reference's output on every case and prints the distance.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]
import cases  # noqa: E402
import make_goldens as mg  # noqa: E402,F401  (the fixture tools' shared helpers; imported for its path set-up as well)
import ncsnpp_wide_cases as nw  # noqa: E402
import ref_import  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def build(ref, cfg):
    """the reference's model on the seeded parameters; its state_dict must be the library's parameter table"""
    torch.manual_seed(0)
    model = ref['models.utils'].create_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert shapes == nw.param_shapes(cfg), cfg.model.name
    p = nw.params(cfg, shapes)
    model.load_state_dict(p)
    return model.eval(), p, shapes


def sdes_for(ref, cfg, paired):
    sl, m = ref['sde_lib'], cfg.model
    if paired:
        return {'x': sl.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sl.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
    return sl.VESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales)


def pc_sampler(ref, cfg, sde, xs):
    pr, co = ref['sampling.predictors'], ref['sampling.correctors']
    return ref['sampling.conditional'].get_pc_conditional_sampler(
        sde, xs, pr.get_predictor(cfg.sampling.predictor), co.get_corrector(cfg.sampling.corrector), snr=cfg.sampling.snr,
        p_steps=nw.P_STEPS, c_steps=1, probability_flow=False, continuous=True, denoise=True, use_path=False, eps=1e-5)


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    mu, L = ref['models.utils'], ref['losses']
    pr, co = ref['sampling.predictors'], ref['sampling.correctors']
    out = {}
    for case in nw.CASES:
        cfg = nw.make_config(case)
        paired = nw.is_paired(case)
        model, p, shapes = build(ref, cfg)
        assert type(model).__name__ == {'ncsnpp': 'NCSNpp', 'ncsnpp_paired': 'NCSNpp_paired', 'ncsnpp_2xSR': 'NCSNpp_2xSR'}[cfg.model.name]
        if case == 'N5':
            out['N5_keys'] = np.array(['%s|%s' % (k, ','.join(map(str, shapes[k]))) for k in model.state_dict()])
        sde = sdes_for(ref, cfg, paired)
        y = nw.case_y(case)
        with torch.no_grad():
            for j, (x, t) in enumerate(nw.forward_inputs(case)):
                if j and case in nw.ONE_TIME_CASES:
                    break
                labels = nw.labels_of(case, cfg, t)
                if paired:
                    sfn = mu.get_score_fn(sde, model, conditional=True, train=False, continuous=True)
                    score = mu.get_conditional_score_fn(sfn, target_domain='x')(x, y, t)
                else:
                    score = mu.get_score_fn(sde, model, conditional=False, train=False, continuous=True)(x, t)
                net = nw.call(model, case, x, y, labels)
                e = rel(net, nw.oracle_forward(p, case, x, y, labels))
                assert torch.isfinite(net).all() and e < 2e-5, (case, j, e)
                out['%s_net%d' % (case, j)] = net.numpy()
                e_sc = rel(nw.score_of(case, cfg, net, t), score)
                assert e_sc < 1e-6, (case, j, e_sc)
            print('case %s: out %s, reference vs the oracle restatement %.2e' % (case, tuple(net.shape), e))
            if case in nw.SAMPLER_CASES:
                xs = nw.shapes(case)[0]
                tp = nw.pc_tape(case)
                with ref_import.TapeRandn(tp) as tr:
                    res, _ = pc_sampler(ref, cfg, sde, xs)(model, y)
                    assert tr.i == len(tp), (case, tr.i, len(tp))
                assert torch.isfinite(res).all() and tuple(res.shape) == xs
                out[case + '_pc'] = res.numpy()
                print('case %s: %d-step PC sample, max |x| %.3f' % (case, nw.P_STEPS, float(res.abs().max())))
        if case in nw.TRAIN_CASES:
            gcfg, x, gy, tvals, tape = nw.grad_inputs(case)
            gm, _, _ = build(ref, gcfg)
            gm.train()
            fn = L.get_general_sde_loss_fn(sdes_for(ref, gcfg, True), True, True, True, True, True)
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
                if prm.grad is None:                 # (the Gaussian Fourier W is a fixed buffer: layerspp.py:37)
                    assert not prm.requires_grad
                    continue
                g = prm.grad.detach().reshape(-1).double().numpy()
                idx = cases.grad_sample_index(k, g.size)
                sm = np.zeros(48)
                sm[:idx.size] = g[idx]
                names.append(k); norms.append(np.sqrt((g * g).sum())); samples.append(sm)
            out[case + '_loss'] = np.float64(loss.item())
            out[case + '_names'], out[case + '_norms'], out[case + '_samples'] = np.array(names), np.array(norms), np.array(samples, np.float32)
            print('case %s: loss %.6f, %d gradients' % (case, loss.item(), len(names)))
        if case == 'N2':
            _, x, dy, labels, w = nw.dx_inputs(case)
            xg = x.clone().requires_grad_(True)
            gx, = torch.autograd.grad((nw.call(model, case, xg, dy, labels) * w).sum(), xg)
            out['N2_dx'] = gx.numpy()
            print('case N2: |d_x| max %.3e' % float(gx.abs().max()))
    cur = nw.lr_input()
    for k in range(2):
        cfg = nw.stage_config('bicubic', k)
        model, _, _ = build(ref, cfg)
        tp = nw.stage_tape('bicubic', k)
        xs = (nw.B,) + tuple(cfg.data.shape_x)
        with ref_import.TapeRandn(tp) as tr, torch.no_grad():
            cur, _ = pc_sampler(ref, cfg, sdes_for(ref, cfg, True), xs)(model, cur)
            assert tr.i == len(tp) and tuple(cur.shape) == xs and torch.isfinite(cur).all()
        out['bicubic_s%d' % k] = cur.numpy()
        print('bicubic cascade stage %d: %s, max |x| %.3f' % (k, tuple(cur.shape), float(cur.abs().max())))
    np.savez_compressed(nw.GOLDEN, **out)
    print('ncsnpp_wide.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(nw.GOLDEN)))


if __name__ == '__main__':
    main()
