"""Build-container tool: run the IMPORTED REFERENCE's ddpm_KxSR / NCSNpp_KxSR (models/ddpm.py:316-331, models/ncsnpp.py:435-450), the
two-SDE score function, the conditional PC sampler and autograd on the seeded cases of tests/kxsr_cases.py and write
tests/golden/kxsr.npz.

    python tools/make_kxsr_goldens.py

The reference builds its two resizes from torchvision's ``Resize(size, interpolation=InterpolationMode.BILINEAR)``.  torchvision is not
installed; oracle/ref_import.install() leaves an existing ``torchvision`` entry of sys.modules alone, so this tool installs its own
stand-in FIRST, whose Resize is

    F.interpolate(img, size=(size, size), mode='bilinear', align_corners=False)

ASSUMPTION: that is torch's bilinear resize WITHOUT antialiasing - what Resize did on tensors in the torchvision releases of the
reference's time, whose ``antialias`` did not default to True.  It only matters for the downward resize (upwards antialiasing changes
nothing).  Every reference source file is imported unmodified.

Uses oracle/ref_import.py, oracle/cases.py, oracle/score_oracle.py and oracle/make_goldens.py (build_ref_model) by import.  The fixture
holds reference OUTPUTS only; parameters, inputs, labels and noise tapes are regenerated from seeds on either side:

  <case>_x<j>, <case>_y<j>   the network's two outputs ([B, cx, S, S] and [B, cy, S / K, S / K]) at t = kxsr_cases.FORWARD_TIMES[j]
  <case>_sx, <case>_sy       models.utils.get_score_fn on the pair {'x': cVESDE, 'y': VESDE} (continuous) at kxsr_cases.score_inputs
  <case>_pc                  get_pc_conditional_sampler on that pair: conditional reverse diffusion + conditional Langevin, P_STEPS
                             steps, continuous, denoise (SAMPLER_CASES)
  <case>_path                the same with use_path = True (PATH_CASE)
  <case>_loss / _names / _norms / _samples
                             the training loss (losses.get_general_sde_loss_fn, train = True, dropout 0) and per parameter the
                             gradient's L2 norm and its values at cases.grad_sample_index - the layout of tests/golden/grads.npz
  <case>_dx                  d/dx of (out_x * w_x).sum() + (out_y * w_y).sum() in eval mode at kxsr_cases.dx_inputs (TRAIN_CASE)

It also checks the float64 restatement kxsr_cases.forward64 against the reference's fp32 output and prints the distance.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]


def install_torchvision_stand_in():
    """see the module docstring: Resize(size, BILINEAR) = torch's bilinear resize to (size, size), align_corners=False, no antialias"""
    assert 'torchvision' not in sys.modules, 'a torchvision is already imported: this tool must install its stand-in first'
    tv = types.ModuleType('torchvision')
    tr = types.ModuleType('torchvision.transforms')
    fn = types.ModuleType('torchvision.transforms.functional')

    class InterpolationMode:
        NEAREST = 'nearest'
        BILINEAR = 'bilinear'
        BICUBIC = 'bicubic'

    class Resize(torch.nn.Module):
        def __init__(self, size, interpolation=InterpolationMode.BILINEAR):
            super().__init__()
            assert interpolation == InterpolationMode.BILINEAR and isinstance(size, int)
            self.size = size

        def forward(self, img):
            return F.interpolate(img, size=(self.size, self.size), mode='bilinear', align_corners=False)

    fn.InterpolationMode = InterpolationMode
    tr.Resize = Resize
    tr.functional = fn
    tr.InterpolationMode = InterpolationMode
    tv.transforms = tr
    sys.modules.update({'torchvision': tv, 'torchvision.transforms': tr, 'torchvision.transforms.functional': fn})


install_torchvision_stand_in()
import cases  # noqa: E402
import kxsr_cases as kc  # noqa: E402
import make_goldens as mg  # noqa: E402
import ref_import  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def sdes_for(ref, cfg):
    sl, m = ref['sde_lib'], cfg.model
    return {'x': sl.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sl.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}


def build(ref, cfg):
    """the reference model of a case with the seeded parameters of kxsr_cases.params"""
    if cfg.model.name == 'ddpm_KxSR':
        return mg.build_ref_model(ref, cfg)
    torch.manual_seed(0)
    model = ref['models.utils'].create_model(cfg)
    p = kc.params(cfg, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict(p)
    return model.eval(), p


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    L, pr, co = ref['losses'], ref['sampling.predictors'], ref['sampling.correctors']
    out = {}
    for case in kc.CASES:
        cfg = kc.make_config(case)
        model, p = build(ref, cfg)
        assert type(model).__name__ in ('ddpm_KxSR', 'NCSNpp_KxSR')
        assert not [k for k in model.state_dict() if 'resize' in k]
        sde = sdes_for(ref, cfg)
        y = kc.case_y(case)
        xs, ys = kc.shapes(case)
        with torch.no_grad():
            for j, (x, t) in enumerate(kc.forward_inputs(case)):
                labels = kc.labels_of(cfg, t)
                net = model({'x': x, 'y': y}, labels)
                assert tuple(net['x'].shape) == xs and tuple(net['y'].shape) == ys
                wx, wy = kc.forward64(p, case, x, y, labels)
                e = max(rel(net['x'], wx), rel(net['y'], wy))
                assert torch.isfinite(net['x']).all() and torch.isfinite(net['y']).all() and e < 1e-5, (case, j, e)
                out['%s_x%d' % (case, j)], out['%s_y%d' % (case, j)] = net['x'].numpy(), net['y'].numpy()
            print('case %s: out %s | %s, fp32 reference vs float64 restatement %.2e' % (case, tuple(net['x'].shape), tuple(net['y'].shape), e))
            sx, sy, st = kc.score_inputs(case)
            score = ref['models.utils'].get_score_fn(sde, model, conditional=True, train=False, continuous=True)({'x': sx, 'y': sy}, st)
            out[case + '_sx'], out[case + '_sy'] = score['x'].numpy(), score['y'].numpy()
            for key, use_path, tp in (('_pc', False, kc.pc_tape(case) if case in kc.SAMPLER_CASES else None),
                                      ('_path', True, kc.path_tape(case) if case == kc.PATH_CASE else None)):
                if tp is None:
                    continue
                fn = ref['sampling.conditional'].get_pc_conditional_sampler(
                    sde, xs, pr.get_predictor(cfg.sampling.predictor), co.get_corrector(cfg.sampling.corrector), snr=cfg.sampling.snr,
                    p_steps=kc.P_STEPS, c_steps=1, probability_flow=False, continuous=True, denoise=True, use_path=use_path, eps=1e-5)
                with ref_import.TapeRandn(tp) as tr:
                    res, _ = fn(model, y)
                    assert tr.i == len(tp), (case, key, tr.i, len(tp))
                assert torch.isfinite(res).all() and tuple(res.shape) == xs
                out[case + key] = res.numpy()
                print('case %s%s: %d-step PC sample, max |x| %.3f' % (case, key, kc.P_STEPS, float(res.abs().max())))
        if case == kc.TRAIN_CASE:
            gcfg, x, gy, tvals, tape = kc.grad_inputs(case)
            gm, _ = build(ref, gcfg)
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
            _, x, dy, labels, wx, wy = kc.dx_inputs(case)
            gm.eval()
            xg = x.clone().requires_grad_(True)
            net = gm({'x': xg, 'y': dy}, labels)
            dx, = torch.autograd.grad((net['x'] * wx).sum() + (net['y'] * wy).sum(), xg)
            out[case + '_dx'] = dx.numpy()
            print('case %s: d_x max %.3e' % (case, float(dx.abs().max())))
    np.savez_compressed(kc.GOLDEN, **out)
    print('kxsr.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(kc.GOLDEN)))


if __name__ == '__main__':
    main()
