"""Build-container tool: run the IMPORTED REFERENCE's 3-D DDPM networks (models/ddpm3D.py) on the seeded cases of
tests/ddpm3d_cases.py and write tests/golden/ddpm3d.npz.

    python tools/make_ddpm3d_goldens.py

Uses oracle/ref_import.py, oracle/cases.py and oracle/score_oracle.py by import, plus importlib.import_module('models.ddpm3D') (ref_import's
module list does not name it).  The fixture holds reference OUTPUTS only - out_<case> (the network's output on the case's inputs; the
paired network's two halves concatenated back), run_<S> (the sampler's result) - and shapes_<case>, the reference state_dict's
(name, shape) list as a JSON string.  Parameters (score_oracle.synth_params(shapes, 0)), inputs, labels and noise tapes are regenerated
from seeds on either side.

Sampler runs: the reference's get_pc_conditional_sampler (sampling/conditional.py:47-228), conditional reverse diffusion + conditional
Langevin, snr = 0.16, p_steps = 3, eps = 1e-5, continuous, denoise, under ref_import.TapeRandn with ddpm3d_cases.sampler_tape:
  S1  case B (ddpm3D_paired_SR3) with cVESDE(0.01, 30, N = 6)
  S2  case A (ddpm3D_paired) with the pair {'x': cVESDE(0.01, 30, N = 6), 'y': VESDE(0.01, 1, N = 6)}: two extra z_y draws per step
A run the reference raises on is left out and reported on stdout.

The tool also prints how far the reference's fp32 output lies from the float64 restatement ddpm3d_cases.forward64 (max-abs-diff /
max-abs-ref), which checks that restatement against the reference.
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]
import cases  # noqa: E402,F401
import ddpm3d_cases as dc  # noqa: E402
import ref_import  # noqa: E402
import score_oracle as so  # noqa: E402


def build(ref, case):
    cfg, B = dc.make_config(case)
    model = ref['models.utils'].create_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    p = so.synth_params(shapes, 0)
    model.load_state_dict(p)
    return cfg, model.eval(), shapes, p


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    importlib.import_module('models.ddpm3D')
    sl, pr, co = ref['sde_lib'], ref['sampling.predictors'], ref['sampling.correctors']
    out, models = {}, {}
    for case in dc.CASES:
        cfg, model, shapes, p = build(ref, case)
        models[case] = (cfg, model)
        x, y, labels = dc.case_inputs(case)
        with torch.no_grad():
            o = dc.call(model, case, x, y, labels)
            o64 = dc.forward64(p, case, x, y, labels)
        assert torch.isfinite(o).all(), case
        err = float((o.double() - o64).abs().max() / o64.abs().max())
        print('case %s: out %s max |out| %.3f, fp32 reference vs float64 restatement %.2e' % (case, tuple(o.shape), float(o.abs().max()), err))
        assert err < 1e-5, (case, err)
        out['out_' + case] = o.numpy()
        out['shapes_' + case] = np.array(json.dumps([[k, list(v)] for k, v in shapes.items()]))
    for run, case in dc.SAMPLER_RUNS.items():
        cfg, model = models[case]
        sx = sl.cVESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
        sde = {'x': sx, 'y': sl.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX_Y, dc.N_SCALES)} if cfg.model.name == 'ddpm3D_paired' else sx
        _, y, _ = dc.case_inputs(case)
        shape = (y.shape[0],) + tuple(cfg.data.shape_x)
        tp = dc.sampler_tape(run)
        try:
            fn = ref['sampling.conditional'].get_pc_conditional_sampler(
                sde, shape, pr.get_predictor('conditional_reverse_diffusion'), co.get_corrector('conditional_langevin'), snr=dc.SNR,
                p_steps=dc.P_STEPS, c_steps=1, probability_flow=False, continuous=True, denoise=True, eps=dc.EPS)
            with ref_import.TapeRandn(tp) as tr:
                res, _ = fn(model, y.clone())
                assert tr.i == len(tp), (run, tr.i, len(tp))
        except Exception as e:      # noqa: BLE001 - a run the reference cannot do is reported, not pinned
            print('run %s: the reference raised %s: %s - not pinned' % (run, type(e).__name__, e))
            continue
        assert torch.isfinite(res).all() and tuple(res.shape) == shape, run
        out['run_' + run] = res.numpy()
        print('run %s: %s max |x| %.3f' % (run, tuple(res.shape), float(res.abs().max())))
    np.savez_compressed(dc.GOLDEN, **out)
    print('ddpm3d.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(dc.GOLDEN)))


if __name__ == '__main__':
    main()
