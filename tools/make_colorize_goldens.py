"""Build-container tool: run the IMPORTED REFERENCE's colorizer on the tiny unconditional network and write tests/golden/colorize.npz.

    python tools/make_colorize_goldens.py

Uses oracle/ref_import.py, oracle/cases.py, the helpers of oracle/make_goldens.py and tests/colorize_cases.py by import.  The fixture
holds reference OUTPUTS only: the network's parameters, the gray image and the noise tapes are regenerated from seeds on either side.

The reference's controllable_generation.py does ``from sampling import NoneCorrector, NonePredictor, shared_*_update_fn``; its `sampling`
package exports none of them.  For the length of that one import the reference's own module `sampling.unconditional` - which defines
the two update functions and imports the two classes - stands under the name `sampling` in sys.modules.  The file itself is imported
unmodified from where it lies.

run_<name>: the reference's get_pc_colorizer (controllable_generation.py:95-191, identity inverse_scaler) on `uncond_tiny` for every row
of colorize_cases.RUNS - N = 4 steps, eps = 1e-3, snr = 0.075, continuous time, the gray image of colorize_cases.gray() and the tape
colorize_cases.run_tape(pred, corr): the prior, then per step [z_corrector] z_colorize [z_predictor] z_colorize.

op_x, op_x_mean, op_scalars: the reference's own re-imposition alone - its colorization update function around the `none` predictor,
taken from the closure of the colorizer - on the seeded [3, 3, 5, 7] state of colorize_cases.op_inputs() under VPSDE at t = 0.4;
op_scalars = (mean scale, std) of that time.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]
import colorize_cases as cc  # noqa: E402
import make_goldens as mg  # noqa: E402
import ref_import  # noqa: E402


def import_controllable_generation(ref):
    import importlib
    pkg = sys.modules['sampling']
    sys.modules['sampling'] = ref['sampling.unconditional']
    try:
        return importlib.import_module('controllable_generation')
    finally:
        sys.modules['sampling'] = pkg


def closure_of(fn):
    return dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))


def main():
    torch.set_num_threads(8)
    ref = ref_import.modules()
    cg = import_controllable_generation(ref)
    sl, pr, co = ref['sde_lib'], ref['sampling.predictors'], ref['sampling.correctors']
    cfg = cc.config()
    model, _ = mg.build_ref_model(ref, cfg)
    model.embedding_type = 'positional'
    gray = cc.gray()
    out = {}
    for name, scls, pred, corr, pf, denoise in cc.RUNS:
        sde = cc.make_sde(sl, scls)
        tp = cc.run_tape(pred, corr)
        fn = cg.get_pc_colorizer(sde, pr.get_predictor(pred), co.get_corrector(corr), lambda v: v, snr=cc.SNR, n_steps=1,
                                 probability_flow=pf, continuous=True, denoise=denoise, eps=cc.EPS)
        with ref_import.TapeRandn(tp) as tr:
            res = fn(model, gray.clone())
            assert tr.i == len(tp) == 1 + cc.n_draws(pred, corr), (name, tr.i, len(tp))
        assert torch.isfinite(res).all(), name
        out['run_' + name] = res.numpy()
        print(name, 'max |x|', float(res.abs().max()))
    # the operator: the reference's update function around the 'none' predictor is the re-imposition alone
    sde = cc.make_sde(sl, 'VPSDE')
    fn = cg.get_pc_colorizer(sde, pr.get_predictor('none'), co.get_corrector('none'), lambda v: v, snr=cc.SNR, continuous=True, eps=cc.EPS)
    update = closure_of(fn)['predictor_colorize_update_fn']
    x, g, z = cc.op_inputs()
    with torch.no_grad(), ref_import.TapeRandn([z]) as tr:
        xn, xm = update(model, g.clone(), x.clone(), torch.tensor(cc.OP_T))
        assert tr.i == 1
    ms, sd = sde.marginal_prob(torch.ones(1, 1, 1, 1), torch.tensor([cc.OP_T]))
    out['op_x'], out['op_x_mean'] = xn.numpy(), xm.numpy()
    out['op_scalars'] = np.array([float(ms.flatten()[0]), float(sd.flatten()[0])], np.float64)
    np.savez_compressed(cc.GOLDEN, **out)
    print('colorize.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(cc.GOLDEN)))


if __name__ == '__main__':
    main()
