"""-m gpu: the on-device noise of the fused PC loop is the tape of its schedule.  For the plain, std_y and use_path modes (inpainting:
test_gpu_inpaint_fused.py::test_seed_equals_the_tape_of_its_streams) a run with ``seed=`` returns the bits of a run on a tape filled,
row by row of csd_pc_noise_draws, with ``ops.randn(shape of the row, seed, the row's Philox stream)`` behind the stream-0 prior: the
loop's tape offsets and its stream ids come from one schedule (csrc/pc_loop.h), and this is the check that they agree on the device."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import kxsr_cases as kc  # noqa: E402
from test_gpu_network import build, dev, sdes_for  # noqa: E402

P_STEPS, B, SEED = 3, 2, 5
_MODELS = {}


def setting(name):
    """-> (model, sde, snr, shape of x, y or None, unconditional_label)"""
    if name not in _MODELS:
        if name == 'kxsr_K1':                              # y_scale: ny < nx
            from test_gpu_kxsr import model_for, sdes_for as kx_sdes
            cfg, model = model_for('K1')
            assert kc.B == B
            _MODELS[name] = (model, kx_sdes(cfg), cfg.sampling.snr, kc.shapes('K1')[0], kc.case_y('K1').to(dev()), None)
        else:
            cfg, _, _, model = build(name)
            assert cases.CASES[name][1] == B
            y = cases.case_y(name).to(dev()) if name != 'uncond_tiny' else None
            _MODELS[name] = (model, sdes_for(cfg), cfg.sampling.snr, (B,) + tuple(cfg.data.shape_x), y, 'sigma' if y is None else None)
    return _MODELS[name]


@pytest.mark.parametrize('name,use_path,pred,corr', [
    ('uncond_tiny', False, 'reverse_diffusion', 'langevin'),
    ('uncond_tiny', False, 'euler_maruyama', 'none'),
    ('cmde_tiny', False, 'conditional_reverse_diffusion', 'conditional_langevin'),
    ('cmde_tiny', False, 'conditional_none', 'conditional_ald'),
    ('cmde_tiny', True, 'conditional_reverse_diffusion', 'conditional_langevin'),
    ('cmde_tiny', True, 'conditional_euler_maruyama', 'conditional_none'),
    ('kxsr_K1', False, 'conditional_reverse_diffusion', 'conditional_langevin'),
    ('kxsr_K1', True, 'conditional_none', 'conditional_langevin'),
])
def test_seed_equals_the_tape_of_its_streams(name, use_path, pred, corr):
    from conditional_score_diffusion_amd import ops
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    model, sde, snr, xs, y, label = setting(name)
    P, C = get_predictor(pred), get_corrector(corr)
    assert fused.fusable(model, sde, P, C, 1, False, True, use_path=use_path)
    pid, cid = fused._rule_ids(P, C)
    std_y = isinstance(sde, dict) and not use_path
    rows = fused.noise_draws(model._h, B, pid, cid, std_y, use_path, False, P_STEPS)
    assert [r[5] for r in rows] == list(range(1, 1 + len(rows)))
    assert any(fused.DRAW_KINDS[r[1]] in ('z_y0', 'z_y', 'zy') for r in rows) == (y is not None)

    def run(**kw):
        return fused.run(model, sde, xs, y, P_STEPS, snr, 1e-5, True, unconditional_label=label, predictor=P, corrector=C,
                         use_path=use_path, **kw)[0]

    ys = tuple(y.shape) if y is not None else None
    tape = [ops.randn(tuple(xs), SEED, 0, dev())]
    for step, kind, phase, elems, offset, stream in rows:
        shape = tuple(xs) if fused.DRAW_KINDS[kind] in ('z', 'z_blend') else ys
        assert elems == int(torch.Size(shape).numel())
        tape.append(ops.randn(shape, SEED, stream, dev()))
    a, b, c = run(seed=SEED), run(seed=SEED), run(seed=SEED + 1)
    d = run(noise_tape=tape)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(a, d)
    assert (a - c).abs().max().item() > 1e-2               # another key: another prior and other noise
