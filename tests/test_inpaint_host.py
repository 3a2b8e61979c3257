"""PC inpainting on the fused device loop, host side: the ABI struct against the header, the per-step tables against
``sde.marginal_prob``, the draw count of the tape layout, and the dispatch of ``get_pc_inpainter(device_loop=...)``."""
import os
import re

import numpy as np
import pytest
import torch

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _struct_fields(name):
    hdr = open(os.path.join(ROOT, 'include', 'csd.h')).read()
    body = hdr[hdr.index('typedef struct %s {' % name):hdr.index('} %s;' % name)]
    return re.findall(r'^\s+(?:const )?[a-z0-9_]+\*? ([a-z0-9_A-Z]+);', body, flags=re.M)


def test_inpaint_params_mirror_the_header():
    from conditional_score_diffusion_amd import _lib
    names = [n for n, _ in _lib.PCInpaintParams._fields_]
    assert names == ['data', 'mask', 'mean_scale', 'std']
    assert _struct_fields('csd_pc_inpaint_params') == names
    import ctypes
    assert ctypes.sizeof(_lib.PCInpaintParams) == 4 * ctypes.sizeof(ctypes.c_void_p)      # four pointers, no padding
    ip = _lib.PCInpaintParams()
    assert not ip.data and not ip.mask and not ip.mean_scale and not ip.std


def test_pc_params_are_unchanged():
    """the inpainting fields live in their own struct: csd_pc_params ends where it ended, and a zero-initialised one is still the
    (reverse diffusion, Langevin) VE pair"""
    from conditional_score_diffusion_amd import _lib
    names = [n for n, _ in _lib.PCParams._fields_]
    assert names[-3:] == ['rd_drift', 'rd_sub_x', 'probability_flow'] and len(names) == 20
    assert _struct_fields('csd_pc_params') == names
    p = _lib.PCParams()
    assert p.predictor == 0 and p.corrector == 0 and not p.noise_tape and not p.record and not p.path_coef and not p.rd_drift
    for name in ('csd_pc_inpaint_scratch_bytes', 'csd_pc_inpaint_sample', 'csd_pc_inpaint_step_begin', 'csd_pc_inpaint_step_end',
                 'csd_inpaint_blend'):
        assert name in _lib.SIGNATURES
    # the counterparts' argument lists plus the inpainting struct
    for a, b in (('csd_pc_sample', 'csd_pc_inpaint_sample'), ('csd_pc_step_begin', 'csd_pc_inpaint_step_begin'),
                 ('csd_pc_step_end', 'csd_pc_inpaint_step_end')):
        assert len(_lib.SIGNATURES[b][1]) == len(_lib.SIGNATURES[a][1]) + 1
    assert _lib.SIGNATURES['csd_pc_inpaint_scratch_bytes'] == _lib.SIGNATURES['csd_pc_scratch_bytes']


def _sdes():
    from conditional_score_diffusion_amd import sde_lib
    return [('ve', sde_lib.VESDE(0.01, 50., 1000)), ('vp_c', sde_lib.VPSDE(0.1, 20., 1000)), ('vp_d', sde_lib.VPSDE(0.1, 20., 1000)),
            ('subvp', sde_lib.subVPSDE(0.1, 20., 1000))]


@pytest.mark.parametrize('key', ['ve', 'vp_c', 'vp_d', 'subvp'])
def test_inpaint_tables_are_the_marginal(key):
    from conditional_score_diffusion_amd.sampling import fused
    sde = dict(_sdes())[key]
    n = 7
    ts = torch.linspace(sde.T, 1e-3, n)
    mean_scale, std = fused.inpaint_tables(sde, ts)
    assert mean_scale.dtype == std.dtype == torch.float32 and tuple(mean_scale.shape) == tuple(std.shape) == (n,)
    for i in range(n):
        m, s = sde.marginal_prob(torch.ones(2, 1, 1, 1), torch.ones(2) * ts[i])       # what the inpainter evaluates on the data
        assert float(mean_scale[i]) == float(m.flatten()[0]) and float(std[i]) == float(s.flatten()[0]), (key, i)
    if key == 've':
        assert bool((mean_scale == 1.0).all())
    else:
        assert float(mean_scale[0]) < 0.1 and float(mean_scale[-1]) > 0.99
    if key == 'vp_d':       # the marginal std, not the score function's table at the truncated label
        _, _, std_x, _, _ = fused.step_scalars(sde, n, 1e-3, 'sigma', continuous=False)
        assert bool((std == fused.step_scalars(sde, n, 1e-3, 'sigma', continuous=True)[2]).all())
        assert not bool((std == std_x).all())


def test_tape_length_counts_every_present_draw():
    from conditional_score_diffusion_amd.sampling import fused
    for N in (1, 6, 12):
        for has_c in (False, True):
            for has_p in (False, True):
                assert fused.inpaint_tape_length(N, has_c, has_p) == 1 + (int(has_c) + int(has_p) + 2) * N
    assert len(cases.inpaint_case()[4]) == fused.inpaint_tape_length(12, True, True)      # the reference's own run (inpaint.npz)


def _inpainter(model_case, n_steps=1, device_loop=True):
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import unconditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    model = mutils.create_model(cases.case_config(model_case)[0])
    fn = unconditional.get_pc_inpainter(sde_lib.VESDE(0.01, 50., 4), get_predictor('reverse_diffusion'), get_corrector('langevin'),
                                        snr=0.15, n_steps=n_steps, continuous=True, device_loop=device_loop)
    data = torch.zeros(2, 3, 16, 16)
    return fn, model, data, torch.ones_like(data)


def test_device_loop_refuses_what_it_does_not_cover():
    fn, model, data, mask = _inpainter('uncond_tiny')
    with pytest.raises(NotImplementedError, match='device loop runs on the GPU'):      # a CPU model: no silent fall-back
        fn(model, data, mask)
    fn, model, data, mask = _inpainter('sr3_tiny')
    with pytest.raises(NotImplementedError, match='unconditional network'):
        fn(model, data, mask)
    fn, model, data, mask = _inpainter('uncond_tiny', n_steps=2)
    with pytest.raises(NotImplementedError, match='n_steps = 2'):
        fn(model, data, mask)


@pytest.mark.parametrize('kw', [dict(noise_tape=[torch.zeros(1)]), dict(seed=3), dict(global_norm=(lambda s: None, 2))])
def test_device_loop_keywords_need_the_device_loop(kw):
    fn, model, data, mask = _inpainter('uncond_tiny', device_loop=False)
    with pytest.raises(NotImplementedError, match='device_loop=True'):
        fn(model, data, mask, **kw)


def test_inpainting_fn_reads_the_config_switch():
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import unconditional
    cfg = cases.case_config('uncond_tiny')[0]
    sde = sde_lib.VESDE(0.01, 50., 4)
    model = mutils.create_model(cfg)
    data = torch.zeros(2, 3, 16, 16)
    assert not cfg.sampling.get('csd_device_loop', False)             # the default stays the step-by-step loop
    cfg.sampling.csd_device_loop = True
    with pytest.raises(NotImplementedError, match='device_loop=True'):
        unconditional.get_inpainting_fn(cfg, sde, 1e-5)(model, data, torch.ones_like(data))
