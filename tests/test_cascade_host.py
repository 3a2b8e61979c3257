"""CPU-only checks of the sequential cascades (sampling/cascade.py, csd_band_split / csd_band_merge / csd_pc_cascade_sample): the surface
exists and the ABI triple agrees, the reference's fp32 chain of tests/golden/cascade.npz lies within the GPU tests' bound of a float64
restatement of the whole cascade while two wrong restatements miss it by far, and the argument errors of get_autoregressive_sampler.

Measured on the fixture (tools/make_cascade_goldens.py prints them), distance of the reference's images to the restatement in units of
the stage's sigma_max_x: bicubic 8.7e-7 / 7.6e-7, haar 3.8e-7 / 6.4e-7, haar_inpaint 2.2e-6 / 2.4e-6; with dy / dx of the second
bicubic squeeze exchanged 4.2e-1 at stage 2, with bands 1 and 2 exchanged 5.1 / 6.2 (haar) and 7.8 / 9.9 (haar_inpaint)."""
import ctypes
import os
import re

import pytest
import torch

import cascade_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_IMAGES = {}


def images64(flow, mangle=None):
    if (flow, mangle) not in _IMAGES:
        with torch.no_grad():
            _IMAGES[(flow, mangle)] = cc.cascade64(flow, mangle)
    return _IMAGES[(flow, mangle)]


def distance(flow, k, image):
    """max |reference - image| in units of the stage's sigma_max_x: the measure of the GPU tests"""
    ref = torch.from_numpy(cc.golden()['%s_s%d' % (flow, k)]).double()
    return float((ref - image.double()).abs().max()) / cc.sigma_max(flow, k)


def test_module_helpers_and_abi_triple():
    from conditional_score_diffusion_amd import _lib, ops
    from conditional_score_diffusion_amd.sampling import cascade
    for name in ('get_autoregressive_sampler', 'haar_forward', 'haar_backward', 'get_dc_coefficients', 'get_hf_coefficients', 'stage_seed'):
        assert callable(getattr(cascade, name)), name
    assert callable(ops.band_split) and callable(ops.band_merge)
    hdr = open(os.path.join(ROOT, 'include', 'csd.h')).read()
    l = _lib.lib()
    for name in ('csd_band_split', 'csd_band_merge', 'csd_pc_cascade_sample'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert hasattr(l, name) and name in _lib.SIGNATURES, name
    assert 'typedef struct csd_cascade_stage' in hdr
    # the binding's struct has the header's fields in the header's order
    body = hdr[hdr.index('typedef struct csd_cascade_stage'):hdr.index('} csd_cascade_stage;')]
    fields = re.findall(r'\b(\w+);', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert fields == [f[0] for f in _lib.CascadeStage._fields_], fields
    # no new sizing entry: the cascade's buffers are expressions of the existing ones
    assert not any('cascade' in n or 'band' in n for n in _lib.SIGNATURES if n.endswith('_bytes'))
    seeds = {cascade.stage_seed(5, k) for k in range(4)} | {cascade.stage_seed(6, 0)}
    assert len(seeds) == 5 and all(0 <= s < 2 ** 63 for s in seeds)


def test_library_refuses_bad_band_and_cascade_arguments_without_a_gpu():
    """argument checks run before any launch: a non-orthogonal matrix names its figure, null / malformed cascades are CSD_ERR_INVALID"""
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    one = ctypes.c_void_p(256)
    bad = (ctypes.c_float * 16)(*([1.0] + [0.0] * 4 + [1.0] + [0.0] * 4 + [1.0] + [0.0] * 4 + [1.001]))
    assert l.csd_band_merge(one, 4, one, 12, one, 16, 1, 1, 2, bad, None) == -1
    msg = l.csd_last_error().decode()
    assert 'not orthogonal' in msg and re.search(r'2\.0\d*e-03', msg), msg
    assert l.csd_band_split(one, 16, one, 16, 1, 1, 2, bad, None) == -1
    assert l.csd_band_split(None, 16, one, 16, 1, 1, 2, None, None) == -1
    assert l.csd_band_merge(one, 1, one, 12, one, 16, 1, 1, 2, None, None) == -1 and 'stride' in l.csd_last_error().decode()
    assert l.csd_pc_cascade_sample(None, 1, 0, None, 1, one, 1, one, 1, one, None, None) == -1
    stage = (_lib.CascadeStage * 1)()
    assert l.csd_pc_cascade_sample(stage, 1, 0, None, 1, one, 1, one, 1, one, None, None) == -1
    assert 'stages[0]' in l.csd_last_error().decode()
    assert l.csd_pc_cascade_sample(stage, 1, 3, None, 1, one, 1, one, 1, one, None, None) == -1
    assert l.csd_pc_cascade_sample(stage, 1, 0, None, 1, one, 1, one, 1, None, None, None) == -1


@pytest.mark.parametrize('flow', cc.FLOWS)
def test_reference_chain_is_within_the_gpu_bound_of_the_float64_restatement(flow):
    for k in range(cc.N_STAGES):
        d = distance(flow, k, images64(flow)[k])
        print('%s stage %d: reference vs float64 restatement %.3e of sigma_max_x' % (flow, k, d))
        assert tuple(images64(flow)[k].shape) == cc.image_shape(flow, k)
        assert d < cc.TRAJECTORY, (flow, k, d)


@pytest.mark.parametrize('flow', cc.FLOWS)
def test_wrong_restatements_miss_the_bound_by_more_than_ten_times(flow):
    """bands 1 and 2 exchanged in the merges (both Haar forms), dy / dx of the squeeze exchanged at the second stage (bicubic): the last
    stage's image misses the bound by more than 10x, so the GPU tests' bound tells these apart"""
    mangle = 'squeeze' if flow == 'bicubic' else 'bands'
    k = cc.N_STAGES - 1
    d = distance(flow, k, images64(flow, mangle)[k])
    print('%s with %s exchanged: last stage %.3e of sigma_max_x' % (flow, mangle, d))
    assert d > 10 * cc.TRAJECTORY, (flow, mangle, d)
    if mangle == 'bands':                      # (the merge of stage 1 is wrong already)
        assert distance(flow, 0, images64(flow, mangle)[0]) > 10 * cc.TRAJECTORY


def test_merge64_is_the_inverse_of_split64_and_band_major():
    x = torch.from_numpy(__import__('numpy').random.RandomState(3).standard_normal((2, 3, 8, 8)))
    bands = cc.split64(x)
    assert tuple(bands.shape) == (2, 12, 4, 4)
    assert torch.allclose(bands[:, 0:3], (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]) / 2)
    assert torch.allclose(bands[:, 3:6], (x[:, :, 0::2, 0::2] - x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] - x[:, :, 1::2, 1::2]) / 2)
    assert torch.allclose(bands[:, 6:9], (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] - x[:, :, 1::2, 0::2] - x[:, :, 1::2, 1::2]) / 2)
    assert torch.allclose(cc.merge64(bands[:, :3], bands[:, 3:]), x, atol=1e-14)


def _stages(flow, order=(0, 1)):
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    out = []
    for k in order:
        cfg = cc.stage_config(flow, k)
        m = cfg.model
        sde = (sde_lib.VESDE(m.sigma_min_x, m.sigma_max_x, cc.P_STEPS) if flow == 'haar_inpaint' else
               {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)})
        out.append((mutils.create_model(cfg), sde, cfg))
    return out


def test_get_autoregressive_sampler_argument_errors():
    from conditional_score_diffusion_amd.sampling import cascade
    with pytest.raises(NotImplementedError, match='wavelet space is not supported'):
        cascade.get_autoregressive_sampler(_stages('bicubic'), 'wavelet')
    for flow in cc.FLOWS:
        with pytest.raises(ValueError, match='low-to-high order.*stage 0 runs at 32, stage 1 at 16'):
            cascade.get_autoregressive_sampler(_stages(flow, (1, 0)), flow)
    with pytest.raises(ValueError, match='stage 0: a Haar stage'):
        cascade.get_autoregressive_sampler(_stages('bicubic'), 'haar')
    with pytest.raises(ValueError, match='stage 0: .*sde.N = 3'):
        cascade.get_autoregressive_sampler(_stages('haar_inpaint'), 'haar_inpaint', p_steps=7)
    with pytest.raises(ValueError, match='no stages'):
        cascade.get_autoregressive_sampler([], 'haar')
    # one_call=True with a stage the device loop does not run: two corrector steps per update at stage 1 (fused.fusable needs c_steps == 1)
    stages = _stages('bicubic')
    stages[1][2].sampling.n_steps_each = 2
    with pytest.raises(NotImplementedError, match=r'one_call=True\): stage 1: c_steps = 2'):
        cascade.get_autoregressive_sampler(stages, 'bicubic', p_steps=cc.P_STEPS, one_call=True)
    sampler = cascade.get_autoregressive_sampler(stages, 'bicubic', p_steps=cc.P_STEPS)
    lr = cc.lr_input('bicubic')
    with pytest.raises(RuntimeError, match='MI355X'):          # (a CPU tensor is refused: there is no CPU route)
        sampler(lr)
    with pytest.raises(NotImplementedError, match='show_evolution'):
        sampler(lr, show_evolution=True)
    why = cascade._why_not_one_call(stages[1][0], stages[1][1], cascade._settings(1, stages[1][1], stages[1][2], 'bicubic', 'default', 'default',
                                                                                 cc.P_STEPS, 'default'), False)
    assert why is not None and 'c_steps = 2' in why


def test_cascade_entry_validation_runs_before_any_device_work():
    """what a stage is and the extents at every link are checked on the host, in front of the buffers: handles made on the CPU and dummy
    addresses are enough to reach each refusal, and each names its stage"""
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    one = ctypes.c_void_p(256)
    pc, ip = _lib.PCParams(), _lib.PCInpaintParams()
    ip.data = ip.mask = 256

    def call(models, links, inpaint, final_link=0, y0=one, outs=None):
        arr = (_lib.CascadeStage * len(models))()
        for k, model in enumerate(models):
            arr[k].net, arr[k].packed, arr[k].pc, arr[k].x, arr[k].link = model._h, 256, ctypes.pointer(pc), 256, links[k]
            arr[k].inpaint = ctypes.pointer(ip) if inpaint[k] else None
            arr[k].out = (outs or [None] * len(models))[k]
        rc = l.csd_pc_cascade_sample(arr, len(models), final_link, y0, cc.B, one, 1, one, 1, one, None, None)
        return rc, l.csd_last_error().decode()

    bic = [s[0] for s in _stages('bicubic')]
    haar = [s[0] for s in _stages('haar')]
    inp = [s[0] for s in _stages('haar_inpaint')]
    # a well-formed cascade gets as far as the buffers: CSD_ERR_WORKSPACE naming the first stage that needs more than one byte
    for models, link, flag, final, outs in ((bic, 0, False, 0, None), (haar, 1, False, 1, [None, 256]), (inp, 2, True, 2, [None, 256])):
        rc, msg = call(models, [0, link], [flag, flag], final, None if flag else one, outs)
        assert rc == -5 and 'stages[0]' in msg and 'workspace too small' in msg, msg
    rc, msg = call(bic, [0, 0], [False, True])
    assert rc == -1 and 'stages[1]' in msg and 'conditional stage' in msg and 'inpaint' in msg, msg
    rc, msg = call(inp, [0, 2], [True, False], y0=None)
    assert rc == -1 and 'stages[1]' in msg and 'unconditional stage needs inpaint' in msg, msg
    rc, msg = call(bic[::-1], [0, 0], [False, False])
    assert rc == -1 and 'stages[1]' in msg and 'link 0' in msg and '64^2' in msg, msg
    rc, msg = call(haar[::-1], [0, 1], [False, False], 1, one, [None, 256])
    assert rc == -1 and 'stages[1]' in msg and 'link 1' in msg, msg
    rc, msg = call(inp[::-1], [0, 2], [True, True], 2, None, [None, 256])
    assert rc == -1 and 'stages[1]' in msg and 'link 2' in msg, msg
    rc, msg = call(inp, [0, 2], [True, True], 2, None, [256, 256])
    assert rc == -1 and 'stages[1]' in msg and 'out must be NULL' in msg, msg
    rc, msg = call(haar, [0, 1], [False, False], 1, one, None)
    assert rc == -1 and 'stages[1]' in msg and 'out is required' in msg, msg
    rc, msg = call(bic, [1, 0], [False, False])
    assert rc == -1 and 'stages[0]' in msg and 'link' in msg, msg
    rc, msg = call(bic, [0, 0], [False, False], y0=None)
    assert rc == -1 and 'stages[0]' in msg and 'y0' in msg, msg
    # a handle with y_scale (the Kx networks) and a 3-D handle
    import ddpm3d_cases as d3
    import kxsr_cases as kc
    from conditional_score_diffusion_amd.models import utils as mutils
    km = mutils.create_model(kc.make_config('K1'))
    rc, msg = call([bic[0], km], [0, 0], [False, False])
    assert rc == -1 and 'stages[1]' in msg and 'y_scale' in msg, msg
    cfg3, _ = d3.make_config('A')
    cfg3.model.csd_planned = True
    m3 = mutils.create_model(cfg3)
    assert m3.planned and m3._h
    rc, msg = call([bic[0], m3], [0, 0], [False, False])
    assert rc == -1 and 'stages[1]' in msg and '3-D' in msg, msg
