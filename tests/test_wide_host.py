"""No GPU: the DDPM family with 9 .. 32 input channels on the host side - what csd_unet_create accepts and refuses, that every such
network plans (inference and the training dry run) in the four precision modes, the sizing entries of the cases of
tests/wide_cases.py, the Python adapter's channel counts - and the sensitivity of the forward bound of tests/test_gpu_wide.py: the
reference's own fp32 output passes it against a float64 restatement, three deliberately wrong restatements miss it by more than 10x."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import wide_cases as wc

PRECISIONS = ('fp32', 'fp16x3', 'fp16', 'fp16f8')


def _create(cfg):
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ncsnpp      # noqa: F401  (registers the model names)
    with torch.device('meta'):                                 # (the handle only: no parameter values)
        return mutils.create_model(cfg)


def _digest(model, B, dropout=0.0):
    """csd_unet_debug_digest: hashes the parameter table, the packed layout, the inference plan and the training dry run - it fails
    where any of them cannot be built"""
    from conditional_score_diffusion_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).csd_unet_debug_digest
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_uint64)]
    d = (ctypes.c_uint64 * 4)()
    rc = fn(model._h, B, float(dropout), d)
    return rc, [int(v) for v in d], _lib.lib().csd_last_error().decode()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_nine_to_thirty_two_channels_create_and_plan(precision):
    """every channel count above the old limit, split x | y in two ways and unconditional, at a size the fused first layer covers (16,
    nf 64) and one it does not (20, nf 32)"""
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    seen = set()
    for c in range(9, 33):
        for name, xc, yc in (('ddpm', c, 0), ('ddpm_paired', c // 2, c - c // 2), ('ddpm_paired_SR3', c - 3, 3)):
            S, nf = (16, 64) if c % 2 else (20, 32)
            cfg = cases.make_config(name=name, nf=nf, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(S // 2,), image_size=S, x_ch=xc,
                                    y_ch=yc if yc else xc)
            cfg.model.csd_precision = precision
            model = _create(cfg)
            assert (model.x_channels, model.y_channels) == (xc, yc)
            assert model.out_channels == {'ddpm': c, 'ddpm_paired': c, 'ddpm_paired_SR3': xc}[name]
            rc, d, msg = _digest(model, 2, 0.1)
            assert rc == 0, (name, c, precision, msg)
            assert l.csd_unet_workspace_bytes(model._h, 3) > 0 and l.csd_unet_packed_bytes(model._h) > 0
            seen.add(tuple(d[1:]))
    assert len(seen) == 24 * 2                     # (layout, plan and training graph follow the channel counts; x | y split the same total alike)


def test_thirty_three_channels_are_refused_naming_the_limit():
    for name, xc, yc in (('ddpm', 33, 0), ('ddpm_paired', 17, 16), ('ddpm_paired_SR3', 30, 3)):
        cfg = cases.make_config(name=name, x_ch=xc, y_ch=yc if yc else xc)
        with pytest.raises(RuntimeError, match=r'x\+y channels must be <= 32'):
            _create(cfg)
    cfg = cases.make_config(name='ddpm_paired_SR3', x_ch=3, y_ch=3)
    cfg.model.output_channels = 33
    with pytest.raises(RuntimeError, match=r'out_channels must be in 1 \.\. 32'):
        _create(cfg)


def test_ncsnpp_keeps_its_limit_and_message():
    cfg = cases.make_ncsnpp_config(channels=9)
    with pytest.raises(RuntimeError, match=r'ncsnpp: x\+y channels must be <= 8'):
        _create(cfg)
    _create(cases.make_ncsnpp_config(channels=8))


@pytest.mark.parametrize('case', wc.ISSUE_CASES)
def test_sizing_entries_of_the_cases(case):
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    for precision in PRECISIONS:
        model = _create(wc.make_config(case, precision))
        assert l.csd_unet_workspace_bytes(model._h, wc.B) > 0
        assert l.csd_pc_scratch_bytes(model._h, wc.B) > 0
        assert l.csd_unet_train_workspace_bytes(model._h, wc.B, 0.0) > 0
        name, xc, yc, S = wc.CASES[case][:4]
        hw, oc = S * S, model.out_channels
        # net_out | x_mean | z | zy | labels | y_t, 64-float granules, + the norm partials (include/csd.h)
        floats = lambda n: (n + 63) // 64 * 64      # noqa: E731
        want = 4 * (floats(wc.B * oc * hw) + 2 * floats(wc.B * xc * hw) + 2 * floats(wc.B * max(yc, 1) * hw) + floats(wc.B))
        assert l.csd_pc_scratch_bytes(model._h, wc.B) == want + wc.B * 64 * 2 * 8 + 256


def test_unconditional_adapter_takes_its_channels_from_the_data():
    """configs/ve/haarflow/*.py name the 12 Haar bands in data.num_channels and set no model.input_channels / output_channels"""
    cfg = wc.make_config('W2')
    del cfg.model['input_channels'], cfg.model['output_channels']
    assert cfg.data.num_channels == 12
    model = _create(cfg)
    assert (model.x_channels, model.y_channels, model.out_channels) == (12, 0, 12)
    shapes = dict(model._param_table())
    assert shapes['all_modules.2.weight'] == (32, 12, 3, 3)
    last = max(int(k.split('.')[1]) for k in shapes)
    assert shapes['all_modules.%d.weight' % last] == (12, 32, 3, 3)


# ---- sensitivity of the forward bound (tests/test_gpu_wide.py: rel < 1e-4) ----------------------------------------------------------------
FORWARD_BOUND = 1e-4


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize('case', wc.ISSUE_CASES + ['W1c'])
def test_forward_bound_passes_the_reference_and_catches_wrong_channel_handling(case):
    """the fixture (the reference's fp32 forward) lies within the bound of the float64 restatement; the restatement with the x and y
    blocks swapped, with the channels from 8 on dropped, or with non-zero padding channels misses the bound by more than 10x"""
    g = wc.golden()
    cfg = wc.make_config(case)
    p = wc.params(cfg)
    y = wc.case_y(case)
    for j, (x, t) in enumerate(wc.forward_inputs(case)):
        if j and case in wc.ONE_TIME_CASES:
            break
        ref = torch.from_numpy(g['%s_net%d' % (case, j)])
        if cfg.model.name == 'ddpm':
            sig = cfg.model.sigma_min_x * (cfg.model.sigma_max_x / cfg.model.sigma_min_x) ** t      # VESDE.marginal_prob's std
            labels = sig.float()
        else:
            labels = t * (cfg.model.num_scales - 1)
        with torch.no_grad():
            assert _rel(ref, wc.forward64(p, cfg, x, y, labels)) < FORWARD_BOUND
            for mangle in ('swap', 'drop', 'pad'):
                e = _rel(wc.forward64(p, cfg, x, y, labels, mangle=mangle), ref)
                assert e > 10 * FORWARD_BOUND, (case, j, mangle, e)
