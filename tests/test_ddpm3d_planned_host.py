"""Host-side checks of the planned 3-D DDPM networks (models/ddpm3d.py with ``csd_planned``; csd_unet_config.arch = 2): the parameter
table of the handle against the reference's recorded state_dict, ``fused.fusable``, and the refusals.  No GPU."""
import ctypes
import itertools

import pytest
import torch

import ddpm3d_cases as dc
from conditional_score_diffusion_amd import _lib, sde_lib
from conditional_score_diffusion_amd.models import utils as mutils


def planned(case, **model_keys):
    cfg, B = dc.make_config(case)
    cfg.model.csd_planned = True
    for k, v in model_keys.items():
        setattr(cfg.model, k, v)
    return cfg, mutils.create_model(cfg)


# ---- H1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(dc.CASES))
def test_state_dict_matches_reference_and_loads(case):
    cfg, model = planned(case)
    assert model.planned and model._h
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == list(dc.golden_shapes(case).items())
    model.load_state_dict(dc.params(case))
    # the handle's own table is that list as well, with the 5-D convolution weights
    n = _lib.lib().csd_unet_num_params(model._h)
    name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 5)()
    table = []
    for i in range(n):
        _lib.check(_lib.lib().csd_unet_param_info(model._h, i, ctypes.byref(name), ctypes.byref(ndim), shape), 'param_info')
        table.append((name.value.decode(), tuple(shape[j] for j in range(ndim.value))))
    assert table == list(dc.golden_shapes(case).items())
    assert any(len(s) == 5 for _, s in table)
    # sizes are planned on the host: packed weights, and a workspace that grows with the batch
    assert _lib.lib().csd_unet_packed_bytes(model._h) > 0
    assert 0 < _lib.lib().csd_unet_workspace_bytes(model._h, 1) < _lib.lib().csd_unet_workspace_bytes(model._h, 2)
    launches, flops, nbytes = model.stats(2)
    assert launches > 0 and flops > 0 and nbytes > 0


def test_opt_in_switches(monkeypatch):
    from conditional_score_diffusion_amd.models import ddpm3d
    cfg, _ = dc.make_config('B')
    assert not mutils.create_model(cfg).planned                      # the default stays the operator path
    assert ddpm3d.DDPM3D_paired_SR3(cfg, planned=True).planned
    monkeypatch.setenv('CSD_PLANNED', '1')
    assert mutils.create_model(cfg).planned
    monkeypatch.setenv('CSD_PLANNED', '0')
    assert not mutils.create_model(cfg).planned
    cfg.model.csd_planned = True
    m = mutils.create_model(cfg)
    assert m.planned and m.volume == (6, 10, 4) and (m.x_channels, m.y_channels) == (1, 1)


# ---- H2 ------------------------------------------------------------------------------------------------------------------------------
def test_fusable():
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    sx = sde_lib.cVESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    sy = sde_lib.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX_Y, dc.N_SCALES)
    cp, cc = get_predictor('conditional_reverse_diffusion'), get_corrector('conditional_langevin')
    runs = [('B', sx, cp, cc), ('A', {'x': sx, 'y': sy}, cp, cc),
            ('C', sde_lib.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES), get_predictor('reverse_diffusion'), get_corrector('langevin'))]
    for case, sde, pred, corr in runs:
        _, model = planned(case)
        assert fused.fusable(model, sde, pred, corr, 1, False, True)
        assert not fused.fusable(model, sde, pred, corr, 1, False, False)          # the VE SDEs: continuous time only
        assert not fused.fusable(model, sde, pred, corr, 2, False, True)
        cfg, _ = dc.make_config(case)
        assert not fused.fusable(mutils.create_model(cfg), sde, pred, corr, 1, False, True)      # a default-configured model


# ---- H3 ------------------------------------------------------------------------------------------------------------------------------
def test_construction_refusals():
    cfg, _ = dc.make_config('B')
    cfg.model.csd_planned = True
    cfg.data.shape_x = [1, 6, 10, 3]                                # 6 x 10 x 3 pools once: odd W
    cfg.data.shape_y = [1, 6, 10, 3]
    with pytest.raises(ValueError, match='odd extent'):
        mutils.create_model(cfg)
    cfg, _ = dc.make_config('A')                                    # two pooled levels: 6 x 20 x 8 -> 3 x 10 x 4 -> odd
    cfg.model.csd_planned = True
    cfg.data.shape_x = [1, 6, 20, 8]
    cfg.data.shape_y = [1, 6, 20, 8]
    with pytest.raises(ValueError, match='odd extent'):
        mutils.create_model(cfg)
    cfg, _ = dc.make_config('B')
    cfg.model.csd_planned = True
    cfg.model.nf = 48
    with pytest.raises(ValueError, match='nf = 48'):
        mutils.create_model(cfg)


def _create(**over):
    """csd_unet_create on case B's configuration with fields overridden -> (status, message)"""
    cfg = _lib.UNetConfig()
    cfg.arch, cfg.nf, cfg.n_levels, cfg.num_res_blocks = 2, 32, 2, 1
    cfg.ch_mult[0], cfg.ch_mult[1] = 1, 2
    cfg.x_channels, cfg.y_channels, cfg.out_channels = 1, 1, 1
    cfg.conditional, cfg.act, cfg.precision = 1, _lib.ACT_IDS['swish'], _lib.PREC_IDS['fp16x3']
    cfg.vol[0], cfg.vol[1], cfg.vol[2] = 6, 10, 4
    for k, v in over.items():
        if isinstance(v, (tuple, list)):
            for i, e in enumerate(v):
                getattr(cfg, k)[i] = e
        else:
            setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = _lib.lib().csd_unet_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().csd_last_error().decode()
    if rc == 0:
        _lib.lib().csd_unet_destroy(h)
    return rc, msg


def test_library_refusals():
    assert _create()[0] == 0
    for over, words in [(dict(resamp_with_conv=1), 'resamp_with_conv'), (dict(conditional=0), 'conditional'), (dict(nf=48), 'nf = 48'),
                        (dict(vol=(6, 10, 3)), 'odd extent'), (dict(vol=(6, 1, 4)), 'odd extent'),
                        (dict(precision=_lib.PREC_IDS['fp16']), 'fp16x3'), (dict(precision=_lib.PREC_IDS['fp16f8']), 'fp16x3')]:
        rc, msg = _create(**over)
        assert rc == -1 and words in msg and '3-D' in msg, (over, rc, msg)
    # a handle of the 3-D family has no training graph, no digest
    cfg, model = planned('B')
    lib = _lib.lib()
    assert lib.csd_unet_train_workspace_bytes(model._h, 2, 0.0) == 0 and '3-D' in lib.csd_last_error().decode()
    assert lib.csd_unet_train_release(model._h, None) == -1 and '3-D' in lib.csd_last_error().decode()
    assert lib.csd_unet_backward_marks(model._h, None, None, 0) == -1 and '3-D' in lib.csd_last_error().decode()


def test_every_up_block_has_a_shortcut_convolution():
    """csd_unet_create refuses a ch_mult for which an up block's concatenated width equals its out_ch (that block would have no Conv_2 and
    the concatenation itself would be the residual).  No ch_mult reaches that refusal: an up block at level l reads h (nf * m_l or
    nf * m_(l+1) channels) and a skip tensor of at least nf channels and puts out nf * m_l, so h alone is already as wide as the output
    or the skip is (nf * m_l, the level's own block or Downsample output).  Checked here over every ch_mult of up to three levels with
    multipliers 1 .. 4 and 1 or 2 blocks per level: the library accepts each, and every up block of the model has Conv_2."""
    from conditional_score_diffusion_amd.models import ddpm3d
    for levels in (1, 2, 3):
        for mult in itertools.product((1, 2, 3, 4), repeat=levels):
            for nrb in (1, 2):
                rc, msg = _create(n_levels=levels, ch_mult=mult, num_res_blocks=nrb, vol=(8, 8, 8))
                assert rc == 0, (mult, nrb, msg)
                cfg, _ = dc.make_config('B')
                cfg.model.ch_mult, cfg.model.num_res_blocks = mult, nrb
                with torch.device('meta'):
                    model = ddpm3d.DDPM3D_paired_SR3(cfg)
                ups = [i for i, (k, a) in enumerate(model._mods) if k == 'res'][-(levels * (nrb + 1)):]
                assert all(hasattr(model.all_modules[i], 'Conv_2') for i in ups), (mult, nrb)


def test_call_refusals():
    from conditional_score_diffusion_amd.sampling import fused
    cfg, model = planned('B')
    model.eval()
    x, y, labels = dc.case_inputs('B')
    # another volume than the configured one: refused before anything touches the device, both volumes named
    with pytest.raises(ValueError, match=r'\(6, 10, 2\).*\(6, 10, 4\)'):
        model({'x': x[..., :2].contiguous(), 'y': y[..., :2].contiguous()}, labels)
    with pytest.raises(ValueError, match=r'\(12, 10, 4\).*\(6, 10, 4\)'):
        model({'x': torch.cat([x, x], dim=2), 'y': torch.cat([y, y], dim=2)}, labels)
    with pytest.raises(RuntimeError, match='no CPU'):                # the configured volume: there is no CPU path
        model({'x': x, 'y': y}, labels)
    model.train()
    with pytest.raises(NotImplementedError, match='training mode'):  # training mode keeps the operator path's behaviour
        model({'x': x, 'y': y}, labels)
    model.eval()
    cfg_c, model_c = planned('C')
    sde = sde_lib.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    shape = (2,) + tuple(cfg_c.data.shape_x)
    with pytest.raises(NotImplementedError, match='3-D'):
        fused.run(model_c, sde, shape, None, 2, dc.SNR, dc.EPS, True, inpaint=(torch.zeros(shape), torch.ones(shape)))
