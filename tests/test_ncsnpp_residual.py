"""progressive_input = 'residual' (the CIFAR-10 / CelebA NCSN++ configs) on the planned NCSN++ graph: the registry, the reference's
state_dict layout and the fused-sampler dispatch.  Host only."""
import os

import numpy as np
import pytest

import cases

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'ncsnpp.npz')


def paired_residual_config():
    return cases.make_ncsnpp_config(name='ncsnpp_paired', channels=6, nf=32, ch_mult=(1, 2), attn_resolutions=(16,),
                                    progressive='none', progressive_input='residual')


def _keys(model):
    return ['%s|%s' % (k, ','.join(map(str, v.shape))) for k, v in model.state_dict().items()]


@pytest.mark.parametrize('case', ['ncsnpp_residual_input', 'ncsnpp_nofir_residual'])
def test_residual_configs_get_the_planned_class(case):
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.models.ddpm import HipUNet
    from conditional_score_diffusion_amd.sampling import correctors, fused, predictors
    cfg, B, x, labels = cases.ncsnpp_case(case)
    model = mutils.create_model(cfg)
    assert isinstance(model, HipUNet)
    assert _keys(model) == [str(s) for s in np.load(GOLD)[case + '_keys']]
    sde = sde_lib.VESDE(0.01, 50., 1000)
    assert fused.fusable(model, sde, predictors.ReverseDiffusionPredictor, correctors.LangevinCorrector, 1, False, True)


def test_paired_residual_config_gets_the_planned_class():
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.models.ddpm import HipUNet
    cfg = paired_residual_config()
    model = mutils.create_model(cfg)
    assert isinstance(model, HipUNet)
    cfg_ops = paired_residual_config()
    cfg_ops.model.name = 'ncsnpp_paired_ops'
    ops_model = mutils.create_model(cfg_ops)
    assert not isinstance(ops_model, HipUNet)
    assert _keys(model) == _keys(ops_model)


@pytest.mark.parametrize('fir,sub', [(True, 'Conv2d_0'), (False, 'Conv_0')])
def test_pyramid_parameters_follow_the_reference_init(fir, sub):
    """layerspp.Downsample(with_conv=True): default_init() (fan-avg, scale 1) weight, zero bias"""
    import torch
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg = cases.make_ncsnpp_config(nf=32, ch_mult=(1, 2, 2), attn_resolutions=(8,), progressive='none', progressive_input='residual',
                                   fir=fir)
    torch.manual_seed(0)
    sd = mutils.create_model(cfg).state_dict()
    mods = {}
    for k in sd:
        mods.setdefault(k.split('.')[1], []).append(k)
    keys = [k for ks in mods.values() if sorted(x.split('.', 2)[2] for x in ks) == [sub + '.bias', sub + '.weight'] for k in ks]
    assert len(keys) == 4                    # the pyramid modules of the two levels below the top, weight + bias each
    for k in keys:
        v = sd[k]
        if k.endswith('bias'):
            assert torch.count_nonzero(v) == 0
            continue
        cout, cin = v.shape[:2]
        bound = np.sqrt(3.0 * 2.0 / ((cin + cout) * 9))      # variance_scaling(1, 'fan_avg', 'uniform')
        assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.5 * bound, k


def test_output_residual_and_other_options_still_raise():
    from conditional_score_diffusion_amd.models import utils as mutils
    with pytest.raises(NotImplementedError):
        mutils.create_model(cases.make_ncsnpp_config(progressive='residual', progressive_input='residual'))
    cfg = cases.make_ncsnpp_config(progressive_input='residual')
    cfg.model.progressive_combine = 'cat'
    with pytest.raises(NotImplementedError):
        mutils.create_model(cfg)
    cfg = cases.make_ncsnpp_config(progressive_input='residual')
    cfg.model.resblock_type = 'ddpm'
    with pytest.raises(NotImplementedError):
        mutils.create_model(cfg)
