"""Host-side checks of the 3-D DDPM networks (models/ddpm3d.py): registry, state_dict layout against the reference's recorded
(name, shape) list, the documented refusals, and the presence of the new C-ABI entries.  No GPU."""
import pytest
import torch

import ddpm3d_cases as dc
from conditional_score_diffusion_amd import _lib
from conditional_score_diffusion_amd.models import utils as mutils

def test_names_registered():
    from conditional_score_diffusion_amd.models import ddpm3d
    assert mutils.get_model('ddpm3D') is ddpm3d.DDPM3D
    assert mutils.get_model('ddpm3D_paired') is ddpm3d.DDPM3D_paired
    assert mutils.get_model('ddpm3D_paired_SR3') is ddpm3d.DDPM3D_paired_SR3


@pytest.mark.parametrize('case', sorted(dc.CASES))
def test_state_dict_matches_reference(case):
    cfg, _ = dc.make_config(case)
    with torch.device('meta'):
        model = mutils.create_model(cfg)
    mine = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    ref = list(dc.golden_shapes(case).items())
    assert mine == ref
    assert any(len(s) == 5 for _, s in mine)          # the conv weights are [Cout, Cin, 3, 3, 3]


def test_construction_refusals(monkeypatch):
    cfg, _ = dc.make_config('B')
    cfg.model.resamp_with_conv = True
    with pytest.raises(NotImplementedError, match='resamp_with_conv'):
        mutils.create_model(cfg)
    cfg, _ = dc.make_config('B')
    cfg.model.conditional = False
    with pytest.raises(NotImplementedError, match='conditional=False'):
        mutils.create_model(cfg)
    for prec in ('fp16', 'fp16f8'):
        cfg, _ = dc.make_config('B', precision=prec)
        with pytest.raises(ValueError, match="'fp32' or 'fp16x3'"):
            mutils.create_model(cfg)
    cfg, _ = dc.make_config('B', precision='bf16')
    with pytest.raises(ValueError, match='unknown csd precision'):
        mutils.create_model(cfg)
    monkeypatch.setenv('CSD_PRECISION', 'fp16f8')
    cfg, _ = dc.make_config('B')
    with pytest.raises(ValueError, match="'fp32' or 'fp16x3'"):
        mutils.create_model(cfg)
    monkeypatch.setenv('CSD_PRECISION', 'fp32')
    assert mutils.create_model(cfg).precision == 'fp32'
    monkeypatch.delenv('CSD_PRECISION')
    assert mutils.create_model(cfg).precision == 'fp16x3'


def test_call_refusals():
    cfg, B = dc.make_config('B')
    model = mutils.create_model(cfg)
    x, y, labels = dc.case_inputs('B')
    model.train()
    with pytest.raises(NotImplementedError, match='training mode'):
        model({'x': x, 'y': y}, labels)
    model.eval()
    with pytest.raises(NotImplementedError, match='input gradients'):
        model({'x': x.clone().requires_grad_(True), 'y': y}, labels)
    # 6 x 10 x 4 pools once; 6 x 10 x 3 has an odd extent at the pooled level, 12 x 10 x 4 would be fine
    with pytest.raises(ValueError, match='odd extent'):
        model({'x': x[..., :3].contiguous(), 'y': y[..., :3].contiguous()}, labels)
    cfg, _ = dc.make_config('A')                      # two pooled levels: 12 x 20 x 8 -> 6 x 10 x 4 -> 3 x 5 x 2; 6 x 20 x 8 -> 3 x .. -> odd
    model = mutils.create_model(cfg).eval()
    xa, ya, _ = dc.case_inputs('A')
    with pytest.raises(ValueError, match='odd extent'):
        model({'x': xa[:, :, :6].contiguous(), 'y': ya[:, :, :6].contiguous()}, labels)
    # no CPU fallback
    with pytest.raises(RuntimeError, match='no CPU'):
        model({'x': xa, 'y': ya}, labels)


def test_device_and_fusable():
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    cfg, _ = dc.make_config('B')
    model = mutils.create_model(cfg)
    assert model.device == torch.device('cpu')
    sde = sde_lib.cVESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    assert not fused.fusable(model, sde, get_predictor('conditional_reverse_diffusion'), get_corrector('conditional_langevin'), 1, False,
                             True)


def test_c_abi_symbols():
    import ctypes
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('csd_conv3d_block', 'csd_conv3d_block_scratch_bytes', 'csd_avgpool3d_2_ndhwc', 'csd_nearest_up2_3d_ndhwc',
                 'csd_groupnorm_scale_shift', 'csd_groupnorm_scale_shift_scratch_bytes'):
        assert hasattr(l, name), name
        assert name in _lib.SIGNATURES, name
    f = l.csd_conv3d_block_scratch_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    # the packed fp16 hi | lo weight of a 64 -> 64 layer: 2 cout tiles x 4 chunks x 27 taps x 2 KiB, plus slack
    assert f(64, 64) >= 2 * 4 * 27 * 2048
    assert f(2, 64) >= 27 * 2 * 64 * 4
