"""Host-side checks of the planned training graph of the 3-D DDPM networks (``DDPM3D(planned_train=...)``, csrc/train_graph3d.h): the
switch and its default, what stays untouched with it off, the refusals that need no GPU, and the workspace the dry run plans.  No GPU."""
import pytest
import torch

import ddpm3d_cases as dc
from conditional_score_diffusion_amd import _lib, losses, sde_lib
from conditional_score_diffusion_amd.models import ddpm3d
from conditional_score_diffusion_amd.models import utils as mutils


def test_switch_spellings_and_default(monkeypatch):
    monkeypatch.delenv('CSD_PLANNED_TRAIN', raising=False)
    cfg, _ = dc.make_config('B')
    m = mutils.create_model(cfg)
    assert m.planned_train is False and m.planned is False           # the default: off
    assert ddpm3d.DDPM3D_paired_SR3(cfg, planned_train=True).planned_train
    cfg.model.csd_planned_train = True
    assert mutils.create_model(cfg).planned_train
    assert not ddpm3d.DDPM3D_paired_SR3(cfg, planned_train=False).planned_train      # the argument wins over the config
    cfg, _ = dc.make_config('B')
    monkeypatch.setenv('CSD_PLANNED_TRAIN', '1')
    assert mutils.create_model(cfg).planned_train
    cfg.model.csd_planned_train = False
    assert not mutils.create_model(cfg).planned_train                # the config wins over the environment
    cfg, _ = dc.make_config('B')
    monkeypatch.setenv('CSD_PLANNED_TRAIN', '0')
    assert not mutils.create_model(cfg).planned_train


@pytest.mark.parametrize('case', sorted(dc.CASES))
def test_on_creates_the_handle_and_off_leaves_everything(case, monkeypatch):
    monkeypatch.delenv('CSD_PLANNED_TRAIN', raising=False)
    monkeypatch.delenv('CSD_PLANNED', raising=False)
    cfg, B = dc.make_config(case)
    off = mutils.create_model(cfg)
    assert getattr(off, 'train_executor', 'operators') == 'operators' and off._h is None and not hasattr(off, 'volume')
    cfg.model.csd_planned_train = True
    on = mutils.create_model(cfg)
    assert on.train_executor == 'planned' and on._h and not on.planned
    name, nf, ch_mult, nrb, B, vol, xc, yc = dc.CASES[case]
    assert on.volume == vol and (on.x_channels, on.y_channels) == (xc, yc)
    assert on._x_shape(B) == (B, xc) + vol and on._out_shape(B) == (B, int(cfg.model.output_channels)) + vol
    assert [k for k, _ in on.named_parameters()] == on._param_names == [k for k, _ in off.named_parameters()]
    # the dry run plans the workspace on the host: it grows with the batch, and dropout adds the masks
    l = _lib.lib()
    w1, w2, w2d = (l.csd_unet_train_workspace_bytes(on._h, b, p) for b, p in ((1, 0.0), (2, 0.0), (2, 0.1)))
    assert 0 < w1 < w2 < w2d
    assert l.csd_unet_train_workspace_bytes(on._h, 0, 0.0) == 0


def test_a_handle_without_the_field_has_no_training_graph():
    """csd_unet_config.planned_train is the opt-in at the handle: 0 in a zeroed struct, and then the training entries refuse the handle
    naming 3-D, as they did before the graph existed (a ``csd_planned``-only model keeps its sizes)"""
    l = _lib.lib()
    assert _lib.UNetConfig().planned_train == 0
    cfg, _ = dc.make_config('B')
    cfg.model.csd_planned = True
    off = mutils.create_model(cfg)
    assert off._h and off._cfg.planned_train == 0 and not hasattr(off, 'train_executor')
    assert l.csd_unet_train_workspace_bytes(off._h, 2, 0.0) == 0 and '3-D' in l.csd_last_error().decode()
    assert l.csd_unet_backward_marks(off._h, None, None, 0) == -1 and 'planned_train' in l.csd_last_error().decode()
    cfg.model.csd_planned_train = True
    on = mutils.create_model(cfg)
    assert on.planned and on._cfg.planned_train == 1
    assert l.csd_unet_train_workspace_bytes(on._h, 2, 0.0) > 0
    assert l.csd_unet_train_release(on._h, None) == 0 and l.csd_unet_backward_marks(on._h, None, None, 0) == 0
    assert l.csd_unet_workspace_bytes(on._h, 2) == l.csd_unet_workspace_bytes(off._h, 2)      # (the inference plan does not know the field)


def test_cpu_tensors_keep_the_refusals():
    x, y, labels = dc.case_inputs('B')
    for planned_train in (False, True):
        cfg, _ = dc.make_config('B')
        cfg.model.csd_planned_train = planned_train
        model = mutils.create_model(cfg)
        model.train()
        with pytest.raises(NotImplementedError, match='training mode is not provided on CPU tensors'):
            model({'x': x, 'y': y}, labels)
        model.eval()
        with pytest.raises(NotImplementedError, match='input gradients are not provided on CPU tensors'):
            model({'x': x.clone().requires_grad_(True), 'y': y}, labels)
    # the planned graph is made for one volume (GPU or not, the shape check comes first on the planned path: see the GPU test)


def test_fused_loss_gate():
    sde = sde_lib.cVESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    x, y, labels = dc.case_inputs('B')
    cfg, _ = dc.make_config('B')
    model = mutils.create_model(cfg)
    with pytest.raises(NotImplementedError, match='3-D classes'):
        losses._require_fused(model, [('x', x)], sde)
    fn = losses.get_general_sde_loss_fn(sde, True, conditional=True, fused=True)
    with pytest.raises(NotImplementedError, match='3-D classes'):
        fn(model, (y, x))
    cfg.model.csd_planned_train = True
    model = mutils.create_model(cfg)
    with pytest.raises(NotImplementedError, match='GPU tensors only'):      # admitted as a model; the fused passes are HIP kernels
        losses._require_fused(model, [('x', x)], sde)
    with pytest.raises(NotImplementedError, match='3 SDEs'):
        losses._require_fused(model, [('x', x)], {'x': sde, 'y': sde, 'z': sde})


def test_likelihood_still_refuses_the_3d_networks():
    from conditional_score_diffusion_amd import likelihood
    cfg, _ = dc.make_config('C')
    cfg.model.csd_planned_train = True
    model = mutils.create_model(cfg)
    sde = sde_lib.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    with pytest.raises(NotImplementedError, match='3-D networks'):
        likelihood.get_likelihood_fn(sde, lambda v: v)(model, torch.zeros((1,) + tuple(cfg.data.shape_x)))
