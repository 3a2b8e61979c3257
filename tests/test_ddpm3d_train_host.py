"""What the bounds of tests/test_gpu_ddpm3d_train.py mean, on the CPU (no GPU needed), in the style of test_train_ops_sensitivity.py:

  * torch's own float32 gradients pass every bound of the operator sweep and of the model-level network test: the bounds are not
    tighter than fp32 itself;
  * a torch emulation of the split-bf16 product of csd_conv3d_wgrad (truncated hi, rounded lo, hi*hi + hi*lo + lo*hi, float64
    accumulation) passes the 5e-5 bound with at least 2x margin on every shape of the sweep, at both dy scales;
  * subtly wrong references miss the bounds by more than 10x: an unflipped weight in dx, D and W swapped in dw, a lost K split
    (one sample's, and one brick's, contribution dropped), the pool backward without its 1/8;
  * CPU tensors in training mode, and CPU input gradients, still raise.

Measured (worst over the sweep; both dy scales give the same figures, the scale is a power of two):
  torch fp32       dw 5.9e-07 (bound 1e-5)   db 4.8e-07 (bound 1e-5)   dx 0.054 of 3e-6 * max(1, sqrt(27 Cout) / 8)
  split bf16       dw 1.8e-05 (bound 5e-5, margin 2.8x); extent 1 with B = 1: 3.3e-05 (one product per weight: within the bound, no 2x
                   margin - shown instead on the same volume with B = 8: 1.5e-05)
  torch fp32 net   worst err / allowance 0.24 (A), 0.19 (B), 0.31 (C) at tol 2e-5
  wrong refs       unflipped dx >= 1.1 (bound <= 1.7e-5), D <-> W in dw >= 1.1, lost sample >= 0.52, lost brick >= 0.32 (bound 5e-5),
                   pool backward without 1/8: 7.0 (bound 1e-6)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddpm3d_cases as dc
import ddpm3d_train_cases as tc


@pytest.mark.parametrize('idx', range(len(tc.SWEEP)))
def test_torch_fp32_and_split_bf16_within_bounds(idx):
    B, vol, Cin, Cout = tc.SWEEP[idx]
    d = tc.op_case(idx)
    rdx, rdw, rdb = tc.op_ref(idx)
    for s in tc.DY_SCALES:
        dy = d['dy'] * s
        dx, dw, db = tc.conv_grads(d['a'], d['w'], dy, torch.float32)
        e = (tc.rel(dx, rdx * s), tc.rel(dw, rdw * s), tc.rel(db, rdb * s))
        eb = tc.rel(tc.dw_split_bf16(d['a'], dy), rdw * s)
        print('case %d scale %g: torch fp32 dx %.2e (bound %.2e) dw %.2e db %.2e; split-bf16 dw %.2e' % (idx, s, e[0], tc.dx_bound(Cout), e[1], e[2], eb))
        assert e[0] < tc.dx_bound(Cout) and e[1] < tc.DW_BOUND['fp32'] and e[2] < tc.DB_BOUND
        # extent 1, B = 1 is ONE product per weight: nothing averages, and the dropped lo*lo term alone is up to 2^-14 = 6e-5 of it.  The
        # shape passes the bound but not with a 2x margin; the margin is shown on the same volume with 8 samples instead (shape changed,
        # not the bound)
        assert eb < tc.DW_BOUND['fp16x3'] / (1 if idx == 0 else 2)
    if idx == 0:
        rs = np.random.RandomState(7)
        a8 = torch.from_numpy(rs.standard_normal((8, 1, 1, 1, Cin)).astype(np.float32))
        dy8 = torch.from_numpy(rs.standard_normal((8, 1, 1, 1, Cout)).astype(np.float32))
        eb = tc.rel(tc.dw_split_bf16(a8, dy8), tc.conv_grads(a8, d['w'], dy8)[1])
        print('extent 1 with B = 8: split-bf16 dw %.2e' % eb)
        assert eb < tc.DW_BOUND['fp16x3'] / 2


def test_extent_one_has_only_the_centre_tap():
    rdx, rdw, rdb = tc.op_ref(0)
    off = rdw.clone()
    off[:, :, 1, 1, 1] = 0
    assert float(off.abs().max()) == 0.0 and float(rdw[:, :, 1, 1, 1].abs().max()) > 0


@pytest.mark.parametrize('idx', [2, 4, 5, 6])
def test_wrong_references_miss_by_10x(idx):
    B, vol, Cin, Cout = tc.SWEEP[idx]
    d = tc.op_case(idx)
    rdx, rdw, rdb = tc.op_ref(idx)
    a, w, dy = d['a'].double(), d['w'].double(), d['dy'].double()
    # dx with the weight transposed but NOT flipped
    wrong = F.conv3d(dy.permute(0, 4, 1, 2, 3), w.transpose(0, 1).contiguous(), padding=1).permute(0, 2, 3, 4, 1)
    e = tc.rel(wrong, rdx)
    print('case %d: unflipped dx %.2e (bound %.2e)' % (idx, e, tc.dx_bound(Cout)))
    assert e > 10 * tc.dx_bound(Cout)
    # dw with the D and W taps swapped
    e = tc.rel(rdw.transpose(2, 4), rdw)
    print('case %d: D <-> W in dw %.2e' % (idx, e))
    assert e > 10 * tc.DW_BOUND['fp16x3']
    # a lost K split: the last sample, or the first 4 x 8 x 4 brick of the first sample
    if B > 1:
        dy2 = dy.clone()
        dy2[-1] = 0
        e = tc.rel(tc.conv_grads(a, w, dy2)[1], rdw)
        print('case %d: lost sample in dw %.2e' % (idx, e))
        assert e > 10 * tc.DW_BOUND['fp16x3']
    dy2 = dy.clone()
    dy2[0, :4, :8, :4] = 0
    e = tc.rel(tc.conv_grads(a, w, dy2)[1], rdw)
    print('case %d: lost brick in dw %.2e' % (idx, e))
    assert e > 10 * tc.DW_BOUND['fp16x3']


def test_pool_backward_without_its_eighth_misses():
    x = torch.randn(2, 3, 4, 6, 2, dtype=torch.float64, requires_grad=True)
    g = torch.randn(2, 3, 2, 3, 1, dtype=torch.float64)
    ref, = torch.autograd.grad(F.avg_pool3d(x, 2, 2), x, g)
    right = F.interpolate(g, scale_factor=2, mode='nearest') / 8
    assert tc.rel(right, ref) < 1e-12
    assert tc.rel(right * 8, ref) > 10 * 1e-6
    y = torch.randn(2, 3, 2, 3, 1, dtype=torch.float64, requires_grad=True)
    gu = torch.randn(2, 3, 4, 6, 2, dtype=torch.float64)
    ref, = torch.autograd.grad(F.interpolate(y, scale_factor=2, mode='nearest'), y, gu)
    assert tc.rel(F.avg_pool3d(gu, 2, 2) * 8, ref) < 1e-12 and tc.rel(F.avg_pool3d(gu, 2, 2), ref) > 10 * 1e-6


@pytest.mark.parametrize('case', sorted(dc.CASES))
def test_torch_fp32_network_gradients_within_bound(case):
    x, y, labels = dc.case_inputs(case)
    p = dc.params(case)
    assert tc.rel(tc.forward_as(p, case, x, y, labels, torch.float64), dc.forward64(p, case, x, y, labels)) < 1e-13
    val, rg, rdx = tc.net_ref(case)
    p32 = {k: v.float().clone().requires_grad_(True) for k, v in p.items()}
    x32 = x.clone().requires_grad_(True)
    (tc.forward_as(p32, case, x32, y, labels, torch.float32) * tc.net_g(case)).sum().backward()
    got = {k: v.grad for k, v in p32.items()}
    got['<x>'] = x32.grad
    ref = dict(rg)
    ref['<x>'] = rdx
    worst, where = tc.grad_check(got, ref, 2e-5, 1e-7)
    print('case %s: torch fp32 worst err / allowance %.3f at %s' % (case, worst, where))
    assert worst <= 1.0


def test_cpu_tensors_still_raise():
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = dc.make_config('C')
    model = mutils.create_model(cfg)
    x, y, labels = dc.case_inputs('C')
    model.train()
    with pytest.raises(NotImplementedError, match='training mode'):
        model(x, labels)
    model.eval()
    with pytest.raises(NotImplementedError, match='input gradients'):
        model(x.clone().requires_grad_(True), labels)
    with pytest.raises(RuntimeError, match='no CPU'):
        model(x, labels)


def test_trainer_picks_the_loss_by_class():
    """conditional for the paired 3-D classes, unconditional for ddpm3D; the 2-D rule (y_channels) is untouched"""
    from conditional_score_diffusion_amd import train

    class T(train.Trainer):
        def __init__(self, model, sde):
            self.config, self.model, self.sde = dc.make_config('B')[0], model, sde
            self.config.training.likelihood_weighting = self.config.training.reduce_mean = True

    seen = []
    orig = train.losses.get_general_sde_loss_fn
    train.losses.get_general_sde_loss_fn = lambda sde, tr, conditional=False, **k: seen.append(conditional)
    try:
        for name, want in (('DDPM3D', False), ('DDPM3D_paired', True), ('DDPM3D_paired_SR3', True), ('DDPM', False), ('NCSNpp', False)):
            seen.clear()
            T(type(name, (), {})(), tc.loss_sdes('C'))._build_loss_fns()
            assert seen == [want, want], (name, seen)
        seen.clear()
        T(type('NCSNpp', (), {'y_channels': 3})(), tc.loss_sdes('C'))._build_loss_fns()
        assert seen == [True, True]
    finally:
        train.losses.get_general_sde_loss_fn = orig
