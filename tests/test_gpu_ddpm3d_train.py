"""-m gpu: training the 3-D DDPM score networks - csd_conv3d_wgrad / the scale-invariant data gradient (csrc/conv3d_grad.hip), the
autograd shells of grad_ops_3d, the differentiable forward of models/ddpm3d.py, the losses and the Trainer on them.

References: float64 torch on the CPU (ddpm3d_train_cases: F.conv3d autograd; autograd of ddpm3d_cases.forward64, which the existing
tests pin to the reference's outputs; the training losses restated over forward64).  Error = max|got - ref| / max|ref| unless a formula
is given.  tests/test_ddpm3d_train_host.py shows on the CPU that torch's own float32 passes these bounds, that the split-bf16 arithmetic
passes its bound with margin and that subtly wrong references miss them by more than 10x.

Bounds:
  dw        fp32 1e-5, split bf16 5e-5 (the figures of test_gpu_train_ops.py); db 1e-5
  dx        3e-6 * max(1, sqrt(27 * Cout) / 8): test_gpu_ddpm3d.py's conv bound at the data gradient's reduction length
            all of them at dy ~ N(0, 1) and at dy ~ 2^-20 N(0, 1) (a naive fp16 split of dy fails the second)
  pool / upsample backward 1e-6; GroupNorm + act backward 2e-5
  network   per tensor err <= tol * scale + 1e-7 * total / sqrt(numel), tol 2e-5 (fp32) / 2e-4 (fp16x3)   (test_planned_graph_equals_operator_graph)
  loss      1e-4 relative; gradients err <= 1e-3 * scale + 1e-6 * total / sqrt(numel)                     (test_training_loss_and_grads_vs_reference)

Measured on the MI355X (both dy scales give the same figures to the printed digits):

  sweep case, B (D, H, W) Cin -> Cout     dw fp32    dw fp16x3    db         dx fp32 (/ bound)    dx fp16x3 (/ bound)
  1 (1, 1, 1)      32 -> 32               4.7e-08    3.3e-05      0          1.7e-07 (0.02)       8.5e-08 (0.01)    off-centre taps exactly 0
  3 (2, 2, 2)      64 -> 2                6.0e-08    6.0e-08      1.3e-07    1.2e-07 (0.04)       1.2e-07 (0.04)    thin: fp32 kernels in both modes
  3 (5, 7, 3)       2 -> 64               2.1e-07    2.1e-07      2.5e-08    7.7e-07 (0.05)       6.0e-07 (0.04)    thin dw; dx on the MFMA kernel
  1 (12, 12, 2)   128 -> 32               5.8e-07    1.4e-05      4.0e-08    9.9e-07 (0.09)       5.2e-07 (0.05)
  3 (3, 5, 2)      96 -> 64               1.4e-07    1.8e-05      6.2e-08    1.3e-06 (0.08)       4.4e-07 (0.03)
  1 (9, 17, 16)    64 -> 64               1.2e-06    1.4e-05      3.3e-08    1.5e-06 (0.09)       8.7e-07 (0.06)
  2 (5, 7, 3)      40 -> 72               2.7e-07    1.3e-05      4.3e-08    1.3e-06 (0.08)       1.3e-06 (0.08)
  bounds                                  1e-5       5e-5         1e-5

  avg_pool3d_2 backward 0 (exact), nearest_up2_3d backward 6.5e-08 (bound 1e-6)
  groupnorm_act backward on (3, 5, 2) x 64: swish dx 1.1e-07 dgamma 6.4e-08 dbeta 8.3e-08; none 1.0e-07 / 6.3e-08 / 5.5e-08 (bound 2e-5)
  network, training mode, worst err / allowance    A 0.29 (fp32) 0.17 (fp16x3)    B 0.19 / 0.11    C 0.34 / 0.14
  network, eval input gradient err / allowance     A 0.13 / 0.007    B 0.08 / 0.006    C 0.09 / 0.007
  eval output with vs without requires_grad        fp32 0 (bitwise)    fp16x3 6.7e-07 (A), 5.0e-07 (B), 5.3e-07 (C)    (bound 1e-5)
  loss, relative to float64 (bound 1e-4)           B 1.5e-07 / 1.2e-08    A 3.4e-08 / 5.4e-08    C 7.4e-08 / 7.1e-08
  loss gradients, worst err / allowance            B 0.007 / 0.043        A 0.008 / 0.031        C 0.008 / 0.034
  SGD with dropout 0.1, case B: 26.96 -> 9.83 (same mask) after 5 steps of lr 3.1e-4; Trainer (Adam, 3 steps): 26.6, 21.7, 24.7
  repeatability, batch independence (bitwise), out-of-domain arguments, dropout streams, one-rank RCCL: exact checks
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddpm3d_cases as dc
import ddpm3d_train_cases as tc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


# ---- operators ---------------------------------------------------------------------------------------------------------------------------
def _gpu_conv_grads(d, scale, precision):
    from conditional_score_diffusion_amd import grad_ops_3d as G
    a = d['a'].to(dev()).requires_grad_(True)
    w = d['w'].to(dev()).requires_grad_(True)
    b = torch.zeros(w.shape[0], device=dev(), requires_grad=True)
    y = G.conv3d(a, w, b, precision)
    y.backward((d['dy'] * scale).to(dev()))
    torch.cuda.synchronize()
    return a.grad, w.grad, b.grad


@pytest.mark.parametrize('scale', tc.DY_SCALES)
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('idx', range(len(tc.SWEEP)))
def test_conv3d_gradients_sweep(idx, precision, scale):
    B, vol, Cin, Cout = tc.SWEEP[idx]
    rdx, rdw, rdb = tc.op_ref(idx)
    dx, dw, db = _gpu_conv_grads(tc.op_case(idx), scale, precision)
    assert tuple(dw.shape) == (Cout, Cin, 3, 3, 3) and tuple(dx.shape) == (B,) + vol + (Cin,)
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all() and torch.isfinite(db).all()
    e = (tc.rel(dx, rdx * scale), tc.rel(dw, rdw * scale), tc.rel(db, rdb * scale))
    print('conv3d grads %s B=%d %s C=%d->%d dy scale %g: dx %.3e (bound %.3e) dw %.3e (bound %.0e) db %.3e' %
          (precision, B, vol, Cin, Cout, scale, e[0], tc.dx_bound(Cout), e[1], tc.DW_BOUND[precision], e[2]))
    if vol == (1, 1, 1):                        # padding is masked, not clamped: the 26 off-centre taps see nothing
        off = dw.clone()
        off[:, :, 1, 1, 1] = 0
        assert float(off.abs().max()) == 0.0
    assert e[0] < tc.dx_bound(Cout)
    assert e[1] < tc.DW_BOUND[precision]
    assert e[2] < tc.DB_BOUND


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('idx', [4, 5, 6])
def test_wgrad_repeatable_and_batch_independent(idx, precision):
    from conditional_score_diffusion_amd import grad_ops_3d as G
    B, vol, Cin, Cout = tc.SWEEP[idx]
    d = tc.op_case(idx)
    a, dy = d['a'].to(dev()), d['dy'].to(dev())
    one = G.conv3d_wgrad(a, dy, precision)
    two = G.conv3d_wgrad(a, dy, precision)
    assert torch.equal(one, two)
    for b in range(B):                           # sample b alone, inside the batch (the others' dy zeroed) and as a batch of one
        dz = torch.zeros_like(dy)
        dz[b] = dy[b]
        assert torch.equal(G.conv3d_wgrad(a, dz, precision), G.conv3d_wgrad(a[b:b + 1].contiguous(), dy[b:b + 1].contiguous(), precision)), b


def test_wgrad_out_of_domain_writes_nothing():
    from conditional_score_diffusion_amd._lib import PREC_IDS, lib, ptr
    a = torch.randn(1, 2, 2, 2, 8, device=dev())
    dy = torch.randn(1, 2, 2, 2, 8, device=dev())
    dw = torch.full((8, 8, 3, 3, 3), 7.0, device=dev())
    sc = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    ok = (1, 8, 8, 2, 2, 2, PREC_IDS['fp16x3'])
    bad = [(0, 8, 8, 2, 2, 2, 1), (1, 0, 8, 2, 2, 2, 1), (1, 8, 0, 2, 2, 2, 1), (1, 8, 8, 0, 2, 2, 1), (1, 8, 8, 2, 2, -1, 0),
           (1, 8, 8, 2, 2, 2, PREC_IDS['fp16']), (1, 8, 8, 2, 2, 2, PREC_IDS['fp16f8']), (1, 8, 8, 1 << 12, 1 << 12, 1 << 12, 1)]
    for args in bad:
        assert lib().csd_conv3d_wgrad(ptr(a), ptr(dy), ptr(dw), *args, ptr(sc), None) == -1, args          # CSD_ERR_INVALID
        assert lib().csd_conv3d_wgrad_scratch_bytes(*args) == 0, args
    for nulls in ((None, ptr(dy), ptr(dw), ptr(sc)), (ptr(a), None, ptr(dw), ptr(sc)), (ptr(a), ptr(dy), None, ptr(sc)), (ptr(a), ptr(dy), ptr(dw), None)):
        assert lib().csd_conv3d_wgrad(nulls[0], nulls[1], nulls[2], *ok, nulls[3], None) == -1
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all())
    assert 0 < lib().csd_conv3d_wgrad_scratch_bytes(*ok) <= sc.numel()
    assert lib().csd_conv3d_wgrad(ptr(a), ptr(dy), ptr(dw), *ok, ptr(sc), None) == 0
    torch.cuda.synchronize()
    assert not bool((dw == 7.0).any())


def test_pool_and_upsample_backward():
    from conditional_score_diffusion_amd import grad_ops_3d as G
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((2, 4, 6, 2, 8)).astype(np.float32))          # [B, D, H, W, C]
    g = torch.from_numpy(rs.standard_normal((2, 2, 3, 1, 8)).astype(np.float32))
    for name, fn, ref_fn, xin, gin in (('avg_pool3d_2', G.avg_pool3d_2, lambda v: F.avg_pool3d(v, 2, 2), x, g),
                                       ('nearest_up2_3d', G.nearest_up2_3d, lambda v: F.interpolate(v, scale_factor=2, mode='nearest'), g, x)):
        x64 = xin.double().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        ref, = torch.autograd.grad(ref_fn(x64), x64, gin.double().permute(0, 4, 1, 2, 3).contiguous())
        xg = xin.to(dev()).requires_grad_(True)
        got, = torch.autograd.grad(fn(xg), xg, gin.to(dev()))
        e = tc.rel(got, ref.permute(0, 2, 3, 4, 1))
        print('%s backward: %.3e' % (name, e))
        assert e < 1e-6


@pytest.mark.parametrize('act', ['swish', 'none'])
def test_groupnorm_act_backward_on_a_volume(act):
    from conditional_score_diffusion_amd import grad_ops_3d as G
    rs = np.random.RandomState(6)
    B, vol, C = 2, (3, 5, 2), 64
    x = torch.from_numpy((1.5 * rs.standard_normal((B,) + vol + (C,)) + 0.3).astype(np.float32))
    gamma = torch.from_numpy((1 + 0.3 * rs.standard_normal(C)).astype(np.float32))
    beta = torch.from_numpy((0.2 * rs.standard_normal(C)).astype(np.float32))
    g = torch.from_numpy(rs.standard_normal((B,) + vol + (C,)).astype(np.float32))
    x64, g64, b64 = x.double().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y64 = F.group_norm(x64, 32, g64, b64, eps=1e-6)
    y64 = F.silu(y64) if act == 'swish' else y64
    rdx, rdg, rdb = torch.autograd.grad(y64, (x64, g64, b64), g.double().permute(0, 4, 1, 2, 3).contiguous())
    xg, gg, bg = x.to(dev()).requires_grad_(True), gamma.to(dev()).requires_grad_(True), beta.to(dev()).requires_grad_(True)
    y = G.groupnorm_act(xg, gg, bg, act=act)
    assert tc.rel(y, y64.permute(0, 2, 3, 4, 1)) < 2e-5
    dx, dg, db = torch.autograd.grad(y, (xg, gg, bg), g.to(dev()))
    e = (tc.rel(dx, rdx.permute(0, 2, 3, 4, 1)), tc.rel(dg, rdg), tc.rel(db, rdb))
    print('groupnorm_act %s backward on %s: dx %.3e dgamma %.3e dbeta %.3e' % (act, vol, *e))
    assert max(e) < 2e-5


# ---- networks ----------------------------------------------------------------------------------------------------------------------------
def build(case, precision, dropout=0.0, trainer_keys=False):
    from conditional_score_diffusion_amd.config_dict import ConfigDict
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = dc.make_config(case, precision=precision)
    cfg.model.dropout = dropout
    cfg.seed = 42
    cfg.training.likelihood_weighting = cfg.training.reduce_mean = True
    if trainer_keys:
        cfg.model.ema_rate = 0.999
        cfg.optim = ConfigDict(weight_decay=0, optimizer='Adam', lr=2e-4, beta1=0.9, eps=1e-8, warmup=2, grad_clip=1)
    model = mutils.create_model(cfg)
    model.load_state_dict(dc.params(case))
    return cfg, model.to(dev())


def gpu_inputs(case):
    x, y, labels = dc.case_inputs(case)
    return x.to(dev()), None if y is None else y.to(dev()), labels.to(dev())


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('fp16x3', 2e-4)])
@pytest.mark.parametrize('case', sorted(dc.CASES))
def test_network_gradients_vs_float64(case, precision, tol):
    """training mode, dropout 0, loss = sum(out * g): every parameter gradient and the input gradient; then eval mode: the input
    gradient of sum(out) alone, and the eval output with and without requires_grad"""
    cfg, model = build(case, precision)
    x, y, labels = gpu_inputs(case)
    val, rg, rdx = tc.net_ref(case)
    model.train()
    xg = x.clone().requires_grad_(True)
    out = dc.call(model, case, xg, y, labels)
    assert out.requires_grad and model._train_calls == 1
    loss = (out * tc.net_g(case).to(dev())).sum()
    loss.backward()
    got = {k: v.grad for k, v in model.named_parameters()}
    got['<x>'] = xg.grad
    ref = dict(rg)
    ref['<x>'] = rdx
    assert set(got) == set(ref)
    worst, where = tc.grad_check(got, ref, tol, 1e-7)
    print('network %s %s training gradients: loss %.6e (float64 %.6e), worst err / allowance %.3f at %s' % (case, precision, float(loss.detach()), val, worst, where))
    assert abs(float(loss.detach()) - val) <= 1e-4 * abs(val) + 1e-4 * float((dc.forward64(dc.params(case), case, *dc.case_inputs(case)).abs() * tc.net_g(case).abs()).sum())
    assert worst <= 1.0, where
    # eval mode
    model.eval()
    xg = x.clone().requires_grad_(True)
    out_g = dc.call(model, case, xg, y, labels)
    dx, = torch.autograd.grad(out_g.sum(), xg)
    assert all(p.grad is got[k] for k, p in model.named_parameters())         # (the parameters took nothing from this)
    _, _, rdx_sum = tc.net_ref(case, 'sum')
    worst, _ = tc.grad_check({'<x>': dx}, {'<x>': rdx_sum}, tol, 1e-7)
    with torch.no_grad():
        out_i = dc.call(model, case, x, y, labels)
    e = tc.rel(out_g, out_i)
    print('network %s %s eval: input gradient err / allowance %.3f; output with vs without requires_grad %.3e' % (case, precision, worst, e))
    assert worst <= 1.0
    assert e < 1e-5


def _loss_and_grads(case, precision, dropout=0.0, model=None):
    from conditional_score_diffusion_amd import losses
    if model is None:
        cfg, model = build(case, precision, dropout)
    name = dc.CASES[case][0]
    x, y = tc.loss_batch(case)
    u, tape = tc.loss_tape(case)
    fn = losses.get_general_sde_loss_fn(tc.loss_sdes(case), True, conditional=name != 'ddpm3D', reduce_mean=True, continuous=True,
                                        likelihood_weighting=True)
    batch = x.to(dev()) if name == 'ddpm3D' else (y.to(dev()), x.to(dev()))
    it = iter(tape)
    o_rand, o_like = torch.rand, torch.randn_like
    torch.rand = lambda *a, **k: u.clone()
    torch.randn_like = lambda t, **k: next(it).to(t.device)
    try:
        model.zero_grad()
        loss = fn(model, batch)
    finally:
        torch.rand, torch.randn_like = o_rand, o_like
    assert model.training and loss.requires_grad
    loss.backward()
    return float(loss.detach()), {k: v.grad.clone() for k, v in model.named_parameters()}, model


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', ['B', 'A', 'C'])
def test_training_loss_and_grads_vs_float64(case, precision):
    """losses.get_general_sde_loss_fn(sde, True, ...): SR3 on cVESDE (B), the two-SDE pair (A), unconditional (C)"""
    loss, grads, _ = _loss_and_grads(case, precision)
    r_loss, r_grads = tc.loss_ref(case)
    worst, where = tc.grad_check(grads, r_grads, 1e-3, 1e-6)
    print('loss %s %s: %.8e (float64 %.8e, rel %.2e); worst gradient err / allowance %.4f at %s' %
          (case, precision, loss, r_loss, abs(loss - r_loss) / abs(r_loss), worst, where))
    assert abs(loss - r_loss) <= 1e-4 * abs(r_loss)
    assert worst <= 1.0, where


def test_dropout_streams():
    """the mask is a pure function of (dropout_seed, _train_calls, index): same call index -> bitwise the same loss and gradients,
    another call index -> another mask; eval mode has no dropout"""
    l1, g1, model = _loss_and_grads('B', 'fp16x3', dropout=0.1)
    assert model._train_calls == 1
    l2, g2, _ = _loss_and_grads('B', 'fp16x3', model=model)
    assert model._train_calls == 2 and l2 != l1
    model._train_calls = 0
    l3, g3, _ = _loss_and_grads('B', 'fp16x3', model=model)
    assert l3 == l1 and all(torch.equal(g1[k], g3[k]) for k in g1)
    l0, _, _ = _loss_and_grads('B', 'fp16x3', dropout=0.0)
    assert l0 != l1
    model.eval()
    x, y, labels = gpu_inputs('B')
    xg = x.clone().requires_grad_(True)
    _, ref = build('B', 'fp16x3', 0.0)
    ref.eval()
    assert torch.equal(model({'x': xg, 'y': y}, labels), ref({'x': x.clone().requires_grad_(True), 'y': y}, labels))


def test_sgd_steps_reduce_the_loss_with_dropout():
    """plain SGD on a fixed batch and fixed noise, dropout 0.1 with a new mask every step.  One step length for all steps, set before
    them from the first gradient g alone: a probe step of 0.2 % of the parameter norm along -g (2 % overshoots on this untrained
    network) gives the curvature along g, the step is a quarter of that parabola's minimiser and at most the probe.  The loss after
    the steps is taken under the FIRST step's mask (call index rewound), so the comparison is not blurred by the mask-to-mask spread of
    the loss (~1 %)."""
    cfg, model = build('B', 'fp16x3', dropout=0.1)
    first, g, _ = _loss_and_grads('B', 'fp16x3', model=model)
    theta = {k: p.detach().clone() for k, p in model.named_parameters()}

    def move(lr, grads):
        with torch.no_grad():
            for k, p in model.named_parameters():
                p.sub_(lr * grads[k])
    pn = float(torch.sqrt(sum((p.double() ** 2).sum() for p in theta.values())))
    g2 = float(sum((v.double() ** 2).sum() for v in g.values()))
    eta0 = 0.002 * pn / np.sqrt(g2)
    move(eta0, g)
    model._train_calls = 0
    probe, _, _ = _loss_and_grads('B', 'fp16x3', model=model)                    # the first mask again
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(theta[k])
    curv = probe - first + eta0 * g2                                            # = eta0^2 g.H.g / 2 on a parabola
    lr = min(eta0, 0.25 * eta0 * eta0 * g2 / (2 * curv)) if curv > 0 else eta0
    vals, grads = [first], g
    for _ in range(4):                                                          # calls 2 .. 5: new masks
        move(lr, grads)
        loss, grads, _ = _loss_and_grads('B', 'fp16x3', model=model)
        vals.append(loss)
    move(lr, grads)
    model._train_calls = 0
    last, grads, _ = _loss_and_grads('B', 'fp16x3', model=model)
    print('SGD with dropout: probe %.5e at %.3e, lr %.3e; losses' % (probe, eta0, lr), ' '.join('%.5e' % v for v in vals), '-> %.5e under the first mask' % last)
    assert all(np.isfinite(vals)) and np.isfinite(last) and all(torch.isfinite(v).all() for v in grads.values())
    assert last < first


def test_trainer_adam_steps():
    """Trainer.train_step on ddpm3D_paired_SR3: the conditional loss is picked by class, clip + Adam + EMA move everything"""
    from conditional_score_diffusion_amd import train
    cfg, model = build('B', 'fp16x3', dropout=0.1, trainer_keys=True)
    tr = train.Trainer(cfg, model, tc.loss_sdes('B'))
    x, y = tc.loss_batch('B')
    batch = (y.to(dev()), x.to(dev()))
    p0 = {k: v.detach().clone() for k, v in model.named_parameters()}
    ema0 = tr.ema.shadow.detach().clone()
    torch.manual_seed(11)
    vals = [float(tr.train_step(batch)) for _ in range(3)]
    print('Trainer (Adam) losses', vals)
    assert all(np.isfinite(vals)) and model._train_calls == 3
    for k, v in model.named_parameters():
        assert torch.isfinite(v).all() and not torch.equal(v, p0[k]), k
    assert torch.isfinite(tr.ema.shadow).all() and not torch.equal(tr.ema.shadow, ema0)
    # the unconditional class gets the unconditional loss (a bare tensor batch)
    cfg, model = build('C', 'fp16x3', dropout=0.1, trainer_keys=True)
    tr = train.Trainer(cfg, model, tc.loss_sdes('C'))
    assert np.isfinite(float(tr.train_step(tc.loss_batch('C')[0].to(dev()))))


def _one_rank_worker(port, q):
    """two Adam steps of case B without a process group, then the same under a one-rank RCCL group"""
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        import sys
        import torch.distributed as dist
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path[:0] = [root, os.path.join(root, 'oracle'), os.path.join(root, 'tests')]
        from conditional_score_diffusion_amd import train
        torch.cuda.set_device(0)
        x, y = tc.loss_batch('B')
        batch = (y.to(dev()), x.to(dev()))

        def run():
            cfg, model = build('B', 'fp16x3', dropout=0.1, trainer_keys=True)
            tr = train.Trainer(cfg, model, tc.loss_sdes('B'), bucket_bytes=256 << 10)
            torch.manual_seed(5)
            vals = [float(tr.train_step(batch)) for _ in range(2)]
            torch.cuda.synchronize()
            return vals, tr.flat.data.detach().cpu().clone(), len(tr.sync.buckets)
        v0, p0, _ = run()
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev())
        v1, p1, nb = run()
        dist.barrier()
        dist.destroy_process_group()
        q.put((v0 == v1, bool(torch.equal(p0, p1)), bool(torch.isfinite(p1).all()), nb, None))
    except Exception:      # pragma: no cover
        import traceback
        q.put((False, False, False, 0, traceback.format_exc()))


def test_one_rank_rccl_gradsync_is_bit_identical():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    pr = ctx.Process(target=_one_rank_worker, args=(port, q))
    pr.start()
    same_loss, same_params, finite, nb, err = q.get(timeout=300)
    pr.join(timeout=60)
    assert err is None, err
    assert nb >= 2 and same_loss and same_params and finite
