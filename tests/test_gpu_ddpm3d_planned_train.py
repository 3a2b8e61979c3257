"""-m gpu: the planned training graph of the 3-D DDPM networks (csrc/train_graph3d.h behind csd_unet_train_forward / csd_unet_backward*,
``DDPM3D(planned_train=True)``): gradients against float64, the input-gradient-only backward, dropout streams against the operator path,
the accumulating backward, determinism, the contract's refusals, the Trainer with accumulation and a one-rank RCCL group, the fused DSM
loss on volumes.

Cases: ddpm3d_cases A (ddpm3D_paired, 3 levels, 12 x 20 x 8: a 3 x 5 x 2 bottom level - odd extents, the W < 3 brick), B
(ddpm3D_paired_SR3, 6 x 10 x 4), C (ddpm3D).  References: the float64 restatements of ddpm3d_train_cases (net_ref, loss_ref), computed once.

Bounds (all set before the first run):
  output     1e-4, max|got - ref| / max|ref|: the network bound of tests/test_gpu_ddpm3d.py
  gradients  tc.grad_check(got, ref, tol, 1e-7), tol 2e-5 (fp32) / 2e-4 (fp16x3): per tensor err <= tol * scale + 1e-7 * total / sqrt(numel)
  eval output with vs without requires_grad 1e-5
  fused loss 1e-4 relative; its gradients grad_check(., 1e-3, 1e-6)        (test_training_loss_and_grads_vs_reference)
  accumulation, determinism, dropout-mask repeatability: bitwise

Measured on the MI355X (the operator path's figures of test_gpu_ddpm3d_train.py are beside them where the check is the same):

  training-mode output vs float64             A 1.5e-06 (fp32) 1.1e-06 (fp16x3)    B 1.4e-06 / 9.1e-07    C 1.2e-06 / 8.4e-07       (bound 1e-4)
  gradients, worst err / allowance            A 0.28 / 0.17    B 0.19 / 0.11    C 0.34 / 0.14       (operator path: 0.29 / 0.17, 0.19 / 0.11, 0.34 / 0.14)
  eval input gradient err / allowance         A 0.13 / 0.007   B 0.09 / 0.006   C 0.08 / 0.006      (operator path: 0.13 / 0.007, 0.08 / 0.006, 0.09 / 0.007)
  eval output with vs without requires_grad   fp32 0 (bitwise)    fp16x3 6.7e-07 (A), 5.0e-07 (B), 5.3e-07 (C)    (bound 1e-5)
  dropout 0.1, planned vs operator path       0 (bitwise) at calls 1 and 2, both precisions; call 2 vs call 1: 0.33
  Trainer, k = 2 vs the whole batch (B)       worst err / allowance 0.005 (fp32), 0.000 (fp16x3); mean loss 26.0251389 vs 26.0251389
  fused loss, relative to float64             A 3.4e-08 / 3.4e-08    B 1.5e-07 / 1.2e-08      (bound 1e-4)
  fused loss gradients, err / allowance       A 0.010 / 0.031        B 0.009 / 0.043
  dropout 0.1 gradients, planned vs operator  worst err / allowance 0.13 (fp32), 0.11 (fp16x3), both at all_modules.3.Dense_0.weight
  flipped / transposed pack vs the weight copy  head GroupNorm and last GroupNorm_1 gradients bitwise the operator path's (A, B; both precisions)
  accumulation, determinism, contract errors, one-rank RCCL: exact checks; the file runs in 19 s
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import ddpm3d_cases as dc
import ddpm3d_train_cases as tc

pytestmark = pytest.mark.gpu

OUT_BOUND = 1e-4
PRECISIONS = [('fp32', 2e-5), ('fp16x3', 2e-4)]


def dev():
    return torch.device('cuda:0')


def build(case, precision, dropout=0.0, trainer_keys=False, planned_train=True):
    from conditional_score_diffusion_amd.config_dict import ConfigDict
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = dc.make_config(case, precision=precision)
    cfg.model.dropout = dropout
    cfg.model.csd_planned_train = planned_train
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


def out64(case):
    return dc.forward64(dc.params(case), case, *dc.case_inputs(case))


# ---- 1, 2: gradients against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision,tol', PRECISIONS)
@pytest.mark.parametrize('case', sorted(dc.CASES))
def test_gradients_vs_float64(case, precision, tol):
    """training mode, dropout 0, loss = sum(out * g): the output, every parameter gradient and d_x from ONE csd_unet_backward_acc"""
    cfg, model = build(case, precision)
    assert model.planned_train and model.train_executor == 'planned' and model._h is not None
    x, y, labels = gpu_inputs(case)
    val, rg, rdx = tc.net_ref(case)
    model.train()
    xg = x.clone().requires_grad_(True)
    out = dc.call(model, case, xg, y, labels)
    assert out.requires_grad and model._train_calls == 1
    e_out = tc.rel(out, out64(case))
    (out * tc.net_g(case).to(dev())).sum().backward()
    got = {k: v.grad for k, v in model.named_parameters()}
    got['<x>'] = xg.grad
    ref = dict(rg)
    ref['<x>'] = rdx
    assert set(got) == set(ref)
    worst, where = tc.grad_check(got, ref, tol, 1e-7)
    print('planned 3-D %s %s: output %.3e; worst gradient err / allowance %.3f at %s' % (case, precision, e_out, worst, where))
    assert e_out < OUT_BOUND
    assert worst <= 1.0, where


@pytest.mark.parametrize('precision,tol', PRECISIONS)
@pytest.mark.parametrize('case', sorted(dc.CASES))
def test_input_gradient_only(case, precision, tol):
    """eval mode with x.requires_grad: csd_unet_backward_ex with grads = NULL; the parameters take nothing"""
    cfg, model = build(case, precision)
    x, y, labels = gpu_inputs(case)
    model.eval()
    xg = x.clone().requires_grad_(True)
    out_g = dc.call(model, case, xg, y, labels)
    dx, = torch.autograd.grad(out_g.sum(), xg)
    assert all(p.grad is None for p in model.parameters())
    _, _, rdx = tc.net_ref(case, 'sum')
    worst, _ = tc.grad_check({'<x>': dx}, {'<x>': rdx}, tol, 1e-7)
    with torch.no_grad():
        out_i = dc.call(model, case, x, y, labels)
    e, e64 = tc.rel(out_g, out_i), tc.rel(out_g, out64(case))
    print('planned 3-D %s %s eval: input gradient err / allowance %.3f; output with vs without requires_grad %.3e, vs float64 %.3e'
          % (case, precision, worst, e, e64))
    assert worst <= 1.0
    assert e < 1e-5 and e64 < OUT_BOUND


# ---- 3: dropout ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_dropout_masks_are_the_operator_paths(precision):
    """p = 0.1, the same dropout_seed and call index: the planned graph and the operator path (the reference here) agree within the
    output bound, which two different masks miss by orders of magnitude (checked: the next call's output does); the same call again
    is bitwise the same"""
    case = 'A'
    _, planned = build(case, precision, dropout=0.1)
    _, oper = build(case, precision, dropout=0.1, planned_train=False)
    assert getattr(oper, 'train_executor', 'operators') == 'operators' and oper._h is None
    x, y, labels = gpu_inputs(case)
    planned.train(), oper.train()
    a1 = dc.call(planned, case, x, y, labels).detach()
    b1 = dc.call(oper, case, x, y, labels).detach()
    assert planned._train_calls == oper._train_calls == 1 and planned.dropout_seed == oper.dropout_seed == 42
    a2 = dc.call(planned, case, x, y, labels).detach()
    b2 = dc.call(oper, case, x, y, labels).detach()
    e1, e2, other = tc.rel(a1, b1), tc.rel(a2, b2), tc.rel(a2, a1)
    print('dropout %s: planned vs operator path %.3e (call 1), %.3e (call 2); call 2 vs call 1 %.3e' % (precision, e1, e2, other))
    assert e1 < OUT_BOUND and e2 < OUT_BOUND
    assert other > 100 * OUT_BOUND                             # another call index: another mask
    planned._train_calls = 0
    assert torch.equal(dc.call(planned, case, x, y, labels).detach(), a1)
    planned.eval()
    with torch.no_grad():
        assert tc.rel(dc.call(planned, case, x, y, labels), out64(case)) < OUT_BOUND      # no dropout in eval mode


def _train_grads(model, case, x, y, labels):
    model.zero_grad()
    xg = x.clone().requires_grad_(True)
    (dc.call(model, case, xg, y, labels) * tc.net_g(case).to(dev())).sum().backward()
    got = {k: v.grad.detach().clone() for k, v in model.named_parameters()}
    got['<x>'] = xg.grad.detach().clone()
    return got


@pytest.mark.parametrize('precision,tol', PRECISIONS)
def test_gradients_through_the_dropout_masks_are_the_operator_paths(precision, tol):
    """p = 0.1, the same seed and call: every gradient of the planned graph (the masks applied in its backward) against the operator
    path's, the reference here as in the forward check, under the gradient rule (two summation groupings of the same kernels' values)"""
    case = 'A'
    _, planned = build(case, precision, dropout=0.1)
    _, oper = build(case, precision, dropout=0.1, planned_train=False)
    x, y, labels = gpu_inputs(case)
    planned.train(), oper.train()
    got, ref = _train_grads(planned, case, x, y, labels), _train_grads(oper, case, x, y, labels)
    assert planned._train_calls == oper._train_calls == 1
    worst, where = tc.grad_check(got, {k: v.cpu() for k, v in ref.items()}, tol, 1e-7)
    print('dropout %s gradients, planned vs operator path: worst err / allowance %.4f at %s' % (precision, worst, where))
    assert worst <= 1.0, where


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', ['A', 'B'])
def test_flipped_transposed_pack_is_bitwise_the_weight_copys(case, precision):
    """the data gradient packs w[ci][co][26 - tap] from the forward layer's weight where the operator path packs a copy of
    weight.flip(2, 3, 4).transpose(0, 1): the same values.  Seen where nothing else differs between the two paths: the head
    GroupNorm's gradients (behind the head's data gradient: the direct kernel's pack, 2 output channels in A, 1 in B) and the last
    residual block's GroupNorm_1 gradients (behind Conv_1's data gradient as well: the MFMA pack in fp16x3) have one consumer each, the
    same forward bits, the same GroupNorm backward kernel and a batch sum of B = 2 rows, which has one order"""
    _, planned = build(case, precision)
    _, oper = build(case, precision, planned_train=False)
    x, y, labels = gpu_inputs(case)
    planned.train(), oper.train()
    got, ref = _train_grads(planned, case, x, y, labels), _train_grads(oper, case, x, y, labels)
    names = list(dict(planned.named_parameters()))
    head_gn = [k for k in names if k.count('.') == 2][-4:-2]                     # all_modules.{n-2}.weight / .bias
    last_res = [k for k in names if 'GroupNorm_1' in k][-2:]
    assert len(head_gn) == 2 and len(last_res) == 2 and all(k.endswith(('weight', 'bias')) for k in head_gn)
    for k in head_gn + last_res:
        assert got[k].abs().sum() > 0 and torch.equal(got[k], ref[k]), k


# ---- the C ABI driven directly ---------------------------------------------------------------------------------------------------------------
class _Graph:
    """one arch-2 handle through csd_unet_train_forward and one of the backward entries, into given buffers"""

    def __init__(self, case, precision, sample=None, ws_fill=None):
        from conditional_score_diffusion_amd._lib import lib, ptr
        self.lib, self.ptr = lib(), ptr
        _, self.model = build(case, precision)
        self.x, self.y, self.labels = gpu_inputs(case)
        if sample is not None:
            sl = slice(sample, sample + 1)
            self.x, self.labels = self.x[sl].contiguous(), self.labels[sl].contiguous()
            self.y = None if self.y is None else self.y[sl].contiguous()
        m = self.model
        self.B = self.x.shape[0]
        self.ps = m._train_params()
        self.table = (ctypes.c_void_p * len(self.ps))(*[q.data_ptr() for q in self.ps])
        self.ws = m._train_workspace(self.B)
        if ws_fill is not None:
            self.ws.view(torch.float32).fill_(ws_fill)
        self.out = torch.full(m._out_shape(self.B), float('nan'), device=dev())
        g = tc.net_g(case).to(dev())
        self.dout = (g if sample is None else g[sample:sample + 1]).contiguous()
        self.call = 0

    def forward(self):
        m, L, ptr = self.model, self.lib, self.ptr
        self.call += 1
        return L.csd_unet_train_forward(m._h, self.table, ptr(self.ws), self.ws.numel(), ptr(self.x), ptr(self.y) if self.y is not None else None,
                                        ptr(self.labels), ptr(self.out), self.B, 0.0, 0, self.call, None)

    def backward(self, grads, entry='ex', accumulate=0, record_marks=1):
        m, L, ptr = self.model, self.lib, self.ptr
        assert self.forward() == 0, L.csd_last_error()
        gtable = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        dx = torch.full(m._x_shape(self.B), float('nan'), device=dev())
        if entry == 'ex':
            rc = L.csd_unet_backward_ex(m._h, self.table, gtable, ptr(dx), ptr(self.ws), self.ws.numel(), ptr(self.dout), self.B, self.call, None)
        else:
            rc = L.csd_unet_backward_acc(m._h, self.table, gtable, ptr(dx), ptr(self.ws), self.ws.numel(), ptr(self.dout), self.B, self.call,
                                         accumulate, record_marks, None)
        assert rc == 0, L.csd_last_error()
        torch.cuda.synchronize()
        return dx


def _magnitudes(shape, rs):
    """random signs, magnitudes log-uniform over 1e-8 ... 1e+2"""
    v = 10.0 ** rs.uniform(-8, 2, size=shape) * rs.choice([-1.0, 1.0], size=shape)
    return torch.from_numpy(v.astype(np.float32))


# ---- 4: accumulation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', ['A', 'C'])
def test_accumulating_backward_is_one_fp32_add_per_parameter(case, precision):
    """the 3-D twin of test_gpu_grad_accumulation's: accumulate = 1 stores R + V for every parameter (V: what csd_unet_backward_ex
    stores, the sum ONE fp32 addition) and does not change d_x; accumulate = 0 is csd_unet_backward_ex"""
    g = _Graph(case, precision)
    rs = np.random.RandomState(5)
    fill = lambda: [torch.full_like(q, float('nan')) for q in g.ps]      # noqa: E731  (an overwrite must not depend on the old content)
    V = fill()
    dx_v = g.backward(V, 'ex')
    assert all(bool(torch.isfinite(v).all()) for v in V) and bool(torch.isfinite(dx_v).all())
    assert all(float(v.abs().sum()) > 0 for v in V)
    V0 = fill()
    dx_0 = g.backward(V0, 'acc', accumulate=0)
    for name, a, b in zip(g.model._param_names, V0, V):
        assert torch.equal(a, b), name
    assert torch.equal(dx_0, dx_v)
    R = [_magnitudes(tuple(q.shape), rs).to(dev()) for q in g.ps]
    A = [r.clone() for r in R]
    dx_a = g.backward(A, 'acc', accumulate=1)
    for name, a, r, v in zip(g.model._param_names, A, R, V):
        assert torch.equal(a, r + v), name
    assert torch.equal(dx_a, dx_v)
    Z = [torch.zeros_like(q) for q in g.ps]
    dx_z = g.backward(Z, 'acc', accumulate=1)
    for name, z, v in zip(g.model._param_names, Z, V):
        assert torch.equal(z, v), name
    assert torch.equal(dx_z, dx_v)


# ---- 5: determinism --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_repeatable_batch_independent_and_blind_to_buffer_contents(precision):
    case = 'A'
    g = _Graph(case, precision, ws_fill=0.0)
    G1 = [torch.zeros_like(q) for q in g.ps]
    dx1 = g.backward(G1)
    out1 = g.out.clone()
    assert bool(torch.isfinite(out1).all())
    # again, into NaN-filled gradient buffers and a NaN-filled workspace
    g.ws.view(torch.float32).fill_(float('nan'))
    g.out.fill_(float('nan'))
    G2 = [torch.full_like(q, float('nan')) for q in g.ps]
    dx2 = g.backward(G2)
    assert torch.equal(g.out, out1) and torch.equal(dx2, dx1)
    for name, a, b in zip(g.model._param_names, G1, G2):
        assert torch.equal(a, b), name
    # sample b alone is sample b inside the batch
    for b in range(g.B):
        s = _Graph(case, precision, sample=b)
        dxs = s.backward([torch.zeros_like(q) for q in s.ps])
        assert torch.equal(s.out[0], out1[b]) and torch.equal(dxs[0], dx1[b]), b


# ---- 6: contract errors ----------------------------------------------------------------------------------------------------------------------
def test_contract_errors():
    """refused before any launch: the output and gradient buffers keep their NaN fill"""
    g = _Graph('C', 'fp16x3')
    L, m, ptr = g.lib, g.model, g.ptr
    G = [torch.full_like(q, float('nan')) for q in g.ps]
    gt = (ctypes.c_void_p * len(G))(*[t.data_ptr() for t in G])
    dx = torch.full(m._x_shape(g.B), float('nan'), device=dev())
    need = L.csd_unet_train_workspace_bytes(m._h, g.B, 0.0)
    assert need > 0 and L.csd_unet_train_workspace_bytes(m._h, g.B, 0.1) > need      # (the masks)
    # a backward with no forward
    assert L.csd_unet_backward_ex(m._h, g.table, gt, ptr(dx), ptr(g.ws), g.ws.numel(), ptr(g.dout), g.B, 1, None) == -3      # CSD_ERR_STATE
    # a short workspace
    g.call += 1
    assert L.csd_unet_train_forward(m._h, g.table, ptr(g.ws), need - 256, ptr(g.x), None, ptr(g.labels), ptr(g.out), g.B, 0.0, 0, g.call,
                                    None) == -5                                                                             # CSD_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(g.out).all())
    assert g.forward() == 0, L.csd_last_error()
    # the wrong call index, no gradient requested, a short workspace
    assert L.csd_unet_backward_ex(m._h, g.table, gt, ptr(dx), ptr(g.ws), g.ws.numel(), ptr(g.dout), g.B, g.call + 1, None) == -3
    assert L.csd_unet_backward_ex(m._h, g.table, None, None, ptr(g.ws), g.ws.numel(), ptr(g.dout), g.B, g.call, None) == -1
    assert L.csd_unet_backward_ex(m._h, g.table, gt, ptr(dx), ptr(g.ws), need - 256, ptr(g.dout), g.B, g.call, None) == -5
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in G) and bool(torch.isnan(dx).all())
    # the forward is still there: the right call succeeds, once
    assert L.csd_unet_backward_ex(m._h, g.table, gt, ptr(dx), ptr(g.ws), g.ws.numel(), ptr(g.dout), g.B, g.call, None) == 0, L.csd_last_error()
    assert L.csd_unet_backward_ex(m._h, g.table, gt, ptr(dx), ptr(g.ws), g.ws.numel(), ptr(g.dout), g.B, g.call, None) == -3
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in G) and bool(torch.isfinite(dx).all())
    # Python: another volume than the configured one
    m.train()
    with pytest.raises(ValueError, match='configured volume'):
        m(torch.zeros(1, 1, 4, 10, 4, device=dev()), g.labels[:1])
    m.eval()
    with pytest.raises(ValueError, match='configured volume'):
        m(torch.zeros(1, 1, 4, 10, 4, device=dev(), requires_grad=True), g.labels[:1])


# ---- 7: Trainer ------------------------------------------------------------------------------------------------------------------------------
def _trainer_window(precision, k):
    """one window of k micro-batches of 4 / k of case B on a fixed tape -> ({name: gradient}, losses); as test_gpu_grad_accumulation._window"""
    from conditional_score_diffusion_amd import train
    from test_gpu_grad_accumulation import U4, _four, _taped
    rs = np.random.RandomState(29)
    cfg, model = build('B', precision, trainer_keys=True)
    x, y = tc.loss_batch('B')
    x4, y4 = _four(x, rs, 0., 1.).to(dev()), _four(y, rs, 0., 1.).to(dev())
    cfg.optim.grad_clip = -1.0
    cfg.training.accumulate_grad_batches = k
    tr = train.Trainer(cfg, model, tc.loss_sdes('B'))
    assert model.grad_sink is True
    normals = [torch.from_numpy(rs.standard_normal(tuple(x4.shape)).astype(np.float32))]
    n, vals = 4 // k, []
    for j in range(k):
        assert tr.pending == j
        with _taped(U4[j * n:(j + 1) * n], [z[j * n:(j + 1) * n] for z in normals]):
            vals.append(float(tr.train_step((y4[j * n:(j + 1) * n].contiguous(), x4[j * n:(j + 1) * n].contiguous()))))
        assert model._last_backward_direct                    # the kernels wrote (or added to) the .grad views themselves
    torch.cuda.synchronize()
    assert tr.pending == 0 and tr.step == 1 and model._train_calls == k
    grads = {name: p.grad.detach().cpu().clone() for name, p in model.named_parameters()}
    tr.close()
    return grads, vals


@pytest.mark.parametrize('precision,tol', PRECISIONS)
def test_trainer_window_equals_the_whole_batch(precision, tol):
    ref, ref_loss = _trainer_window(precision, 1)
    got, vals = _trainer_window(precision, 2)
    worst, where = tc.grad_check(got, ref, tol, 1e-7)
    mean = float(np.mean(vals))
    print('planned 3-D B %s k = 2: worst err / allowance %.3f at %s; loss %.8e vs %.8e' % (precision, worst, where, mean, ref_loss[0]))
    assert worst <= 1.0, where
    assert abs(mean - ref_loss[0]) <= 1e-5 * abs(ref_loss[0])


def _one_rank_worker(port, q):
    """two optimizer steps of k = 2 on the planned 3-D graph without a process group, then the same under a one-rank RCCL group"""
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        import sys
        import torch.distributed as dist
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path[:0] = [root, os.path.join(root, 'oracle'), os.path.join(root, 'tests')]
        from conditional_score_diffusion_amd import train
        from conditional_score_diffusion_amd._lib import lib
        torch.cuda.set_device(0)
        x, y = tc.loss_batch('B')
        batch = (y.to(dev()), x.to(dev()))

        def run():
            cfg, model = build('B', 'fp16x3', dropout=0.1, trainer_keys=True)
            cfg.optim.warmup = 1
            cfg.training.accumulate_grad_batches = 2
            tr = train.Trainer(cfg, model, tc.loss_sdes('B'), bucket_bytes=256 << 10)
            seen, vals, epochs = [], [], []
            for i in range(4):
                torch.manual_seed(10 + i)
                vals.append(float(tr.train_step(batch)))
                seen.append(int(getattr(tr.sync, 'overlapped_launches', 0)))
                epochs.append(int(lib().csd_unet_backward_marks_epoch(model._h)))
            torch.cuda.synchronize()
            res = (vals, tr.flat.data.detach().cpu().clone(), len(tr.sync.buckets), seen, tr.step,
                   bool(getattr(model, '_last_backward_direct', False)), epochs)
            tr.close()
            return res
        v0, p0, _, seen0, _, _, _ = run()
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev())
        v1, p1, nb, seen1, steps, direct, epochs = run()
        dist.barrier()
        dist.destroy_process_group()
        q.put((dict(same_loss=v0 == v1, same_params=bool(torch.equal(p0, p1)), finite=bool(torch.isfinite(p1).all()), nb=nb, seen0=seen0,
                    seen1=seen1, steps=steps, direct=direct, epochs=epochs), None))
    except Exception:      # pragma: no cover
        import traceback
        q.put((None, traceback.format_exc()))


def test_one_rank_rccl_group_launches_each_bucket_once_per_window():
    import queue
    import socket
    import time
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    pr = ctx.Process(target=_one_rank_worker, args=(port, q))
    pr.start()
    deadline = time.monotonic() + 300
    while True:                                              # (a worker that died without a result ends the wait at once)
        try:
            r, err = q.get(timeout=0.5)
            break
        except queue.Empty:
            assert pr.exitcode in (None, 0) and time.monotonic() < deadline, 'worker exit code %s without a result' % pr.exitcode
    pr.join(timeout=60)
    assert err is None, err
    nb = r['nb']
    assert nb >= 2 and r['steps'] == 2 and r['direct'], r
    assert r['seen0'] == [0, 0, 0, 0], r
    assert r['seen1'] == [0, nb, nb, 2 * nb], r              # never during a held micro-batch; once per optimizer step
    e = r['epochs']
    assert [e[1] - e[0], e[2] - e[1], e[3] - e[2]] == [1, 0, 1], r      # the marks epoch advances once per window
    assert r['same_loss'] and r['same_params'] and r['finite'], r


# ---- 8: the fused DSM loss on volumes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', ['A', 'B'])
def test_fused_loss_vs_float64(case, precision):
    """csd_dsm_perturb -> the planned 3-D network -> csd_dsm_residual with loss_tape as the explicit noise: the two-SDE pair (A), SR3 (B)"""
    from conditional_score_diffusion_amd import losses
    cfg, model = build(case, precision)
    x, y = tc.loss_batch(case)
    u, tape = tc.loss_tape(case)
    fn = losses.get_general_sde_loss_fn(tc.loss_sdes(case), True, conditional=True, reduce_mean=True, continuous=True,
                                        likelihood_weighting=True, fused=True)
    model.zero_grad()
    loss = fn(model, (y.to(dev()), x.to(dev())), noise=[z.to(dev()) for z in tape], t=u * (1 - 1e-5) + 1e-5)
    assert model.training and loss.requires_grad and model._train_calls == 1
    loss.backward()
    grads = {k: v.grad for k, v in model.named_parameters()}
    r_loss, r_grads = tc.loss_ref(case)
    worst, where = tc.grad_check(grads, r_grads, 1e-3, 1e-6)
    val = float(loss.detach())
    print('fused loss %s %s: %.8e (float64 %.8e, rel %.2e); worst gradient err / allowance %.4f at %s' %
          (case, precision, val, r_loss, abs(val - r_loss) / abs(r_loss), worst, where))
    assert abs(val - r_loss) <= 1e-4 * abs(r_loss)
    assert worst <= 1.0, where
