"""-m gpu: gradient accumulation - csd_unet_backward_acc (the planned backward that ADDS to the caller's gradient buffers), the hold of
distributed.GradSync and train.Trainer with ``training.accumulate_grad_batches`` (Lightning's, run_lib.py:58,68,98).

Shapes: the tiny cases of oracle/cases.py and the 3-D case 'B' (6 x 10 x 4).  The library-level checks are bitwise: accumulate = 1 must
store fl32(R + V) with V the value the overwrite form stores.  The Trainer-level comparison of k micro-batches against one batch is a
comparison of two summation orders of one gradient and uses the project's rule for that (test_planned_graph_equals_operator_graph):
per tensor err <= tol * scale + 1e-7 * total / sqrt(numel), tol 2e-5 (fp32) / 2e-4 (fp16x3).
"""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import cases
import ddpm3d_train_cases as tc
from test_gpu_network import build, dev, sdes_for

pytestmark = pytest.mark.gpu

LIB_CASES = ['sr3_tiny', 'cmde_tiny', 'ncsnpp_fourier_skip', 'ncsnpp_residual_input', 'ncsnpp_nofir_skip']
FOURIER_CASES = ('ncsnpp_fourier_skip', 'ncsnpp_residual_input')      # embedding_type = 'fourier': the frozen Gaussian-Fourier W


# ---- library level ------------------------------------------------------------------------------------------------------------------------
def _ncsnpp_model(cfg, precision):
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg.model.csd_precision = precision
    cfg.model.dropout = 0.0
    model = mutils.create_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(cases.ncsnpp_params(shapes, 5))      # (the reference's init_scale = 0 would zero every upstream gradient)
    return model.to(dev())


def _lib_case(case, precision):
    """-> model, x, y (None: unconditional), labels, B"""
    if case in cases.CASES:
        cfg, B, x, y, u, tape = cases.grad_case(case)
        cfg, nc, p, model = build(cfg, precision)
        return model, x.to(dev()), y.to(dev()), torch.tensor([830., 21.5][:B], device=dev()), B
    cfg, B, x, labels = cases.ncsnpp_case(case)
    return _ncsnpp_model(cfg, precision), x.to(dev()), None, labels.to(dev()), B


def _magnitudes(shape, rs):
    """random signs, magnitudes log-uniform over 1e-8 ... 1e+2"""
    v = 10.0 ** rs.uniform(-8, 2, size=shape) * rs.choice([-1.0, 1.0], size=shape)
    return torch.from_numpy(v.astype(np.float32))


class _Graph:
    """one network handle driven through the C ABI: forward, then one of the backward entries into given gradient buffers"""

    def __init__(self, case, precision):
        from conditional_score_diffusion_amd._lib import lib, ptr
        self.lib, self.ptr = lib(), ptr
        self.model, self.x, self.y, self.labels, self.B = _lib_case(case, precision)
        m = self.model
        self.ps = m._train_params()
        self.table = (ctypes.c_void_p * len(self.ps))(*[q.data_ptr() for q in self.ps])
        self.ws = m._train_workspace(self.B)
        self.out = torch.empty(m._out_shape(self.B), device=dev())
        rs = np.random.RandomState(17)
        self.dout = torch.from_numpy(rs.standard_normal(tuple(self.out.shape)).astype(np.float32)).to(dev())
        self.call = 0

    def backward(self, grads, entry, accumulate=0, record_marks=1):
        """grads: the buffers the backward writes (their content is the accumulate form's `old`); -> d_x"""
        m, L, ptr = self.model, self.lib, self.ptr
        self.call += 1
        assert L.csd_unet_train_forward(m._h, self.table, ptr(self.ws), self.ws.numel(), ptr(self.x), ptr(self.y) if self.y is not None else None,
                                        ptr(self.labels), ptr(self.out), self.B, 0.0, 0, self.call, None) == 0, L.csd_last_error()
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


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', LIB_CASES)
def test_accumulating_backward_is_one_fp32_add_per_parameter(case, precision):
    """csd_unet_backward_acc: accumulate = 1 stores R + V for every parameter (V: what csd_unet_backward_ex stores, the sum ONE fp32
    addition), leaves the slot of the frozen Fourier W as it was, and does not change d_x; accumulate = 0 is csd_unet_backward_ex"""
    g = _Graph(case, precision)
    rs = np.random.RandomState(5)
    fill = lambda: [torch.full_like(q, float('nan')) for q in g.ps]      # noqa: E731  (an overwrite must not depend on the old content)
    V = fill()
    dx_v = g.backward(V, 'ex')
    assert all(bool(torch.isfinite(v).all()) for v in V) and bool(torch.isfinite(dx_v).all())
    assert sum(float(v.abs().sum()) for v in V) > 0
    V0 = fill()
    dx_0 = g.backward(V0, 'acc', accumulate=0)
    for name, a, b in zip(g.model._param_names, V0, V):
        assert torch.equal(a, b), name
    assert torch.equal(dx_0, dx_v)
    R = [_magnitudes(tuple(q.shape), rs).to(dev()) for q in g.ps]
    A = [r.clone() for r in R]
    dx_a = g.backward(A, 'acc', accumulate=1)
    frozen = 0
    for name, q, a, r, v in zip(g.model._param_names, g.ps, A, R, V):
        assert torch.equal(a, r + v), name
        if not q.requires_grad:                              # the fixed Gaussian-Fourier W: requires_grad = False in the reference
            frozen += 1
            assert torch.equal(a, r), name
    assert frozen == (1 if case in FOURIER_CASES else 0)
    assert torch.equal(dx_a, dx_v)
    Z = [torch.zeros_like(q) for q in g.ps]
    dx_z = g.backward(Z, 'acc', accumulate=1)
    for name, z, v in zip(g.model._param_names, Z, V):
        assert torch.equal(z, v), name
    assert torch.equal(dx_z, dx_v)


def test_record_marks_controls_the_events_and_the_epoch():
    g = _Graph('sr3_tiny', 'fp32')
    L, m = g.lib, g.model
    ev = L.csd_event_create()
    assert ev
    try:
        fm = (ctypes.c_int * 1)(0)
        evs = (ctypes.c_void_p * 1)(ev)
        assert L.csd_unet_backward_marks(m._h, fm, evs, 1) == 0
        e0 = int(L.csd_unet_backward_marks_epoch(m._h))
        G = [torch.zeros_like(q) for q in g.ps]
        g.backward(G, 'acc', accumulate=0, record_marks=0)
        assert int(L.csd_unet_backward_marks_epoch(m._h)) == e0
        g.backward(G, 'acc', accumulate=1, record_marks=0)
        assert int(L.csd_unet_backward_marks_epoch(m._h)) == e0
        g.backward(G, 'acc', accumulate=1, record_marks=1)
        assert int(L.csd_unet_backward_marks_epoch(m._h)) == e0 + 1
        assert L.csd_event_query(ctypes.c_void_p(ev)) == 1
        g.backward(G, 'ex')
        assert int(L.csd_unet_backward_marks_epoch(m._h)) == e0 + 2
        # arguments out of their domain are refused
        g.call += 1
        assert L.csd_unet_train_forward(m._h, g.table, g.ptr(g.ws), g.ws.numel(), g.ptr(g.x), g.ptr(g.y), g.ptr(g.labels), g.ptr(g.out), g.B,
                                        0.0, 0, g.call, None) == 0
        gt = (ctypes.c_void_p * len(G))(*[t.data_ptr() for t in G])
        assert L.csd_unet_backward_acc(m._h, g.table, gt, None, g.ptr(g.ws), g.ws.numel(), g.ptr(g.dout), g.B, g.call, 2, 1, None) != 0
        dx = torch.empty(m._x_shape(g.B), device=dev())
        assert L.csd_unet_backward_acc(m._h, g.table, None, g.ptr(dx), g.ptr(g.ws), g.ws.numel(), g.ptr(g.dout), g.B, g.call, 1, 1, None) != 0
        assert b'accumulate' in L.csd_last_error()
    finally:
        L.csd_unet_backward_marks(m._h, None, None, 0)
        L.csd_event_destroy(ctypes.c_void_p(ev))
    torch.cuda.synchronize()


# ---- Trainer --------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _taped(u, normals):
    """the loss's torch.rand / torch.randn_like replaced by a fixed tape (as test_gpu_training._hip_loss_and_grads)"""
    it = iter(normals)
    o_rand, o_like = torch.rand, torch.randn_like
    torch.rand = lambda *a, **k: u.clone()
    torch.randn_like = lambda t, **k: next(it).to(t.device)
    try:
        yield
    finally:
        torch.rand, torch.randn_like = o_rand, o_like


def _four(t, rs, lo=None, hi=None):
    """a batch of 4 from a case tensor of 2: the case's samples and perturbed copies of them"""
    p = t + torch.from_numpy((0.1 * rs.standard_normal(tuple(t.shape))).astype(np.float32))
    if lo is not None:
        p = p.clamp(lo, hi)
    return torch.cat([t, p])


U4 = torch.tensor([0.83, 0.21, 0.47, 0.64])
KINDS = ['sr3_planned', 'sr3_operators', 'ncsnpp_paired_skip', 'ddpm3d_B']


def _trainer_setup(kind, precision, k, dropout=0.0):
    """-> Trainer, batch of 4 (y, x), [normals of the loss's draws, batch 4]"""
    from conditional_score_diffusion_amd import sde_lib, train
    rs = np.random.RandomState(29)
    if kind.startswith('sr3'):
        cfg, B, x, y, u, tape = cases.grad_case('sr3_tiny')
        cfg.model.dropout = dropout
        cfg, nc, p, model = build(cfg, precision)
        model.train_executor = kind.split('_')[1]
        sde = sdes_for(cfg)
        x4, y4 = _four(x, rs, 0., 1.), _four(y, rs, 0., 1.)
        shapes = [tuple(x4.shape)]
    elif kind.startswith('ncsnpp'):
        from test_gpu_training import _ncsnpp_train_case
        cfg, xx = _ncsnpp_train_case()
        model = _ncsnpp_model(cfg, precision)
        cfg.model.dropout = dropout
        sde = {'x': sde_lib.cVESDE(0.01, 50., 1000), 'y': sde_lib.VESDE(0.01, 1.0, 1000)}
        xx4 = _four(xx, rs)
        x4, y4 = xx4[:, :3].contiguous(), xx4[:, 3:].contiguous()
        shapes = [tuple(y4.shape), tuple(x4.shape)]
    else:
        from test_gpu_ddpm3d_train import build as build3d
        cfg, model = build3d('B', precision, dropout=dropout, trainer_keys=True)
        sde = tc.loss_sdes('B')
        x, y = tc.loss_batch('B')
        x4, y4 = _four(x, rs, 0., 1.), _four(y, rs, 0., 1.)
        shapes = [tuple(x4.shape)]
    cfg.optim.grad_clip = -1.0
    if k is not None:
        cfg.training.accumulate_grad_batches = k
    tr = train.Trainer(cfg, model, sde)
    normals = [torch.from_numpy(rs.standard_normal(s).astype(np.float32)) for s in shapes]
    return tr, (y4.to(dev()), x4.to(dev())), normals


@functools.lru_cache(maxsize=None)
def _window(kind, precision, k):
    """one window of k micro-batches of 4 / k on the fixed batch and tape -> ({name: gradient after the window}, micro-batch losses)"""
    tr, (y4, x4), normals = _trainer_setup(kind, precision, k)
    n = 4 // k
    vals = []
    for j in range(k):
        assert tr.pending == j
        with _taped(U4[j * n:(j + 1) * n], [z[j * n:(j + 1) * n] for z in normals]):
            vals.append(float(tr.train_step((y4[j * n:(j + 1) * n].contiguous(), x4[j * n:(j + 1) * n].contiguous()))))
    torch.cuda.synchronize()
    assert tr.pending == 0 and tr.step == 1 and tr.optimizer.num_steps == 1
    assert tr.model._train_calls == k
    grads = {name: p.grad.detach().cpu().clone() for name, p in tr.model.named_parameters() if p.requires_grad}
    tr.close()
    return grads, vals


@pytest.mark.parametrize('k', [2, 4])
@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('fp16x3', 2e-4)])
@pytest.mark.parametrize('kind', KINDS)
def test_trainer_window_equals_the_whole_batch(kind, precision, tol, k):
    """k micro-batches of 4 / k through Trainer.train_step leave the gradient of the whole batch of 4 in the flat buffer; the
    micro-batch losses average to the whole batch's"""
    ref, ref_loss = _window(kind, precision, 1)
    got, vals = _window(kind, precision, k)
    assert set(got) == set(ref) and len(vals) == k
    worst, where = tc.grad_check(got, ref, tol, 1e-7)
    mean = float(np.mean(vals))
    print('%s %s k = %d: worst err / allowance %.3f at %s; loss %.8e vs %.8e' % (kind, precision, k, worst, where, mean, ref_loss[0]))
    assert worst <= 1.0, where
    assert abs(mean - ref_loss[0]) <= 1e-5 * abs(ref_loss[0])


def test_trainer_counts_optimizer_steps_and_flushes():
    tr, (y4, x4), _ = _trainer_setup('sr3_planned', 'fp32', 3, dropout=0.1)
    batch = (y4[:2].contiguous(), x4[:2].contiguous())
    torch.manual_seed(3)
    for _ in range(7):
        assert np.isfinite(float(tr.train_step(batch)))
    assert tr.optimizer.num_steps == tr.step == 2 and tr.pending == 1
    assert tr.model._train_calls == 7                        # the dropout streams advance per micro-batch
    with pytest.raises(RuntimeError, match='accumulation window'):
        tr.state_dict()
    assert tr.flush() is True
    assert tr.optimizer.num_steps == tr.step == 3 and tr.pending == 0
    assert tr.flush() is False and tr.step == 3
    assert tr.state_dict()['step'] == 3
    tr.close()
    with pytest.raises(ValueError, match='accumulate_grad_batches'):
        _trainer_setup('sr3_planned', 'fp32', 0)


def test_no_key_and_k_1_are_the_same_run():
    out = []
    for k in (None, 1):
        tr, (y4, x4), _ = _trainer_setup('sr3_planned', 'fp32', k, dropout=0.1)
        vals = []
        for i in range(3):
            torch.manual_seed(40 + i)
            vals.append(float(tr.train_step((y4, x4))))
        torch.cuda.synchronize()
        assert tr.step == 3 and tr.pending == 0
        out.append((vals, tr.flat.data.clone(), tr.ema.shadow.clone()))
        tr.close()
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


# ---- one-rank RCCL group: the event-driven bucket launches under accumulation ------------------------------------------------------------
def _one_rank_worker(port, q):
    """two optimizer steps of k = 2 on the planned sr3_tiny graph without a process group, then the same under a one-rank RCCL group"""
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        import sys
        import torch.distributed as dist
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path[:0] = [root, os.path.join(root, 'oracle'), os.path.join(root, 'tests')]
        from conditional_score_diffusion_amd import train
        torch.cuda.set_device(0)
        cfg0, B, x, y, u, tape = cases.grad_case('sr3_tiny')
        batch = (y.to(dev()), x.to(dev()))

        def run():
            cfg, B, x, y, u, tape = cases.grad_case('sr3_tiny')
            cfg.model.dropout = 0.1
            cfg.optim.warmup = 1
            cfg.training.accumulate_grad_batches = 2
            cfg, nc, p, model = build(cfg)
            tr = train.Trainer(cfg, model, sdes_for(cfg), bucket_bytes=256 << 10)
            seen, vals = [], []
            for i in range(4):
                torch.manual_seed(10 + i)
                vals.append(float(tr.train_step(batch)))
                seen.append(int(getattr(tr.sync, 'overlapped_launches', 0)))
            torch.cuda.synchronize()
            res = (vals, tr.flat.data.detach().cpu().clone(), len(tr.sync.buckets), seen, tr.step,
                   bool(getattr(model, '_last_backward_direct', False)))
            tr.close()
            return res
        v0, p0, _, seen0, _, _ = run()
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev())
        v1, p1, nb, seen1, steps, direct = run()
        dist.barrier()
        dist.destroy_process_group()
        q.put((dict(same_loss=v0 == v1, same_params=bool(torch.equal(p0, p1)), finite=bool(torch.isfinite(p1).all()), nb=nb, seen0=seen0,
                    seen1=seen1, steps=steps, direct=direct), None))
    except Exception:      # pragma: no cover
        import traceback
        q.put((None, traceback.format_exc()))


def test_one_rank_rccl_group_launches_each_bucket_once_per_window():
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
    import queue
    import time
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
    assert nb >= 3 and r['steps'] == 2 and r['direct'], r
    assert r['seen0'] == [0, 0, 0, 0], r
    # never during a held micro-batch; from its event, once per optimizer step: overlapped_launches == steps * len(buckets)
    assert r['seen1'] == [0, nb, nb, 2 * nb], r
    assert r['same_loss'] and r['same_params'] and r['finite'], r
