"""Gradient accumulation, host side (no GPU): GradSync.hold() - DDP's no_sync - on the autograd hooks, two gloo ranks on the CPU.

Bound of the gradient comparison (test_two_rank_hold_accumulates_the_global_batch_gloo).  Every entry of the gradient of the global
batch's mean loss is the sum g = sum_b g_b over the N = 24 samples.  One process adds them inside its matmuls; the two ranks add
k micro-batch sums into .grad and then 2 rank sums in the all-reduce: two orders of one N-term sum, each within (N - 1) eps of the exact
value relative to sum_b |g_b|, plus k + 2 further roundings for the window and the ranks (the 1 / 2 of scale_loss is exact, the 1 / 3
of k = 3 is one more rounding per term).  The per-sample chains themselves (three matmuls of fan-in <= 16, tanh) may be contracted
differently at batch 4 and batch 24: 24 eps more.  Allowance per entry: (2 (N + k + 2) + 24) eps sum_b |g_b|, eps = 2^-24, with
sum_b |g_b| from float64 per-sample gradients - 82 eps at k = 3.  A rank that reduced after every micro-batch, or that dropped or
double-counted one, misses it by orders of magnitude (its error is of the size of a micro-batch's gradient).
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_distributed_cpu import _by_value, _free_port, _from_value, _rendezvous_retry, _tiny_net

N_ROWS = 24


def _data():
    g = torch.Generator().manual_seed(7)
    return torch.rand(N_ROWS, 6, generator=g) * 2 - 1


def _hold_worker(rank, world, port, q, k):
    """(a worker that fails says so on the queue: the parent must never wait for a result that cannot come)"""
    try:
        _hold_rank(rank, world, port, q, k)
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc()))


def _collect(procs, q, world, patience=120.0):
    """one result per rank; a rank that reported an error or died without a result ends the wait at once (the other rank may sit in a
    collective its peer never joins: every worker is stopped before the failure is raised)"""
    import queue
    import time
    res, deadline = [], time.monotonic() + patience
    try:
        while len(res) < world:
            try:
                r = q.get(timeout=0.5)
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                if dead or time.monotonic() > deadline:
                    raise RuntimeError('worker exit codes %s, %d of %d results' % ([p.exitcode for p in procs], len(res), world))
                continue
            if r[1] is None:
                raise RuntimeError('rank %d failed:\n%s' % (r[0], r[2]))
            res.append(_from_value(r))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    return sorted(res, key=lambda t: t[0])


def _hold_rank(rank, world, port, q, k):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from conditional_score_diffusion_amd import distributed as D, optim
    calls = []
    real = dist.all_reduce

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    dist.all_reduce = counting                               # (GradSync reaches the collective through the module attribute)
    net = _tiny_net()
    flat = optim.FlatParams(net.parameters())
    sync = D.GradSync(flat, bucket_bytes=4 * 60)             # four buckets (the net has 435 parameters)
    data = _data()
    lo, hi = D.shard_bounds(N_ROWS, rank, world)
    per = (hi - lo) // k
    out = []
    for it in range(2):                                      # two windows: the hook bookkeeping resets
        seen = []
        flat.zero_grad()
        for j in range(k):
            sync.hold(j + 1 < k)
            loss = (net(data[lo + j * per:lo + (j + 1) * per] + it) ** 2).mean()
            (sync.scale_loss(loss) / k).backward()
            seen.append(len(calls))
        after_backward = len(calls)
        sync.finish()
        out.append((flat.grad.clone(), seen, after_backward, len(calls)))
        del calls[:]
    q.put(_by_value((rank, out, len(sync.buckets))))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('k', [2, 3])
@_rendezvous_retry
def test_two_rank_hold_accumulates_the_global_batch_gloo(k):
    """under hold no all_reduce is issued during the first k - 1 backwards; the k-th launches every bucket exactly once from the
    hooks; afterwards both ranks hold the gradient of the global batch"""
    from conditional_score_diffusion_amd import optim
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_hold_worker, args=(r, world, port, q, k)) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, world)
    nb = res[0][2]
    assert nb >= 3
    data = _data()
    eps = 2.0 ** -24
    for it in range(2):
        net = _tiny_net()
        flat = optim.FlatParams(net.parameters())
        (net(data + it) ** 2).mean().backward()              # one process, global batch
        net64 = _tiny_net().double()
        abs_sum = torch.zeros(flat.grad.numel(), dtype=torch.float64)
        for b in range(N_ROWS):                              # sum_b |g_b| in float64
            net64.zero_grad()
            ((net64(data[b:b + 1].double() + it) ** 2).sum() / (N_ROWS * 3)).backward()
            for p, o in zip(net64.parameters(), flat.offsets[:-1]):      # (the flat buffer's layout: its padding stays 0)
                abs_sum[int(o):int(o) + p.numel()] += p.grad.reshape(-1).abs()
        allow = (2 * (N_ROWS + k + 2) + 24) * eps * abs_sum
        for r in range(world):
            grad, seen, after_backward, total = res[r][1][it]
            assert seen[:k - 1] == [0] * (k - 1), seen      # held: nothing issued
            assert after_backward == nb and total == nb, (seen, after_backward, total, nb)      # the last backward: each bucket once
            err = (grad.double() - flat.grad.double()).abs()
            assert bool((err <= allow).all()), float((err / allow.clamp_min(1e-300)).max())
            assert torch.allclose(grad, flat.grad, rtol=1e-5, atol=1e-7)
        assert torch.equal(res[0][1][it][0], res[1][1][it][0])      # every rank holds the same reduced gradient


def test_hold_without_a_process_group_and_finish_while_held():
    from conditional_score_diffusion_amd import distributed as D, optim
    net = _tiny_net()
    flat = optim.FlatParams(net.parameters())
    sync = D.GradSync(flat, bucket_bytes=4 * 60)
    x = _data()
    flat.zero_grad()
    sync.hold(True)
    (net(x[:12]) ** 2).mean().backward()
    with pytest.raises(RuntimeError, match='held'):
        sync.finish()
    g1 = flat.grad.clone()
    sync.hold(False)
    (net(x[12:]) ** 2).mean().backward()                     # autograd accumulates into the flat buffer's views
    sync.finish()
    net2 = _tiny_net()
    flat2 = optim.FlatParams(net2.parameters())
    (net2(x[12:]) ** 2).mean().backward()
    assert torch.equal(flat.grad, g1 + flat2.grad)
