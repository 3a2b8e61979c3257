"""Side bench (not the headline metric): training steps/s of BASELINE configs[3]-shaped work - VS-CMDE edges2shoes 64x64,
`ddpm_paired` nf=128, ch_mult (1,1,2,2), attention at 16/8, dropout 0.1, global batch 50 (configs/ve/inverse_problems/
image_to_image_translation/edges2shoes_ours_DV.py) - one full step = loss forward + HIP backward + bucketed gradient
all-reduce + fused clip/Adam/EMA.  One process per GPU (launch with torch.distributed.run for N > 1; the batch is sharded).

    python tools/bench_train.py [--steps 10 --warmup 3 --batch 50 --precision fp32]

`--accumulate K` (one process): one optimizer step of K micro-batches of batch / K (training.accumulate_grad_batches = K) timed three
ways - the accumulating planned backward (csd_unet_backward_acc adds to the flat gradient), the same with direct mode off (the backward
fills a temporary buffer and autograd adds it per parameter: the only route before csd_unet_backward_acc), and one step at K = 1 on the
whole batch - written under a new key of profiles/train_accumulate.json (`--out`).

`--fused-loss` (one process): the default loss route against `training.csd_fused_loss` in alternating windows of --steps steps on one
device, at the config's batch of 50 and at 7 (one rank's shard of 50 over 8), with the default route's own window-to-window spread as
the yardstick; the time of csd_dsm_perturb + csd_dsm_residual alone at those shapes (the loss path's share of a step); and both noise
forms of the two kernels (normals made in registers twice / one csd_randn fill read twice) at the SR3-160 shape, B = 64 - written to
profiles/train_fused_loss.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conditional_score_diffusion_amd import sde_lib, train  # noqa: E402
from conditional_score_diffusion_amd.config_dict import ConfigDict  # noqa: E402
from conditional_score_diffusion_amd.models import utils as mutils  # noqa: E402
import conditional_score_diffusion_amd.models.ddpm  # noqa: E402,F401

FWD_GFLOP_PER_IMAGE = 30.2          # SURVEY.md 8(d), cfg4 forward; a training step is ~3x (forward + dX + dW)


def make_config(precision):
    S = 64
    c = ConfigDict()
    c.training = ConfigDict(continuous=True, sde='vesde', likelihood_weighting=True, reduce_mean=True, batch_size=50)
    c.data = ConfigDict(image_size=S, effective_image_size=S, centered=False, shape_x=[3, S, S], shape_y=[3, S, S], num_channels=6)
    smax = float(np.sqrt(3 * S * S))
    c.model = ConfigDict(name='ddpm_paired', nf=128, ch_mult=(1, 1, 2, 2), num_res_blocks=2, attn_resolutions=(16, 8),
                         dropout=0.1, resamp_with_conv=True, conditional=True, nonlinearity='swish', num_scales=1000,
                         sigma_min_x=5e-3, sigma_max_x=smax, sigma_min_y=5e-3, sigma_max_y=smax, input_channels=6,
                         output_channels=6, embedding_type='positional', scale_by_sigma=True, ema_rate=0.999,
                         reach_target_steps=300000, sigma_max_y_target=1.0, sigma_min_y_target=5e-3,     # VS-CMDE schedule (edges2shoes_ours_DV.py:101-107)
                         csd_precision=precision)
    c.optim = ConfigDict(weight_decay=0, optimizer='Adam', lr=2e-4, beta1=0.9, eps=1e-8, warmup=2500, grad_clip=1)
    c.seed = 42
    return c


def make_ncsnpp_config(precision):
    """the same work shape on the architecture north_star names: ncsnpp_paired (BigGAN blocks, FIR resampling, input / output skips,
    skip_rescale) with the configs[3] hyper-parameters (64 x 64, nf = 128, ch_mult (1, 1, 2, 2), attention at 16, dropout 0.1)"""
    c = make_config(precision)
    m = c.model
    m.name = 'ncsnpp_paired'
    m.attn_resolutions = (16,)
    for k, v in dict(fir=True, fir_kernel=[1, 3, 3, 1], skip_rescale=True, resblock_type='biggan', progressive='output_skip',
                     progressive_input='input_skip', progressive_combine='sum', attention_type='ddpm', init_scale=0.,
                     fourier_scale=16, conv_size=3, sigma_min=5e-3, sigma_max=m.sigma_max_x).items():
        setattr(m, k, v)
    return c


def bench_accumulate(a, dev):
    """-> the record of one `--accumulate K` run (single process)"""
    K = a.accumulate
    if a.batch % K:
        sys.exit('--accumulate %d does not divide --batch %d' % (K, a.batch))

    def timed(k, direct):
        cfg = make_config(a.precision) if a.model == 'ddpm_paired' else make_ncsnpp_config(a.precision)
        if k > 1:
            cfg.training.accumulate_grad_batches = k
        torch.manual_seed(0)
        model = mutils.create_model(cfg).to(dev)
        m = cfg.model
        sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
        tr = train.Trainer(cfg, model, sde)
        if not direct:
            model.grad_sink = False           # the planned backward hands autograd one gradient per parameter to accumulate
        B = a.batch // k
        g = torch.Generator().manual_seed(1)
        batch = (torch.rand(B, 3, 64, 64, generator=g).to(dev), torch.rand(B, 3, 64, 64, generator=g).to(dev))
        for _ in range(a.warmup * k):
            loss = tr.train_step(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps * k):
            loss = tr.train_step(batch)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / a.steps
        assert tr.step == a.warmup + a.steps and tr.pending == 0
        rec = {'ms_per_optimizer_step': ms, 'micro_batches': k, 'micro_batch': B, 'loss': float(loss),
               'peak_memory_MiB': torch.cuda.max_memory_allocated(dev) / 2.0 ** 20}
        n_tensors = len(tr.flat.params)
        tr.close()
        del tr, model
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        return rec, n_tensors

    acc, n_tensors = timed(K, True)
    auto, _ = timed(K, False)
    full, _ = timed(1, True)
    return {'model': a.model, 'precision': a.precision, 'batch': a.batch, 'accumulate': K, 'steps': a.steps, 'warmup': a.warmup,
            'accumulating_backward': acc, 'autograd_accumulation': auto, 'full_batch_k1': full,
            # launches on top of the overwrite form, per micro-batch: the accumulating backward adds none (each final writer reads the
            # old value itself; the q | k | v bias slices run as 3 one-row kernels per attention block in place of 3 device copies);
            # autograd's route adds one elementwise add per parameter tensor and one allocation of the whole gradient
            'extra_launches_per_micro_batch': {'accumulating_backward': 0, 'autograd_accumulation': n_tensors},
            'device': torch.cuda.get_device_name(dev), 'data': 'synthetic'}


def _event_ms(fn, reps, warmup, dev):
    """mean device time of fn() in ms between two events, after warm-up"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / reps


def _loss_kernels_ms(B, shapes, dev, form, reps=50):
    """csd_dsm_perturb per tensor + one csd_dsm_residual over them (with d_out), noise `form`: 'registers' | 'fill'"""
    from conditional_score_diffusion_amd import ops
    g = torch.Generator().manual_seed(2)
    xs = [torch.rand((B,) + s, generator=g).to(dev) for s in shapes]
    coef = [(torch.rand(B, generator=g) + 0.5).to(dev) for _ in range(3)]
    per = [int(np.prod(s)) for s in shapes]
    net = torch.randn(B, sum(per), generator=g).to(dev)

    def run():
        z = [ops.randn(x.shape, 7, (1 << 63) + k, dev) if form == 'fill' else None for k, x in enumerate(xs)]
        for k, x in enumerate(xs):
            ops.dsm_perturb(x, coef[0], None, z[k], 7, (1 << 63) + k)
        segs, off = [], 0
        for k, n in enumerate(per):
            segs.append({'offset': off, 'length': n, 'a': coef[0], 'b': coef[1], 'w': coef[2], 'z': z[k], 'stream_id': (1 << 63) + k})
            off += n
        ops.dsm_residual(net, segs, 7)

    return _event_ms(run, reps, 5, dev)


def bench_fused_loss(a, dev, windows=3):
    """-> the record of one `--fused-loss` run (single process)"""
    rec = {'model': a.model, 'precision': a.precision, 'steps_per_window': a.steps, 'warmup': a.warmup, 'windows': windows,
           'device': torch.cuda.get_device_name(dev), 'data': 'synthetic', 'routes': {}}
    for B in (a.batch, 7):
        trainers = {}
        for fused in (False, True):
            cfg = make_config(a.precision)
            cfg.training.csd_fused_loss = fused
            torch.manual_seed(0)
            model = mutils.create_model(cfg).to(dev)
            m = cfg.model
            sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
            trainers[fused] = train.Trainer(cfg, model, sde)
        g = torch.Generator().manual_seed(1)
        batch = (torch.rand(B, 3, 64, 64, generator=g).to(dev), torch.rand(B, 3, 64, 64, generator=g).to(dev))
        sps = {False: [], True: []}
        for fused in (False, True):
            for _ in range(a.warmup):
                trainers[fused].train_step(batch)
        for _ in range(windows):
            for fused in (False, True):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss = trainers[fused].train_step(batch)
                torch.cuda.synchronize(dev)
                sps[fused].append(a.steps / (time.perf_counter() - t0))
        kern_ms = _loss_kernels_ms(B, [(3, 64, 64), (3, 64, 64)], dev, 'registers')
        d, f = sps[False], sps[True]
        spread = max(d) - min(d)
        rec['routes']['B%d' % B] = {
            'default_steps_per_s': d, 'fused_steps_per_s': f, 'default_mean': float(np.mean(d)), 'fused_mean': float(np.mean(f)),
            'default_window_spread': spread, 'fused_not_slower_than_default_by_more_than_spread': bool(np.mean(f) >= np.mean(d) - spread),
            'fused_loss_kernels_ms': kern_ms, 'fused_loss_kernels_share_of_step': kern_ms * 1e-3 * float(np.mean(f)),
            'default_minus_fused_ms_per_step': 1e3 * (1.0 / float(np.mean(d)) - 1.0 / float(np.mean(f)))}
        for tr in trainers.values():
            tr.close()
        del trainers
        torch.cuda.empty_cache()
    forms = {form: _loss_kernels_ms(64, [(3, 160, 160)], dev, form) for form in ('registers', 'fill')}
    again = {form: _loss_kernels_ms(64, [(3, 160, 160)], dev, form) for form in ('registers', 'fill')}
    rec['noise_forms'] = {'shape': 'SR3-160, B = 64: perturb + residual over 64 x 3 x 160 x 160', 'ms': forms, 'ms_repeat': again,
                          'faster': min(forms, key=forms.get)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='ddpm_paired', choices=['ddpm_paired', 'ncsnpp_paired'])
    ap.add_argument('--executor', default=None, choices=['planned', 'operators'], help='training executor (default: the model\'s = planned)')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=50, help='global batch')
    ap.add_argument('--precision', default='fp32')
    ap.add_argument('--accumulate', type=int, default=0, help='K > 1: time one optimizer step of K micro-batches of batch / K (see above)')
    ap.add_argument('--fused-loss', action='store_true', help='default loss route vs training.csd_fused_loss, and the noise forms (see above)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'train_accumulate.json'),
                    help='--accumulate: the JSON file that receives the record under its own key')
    a = ap.parse_args()
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    grouped = 'RANK' in os.environ and 'MASTER_PORT' in os.environ      # launched by torch.distributed.run: RCCL also at world size 1
    if grouped:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    if a.executor:
        os.environ['CSD_TRAIN_EXECUTOR'] = a.executor
    cfg = make_config(a.precision) if a.model == 'ddpm_paired' else make_ncsnpp_config(a.precision)
    import conditional_score_diffusion_amd.models.ncsnpp  # noqa: F401
    if a.fused_loss:
        if grouped or world > 1 or a.model != 'ddpm_paired':
            sys.exit('--fused-loss is a one-process measurement of ddpm_paired')
        rec = bench_fused_loss(a, dev)
        out = os.path.join(os.path.dirname(a.out), 'train_fused_loss.json') if os.path.basename(a.out) == 'train_accumulate.json' else a.out
        with open(out, 'w') as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write('\n')
        print(json.dumps(rec))
        return
    if a.accumulate > 1:
        if grouped or world > 1:
            sys.exit('--accumulate is a one-process measurement')
        rec = bench_accumulate(a, dev)
        key = '%s_%s_B%d_K%d' % (a.model, a.precision, a.batch, a.accumulate)
        book = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                book = json.load(f)
        book[key] = rec
        with open(a.out, 'w') as f:
            json.dump(book, f, indent=1, sort_keys=True)
            f.write('\n')
        print(json.dumps({key: rec}))
        return
    torch.manual_seed(0)
    model = mutils.create_model(cfg).to(dev)
    m = cfg.model
    sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales),
           'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
    tr = train.Trainer(cfg, model, sde)
    from conditional_score_diffusion_amd.distributed import shard_bounds
    lo, hi = shard_bounds(a.batch, rank, world)       # the config's global batch of 50 over 8 GPUs: 7,7,7,7,7,7,7,1 (ragged)
    B = hi - lo
    if B == 0:
        sys.exit('rank %d has no images (global batch %d over %d ranks)' % (rank, a.batch, world))
    global_n = a.batch if a.batch % world else None
    g = torch.Generator().manual_seed(1 + rank)
    batch = (torch.rand(B, 3, 64, 64, generator=g).to(dev), torch.rand(B, 3, 64, 64, generator=g).to(dev))

    def sync():
        if grouped:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(a.warmup):
        loss = tr.train_step(batch, global_n=global_n)
    sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = tr.train_step(batch, global_n=global_n)
    sync()
    dt = torch.tensor([time.perf_counter() - t0], device=dev)
    if grouped:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    dt = float(dt)
    if rank == 0:
        sps = a.steps / dt
        print(json.dumps({'metric': 'training steps/sec, VS-CMDE edges2shoes 64x64 (%s nf=128), fwd+bwd+all-reduce+Adam/EMA' % a.model,
                          'executor': getattr(model, 'train_executor', None),
                          'value': sps, 'unit': 'steps/sec', 'images_per_sec': sps * a.batch, 'n_gpus': world,
                          'global_batch': a.batch, 'rank0_batch': B, 'ms_per_step': 1e3 * dt / a.steps, 'steps': a.steps, 'warmup': a.warmup,
                          'precision': a.precision, 'params': tr.flat.numel, 'loss': float(loss),
                          'achieved_TFLOPs_3x_fwd': 3 * FWD_GFLOP_PER_IMAGE * 1e-3 * sps * a.batch, 'data': 'synthetic'}))
    if grouped:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
