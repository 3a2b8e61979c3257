"""Side bench of the 3-D DDPM score network (models/ddpm3d.py, csrc/conv3d.hip) at the shape of the reference's MRI -> PET config
(configs/ve/inverse_problems/MRI_to_PET/MRI_to_PET_slices3D.py): ``ddpm3D_paired``, B = 4, 2 x 96 x 96 x 16, nf 64, ch_mult (1, 1, 2, 2),
2 residual blocks per level, swish, fp16x3.

    python tools/bench_ddpm3d.py [--batch 4] [--warmup 2] [--repeats 5] [--evals 3] [--small] [--train | --planned]

Writes profiles/ddpm3d_bench.json (``--out`` to change) and prints it:
  network      evaluations per second: `repeats` windows of `evals` forwards each between device synchronisations, median and spread
  classes      one extra forward with a device-event pair around every operator call, summed per kernel class (the event pairs serialise
               the launches, so the classes add up to more than the untimed forward; shares are what to read)
  layers       csd_conv3d_block (GroupNorm prologue + bias epilogue, weight pack included: it runs in every call) at the two dominant
               layers, 64 -> 64 at 96 x 96 x 16 and 128 -> 128 at 24 x 24 x 4, as achieved TFLOP/s = 2 * 27 * Cin * Cout * voxels * B / time;
               and, as a yardstick outside the code under test, torch's own fp32 F.conv3d (channels-first, no prologue) at the same two
               layers on the same GPU in the same run, the two alternating.
``--train`` measures training instead and writes it under the key ``training`` of the same file (the other keys are kept):
  steps        Trainer.train_step (loss, backward on the grad_ops_3d operators, clip + Adam + EMA) of ``ddpm3D_paired`` with the two-SDE
               loss at B = 2 (``--batch`` is ignored), steps per second over `repeats` windows of `evals` steps
  planned_train  the same step on the planned training graph (``csd_planned_train``: csd_unet_train_forward / csd_unet_backward_acc writing
               the flat gradient) on the same weights and batch in the same process, the two paths' windows alternating: steps per second,
               the ratio, the planned workspace bytes (csd_unet_train_workspace_bytes) beside torch's peak allocated bytes over one step
               of either path (and what was allocated before the step: parameters, optimizer state, both models)
  wgrad        csd_conv3d_wgrad (split bf16) at the same two layers as achieved TFLOP/s = 2 * 27 * Cin * Cout * voxels * B / time, beside
               torch's own fp32 conv3d weight gradient (torch.nn.grad.conv3d_weight, channels-first), the two alternating
``--planned`` measures the planned path (``csd_planned``: one csd_unet_forward per evaluation, the PC loop on the device) beside the
operator path in the same run and writes it under the key ``planned`` (the other keys are kept):
  network      evaluations per second of the operator path and of the planned path on the same weights and inputs, `repeats` windows of
               `evals` forwards each, the two alternating; whether the two outputs are bitwise equal; launches, workspace and packed bytes;
               one extra forward of each path with an event pair around every launch, summed per kernel class
  pc           ms per predictor-corrector step of the two-SDE conditional sampler (cVESDE / VESDE, reverse diffusion + Langevin): the fused
               device loop on the planned model beside the step-by-step loop on the operator-path model, 10 steps after 2 of warm-up,
               `repeats` runs each, alternating
``--small`` runs the same code at a toy shape (a rehearsal of the script; its numbers measure overheads).
Needs the GPU: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
from conditional_score_diffusion_amd import ops  # noqa: E402
from conditional_score_diffusion_amd.config_dict import ConfigDict  # noqa: E402
from conditional_score_diffusion_amd.models import ddpm3d  # noqa: E402
from conditional_score_diffusion_amd.models import utils as mutils  # noqa: E402


def make_config(vol, nf, ch_mult, nrb):
    c = ConfigDict()
    c.training = ConfigDict(continuous=True, sde='vesde')
    c.data = ConfigDict(centered=False, shape_x=[1] + list(vol), shape_y=[1] + list(vol), num_channels=2)
    c.model = ConfigDict(name='ddpm3D_paired', nf=nf, ch_mult=tuple(ch_mult), num_res_blocks=nrb, dropout=0.1, resamp_with_conv=False,
                         conditional=True, nonlinearity='swish', input_channels=2, output_channels=2, csd_precision='fp16x3')
    return c


def conv_flops(model, B, vol):
    """2 * MACs of every 3x3x3 convolution of one evaluation"""
    total = 0.0
    ext = list(vol)
    lvl = 0
    for kind, a in model._mods:
        v = (ext[0] >> lvl) * (ext[1] >> lvl) * (ext[2] >> lvl)
        if kind == 'conv':
            total += 2.0 * 27 * a['cin'] * a['cout'] * v * B
        elif kind == 'res':
            n = a['cin'] * a['cout'] + a['cout'] * a['cout'] + (a['cin'] * a['cout'] if a['cin'] != a['cout'] else 0)
            total += 2.0 * 27 * n * v * B
        elif kind == 'down':
            lvl += 1
        elif kind == 'up':
            lvl -= 1
    return total


class ClassTimer:
    """device-event pairs around the operator calls of models/ddpm3d.py, summed per kernel class"""

    CLASSES = {'conv3d_block': 'conv3d_block', 'groupnorm_scale_shift': 'gn_stats', 'avg_pool3d_2': 'resample', 'nearest_up2_3d': 'resample',
               'linear': 'embedding', 'timestep_embedding': 'embedding', 'axpby': 'other'}

    def __init__(self):
        self.pairs = []

    def wrap(self, name, fn):
        def timed(*a, **k):
            cls = self.CLASSES[name]
            if name == 'conv3d_block' and a[0].shape[-1] % 16:
                cls = 'conv3d_block_direct'
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.pairs.append((cls, e0, e1))
            return out
        return timed

    def run(self, fn):
        saved = {n: getattr(ops, n) for n in self.CLASSES}
        try:
            for n, f in saved.items():
                setattr(ops, n, self.wrap(n, f))
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
        torch.cuda.synchronize()
        ms, calls = {}, {}
        for cls, e0, e1 in self.pairs:
            ms[cls] = ms.get(cls, 0.0) + e0.elapsed_time(e1)
            calls[cls] = calls.get(cls, 0) + 1
        return {'total_ms': t0.elapsed_time(t1), 'classes': {c: {'ms': ms[c], 'calls': calls[c]} for c in sorted(ms)}}


def timed_windows(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner)
    return out


def layer_bench(B, vol, C, warmup, repeats, dev):
    """csd_conv3d_block against torch's fp32 F.conv3d at one layer, alternating windows"""
    g = torch.Generator(device='cpu').manual_seed(0)
    x = torch.randn(B, *vol, C, generator=g).to(dev)
    w = (torch.randn(C, C, 3, 3, 3, generator=g) * (2.0 / (27 * 2 * C)) ** 0.5).to(dev)
    b = torch.zeros(C, device=dev)
    ns, nh = torch.ones(B, C, device=dev), torch.zeros(B, C, device=dev)
    xc = x.permute(0, 4, 1, 2, 3).contiguous()
    flops = 2.0 * 27 * C * C * vol[0] * vol[1] * vol[2] * B
    inner = max(1, int(2e12 / flops / 10))          # windows of >= ~0.1 s at a few TFLOP/s, more at speed
    ours = lambda: ops.conv3d_block(x, w, b, nscale=ns, nshift=nh, act='swish', precision='fp16x3')      # noqa: E731
    theirs = lambda: F.conv3d(xc, w, b, padding=1)                                                        # noqa: E731
    t_o, t_t = [], []
    for f in (ours, theirs):
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    for _ in range(repeats):
        t_o += timed_windows(ours, 0, 1, inner)
        t_t += timed_windows(theirs, 0, 1, inner)
    mo, mt = statistics.median(t_o), statistics.median(t_t)
    return {'layer': '%d->%d at %dx%dx%d, B=%d' % (C, C, vol[0], vol[1], vol[2], B), 'gflop': flops / 1e9, 'calls_per_window': inner,
            'conv3d_block_fp16x3': {'ms': mo * 1e3, 'ms_min': min(t_o) * 1e3, 'ms_max': max(t_o) * 1e3, 'tflops': flops / mo / 1e12},
            'torch_fp32_conv3d': {'ms': mt * 1e3, 'ms_min': min(t_t) * 1e3, 'ms_max': max(t_t) * 1e3, 'tflops': flops / mt / 1e12},
            'conv3d_block_over_torch': mt / mo}


def wgrad_bench(B, vol, C, warmup, repeats, dev):
    """csd_conv3d_wgrad (split bf16) against torch's fp32 conv3d weight gradient at one layer, alternating windows"""
    from conditional_score_diffusion_amd import grad_ops_3d as G
    g = torch.Generator(device='cpu').manual_seed(0)
    a = torch.randn(B, *vol, C, generator=g).to(dev)
    dy = torch.randn(B, *vol, C, generator=g).to(dev)
    ac, dyc = a.permute(0, 4, 1, 2, 3).contiguous(), dy.permute(0, 4, 1, 2, 3).contiguous()
    flops = 2.0 * 27 * C * C * vol[0] * vol[1] * vol[2] * B
    inner = max(1, int(2e12 / flops / 10))
    ours = lambda: G.conv3d_wgrad(a, dy, 'fp16x3')                                                      # noqa: E731
    theirs = lambda: torch.nn.grad.conv3d_weight(ac, (C, C, 3, 3, 3), dyc, padding=1)                  # noqa: E731
    t_o, t_t = [], []
    for f in (ours, theirs):
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    for _ in range(repeats):
        t_o += timed_windows(ours, 0, 1, inner)
        t_t += timed_windows(theirs, 0, 1, inner)
    mo, mt = statistics.median(t_o), statistics.median(t_t)
    return {'layer': '%d->%d at %dx%dx%d, B=%d' % (C, C, vol[0], vol[1], vol[2], B), 'gflop': flops / 1e9, 'calls_per_window': inner,
            'conv3d_wgrad_split_bf16': {'ms': mo * 1e3, 'ms_min': min(t_o) * 1e3, 'ms_max': max(t_o) * 1e3, 'tflops': flops / mo / 1e12},
            'torch_fp32_conv3d_weight': {'ms': mt * 1e3, 'ms_min': min(t_t) * 1e3, 'ms_max': max(t_t) * 1e3, 'tflops': flops / mt / 1e12},
            'conv3d_wgrad_over_torch': mt / mo}


def train_bench(args, dev):
    from conditional_score_diffusion_amd import sde_lib, train
    vol, nf, ch_mult, nrb = ((12, 12, 8), 32, (1, 2), 1) if args.small else ((96, 96, 16), 64, (1, 1, 2, 2), 2)
    B = 2

    def config(planned_train):
        cfg = make_config(vol, nf, ch_mult, nrb)
        cfg.training.likelihood_weighting = cfg.training.reduce_mean = True
        cfg.model.ema_rate = 0.999
        cfg.model.num_scales, cfg.model.sigma_min_y, cfg.model.sigma_max_y = 1000, 0.01, 1.
        cfg.model.csd_planned_train = planned_train
        cfg.optim = ConfigDict(weight_decay=0, optimizer='Adam', lr=2e-4, beta1=0.9, eps=1e-8, warmup=100, grad_clip=1)
        cfg.seed = 42
        return cfg
    cfg = config(False)
    torch.manual_seed(0)
    model = mutils.create_model(cfg)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if v.dim() == 5:
                v.copy_((torch.rand_like(v) * 2 - 1) * (3.0 / (27 * (v.shape[0] + v.shape[1]) / 2)) ** 0.5)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    sde = {'x': sde_lib.cVESDE(0.01, 30., 1000), 'y': sde_lib.VESDE(0.01, 1., 1000)}
    tr = train.Trainer(cfg, model, sde)
    batch = (torch.rand(B, 1, *vol).to(dev), torch.rand(B, 1, *vol).to(dev))
    losses = []
    step = lambda: losses.append(tr.train_step(batch))      # noqa: E731
    # the planned training graph (planned_train) on the same weights, batch and seeds, in the same process
    from conditional_score_diffusion_amd._lib import lib
    cfg_p = config(True)
    model_p = mutils.create_model(cfg_p)
    model_p.load_state_dict(state)
    model_p = model_p.to(dev)
    tr_p = train.Trainer(cfg_p, model_p, sde)
    losses_p = []
    step_p = lambda: losses_p.append(tr_p.train_step(batch))      # noqa: E731

    def peak_of(fn):
        """torch's peak allocated bytes over one step, and what was allocated before it"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return {'peak_allocated_bytes': int(torch.cuda.max_memory_allocated()), 'allocated_before_bytes': int(base)}

    for f in (step, step_p):
        timed_windows(f, args.warmup, 0, 0)
    win, win_p = [], []
    for _ in range(args.repeats):                           # the two paths alternate
        win += timed_windows(step, 0, 1, args.evals)
        win_p += timed_windows(step_p, 0, 1, args.evals)
    mem, mem_p = peak_of(step), peak_of(step_p)
    vals = [float(v) for v in losses]
    vals_p = [float(v) for v in losses_p]
    assert all(v == v and abs(v) != float('inf') for v in vals + vals_p), (vals, vals_p)
    med, med_p = statistics.median(win), statistics.median(win_p)
    planned_train = {
        'steps': {'steps_per_s': 1.0 / med_p, 'ms_per_step': med_p * 1e3, 'ms_min': min(win_p) * 1e3, 'ms_max': max(win_p) * 1e3,
                  'windows': len(win_p), 'steps_per_window': args.evals, 'first_loss': vals_p[0], 'last_loss': vals_p[-1]},
        'operator_path_steps_per_s': 1.0 / med, 'planned_over_operator': med / med_p,
        'planned_workspace_bytes': int(lib().csd_unet_train_workspace_bytes(model_p._h, B, 0.1)),
        'planned_step_memory': mem_p, 'operator_path_step_memory': mem,
        'backward_direct': bool(getattr(model_p, '_last_backward_direct', False))}
    lv = [((12, 12, 8), 32), ((6, 6, 4), 64)] if args.small else [((96, 96, 16), 64), ((24, 24, 4), 128)]
    return {'device': torch.cuda.get_device_name(0), 'model': 'ddpm3D_paired', 'precision': 'fp16x3', 'batch': B, 'volume': list(vol), 'nf': nf,
            'ch_mult': list(ch_mult), 'num_res_blocks': nrb, 'small': bool(args.small), 'dropout': 0.1,
            'steps': {'steps_per_s': 1.0 / med, 'ms_per_step': med * 1e3, 'ms_min': min(win) * 1e3, 'ms_max': max(win) * 1e3, 'windows': len(win),
                      'steps_per_window': args.evals, 'first_loss': vals[0], 'last_loss': vals[-1]},
            'planned_train': planned_train,
            'wgrad': [wgrad_bench(B, v, C, args.warmup, args.repeats, dev) for v, C in lv], 'torch': torch.__version__}


def planned_bench(args, dev):
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd._lib import lib
    from conditional_score_diffusion_amd.sampling import conditional, fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    vol, nf, ch_mult, nrb = ((12, 12, 8), 32, (1, 2), 1) if args.small else ((96, 96, 16), 64, (1, 1, 2, 2), 2)
    B = args.batch
    torch.manual_seed(0)
    op_model = mutils.create_model(make_config(vol, nf, ch_mult, nrb))
    with torch.no_grad():
        for k, v in op_model.state_dict().items():
            if v.dim() == 5:
                v.copy_((torch.rand_like(v) * 2 - 1) * (3.0 / (27 * (v.shape[0] + v.shape[1]) / 2)) ** 0.5)
    cfg = make_config(vol, nf, ch_mult, nrb)
    cfg.model.csd_planned = True
    model = mutils.create_model(cfg)
    model.load_state_dict(op_model.state_dict())
    op_model, model = op_model.to(dev).eval(), model.to(dev).eval()
    x = (5.0 * torch.randn(B, 1, *vol)).to(dev)
    y = torch.rand(B, 1, *vol).to(dev)
    labels = torch.linspace(3., 420.5, B).to(dev)
    fwd_op = lambda: op_model({'x': x, 'y': y}, labels)      # noqa: E731
    fwd_pl = lambda: model({'x': x, 'y': y}, labels)         # noqa: E731
    a, b = fwd_op(), fwd_pl()
    torch.cuda.synchronize()
    equal = all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.isfinite(v).all() for v in b.values())
    for f in (fwd_op, fwd_pl):
        timed_windows(f, args.warmup, 0, 0)
    t_op, t_pl = [], []
    for _ in range(args.repeats):
        t_op += timed_windows(fwd_op, 0, 1, args.evals)
        t_pl += timed_windows(fwd_pl, 0, 1, args.evals)
    m_op, m_pl = statistics.median(t_op), statistics.median(t_pl)
    launches, flops, nbytes = model.stats(B)
    # one extra forward each with an event pair around every launch (planned: the library's own profiler), summed per class
    from conditional_score_diffusion_amd import _lib
    prof_op = ClassTimer().run(fwd_op)
    _lib.profile_select(None, 1)
    _lib.profile_start()
    fwd_pl()
    prof_pl = {c: {'ms': v['ms'], 'launches': v['launches']} for c, v in _lib.profile_stop().items() if v['launches']}
    side = lambda t, m: {'evals_per_s': 1.0 / m, 'ms_per_eval': m * 1e3, 'ms_min': min(t) * 1e3, 'ms_max': max(t) * 1e3}      # noqa: E731
    net = {'operator_path': side(t_op, m_op), 'planned': side(t_pl, m_pl), 'planned_over_operator': m_op / m_pl, 'bitwise_equal': equal,
           'windows': len(t_pl), 'evals_per_window': args.evals, 'planned_launches': launches, 'planned_gflop': flops / 1e9,
           'workspace_bytes': int(lib().csd_unet_workspace_bytes(model._h, B)), 'packed_bytes': int(lib().csd_unet_packed_bytes(model._h)),
           'profile_pass': {'operator_path': prof_op, 'planned': prof_pl}}

    # the PC sampler: fused device loop (planned model) beside the step-by-step loop (operator-path model)
    sde = {'x': sde_lib.cVESDE(0.01, 30., 1000), 'y': sde_lib.VESDE(0.01, 1., 1000)}
    pred, corr = get_predictor('conditional_reverse_diffusion'), get_corrector('conditional_langevin')
    assert fused.fusable(model, sde, pred, corr, 1, False, True) and not fused.fusable(op_model, sde, pred, corr, 1, False, True)
    shape = (B, 1) + tuple(vol)
    mk = lambda n: conditional.get_pc_conditional_sampler(sde, shape, pred, corr, snr=0.16, p_steps=n, c_steps=1, continuous=True,      # noqa: E731
                                                          denoise=True, eps=1e-5)
    steps = 10

    def run(sampler, m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, _ = sampler(m, y)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return time.perf_counter() - t0

    t_f, t_s = [], []
    run(mk(2), model)
    run(mk(2), op_model)
    for _ in range(args.repeats):
        t_f.append(run(mk(steps), model) / steps)
        t_s.append(run(mk(steps), op_model) / steps)
    m_f, m_s = statistics.median(t_f), statistics.median(t_s)
    pc = {'steps': steps, 'warmup_steps': 2, 'runs': args.repeats,
          'fused_loop': {'ms_per_step': m_f * 1e3, 'ms_min': min(t_f) * 1e3, 'ms_max': max(t_f) * 1e3},
          'step_by_step': {'ms_per_step': m_s * 1e3, 'ms_min': min(t_s) * 1e3, 'ms_max': max(t_s) * 1e3},
          'fused_over_step_by_step': m_s / m_f,
          'pc_scratch_bytes': int(lib().csd_pc_scratch_bytes(model._h, B))}
    return {'device': torch.cuda.get_device_name(0), 'model': 'ddpm3D_paired', 'precision': 'fp16x3', 'batch': B, 'volume': list(vol), 'nf': nf,
            'ch_mult': list(ch_mult), 'num_res_blocks': nrb, 'small': bool(args.small), 'network': net, 'pc': pc, 'torch': torch.__version__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--evals', type=int, default=3)
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--train', action='store_true')
    ap.add_argument('--planned', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ddpm3d_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ddpm3d.py needs the MI355X: there is no CPU path')
    dev = torch.device('cuda:0')
    if args.train or args.planned:
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        key = 'training' if args.train else 'planned'
        res[key] = train_bench(args, dev) if args.train else planned_bench(args, dev)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res[key]))
        return
    vol, nf, ch_mult, nrb = ((12, 12, 8), 32, (1, 2), 1) if args.small else ((96, 96, 16), 64, (1, 1, 2, 2), 2)
    B = args.batch
    torch.manual_seed(0)
    model = mutils.create_model(make_config(vol, nf, ch_mult, nrb))
    assert isinstance(model, ddpm3d.DDPM3D_paired)
    with torch.no_grad():       # the reference zero-initialises Conv_1 and the head: give them weights so that nothing is degenerate
        for k, v in model.state_dict().items():
            if v.dim() == 5:
                v.copy_((torch.rand_like(v) * 2 - 1) * (3.0 / (27 * (v.shape[0] + v.shape[1]) / 2)) ** 0.5)
    model = model.to(dev).eval()
    x = (5.0 * torch.randn(B, 1, *vol)).to(dev)
    y = torch.rand(B, 1, *vol).to(dev)
    labels = torch.linspace(3., 420.5, B).to(dev)
    fwd = lambda: model({'x': x, 'y': y}, labels)         # noqa: E731
    out = fwd()
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in out.values())
    win = timed_windows(fwd, args.warmup, args.repeats, args.evals)
    med = statistics.median(win)
    flops = conv_flops(model, B, vol)
    res = {'device': torch.cuda.get_device_name(0), 'model': 'ddpm3D_paired', 'precision': 'fp16x3', 'batch': B, 'volume': list(vol), 'nf': nf,
           'ch_mult': list(ch_mult), 'num_res_blocks': nrb, 'small': bool(args.small),
           'network': {'evals_per_s': 1.0 / med, 'volumes_per_s': B / med, 'ms_per_eval': med * 1e3, 'ms_min': min(win) * 1e3,
                       'ms_max': max(win) * 1e3, 'windows': len(win), 'evals_per_window': args.evals, 'conv_gflop_per_eval': flops / 1e9,
                       'conv_tflops_end_to_end': flops / med / 1e12},
           'profile_pass': ClassTimer().run(fwd)}
    lv = [((12, 12, 8), 32), ((6, 6, 4), 64)] if args.small else [((96, 96, 16), 64), ((24, 24, 4), 128)]
    res['layers'] = [layer_bench(B, v, C, args.warmup, args.repeats, dev) for v, C in lv]
    res['torch'] = torch.__version__
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
