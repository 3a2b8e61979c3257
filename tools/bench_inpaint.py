"""Side bench of PC inpainting with an unconditional network (sampling/unconditional.py:get_pc_inpainter; not the driver's bench):
the step-by-step loop against the fused device loop (`device_loop=True`), measured alternately in ONE process on the same model,
data, mask and schedule.

Workload: `ddpm`, nf 128, ch_mult (1, 2, 2, 2), 2 residual blocks, attention at 16 x 16, 64 x 64 images, B = 64, half-image mask,
VE SDE with (reverse diffusion, Langevin), random weights.  A run is one call of the inpainter (sde.N = --steps PC steps, two network
evaluations each); its time is a host clock around the call and a device synchronise.  One warm-up run per path, then --reps
alternating pairs.  Reports ms per PC step of both paths (mean, min, max over the repeats) and writes the JSON:

  python tools/bench_inpaint.py [--steps 20] [--reps 5] [--batch 64] [--precision fp16x3] [--out profiles/inpaint_bench.json]

--colorize measures PC colorization (get_pc_colorizer) the same way on the same network and schedule, with a gray-scale batch in place
of data and mask, and writes profiles/colorize_bench.json.  It also times the two re-imposition kernels alone at the run's state size,
alternately, between device events: ops.inpaint_blend and ops.colorize_blend, both drawing their noise in registers and both writing
x_mean (`blend_kernels_us`).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from conditional_score_diffusion_amd import sde_lib  # noqa: E402
from conditional_score_diffusion_amd.models import utils as mutils  # noqa: E402
from conditional_score_diffusion_amd.sampling import unconditional  # noqa: E402
from conditional_score_diffusion_amd.sampling.correctors import get_corrector  # noqa: E402
from conditional_score_diffusion_amd.sampling.predictors import get_predictor  # noqa: E402


def ddpm_64_config():
    """an unconditional DDPM at 64 x 64: the keys the hot path reads (cf. bench.sr3_160_config)"""
    from conditional_score_diffusion_amd.config_dict import ConfigDict
    c = bench.sr3_160_config()
    S = 64
    smax = float(np.sqrt(3 * S * S))
    c.training.conditioning_approach = None
    c.sampling.predictor, c.sampling.corrector = 'reverse_diffusion', 'langevin'
    c.data = ConfigDict(image_size=S, effective_image_size=S, centered=False, shape_x=[3, S, S], shape_y=[3, S, S], num_channels=3)
    c.model.update(dict(name='ddpm', nf=128, ch_mult=(1, 2, 2, 2), num_res_blocks=2, attn_resolutions=(16,), sigma_max_x=smax,
                        sigma_max=smax, input_channels=3, output_channels=3))
    return c


def timed(fn, model, data, mask, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, _ = fn(model, data, mask, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if not bool(torch.isfinite(x).all()):
        raise RuntimeError('the inpainter returned non-finite values')
    return dt, x


def timed_colorize(fn, model, gray, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, _ = fn(model, gray, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if not bool(torch.isfinite(x).all()):
        raise RuntimeError('the colorizer returned non-finite values')
    return dt, x


def blend_kernels_us(shape, dev, reps=50):
    """microseconds per launch of the two re-imposition kernels on a state of ``shape``, alternating windows of 10 launches"""
    from conditional_score_diffusion_amd import ops
    x = ops.randn(shape, 3, 0, dev)
    data, mask = torch.rand(shape, device=dev), (torch.rand(shape, device=dev) < 0.5).float()
    gray0 = ops.colorize_gray0(torch.rand(shape, device=dev))
    calls = {'inpaint_blend': lambda: ops.inpaint_blend(x, data, mask, None, 1.0, 0.5, seed=1, stream_id=1),
             'colorize_blend': lambda: ops.colorize_blend(x, gray0, None, 1.0, 0.5, seed=1, stream_id=1)}
    us = {k: [] for k in calls}
    for fn in calls.values():
        fn()
    for _ in range(reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 100.0)
    return {k: {'mean': float(np.mean(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in us.items()}


def main_colorize(a, cfg, model, dev):
    S, B = cfg.data.image_size, a.batch
    rs = np.random.RandomState(78)
    gray = torch.from_numpy(np.repeat(rs.uniform(0, 1, size=(B, 1, S, S)).astype(np.float32), 3, axis=1).copy()).to(dev)
    sde = sde_lib.VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, a.steps)
    kw = dict(snr=cfg.sampling.snr, n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-5)
    paths = {'step_by_step': (unconditional.get_pc_colorizer(sde, get_predictor('reverse_diffusion'), get_corrector('langevin'), **kw), {}),
             'device_loop': (unconditional.get_pc_colorizer(sde, get_predictor('reverse_diffusion'), get_corrector('langevin'),
                                                            device_loop=True, **kw), {'seed': 1})}
    for name, (fn, extra) in paths.items():                 # warm-up
        timed_colorize(fn, model, gray, **extra)
    ms = {name: [] for name in paths}
    for _ in range(a.reps):
        for name, (fn, extra) in paths.items():
            ms[name].append(timed_colorize(fn, model, gray, **extra)[0] * 1e3 / a.steps)
    r = {'workload': 'PC colorization, unconditional ddpm nf 128 ch_mult (1,2,2,2) 64x64, VE reverse_diffusion/langevin',
         'device': torch.cuda.get_device_name(0), 'batch': B, 'precision': a.precision, 'pc_steps_per_run': a.steps, 'reps': a.reps}
    for name, v in ms.items():
        r[name] = {'ms_per_pc_step_mean': float(np.mean(v)), 'ms_per_pc_step_min': float(np.min(v)), 'ms_per_pc_step_max': float(np.max(v)),
                   'ms_per_pc_step_runs': [round(float(t), 4) for t in v]}
    r['step_by_step_over_device_loop'] = r['step_by_step']['ms_per_pc_step_mean'] / r['device_loop']['ms_per_pc_step_mean']
    r['blend_kernels_us'] = blend_kernels_us((B, 3, S, S), dev)
    r['colorize_blend_over_inpaint_blend'] = r['blend_kernels_us']['colorize_blend']['mean'] / r['blend_kernels_us']['inpaint_blend']['mean']
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--precision', default='fp16x3')
    ap.add_argument('--colorize', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'colorize_bench.json' if a.colorize else 'inpaint_bench.json')
    if not torch.cuda.is_available():
        raise SystemExit('bench_inpaint.py measures on the GPU; there is none here (nothing measured)')
    dev = torch.device('cuda:0')
    cfg = ddpm_64_config()
    cfg.model.csd_precision = a.precision
    model = mutils.create_model(cfg)
    model.load_state_dict(bench.synth_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0))
    model = model.to(dev).eval()
    if a.colorize:
        return write(a.out, main_colorize(a, cfg, model, dev))
    S, B = cfg.data.image_size, a.batch
    rs = np.random.RandomState(77)
    data = torch.from_numpy(rs.uniform(0, 1, size=(B, 3, S, S)).astype(np.float32)).to(dev)
    mask = torch.zeros(B, 3, S, S, device=dev)
    mask[:, :, :, : S // 2] = 1.
    sde = sde_lib.VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, a.steps)
    kw = dict(snr=cfg.sampling.snr, n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-5)
    paths = {'step_by_step': (unconditional.get_pc_inpainter(sde, get_predictor('reverse_diffusion'), get_corrector('langevin'), **kw), {}),
             'device_loop': (unconditional.get_pc_inpainter(sde, get_predictor('reverse_diffusion'), get_corrector('langevin'),
                                                            device_loop=True, **kw), {'seed': 1})}
    known_err = {}
    for name, (fn, extra) in paths.items():                 # warm-up: code objects, the plan, the workspace
        _, x = timed(fn, model, data, mask, **extra)
        known_err[name] = float(((x - data) * mask).abs().max())
    ms = {name: [] for name in paths}
    for _ in range(a.reps):
        for name, (fn, extra) in paths.items():
            ms[name].append(timed(fn, model, data, mask, **extra)[0] * 1e3 / a.steps)
    r = {'workload': 'PC inpainting, unconditional ddpm nf 128 ch_mult (1,2,2,2) 64x64, VE reverse_diffusion/langevin, half-image mask',
         'device': torch.cuda.get_device_name(0), 'batch': B, 'precision': a.precision, 'pc_steps_per_run': a.steps, 'reps': a.reps,
         'known_pixels_max_abs_err': known_err}
    for name, v in ms.items():
        r[name] = {'ms_per_pc_step_mean': float(np.mean(v)), 'ms_per_pc_step_min': float(np.min(v)), 'ms_per_pc_step_max': float(np.max(v)),
                   'ms_per_pc_step_runs': [round(float(t), 4) for t in v]}
    r['step_by_step_over_device_loop'] = r['step_by_step']['ms_per_pc_step_mean'] / r['device_loop']['ms_per_pc_step_mean']
    write(a.out, r)


def write(out, r):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(r, f, indent=1)
        f.write('\n')
    print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
