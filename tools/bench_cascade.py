"""Side bench of the sequential cascades (sampling/cascade.py; bench.py is the flagship's and is not involved).

    python tools/bench_cascade.py [--pc-steps 8] [--steps 20] [--warmup 5] [--precision fp16x3] [--batch 64] [--out profiles/cascade_bench.json]

The celebAHQ 40 -> 80 -> 160 bicubic cascade at the stage shapes of configs/ve/srflow/celebAHQ160/sequential/bicubic/config_{80,160}.py
(ddpm_2xSR, nf 96, ch_mult (1, 1, 2, 2), two blocks per level, attention at 20 / 10 / 5), random weights (score_oracle.synth_params),
a synthetic 40^2 input, B = 64, `pc-steps` PC steps per stage with on-device noise.  Reported:
  one_call_ms       the whole cascade as ONE csd_pc_cascade_sample (get_autoregressive_sampler(one_call=True)): both stages' loops
                    enqueued back to back, one synchronisation
  chained_ms        the same stages through their per-stage samplers chained in Python (one_call=False): one synchronisation per stage
  host_round_trip_ms  chained_ms - one_call_ms: what the removed synchronisation(s) and the per-stage Python set-up between them are
                    worth.  The stages are the same launches on both routes (bitwise_equal checks the results).
  band_split_gbs / band_merge_gbs   the band kernels alone on [B, 3, 160, 160] <-> [B, 12, 80, 80]: bytes read + written per second
Timing as tools/bench_sr.py: the cascades one warm run, then the median of three runs between device events (each run ends with the
library's own synchronisation); the band kernels `warmup` calls, then the median of three device-event windows of `steps` calls.  One
JSON object, also printed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
import cases  # noqa: E402
import score_oracle as so  # noqa: E402

NET = dict(nf=96, ch_mult=(1, 1, 2, 2), attn_resolutions=(20, 10, 5), num_res_blocks=2)
SIDES = (40, 80)              # the side each stage's network runs at (= the side of its condition)
BATCH = 64


def make_config(S, precision):
    """a 2x stage on 3-channel images: configs/ve/srflow/celebAHQ160/sequential/bicubic/config_160.py:81-87,103-104,140-141"""
    cfg = cases.make_config(name='ddpm_2xSR', image_size=S, x_ch=12, y_ch=3, **NET)
    d, m = cfg.data, cfg.model
    d.num_channels = 15
    m.input_channels = m.output_channels = 15
    d.image_size, d.effective_image_size = 2 * S, S
    d.shape_x, d.shape_y = [3, 2 * S, 2 * S], [3, S, S]
    m.sigma_max_x = m.sigma_max = float(np.sqrt(12 * S * S))
    m.sigma_max_y = float(np.sqrt(3 * S * S))
    m.csd_precision = precision
    return cfg


def event_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def median3(fn):
    v = sorted(fn() for _ in range(3))
    return v[1], [v[0], v[2]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pc-steps', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--precision', default='fp16x3')
    ap.add_argument('--batch', type=int, default=BATCH)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cascade_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_cascade.py needs the MI355X: there is no CPU path to time')
    from conditional_score_diffusion_amd import ops, sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import cascade
    dev = torch.device('cuda:0')
    B = args.batch
    stages = []
    for S in SIDES:
        cfg = make_config(S, args.precision)
        m = cfg.model
        net = mutils.create_model(cfg)
        net.load_state_dict(so.synth_params(so.ddpm_param_shapes(so.NetCfg.from_config(cfg)), 0))
        sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
        stages.append((net.to(dev).eval(), sde, cfg))
    lr = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, (B, 3, SIDES[0], SIDES[0])).astype(np.float32)).to(dev)
    routes = {key: cascade.get_autoregressive_sampler(stages, 'bicubic', p_steps=args.pc_steps, one_call=flag)
              for key, flag in (('one_call_ms', True), ('chained_ms', False))}
    out = {'device': torch.cuda.get_device_name(0), 'precision': args.precision, 'batch': B, 'pc_steps_per_stage': args.pc_steps,
           'stage_sides': [[S, 2 * S] for S in SIDES], 'nf': NET['nf'], 'ch_mult': list(NET['ch_mult']), 'steps': args.steps,
           'warmup': args.warmup}
    results = {}
    for key, fn in routes.items():
        results[key] = fn(lr, seed=1)[0]                       # the warm run
        torch.cuda.synchronize()
    out['bitwise_equal'] = bool(torch.equal(results['one_call_ms'], results['chained_ms']))
    rounds = {key: [] for key in routes}
    for _ in range(3):                                         # alternating runs
        for key, fn in routes.items():
            rounds[key].append(event_ms(lambda: fn(lr, seed=1)))
    for key, v in rounds.items():
        v = sorted(v)
        out[key], out[key + '_spread'] = v[1], [v[0], v[2]]
    out['host_round_trip_ms'] = out['chained_ms'] - out['one_call_ms']
    out['images_per_s_one_call'] = B * 1e3 / out['one_call_ms']
    # the band kernels alone
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((B, 3, 160, 160)).astype(np.float32)).to(dev)
    bands = ops.band_split(x)
    image = torch.empty_like(x)
    nbytes = 2.0 * x.numel() * 4
    calls = {'band_split': lambda: ops.band_split(x), 'band_merge': lambda: ops.band_merge(bands[:, :3], bands[:, 3:], out=image)}
    for key, fn in calls.items():
        for _ in range(args.warmup):
            fn()
        ms, spread = median3(lambda: event_ms(fn, args.steps))
        out[key + '_ms'], out[key + '_ms_spread'] = ms, spread
        out[key + '_gbs'] = nbytes / (ms * 1e-3) / 1e9
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
