"""Side bench of the DDPM family on images with more than 8 channels (bench.py is the flagship's and is not involved).

    python tools/bench_wide.py [--steps 20] [--warmup 5] [--pc-steps 8] [--precision fp16x3] [--out profiles/wide_bench.json]

Two shapes, random weights (score_oracle.synth_params), synthetic inputs:
  mri_slices  ddpm_paired, 16 + 16 channels in, 32 out, 96^2, nf 128, ch_mult (1, 1, 2, 2, 2), attention at 24 / 12 / 6, two blocks per
              level, B = 12 (configs/ve/inverse_problems/MRI_to_PET/MRI_to_PET_slices.py)
  haar_80     ddpm, 12 channels (the Haar bands), 80^2, nf 128, ch_mult (1, 1, 2, 2), attention at 20 / 10 / 5, two blocks per level,
              B = 64 (the shape of configs/ve/srflow/celebA/haar/config_80.py)
Per shape: network evaluations per second (csd_unet_forward, device events around `steps` calls) and milliseconds per PC step of the
fused device loop (reverse diffusion + Langevin, the two-SDE pair for mri_slices: two evaluations per step, on-device noise), and the
first layer alone as an operator, alternating the one-launch wide layer (stem.hip: stem_wide_kernel) with the assemble pass + generic
convolution (ops.input_conv; both timings include the operator's own weight pack, two small launches).  One JSON object, also printed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
import cases  # noqa: E402
import score_oracle as so  # noqa: E402

SHAPES = {
    'mri_slices': dict(name='ddpm_paired', x_ch=16, y_ch=16, image_size=96, nf=128, ch_mult=(1, 1, 2, 2, 2), attn_resolutions=(24, 12, 6),
                       num_res_blocks=2, B=12),
    'haar_80': dict(name='ddpm', x_ch=12, y_ch=12, image_size=80, nf=128, ch_mult=(1, 1, 2, 2), attn_resolutions=(20, 10, 5),
                    num_res_blocks=2, B=64),
}


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_shape(tag, kw, args):
    from conditional_score_diffusion_amd import ops, sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    kw = dict(kw)
    B = args.batch or kw.pop('B')
    kw.pop('B', None)
    cfg = cases.make_config(**kw)
    cfg.model.csd_precision = args.precision
    dev = torch.device('cuda:0')
    model = mutils.create_model(cfg)
    model.load_state_dict(so.synth_params(so.ddpm_param_shapes(so.NetCfg.from_config(cfg)), 0))
    model = model.to(dev).eval()
    m, S, cx = cfg.model, cfg.data.image_size, kw['x_ch']
    paired = m.name != 'ddpm'
    cy = kw['y_ch'] if paired else 0
    rs = np.random.RandomState(0)
    x = torch.from_numpy((rs.standard_normal((B, cx, S, S)) * 5).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.uniform(0, 1, (B, cy, S, S)).astype(np.float32)).to(dev) if paired else None
    labels = torch.from_numpy(rs.uniform(1, 999, B).astype(np.float32)).to(dev)
    call = (lambda: model({'x': x, 'y': y}, labels)) if paired else (lambda: model(x, labels))
    res = {'model': m.name, 'channels_in': cx + cy, 'channels_out': int(m.output_channels), 'image_size': S, 'nf': m.nf, 'batch': B,
           'precision': args.precision}
    with torch.no_grad():
        for _ in range(args.warmup):
            call()
        ms = sorted(event_ms(call, args.steps) for _ in range(3))
    res['forward_ms'] = ms[1]
    res['forward_ms_spread'] = [ms[0], ms[2]]
    res['evaluations_per_s'] = 1e3 / ms[1]
    res['samples_per_s'] = B * 1e3 / ms[1]
    # fused PC loop: reverse diffusion + Langevin (the conditional forms for the paired network), continuous, on-device noise
    if paired:
        sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
        P, C = get_predictor('conditional_reverse_diffusion'), get_corrector('conditional_langevin')
    else:
        sde = sde_lib.VESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales)
        P, C = get_predictor('reverse_diffusion'), get_corrector('langevin')
    assert fused.fusable(model, sde, P, C, 1, False, True)
    xs = (B, cx, S, S)
    extra = {} if paired else {'unconditional_label': 'sigma'}

    def pc():
        fused.run(model, sde, xs, y, args.pc_steps, cfg.sampling.snr, 1e-5, True, seed=1, predictor=P, corrector=C, probability_flow=False,
                  continuous=True, **extra)
    pc()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        pc()                                   # (the loop's last call synchronises: the finiteness check)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / args.pc_steps)
    ts.sort()
    res['pc_step_ms'] = ts[1]
    res['pc_step_ms_spread'] = [ts[0], ts[2]]
    # the first layer alone, fused and generic alternating
    w = model.all_modules[2].weight.detach().contiguous()
    b = model.all_modules[2].bias.detach().contiguous()
    fl = {}
    for fused_flag in (True, False):
        ops.input_conv(x, y, w, b, precision=args.precision, fused=fused_flag)
    rounds = {True: [], False: []}
    for _ in range(5):
        for fused_flag in (True, False):
            rounds[fused_flag].append(event_ms(lambda: ops.input_conv(x, y, w, b, precision=args.precision, fused=fused_flag), args.steps))
    for fused_flag, key in ((True, 'fused_wide_stem_us'), (False, 'assemble_plus_generic_conv_us')):
        v = sorted(rounds[fused_flag])
        fl[key] = v[2] * 1e3
        fl[key + '_spread'] = [v[0] * 1e3, v[4] * 1e3]
    out_bytes = B * S * S * m.nf * 4
    fl['output_mb'] = out_bytes / 1e6
    fl['fused_output_gb_per_s'] = out_bytes / (fl['fused_wide_stem_us'] * 1e-6) / 1e9
    res['first_layer'] = fl
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--pc-steps', type=int, default=8)
    ap.add_argument('--precision', default='fp16x3')
    ap.add_argument('--batch', type=int, default=0, help='override both shapes\' batch sizes')
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wide_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_wide.py needs the MI355X: there is no CPU path to time')
    out = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'pc_steps': args.pc_steps, 'shapes': {}}
    for tag in args.shapes.split(','):
        out['shapes'][tag] = bench_shape(tag, SHAPES[tag], args)
    text = json.dumps(out, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
