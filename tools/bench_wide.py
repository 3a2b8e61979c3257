"""Side bench of the DDPM family on images with more than 8 channels (bench.py is the flagship's and is not involved).

    python tools/bench_wide.py [--steps 20] [--warmup 5] [--pc-steps 8] [--precision fp16x3] [--out profiles/wide_bench.json]

Two shapes, random weights (score_oracle.synth_params), synthetic inputs:
  mri_slices  ddpm_paired, 16 + 16 channels in, 32 out, 96^2, nf 128, ch_mult (1, 1, 2, 2, 2), attention at 24 / 12 / 6, two blocks per
              level, B = 12 (configs/ve/inverse_problems/MRI_to_PET/MRI_to_PET_slices.py)
  haar_80     ddpm, 12 channels (the Haar bands), 80^2, nf 128, ch_mult (1, 1, 2, 2), attention at 20 / 10 / 5, two blocks per level,
              B = 64 (the shape of configs/ve/srflow/celebA/haar/config_80.py)
``--family ncsnpp`` runs the same two shapes on NCSN++ (ncsnpp_paired; the 12 Haar bands as the 9 + 3 SR-flow network, since more than
8 channels are provided for the paired NCSN++ networks; Fourier embedding, FIR resampling, input and output
skip pyramids) and MERGES its results into the output file under the keys ncsnpp_mri_slices / ncsnpp_haar_80 (+ ``--suffix``), beside
the DDPM figures and without touching them.  ``--suffix _fused_stem`` is meant for a tuning build of the library run with
CSD_PP_WIDE_STEM=1 (the fused wide first layer in the NCSN++ plan; csrc/unet_layout.h): the A/B partner of the default plan, which keeps
the assemble pass + generic convolution.
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


_PP = dict(embedding_type='fourier', progressive='output_skip', progressive_input='input_skip')
SHAPES_PP = {
    'ncsnpp_mri_slices': dict(name='ncsnpp_paired', x_ch=16, y_ch=16, image_size=96, nf=128, ch_mult=(1, 1, 2, 2, 2), attn_resolutions=(24, 12, 6),
                              num_res_blocks=2, B=12),
    'ncsnpp_haar_80': dict(name='ncsnpp_paired', x_ch=9, y_ch=3, image_size=80, nf=128, ch_mult=(1, 1, 2, 2), attn_resolutions=(20, 10, 5),
                           num_res_blocks=2, B=64),
}


def make_ncsnpp(kw, precision):
    """(config, parameters) of an NCSN++ shape: oracle/cases.py make_ncsnpp_config plus the shapes and noise scales the samplers read"""
    from conditional_score_diffusion_amd.models import utils as mutils
    cx, cy, S = kw['x_ch'], kw['y_ch'], kw['image_size']
    cfg = cases.make_ncsnpp_config(name=kw['name'], nf=kw['nf'], ch_mult=kw['ch_mult'], num_res_blocks=kw['num_res_blocks'],
                                   attn_resolutions=kw['attn_resolutions'], image_size=S, channels=cx + cy, **_PP)
    d, m = cfg.data, cfg.model
    d.shape_x, d.shape_y = [cx, S, S], [cy if cy else cx, S, S]
    m.sigma_min_x = m.sigma_min = m.sigma_min_y = 5e-3
    m.sigma_max_x = m.sigma_max = float(np.sqrt(cx * S * S))
    m.sigma_max_y = 1.0
    m.output_channels = cx + cy
    m.csd_precision = precision
    cfg.sampling.snr = 0.15
    with torch.device('meta'):
        shapes = {k: tuple(v.shape) for k, v in mutils.create_model(cfg).state_dict().items()}
    return cfg, cases.ncsnpp_params(shapes, 0)


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
    pp = kw['name'].startswith('ncsnpp')
    dev = torch.device('cuda:0')
    if pp:
        cfg, params = make_ncsnpp(kw, args.precision)
    else:
        cfg = cases.make_config(**kw)
        cfg.model.csd_precision = args.precision
        params = so.synth_params(so.ddpm_param_shapes(so.NetCfg.from_config(cfg)), 0)
    model = mutils.create_model(cfg)
    model.load_state_dict(params)
    model = model.to(dev).eval()
    m, S, cx = cfg.model, cfg.data.image_size, kw['x_ch']
    paired = m.name not in ('ddpm', 'ncsnpp')
    cy = kw['y_ch'] if paired else 0
    rs = np.random.RandomState(0)
    x = torch.from_numpy((rs.standard_normal((B, cx, S, S)) * 5).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.uniform(0, 1, (B, cy, S, S)).astype(np.float32)).to(dev) if paired else None
    labels = torch.from_numpy(rs.uniform(1, 999, B).astype(np.float32)).to(dev)
    if pp and not paired:
        labels = torch.log(labels / 20.)       # (the unconditional Fourier network's label is log sigma)
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
    extra = {} if paired else {'unconditional_label': 'fourier' if pp else 'sigma'}

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
    stem = model.all_modules[3 if pp else 2]       # (behind the Fourier matrix and the two Linear layers / the two Linear layers)
    w = stem.weight.detach().contiguous()
    b = stem.bias.detach().contiguous()
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
    ap.add_argument('--family', default='ddpm', choices=('ddpm', 'ncsnpp'))
    ap.add_argument('--suffix', default='', help='appended to the shape keys (ncsnpp: _fused_stem for the tuning build\'s plan)')
    ap.add_argument('--shapes', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wide_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_wide.py needs the MI355X: there is no CPU path to time')
    table = SHAPES_PP if args.family == 'ncsnpp' else SHAPES
    out = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'pc_steps': args.pc_steps, 'shapes': {}}
    if os.path.exists(args.out):
        old = json.load(open(args.out))
        if args.family == 'ncsnpp':                # merge: the DDPM figures of the file stay as they are
            out = old
        else:                                      # (and a DDPM run keeps the NCSN++ entries of the file)
            out['shapes'].update({k: v for k, v in old.get('shapes', {}).items() if k.startswith('ncsnpp')})
    for tag in (args.shapes.split(',') if args.shapes else list(table)):
        out['shapes'][tag + args.suffix] = bench_shape(tag, table[tag], args)
        if args.family == 'ncsnpp':
            out['shapes'][tag + args.suffix].update(steps=args.steps, warmup=args.warmup, pc_steps=args.pc_steps)
    text = json.dumps(out, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
