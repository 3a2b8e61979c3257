"""Side bench of the direct Kx super-resolution networks (ddpm_KxSR; bench.py is the flagship's and is not involved).

    python tools/bench_kxsr.py [--steps 20] [--warmup 5] [--pc-steps 8] [--precision fp16x3] [--batch 64] [--out profiles/kxsr_bench.json]

One shape, random weights (score_oracle.synth_params), synthetic inputs: configs/ve/srflow/celebAHQ160/direct/8x.py - x 3 x 160^2,
y 3 x 20^2 (K = 8), nf 96, ch_mult (1, 1, 2, 2, 3, 3), attention at 20 / 10 / 5, two blocks per level, B = 64.  Reported:
  forward_ms              one evaluation of ddpm_KxSR on the low-resolution y (csd_unet_forward with y_scale: the upsample is computed in
                          the first layer's loads, the y output is downsampled behind the head)
  forward_preupsampled_ms the same weights as ddpm_paired on ops.bilinear_up(y, 8), 3 x 160^2 (no resampling anywhere) - the two are
                          timed in alternating windows; boundary_ms is their difference, the cost of the boundary
  first_layer_ms / first_layer_preupsampled_ms
                          the first layer alone (ops.input_conv, fused): y_scale = 8 on the low-resolution y against the plain layer
                          on the pre-upsampled y, alternating windows
  resample_ms             what the two resizes cost as launches of their own (ops.bilinear_up of y, ops.bilinear_down of a y output) -
                          the alternative the library boundary replaces on the input side
  pc_step_ms              one predictor-corrector step (two evaluations, the two-SDE VE pair, on-device noise) on the fused device loop
  pc_step_by_step_ms      the same step on the step-by-step loop (sampling/conditional.py's fallback, torch noise)
Windows as tools/bench_sr.py: `warmup` calls, then the median of three device-event windows of `steps` calls; the PC loops: one warm
run, then the median of three timed runs of `pc-steps` steps.  One JSON object, also printed.
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

SHAPE = dict(x_channels=3, y_channels=3, S=160, K=8, nf=96, ch_mult=(1, 1, 2, 2, 3, 3), attn_resolutions=(20, 10, 5), num_res_blocks=2, B=64)


def make_config(name, precision):
    k = SHAPE
    cx, cy, S = k['x_channels'], k['y_channels'], k['S']
    cfg = cases.make_config(name=name, nf=k['nf'], ch_mult=k['ch_mult'], num_res_blocks=k['num_res_blocks'],
                            attn_resolutions=k['attn_resolutions'], image_size=S, x_ch=cx, y_ch=cy)
    d, m = cfg.data, cfg.model
    m.input_channels = m.output_channels = cx + cy
    d.target_resolution, d.scale = S, k['K']
    m.sigma_max_y = float(np.sqrt(cy * S * S))
    m.csd_precision = precision
    return cfg


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


class StepByStep(torch.nn.Module):
    """the same network behind a class the fused loop does not know: the sampler then runs its step-by-step loop"""

    def __init__(self, net):
        super().__init__()
        self.net = net

    @property
    def device(self):
        return self.net.device

    def forward(self, x, labels):
        return self.net(x, labels)


def median3(fn):
    v = sorted(fn() for _ in range(3))
    return v[1], [v[0], v[2]]


def alternating(calls, warmup, steps):
    """{name: (median, [min, max])} of three windows per call, the calls taking turns"""
    for _ in range(warmup):
        for c in calls.values():
            c()
    rounds = {k: [] for k in calls}
    for _ in range(3):
        for k, c in calls.items():
            rounds[k].append(event_ms(c, steps))
    return {k: (sorted(v)[1], [min(v), max(v)]) for k, v in rounds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--pc-steps', type=int, default=8)
    ap.add_argument('--precision', default='fp16x3')
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kxsr_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_kxsr.py needs the MI355X: there is no CPU path to time')
    from conditional_score_diffusion_amd import ops, sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import conditional, fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    dev = torch.device('cuda:0')
    B = args.batch or SHAPE['B']
    cx, cy, S, K = SHAPE['x_channels'], SHAPE['y_channels'], SHAPE['S'], SHAPE['K']
    cfg = make_config('ddpm_KxSR', args.precision)
    p = so.synth_params(so.ddpm_param_shapes(so.NetCfg.from_config(cfg)), 0)
    nets = {}
    for name in ('ddpm_KxSR', 'ddpm_paired'):
        net = mutils.create_model(make_config(name, args.precision))
        net.load_state_dict(p)
        nets[name] = net.to(dev).eval()
    rs = np.random.RandomState(0)
    x = torch.from_numpy((rs.standard_normal((B, cx, S, S)) * 5).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.uniform(0, 1, (B, cy, S // K, S // K)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rs.uniform(1, 999, B).astype(np.float32)).to(dev)
    y_up = ops.bilinear_up(y, K)
    calls = {'ddpm_KxSR': lambda: nets['ddpm_KxSR']({'x': x, 'y': y}, labels), 'ddpm_paired': lambda: nets['ddpm_paired']({'x': x, 'y': y_up}, labels)}
    out = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'pc_steps': args.pc_steps,
           'precision': args.precision, 'batch': B, 'x': [cx, S, S], 'y': [cy, S // K, S // K], 'scale': K, 'nf': SHAPE['nf'],
           'ch_mult': list(SHAPE['ch_mult'])}
    w0, b0 = p['all_modules.2.weight'].to(dev), p['all_modules.2.bias'].to(dev)
    layer = {'kx': lambda: ops.input_conv(x, y, w0, b0, precision=args.precision, y_scale=K),
             'plain': lambda: ops.input_conv(x, y_up, w0, b0, precision=args.precision)}
    with torch.no_grad():
        a, r = calls['ddpm_KxSR'](), calls['ddpm_paired']()
        same = torch.equal(a['x'], r['x']) and torch.equal(a['y'], ops.bilinear_down(r['y'].contiguous(), K))
        same_layer = torch.equal(layer['kx'](), layer['plain']())
        fw = alternating(calls, args.warmup, args.steps)
        fl = alternating(layer, args.warmup, args.steps)
        ry = r['y'].contiguous()
        rs_ms, rs_spread = median3(lambda: event_ms(lambda: (ops.bilinear_up(y, K), ops.bilinear_down(ry, K)), args.steps))
    out['bitwise_equal_to_preupsampled'] = bool(same)
    out['first_layer_bitwise_equal_to_preupsampled'] = bool(same_layer)
    for src, k, key in ((fw, 'ddpm_KxSR', 'forward_ms'), (fw, 'ddpm_paired', 'forward_preupsampled_ms'), (fl, 'kx', 'first_layer_ms'),
                        (fl, 'plain', 'first_layer_preupsampled_ms')):
        out[key], out[key + '_spread'] = src[k]
    out['boundary_ms'] = out['forward_ms'] - out['forward_preupsampled_ms']
    out['resample_ms'], out['resample_ms_spread'] = rs_ms, rs_spread
    out['evaluations_per_s'] = 1e3 / out['forward_ms']
    out['samples_per_s'] = B * 1e3 / out['forward_ms']
    # PC sampling: conditional reverse diffusion + conditional Langevin on the two-SDE VE pair
    m = cfg.model
    sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
    P, C = get_predictor('conditional_reverse_diffusion'), get_corrector('conditional_langevin')
    net = nets['ddpm_KxSR']
    assert fused.fusable(net, sde, P, C, 1, False, True)
    sampler = conditional.get_pc_conditional_sampler(sde, (B, cx, S, S), P, C, snr=cfg.sampling.snr, p_steps=args.pc_steps, c_steps=1,
                                                     continuous=True, denoise=True, eps=1e-5)
    plain = StepByStep(net)
    assert not fused.fusable(plain, sde, P, C, 1, False, True)

    def timed(fn):
        def one():
            t0 = time.perf_counter()
            fn()                                   # (the fused loop's last call synchronises: the finiteness check)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.pc_steps
        fn()
        torch.cuda.synchronize()
        return median3(one)
    out['pc_step_ms'], out['pc_step_ms_spread'] = timed(lambda: sampler(net, y, seed=1))
    out['pc_step_by_step_ms'], out['pc_step_by_step_ms_spread'] = timed(lambda: sampler(plain, y))
    text = json.dumps(out, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
