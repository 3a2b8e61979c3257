"""Side bench of the 2x super-resolution networks (ddpm_2xSR; bench.py is the flagship's and is not involved).

    python tools/bench_sr.py [--steps 20] [--warmup 5] [--pc-steps 8] [--precision fp16x3] [--batch 64] [--out profiles/sr_bench.json]

One shape, random weights (score_oracle.synth_params), synthetic inputs: the last stage of the 40 -> 80 -> 160 cascade
(configs/ve/srflow/celebAHQ160/sequential/bicubic/config_160.py: x 3 x 160^2, y 3 x 80^2, the network on 12 + 3 channels at 80^2,
attention at 20 / 10 / 5, two blocks per level) at nf 96, ch_mult (1, 1, 2, 2), B = 64.  Reported:
  forward_ms            one evaluation of ddpm_2xSR on the image x (csd_unet_forward with x_squeeze: the squeeze is addressing in the
                        first layer's loads and the head's stores)
  forward_presqueezed_ms  the same weights as ddpm_paired on x already squeezed to 12 x 80^2 (no squeeze anywhere) - the two are timed
                        in alternating windows; boundary_ms is their difference, the cost of the boundary
  torch_squeeze_ms      what the two permute copies (squeeze of x, unsqueeze of the x output) cost in torch - the alternative the
                        library boundary replaces
  pc_step_ms            one predictor-corrector step (two evaluations, the two-SDE VE pair, on-device noise) on the fused device loop
  pc_step_by_step_ms    the same step on the step-by-step loop (sampling/conditional.py's fallback, torch noise)
``--family ncsnpp`` runs the same stage on ncsnpp_2xSR / ncsnpp_paired (Fourier embedding, FIR resampling, input and output skip
pyramids) and MERGES its result into the output file under the key ``ncsnpp_2xSR``, beside the DDPM figures and without touching them.
Windows as tools/bench_wide.py: `warmup` calls, then the median of three device-event windows of `steps` calls; the PC loops: one warm
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

SHAPE = dict(image_channels=3, y_channels=3, S=80, nf=96, ch_mult=(1, 1, 2, 2), attn_resolutions=(20, 10, 5), num_res_blocks=2, B=64)


def make_config(name, precision):
    k = SHAPE
    cx, cy, S = k['image_channels'], k['y_channels'], k['S']
    if name.startswith('ncsnpp'):
        cfg = cases.make_ncsnpp_config(name=name, nf=k['nf'], ch_mult=k['ch_mult'], num_res_blocks=k['num_res_blocks'],
                                       attn_resolutions=k['attn_resolutions'], image_size=S, channels=4 * cx + cy)
        d, m = cfg.data, cfg.model
        d.shape_x, d.shape_y = [4 * cx, S, S], [cy, S, S]
        if name == 'ncsnpp_2xSR':
            d.image_size, d.effective_image_size = 2 * S, S
            d.shape_x = [cx, 2 * S, 2 * S]
        m.sigma_min_x = m.sigma_min = m.sigma_min_y = 5e-3
        m.sigma_max_x = m.sigma_max = float(np.sqrt(4 * cx * S * S))
        m.sigma_max_y = float(np.sqrt(cy * S * S))
        m.csd_precision = precision
        cfg.sampling.snr = 0.15
        cfg.sampling.predictor, cfg.sampling.corrector = 'conditional_reverse_diffusion', 'conditional_langevin'
        return cfg
    cfg = cases.make_config(name=name, nf=k['nf'], ch_mult=k['ch_mult'], num_res_blocks=k['num_res_blocks'],
                            attn_resolutions=k['attn_resolutions'], image_size=S, x_ch=4 * cx, y_ch=cy)
    d, m = cfg.data, cfg.model
    d.num_channels = 4 * cx + cy
    m.input_channels = m.output_channels = d.num_channels
    if name == 'ddpm_2xSR':
        d.image_size, d.effective_image_size = 2 * S, S
        d.shape_x, d.shape_y = [cx, 2 * S, 2 * S], [cy, S, S]
    m.sigma_max_x = m.sigma_max = float(np.sqrt(4 * cx * S * S))
    m.sigma_max_y = float(np.sqrt(cy * S * S))
    m.csd_precision = precision
    return cfg


def squeeze(x):
    Bq, C, H, W = x.shape
    return x.reshape(Bq, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(Bq, 4 * C, H // 2, W // 2)


def unsqueeze(z):
    Bq, C4, H, W = z.shape
    return z.reshape(Bq, C4 // 4, 2, 2, H, W).permute(0, 1, 4, 2, 5, 3).reshape(Bq, C4 // 4, 2 * H, 2 * W)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--pc-steps', type=int, default=8)
    ap.add_argument('--precision', default='fp16x3')
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--family', default='ddpm', choices=('ddpm', 'ncsnpp'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sr_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sr.py needs the MI355X: there is no CPU path to time')
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import conditional, fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    dev = torch.device('cuda:0')
    B = args.batch or SHAPE['B']
    cx, cy, S = SHAPE['image_channels'], SHAPE['y_channels'], SHAPE['S']
    pp = args.family == 'ncsnpp'
    sq_name, plain_name = ('ncsnpp_2xSR', 'ncsnpp_paired') if pp else ('ddpm_2xSR', 'ddpm_paired')
    cfg = make_config(sq_name, args.precision)
    if pp:
        with torch.device('meta'):
            shapes = {k: tuple(v.shape) for k, v in mutils.create_model(cfg).state_dict().items()}
        p = cases.ncsnpp_params(shapes, 0)
    else:
        p = so.synth_params(so.ddpm_param_shapes(so.NetCfg.from_config(cfg)), 0)
    nets = {}
    for name, key in ((sq_name, 'ddpm_2xSR'), (plain_name, 'ddpm_paired')):      # (keys: the roles, named after the DDPM pair)
        net = mutils.create_model(make_config(name, args.precision))
        net.load_state_dict(p)
        nets[key] = net.to(dev).eval()
    rs = np.random.RandomState(0)
    x = torch.from_numpy((rs.standard_normal((B, cx, 2 * S, 2 * S)) * 5).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.uniform(0, 1, (B, cy, S, S)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rs.uniform(1, 999, B).astype(np.float32)).to(dev)
    xs = squeeze(x).contiguous()
    calls = {'ddpm_2xSR': lambda: nets['ddpm_2xSR']({'x': x, 'y': y}, labels), 'ddpm_paired': lambda: nets['ddpm_paired']({'x': xs, 'y': y}, labels)}
    out = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'pc_steps': args.pc_steps,
           'precision': args.precision, 'batch': B, 'image_x': [cx, 2 * S, 2 * S], 'network': [4 * cx + cy, S, S], 'nf': SHAPE['nf'],
           'ch_mult': list(SHAPE['ch_mult'])}
    with torch.no_grad():
        same = torch.equal(calls['ddpm_2xSR']()['x'], unsqueeze(calls['ddpm_paired']()['x']))
        for _ in range(args.warmup):
            for c in calls.values():
                c()
        rounds = {k: [] for k in calls}
        for _ in range(3):                                   # alternating windows
            for k, c in calls.items():
                rounds[k].append(event_ms(c, args.steps))
        torch_ms, torch_spread = median3(lambda: event_ms(lambda: (squeeze(x).contiguous(), unsqueeze(xs).contiguous()), args.steps))
    out['bitwise_equal_to_presqueezed'] = bool(same)
    for k, key in (('ddpm_2xSR', 'forward_ms'), ('ddpm_paired', 'forward_presqueezed_ms')):
        v = sorted(rounds[k])
        out[key], out[key + '_spread'] = v[1], [v[0], v[2]]
    out['boundary_ms'] = out['forward_ms'] - out['forward_presqueezed_ms']
    out['torch_squeeze_ms'], out['torch_squeeze_ms_spread'] = torch_ms, torch_spread
    out['evaluations_per_s'] = 1e3 / out['forward_ms']
    out['samples_per_s'] = B * 1e3 / out['forward_ms']
    # PC sampling: conditional reverse diffusion + conditional Langevin on the two-SDE VE pair
    m = cfg.model
    sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
    P, C = get_predictor('conditional_reverse_diffusion'), get_corrector('conditional_langevin')
    net = nets['ddpm_2xSR']
    assert fused.fusable(net, sde, P, C, 1, False, True)
    shape = (B, cx, 2 * S, 2 * S)
    sampler = conditional.get_pc_conditional_sampler(sde, shape, P, C, snr=cfg.sampling.snr, p_steps=args.pc_steps, c_steps=1, continuous=True,
                                                     denoise=True, eps=1e-5)
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
    if pp:                                         # merge: the DDPM figures of the file stay as they are
        out['model'] = sq_name
        whole = json.load(open(args.out)) if os.path.exists(args.out) else {}
        whole['ncsnpp_2xSR'] = out
        out = whole
    elif os.path.exists(args.out):                 # (and a DDPM run keeps the NCSN++ entry of the file)
        old = json.load(open(args.out))
        if 'ncsnpp_2xSR' in old:
            out['ncsnpp_2xSR'] = old['ncsnpp_2xSR']
    text = json.dumps(out, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
