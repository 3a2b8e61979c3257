"""Side bench of NCSN++ with the 'residual' input pyramid at the CIFAR-10 shape (configs/ve/cifar10_ncsnpp_continuous.py: nf 128,
ch_mult (1, 2, 2, 2), 4 res blocks, attention at 16, Fourier embedding, FIR (1, 3, 3, 1), skip_rescale, 32 x 32, VE sigma 0.01 .. 50),
random weights, B = 128, fp16x3 (not the driver's bench).  One JSON line:

  forward_ms          one inference forward of the planned class (csd_unet_forward)
  forward_ops_ms      the same forward on the operator-granular class (ncsnpp_ops, same weights): the A/B yardstick
  pc_step_ms          one step of the fused PC loop (reverse diffusion + Langevin: 2 network evaluations), from the 3- and 13-step loops
  rhs_ms              one fused probability-flow right-hand side (state upload, train forward, input-only backward, csd_pf_ode_rhs)
  bwd_input_ms / bwd_full_ms   csd_unet_backward_ex(grads = NULL, d_x) against csd_unet_backward (every parameter gradient)

  python tools/bench_ncsnpp_cifar.py [--batch 128] [--reps 5] [--precision fp16x3]
  python tools/bench_ncsnpp_cifar.py --trace forward|rhs N    N evaluations after one warm-up, nothing else (the rocprofv3 runs of DESIGN.md)
  python tools/bench_ncsnpp_cifar.py --summarize KERNEL_TRACE.csv forward|rhs   split a rocprofv3 kernel trace per evaluation and report
                                                                                the pyramid kernels' share of the last one"""
import argparse
import collections
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def cifar_config(name='ncsnpp'):
    from conditional_score_diffusion_amd.config_dict import ConfigDict
    c = ConfigDict()
    c.training = ConfigDict(continuous=True, sde='vesde', likelihood_weighting=False, reduce_mean=False)
    c.sampling = ConfigDict(method='pc', predictor='reverse_diffusion', corrector='langevin', n_steps_each=1, noise_removal=True,
                            probability_flow=False, snr=0.16)
    c.data = ConfigDict(image_size=32, effective_image_size=32, centered=False, num_channels=3)
    c.model = ConfigDict(name=name, nf=128, ch_mult=(1, 2, 2, 2), num_res_blocks=4, attn_resolutions=(16,), dropout=0.1,
                         resamp_with_conv=True, conditional=True, nonlinearity='swish', num_scales=1000, sigma_min=0.01, sigma_max=50.,
                         fir=True, fir_kernel=[1, 3, 3, 1], skip_rescale=True, resblock_type='biggan', progressive='none',
                         progressive_input='residual', progressive_combine='sum', attention_type='ddpm', init_scale=0.,
                         embedding_type='fourier', fourier_scale=16, conv_size=3, scale_by_sigma=True)
    return c


# marker kernel of one evaluation in a kernel trace: the input assembly of the inference plan, the state conversion of an RHS
MARKERS = {'forward': 'assemble', 'rhs': 'pf_state_kernel'}


def summarize(path, mode):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    evals, cur = [], None
    for r in rows:
        name = r['Kernel_Name']
        if MARKERS[mode] in name:
            cur = []
            evals.append(cur)
        if cur is not None:
            cur.append((name, int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
    out = {'mode': mode, 'evaluations': len(evals)}
    if not evals:
        return out
    last = evals[-1]
    total = sum(d for _, d in last)
    pyr = collections.OrderedDict()
    for name, d in last:
        if 'fir_pyr' in name:
            key = name.split('(')[0].replace('void ', '')
            pyr.setdefault(key, []).append(d / 1e3)
    pyr_total = sum(sum(v) for v in pyr.values()) * 1e3
    out.update(kernels=len(last), kernel_time_ms=total / 1e6, pyramid_share=pyr_total / total,
               pyramid_launches_us={k: [round(x, 1) for x in v] for k, v in pyr.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--precision', default='fp16x3')
    ap.add_argument('--trace', nargs=2, metavar=('MODE', 'N'))
    ap.add_argument('--summarize', nargs=2, metavar=('CSV', 'MODE'))
    a = ap.parse_args()
    if a.summarize:
        print(json.dumps(summarize(a.summarize[0], a.summarize[1])))
        return
    import numpy as np
    import torch
    import bench
    import bench_likelihood as bl
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import fused
    dev = torch.device('cuda:0')
    B = a.batch

    def build(name):
        cfg = cifar_config(name)
        cfg.model.csd_precision = a.precision
        m = mutils.create_model(cfg)
        m.load_state_dict(bench.synth_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, 0))
        return m.to(dev).eval()

    model = build('ncsnpp')
    sde = sde_lib.VESDE(0.01, 50., 1000)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, size=(B, 3, 32, 32)).astype(np.float32)).to(dev)
    e = torch.from_numpy((rs.randint(0, 2, size=x.shape) * 2 - 1).astype(np.float32)).to(dev)
    lab = torch.from_numpy(np.log(rs.uniform(0.01, 50., size=B)).astype(np.float32)).to(dev)
    if a.trace:
        mode, n = a.trace[0], int(a.trace[1])
        if mode == 'forward':
            with torch.no_grad():
                for _ in range(n + 1):
                    model(x, lab)
        else:
            bl.rhs_ms(model, sde, x, None, e, False, n)
        torch.cuda.synchronize()
        return
    r = {'workload': 'NCSN++ CIFAR-10 (cifar10_ncsnpp_continuous: residual input pyramid), 32x32', 'batch': B, 'precision': a.precision}
    r['forward_ms'] = bl.forward_ms(model, x, None, lab, a.reps)
    ops = build('ncsnpp_ops')
    r['forward_ops_ms'] = bl.forward_ms(ops, x, None, lab, a.reps)
    r['planned_speedup_vs_ops'] = r['forward_ops_ms'] / r['forward_ms']
    del ops
    t = {}
    for n in (3, 13, 3, 13):                         # (the first pair warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fused.run(model, sde, (B, 3, 32, 32), None, n, 0.16, 1e-5, True, seed=1)
        torch.cuda.synchronize()
        t[n] = time.perf_counter() - t0
    r['pc_step_ms'] = (t[13] - t[3]) / 10 * 1e3
    r['rhs_ms'] = bl.rhs_ms(model, sde, x, None, e, False, a.reps)
    r['bwd_input_ms'], r['bwd_full_ms'] = bl.backward_ms(model, x, None, lab, a.reps)
    print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
