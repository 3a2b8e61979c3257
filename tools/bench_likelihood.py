"""Side bench of the probability-flow likelihood (conditional_score_diffusion_amd/likelihood.py; not the driver's bench): SR3-160 CDE
at B = 64 and NCSN++ 256 x 256 at B = 8, random weights.  One JSON line per shape:

  rhs_ms            one fused right-hand-side evaluation (state upload, train forward, input-only backward, csd_pf_ode_rhs, download)
  rhs_vs_forward    rhs_ms / one inference forward (csd_unet_forward) at the same shape
  bwd_input_ms / bwd_full_ms   csd_unet_backward_ex(grads = NULL, d_x) against csd_unet_backward (every parameter gradient)
  nfe, s_per_image  one full likelihood (scipy RK45, rtol = atol = 1e-5, eps = 1e-5) of the batch

--device-loop adds the device-resident RK45 (ode_solver.py, csrc/ode_rk45.hip) beside scipy's host loop, same process, same inputs,
the two loops alternating --full-reps times (times are the mean, every run is listed):

  s_per_image_device_loop, nfe_device_loop, device_vs_host     the full likelihood with device_loop=True; ratio of the two times
  and one more line, 'ode sampler ncsnpp256' (get_ode_sampler, NCSN++ 256 x 256 VE, B = 8, rtol = atol = 1e-5, no denoising step):
  ms_per_evaluation / ms_per_evaluation_device_loop            wall time of a whole sample / nfe on each loop, beside forward_ms

  python tools/bench_likelihood.py [--shapes sr3,ncsnpp256] [--reps 5] [--no-full] [--rhs-only N] [--device-loop] [--full-reps 1]
--rhs-only N: N right-hand-side evaluations of SR3-160 and nothing else (the rocprofv3 kernel trace of DESIGN.md)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from conditional_score_diffusion_amd import likelihood, sde_lib  # noqa: E402
from conditional_score_diffusion_amd._lib import check, current_stream, lib, ptr  # noqa: E402
from conditional_score_diffusion_amd.config_dict import ConfigDict  # noqa: E402
from conditional_score_diffusion_amd.models import utils as mutils  # noqa: E402

dev = torch.device('cuda:0')


def build(cfg, precision):
    cfg.model.csd_precision = precision
    model = mutils.create_model(cfg)
    model.load_state_dict(bench.synth_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0))
    return model.to(dev).eval()


def sr3(precision):
    cfg = bench.sr3_160_config()
    m = cfg.model
    return build(cfg, precision), sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), True


def ncsnpp256(precision):
    from bench_other import ncsnpp_config
    c = ncsnpp_config('ncsnpp')
    S = 256
    c.data = ConfigDict(image_size=S, effective_image_size=S, centered=False, num_channels=3)
    c.model.nf, c.model.ch_mult, c.model.attn_resolutions, c.model.embedding_type = 128, (1, 1, 2, 2, 2, 2, 2), (16,), 'fourier'
    c.model.num_scales, c.model.sigma_max = 2000, 348.
    return build(c, precision), sde_lib.VESDE(0.01, 348., 2000), False


def inputs(model, B, seed=0):
    rs = np.random.RandomState(seed)
    S = model.image_size
    x = torch.from_numpy(rs.uniform(0, 1, size=(B, model.x_channels, S, S)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.uniform(0, 1, size=(B, model.y_channels, S, S)).astype(np.float32)).to(dev) if model.y_channels else None
    e = torch.from_numpy((rs.randint(0, 2, size=x.shape) * 2 - 1).astype(np.float32)).to(dev)
    return x, y, e


def forward_ms(model, x, y, lab, reps):
    with torch.no_grad():
        model({'x': x, 'y': y}, lab) if y is not None else model(x, lab)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            model({'x': x, 'y': y}, lab) if y is not None else model(x, lab)
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def backward_ms(model, x, y, lab, reps):
    """(input-only backward, full backward) in ms, each after its own csd_unet_train_forward (dropout 0)"""
    B, S = x.shape[0], model.image_size
    s = current_stream(dev)
    params = model._train_params()
    table = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
    ws = torch.empty(lib().csd_unet_train_workspace_bytes(model._h, B, 0.0), dtype=torch.uint8, device=dev)
    out = torch.empty(B, model.out_channels, S, S, device=dev)
    dout = torch.randn_like(out)
    dx = torch.empty_like(x)
    grads = [torch.empty_like(p) for p in params]
    gtable = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    res = {}
    for mode in ('input', 'full', 'input', 'full'):          # (the first pair warms up)
        tot = 0.0
        for r in range(reps):
            check(lib().csd_unet_train_forward(model._h, table, ptr(ws), ws.numel(), ptr(x), ptr(y), ptr(lab), ptr(out), B, 0.0, 0, 1, s),
                  'train_forward')
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if mode == 'input':
                check(lib().csd_unet_backward_ex(model._h, table, None, ptr(dx), ptr(ws), ws.numel(), ptr(dout), B, 1, s), 'backward_ex')
            else:
                check(lib().csd_unet_backward(model._h, table, gtable, ptr(ws), ws.numel(), ptr(dout), B, 1, s), 'backward')
            e1.record()
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1)
        res[mode] = tot / reps
    lib().csd_unet_train_release(model._h, ptr(ws))
    return res['input'], res['full']


def rhs_ms(model, sde, x, y, e, cond, reps):
    rhs = likelihood._FusedRHS(model, sde, x, y, e, cond)
    B = x.shape[0]
    state = np.concatenate([x.double().cpu().numpy().reshape(-1), np.zeros(B)])
    rhs(0.5, state)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(reps):
        rhs(0.5 + 0.01 * r, state)
    dt = (time.perf_counter() - t0) / reps * 1e3
    rhs.close()
    return dt


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def full_likelihood(r, model, sde, cond, x, y, e, device_loop, reps):
    """one full likelihood of the batch on the host loop and - device_loop - on the device loop, alternating"""
    B = x.shape[0]
    get = likelihood.get_conditional_likelihood_fn if cond else likelihood.get_likelihood_fn
    runs = {False: [], True: []}
    for _ in range(reps):
        for on_device in ((False, True) if device_loop else (False,)):
            fn = get(sde, lambda v: v, device_loop=True) if on_device else get(sde, lambda v: v)
            dt, (bpd, _, nfe) = timed(lambda: fn(model, x, y, epsilon=e) if cond else fn(model, x, epsilon=e))
            runs[on_device].append((dt / B, int(nfe), float(bpd.mean())))
    mean = lambda on_device: sum(t for t, _, _ in runs[on_device]) / len(runs[on_device])     # noqa: E731
    r['nfe'], r['s_per_image'], r['bpd_mean'] = runs[False][0][1], mean(False), runs[False][0][2]
    if device_loop:
        r['nfe_device_loop'], r['s_per_image_device_loop'], r['bpd_mean_device_loop'] = runs[True][0][1], mean(True), runs[True][0][2]
        r['device_vs_host'] = mean(True) / mean(False)
        r['s_per_image_runs'] = {'host': [t for t, _, _ in runs[False]], 'device_loop': [t for t, _, _ in runs[True]]}


def ode_sampler_line(precision, reps, full_reps):
    """get_ode_sampler on both loops at the NCSN++-256 shape (SR3-160 is conditional; the ODE sampler is unconditional)"""
    from conditional_score_diffusion_amd.sampling.unconditional import get_ode_sampler
    model, sde, _ = ncsnpp256(precision)
    B, S = 8, model.image_size
    shape = (B, model.x_channels, S, S)
    z = (torch.from_numpy(np.random.RandomState(1).standard_normal(shape).astype(np.float32)) * float(sde.sigma_max)).to(dev)
    lab = torch.full((B,), float(np.log(3.7)), device=dev)
    r = {'workload': 'ode sampler ncsnpp256', 'batch': B, 'precision': precision}
    r['forward_ms'] = forward_ms(model, z, None, lab, reps)
    runs = {False: [], True: []}
    for _ in range(full_reps):
        for on_device in (False, True):
            fn = get_ode_sampler(sde, shape, denoise=False, eps=1e-5, device_loop=on_device)
            dt, (x, nfe) = timed(lambda: fn(model, z=z))
            runs[on_device].append((dt * 1e3 / nfe, int(nfe), x))
    mean = lambda on_device: sum(t for t, _, _ in runs[on_device]) / len(runs[on_device])     # noqa: E731
    r['nfe'], r['ms_per_evaluation'] = runs[False][0][1], mean(False)
    r['nfe_device_loop'], r['ms_per_evaluation_device_loop'] = runs[True][0][1], mean(True)
    r['device_vs_host'] = mean(True) / mean(False)
    r['ms_per_evaluation_runs'] = {'host': [t for t, _, _ in runs[False]], 'device_loop': [t for t, _, _ in runs[True]]}
    xh, xd = runs[False][0][2], runs[True][0][2]
    r['sample_max_rel_diff'] = float((xh - xd).abs().max() / xh.abs().max())
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='sr3,ncsnpp256')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--precision', default='fp16x3')
    ap.add_argument('--no-full', action='store_true', help='skip the full likelihood (nfe, seconds per image)')
    ap.add_argument('--rhs-only', type=int, default=0, metavar='N')
    ap.add_argument('--device-loop', action='store_true', help='also time the device-resident RK45 loop, and the ODE sampler on both')
    ap.add_argument('--full-reps', type=int, default=1, help='runs of the full likelihood / the ODE sampler per loop')
    a = ap.parse_args()
    if a.rhs_only:
        model, sde, cond = sr3(a.precision)
        x, y, e = inputs(model, 64)
        rhs_ms(model, sde, x, y, e, cond, a.rhs_only)
        return
    for name in a.shapes.split(','):
        model, sde, cond = {'sr3': sr3, 'ncsnpp256': ncsnpp256}[name](a.precision)
        B = 64 if name == 'sr3' else 8
        x, y, e = inputs(model, B)
        lab = torch.full((B,), 500.0 if name == 'sr3' else float(np.log(3.7)), device=dev)
        r = {'workload': 'likelihood %s' % name, 'batch': B, 'precision': a.precision}
        r['forward_ms'] = forward_ms(model, x, y, lab, a.reps)
        r['rhs_ms'] = rhs_ms(model, sde, x, y, e, cond, a.reps)
        r['rhs_vs_forward'] = r['rhs_ms'] / r['forward_ms']
        r['bwd_input_ms'], r['bwd_full_ms'] = backward_ms(model, x, y, lab, a.reps)
        r['bwd_input_vs_full'] = r['bwd_input_ms'] / r['bwd_full_ms']
        if not a.no_full:
            full_likelihood(r, model, sde, cond, x, y, e, a.device_loop, a.full_reps)
        print(json.dumps(r), flush=True)
        del model
    if a.device_loop and not a.no_full:
        ode_sampler_line(a.precision, a.reps, a.full_reps)


if __name__ == '__main__':
    main()
