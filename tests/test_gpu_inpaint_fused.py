"""-m gpu: PC inpainting on the fused device loop (csd_pc_inpaint_sample, inpaint_blend_kernel).  The loop against the reference's own
inpainting runs (tests/golden/inpaint.npz, tests/golden/inpaint_runs.npz from tools/make_inpaint_goldens.py) and against the project's
predictor / corrector classes driven step by step with the reference's blend in plain torch; the blend kernel alone; the on-device
noise; the step-wise global-norm form; recording; and the Philox fill restated in numpy."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from test_gpu_network import build, dev, rel  # noqa: E402
from test_gpu_steps import _Tape  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
N, EPS, SNR = 6, 1e-3, 0.075                              # tools/make_inpaint_goldens.py
VP_KW = dict(beta_min=0.1, beta_max=5.)                   # (beta_max / N < 1 at N = 6)

_MODELS = {}


def model_for(precision='fp32'):
    if precision not in _MODELS:
        _MODELS[precision] = build('uncond_tiny', precision)
    return _MODELS[precision]


def make_sde(scls, cfg, n=N, full=False):
    """the SDEs of tools/make_inpaint_goldens.py; full: the usual 1000-step schedules (run for a few steps through fused.run)"""
    from conditional_score_diffusion_amd import sde_lib
    if scls == 'VESDE':
        return sde_lib.VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, 1000 if full else n)
    if full:
        return getattr(sde_lib, scls)(0.1, 20., 1000)
    return getattr(sde_lib, scls)(VP_KW['beta_min'], VP_KW['beta_max'], n)


def inpainter(sde, pred, corr, snr=SNR, eps=EPS, continuous=True, pf=False, denoise=True):
    from conditional_score_diffusion_amd.sampling import unconditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    return unconditional.get_pc_inpainter(sde, get_predictor(pred), get_corrector(corr), snr=snr, n_steps=1, probability_flow=pf,
                                          continuous=continuous, denoise=denoise, eps=eps, device_loop=True)


def inputs():
    cfg, B, data, mask, tape = cases.inpaint_case()
    return cfg, B, data, mask, tape


def run_tape(n_phases, n=N, seed=42):
    cfg, B, data, mask, _ = inputs()
    return cases.tape([tuple(data.shape)] * (1 + (n_phases + 2) * n), seed)


# ---- 1. the reference's own 12-step VE run (oracle/make_goldens.py:gen_inpaint) ---------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_device_loop_vs_the_reference_run(precision):
    """tests/golden/inpaint.npz: VESDE, N = 12, reverse diffusion / Langevin, snr 0.15, eps 1e-5, denoise, half-image mask"""
    from conditional_score_diffusion_amd import sde_lib
    g = np.load(os.path.join(GOLD, 'inpaint.npz'))
    cfg, B, data, mask, tape = inputs()
    _, _, _, model = model_for(precision)
    sde = sde_lib.VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, 12)
    fn = inpainter(sde, 'reverse_diffusion', 'langevin', snr=0.15, eps=1e-5)
    x, info = fn(model, data.to(dev()), mask.to(dev()), noise_tape=tape)
    assert info == {}
    x = x.cpu()
    err = float(np.abs(x.numpy() - g['x']).max())
    print('inpaint.npz %s: max abs err %.3e (sigma_max %.2f), relative to max(|ref|, 1) %.3e' % (
        precision, err, cfg.model.sigma_max_x, rel(x.numpy(), g['x'], floor=1.0)))
    assert float(((x - data) * mask).abs().max()) == 0.0           # a 0/1 mask returns the known pixels exactly
    if precision == 'fp32':
        assert err <= 2e-4 * float(cfg.model.sigma_max_x)          # the bound of test_gpu_steps.py::test_pc_inpainter_vs_reference
    else:
        assert rel(x.numpy(), g['x'], floor=1.0) < 1e-3            # the project's contract


# ---- 2. the reference's VP / sub-VP / channel-mask runs -------------------------------------------------------------------------------
RUNS = [            # tools/make_inpaint_goldens.py:RUNS
    ('vp_rd_lang_c', 'VPSDE', 'reverse_diffusion', 'langevin', True, False),
    ('vp_rd_lang_d', 'VPSDE', 'reverse_diffusion', 'langevin', False, False),
    ('vp_anc_none_d', 'VPSDE', 'ancestral_sampling', 'none', False, False),
    ('subvp_rd_none', 'subVPSDE', 'reverse_diffusion', 'none', True, False),
    ('ve_rd_none', 'VESDE', 'reverse_diffusion', 'none', True, False),
    ('ve_rd_lang_chmask', 'VESDE', 'reverse_diffusion', 'langevin', True, True),
]


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('name,scls,pred,corr,continuous,chmask', RUNS)
def test_device_loop_vs_reference_runs(name, scls, pred, corr, continuous, chmask, precision):
    from conditional_score_diffusion_amd.sampling import fused
    g = np.load(os.path.join(GOLD, 'inpaint_runs.npz'))
    cfg, B, data, mask, _ = inputs()
    _, _, _, model = model_for(precision)
    sde = make_sde(scls, cfg)
    if chmask:
        mask = torch.tensor([1., 0., 0.]).reshape(1, 3, 1, 1)      # the Haar multi-scale model's mask: broadcast on the host
    tape = run_tape((pred != 'none') + (corr != 'none'))
    x, _ = inpainter(sde, pred, corr, continuous=continuous)(model, data.to(dev()), mask.to(dev()), noise_tape=tape)
    x = x.cpu().numpy()
    err = rel(x, g['run_' + name], floor=1.0)
    print('%s %s: device loop vs the reference run %.3e (max |ref| %.1f)' % (name, precision, err, np.abs(g['run_' + name]).max()))
    assert err < 1e-3                                              # the project's contract
    if precision == 'fp32':
        assert err < 2e-4                                          # what test_gpu_vp_sampling.py holds its fp32 tiny trajectories to
    ms, _ = fused.inpaint_tables(sde, torch.linspace(sde.T, EPS, N))
    known = np.broadcast_to(mask.numpy(), x.shape) == 1
    want = np.float32(ms[-1].item()) * data.numpy()
    assert np.array_equal(x[known].view(np.uint32), want[known].view(np.uint32))      # denoise: the known pixels are m(t_last) * data


# ---- 3. against the step-by-step classes with the reference's blend in torch -------------------------------------------------------------
LOOP_CASES = [      # SDE class, predictor, corrector, continuous, probability_flow
    ('VESDE', 'reverse_diffusion', 'langevin', True, False),
    ('VESDE', 'euler_maruyama', 'ald', True, False),
    ('VESDE', 'reverse_diffusion', 'none', True, True),
    ('VPSDE', 'reverse_diffusion', 'langevin', True, False),
    ('VPSDE', 'ancestral_sampling', 'none', False, False),
    ('subVPSDE', 'euler_maruyama', 'none', True, False),
]


@pytest.mark.parametrize('scls,pred_name,corr_name,continuous,pf', LOOP_CASES)
def test_device_loop_matches_the_step_by_step_classes(scls, pred_name, corr_name, continuous, pf):
    """4 steps of the 1000-step schedules.  The blend here is plain torch, in the order of operations of sampling/unconditional.py:268-271."""
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    n = 4
    cfg, B, data, mask, _ = inputs()
    _, _, _, model = model_for()
    sde = make_sde(scls, cfg, full=True)
    P, C = get_predictor(pred_name), get_corrector(corr_name)
    assert fused.fusable(model, sde, P, C, 1, pf, continuous)
    phases = (pred_name != 'none') + (corr_name != 'none')
    tape = run_tape(phases, n, seed=17)
    assert len(tape) == fused.inpaint_tape_length(n, corr_name != 'none', pred_name != 'none')
    x_f, _, _ = fused.run(model, sde, tuple(data.shape), None, n, SNR, EPS, True, noise_tape=tape, unconditional_label='sigma',
                          predictor=P, corrector=C, probability_flow=pf, continuous=continuous, inpaint=(data, mask))
    sfn = mutils.get_score_fn(sde, model, conditional=False, continuous=continuous)
    data_d, mask_d = data.to(dev()), mask.to(dev())
    with _Tape(tape[1:]) as tp:
        pred, corr = P(sde, sfn, pf), C(sde, sfn, SNR, 1)
        prior = (tape[0] * (sde.sigma_max if scls == 'VESDE' else 1.0)).to(dev())
        x = data_d * mask_d + prior * (1. - mask_d)
        ts = torch.linspace(sde.T, EPS, n)
        for i in range(n):
            vec_t = torch.ones(B, device=dev()) * ts[i]
            for obj in (corr, pred):
                x, x_mean = obj.update_fn(x, vec_t)
                mean, std = sde.marginal_prob(data_d, vec_t)
                noisy = mean + torch.randn_like(x) * std[:, None, None, None]
                x = x * (1. - mask_d) + noisy * mask_d
                x_mean = x * (1. - mask_d) + mean * mask_d          # (from the new x)
        assert tp.i == len(tape) - 1                       # both sides consumed the same number of draws
    assert torch.isfinite(x_f).all()
    err = rel(x_mean.cpu().numpy(), x_f.cpu().numpy(), floor=1.0)
    print('%s %s/%s: device loop vs step by step %.3e' % (scls, pred_name, corr_name, err))
    assert err < 1e-5                                      # the bound of test_fused_loop_matches_the_step_by_step_classes


# ---- 4. the kernel alone --------------------------------------------------------------------------------------------------------------
def _offset_view(t, offset):
    """the same values on the device, at a 16-byte aligned address or one float behind it"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _blend_ref(x, data, mask, z, m, std):
    """the four expressions of sampling/unconditional.py:268-271 in fp32 torch on the host"""
    m, std = torch.tensor(m, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    masked_mean = m * data
    masked = masked_mean + std * z
    x = x * (1. - mask) + masked * mask
    x_mean = x * (1. - mask) + masked_mean * mask
    return x, x_mean


@pytest.mark.parametrize('shape', [(1, 3, 5, 5), (2, 3, 16, 16)])      # 75 elements: a scalar tail; 1536: two blocks of float4 groups
@pytest.mark.parametrize('offset', [0, 1])                            # 1: every tensor one float off 16-byte alignment
@pytest.mark.parametrize('soft', [False, True])
def test_blend_kernel_vs_torch(shape, offset, soft):
    from conditional_score_diffusion_amd import ops
    g = torch.Generator().manual_seed(5 + offset)
    x0 = torch.randn(shape, generator=g) * 30.
    data = torch.rand(shape, generator=g)
    z = torch.randn(shape, generator=g)
    mask = torch.rand(shape, generator=g) if soft else (torch.rand(shape, generator=g) < 0.5).float()
    m, std = 0.8125 + 1e-3, 3.7
    ulp2 = 2 * float(np.finfo(np.float32).eps) * max(float(x0.abs().max()), float((std * z).abs().max()), 1.0)
    for use_mean in (True, False):
        for sd in (std, 0.0):
            xr, xmr = _blend_ref(x0, data, mask, z, m, sd)
            x, xm = ops.inpaint_blend(_offset_view(x0, offset), _offset_view(data, offset), _offset_view(mask, offset),
                                      _offset_view(z, offset), m, sd, x_mean=use_mean)
            assert x.data_ptr() % 16 == 4 * offset
            assert float((x.cpu() - xr).abs().max()) <= ulp2
            assert (xm is None) == (not use_mean)
            if use_mean:
                assert float((xm.cpu() - xmr).abs().max()) <= ulp2
            if not soft:
                known = mask == 1
                assert torch.equal(x.cpu()[known], (xr)[known])
    # std = 0 without a tensor draws nothing: masked = masked_mean (the initial state prior*(1 - mask) + data*mask)
    x, _ = ops.inpaint_blend(_offset_view(x0, offset), _offset_view(data, offset), _offset_view(mask, offset), None, 1.0, 0.0,
                             x_mean=False)
    assert float((x.cpu() - (x0 * (1. - mask) + data * mask)).abs().max()) <= ulp2


@pytest.mark.parametrize('shape', [(1, 3, 5, 5), (2, 3, 16, 16)])
@pytest.mark.parametrize('offset', [0, 1])
def test_blend_kernel_philox_equals_the_randn_fill(shape, offset):
    """z = None: the normals made in registers are the bits of ops.randn(shape, seed, stream)"""
    from conditional_score_diffusion_amd import ops
    g = torch.Generator().manual_seed(9)
    x0, data = (torch.randn(shape, generator=g) * 30.).to(dev()), torch.rand(shape, generator=g).to(dev())
    mask = (torch.rand(shape, generator=g) < 0.5).float().to(dev())
    for seed, stream in ((7, 3), (2 ** 40 + 11, 2 ** 33 + 5)):
        z = ops.randn(shape, seed, stream, dev())
        a, am = ops.inpaint_blend(_offset_view(x0, offset), _offset_view(data, offset), _offset_view(mask, offset), z, 0.9, 2.5)
        b, bm = ops.inpaint_blend(_offset_view(x0, offset), _offset_view(data, offset), _offset_view(mask, offset), None, 0.9, 2.5,
                                  seed=seed, stream_id=stream)
        assert torch.equal(a, b) and torch.equal(am, bm)
        assert float((a - x0).abs().max()) > 0.1


# ---- 5. the whole loop on the on-device noise ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scls,pred,corr', [('VESDE', 'reverse_diffusion', 'langevin'), ('VPSDE', 'reverse_diffusion', 'langevin'),
                                            ('subVPSDE', 'euler_maruyama', 'none')])
def test_seed_equals_the_tape_of_its_streams(scls, pred, corr):
    """stream 0 is the prior (times sigma_max for VE, which fused.run applies to the tape's standard normal as well); draw k of step i
    is stream 1 + i*draws_per_step + k in the order [z_corrector] z_blend [z_predictor] z_blend (include/csd.h)"""
    from conditional_score_diffusion_amd import ops
    cfg, B, data, mask, _ = inputs()
    _, _, _, model = model_for()
    sde = make_sde(scls, cfg)
    fn = inpainter(sde, pred, corr)
    data_d, mask_d = data.to(dev()), mask.to(dev())
    a, _ = fn(model, data_d, mask_d, seed=5)
    b, _ = fn(model, data_d, mask_d, seed=5)
    c, _ = fn(model, data_d, mask_d, seed=6)
    draws = (pred != 'none') + (corr != 'none') + 2
    tape = [ops.randn(tuple(data.shape), 5, k, dev()) for k in range(1 + draws * N)]
    d, _ = fn(model, data_d, mask_d, noise_tape=tape)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(a, d)
    assert (a - c).abs().max().item() > 1e-2               # another key: another prior and other noise


# ---- 6. the step-wise global-norm form ----------------------------------------------------------------------------------------------------
def test_step_forms_reproduce_the_one_call_form():
    """csd_pc_inpaint_step_begin / _step_end with global_batch == B and no exchange ARE csd_pc_inpaint_sample: 1e-6 of the prior's
    scale, 1 for the VP SDE (the bound of test_gpu_vp_sampling.py::test_step_begin_end_reproduce_pc_sample_for_vp_langevin)"""
    cfg, B, data, mask, _ = inputs()
    _, _, _, model = model_for()
    fn = inpainter(make_sde('VPSDE', cfg), 'reverse_diffusion', 'langevin')
    tape = run_tape(2, seed=91)
    a, _ = fn(model, data.to(dev()), mask.to(dev()), noise_tape=tape)
    b, _ = fn(model, data.to(dev()), mask.to(dev()), noise_tape=tape, global_norm=(lambda s: None, B))
    err = np.abs(a.cpu().numpy() - b.cpu().numpy()).max() / 1.0
    print('inpaint step_begin/step_end vs one call (VP): %.3e, max |x| %.2f' % (err, a.abs().max().item()))
    assert torch.isfinite(a).all() and err < 1e-6


# ---- 7. recording ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scls,pred,corr', [('VESDE', 'reverse_diffusion', 'langevin'), ('VPSDE', 'reverse_diffusion', 'none')])
def test_show_evolution_records_the_initial_state_and_every_step(scls, pred, corr):
    from conditional_score_diffusion_amd.sampling import fused
    cfg, B, data, mask, _ = inputs()
    _, _, _, model = model_for()
    sde = make_sde(scls, cfg)
    draws = (pred != 'none') + (corr != 'none') + 2
    tape = run_tape(draws - 2, seed=3)
    x, info = inpainter(sde, pred, corr, denoise=False)(model, data.to(dev()), mask.to(dev()), show_evolution=True, noise_tape=tape)
    ev = info['evolution']
    assert tuple(ev.shape) == (N + 1,) + tuple(data.shape) and ev.device.type == 'cpu'
    prior = tape[0] * (sde.sigma_max if scls == 'VESDE' else 1.0)
    assert torch.equal(ev[0], prior * (1. - mask) + data * mask)
    assert torch.equal(ev[-1], x.cpu())                              # (denoise off: the last recorded state is the result)
    ms, sd = fused.inpaint_tables(sde, torch.linspace(sde.T, EPS, N))
    known = mask == 1
    for i in range(N):
        z = tape[1 + i * draws + draws - 1]                          # the blend draw behind the predictor: the step's last
        want = ms[i] * data + sd[i] * z                              # fp32, the kernel's order of operations
        assert torch.equal(ev[i + 1][known], want[known]), i


def test_non_finite_data_raises():
    """the finiteness contract of the device loop holds for the inpainter: an Inf among the known pixels is reported, not returned"""
    from conditional_score_diffusion_amd._lib import NonFiniteError
    cfg, B, data, mask, _ = inputs()
    _, _, _, model = model_for()
    bad = data.clone()
    bad[0, 0, 0, 0] = float('inf')
    with pytest.raises(NonFiniteError):
        inpainter(make_sde('VESDE', cfg), 'reverse_diffusion', 'none')(model, bad.to(dev()), mask.to(dev()), seed=1)


# ---- 8. randn_kernel after sharing its body with the blend ------------------------------------------------------------------------------------
def _philox_uniform_bits(n4, seed, stream):
    """Philox4x32-10: counter (i, stream), key seed -> four 32-bit words per counter"""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    mask32 = np.uint64(0xFFFFFFFF)
    i = np.arange(n4, dtype=np.uint64)
    c = [i & mask32, i >> np.uint64(32), np.full(n4, stream & 0xFFFFFFFF, np.uint64), np.full(n4, stream >> 32, np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask32, (k1 + np.uint64(0xBB67AE85)) & mask32
    return c


def _randn_numpy(n, seed, stream):
    """csd_randn restated: element e = lane e % 4 of counter e / 4; uniforms from the top 24 bits (exact in fp32), Box-Muller with the
    angle rounded to fp32 as the kernel rounds it, everything else in fp64"""
    c = _philox_uniform_bits((n + 3) // 4, seed, stream)
    top = [(w >> np.uint64(8)).astype(np.float64) for w in c]
    u0, u1, u2, u3 = (top[0] + 1.0) / 2 ** 24, (top[1] + 0.5) / 2 ** 24, (top[2] + 1.0) / 2 ** 24, (top[3] + 0.5) / 2 ** 24
    two_pi = np.float32(6.283185307179586)
    a0 = (two_pi * u1.astype(np.float32)).astype(np.float64)
    a1 = (two_pi * u3.astype(np.float32)).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1).reshape(-1)[:n]


@pytest.mark.parametrize('n', [75, 4096])
@pytest.mark.parametrize('seed,stream', [(42, 7), (2 ** 40 + 11, 2 ** 33 + 5)])
def test_randn_fill_is_philox_box_muller(n, seed, stream):
    """No earlier test pins the values of ops.randn (test_gpu_ops.py checks moments and determinism).  The counters, the key schedule
    and the uniforms are integer / exact in fp32; the bound covers the device's logf, sqrtf and sincosf only: r <= sqrt(-2 ln 2^-24)
    = 5.77, r carries <= 2.25 ulp (logf 2 ulp halved by the root, its rounding, sqrtf 1 ulp), sin / cos <= 2 ulp of 1, the product
    half an ulp: 5.77 * (2.25 + 2 + 0.5) * 2^-23 = 3.3e-6.  A wrong counter, lane, key or stream moves values by O(1)."""
    from conditional_score_diffusion_amd import ops
    got = ops.randn((n,), seed, stream, dev()).cpu().numpy().astype(np.float64)
    want = _randn_numpy(n, seed, stream)
    err = np.abs(got - want).max()
    print('randn n=%d seed=%d stream=%d: max abs err vs numpy %.3e' % (n, seed, stream, err))
    assert err <= 3.3e-6


# ---- 9. what the C entry point refuses --------------------------------------------------------------------------------------------------------
def _raw_inpaint_call(model, B, y=None, std_y=False, path=False, with_ip=True):
    """csd_pc_inpaint_sample with a one-step (reverse diffusion, none) schedule, straight through ctypes -> (status, message)"""
    import ctypes
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd._lib import current_stream, lib, ptr
    model._ensure_packed()
    ws = model._workspace(B)
    scratch = torch.empty(lib().csd_pc_inpaint_scratch_bytes(model._h, B), dtype=torch.uint8, device=dev())
    S = model.image_size
    x = torch.zeros(B, model.x_channels, S, S, device=dev())
    data, mask = torch.zeros_like(x), torch.ones_like(x)
    one = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    p = _lib.PCParams()
    p.n_steps, p.corrector = 1, 2
    p.labels = p.std_x = p.G = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
    if std_y:
        p.std_y = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
    if path:
        p.path_coef = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
    ip = _lib.PCInpaintParams()
    ip.data, ip.mask = data.data_ptr(), mask.data_ptr()
    ip.mean_scale = ip.std = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
    rc = lib().csd_pc_inpaint_sample(model._h, ptr(model._packed), ptr(ws), ws.numel(), ptr(scratch), scratch.numel(), ptr(x),
                                     ptr(y), B, ctypes.byref(p), ctypes.byref(ip) if with_ip else None, current_stream(dev()))
    torch.cuda.synchronize()
    return rc, lib().csd_last_error().decode()


def test_entry_point_refuses_conditional_use():
    _, _, _, model = model_for()
    rc, msg = _raw_inpaint_call(model, 2)
    assert rc == 0, msg                                    # (the call itself is well-formed)
    rc, msg = _raw_inpaint_call(model, 2, std_y=True)
    assert rc == -1 and 'std_y' in msg                     # CSD_ERR_INVALID
    rc, msg = _raw_inpaint_call(model, 2, path=True)
    assert rc == -1 and 'path_coef' in msg
    rc, msg = _raw_inpaint_call(model, 2, with_ip=False)
    assert rc == -1 and 'data, mask' in msg
    cfg, nc, p, sr3 = build('sr3_tiny')
    rc, msg = _raw_inpaint_call(sr3, 2, y=cases.case_y('sr3_tiny').to(dev()))
    assert rc == -1 and 'unconditional' in msg
