"""-m gpu: PC colorization with an unconditional network (colorize_blend_kernel, csd_pc_colorize_sample).  The operator against a float64
evaluation of its formulas and the reference's recorded output; the step-by-step colorizer and the device loop against the reference's own
runs (tests/golden/colorize.npz from tools/make_colorize_goldens.py) and against each other; the on-device noise, recording, the
global-norm form, the finiteness contract, and what the C entry refuses without writing a caller's buffer."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import colorize_cases as cc  # noqa: E402
import guarded  # noqa: E402
from test_gpu_network import build, dev, rel  # noqa: E402

OP_BOUND = 5e-6                                   # what tests/test_gpu_vp_sampling.py holds the fp32 step kernels to
RUN_BOUND = 2e-4                                  # of sigma_max (VE) or of 1 (VP, sub-VP): DESIGN.md 4d, the inpainting row
M_SCALE, STD = 0.8125 + 1e-3, 3.7

_MODEL = []


def model():
    if not _MODEL:
        _MODEL.append(build('uncond_tiny')[3])
    return _MODEL[0]


def colorizer(name, device_loop, denoise=None):
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import unconditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    _, scls, pred, corr, pf, dn = cc.run(name)
    sde = cc.make_sde(sde_lib, scls)
    fn = unconditional.get_pc_colorizer(sde, get_predictor(pred), get_corrector(corr), snr=cc.SNR, n_steps=1, probability_flow=pf,
                                        continuous=True, denoise=dn if denoise is None else denoise, eps=cc.EPS, device_loop=device_loop)
    return fn, sde


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------------------
def _view(t, offset):
    """the same values on the device, at a 16-byte aligned address or ``offset`` floats behind one"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _op_inputs(shape, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 30.
    gray = torch.rand((shape[0], 1) + tuple(shape[2:]), generator=g).repeat(1, 3, 1, 1)
    z = torch.randn(shape, generator=g)
    return x, gray, z


OP_SHAPES = [((2, 3, 4, 4), 0), ((3, 3, 5, 7), 0), ((1, 3, 16, 16), 1)]      # full float4 groups | a partial group, unaligned planes | a view one float off


def _close(got, want):
    want = want.numpy() if isinstance(want, torch.Tensor) else want
    return rel(got.cpu().numpy(), want) <= OP_BOUND


@pytest.mark.parametrize('shape,offset', OP_SHAPES)
@pytest.mark.parametrize('form', ['tape', 'seed', 'neither'])
def test_blend_vs_float64(shape, offset, form):
    from conditional_score_diffusion_amd import ops
    x0, gray, z = _op_inputs(shape)
    gray0 = ops.colorize_gray0(gray.to(dev()))
    want_g0 = cc.gray0_64(gray)
    assert tuple(gray0.shape) == (shape[0], 1) + tuple(shape[2:]) and _close(gray0, want_g0)
    g0 = _view(gray0, offset)
    if form == 'tape':
        x, xm = ops.colorize_blend(_view(x0, offset), g0, _view(z, offset), M_SCALE, STD)
        zr, sd = z, STD
    elif form == 'seed':
        x, xm = ops.colorize_blend(_view(x0, offset), g0, None, M_SCALE, STD, seed=2 ** 40 + 11, stream_id=2 ** 33 + 5)
        zr, sd = ops.randn(shape, 2 ** 40 + 11, 2 ** 33 + 5, dev()).cpu(), STD
    else:
        x, xm = ops.colorize_blend(_view(x0, offset), g0, None, M_SCALE, 0.0)
        zr, sd = None, 0.0
    assert x.data_ptr() % 16 == 4 * offset
    xr, xmr = cc.blend64(x0, want_g0, zr, M_SCALE, sd)
    ex, em = rel(x.cpu().numpy(), xr.numpy()), rel(xm.cpu().numpy(), xmr.numpy())
    print('colorize_blend %s offset %d %s: x %.3e, x_mean %.3e' % (shape, offset, form, ex, em))
    assert ex <= OP_BOUND and em <= OP_BOUND
    # channel 0 of the decoupled result is the perturbed gray channel
    m64, _ = cc.matrices64()
    want0 = M_SCALE * want_g0[:, 0] + (sd * zr[:, 0].double() if zr is not None else 0.)
    assert rel(cc.decouple64(x.cpu(), m64)[:, 0].numpy(), want0.numpy()) <= OP_BOUND
    # x_mean=False writes the same x and no second tensor
    x2, none = ops.colorize_blend(_view(x0, offset), g0, _view(zr, offset) if zr is not None else None, M_SCALE, sd, x_mean=False)
    assert none is None and torch.equal(x2, x)


def test_tape_form_vs_the_references_operator():
    """tests/golden/colorize.npz op_x / op_x_mean: the reference's own update function around the `none` predictor"""
    from conditional_score_diffusion_amd import ops, sde_lib
    g = cc.golden()
    x0, gray, z = cc.op_inputs()
    sde = cc.make_sde(sde_lib, 'VPSDE')
    ms, sd = sde.marginal_prob(torch.ones(1, 1, 1, 1), torch.tensor([cc.OP_T]))
    assert [float(ms.flatten()[0]), float(sd)] == list(g['op_scalars'])          # the same fp32 scalars as the reference's
    x, xm = ops.colorize_blend(x0.to(dev()), ops.colorize_gray0(gray.to(dev())), z.to(dev()), float(ms.flatten()[0]), float(sd))
    ex, em = rel(x.cpu().numpy(), g['op_x']), rel(xm.cpu().numpy(), g['op_x_mean'])
    print('colorize_blend vs the reference operator: x %.3e, x_mean %.3e' % (ex, em))
    assert ex <= OP_BOUND and em <= OP_BOUND


@pytest.mark.parametrize('shape,offset', OP_SHAPES)
def test_seed_form_is_the_tape_form_of_its_stream(shape, offset):
    """bit for bit; channels 1 and 2 of the draw are never read; two calls agree; sample 0 does not depend on the batch"""
    from conditional_score_diffusion_amd import ops
    x0, gray, _ = _op_inputs(shape, seed=9)
    g0 = _view(ops.colorize_gray0(gray.to(dev())), offset)
    for seed, stream in ((7, 3), (2 ** 40 + 11, 2 ** 33 + 5)):
        z = ops.randn(shape, seed, stream, dev())
        a, am = ops.colorize_blend(_view(x0, offset), g0, _view(z, offset), 0.9, 2.5)
        b, bm = ops.colorize_blend(_view(x0, offset), g0, None, 0.9, 2.5, seed=seed, stream_id=stream)
        assert torch.equal(a, b) and torch.equal(am, bm)
        assert float((a - x0.to(dev())).abs().max()) > 0.1
        zz = z.clone()
        zz[:, 1:] = float('nan')
        c, cm = ops.colorize_blend(_view(x0, offset), g0, _view(zz, offset), 0.9, 2.5)
        assert torch.equal(a, c) and torch.equal(am, cm)
        d, dm = ops.colorize_blend(_view(x0, offset), g0, None, 0.9, 2.5, seed=seed, stream_id=stream)
        assert torch.equal(b, d) and torch.equal(bm, dm)
    if shape[0] > 1:
        z = ops.randn(shape, 7, 3, dev())
        full, full_m = ops.colorize_blend(x0.to(dev()), g0.contiguous(), z, 0.9, 2.5)
        one, one_m = ops.colorize_blend(x0[:1].to(dev()), g0[:1].contiguous(), z[:1].contiguous(), 0.9, 2.5)
        assert torch.equal(full[:1], one) and torch.equal(full_m[:1], one_m)
        full, _ = ops.colorize_blend(x0.to(dev()), g0.contiguous(), None, 0.9, 2.5, seed=7, stream_id=3)
        one, _ = ops.colorize_blend(x0[:1].to(dev()), g0[:1].contiguous(), None, 0.9, 2.5, seed=7, stream_id=3)
        assert torch.equal(full[:1], one)


@pytest.mark.parametrize('shape,offset', OP_SHAPES)
def test_initial_state_vs_float64(shape, offset):
    """couple(decouple(gray) * mask + decouple(prior * (1 - mask))): the prior masked in image space"""
    from conditional_score_diffusion_amd import ops
    prior, gray, _ = _op_inputs(shape, seed=13)
    x = ops.colorize_start(_view(prior, offset), _view(ops.colorize_gray0(gray.to(dev())), offset))
    m, inv = cc.matrices64()
    mask = torch.tensor([1., 0., 0.], dtype=torch.float64).reshape(1, 3, 1, 1)
    want = cc.decouple64(cc.decouple64(gray, m) * mask + cc.decouple64(prior.double() * (1. - mask), m), inv)
    assert _close(x, want)


def test_operator_refusals():
    from conditional_score_diffusion_amd import ops
    x0, gray, z = _op_inputs((2, 3, 4, 4))
    g0 = ops.colorize_gray0(gray.to(dev()))
    skew = torch.tensor(cc.M) + torch.tensor([[0., 0., 0.], [0., 1e-3, 0.], [0., 0., 0.]])
    with pytest.raises(RuntimeError, match='not orthogonal'):
        ops.colorize_blend(x0.to(dev()), g0, z.to(dev()), 1.0, 1.0, matrix=skew)
    with pytest.raises(RuntimeError, match='not orthogonal'):
        ops.colorize_gray0(gray.to(dev()), matrix=skew)
    with pytest.raises(RuntimeError, match='3 x 3'):
        ops.colorize_blend(x0.to(dev()), g0, z.to(dev()), 1.0, 1.0, matrix=torch.eye(4))
    for c in (2, 4):
        bad = torch.zeros(2, c, 4, 4, device=dev())
        with pytest.raises(RuntimeError, match=r'\[B, 3, H, W\]'):
            ops.colorize_blend(bad, g0, None, 1.0, 0.0)
        with pytest.raises(RuntimeError, match=r'\[B, 3, H, W\]'):
            ops.colorize_gray0(bad)
    # another orthogonal matrix is taken: a permutation makes channel 2 the imposed one
    perm = torch.tensor([[0., 1., 0.], [0., 0., 1.], [1., 0., 0.]])
    x, _ = ops.colorize_blend(x0.to(dev()), ops.colorize_gray0(gray.to(dev()), matrix=perm), None, 1.0, 0.0, matrix=perm)
    assert torch.equal(x[:, 2].cpu(), gray[:, 2]) and torch.equal(x[:, :2].cpu(), x0[:, :2])


# ---- 2. the runs ----------------------------------------------------------------------------------------------------------------------------------
_RESULTS = {}


def results(name):
    """(step by step, device loop) of a run on its tape, computed once"""
    if name not in _RESULTS:
        _, scls, pred, corr, pf, dn = cc.run(name)
        tape = cc.run_tape(pred, corr)
        gray = cc.gray().to(dev())
        fn, _ = colorizer(name, False)
        with cc.Tape(tape) as tp:
            step, info = fn(model(), gray)
            assert tp.i == len(tape) and info == {}
        fn, _ = colorizer(name, True)
        loop, info = fn(model(), gray, noise_tape=tape)
        assert info == {}
        _RESULTS[name] = (step.cpu().numpy(), loop.cpu().numpy())
    return _RESULTS[name]


@pytest.mark.parametrize('name', [r[0] for r in cc.RUNS])
def test_step_by_step_vs_the_reference_run(name):
    ref = cc.golden()['run_' + name]
    err = float(np.abs(results(name)[0] - ref).max()) / cc.scale(cc.run(name)[1])
    print('%s: step by step vs the reference run %.3e of scale (max |ref| %.1f)' % (name, err, np.abs(ref).max()))
    assert err <= RUN_BOUND


@pytest.mark.parametrize('name', [r[0] for r in cc.RUNS])
def test_device_loop_vs_the_reference_run(name):
    ref = cc.golden()['run_' + name]
    err = float(np.abs(results(name)[1] - ref).max()) / cc.scale(cc.run(name)[1])
    print('%s: device loop vs the reference run %.3e of scale (max |ref| %.1f)' % (name, err, np.abs(ref).max()))
    assert np.isfinite(results(name)[1]).all() and err <= RUN_BOUND


@pytest.mark.parametrize('name', [r[0] for r in cc.RUNS])
def test_device_loop_vs_step_by_step(name):
    step, loop = results(name)
    err = rel(loop, step)
    print('%s: device loop vs step by step %.3e' % (name, err))
    assert err <= 1e-5


@pytest.mark.parametrize('name', ['ve_rd_lang', 'vp_em_none'])
def test_record_returns_the_initial_state_and_every_step(name):
    _, scls, pred, corr, pf, _ = cc.run(name)
    tape = cc.run_tape(pred, corr, seed=3)
    fn, sde = colorizer(name, True, denoise=False)
    x, info = fn(model(), cc.gray().to(dev()), show_evolution=True, noise_tape=tape)
    ev = info['evolution']
    assert tuple(ev.shape) == (cc.N + 1,) + cc.shape() and ev.device.type == 'cpu'
    assert torch.equal(ev[-1], x.cpu())                              # (denoise off: the last recorded state is the result)
    m, inv = cc.matrices64()
    mask = torch.tensor([1., 0., 0.], dtype=torch.float64).reshape(1, 3, 1, 1)
    prior = tape[0].double() * (sde.sigma_max if scls == 'VESDE' else 1.0)
    want = cc.decouple64(cc.decouple64(cc.gray(), m) * mask + cc.decouple64(prior * (1. - mask), m), inv)
    assert rel(ev[0].numpy(), want.numpy()) <= OP_BOUND
    # the step-by-step loop records the same
    with cc.Tape(tape):
        xs, infos = colorizer(name, False, denoise=False)[0](model(), cc.gray().to(dev()), show_evolution=True)
    assert tuple(infos['evolution'].shape) == tuple(ev.shape) and torch.equal(infos['evolution'][-1], xs.cpu())
    assert rel(ev.numpy(), infos['evolution'].numpy()) <= 1e-5


def test_seed_is_reproducible_and_equals_the_tape_of_its_streams():
    from conditional_score_diffusion_amd import ops
    name = 've_rd_lang'
    _, _, pred, corr, _, _ = cc.run(name)
    fn, _ = colorizer(name, True)
    gray = cc.gray().to(dev())
    a, _ = fn(model(), gray, seed=5)
    b, _ = fn(model(), gray, seed=5)
    c, _ = fn(model(), gray, seed=6)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert (a - c).abs().max().item() > 1e-2
    tape = [ops.randn(cc.shape(), 5, k, dev()) for k in range(1 + cc.n_draws(pred, corr))]
    d, _ = fn(model(), gray, noise_tape=tape)
    assert torch.equal(a, d)


def test_short_tape_is_refused_with_the_count():
    name = 'vp_rd_lang'
    _, _, pred, corr, _, _ = cc.run(name)
    tape = cc.run_tape(pred, corr)
    n = cc.n_draws(pred, corr)
    with pytest.raises(RuntimeError, match='noise tape holds %d draws after the prior, the loop needs %d' % (n - 1, n)):
        colorizer(name, True)[0](model(), cc.gray().to(dev()), noise_tape=tape[:-1])


def test_global_norm_on_one_rank_is_the_plain_run():
    """csd_pc_colorize_step_begin / _step_end with global_batch == B and no exchange: 1e-6 of the prior's scale, the bound of
    test_gpu_inpaint_fused.py::test_step_forms_reproduce_the_one_call_form"""
    for name in ('ve_rd_lang', 'vp_rd_lang'):
        _, scls, pred, corr, _, _ = cc.run(name)
        tape = cc.run_tape(pred, corr, seed=91)
        fn, _ = colorizer(name, True)
        a, _ = fn(model(), cc.gray().to(dev()), noise_tape=tape)
        b, _ = fn(model(), cc.gray().to(dev()), noise_tape=tape, global_norm=(lambda s: None, cc.B))
        err = float((a - b).abs().max()) / cc.scale(scls)
        print('%s: step_begin / step_end vs one call %.3e of scale' % (name, err))
        assert torch.isfinite(a).all() and err < 1e-6


def test_nan_weight_raises():
    from conditional_score_diffusion_amd._lib import NonFiniteError
    bad = build('uncond_tiny')[3]
    with torch.no_grad():
        next(bad.parameters()).view(-1)[0] = float('nan')
    for name in ('ve_rd_lang', 've_em_none'):                      # the Langevin norms / the pass over the returned state
        with pytest.raises(NonFiniteError):
            colorizer(name, True)[0](bad, cc.gray().to(dev()), seed=1)


def test_colorization_fn_reads_csd_device_loop():
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import unconditional
    cfg = cc.config()
    cfg.training.continuous = True
    sde = cc.make_sde(sde_lib, 'VESDE')
    gray = cc.gray().to(dev())
    with pytest.raises(NotImplementedError, match='device_loop=True'):      # the default: the step-by-step loop, which takes no seed
        unconditional.get_colorization_fn(cfg, sde, cc.EPS)(model(), gray, seed=3)
    cfg.sampling.csd_device_loop = True
    cfg.sampling.snr = cc.SNR
    a, _ = unconditional.get_colorization_fn(cfg, sde, cc.EPS)(model(), gray, seed=5)
    b, _ = colorizer('ve_rd_lang', True)[0](model(), gray, seed=5)
    assert torch.equal(a, b)


# ---- 3. what the C entry refuses, and what it leaves alone ------------------------------------------------------------------------------------
def _meta_handle(cfg):
    from conditional_score_diffusion_amd.models import utils as mutils
    with torch.device('meta'):
        return mutils.create_model(cfg)


def _refused_handles():
    import sr_cases
    import wide_cases as wc
    from test_pc_draws_host import handle
    return [(handle('ddpm3d_B')[0], '3-D'), (handle('kxsr_K1')[0], 'y_scale'), (_meta_handle(sr_cases.make_config('R1')), 'x_squeeze'),
            (handle('paired_3_1')[0], 'unconditional networks only'), (_meta_handle(wc.make_config('W2')), 'x_channels = 12')]


def test_entry_refusals_leave_every_buffer_unwritten():
    """csd_pc_colorize_sample refuses the handle before it looks at another argument: every caller buffer - packed weights, workspace,
    scratch, state, gray0, the record - keeps the byte it was filled with, guards included (tests/guarded.py)"""
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd._lib import current_stream, lib
    fill, nbytes = 0xA5, 1 << 16
    one = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    for h, words in _refused_handles():
        bufs = {k: guarded.guarded(nbytes, dev(), fill) for k in ('packed', 'workspace', 'scratch', 'x', 'gray0', 'record')}
        addr = {k: ctypes.c_void_p(b.data_ptr()) for k, (b, _) in bufs.items()}
        p = _lib.PCParams()
        p.n_steps, p.corrector = 1, 2
        p.labels = p.std_x = p.G = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
        p.record = addr['record']
        cp = _lib.PCColorizeParams()
        cp.gray0 = addr['gray0']
        cp.mean_scale = cp.std = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
        rc = lib().csd_pc_colorize_sample(h._h, addr['packed'], addr['workspace'], nbytes, addr['scratch'], nbytes, addr['x'], None, 2,
                                          ctypes.byref(p), ctypes.byref(cp), current_stream(dev()))
        msg = lib().csd_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and 'pc_colorize' in msg and words in msg, (rc, msg)      # CSD_ERR_INVALID
        for k, (body, chk) in bufs.items():
            chk(k)
            assert bool((body == fill).all()), '%s was written by a refused call (%s)' % (k, words)
    # a well-formed call with conditional arguments is refused by name as well
    m = model()
    m._ensure_packed()
    ws = m._workspace(2)
    scratch = torch.empty(lib().csd_pc_scratch_bytes(m._h, 2), dtype=torch.uint8, device=dev())
    x = torch.zeros(2, 3, 16, 16, device=dev())
    g0 = torch.zeros(2, 1, 16, 16, device=dev())
    for field, words in (('std_y', 'std_y given'), ('path_coef', 'path_coef belong'), (None, '')):
        p = _lib.PCParams()
        p.n_steps, p.corrector = 1, 2
        p.labels = p.std_x = p.G = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
        if field:
            setattr(p, field, ctypes.cast(one, ctypes.POINTER(ctypes.c_float)))
        cp = _lib.PCColorizeParams()
        cp.gray0 = g0.data_ptr()
        cp.mean_scale = cp.std = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
        rc = lib().csd_pc_colorize_sample(m._h, _lib.ptr(m._packed), _lib.ptr(ws), ws.numel(), _lib.ptr(scratch), scratch.numel(),
                                          _lib.ptr(x), None, 2, ctypes.byref(p), ctypes.byref(cp), current_stream(dev()))
        torch.cuda.synchronize()
        msg = lib().csd_last_error().decode()
        assert (rc == -1 and words in msg) if field else rc == 0, (field, rc, msg)
    rc = lib().csd_pc_colorize_sample(m._h, _lib.ptr(m._packed), _lib.ptr(ws), ws.numel(), _lib.ptr(scratch), scratch.numel(), _lib.ptr(x),
                                      None, 2, ctypes.byref(p), None, current_stream(dev()))
    assert rc == -1 and 'gray0, mean_scale and std' in lib().csd_last_error().decode()


def test_sample_sharded_takes_the_gray_batch_as_its_condition():
    """distributed.sample_sharded shards y_global and hands the shard on as the sampler's second argument: the gray batch"""
    from conditional_score_diffusion_amd import distributed
    fn, _ = colorizer('ve_rd_lang', True)
    gray = cc.gray().to(dev())
    a, _ = distributed.sample_sharded(fn, model(), y_global=gray, seed=5)
    b, _ = fn(model(), gray, seed=distributed.rank_seed(5, 0))
    assert tuple(a.shape) == cc.shape() and torch.equal(a, b)
