"""-m gpu: the band split / merge kernels (csd_band_split, csd_band_merge) and the sequential cascades (sampling/cascade.py on
csd_pc_cascade_sample) on the cases of tests/cascade_cases.py, against float64 and against the reference's stage-by-stage run
tests/golden/cascade.npz (tools/make_cascade_goldens.py).

Bounds.  Band operators: 1e-6 of the output's maximum - every value is a four-term fp32 fma chain, rounding about 2e-7.  Cascades: the
project's sampler bound, 1e-3 of the stage's sigma_max_x (tests/test_gpu_sr.py TRAJECTORY), for every stage's image; the second stage
does not amplify the first stage's error (a 1e-4 perturbation of the stage-2 condition moved the reference's stage-2 result by 5.5e-7
of sigma_max).  Everything between routes is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cascade_cases as cc  # noqa: E402
import cases  # noqa: E402
import guarded  # noqa: E402

BAND_SHAPES = [(2, 3, 5), (2, 3, 16), (1, 1, 8), (2, 8, 6)]          # (B, C, S): odd S, the 16-byte route, one channel, an even S % 4 != 0
BAND_TOL = 1e-6
_MODELS = {}


def dev():
    return torch.device('cuda:0')


def matrix_for(kind):
    if kind == 'haar':
        return None, cc.HAAR
    q, _ = np.linalg.qr(np.random.RandomState(17).standard_normal((4, 4)))
    m = torch.from_numpy(q.astype(np.float32))
    return m, m.double()


def image_for(B, C, S, seed=5):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((B, C, 2 * S, 2 * S)).astype(np.float32))


def close(a, ref):
    ref = ref.double()
    return float((a.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


# ---- 1. the band operators ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['haar', 'orthogonal'])
@pytest.mark.parametrize('B,C,S', BAND_SHAPES)
def test_band_split_and_merge_vs_float64(B, C, S, kind):
    from conditional_score_diffusion_amd import ops
    m32, m64 = matrix_for(kind)
    x = image_for(B, C, S)
    xd = x.to(dev())
    bands = ops.band_split(xd, m32)
    assert tuple(bands.shape) == (B, 4 * C, S, S)
    e_split = close(bands, cc.split64(x, m64))
    lo, hi = bands[:, :C], bands[:, C:]                                 # channel slices: no cat, no copy
    back = ops.band_merge(lo, hi, m32)
    e_merge = close(back, cc.merge64(lo.cpu(), hi.cpu(), m64))
    e_round = close(back, x)
    print('(%d, %d, %d) %s: split %.2e, merge %.2e, merge(split(x)) vs x %.2e' % (B, C, S, kind, e_split, e_merge, e_round))
    assert e_split < BAND_TOL and e_merge < BAND_TOL and e_round < BAND_TOL
    # bitwise repeatable, and a split of a channel slice of a wider image equals the split of its copy
    assert torch.equal(ops.band_split(xd, m32), bands) and torch.equal(ops.band_merge(lo, hi, m32), back)
    wide = torch.cat([xd, xd + 1.], dim=1)
    assert torch.equal(ops.band_split(wide[:, :C], m32), bands)


@pytest.mark.parametrize('kind', ['haar', 'orthogonal'])
@pytest.mark.parametrize('B,C,S', BAND_SHAPES)
def test_band_merge_into_the_first_channels_of_a_wider_buffer(B, C, S, kind):
    """the inpainting form's hand-over: out = buf[:, :C] of a [B, 4C, 2S, 2S] buffer between guards; the other 3C channels and both
    guards keep their fill, the written channels are bitwise the dense merge"""
    from conditional_score_diffusion_amd import ops
    m32, _ = matrix_for(kind)
    bands = ops.band_split(image_for(B, C, S).to(dev()), m32)
    dense = ops.band_merge(bands[:, :C], bands[:, C:], m32)
    for fill in (0x00, 0xFF):
        body, chk = guarded.guarded(B * 4 * C * 4 * S * S * 4, dev(), fill)
        buf = body.view(torch.float32).view(B, 4 * C, 2 * S, 2 * S)
        out = ops.band_merge(bands[:, :C], bands[:, C:], m32, out=buf[:, :C])
        torch.cuda.synchronize()
        assert out.data_ptr() == buf.data_ptr()
        chk('band_merge into a channel slice')
        assert torch.equal(buf[:, :C], dense)
        rest = body.view(B, -1)[:, C * 4 * S * S * 4:]
        assert int((rest != fill).sum()) == 0, 'band_merge wrote outside its %d channels' % C


def test_haar_split_of_a_constant_image_is_exact():
    from conditional_score_diffusion_amd import ops
    for S in (5, 8):
        c = 0.3
        bands = ops.band_split(torch.full((2, 3, 2 * S, 2 * S), c, device=dev()))
        assert torch.equal(bands[:, :3], torch.full((2, 3, S, S), np.float32(c) * 2, device=dev()))
        assert int((bands[:, 3:] != 0).sum()) == 0


def test_band_operators_refuse_bad_arguments():
    from conditional_score_diffusion_amd import ops
    x = image_for(1, 2, 4).to(dev())
    bad = torch.eye(4)
    bad[3, 3] = 1.001
    with pytest.raises(RuntimeError, match='not orthogonal.*2.0'):
        ops.band_split(x, bad)
    with pytest.raises(RuntimeError, match='not orthogonal'):
        ops.band_merge(x[:, :, :4, :4].contiguous(), torch.zeros(1, 6, 4, 4, device=dev()), bad)
    with pytest.raises(RuntimeError, match='even'):
        ops.band_split(torch.zeros(1, 2, 7, 7, device=dev()))
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.band_split(x.cpu())
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.band_merge(torch.zeros(1, 2, 4, 4), torch.zeros(1, 6, 4, 4))
    with pytest.raises(RuntimeError, match='3C'):
        ops.band_merge(torch.zeros(1, 2, 4, 4, device=dev()), torch.zeros(1, 4, 4, 4, device=dev()))


def test_the_four_helpers():
    from conditional_score_diffusion_amd import ops
    from conditional_score_diffusion_amd.sampling import cascade
    x = image_for(2, 3, 8).to(dev())
    bands = cascade.haar_forward(x)
    assert torch.equal(bands, ops.band_split(x))
    assert torch.equal(cascade.get_dc_coefficients(x), bands[:, :3]) and torch.equal(cascade.get_hf_coefficients(x), bands[:, 3:])
    assert close(cascade.haar_backward(bands), x.cpu()) < BAND_TOL
    dc2 = cascade.get_dc_coefficients(x, levels=2)
    assert tuple(dc2.shape) == (2, 3, 4, 4) and close(dc2, cc.split64(cc.split64(x.cpu())[:, :3])[:, :3]) < BAND_TOL


# ---- 2. the cascades -----------------------------------------------------------------------------------------------------------------------
def stages_for(flow, precision='fp32', fresh=False, sigma_max_y=None):
    """[(model, sde or pair, config)] of a flow, the models cached per (flow, stage, precision)"""
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    out = []
    for k in range(cc.N_STAGES):
        cfg = cc.stage_config(flow, k, precision)
        key = (flow, k, precision)
        if fresh or key not in _MODELS:
            model = mutils.create_model(cfg)
            res = model.load_state_dict(cc.stage_params(flow, k))
            assert not res.missing_keys and not res.unexpected_keys
            model = model.to(dev()).eval()
            if not fresh:
                _MODELS[key] = model
        else:
            model = _MODELS[key]
        m = cfg.model
        if flow == 'haar_inpaint':
            sde = sde_lib.VESDE(m.sigma_min_x, m.sigma_max_x, cc.P_STEPS)
        else:
            smax_y = m.sigma_max_y if sigma_max_y is None or k == 0 else sigma_max_y
            sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, smax_y, m.num_scales)}
        out.append((model, sde, cfg))
    return out


def sampler_for(flow, stages, one_call=True, **kw):
    from conditional_score_diffusion_amd.sampling import cascade
    if flow != 'haar_inpaint':
        kw.setdefault('p_steps', cc.P_STEPS)
    return cascade.get_autoregressive_sampler(stages, flow, one_call=one_call, **kw)


def tapes(flow):
    return [cc.tape(flow, k) for k in range(cc.N_STAGES)]


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('flow', cc.FLOWS)
def test_one_call_vs_reference_fixture(flow, precision):
    """every stage's image of the one-call cascade on the fixture's tapes within 1e-3 of the stage's sigma_max_x of the reference's
    stage-by-stage run"""
    g = cc.golden()
    lr = cc.lr_input(flow).to(dev())
    images, info = sampler_for(flow, stages_for(flow, precision))(lr, return_intermediate_images=True, noise_tapes=tapes(flow))
    assert info == [] and len(images) == cc.N_STAGES + 1 and torch.equal(images[0], lr.cpu())
    for k in range(cc.N_STAGES):
        ref = g['%s_s%d' % (flow, k)]
        assert tuple(images[k + 1].shape) == cc.image_shape(flow, k) == tuple(ref.shape)
        d = float(np.abs(images[k + 1].numpy().astype(np.float64) - ref).max()) / cc.sigma_max(flow, k)
        print('%s %s stage %d: one call vs reference %.3e of sigma_max_x' % (flow, precision, k, d))
        assert d < cc.TRAJECTORY, (flow, precision, k, d)
    final, info = sampler_for(flow, stages_for(flow, precision))(lr, noise_tapes=tapes(flow))
    assert info == [] and final.is_cuda and torch.equal(final.cpu(), images[-1])


def _single_stage(flow, stage, lr, k=0, **kw):
    """stage k alone through its existing fused sampler -> the stage's state"""
    from conditional_score_diffusion_amd.sampling import conditional, unconditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    model, sde, cfg = stage
    pred, corr = get_predictor(cfg.sampling.predictor), get_corrector(cfg.sampling.corrector)
    if flow == 'haar_inpaint':
        data = torch.zeros(lr.shape[0], 12, lr.shape[2], lr.shape[3], device=dev())
        data[:, :3] = lr
        mask = torch.zeros(1, 12, 1, 1, device=dev())
        mask[:, :3] = 1.
        fn = unconditional.get_pc_inpainter(sde, pred, corr, cfg.sampling.snr, n_steps=1, continuous=True, denoise=True, eps=cc.EPS, device_loop=True)
        return fn(model, data, mask, **kw)[0]
    fn = conditional.get_pc_conditional_sampler(sde, model._x_shape(lr.shape[0]), pred, corr, snr=cfg.sampling.snr, p_steps=cc.P_STEPS, c_steps=1,
                                                continuous=True, denoise=True, eps=cc.EPS)
    return fn(model, lr, **kw)[0]


def _image_of(flow, lr, state):
    from conditional_score_diffusion_amd import ops
    if flow == 'bicubic':
        return state
    return ops.band_merge(lr, state[:, 3:] if flow == 'haar_inpaint' else state)


@pytest.mark.parametrize('flow', cc.FLOWS)
def test_routes_give_the_same_bits(flow):
    """one call == the chained Python route == the existing single-stage fused call on stage 1; with seed=: the cascade == the stages one
    by one with stage_seed(s, k); the same seed repeats, another seed differs"""
    from conditional_score_diffusion_amd.sampling import cascade
    stages = stages_for(flow, 'fp16x3')
    lr = cc.lr_input(flow).to(dev())
    tp = tapes(flow)
    one, _ = sampler_for(flow, stages, True)(lr, return_intermediate_images=True, noise_tapes=tp)
    chained, _ = sampler_for(flow, stages, False)(lr, return_intermediate_images=True, noise_tapes=tp)
    auto, _ = sampler_for(flow, stages, None)(lr, return_intermediate_images=True, noise_tapes=tp)
    for a, b, c in zip(one, chained, auto):
        assert torch.equal(a, b) and torch.equal(a, c)
    first = _image_of(flow, lr, _single_stage(flow, stages[0], lr, noise_tape=tp[0]))
    assert torch.equal(first.cpu(), one[1])
    # seeds
    a, _ = sampler_for(flow, stages, True)(lr, return_intermediate_images=True, seed=11)
    b, _ = sampler_for(flow, stages, True)(lr, return_intermediate_images=True, seed=11)
    c, _ = sampler_for(flow, stages, False)(lr, return_intermediate_images=True, seed=11)
    d, _ = sampler_for(flow, stages, True)(lr, return_intermediate_images=True, seed=12)
    cur = lr
    for k in range(cc.N_STAGES):
        cur = _image_of(flow, cur, _single_stage(flow, stages[k], cur, seed=cascade.stage_seed(11, k))).contiguous()
        assert torch.equal(cur.cpu(), a[k + 1]), (flow, k)
        assert torch.equal(a[k + 1], b[k + 1]) and torch.equal(a[k + 1], c[k + 1]) and not torch.equal(a[k + 1], d[k + 1])
        assert bool(torch.isfinite(a[k + 1]).all())


@pytest.mark.parametrize('flow', cc.FLOWS)
def test_sample_zero_of_a_batch_equals_the_batch_of_one(flow):
    """without a corrector (multi_scale_test's 'conditional_none'; the Langevin step size couples a batch through its mean norms) sample 0
    of B = 2 equals B = 1 on the same tape rows, for every stage"""
    none = 'none' if flow == 'haar_inpaint' else 'conditional_none'
    stages = stages_for(flow, 'fp16x3')
    lr = cc.lr_input(flow).to(dev())
    tp = []
    for k in range(cc.N_STAGES):
        xs, ys = cc.state_shape(flow, k), cc.cond_shape(flow, k)
        # no corrector: the predictor's draws only; the inpainting stage still blends behind the 'none' phase
        per_step = [xs, xs, xs] if ys is None else [ys, xs]
        tp.append(cases.tape([xs] + per_step * cc.P_STEPS, seed=900 + k))
    two, _ = sampler_for(flow, stages, True, corrector=none)(lr, return_intermediate_images=True, noise_tapes=tp)
    one, _ = sampler_for(flow, stages, True, corrector=none)(lr[:1].contiguous(), return_intermediate_images=True,
                                                              noise_tapes=[[t[:1].contiguous() for t in tape] for tape in tp])
    for k in range(cc.N_STAGES + 1):
        assert torch.equal(two[k][:1], one[k]), (flow, k)
    assert not torch.equal(two[-1][:1], two[-1][1:])


@pytest.mark.parametrize('flow', cc.FLOWS)
def test_results_do_not_depend_on_what_the_buffers_held(flow):
    """workspace, scratch (with the hand-over images that have no caller buffer: return_intermediate_images = False), stage outputs, data
    buffers, priors and stage_flags between guards, pre-filled with 0x00 and with 0xFF: the same bits, every guard intact"""
    stages = stages_for(flow, 'fp16x3')
    lr = cc.lr_input(flow).to(dev())
    tp = tapes(flow)
    want, _ = sampler_for(flow, stages, True)(lr, noise_tapes=tp)
    for keep in (False, True):
        for fill in (0x00, 0xFF):
            with guarded.seam(fill) as rec:
                for model, _, _ in stages:
                    guarded.reset_model_buffers(model)
                got, _ = sampler_for(flow, stages, True)(lr, return_intermediate_images=keep, noise_tapes=tp)
                torch.cuda.synchronize()
                got = got[-1] if keep else got.cpu()
            rec.check_guards()
            assert rec.checks
            assert torch.equal(got, want.cpu()), 'fill 0x%02X changes the result (return_intermediate_images = %s)' % (fill, keep)
    for model, _, _ in stages:
        guarded.reset_model_buffers(model)


def test_a_non_finite_condition_at_stage_two_names_stage_two():
    """stage 2's condition SDE has sigma_max_y = inf: y_t = y + inf * z is not finite from stage 2's first evaluation on, stage 1 is
    untouched.  (An infinite output bias at stage 1 would make stage 1's own state non-finite, and the call would rightly name stage 1.)
    Arithmetic only: NaN flows through the kernels, nothing faults."""
    from conditional_score_diffusion_amd._lib import NonFiniteError
    flow = 'bicubic'
    stages = stages_for(flow, 'fp32', sigma_max_y=float('inf'))
    sampler = sampler_for(flow, stages, True)
    with pytest.raises(NonFiniteError, match=r'stage 2 of 2 \(stages\[1\]\)'):
        sampler(cc.lr_input(flow).to(dev()), noise_tapes=tapes(flow))
    flags = sampler.stage_flags.cpu().tolist()
    assert flags[0] == 0 and flags[1] != 0, flags


def _c_cascade(flow, stages, order=(0, 1), links=None, ws_short=0, scratch_short=0, y_scale_handle=None):
    """csd_pc_cascade_sample called directly on prepared stages -> (status, message); nothing is enqueued when validation fails"""
    from conditional_score_diffusion_amd import _lib, ops
    from conditional_score_diffusion_amd.sampling import fused
    l = _lib.lib()
    n = len(order)
    arr = (_lib.CascadeStage * n)()
    preps = []
    for j, k in enumerate(order):
        model, sde, cfg = stages[k]
        prep = fused.prepare(model, sde, model._x_shape(cc.B), None, cc.P_STEPS, cfg.sampling.snr, cc.EPS, True, noise_tape=cc.tape(flow, k))
        preps.append(prep)
        arr[j].net, arr[j].packed, arr[j].pc, arr[j].x = model._h, model._packed.data_ptr(), ctypes.pointer(prep.p), prep.x.data_ptr()
        arr[j].link = 0 if j == 0 else ({'bicubic': 0, 'haar': 1}[flow] if links is None else links)
    if y_scale_handle is not None:
        arr[n - 1].net, arr[n - 1].packed = y_scale_handle._h, y_scale_handle._packed.data_ptr()
    ws = ops._scratch(max(l.csd_unet_workspace_bytes(stages[k][0]._h, cc.B) for k in order) - ws_short, dev())
    pc = max((l.csd_pc_scratch_bytes(stages[k][0]._h, cc.B) + 255) // 256 * 256 for k in order)
    hand = sum((cc.B * 3 * 4 * stages[k][0].image_size ** 2 * 4 + 255) // 256 * 256 for k in order[:-1]) if flow == 'haar' else 0
    scratch = ops._scratch(pc + hand - scratch_short, dev())
    flags = torch.zeros(n, dtype=torch.int32, device=dev())
    out = torch.empty(cc.image_shape(flow, order[-1]), device=dev())
    if flow == 'haar':
        arr[n - 1].out = out.data_ptr()
    rc = l.csd_pc_cascade_sample(arr, n, 1 if flow == 'haar' else 0, ctypes.c_void_p(cc.lr_input(flow).to(dev()).data_ptr()), cc.B,
                                 ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(scratch.data_ptr()), scratch.numel(),
                                 ctypes.c_void_p(flags.data_ptr()), None, None)
    torch.cuda.synchronize()
    return rc, l.csd_last_error().decode()


def test_entry_validation_names_the_stage():
    from conditional_score_diffusion_amd.models import utils as mutils
    import kxsr_cases as kc
    for flow in ('bicubic', 'haar'):
        stages = stages_for(flow, 'fp32')
        rc, msg = _c_cascade(flow, stages)
        assert rc == 0, msg
        rc, msg = _c_cascade(flow, stages, order=(1, 0))                 # mismatched extents at the link
        assert rc == -1 and 'stages[1]' in msg and 'link %d' % (0 if flow == 'bicubic' else 1) in msg, msg
        rc, msg = _c_cascade(flow, stages, links=1 if flow == 'bicubic' else 0)      # the other flow's link
        assert rc == -1 and 'stages[1]' in msg, msg
        rc, msg = _c_cascade(flow, stages, links=2)                      # link 2 joins inpainting stages
        assert rc == -1 and 'stages[1]' in msg and 'inpaint' in msg, msg
        rc, msg = _c_cascade(flow, stages, ws_short=256)
        assert rc == -5 and 'stages[1]' in msg and 'workspace' in msg, msg
        rc, msg = _c_cascade(flow, stages, scratch_short=256)
        assert rc == -5 and 'stages[1]' in msg and 'scratch' in msg, msg
    # a handle with y_scale in the last slot
    case = sorted(kc.CASES)[0]
    kcfg = kc.make_config(case)
    km = mutils.create_model(kcfg).to(dev()).eval()
    km._ensure_packed()
    assert km.y_scale >= 2
    rc, msg = _c_cascade('bicubic', stages_for('bicubic', 'fp32'), y_scale_handle=km)
    assert rc == -1 and 'stages[1]' in msg and 'y_scale' in msg, msg
