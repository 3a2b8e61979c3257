"""-m gpu: the DDPM family on images with more than 8 channels (9 .. 32 in, up to 32 out) through every layer that 8-channel networks
reach: planned inference, the fused PC loop, device-loop inpainting, the planned training graph and its input gradient, the fused
likelihood right-hand side - against the reference's fixture tests/golden/wide_channels.npz (tools/make_wide_goldens.py) on the cases
of tests/wide_cases.py - and the first layer as an operator (stem_wide_kernel beside assemble + generic convolution).

Bounds are those of the 8-channel tests they mirror; each test names its source."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import wide_cases as wc  # noqa: E402
from test_gpu_steps import _Tape  # noqa: E402

# test_gpu_network.py:71-72 (fp32), :107 (the fp16-operand modes on sr3_tiny / cmde_tiny): net tolerance
NET_TOL = {'fp32': 1e-4, 'fp16x3': 1e-4, 'fp16f8': 3e-4, 'fp16': 2e-2}
_MODELS = {}


def dev():
    return torch.device('cuda:0')


def rel(a, b, floor=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-30)


def model_for(case, precision='fp32', dropout=None):
    key = (case, precision, dropout)
    if key not in _MODELS:
        from conditional_score_diffusion_amd.models import utils as mutils
        cfg = wc.make_config(case, precision)
        if dropout is not None:
            cfg.model.dropout = dropout
        p = wc.params(cfg)
        model = mutils.create_model(cfg)
        missing = model.load_state_dict(p)
        assert not missing.missing_keys and not missing.unexpected_keys
        _MODELS[key] = (cfg, p, model.to(dev()).eval())
    return _MODELS[key]


def sdes_for(cfg):
    from conditional_score_diffusion_amd import sde_lib
    m = cfg.model
    if m.name == 'ddpm_paired':
        return {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
    if m.name == 'ddpm':
        return sde_lib.VESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales)
    return sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales)


def forward_args(case, cfg, j=0, B=wc.B):
    """(x, y, labels) on the GPU for forward time j, the first B samples"""
    sde = sdes_for(cfg)
    x, t = wc.forward_inputs(case)[j]
    y = wc.case_y(case)
    labels = sde.marginal_prob(x, t)[1] if cfg.model.name == 'ddpm' else t * (cfg.model.num_scales - 1)
    return x[:B].contiguous().to(dev()), (y[:B].contiguous().to(dev()) if y is not None else None), labels[:B].contiguous().to(dev())


# ---- forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', list(NET_TOL))
@pytest.mark.parametrize('case', list(wc.CASES))
def test_forward_and_score_vs_fixture(case, precision):
    """network output and score against the reference (test_gpu_network.test_forward_and_score_vs_golden: rel < 1e-4 in fp32 and
    fp16x3; test_fp16_mfma_modes_vs_golden's net bounds for fp16f8 / fp16).  W6 runs the fused wide first layer in the fp16 modes."""
    from conditional_score_diffusion_amd.models import utils as mutils
    g = wc.golden()
    cfg, p, model = model_for(case, precision)
    sde = sdes_for(cfg)
    for j, (x, t) in enumerate(wc.forward_inputs(case)):
        if j and case in wc.ONE_TIME_CASES:
            break
        xd, yd, labels = forward_args(case, cfg, j)
        with torch.no_grad():
            net = wc.call(model, cfg, xd, yd, labels)
            if cfg.model.name == 'ddpm':
                score = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)(xd, t.to(dev()))
            else:
                sfn = mutils.get_conditional_score_fn(mutils.get_score_fn(sde, model, conditional=True, train=False, continuous=True), 'x')
                score = sfn(xd, yd, t.to(dev()))
        e_net = rel(net.cpu().numpy(), g['%s_net%d' % (case, j)])
        print('%s %s t[%d]: net %.3e' % (case, precision, j, e_net))
        assert e_net < NET_TOL[precision], (case, precision, j, e_net)
        if case not in wc.ONE_TIME_CASES:
            e_sc = rel(score.cpu().numpy(), g['%s_score%d' % (case, j)])
            print('%s %s t[%d]: score %.3e' % (case, precision, j, e_sc))
            assert e_sc < NET_TOL[precision], (case, precision, j, e_sc)


# ---- the first layer as an operator: stem_wide_kernel beside assemble + generic convolution --------------------------------------------
# fp16x3 / fp16f8: the first layer keeps both operand planes (hi * hi + hi * lo + lo * hi): what is dropped is lo * lo, 2^-22 of a
# product, plus fp32 accumulation over K <= 288 - 1e-5 of max |out| leaves an order of magnitude; fp16: operands rounded to 2^-11
# each, 5e-3 as test_gpu_network.test_unconditional_nf96_first_layer_without_a_condition allows that mode
STEM_TOL = {'fp32': 1e-5, 'fp16x3': 1e-5, 'fp16f8': 1e-5, 'fp16': 5e-3}
STEM_SHAPES = [      # B, Cx, Cy, Cout, S, centered, y noise
    (2, 16, 16, 64, 16, False, True),        # two K steps per tap, 2 tiles per sample, y + sigma z on 16 channels
    (3, 12, 0, 96, 48, False, False),        # one K step (12 -> 16), three cout tiles, 18 tiles per sample, odd batch
    (2, 5, 12, 128, 32, True, True),         # 17 -> 32: the x | y boundary inside a chunk, two cout groups, centered
    (1, 6, 3, 64, 32, False, False),         # 9 -> 16: just over the 8-channel kernel
]


def _stem_case(B, Cx, Cy, Cout, S, seed=5):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy((rs.standard_normal((B, Cx, S, S)) * 3).astype(np.float32))
    y = torch.from_numpy(rs.uniform(0, 1, (B, Cy, S, S)).astype(np.float32)) if Cy else None
    z = torch.from_numpy(rs.standard_normal((B, Cy, S, S)).astype(np.float32)) if Cy else None
    w = torch.from_numpy((rs.standard_normal((Cout, Cx + Cy, 3, 3)) / np.sqrt(9 * (Cx + Cy))).astype(np.float32))
    b = torch.from_numpy((rs.standard_normal(Cout) * 0.1).astype(np.float32))
    return x, y, z, w, b


def _stem_ref(x, y, z, sig, w, b, centered):
    h = x.double() if y is None else torch.cat([x.double(), y.double() + (sig * z.double() if z is not None else 0.)], dim=1)
    if not centered:
        h = 2 * h - 1.
    return F.conv2d(h, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('precision', ['fp16x3', 'fp16f8', 'fp16', 'fp32'])
@pytest.mark.parametrize('B,Cx,Cy,Cout,S,centered,noise', STEM_SHAPES)
def test_first_layer_fused_and_generic_vs_float64(B, Cx, Cy, Cout, S, centered, noise, precision):
    """ops.input_conv: the one-launch wide first layer (fp16-operand modes) and the assemble + generic convolution fallback (every
    mode) against F.conv2d in float64; the fused layer's tile statistics against sums of its own output; both bitwise repeatable"""
    from conditional_score_diffusion_amd import ops
    x, y, z, w, b = _stem_case(B, Cx, Cy, Cout, S)
    sig = 0.37
    ref = _stem_ref(x, y, z if noise else None, sig, w, b, centered)
    d = lambda t: None if t is None else t.to(dev())      # noqa: E731
    kw = dict(y_noise=d(z) if noise else None, y_sigma=sig if noise else 0.0, centered=centered, precision=precision)
    gen = ops.input_conv(d(x), d(y), d(w), d(b), fused=False, **kw)
    e_gen = rel(gen.cpu().numpy(), ref.numpy())
    print('first layer %d+%d -> %d at %d^2 %s: generic %.3e' % (Cx, Cy, Cout, S, precision, e_gen))
    assert e_gen < STEM_TOL[precision]
    assert torch.equal(gen, ops.input_conv(d(x), d(y), d(w), d(b), fused=False, **kw))
    if precision == 'fp32':
        with pytest.raises(RuntimeError, match='fused first layer does not cover'):      # a missing kernel is an error, never a fall-back
            ops.input_conv(d(x), d(y), d(w), d(b), fused=True, **kw)
        return
    out, stats = ops.input_conv(d(x), d(y), d(w), d(b), fused=True, want_stats=True, **kw)
    e_fused = rel(out.cpu().numpy(), ref.numpy())
    print('first layer %d+%d -> %d at %d^2 %s: fused %.3e' % (Cx, Cy, Cout, S, precision, e_fused))
    assert e_fused < STEM_TOL[precision]
    out2, stats2 = ops.input_conv(d(x), d(y), d(w), d(b), fused=True, want_stats=True, **kw)
    assert torch.equal(out, out2) and torch.equal(stats, stats2)
    # tile statistics: (sum, sum of squares) of every 16 x 8 tile of the written tensor, tiles row-major inside a sample
    o = out.double().cpu().reshape(B, S // 8, 8, S // 16, 16, Cout)
    want = torch.stack([o.sum(dim=(2, 4)), (o * o).sum(dim=(2, 4))], dim=-1).reshape(B * (S // 8) * (S // 16), Cout, 2)
    assert rel(stats.cpu().numpy(), want.numpy()) < 1e-5      # (fp32 partial sums over 32 pixels per lane, fp64 across the waves)


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
def _pc_sampler(cfg, sde):
    from conditional_score_diffusion_amd.sampling import conditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    xs = (wc.B,) + tuple(cfg.data.shape_x)
    return conditional.get_pc_conditional_sampler(sde, xs, get_predictor(cfg.sampling.predictor), get_corrector(cfg.sampling.corrector),
                                                  snr=cfg.sampling.snr, p_steps=wc.P_STEPS, c_steps=1, continuous=True, denoise=True, eps=1e-5)


def _pc_step_by_step(cfg, sde, model, y, tape):
    """the loop of sampling/conditional.py's step-by-step sampler on a tape: corrector then predictor, a fresh y_t per update for the
    two-SDE pair"""
    from conditional_score_diffusion_amd.sampling import conditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    c_sde = sde['x'] if isinstance(sde, dict) else sde
    pred = lambda **k: conditional.conditional_shared_predictor_update_fn(      # noqa: E731
        sde=sde, predictor=get_predictor(cfg.sampling.predictor), probability_flow=False, continuous=True, **k)
    corr = lambda **k: conditional.conditional_shared_corrector_update_fn(      # noqa: E731
        sde=sde, corrector=get_corrector(cfg.sampling.corrector), continuous=True, snr=cfg.sampling.snr, n_steps=1, **k)
    with _Tape(tape[1:]) as tp, torch.no_grad():
        x = (tape[0] * c_sde.sigma_max).to(dev())
        ts = torch.linspace(c_sde.T, 1e-5, wc.P_STEPS)
        for i in range(wc.P_STEPS):
            vec_t = torch.ones(wc.B, device=dev()) * ts[i]
            for fn in (corr, pred):
                y_in = y
                if isinstance(sde, dict):
                    std = sde['y'].marginal_prob(y, vec_t)[1]
                    y_in = y + torch.randn_like(y) * std[:, None, None, None]
                x, x_mean = fn(x=x, y=y_in, t=vec_t, model=model)
        assert tp.i == len(tape) - 1
    return x_mean


@pytest.mark.parametrize('case', wc.SAMPLER_CASES)
def test_pc_sampling_vs_fixture_and_step_by_step(case):
    """3-step fused PC sampling with a noise tape against the reference run (max-abs / sigma_max < 2e-4:
    test_gpu_network.test_pc_trajectory_vs_golden) and against the step-by-step loop on the same tape (< 1e-5 of sigma_max).
    W1: the two-SDE VE pair - the y perturbation covers 16 channels; W3: cVESDE"""
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    g = wc.golden()
    cfg, p, model = model_for(case)
    sde = sdes_for(cfg)
    y = wc.case_y(case).to(dev())
    assert fused.fusable(model, sde, get_predictor(cfg.sampling.predictor), get_corrector(cfg.sampling.corrector), 1, False, True)
    tape = wc.pc_tape(case)
    res, _ = _pc_sampler(cfg, sde)(model, y, noise_tape=tape)
    smax = cfg.model.sigma_max_x
    err = rel(res.cpu().numpy(), g[case + '_pc'], floor=smax)
    step = _pc_step_by_step(cfg, sde, model, y, tape)
    e_step = float((res - step).abs().max()) / smax
    print('%s: fused PC vs reference %.3e, vs step by step %.3e' % (case, err, e_step))
    assert err < 2e-4, (case, err)
    assert e_step < 1e-5, (case, e_step)


# ---- inpainting ----------------------------------------------------------------------------------------------------------------------
def test_haar_mask_inpainting_on_the_device_loop():
    """W2 with the Haar mask [1, 12, 1, 1] (the first three channels known) at its real width: the device loop against the reference's
    get_pc_inpainter run (test_gpu_inpaint_fused.test_device_loop_vs_the_reference_run: <= 2e-4 sigma_max, known channels exact) and
    against the step-by-step loop with the reference's blend in torch (test_device_loop_matches_the_step_by_step_classes: < 1e-5)"""
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import unconditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    g = wc.golden()
    cfg, data, mask, tape = wc.inpaint_inputs()
    _, p, model = model_for('W2')
    sde = sde_lib.VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, wc.INPAINT_N)
    P, C = get_predictor('reverse_diffusion'), get_corrector('langevin')
    fn = unconditional.get_pc_inpainter(sde, P, C, snr=0.15, n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-5,
                                        device_loop=True)
    x, info = fn(model, data.to(dev()), mask.to(dev()), noise_tape=tape)
    x = x.cpu()
    err = float(np.abs(x.numpy() - g['W2_inpaint']).max())
    assert float(((x - data) * mask).abs().max()) == 0.0           # a 0/1 mask returns the known channels exactly
    assert err <= 2e-4 * float(cfg.model.sigma_max_x), err
    # step by step on the same tape (sampling/unconditional.py:268-271's blend in plain torch)
    sfn = mutils.get_score_fn(sde, model, conditional=False, continuous=True)
    data_d, mask_d = data.to(dev()), mask.to(dev())
    with _Tape(tape[1:]) as tp, torch.no_grad():
        pred, corr = P(sde, sfn, False), C(sde, sfn, 0.15, 1)
        xs = data_d * mask_d + (tape[0] * sde.sigma_max).to(dev()) * (1. - mask_d)
        ts = torch.linspace(sde.T, 1e-5, wc.INPAINT_N)
        for i in range(wc.INPAINT_N):
            vec_t = torch.ones(wc.B, device=dev()) * ts[i]
            for obj in (corr, pred):
                xs, x_mean = obj.update_fn(xs, vec_t)
                mean, std = sde.marginal_prob(data_d, vec_t)
                noisy = mean + torch.randn_like(xs) * std[:, None, None, None]
                xs = xs * (1. - mask_d) + noisy * mask_d
                x_mean = xs * (1. - mask_d) + mean * mask_d
        assert tp.i == len(tape) - 1
    e_step = rel(x_mean.cpu().numpy(), x.numpy(), floor=1.0)
    print('W2 inpainting: vs reference %.3e (sigma_max %.1f), vs step by step %.3e' % (err, cfg.model.sigma_max_x, e_step))
    assert e_step < 1e-5


# ---- training ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', wc.TRAIN_CASES)
def test_planned_training_gradients_vs_reference(case):
    """loss.backward() through the planned training graph: the loss and every parameter gradient against the reference's autograd
    (test_oracle_golden.check_grads_vs_fixture with tol 1e-3, as test_gpu_training.test_training_loss_and_grads_vs_reference), and the
    eval-mode input gradient d_x against the reference's (test_gpu_input_grad.TOL = 1e-3)"""
    from conditional_score_diffusion_amd import losses
    from test_oracle_golden import check_grads_vs_fixture
    g = wc.golden()
    cfg, x, y, u, tape = wc.grad_inputs(case)
    _, p, model = model_for(case, 'fp32', dropout=0.0)
    assert model.train_executor == 'planned'
    sde = sdes_for(cfg)
    fn = losses.get_general_sde_loss_fn(sde, True, True, True, True, True)
    it = iter(tape)
    o_rand, o_like = torch.rand, torch.randn_like
    torch.rand = lambda *a, **k: u.clone()
    torch.randn_like = lambda t, **k: next(it).to(t.device)
    model.zero_grad()
    try:
        loss = fn(model, (y.to(dev()), x.to(dev())))
    finally:
        torch.rand, torch.randn_like = o_rand, o_like
    assert model.training and loss.requires_grad
    loss.backward()
    grads = {k: v.grad for k, v in model.named_parameters()}
    worst = check_grads_vs_fixture(g, case, float(loss.detach()), grads, 1e-3)
    model.zero_grad()
    model.eval()
    _, x, y, labels, w = wc.dx_inputs(case)
    xg = x.to(dev()).requires_grad_(True)
    out = wc.call(model, cfg, xg, y.to(dev()), labels.to(dev()))
    gx, = torch.autograd.grad((out * w.to(dev())).sum(), xg)
    e_dx = rel(gx.cpu().numpy(), g[case + '_dx'])
    print('%s: worst sampled gradient error %.3e, d_x %.3e' % (case, worst, e_dx))
    assert e_dx <= 1e-3, (case, e_dx)


# ---- likelihood ----------------------------------------------------------------------------------------------------------------------
def test_fused_likelihood_rhs_matches_the_generic_path():
    """one evaluation of the fused probability-flow right-hand side on W2 (VESDE) - the planned forward, the input-only backward and
    csd_pf_ode_rhs - against the generic autograd path, drift and divergence estimate, at test_gpu_likelihood.py's 1e-3"""
    from conditional_score_diffusion_amd import likelihood, sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from test_gpu_likelihood import Generic
    cfg, p, model = model_for('W2')
    sde = sde_lib.VESDE(0.01, 5.0, 1000)
    rs = np.random.RandomState(17)
    x = torch.from_numpy(rs.uniform(0, 1, size=(wc.B,) + tuple(cfg.data.shape_x)).astype(np.float32)).to(dev())
    e = torch.from_numpy((rs.randint(0, 2, size=tuple(x.shape)) * 2 - 1).astype(np.float32)).to(dev())
    t = 0.4
    state = np.concatenate([x.cpu().numpy().reshape(-1).astype(np.float64), np.zeros(wc.B)])
    assert likelihood._fused_supported(model, sde, False)
    with torch.no_grad():
        rhs = likelihood._FusedRHS(model, sde, x, None, e, False)
        try:
            got = rhs(t, state)
        finally:
            rhs.close()
    generic = Generic(model)

    def drift_fn(xx, tt):
        return sde.reverse(mutils.get_score_fn(sde, generic, train=False, continuous=True), probability_flow=True).sde(xx, tt)[0]

    vec_t = torch.ones(wc.B, device=dev()) * t
    with torch.no_grad():
        drift = drift_fn(x, vec_t).reshape(-1).double().cpu().numpy()
    div = likelihood.get_div_fn(drift_fn)(x, vec_t, e).double().cpu().numpy()
    n = drift.size
    e_drift, e_div = rel(got[:n], drift), rel(got[n:], div)
    print('W2 likelihood rhs: drift %.3e, divergence %.3e' % (e_drift, e_div))
    assert e_drift <= 1e-3 and e_div <= 1e-3


# ---- determinism, batch position, caller buffers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', ['W1', 'W2', 'W3', 'W4', 'W5', 'W6'])
def test_bitwise_repeatable_and_independent_of_the_batch(case, precision):
    cfg, p, model = model_for(case, precision)
    x, y, labels = forward_args(case, cfg)
    x1, y1, l1 = forward_args(case, cfg, B=1)
    with torch.no_grad():
        a = wc.call(model, cfg, x, y, labels)
        b = wc.call(model, cfg, x, y, labels)
        one = wc.call(model, cfg, x1, y1, l1)
    assert torch.equal(a, b)
    assert torch.equal(a[:1], one)


def _two_fills(run, setup=None):
    """run() under tests/guarded.py's seam with the buffers pre-filled with 0x00 and with 0xFF: finite, bitwise equal results, every
    guard intact, no byte buffer of a size that no csd_*_bytes entry declared"""
    outs = []
    for fill in (0x00, 0xFF):
        with guarded.seam(fill) as rec:
            if setup is not None:
                setup()
            got = run()
            torch.cuda.synchronize()
            got = {k: v.detach().cpu().clone() for k, v in got.items()}
        rec.check_guards()
        assert rec.checks, 'no buffer of this run came through the seam'
        rec.assert_sized_by([])
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), 'fill 0x%02X: %s is not finite' % (fill, k)
        outs.append(got)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), '%s depends on the previous contents of a buffer' % k
    return outs[0]


@pytest.mark.parametrize('case,precision', [('W1', 'fp32'), ('W1', 'fp16x3'), ('W4', 'fp16x3'), ('W3', 'fp16'), ('W5', 'fp16x3'), ('W5', 'fp16'),
                                            ('W6', 'fp16x3'), ('W6', 'fp16f8')])
def test_forward_does_not_depend_on_what_the_buffers_held(case, precision):
    """packed weights, workspace and output between guards, filled with 0x00 / 0xFF: the padded input channels and the padded weights
    are written, not assumed (W6: by the fused wide first layer)"""
    cfg, p, model = model_for(case, precision)
    x, y, labels = forward_args(case, cfg)

    def run():
        with torch.no_grad():
            return {'out': wc.call(model, cfg, x, y, labels)}
    out = _two_fills(run, setup=lambda: guarded.reset_model_buffers(model))['out']
    assert rel(out.numpy(), wc.golden()[case + '_net0']) < NET_TOL[precision]
    guarded.reset_model_buffers(model)


def test_first_layer_operator_does_not_depend_on_what_its_buffers_held():
    from conditional_score_diffusion_amd import ops
    B, Cx, Cy, Cout, S = 2, 5, 12, 128, 32
    x, y, z, w, b = (None if t is None else t.to(dev()) for t in _stem_case(B, Cx, Cy, Cout, S))

    def run():
        out, stats = ops.input_conv(x, y, w, b, y_noise=z, y_sigma=0.2, precision='fp16x3', fused=True, want_stats=True)
        return {'out': out, 'stats': stats, 'generic': ops.input_conv(x, y, w, b, y_noise=z, y_sigma=0.2, precision='fp16x3', fused=False)}
    _two_fills(run)


def test_sampling_inpainting_and_training_do_not_depend_on_what_the_buffers_held():
    """PC scratch, workspace, packed weights, the training workspace and every result between guards: 3-step PC sampling on W1,
    device-loop inpainting on W2, the planned training step and the input gradient on W3"""
    from conditional_score_diffusion_amd import losses, sde_lib
    from conditional_score_diffusion_amd.sampling import unconditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    cfg1, _, m1 = model_for('W1')
    sde1, y1, tape1 = sdes_for(cfg1), wc.case_y('W1').to(dev()), wc.pc_tape('W1')
    _two_fills(lambda: {'x': _pc_sampler(cfg1, sde1)(m1, y1, noise_tape=tape1)[0]}, setup=lambda: guarded.reset_model_buffers(m1))
    cfg2, data, mask, tape2 = wc.inpaint_inputs()
    _, _, m2 = model_for('W2')
    fn = unconditional.get_pc_inpainter(sde_lib.VESDE(cfg2.model.sigma_min_x, cfg2.model.sigma_max_x, wc.INPAINT_N),
                                        get_predictor('reverse_diffusion'), get_corrector('langevin'), snr=0.15, n_steps=1,
                                        continuous=True, denoise=True, eps=1e-5, device_loop=True)
    _two_fills(lambda: {'x': fn(m2, data.to(dev()), mask.to(dev()), noise_tape=tape2)[0]}, setup=lambda: guarded.reset_model_buffers(m2))
    cfg3, x, y, u, tape3 = wc.grad_inputs('W3')
    _, _, m3 = model_for('W3', 'fp32', dropout=0.0)
    loss_fn = losses.get_general_sde_loss_fn(sdes_for(cfg3), True, True, True, True, True)

    def train():
        it = iter(tape3)
        o_rand, o_like = torch.rand, torch.randn_like
        torch.rand = lambda *a, **k: u.clone()
        torch.randn_like = lambda t, **k: next(it).to(t.device)
        m3.train()
        m3.zero_grad()
        try:
            loss = loss_fn(m3, (y.to(dev()), x.to(dev())))
        finally:
            torch.rand, torch.randn_like = o_rand, o_like
        loss.backward()
        got = {'loss': loss.detach().reshape(1)}
        got.update({k: v.grad.clone() for k, v in m3.named_parameters()})
        m3.eval()
        xg = x.to(dev()).requires_grad_(True)
        out = wc.call(m3, cfg3, xg, y.to(dev()), torch.tensor([12.25, 871.0], device=dev()))
        got['dx'], = torch.autograd.grad(out.square().sum(), xg)
        return got
    _two_fills(train, setup=lambda: guarded.reset_model_buffers(m3))
    for m in (m1, m2, m3):
        guarded.reset_model_buffers(m)
        m.zero_grad()
