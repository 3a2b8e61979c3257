"""-m gpu: NCSN++ on images with more than 8 channels (9 .. 32) and ncsnpp_2xSR through every layer the 8-channel networks reach -
planned inference, the NCSN++ operators at the new widths and pitches, the fused PC loop, the planned training graph and its input
gradient and the cascades - against the reference's fixture
tests/golden/ncsnpp_wide.npz (tools/make_ncsnpp_wide_goldens.py) on the cases of tests/ncsnpp_wide_cases.py.

The wide networks are the paired ones (ncsnpp_paired, ncsnpp_2xSR): the unconditional ncsnpp keeps its limit of 8 channels, so
inpainting and the likelihood, which exist for unconditional networks only, are not here.

Bounds are those of the 8-channel NCSN++ and wide DDPM tests that each test mirrors; each test names its source."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import ncsnpp_wide_cases as nw  # noqa: E402
import score_oracle as so  # noqa: E402
import sr_cases as sc  # noqa: E402
from test_gpu_steps import _Tape  # noqa: E402

# tests/test_gpu_wide.py:19 NET_TOL (test_gpu_network.py:71-72,107): the wide networks' forward at both ends of the noise schedule
NET_TOL = {'fp32': 1e-4, 'fp16x3': 1e-4, 'fp16f8': 3e-4, 'fp16': 2e-2}
TRAJECTORY = 1e-3             # tests/test_gpu_sr.py:22, tests/test_gpu_cascade.py:184 (cascade_cases.TRAJECTORY)
_MODELS = {}


def dev():
    return torch.device('cuda:0')


def rel(a, b, floor=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-30)


def load(cfg, p):
    from conditional_score_diffusion_amd.models import utils as mutils
    model = mutils.create_model(cfg)
    res = model.load_state_dict(p)
    assert not res.missing_keys and not res.unexpected_keys
    return model.to(dev()).eval()


def model_for(case, precision='fp32', dropout=None, name=None):
    key = (case, precision, dropout, name)
    if key not in _MODELS:
        cfg = nw.make_config(case, precision, name=name)
        if dropout is not None:
            cfg.model.dropout = dropout
        p = nw.params(nw.make_config(case))
        _MODELS[key] = (cfg, p, load(cfg, p))
    return _MODELS[key]


def sdes_for(cfg, paired):
    from conditional_score_diffusion_amd import sde_lib
    m = cfg.model
    if paired:
        return {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
    return sde_lib.VESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales)


def forward_args(case, cfg, j=0, B=nw.B):
    """(x, y, labels) on the GPU for forward time j, the first B samples"""
    x, t = nw.forward_inputs(case)[j]
    y = nw.case_y(case)
    labels = nw.labels_of(case, cfg, t)
    return x[:B].contiguous().to(dev()), (y[:B].contiguous().to(dev()) if y is not None else None), labels[:B].contiguous().to(dev())


def reference_net(case, j):
    """the fixture's network output"""
    return nw.golden()['%s_net%d' % (case, j)]


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', list(NET_TOL))
@pytest.mark.parametrize('case', list(nw.CASES))
def test_forward_and_score_vs_fixture(case, precision):
    """network output and score against the reference (tests/test_gpu_wide.py:69 test_forward_and_score_vs_fixture, NET_TOL of :19).
    The reference's score is its network output over sigma_x(t) (nw.score_of, asserted against the reference's score function where
    the fixture is written): the file holds the outputs only"""
    from conditional_score_diffusion_amd.models import utils as mutils
    g = nw.golden()
    cfg, p, model = model_for(case, precision)
    paired = nw.is_paired(case)
    sde = sdes_for(cfg, paired)
    for j, (x, t) in enumerate(nw.forward_inputs(case)):
        if j and case in nw.ONE_TIME_CASES:
            break
        xd, yd, labels = forward_args(case, cfg, j)
        with torch.no_grad():
            net = nw.call(model, case, xd, yd, labels)
            if paired:
                sfn = mutils.get_conditional_score_fn(mutils.get_score_fn(sde, model, conditional=True, train=False, continuous=True), 'x')
                score = sfn(xd, yd, t.to(dev()))
            else:
                score = mutils.get_score_fn(sde, model, conditional=False, train=False, continuous=True)(xd, t.to(dev()))
        e_net = rel(net.cpu().numpy(), reference_net(case, j))
        print('%s %s t[%d]: net %.3e' % (case, precision, j, e_net))
        assert e_net < NET_TOL[precision], (case, precision, j, e_net)
        if case not in nw.ONE_TIME_CASES:
            e_sc = rel(score.cpu().numpy(), nw.score_of(case, cfg, torch.from_numpy(g['%s_net%d' % (case, j)]), t).numpy())
            print('%s %s t[%d]: score %.3e' % (case, precision, j, e_sc))
            assert e_sc < NET_TOL[precision], (case, precision, j, e_sc)


@pytest.mark.parametrize('case', ['N1', 'N2', 'N2n', 'N3', 'N4'])
def test_planned_graph_vs_the_operator_classes(case):
    """ncsnpp_ops / ncsnpp_paired_ops (torch.cat + ops.conv2d: width-agnostic) on the same parameters: against the fixture at the
    bound the planned class has (tests/test_ncsnpp.py:95 holds both classes to one bound) and against the planned graph"""
    cfg, p, model = model_for(case, 'fp32')
    _, _, twin = model_for(case, 'fp32', name=cfg.model.name + '_ops')
    for j in range(1 if case in nw.ONE_TIME_CASES else 2):
        xd, yd, labels = forward_args(case, cfg, j)
        with torch.no_grad():
            a, b = nw.call(model, case, xd, yd, labels), nw.call(twin, case, xd, yd, labels)
        e_ops, e_ab = rel(b.cpu().numpy(), reference_net(case, j)), rel(a.cpu().numpy(), b.cpu().numpy())
        print('%s t[%d]: operator class vs fixture %.3e, planned vs operator class %.3e' % (case, j, e_ops, e_ab))
        assert e_ops < NET_TOL['fp32'] and e_ab < NET_TOL['fp32']


@pytest.mark.parametrize('precision', ['fp16x3', 'fp32'])
def test_2xsr_is_bitwise_the_paired_network_on_a_squeezed_input(precision):
    """tests/test_gpu_sr.py:95 test_forward_is_bitwise_the_unsqueezed_network_on_a_squeezed_input: the squeeze is addressing - in the
    assemble pass (kept beside the input pyramid) and in the head's residual + scattered store"""
    cfg, _, model = model_for('N5', precision)
    _, _, twin = model_for('N5', precision, name='ncsnpp_paired')
    for j in range(2):
        x, y, labels = forward_args('N5', cfg, j)
        with torch.no_grad():
            out = model({'x': x, 'y': y}, labels)
            ref = twin({'x': sc.squeeze(x).contiguous(), 'y': y}, labels)
        assert tuple(out['x'].shape) == tuple(x.shape)
        assert torch.equal(out['x'], sc.unsqueeze(ref['x'])), (precision, j)
        assert torch.equal(out['y'], ref['y']), (precision, j)


def test_2xsr_gradients_are_bitwise_the_paired_networks():
    """tests/test_gpu_sr.py:109 test_gradients_are_bitwise_the_unsqueezed_networks: training-mode parameter gradients (dropout 0) and
    the eval-mode d_x; the boundary's gather and scatter only move elements"""
    cfg, _, model = model_for('N5', 'fp32', dropout=0.0)
    _, _, twin = model_for('N5', 'fp32', dropout=0.0, name='ncsnpp_paired')
    xs, ys = nw.shapes('N5')
    rs = np.random.RandomState(3)
    x = torch.from_numpy(np.random.RandomState(7).uniform(0, 1, size=xs).astype(np.float32)).to(dev())
    wx, wy = (torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev()) for s in (xs, ys))
    y, labels = nw.case_y('N5').to(dev()), torch.tensor([12.25, 871.0], device=dev())
    grads, dxs = [], []
    for net, xin, w in ((model, x, wx), (twin, sc.squeeze(x).contiguous(), sc.squeeze(wx).contiguous())):
        assert net.train_executor == 'planned'
        net.train()
        net.zero_grad()
        out = net({'x': xin, 'y': y}, labels)
        ((out['x'] * w).sum() + (out['y'] * wy).sum()).backward()
        grads.append({k: v.grad.clone() for k, v in net.named_parameters() if v.requires_grad})
        net.zero_grad()
        net.eval()
        xg = xin.clone().requires_grad_(True)
        out = net({'x': xg, 'y': y}, labels)
        dxs.append(torch.autograd.grad((out['x'] * w).sum() + (out['y'] * wy).sum(), xg)[0])
    assert list(grads[0]) == list(grads[1]) and any(float(v.abs().max()) > 0 for v in grads[0].values())
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
    assert tuple(dxs[0].shape) == xs and float(dxs[0].abs().max()) > 0
    assert torch.equal(dxs[0], sc.unsqueeze(dxs[1]))


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', ['N1', 'N2', 'N2n', 'N3', 'N4', 'N5', 'N6', 'N6s'])
def test_bitwise_repeatable_and_independent_of_the_batch(case, precision):
    """tests/test_gpu_wide.py:338: a repeated call and B = 2 against two B = 1 calls, bit for bit"""
    cfg, p, model = model_for(case, precision)
    x, y, labels = forward_args(case, cfg)
    with torch.no_grad():
        a = nw.call(model, case, x, y, labels)
        b = nw.call(model, case, x, y, labels)
        ones = [nw.call(model, case, x[i:i + 1].contiguous(), y[i:i + 1].contiguous() if y is not None else None,
                        labels[i:i + 1].contiguous()) for i in range(nw.B)]
    assert torch.equal(a, b)
    assert torch.equal(a, torch.cat(ones))


# ---- 2. the NCSN++ operators at the new widths and pitches -------------------------------------------------------------------------------
def _pyr_ref64(x, w, b, res, taps, scale):
    """tests/test_gpu_ncsnpp_residual.py:18 pyr_ref64: layerspp.Downsample(with_conv=True) in float64 on NCHW"""
    x, w = x.double(), w.double()
    C = x.shape[1]
    if taps is None:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    else:
        k = torch.tensor(taps, dtype=torch.float64)
        k2 = torch.outer(k, k)
        k2 = torch.flip(k2 / k2.sum(), [0, 1])
        y = F.conv2d(F.conv2d(F.pad(x, (2, 2, 2, 2)), k2[None, None].repeat(C, 1, 1, 1), groups=C), w, stride=2)
    return (y + b.double()[None, :, None, None] + res.double()) * scale


@pytest.mark.parametrize('taps', [(1, 3, 3, 1), None], ids=['fir1331', 'nofir'])
@pytest.mark.parametrize('Cin,H', [(9, 4), (12, 6), (17, 4), (32, 6), (12, 16)])
def test_fir_pyr_conv_under_the_padded_pixel_stride(Cin, H, taps):
    """csd_fir_pyr_conv at level 0 of a wide network: Cin channels under the pixel stride of the assembled input (16 or 32), the padding
    channels poisoned with NaN - they must not be read; bound of tests/test_gpu_ncsnpp_residual.py:59"""
    from conditional_score_diffusion_amd import ops
    B, Cout, pix = 2, 32, (Cin + 15) // 16 * 16
    rs = np.random.RandomState(Cin * 7 + H)
    x = torch.from_numpy(rs.standard_normal((B, Cin, H, H)).astype(np.float32) * 2.0)
    w = torch.from_numpy((rs.uniform(-1, 1, (Cout, Cin, 3, 3)) / np.sqrt(9.0 * Cin)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(Cout).astype(np.float32))
    res = torch.from_numpy(rs.standard_normal((B, Cout, H // 2, H // 2)).astype(np.float32))
    xp = torch.full((B, H, H, pix), float('nan'))
    xp[..., :Cin] = x.permute(0, 2, 3, 1)
    scale = 1.0 / np.sqrt(2.0)
    args = (xp.to(dev()), w.to(dev()), b.to(dev()), res.permute(0, 2, 3, 1).contiguous().to(dev()))
    got = ops.fir_pyr_conv(*args, fir_kernel=taps, out_scale=scale)
    again = ops.fir_pyr_conv(*args, fir_kernel=taps, out_scale=scale)
    ref = _pyr_ref64(x, w, b, res, taps, scale).permute(0, 2, 3, 1)
    err = rel(got.cpu().numpy(), ref.numpy())
    print('fir_pyr_conv Cin %d under stride %d, H %d, %s: %.3e' % (Cin, pix, H, 'fir' if taps else 'no fir', err))
    assert tuple(got.shape) == (B, H // 2, H // 2, Cout)
    assert err < 2e-6 * max(1.0, np.sqrt(9.0 * Cin) / 8.0), err
    assert torch.equal(got, again)
    if pix == Cin:
        return
    dense = ops.fir_pyr_conv(x.permute(0, 2, 3, 1).contiguous().to(dev()), *args[1:], fir_kernel=taps, out_scale=scale)
    assert torch.equal(got, dense)                 # the pitch is addressing: the bits of the dense source


@pytest.mark.parametrize('up', [False, True], ids=['down', 'up'])
@pytest.mark.parametrize('C', [9, 15, 17, 32])
def test_fir_resample_at_pitches_that_are_no_multiple_of_four(C, up):
    """the NHWC FIR resample of the pyramids (pyramid_upsample at the output width, pyramid_downsample of the padded input) against
    score_oracle.upfirdn2d_ref with the pads of upsample_2d / downsample_2d; odd sides where upsampling, a ragged 6 x 10 map where
    downsampling.  fp32 sums of at most 16 products: 1e-6 of the maximum (tests/test_gpu_cascade.py:22 BAND_TOL, the four-term chains)"""
    from conditional_score_diffusion_amd import ops
    B, H, W = 2, (5 if up else 6), (7 if up else 10)
    x = torch.from_numpy(np.random.RandomState(C + up).standard_normal((B, C, H, W)).astype(np.float32))
    taps = (1, 3, 3, 1)
    k = so.fir_kernel_2d(taps, 4.0 if up else 1.0).double()
    ref = so.upfirdn2d_ref(x.double(), k, up=2, pad=(2, 1)) if up else so.upfirdn2d_ref(x.double(), k, down=2, pad=(1, 1))
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev())
    got = ops.fir_resample_nhwc(xd, taps, up=up)
    err = rel(got.permute(0, 3, 1, 2).cpu().numpy(), ref.numpy())
    print('fir resample %s C %d: %.3e' % ('up' if up else 'down', C, err))
    assert tuple(got.shape) == ((B, 2 * H, 2 * W, C) if up else (B, H // 2, W // 2, C))
    assert err < 1e-6
    assert torch.equal(got, ops.fir_resample_nhwc(xd, taps, up=up))
    # a source that is not 16-byte aligned (a C caller's offset pointer) takes the scalar form: the same sums in the same order
    flat = torch.empty(xd.numel() + 1, device=dev())
    off = flat[1:].view(xd.shape)
    off.copy_(xd)
    assert off.data_ptr() % 16 == 4 and torch.equal(ops.fir_resample_nhwc(off, taps, up=up), got)
    # zeros in, zeros out: the padding channels of an assembled input stay exact zeros through every level of the pyramid
    z = xd.clone()
    z[..., C // 2:] = 0.
    assert int((ops.fir_resample_nhwc(z, taps, up=up)[..., C // 2:] != 0).sum()) == 0


@pytest.mark.parametrize('Cx,Cy', [(9, 0), (12, 3), (5, 12), (16, 16)])
def test_first_layer_operator_at_the_combine_widths(Cx, Cy):
    """ops.input_conv, assemble pass + generic convolution (what the wide NCSN++ plans run), at the widths of the cases, fp32 and
    fp16x3 against float64: tests/test_gpu_wide.py:100 STEM_TOL"""
    from conditional_score_diffusion_amd import ops
    B, S, Cout = 2, 16, 32
    rs = np.random.RandomState(5 + Cx)
    x = torch.from_numpy((rs.standard_normal((B, Cx, S, S)) * 3).astype(np.float32))
    y = torch.from_numpy(rs.uniform(0, 1, (B, Cy, S, S)).astype(np.float32)) if Cy else None
    w = torch.from_numpy((rs.standard_normal((Cout, Cx + Cy, 3, 3)) / np.sqrt(9 * (Cx + Cy))).astype(np.float32))
    b = torch.from_numpy((rs.standard_normal(Cout) * 0.1).astype(np.float32))
    h = 2 * (torch.cat([x, y], dim=1) if Cy else x).double() - 1.
    ref = F.conv2d(h, w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    d = lambda t: None if t is None else t.to(dev())      # noqa: E731
    for precision in ('fp32', 'fp16x3'):
        got = ops.input_conv(d(x), d(y), d(w), d(b), fused=False, precision=precision)
        e = rel(got.cpu().numpy(), ref.numpy())
        print('first layer %d+%d %s: %.3e' % (Cx, Cy, precision, e))
        assert e < 1e-5


# ---- 3. sampling -------------------------------------------------------------------------------------------------------------------------
def _pc_sampler(cfg, sde):
    from conditional_score_diffusion_amd.sampling import conditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    xs = (nw.B,) + tuple(cfg.data.shape_x)
    return conditional.get_pc_conditional_sampler(sde, xs, get_predictor(cfg.sampling.predictor), get_corrector(cfg.sampling.corrector),
                                                  snr=cfg.sampling.snr, p_steps=nw.P_STEPS, c_steps=1, continuous=True, denoise=True, eps=1e-5)


def _pc_step_by_step(cfg, sde, model, y, tape):
    """tests/test_gpu_wide.py:168 _pc_step_by_step: corrector then predictor, a fresh y_t per update"""
    from conditional_score_diffusion_amd.sampling import conditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    pred = lambda **k: conditional.conditional_shared_predictor_update_fn(      # noqa: E731
        sde=sde, predictor=get_predictor(cfg.sampling.predictor), probability_flow=False, continuous=True, **k)
    corr = lambda **k: conditional.conditional_shared_corrector_update_fn(      # noqa: E731
        sde=sde, corrector=get_corrector(cfg.sampling.corrector), continuous=True, snr=cfg.sampling.snr, n_steps=1, **k)
    with _Tape(tape[1:]) as tp, torch.no_grad():
        x = (tape[0] * sde['x'].sigma_max).to(dev())
        ts = torch.linspace(sde['x'].T, 1e-5, nw.P_STEPS)
        for i in range(nw.P_STEPS):
            vec_t = torch.ones(nw.B, device=dev()) * ts[i]
            for fn in (corr, pred):
                std = sde['y'].marginal_prob(y, vec_t)[1]
                x, x_mean = fn(x=x, y=y + torch.randn_like(y) * std[:, None, None, None], t=vec_t, model=model)
        assert tp.i == len(tape) - 1
    return x_mean


@pytest.mark.parametrize('case', nw.SAMPLER_CASES)
def test_pc_sampling_vs_fixture_and_step_by_step(case):
    """3-step fused PC sampling of the two-SDE VE pair on the reference's tape.  N1, N4: tests/test_gpu_wide.py:194 (max-abs /
    sigma_max < 2e-4 against the reference run, < 1e-5 of sigma_max against the step-by-step loop); N5: tests/test_gpu_sr.py:178 (the
    fused loop, the step-by-step loop and the reference within TRAJECTORY of each other)"""
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    g = nw.golden()
    cfg, p, model = model_for(case)
    sde = sdes_for(cfg, True)
    y = nw.case_y(case).to(dev())
    assert fused.fusable(model, sde, get_predictor(cfg.sampling.predictor), get_corrector(cfg.sampling.corrector), 1, False, True)
    tape = nw.pc_tape(case)
    res, _ = _pc_sampler(cfg, sde)(model, y, noise_tape=tape)
    assert tuple(res.shape) == nw.shapes(case)[0]
    step = _pc_step_by_step(cfg, sde, model, y, tape)
    smax = cfg.model.sigma_max_x
    if case == 'N5':
        e_fused, e_step = rel(res.cpu().numpy(), g[case + '_pc']), rel(step.cpu().numpy(), g[case + '_pc'])
        e_both = rel(res.cpu().numpy(), step.cpu().numpy())
        print('%s: fused vs reference %.3e, step by step vs reference %.3e, fused vs step by step %.3e' % (case, e_fused, e_step, e_both))
        assert e_fused < TRAJECTORY and e_step < TRAJECTORY and e_both < TRAJECTORY
        return
    err = rel(res.cpu().numpy(), g[case + '_pc'], floor=smax)
    e_step = float((res - step).abs().max()) / smax
    print('%s: fused PC vs reference %.3e, vs step by step %.3e' % (case, err, e_step))
    assert err < 2e-4, (case, err)
    assert e_step < 1e-5, (case, e_step)


# ---- 4. training ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', nw.TRAIN_CASES)
def test_planned_training_gradients_vs_reference(case):
    """loss.backward() through the planned training graph (arch 1): the loss and every trained parameter's gradient against the
    reference's autograd - check_grads_vs_fixture with tol 1e-3, as tests/test_gpu_wide.py:262, tests/test_gpu_sr.py:277 and
    test_gpu_training.test_training_loss_and_grads_vs_reference"""
    from conditional_score_diffusion_amd import losses
    from test_oracle_golden import check_grads_vs_fixture
    cfg, x, y, u, tape = nw.grad_inputs(case)
    _, p, model = model_for(case, 'fp32', dropout=0.0)
    assert model.train_executor == 'planned'
    fn = losses.get_general_sde_loss_fn(sdes_for(cfg, True), True, True, True, True, True)
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
    grads = {k: v.grad for k, v in model.named_parameters() if v.requires_grad}
    worst = check_grads_vs_fixture(nw.golden(), case, float(loss.detach()), grads, 1e-3)
    print('%s: loss %.6f, worst sampled gradient error %.3e' % (case, float(loss.detach()), worst))
    model.zero_grad()
    model.eval()


@pytest.fixture
def oracle64(monkeypatch):
    """tests/test_gpu_ncsnpp_residual.py:120: the CPU oracle with its two fp32 constants widened, so that a float64 call stays float64"""
    te, fk = so.timestep_embedding, so.fir_kernel_2d
    monkeypatch.setattr(so, 'timestep_embedding', lambda *a, **k: te(*a, **k).double())
    monkeypatch.setattr(so, 'fir_kernel_2d', lambda *a, **k: fk(*a, **k).double())
    return so


def _oracle64_grads(cfg, p, x, y, labels, w):
    """float64 autograd through oracle/score_oracle.py ncsnpp_forward (pinned to the reference by the fixture): every parameter's
    gradient and d_x of (out * w).sum() - a reference that shares no code with either HIP route"""
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    xr = x.double().requires_grad_(True)
    ref = so.ncsnpp_forward(p64, cfg, torch.cat([xr, y.double().cpu()], dim=1), labels.double().cpu())
    (ref * w.double()).sum().backward()
    return {k: v.grad for k, v in p64.items()}, xr.grad


def _pyramid_keys(ref):
    """the weights of layerspp.Downsample(with_conv=True): a module that holds one 3x3 convolution and no GroupNorm"""
    return [k for k, v in ref.items() if k.endswith('.weight') and v.dim() == 4 and v.shape[-1] == 3 and k.count('.') == 3 and
            k.rsplit('.', 2)[0] + '.GroupNorm_0.weight' not in ref]


def _check_grads(got, ref, what):
    """the per-parameter bound of tests/test_ncsnpp.py:281-282 (test_training_mode_gradients_vs_oracle_autograd)"""
    total = float(np.sqrt(sum(float((ref[k].double() ** 2).sum()) for k in got)))
    for k, g in got.items():
        r = ref[k].double()
        scale = max(float(r.abs().max()), float(r.norm()) / np.sqrt(r.numel()))
        err = float((g.double() - r).abs().max())
        assert err <= 1e-3 * scale + 1e-6 * total / np.sqrt(r.numel()), (what, k, err, scale)


def _planned_vs_operators(make, call, w_seed=2, w_shape=None, oracle=None):
    """tests/test_gpu_ncsnpp_residual.py:173: every parameter gradient and d_x of the planned graph against the operator twin on the
    same parameters, 1e-3 of the gradient's scale; ``oracle(w) -> (gradients, d_x)``: and both routes against float64 autograd over the
    CPU oracle, so that an error the two HIP routes share does not pass"""
    grads, dx = {}, {}
    for executor in ('planned', 'operators'):
        model, x = make()
        model.train_executor = executor
        model.train()
        w = torch.from_numpy(np.random.RandomState(w_seed).standard_normal(w_shape or tuple(x.shape)).astype(np.float32)).to(dev())
        xg = x.to(dev()).requires_grad_(True)
        (call(model, xg) * w).sum().backward()
        grads[executor] = {k: q.grad.detach().cpu().double() for k, q in model.named_parameters() if q.requires_grad}
        dx[executor] = xg.grad.detach().cpu()
    ref = grads['operators']
    total = float(np.sqrt(sum(float((g ** 2).sum()) for g in ref.values())))
    assert set(grads['planned']) == set(ref) and len(ref) > 20
    for k, r in ref.items():
        g = grads['planned'][k]
        scale = max(float(r.abs().max()), float(r.norm()) / np.sqrt(r.numel()))
        assert float((g - r).abs().max()) <= 1e-3 * scale + 1e-6 * total / np.sqrt(r.numel()), (k, float((g - r).abs().max()), scale)
    assert rel(dx['planned'].numpy(), dx['operators'].numpy()) <= 1e-3      # (tests/test_gpu_ncsnpp_residual.py:169)
    if oracle is not None:
        w = torch.from_numpy(np.random.RandomState(w_seed).standard_normal(w_shape or tuple(x.shape)).astype(np.float32))
        ref64, dx64 = oracle(w)
        pyr = _pyramid_keys(ref64)
        assert pyr and all(k in grads['planned'] for k in pyr), pyr
        for route in ('planned', 'operators'):
            _check_grads(grads[route], ref64, route)
            e = rel(dx[route].numpy(), dx64.numpy())
            print('%s: %d gradients (%d pyramid weights) and d_x vs float64 oracle, d_x %.3e' % (route, len(grads[route]), len(pyr), e))
            assert e <= 1e-3, (route, e)                                        # (tests/test_gpu_ncsnpp_residual.py:152)


def test_planned_training_of_the_residual_pyramid_matches_the_operator_twin_and_the_reference_dx(oracle64):
    """N2 (9 + 3 channels, two 'residual' pyramid levels each way): the pyramid's dgrad (nc = 12) and wgrad in the graph against the
    operator twin, and the eval-mode input gradient against the reference's (tests/test_gpu_input_grad.py TOL = 1e-3, as
    tests/test_gpu_wide.py:296)"""
    cfg, x, y, labels, w = nw.dx_inputs('N2')
    cfg.model.dropout = 0.0
    p = nw.params(cfg)
    y, labels = y.to(dev()), labels.to(dev())
    # (against float64 with labels of a few units: at 871 the Fourier argument's fp32 rounding is part of the reference's result -
    # csrc/elementwise.hip fourier_embedding_kernel - and a float64 restatement lies 3e-3 from it)
    small = torch.log(torch.tensor([0.02, 7.5])).to(dev())
    _planned_vs_operators(lambda: (load(cfg, p), x), lambda m, xg: nw.call(m, 'N2', xg, y, small), w_shape=tuple(w.shape),
                          oracle=lambda w_: _oracle64_grads(cfg, p, x, y, small, w_))
    _, _, model = model_for('N2', 'fp32', dropout=0.0)
    xg = x.to(dev()).requires_grad_(True)
    gx, = torch.autograd.grad((nw.call(model, 'N2', xg, y, labels) * w.to(dev())).sum(), xg)
    e_dx = rel(gx.cpu().numpy(), nw.golden()['N2_dx'])
    print('N2: eval-mode d_x vs reference %.3e' % e_dx)
    assert e_dx <= 1e-3


@pytest.mark.parametrize('fir', [True, False], ids=['fir', 'nofir'])
@pytest.mark.parametrize('channels', [9, 17, 32])
def test_residual_pyramid_gradients_at_the_other_widths(channels, fir, oracle64):
    """the 'residual' pyramid's dgrad and wgrad at Cin 9, 17 and 32 (ncsnpp_paired on (channels - 3) + 3, level 0 at 8^2, both tap
    sets), through the planned training graph against the operator twin"""
    import cases
    cfg = cases.make_ncsnpp_config(name='ncsnpp_paired', channels=channels, nf=32, ch_mult=(1, 2), attn_resolutions=(), image_size=8, fir=fir,
                                   embedding_type='positional', progressive='output_skip' if fir else 'none', progressive_input='residual')
    cfg.model.dropout = 0.0
    cfg.data.shape_x, cfg.data.shape_y = [channels - 3, 8, 8], [3, 8, 8]
    p = cases.ncsnpp_params(nw.param_shapes(cfg), 5)
    rs = np.random.RandomState(channels)
    x = torch.from_numpy(rs.uniform(0, 1, size=(2, channels - 3, 8, 8)).astype(np.float32))
    y = torch.from_numpy(rs.uniform(0, 1, size=(2, 3, 8, 8)).astype(np.float32)).to(dev())
    labels = torch.tensor([12.25, 871.0], device=dev())

    def call(m, xg):
        out = m({'x': xg, 'y': y}, labels)
        return torch.cat([out['x'], out['y']], dim=1)
    _planned_vs_operators(lambda: (load(cfg, p), x), call, w_shape=(2, channels, 8, 8),
                          oracle=lambda w_: _oracle64_grads(cfg, p, x, y, labels, w_))


# ---- 5. cascades -------------------------------------------------------------------------------------------------------------------------
def stages_for(flow):
    from conditional_score_diffusion_amd import sde_lib
    out = []
    for k in range(2):
        cfg = nw.stage_config(flow, k, 'fp32')
        key = ('stage', flow, k)
        if key not in _MODELS:
            _MODELS[key] = load(cfg, nw.stage_params(flow, k))
        m = cfg.model
        sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
        out.append((_MODELS[key], sde, cfg))
    return out


def cascade_for(flow, one_call):
    from conditional_score_diffusion_amd.sampling import cascade
    return cascade.get_autoregressive_sampler(stages_for(flow), nw.CASCADE_SPACE[flow], one_call=one_call, p_steps=nw.P_STEPS)


@pytest.mark.parametrize('flow', list(nw.CASCADE_STAGES))
def test_cascade_in_one_call_is_bitwise_the_chained_stages(flow):
    """tests/test_gpu_cascade.py: everything between routes is bitwise - NCSN++ stages in the two conditional coordinate spaces and
    beside a DDPM stage, on the stage tapes and on a seed"""
    lr = nw.lr_input().to(dev())
    tapes = [nw.stage_tape(flow, k) for k in range(2)]
    one, info = cascade_for(flow, True)(lr, return_intermediate_images=True, noise_tapes=tapes)
    two, _ = cascade_for(flow, False)(lr, return_intermediate_images=True, noise_tapes=tapes)
    assert info == [] and len(one) == len(two) == 3 and torch.equal(one[0], lr.cpu())
    for k in range(1, 3):
        assert tuple(one[k].shape) == (nw.B, 3, 8 << k, 8 << k) and bool(torch.isfinite(one[k]).all())
        assert torch.equal(one[k], two[k]), (flow, k)
    a, _ = cascade_for(flow, True)(lr, seed=11)
    b, _ = cascade_for(flow, False)(lr, seed=11)
    assert a.is_cuda and torch.equal(a, b)


def test_bicubic_cascade_of_two_2xsr_stages_vs_the_reference_chain():
    """every stage's image of the one-call cascade within 1e-3 of the stage's sigma_max_x of the reference's samplers chained on the
    stage tapes (tests/test_gpu_cascade.py:172-184)"""
    g = nw.golden()
    lr = nw.lr_input().to(dev())
    images, _ = cascade_for('bicubic', True)(lr, return_intermediate_images=True, noise_tapes=[nw.stage_tape('bicubic', k) for k in range(2)])
    for k in range(2):
        ref = g['bicubic_s%d' % k]
        smax = float(nw.stage_config('bicubic', k).model.sigma_max_x)
        d = float(np.abs(images[k + 1].numpy().astype(np.float64) - ref).max()) / smax
        print('bicubic stage %d: one call vs reference %.3e of sigma_max_x' % (k, d))
        assert tuple(images[k + 1].shape) == tuple(ref.shape) and d < TRAJECTORY, (k, d)
