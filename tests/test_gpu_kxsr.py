"""-m gpu: the direct Kx super-resolution networks (ddpm_KxSR, ncsnpp_KxSR: a paired network behind the bilinear upsample of the
low-resolution y, its y output resized back - csd_unet_config.y_scale, resampling inside the library's boundary kernels) through every
layer the paired networks reach - the resamplers as operators, planned inference, the two-SDE score function, the fused PC loop and its
step forms, planned training and the input gradient - against the reference's fixture tests/golden/kxsr.npz
(tools/make_kxsr_goldens.py) on the cases of tests/kxsr_cases.py, and BITWISE against the paired network with the same parameters that
is fed ops.bilinear_up(y, K) and whose y output goes through ops.bilinear_down: every kernel that resamples uses the same device
functions (csrc/common.h), so the value of a pixel does not depend on the kernel that computed it.

Bounds are those of the tests they mirror; each test names its source.  Worst measured error of each group on the MI355X, next to its
bound (from this file's own prints):

    operators vs F.interpolate in float64, adjoint identity        1.5e-7                       1e-6
    forward vs the fixture, K1 - K4: fp32 / fp16x3                 4.2e-6                       1e-4
                                     fp16f8 (worst: K2 at t = 1e-5) 6.1e-5                       3e-4
                                     fp16 (worst: K3, y output)    2.8e-3                       2e-2
    two-SDE scores vs the fixture, K1 - K4: fp32 / fp16x3          1.9e-6                       1e-4
                                     fp16f8 (worst: K2)            1.3e-5                       3e-4
                                     fp16 (worst: K3)              1.7e-3                       2e-2
    the twin (outputs, gradients, d_x; the first layer with and
    without the y perturbation, nf 64 / 96 / 128)                  bitwise                      bitwise
    fused / step-by-step sampling vs the fixture, each other       3.4e-7 / 3.4e-7 / 4.2e-8     1e-3
    step forms (global_norm) vs one call                           0                            1e-6 of sigma_max
    use_path vs the fixture                                        3.0e-7                       1e-3
    training gradients (check_grads_vs_fixture) / d_x              pass / 4.3e-6                1e-3 + its floor / 1e-3
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import kxsr_cases as kc  # noqa: E402
from test_gpu_steps import _Tape  # noqa: E402

# tests/test_gpu_sr.py (tests/test_gpu_wide.py: NET_TOL; test_gpu_network.py:71-72,107)
NET_TOL = {'fp32': 1e-4, 'fp16x3': 1e-4, 'fp16f8': 3e-4, 'fp16': 2e-2}
FORWARD = [(c, p) for c in kc.CASES for p in NET_TOL]          # every case in all four precision modes (forward and scores)
TWO_MODES = [(c, p) for c in kc.CASES for p in ('fp16x3', 'fp32')]
TRAJECTORY = 1e-3             # the project's trajectory parity bound (tests/test_gpu_sr.py)
OP_TOL = 1e-6                 # an output is a convex combination of at most four fp32 values (torch's own fp32 result: 8e-8)
_MODELS = {}


def dev():
    return torch.device('cuda:0')


def rel(a, b, floor=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-30)


def cat(out):
    """the network's two outputs as one vector per sample (the layout of the buffer the library writes)"""
    return torch.cat([out['x'].flatten(1), out['y'].flatten(1)], dim=1)


def model_for(case, precision='fp32', dropout=None, twin=False, fresh=False):
    key = (case, precision, dropout, twin)
    if fresh or key not in _MODELS:
        from conditional_score_diffusion_amd.models import utils as mutils
        import conditional_score_diffusion_amd.models.ncsnpp  # noqa: F401
        cfg = kc.make_config(case, precision, twin=twin)
        if dropout is not None:
            cfg.model.dropout = dropout
        model = mutils.create_model(cfg)
        res = model.load_state_dict(kc.params(cfg, {k: tuple(v.shape) for k, v in model.state_dict().items()}))
        assert not res.missing_keys and not res.unexpected_keys
        if fresh:
            return cfg, model.to(dev()).eval()
        _MODELS[key] = (cfg, model.to(dev()).eval())
    return _MODELS[key]


def sdes_for(cfg):
    from conditional_score_diffusion_amd import sde_lib
    m = cfg.model
    return {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}


def forward_args(case, cfg, j=0, B=kc.B):
    x, t = kc.forward_inputs(case)[j]
    return x[:B].contiguous().to(dev()), kc.case_y(case)[:B].contiguous().to(dev()), kc.labels_of(cfg, t)[:B].contiguous().to(dev())


def fixture_cat(g, case, j):
    return np.concatenate([g['%s_x%d' % (case, j)].reshape(kc.B, -1), g['%s_y%d' % (case, j)].reshape(kc.B, -1)], axis=1)


# ---- 1. the resamplers as operators ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [2, 3, 4, 8])
def test_operators_vs_interpolate(K):
    """ops.bilinear_up / ops.bilinear_down against F.interpolate in float64 at full-resolution sides 8 .. 32, ragged B and C; the
    adjoint of the downsample as <down(v), g> == <v, down^T(g)>"""
    from conditional_score_diffusion_amd import ops
    rs = np.random.RandomState(100 + K)
    worst = 0.0
    for S in [s for s in (8, 9, 12, 15, 16, 24, 27, 32) if s % K == 0]:
        s = S // K
        for Bq, C in ((1, 1), (3, 5), (2, 7)):
            y = torch.from_numpy(rs.standard_normal((Bq, C, s, s)).astype(np.float32))
            v = torch.from_numpy(rs.standard_normal((Bq, C, S, S)).astype(np.float32))
            g = torch.from_numpy(rs.standard_normal((Bq, C, s, s)).astype(np.float32))
            up = ops.bilinear_up(y.to(dev()), K)
            down = ops.bilinear_down(v.to(dev()), K)
            adj = ops.bilinear_down_adjoint(g.to(dev()), K)
            assert tuple(up.shape) == (Bq, C, S, S) and tuple(down.shape) == (Bq, C, s, s) and tuple(adj.shape) == (Bq, C, S, S)
            e_up = rel(up.cpu().numpy(), F.interpolate(y.double(), size=(S, S), mode='bilinear', align_corners=False).numpy())
            e_dn = rel(down.cpu().numpy(), F.interpolate(v.double(), size=(s, s), mode='bilinear', align_corners=False).numpy())
            lhs = float((down.double().cpu() * g.double()).sum())
            rhs = float((v.double() * adj.double().cpu()).sum())
            e_adj = abs(lhs - rhs) / max(float((down.double().cpu().abs() * g.double().abs()).sum()), 1e-30)
            worst = max(worst, e_up, e_dn, e_adj)
            assert e_up < OP_TOL and e_dn < OP_TOL and e_adj < OP_TOL, (K, S, Bq, C, e_up, e_dn, e_adj)
            # the autograd form of the downsample is that adjoint
            vg = v.to(dev()).requires_grad_(True)
            gr, = torch.autograd.grad((ops.bilinear_down(vg, K) * g.to(dev())).sum(), vg)
            assert torch.equal(gr, adj)
    print('K %d: worst operator error %.3e' % (K, worst))


@pytest.mark.parametrize('nf,S,K', [(64, 32, 8), (96, 32, 4), (96, 48, 3), (128, 16, 2)])
@pytest.mark.parametrize('precision', ['fp16x3', 'fp16'])
def test_first_layer_is_bitwise_the_paired_layer_on_an_upsampled_y(nf, S, K, precision):
    """ops.input_conv(y_scale=K) - the fused first layer's y_scale variants: nf 64 / 128 hold the y taps across the K loop, nf 96 (three
    cout tiles per wave) requests them behind it; both operand-plane counts - against the plain layer on ops.bilinear_up(y, K), with
    and without the sampler's y perturbation (perturbed at LOW resolution: ops.bilinear_up(y + sigma z), bitwise too), and the assemble pass +
    generic convolution against ITS plain form.  The K cases reach nf 64 only (K2), so the other variants are pinned here."""
    from conditional_score_diffusion_amd import ops
    rs = np.random.RandomState(nf + S + K)
    Bq, cx, cy, s = 3, 3, 3, S // K
    x = torch.from_numpy(rs.standard_normal((Bq, cx, S, S)).astype(np.float32)).to(dev())
    y = torch.from_numpy(rs.uniform(0, 1, (Bq, cy, s, s)).astype(np.float32)).to(dev())
    z = torch.from_numpy(rs.standard_normal((Bq, cy, s, s)).astype(np.float32)).to(dev())
    w = torch.from_numpy((rs.standard_normal((nf, cx + cy, 3, 3)) * 0.2).astype(np.float32)).to(dev())
    b = torch.from_numpy(rs.standard_normal(nf).astype(np.float32)).to(dev())
    sig = 0.37
    # y + sigma z in ONE rounding, as the library perturbs (bilin_perturb is an fma): the product of two fp32 values is exact in float64
    y_t = (y.double() + z.double() * float(np.float32(sig))).float()
    for fused in (True, False):
        a, sa = ops.input_conv(x, y, w, b, precision=precision, fused=fused, y_scale=K, want_stats=True) if fused else \
            (ops.input_conv(x, y, w, b, precision=precision, fused=False, y_scale=K), None)
        r, sr = ops.input_conv(x, ops.bilinear_up(y, K), w, b, precision=precision, fused=fused, want_stats=True) if fused else \
            (ops.input_conv(x, ops.bilinear_up(y, K), w, b, precision=precision, fused=False), None)
        assert torch.equal(a, r), (nf, S, K, precision, fused)
        if fused:
            assert torch.equal(sa, sr)
        an = ops.input_conv(x, y, w, b, y_noise=z, y_sigma=sig, precision=precision, fused=fused, y_scale=K)
        rn = ops.input_conv(x, ops.bilinear_up(y_t, K), w, b, precision=precision, fused=fused)
        assert torch.equal(an, rn), (nf, S, K, precision, fused)
        assert not torch.equal(an, a)


# ---- 2. forward and scores ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,precision', FORWARD)
def test_forward_vs_fixture(case, precision):
    """both outputs at both ends of the noise schedule against the imported reference (tests/test_gpu_sr.py test_forward_vs_fixture:
    max error over max |reference| of the whole output < NET_TOL)"""
    g = kc.golden()
    cfg, model = model_for(case, precision)
    for j in range(len(kc.FORWARD_TIMES)):
        x, y, labels = forward_args(case, cfg, j)
        x0, y0 = x.clone(), y.clone()
        with torch.no_grad():
            out = model({'x': x, 'y': y}, labels)
        assert tuple(out['x'].shape) == tuple(x.shape) and tuple(out['y'].shape) == tuple(y.shape)
        assert torch.equal(x, x0) and torch.equal(y, y0)                   # a forward writes neither input
        e = rel(cat(out).cpu().numpy(), fixture_cat(g, case, j))
        ex = rel(out['x'].cpu().numpy(), g['%s_x%d' % (case, j)])
        ey = rel(out['y'].cpu().numpy(), g['%s_y%d' % (case, j)])
        print('%s %s t[%d]: net %.3e (x alone %.3e, y alone %.3e)' % (case, precision, j, e, ex, ey))
        assert e < NET_TOL[precision], (case, precision, j, e)
        assert ex < NET_TOL[precision] and ey < NET_TOL[precision], (case, precision, j, ex, ey)


@pytest.mark.parametrize('case,precision', FORWARD)
def test_two_sde_scores_vs_fixture(case, precision):
    """models.utils.get_score_fn on {'x': cVESDE, 'y': VESDE}, continuous: both scores against the reference's (NET_TOL, as the forward)"""
    from conditional_score_diffusion_amd.models import utils as mutils
    g = kc.golden()
    cfg, model = model_for(case, precision)
    x, y, t = (v.to(dev()) for v in kc.score_inputs(case))
    with torch.no_grad():
        score = mutils.get_score_fn(sdes_for(cfg), model, conditional=True, train=False, continuous=True)({'x': x, 'y': y}, t)
    assert tuple(score['y'].shape) == kc.shapes(case)[1]
    ex, ey = rel(score['x'].cpu().numpy(), g[case + '_sx']), rel(score['y'].cpu().numpy(), g[case + '_sy'])
    print('%s %s: score x %.3e, score y %.3e' % (case, precision, ex, ey))
    assert ex < NET_TOL[precision] and ey < NET_TOL[precision], (case, precision, ex, ey)


# ---- 3. the twin: the same arithmetic in the same order ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case,precision', TWO_MODES)
def test_forward_is_bitwise_the_paired_network_on_an_upsampled_y(case, precision):
    from conditional_score_diffusion_amd import ops
    K = kc.CASES[case][4]
    cfg, model = model_for(case, precision)
    _, twin = model_for(case, precision, twin=True)
    for j in range(len(kc.FORWARD_TIMES)):
        x, y, labels = forward_args(case, cfg, j)
        with torch.no_grad():
            out = model({'x': x, 'y': y}, labels)
            ref = twin({'x': x, 'y': ops.bilinear_up(y, K)}, labels)
            ref_y = ops.bilinear_down(ref['y'].contiguous(), K)
        assert torch.equal(out['x'], ref['x']), (case, precision, j)
        assert torch.equal(out['y'], ref_y), (case, precision, j)


@pytest.mark.parametrize('case', ['K1', 'K3', 'K4'])
@pytest.mark.parametrize('precision', ['fp16x3', 'fp32'])
def test_gradients_are_bitwise_the_paired_networks(case, precision):
    """training-mode parameter gradients (dropout 0) and the eval-mode d_x of (out_x * w_x).sum() + (out_y * w_y).sum(): the planned
    graph runs at S x S either way; the boundary upsamples y, downsamples the y output and applies the downsample's adjoint to d_out"""
    from conditional_score_diffusion_amd import ops
    K = kc.CASES[case][4]
    cfg, model = model_for(case, precision, dropout=0.0)
    _, twin = model_for(case, precision, dropout=0.0, twin=True)
    _, x, y, labels, wx, wy = kc.dx_inputs(case)
    x, y, labels, wx, wy = (t.to(dev()) for t in (x, y, labels, wx, wy))
    y_up = ops.bilinear_up(y, K)

    def scalar(net, xin, is_twin):
        out = net({'x': xin, 'y': y_up if is_twin else y}, labels)
        oy = ops.bilinear_down(out['y'].contiguous(), K) if is_twin else out['y']
        return out, (out['x'] * wx).sum() + (oy * wy).sum()

    grads = []
    for net, is_twin in ((model, False), (twin, True)):
        assert net.train_executor == 'planned'
        net.train()
        net.zero_grad()
        out, val = scalar(net, x, is_twin)
        assert out['x'].requires_grad
        val.backward()
        grads.append({k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None})
        net.zero_grad()
        net.eval()
    assert list(grads[0]) == list(grads[1])
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), (case, precision, k)
    assert any(float(v.abs().max()) > 0 for v in grads[0].values())
    dxs = []
    for net, is_twin in ((model, False), (twin, True)):
        xg = x.clone().requires_grad_(True)
        _, val = scalar(net, xg, is_twin)
        dxs.append(torch.autograd.grad(val, xg)[0])
    assert tuple(dxs[0].shape) == tuple(x.shape) and float(dxs[0].abs().max()) > 0
    assert torch.equal(dxs[0], dxs[1]), (case, precision)


# ---- 4. sampling -------------------------------------------------------------------------------------------------------------------------
def _sampler(cfg, sde, case, denoise=True, use_path=False):
    from conditional_score_diffusion_amd.sampling import conditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    return conditional.get_pc_conditional_sampler(sde, kc.shapes(case)[0], get_predictor(cfg.sampling.predictor),
                                                  get_corrector(cfg.sampling.corrector), snr=cfg.sampling.snr, p_steps=kc.P_STEPS,
                                                  c_steps=1, continuous=True, denoise=denoise, use_path=use_path, eps=1e-5)


def _step_by_step(cfg, sde, model, y, tape):
    """the step-by-step loop of sampling/conditional.py on a tape (tests/test_gpu_sr.py: _step_by_step): corrector then predictor, a
    fresh y_t at S / K per update (perturbed at LOW resolution, as the reference does), the state and its noise at S"""
    from conditional_score_diffusion_amd.sampling import conditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    c_sde = sde['x']
    pred = lambda **k: conditional.conditional_shared_predictor_update_fn(      # noqa: E731
        sde=sde, predictor=get_predictor(cfg.sampling.predictor), probability_flow=False, continuous=True, **k)
    corr = lambda **k: conditional.conditional_shared_corrector_update_fn(      # noqa: E731
        sde=sde, corrector=get_corrector(cfg.sampling.corrector), continuous=True, snr=cfg.sampling.snr, n_steps=1, **k)
    with _Tape(tape[1:]) as tp, torch.no_grad():
        x = (tape[0] * c_sde.sigma_max).to(dev())
        ts = torch.linspace(c_sde.T, 1e-5, kc.P_STEPS)
        for i in range(kc.P_STEPS):
            vec_t = torch.ones(kc.B, device=dev()) * ts[i]
            for fn in (corr, pred):
                std = sde['y'].marginal_prob(y, vec_t)[1]
                y_in = y + torch.randn_like(y) * std[:, None, None, None]
                x, x_mean = fn(x=x, y=y_in, t=vec_t, model=model)
        assert tp.i == len(tape) - 1
    return x_mean


@pytest.mark.parametrize('case', kc.SAMPLER_CASES)
@pytest.mark.parametrize('precision', ['fp16x3', 'fp32'])
def test_pc_sampling_vs_fixture_and_step_by_step(case, precision):
    """3 PC steps of the two-SDE VE pair on the reference's tape (z_y at (S / K)^2 and z_x at S^2 per phase): the fused loop and the
    step-by-step loop against the reference's run, and against each other, at the project's 1e-3; csd_pc_step_begin / _end against
    csd_pc_sample (tests/test_gpu_sr.py: 1e-6 of sigma_max)"""
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    g = kc.golden()
    cfg, model = model_for(case, precision)
    sde = sdes_for(cfg)
    y = kc.case_y(case).to(dev())
    assert fused.fusable(model, sde, get_predictor(cfg.sampling.predictor), get_corrector(cfg.sampling.corrector), 1, False, True)
    tape = kc.pc_tape(case)
    sampler = _sampler(cfg, sde, case)
    res, _ = sampler(model, y, noise_tape=tape)
    assert tuple(res.shape) == kc.shapes(case)[0]
    step = _step_by_step(cfg, sde, model, y, tape)
    two, _ = sampler(model, y, noise_tape=tape, global_norm=(lambda s: None, kc.B))
    smax = cfg.model.sigma_max_x
    e_fused, e_step = rel(res.cpu().numpy(), g[case + '_pc']), rel(step.cpu().numpy(), g[case + '_pc'])
    e_both = rel(res.cpu().numpy(), step.cpu().numpy())
    d_two = float((res - two).abs().max()) / smax
    print('%s %s: fused vs reference %.3e, step by step vs reference %.3e, fused vs step by step %.3e, step forms %.3e of sigma_max'
          % (case, precision, e_fused, e_step, e_both, d_two))
    assert e_fused < TRAJECTORY and e_step < TRAJECTORY and e_both < TRAJECTORY
    assert d_two < 1e-6
    with pytest.raises(RuntimeError, match='noise tape holds'):               # a tape with a draw missing is refused
        sampler(model, y, noise_tape=tape[:-1])
    xs_, ys_ = kc.shapes(case)
    full = [t if tuple(t.shape) == xs_ else torch.zeros(ys_[0], ys_[1], xs_[2], xs_[3]) for t in tape]
    with pytest.raises(RuntimeError, match='noise tape holds .* elements'):   # ... and so is one whose y draws are full-resolution
        sampler(model, y, noise_tape=full)


def test_record_and_seed():
    """record rows have the shape of x and the last one is the pre-denoise state; seed= repeats"""
    cfg, model = model_for('K1', 'fp16x3')
    sde = sdes_for(cfg)
    y = kc.case_y('K1').to(dev())
    tape = kc.pc_tape('K1')
    xs = kc.shapes('K1')[0]
    out, info = _sampler(cfg, sde, 'K1', denoise=False)(model, y, show_evolution=True, noise_tape=tape)
    ev = info['evolution']['x']
    assert tuple(ev.shape) == (kc.P_STEPS,) + xs
    assert torch.equal(ev[-1], out.cpu())
    out_d, info_d = _sampler(cfg, sde, 'K1')(model, y, show_evolution=True, noise_tape=tape)
    assert torch.equal(info_d['evolution']['x'], ev) and not torch.equal(out_d.cpu(), ev[-1])
    for case in kc.SAMPLER_CASES:
        cfg, model = model_for(case, 'fp16x3')
        sampler = _sampler(cfg, sdes_for(cfg), case)
        y = kc.case_y(case).to(dev())
        with pytest.raises(RuntimeError, match='low-resolution'):            # seed= path: a full-resolution y is refused, not misread
            sampler(model, torch.zeros(kc.B, y.shape[1], kc.CASES[case][3], kc.CASES[case][3], device=dev()), seed=5)
        a, _ = sampler(model, y, seed=5)
        b, _ = sampler(model, y, seed=5)
        c, _ = sampler(model, y, seed=6)
        assert tuple(a.shape) == kc.shapes(case)[0] and bool(torch.isfinite(a).all())
        assert torch.equal(a, b) and not torch.equal(a, c)


def test_use_path_vs_fixture():
    """fused.run(use_path=True): y_t follows the bridge at S / K (tests/test_gpu_sr.py test_use_path_vs_fixture: the project's 1e-3)"""
    from conditional_score_diffusion_amd.sampling import fused
    case = kc.PATH_CASE
    g = kc.golden()
    cfg, model = model_for(case, 'fp32')
    sde = sdes_for(cfg)
    y = kc.case_y(case).to(dev())
    x, _, _ = fused.run(model, sde, kc.shapes(case)[0], y, kc.P_STEPS, cfg.sampling.snr, 1e-5, True, noise_tape=kc.path_tape(case),
                        use_path=True)
    e = rel(x.cpu().numpy(), g[case + '_path'])
    print('%s use_path: fused vs reference %.3e' % (case, e))
    assert e < TRAJECTORY


# ---- 5. training -------------------------------------------------------------------------------------------------------------------------
def _loss(model, cfg, x, y, u, tape):
    from conditional_score_diffusion_amd import losses
    fn = losses.get_general_sde_loss_fn(sdes_for(cfg), True, True, True, True, True)
    it = iter(tape)
    o_rand, o_like = torch.rand, torch.randn_like
    torch.rand = lambda *a, **k: u.clone()
    torch.randn_like = lambda t, **k: next(it).to(t.device)
    try:
        return fn(model, (y.to(dev()), x.to(dev())))
    finally:
        torch.rand, torch.randn_like = o_rand, o_like


def test_planned_training_gradients_and_dx_vs_reference():
    """loss.backward() through the planned training graph: the loss and every parameter gradient against the reference's autograd
    (tests/test_gpu_sr.py: check_grads_vs_fixture with tol 1e-3), and the eval-mode d_x (tests/test_gpu_wide.py: 1e-3)"""
    from test_oracle_golden import check_grads_vs_fixture
    case = kc.TRAIN_CASE
    g = kc.golden()
    cfg, x, y, u, tape = kc.grad_inputs(case)
    _, model = model_for(case, 'fp32', dropout=0.0)
    assert model.train_executor == 'planned'
    model.zero_grad()
    loss = _loss(model, cfg, x, y, u, tape)
    assert model.training and loss.requires_grad
    loss.backward()
    worst = check_grads_vs_fixture(g, case, float(loss.detach()), {k: v.grad for k, v in model.named_parameters()}, 1e-3)
    model.zero_grad()
    model.eval()
    _, x, y, labels, wx, wy = kc.dx_inputs(case)
    xg = x.to(dev()).requires_grad_(True)
    out = model({'x': xg, 'y': y.to(dev())}, labels.to(dev()))
    dx, = torch.autograd.grad((out['x'] * wx.to(dev())).sum() + (out['y'] * wy.to(dev())).sum(), xg)
    e_dx = rel(dx.cpu().numpy(), g[case + '_dx'])
    print('%s: loss %.6f, worst sampled gradient error %.3e, d_x %.3e' % (case, float(loss.detach()), worst, e_dx))
    assert e_dx <= 1e-3, (case, e_dx)


def test_two_trainer_steps_move_every_parameter():
    from conditional_score_diffusion_amd import train
    case = kc.TRAIN_CASE
    cfg, x, y, u, tape = kc.grad_inputs(case)
    cfg, model = model_for(case, 'fp16x3', dropout=0.1, fresh=True)
    cfg.optim.warmup = 2
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    tr = train.Trainer(cfg, model, sdes_for(cfg))
    batch = (y.to(dev()), x.to(dev()))
    vals = [float(tr.train_step(batch)) for _ in range(2)]
    assert np.isfinite(vals).all() and tr.step == 2
    for k, v in model.named_parameters():
        assert not torch.equal(v.detach(), before[k]), k
    with torch.no_grad():                                       # the inference plan picks up the updated weights
        xd, yd, labels = forward_args(case, cfg)
        out = model.eval()({'x': xd, 'y': yd}, labels)
    assert bool(torch.isfinite(out['x']).all()) and bool(torch.isfinite(out['y']).all())


# ---- 6. caller buffers, refusals ---------------------------------------------------------------------------------------------------------
def _two_fills(run, sized_by, setup=None):
    """run() under tests/guarded.py's seam with the buffers pre-filled with 0x00 and with 0xFF (tests/test_gpu_buffers.py): finite,
    bitwise equal results, every guard intact, every byte buffer sized by a csd_*_bytes entry"""
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
        rec.assert_sized_by(sized_by)
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), 'fill 0x%02X: %s is not finite' % (fill, k)
        outs.append(got)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), '%s depends on the previous contents of a buffer' % k
    return outs[0]


@pytest.mark.parametrize('case,precision', [('K1', 'fp32'), ('K1', 'fp16x3'), ('K2', 'fp16x3'), ('K2', 'fp16'), ('K3', 'fp16x3'), ('K4', 'fp16x3')])
def test_forward_does_not_depend_on_what_the_buffers_held(case, precision):
    """packed weights, workspace (with the head's full-resolution tensor) and the output between guards: the x block and the
    downsampled y block together cover every element of `out` (a hole would keep the fill), and nothing lands outside it"""
    cfg, model = model_for(case, precision)
    x, y, labels = forward_args(case, cfg)
    x0, y0 = x.clone(), y.clone()

    def run():
        with torch.no_grad():
            out = model({'x': x, 'y': y}, labels)
        return {'x': out['x'], 'y': out['y']}
    got = _two_fills(run, ['csd_unet_packed_bytes', 'csd_unet_workspace_bytes'], setup=lambda: guarded.reset_model_buffers(model))
    assert torch.equal(x, x0) and torch.equal(y, y0)
    g = kc.golden()
    assert rel(got['x'].numpy(), g[case + '_x0']) < NET_TOL[precision] and rel(got['y'].numpy(), g[case + '_y0']) < NET_TOL[precision]
    guarded.reset_model_buffers(model)


def test_sampling_and_training_do_not_depend_on_what_the_buffers_held():
    """PC scratch, workspace, packed weights, the record, the training workspace and every gradient between guards: 3-step PC sampling
    on K1 and K4, the planned training step and the input gradient on K1"""
    for case in kc.SAMPLER_CASES:
        cfg, model = model_for(case, 'fp16x3')
        sde, y, tape = sdes_for(cfg), kc.case_y(case).to(dev()), kc.pc_tape(case)

        def sample():
            x, info = _sampler(cfg, sde, case)(model, y, show_evolution=True, noise_tape=tape)
            return {'x': x, 'record': info['evolution']['x']}
        got = _two_fills(sample, ['csd_unet_packed_bytes', 'csd_unet_workspace_bytes', 'csd_pc_scratch_bytes'],
                         setup=lambda: guarded.reset_model_buffers(model))
        assert rel(got['x'].numpy(), kc.golden()[case + '_pc']) < TRAJECTORY
        guarded.reset_model_buffers(model)
    case = kc.TRAIN_CASE
    cfg, x, y, u, tape = kc.grad_inputs(case)
    _, model = model_for(case, 'fp32', dropout=0.0)

    def train():
        model.train()
        model.zero_grad()
        loss = _loss(model, cfg, x, y, u, tape)
        loss.backward()
        got = {'loss': loss.detach().reshape(1)}
        got.update({k: v.grad.clone() for k, v in model.named_parameters()})
        model.eval()
        xg = x.to(dev()).requires_grad_(True)
        out = model({'x': xg, 'y': y.to(dev())}, torch.tensor([12.25, 871.0], device=dev()))
        got['dx'], = torch.autograd.grad(out['x'].square().sum() + out['y'].square().sum(), xg)
        return got
    _two_fills(train, ['csd_unet_train_workspace_bytes'], setup=lambda: guarded.reset_model_buffers(model))
    guarded.reset_model_buffers(model)
    model.zero_grad()


def test_refusals_return_invalid_and_write_nothing():
    """csd_pc_inpaint_sample and csd_unet_debug_digest on a y_scale handle: CSD_ERR_INVALID (-1) naming the field, the state and the
    digest untouched; the Python entries raise NotImplementedError naming the classes"""
    from conditional_score_diffusion_amd import _lib, likelihood, sde_lib
    from conditional_score_diffusion_amd.sampling import fused
    l = _lib.lib()
    for case in ('K1', 'K4'):
        cfg, model = model_for(case, 'fp16x3')
        xs = kc.shapes(case)[0]
        x = torch.full(xs, 3.25, device=dev())
        model._ensure_packed()
        ws = model._workspace(kc.B)
        nbytes = l.csd_pc_inpaint_scratch_bytes(model._h, kc.B)
        scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
        p, ip = _lib.PCParams(), _lib.PCInpaintParams()
        p.n_steps = 1
        rc = l.csd_pc_inpaint_sample(model._h, _lib.ptr(model._packed), _lib.ptr(ws), ws.numel(), _lib.ptr(scratch), nbytes, _lib.ptr(x),
                                     None, kc.B, ctypes.byref(p), ctypes.byref(ip), _lib.current_stream(dev()))
        msg = l.csd_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and 'y_scale' in msg, (rc, msg)
        assert bool((x == 3.25).all()) and not bool(scratch.any())
        fn = ctypes.CDLL(_lib.LIB_PATH).csd_unet_debug_digest
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_uint64)]
        d = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
        assert fn(model._h, kc.B, 0.0, d) == -1 and 'y_scale' in l.csd_last_error().decode() and list(d) == [7, 7, 7, 7]
        name = type(model).__name__
        with pytest.raises(NotImplementedError, match=name):
            fused.run(model, sde_lib.VESDE(0.01, 5.0, 1000), xs, None, kc.P_STEPS, 0.15, 1e-5, True, inpaint=(x, torch.ones_like(x)))
        with pytest.raises(NotImplementedError, match=name):
            likelihood.get_conditional_likelihood_fn(sde_lib.cVESDE(0.01, 5.0, 1000), lambda v: v)(model, x, kc.case_y(case).to(dev()))
        with pytest.raises(RuntimeError, match='y has shape'):                # a full-resolution y is refused, not resampled silently
            model({'x': x, 'y': torch.zeros(xs[0], kc.CASES[case][2], xs[2], xs[3], device=dev())}, torch.ones(kc.B, device=dev()))


# ---- 7. repeatable, independent of the batch position ------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,precision', TWO_MODES)
def test_bitwise_repeatable_and_independent_of_the_batch(case, precision):
    cfg, model = model_for(case, precision)
    x, y, labels = forward_args(case, cfg)
    x1, y1, l1 = forward_args(case, cfg, B=1)
    with torch.no_grad():
        a = cat(model({'x': x, 'y': y}, labels))
        b = cat(model({'x': x, 'y': y}, labels))
        one = cat(model({'x': x1, 'y': y1}, l1))
    assert torch.equal(a, b)
    assert torch.equal(a[:1], one)
