"""-m gpu: networks built with config.model.nonlinearity = 'relu' / 'lrelu' / 'elu' (models/layers.py:29-41; LeakyReLU slope 0.2).
A network that is not SiLU does not merely evaluate another scalar function: build_packed_layout gives the fused-prologue kernels
(conv_ff / conv_xk / conv_fx) and the tap-partial head (conv_pw16) to SiLU networks only, so every GroupNorm-ed 3x3 conv of such a
network - at the large maps too - runs the quad or the loader/consumer schedule behind gn_apply16 / gn_fused16, the FIR pass of the
NCSN++ up / down blocks takes its generic activation arm, and the head takes the ordinary 3x3 path.  References: the oracle
(oracle/score_oracle.py) evaluated in float64.

Worst errors measured on the MI355X next to their bounds (max-abs-diff / max-abs-ref unless stated; the shape with the largest
error / bound ratio of each group):

  forward, DDPM family (test_ddpm_forward_vs_oracle64; sr3_tiny, nf = 96 at 32 x 32, nf = 128 at 16 x 16)
    activation   fp32                 fp16x3               fp16f8               fp16
    relu         1.3e-6  (2e-5)       9.3e-7  (2e-5)       8.7e-6  (2e-4)       8.0e-4  (5e-3)
    lrelu        1.5e-6  (2e-5)       7.4e-7  (2e-5)       7.0e-6  (2e-4)       8.2e-4  (5e-3)
    elu          1.6e-6  (2e-5)       1.1e-6  (3e-5)       8.0e-6  (2e-4)       8.5e-4  (5e-3)
  forward, NCSN++ (test_ncsnpp_forward_vs_oracle64; of which ~1e-5 is the fp32 evaluation of the Gaussian-Fourier embedding: the
  fp32 oracle sits at 1.1e-5 from the float64 one on ncsnpp_fourier_skip and ncsnpp_paired_skip, at 7e-7 on the positional case)
    relu         1.12e-5 (2e-5)       1.12e-5 (2e-5)
    lrelu        9.1e-6  (2e-5)       9.0e-6  (2e-5)
    elu          1.02e-5 (2e-5)       1.01e-5 (2e-5)
  input gradient in eval mode (test_eval_input_grad_vs_oracle64)
    elu          1.1e-5  (1e-3)       1.1e-5  (1e-3)       max-abs
    lrelu        3.1e-6  (1e-3)       3.1e-6  (1e-3)       norm-wise
  training mode, planned against operator executor, fp32 (test_training_mode_planned_vs_operators)
    elu          1.8e-6  (1e-3)       worst parameter, max-abs over the parameter's gradient scale
    relu         5.9e-7  (1e-3)       norm-wise over all parameters
  ELU against SiLU 0.46, ReLU against LeakyReLU 0.23 (both must exceed 1e-2); fused PC loop against the per-step path 0 (1e-5).
"""
import numpy as np
import pytest
import torch

import cases
import score_oracle as so

pytestmark = pytest.mark.gpu

ACTS = ['relu', 'lrelu', 'elu']
TOL = 1e-3          # the project's parity bound of the gradient tests: max-abs-diff / max-abs-ref (tests/test_gpu_input_grad.py)


def dev():
    return torch.device('cuda:0')


def rel(a, b):
    """max-abs-diff / max-abs-ref, in float64"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


def normwise(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


@pytest.fixture
def oracle64(monkeypatch):
    """the oracle in float64: its two fp32 constants (the sinusoidal embedding, the FIR kernel) are widened"""
    te, fk = so.timestep_embedding, so.fir_kernel_2d
    monkeypatch.setattr(so, 'timestep_embedding', lambda *a, **k: te(*a, **k).double())
    monkeypatch.setattr(so, 'fir_kernel_2d', lambda *a, **k: fk(*a, **k).double())
    return so


def widen(p):
    return {k: v.double() for k, v in p.items()}


# ---- the DDPM family ----------------------------------------------------------------------------------------------------------
# shape name -> (config, batch, sr3, {precision: tolerance})
def ddpm_shape(shape):
    if shape == 'sr3_tiny':
        # 20 / 10 / 5 levels: tiles straddle samples, gn_fused16.  Bounds: what the swish network of this case is held to against the
        # reference's fixture (test_gpu_network.py: test_forward_and_score_vs_golden 1e-4, test_fp16_mfma_modes_vs_golden 1e-4 / 3e-4 / 2e-2)
        cfg, B = cases.case_config('sr3_tiny')
        return cfg, B, True, {'fp32': 1e-4, 'fp16x3': 1e-4, 'fp16f8': 3e-4, 'fp16': 2e-2}
    if shape == 'nf96_32':
        # 16-divisible maps (a swish network runs conv_ff there; here the quad / loader-consumer schedules), groups of 96 couts, an odd
        # batch, a two-source concat on the up path.  Bounds: test_nf96_batch_unmasked_tiles
        cfg = cases.make_config(name='ddpm_paired_SR3', nf=96, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(16,), image_size=32)
        return cfg, 3, True, {'fp32': 2e-5, 'fp16x3': 2e-5, 'fp16f8': 2e-4, 'fp16': 5e-3}
    assert shape == 'nf128_16'
    # groups of 128 couts and a 6-channel head.  Bounds: test_nf128_network_vs_oracle
    cfg = cases.make_config(name='ddpm_paired', nf=128, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(8,), image_size=16)
    return cfg, 3, False, {'fp32': 3e-5, 'fp16x3': 3e-5, 'fp16f8': 3e-4, 'fp16': 5e-3}


def ddpm_inputs(cfg, B, seed=0):
    """x (sigma 5), y in [0, 1), non-constant labels"""
    S = cfg.data.image_size
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((B, 3, S, S)).astype(np.float32) * 5)
    y = torch.from_numpy(rs.uniform(0, 1, (B, 3, S, S)).astype(np.float32))
    labels = torch.tensor([3., 420.5, 998.][:B])
    return x, y, labels


def ddpm_model(cfg, act, precision):
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg.model.nonlinearity = act
    cfg.model.csd_precision = precision
    nc = so.NetCfg.from_config(cfg)
    p = so.synth_params(so.ddpm_param_shapes(nc), 0)
    model = mutils.create_model(cfg)
    missing = model.load_state_dict(p)
    assert not missing.missing_keys and not missing.unexpected_keys
    return nc, p, model.to(dev()).eval()


def flat(r):
    return torch.cat([r['x'], r['y']], dim=1) if isinstance(r, dict) else r


_REF = {}      # (family, shape, act) -> float64 oracle output: computed once, shared by the precision modes, never written to


def ddpm_ref64(shape, act):
    """(call with the oracle64 fixture active)"""
    key = ('ddpm', shape, act)
    if key not in _REF:
        cfg, B, sr3, _ = ddpm_shape(shape)
        cfg.model.nonlinearity = act
        nc = so.NetCfg.from_config(cfg)
        p = so.synth_params(so.ddpm_param_shapes(nc), 0)
        x, y, labels = ddpm_inputs(cfg, B)
        with torch.no_grad():
            _REF[key] = flat(so.paired_forward(widen(p), nc, x.double(), y.double(), labels.double(), sr3))
    return _REF[key]


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3', 'fp16f8', 'fp16'])
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('shape', ['sr3_tiny', 'nf96_32', 'nf128_16'])
def test_ddpm_forward_vs_oracle64(oracle64, shape, act, precision):
    """the planned executor of a relu / lrelu / elu network in every arithmetic mode against the float64 oracle, at the bounds the
    project holds its swish networks of the same structure to (ddpm_shape).  The activations are continuous: the kinks of ReLU and
    LeakyReLU are no reason for a wider bound.  Before the head was kept off the tap-partial form every fp16-mode case here failed with
    'pw16: temb / NCHW output / an activation without a GroupNorm are not supported'."""
    cfg, B, sr3, tols = ddpm_shape(shape)
    nc, p, model = ddpm_model(cfg, act, precision)
    x, y, labels = ddpm_inputs(cfg, B)
    with torch.no_grad():
        out = flat(model({'x': x.to(dev()), 'y': y.to(dev())}, labels.to(dev())))
    err = rel(out, ddpm_ref64(shape, act))
    print('forward %s %s %s: %.3e (bound %.0e)' % (shape, act, precision, err, tols[precision]))
    assert err < tols[precision], (shape, act, precision, err)


def test_the_activation_is_really_applied():
    """same weights, same inputs, default arithmetic: ELU against SiLU and ReLU against LeakyReLU differ by far more than any
    rounding - a path that dropped the activation or put another in its place (a head that skipped it, a kernel that knows SiLU only)
    would make a pair agree.  (On the CPU oracle the two pairs differ by 0.46 and 0.23 of the output's largest value.)"""
    out = {}
    for act in ('swish', 'elu', 'relu', 'lrelu'):
        cfg, B = cases.case_config('sr3_tiny')
        nc, p, model = ddpm_model(cfg, act, 'fp16x3')
        x, y, labels = ddpm_inputs(cfg, B)
        with torch.no_grad():
            out[act] = model({'x': x.to(dev()), 'y': y.to(dev())}, labels.to(dev())).cpu()
    d_es, d_rl = rel(out['elu'], out['swish']), rel(out['relu'], out['lrelu'])
    print('elu vs swish %.3e, relu vs lrelu %.3e' % (d_es, d_rl))
    assert d_es > 1e-2 and d_rl > 1e-2


def test_batch_independence_of_a_lrelu_network():
    """same sample, different batch position / batch size -> identical bits (test_batch_independence_of_network for a network whose
    20 x 20 level also runs the quad schedule, in the default arithmetic)"""
    cfg, B = cases.case_config('sr3_tiny')
    nc, p, model = ddpm_model(cfg, 'lrelu', 'fp16x3')
    y = cases.case_y('sr3_tiny', B=5).to(dev())
    x = torch.randn(5, 3, 20, 20, generator=torch.Generator().manual_seed(3)).to(dev()) * 30
    lab = torch.full((5,), 700.0, device=dev())
    with torch.no_grad():
        full = model({'x': x, 'y': y}, lab)
        one = model({'x': x[3:4].contiguous(), 'y': y[3:4].contiguous()}, lab[:1])
    assert torch.equal(full[3:4], one)


def test_fused_pc_loop_of_an_elu_network_matches_the_per_step_path():
    """three fused PC steps with a noise tape == the predictor / corrector classes driven step by step on the same network
    (test_generic_per_step_path_matches_fused with ELU in fp16x3): the device loop assumes SiLU nowhere"""
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import fused
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    case = 'sr3_tiny'
    cfg, B = cases.case_config(case)
    nc, p, model = ddpm_model(cfg, 'elu', 'fp16x3')
    sde = sde_lib.cVESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, cfg.model.num_scales)
    y = cases.case_y(case).to(dev())
    tape = cases.tape(cases.pc_tape_shapes(case, 3))
    xs = (B,) + tuple(cfg.data.shape_x)
    x_f, _, _ = fused.run(model, sde, xs, y, 3, cfg.sampling.snr, 1e-5, True, noise_tape=tape)
    it = iter(tape[1:])
    orig = torch.randn_like
    torch.randn_like = lambda t, **k: next(it).to(t.device)
    try:
        sfn = mutils.get_conditional_score_fn(mutils.get_score_fn(sde, model, conditional=True, continuous=True), 'x')
        pred = get_predictor('conditional_reverse_diffusion')(sde, sfn, False)
        corr = get_corrector('conditional_langevin')(sde, sfn, cfg.sampling.snr, 1)
        x = (tape[0] * sde.sigma_max).to(dev())
        ts = torch.linspace(sde.T, 1e-5, 3)
        for i in range(3):
            vt = torch.ones(B, device=dev()) * ts[i]
            x, xm = corr.update_fn(x, y, vt)
            x, xm = pred.update_fn(x, y, vt)
    finally:
        torch.randn_like = orig
    assert torch.isfinite(x_f).all()
    err = float((xm.cpu().double() - x_f.cpu().double()).abs().max()) / float(sde.sigma_max)
    print('fused vs per-step, elu fp16x3: %.3e of sigma_max' % err)
    assert err < 1e-5


# ---- NCSN++ -------------------------------------------------------------------------------------------------------------------
def ncsnpp_model(case, act, precision, dropout=None):
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B, x, labels = cases.ncsnpp_case(case)
    cfg.model.nonlinearity = act
    cfg.model.csd_precision = precision
    if dropout is not None:
        cfg.model.dropout = dropout
    model = mutils.create_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    p = cases.ncsnpp_params(shapes, 5)
    model.load_state_dict(p)
    return cfg, p, model.to(dev()).eval(), x, labels


def ncsnpp_call(cfg, model, x, labels):
    if cfg.model.name == 'ncsnpp_paired':
        return flat(model({'x': x[:, :3].contiguous(), 'y': x[:, 3:].contiguous()}, labels))
    return model(x, labels)


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('fp16x3', 2e-5)])
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('case', ['ncsnpp_fourier_skip', 'ncsnpp_nofir_residual', 'ncsnpp_paired_skip'])
def test_ncsnpp_forward_vs_oracle64(oracle64, case, act, precision, tol):
    """NCSN++ with the three activations at the bounds of test_ncsnpp.py:test_forward_vs_reference: FIR up / down blocks (fir_resample2
    with the activation in its prologue) and the output pyramid, the non-FIR path behind gn_apply32, a 6-channel head"""
    cfg, p, model, x, labels = ncsnpp_model(case, act, precision)
    with torch.no_grad():
        out = ncsnpp_call(cfg, model, x.to(dev()), labels.to(dev()))
    key = ('ncsnpp', case, act)
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = so.ncsnpp_forward(widen(p), cfg, x.double(), labels.double())
    err = rel(out, _REF[key])
    print('forward %s %s %s: %.3e (bound %.0e)' % (case, act, precision, err, tol))
    assert err < tol, (case, act, precision, err)


# ---- input gradient in eval mode ------------------------------------------------------------------------------------------------
def grad_case(family, case, act, precision=None):
    """-> (cfg, params, oracle forward(p, x), x, y, labels, cotangent w) on the CPU; the network is built by the caller"""
    if family == 'ddpm':
        cfg, B = cases.case_config(case)
        rs = np.random.RandomState(7)
        x = torch.from_numpy(rs.uniform(0, 1, size=(B,) + tuple(cfg.data.shape_x)).astype(np.float32))
        y = cases.case_y(case)
        labels = torch.tensor([12.25, 871.0][:B])
        cfg.model.nonlinearity = act
        nc = so.NetCfg.from_config(cfg)
        p = so.synth_params(so.ddpm_param_shapes(nc), 0)
        out_ch = cfg.model.output_channels

        def ref(pp, xx):
            return so.ddpm_forward(pp, nc, torch.cat([xx, y.to(xx.dtype)], dim=1), labels.to(xx.dtype))
    else:
        cfg, B, x, labels = cases.ncsnpp_case(case)
        y = None
        cfg.model.nonlinearity = act
        import conditional_score_diffusion_amd.models.ncsnpp  # noqa: F401  (registers the model names)
        from conditional_score_diffusion_amd.models import utils as mutils
        with torch.device('meta'):
            shapes = {k: tuple(v.shape) for k, v in mutils.create_model(cfg).state_dict().items()}
        p = cases.ncsnpp_params(shapes, 5)
        out_ch = cfg.data.num_channels

        def ref(pp, xx):
            return so.ncsnpp_forward(pp, cfg, xx, labels.to(xx.dtype))
    cfg.model.dropout = 0.0
    if precision is not None:
        cfg.model.csd_precision = precision
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((x.shape[0], out_ch) + tuple(x.shape[2:])).astype(np.float32))
    return cfg, p, ref, x, y, labels, w


def oracle_input_grad(ref, p, x, w, dtype):
    xx = x.to(dtype).requires_grad_(True)
    r = ref({k: v.to(dtype) for k, v in p.items()}, xx)
    g, = torch.autograd.grad((r * w.to(dtype)).sum(), xx)
    return r.detach(), g


# LeakyReLU's derivative jumps at 0: a pre-activation within rounding of zero takes the other slope, in ANY fp32 evaluation.  The
# bound is norm-wise, ||g - g_ref|| / ||g_ref|| <= max(TOL, 4 x what the fp32 oracle's autograd shows against the float64 oracle's on
# the same seeded inputs, on the CPU); the factor 4 covers another summation order flipping another handful of elements.  Measured
# on the CPU: 1.4e-6 (sr3_tiny) and 3.1e-6 (ncsnpp_residual_input) - no slope flipped at these seeds, 4 x either is far below TOL, so
# the bound is TOL = 1e-3 for both.
LRELU_CPU_NORMWISE = {'sr3_tiny': 1.4e-6, 'ncsnpp_residual_input': 3.1e-6}


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('family,case', [('ddpm', 'sr3_tiny'), ('ncsnpp', 'ncsnpp_residual_input')])
@pytest.mark.parametrize('act', ['elu', 'lrelu'])
def test_eval_input_grad_vs_oracle64(oracle64, act, family, case, precision):
    """d(out . w)/dx of model.eval() under autograd (the planned training graph without dropout + the input-only backward) against
    float64 autograd of the oracle, as test_gpu_input_grad.py:test_eval_input_grad_vs_oracle does for SiLU.  ELU has a continuous
    derivative: that test's bound (max-abs, 1e-3).  LeakyReLU: norm-wise; measured on the CPU 1.4e-6 / 3.1e-6, hence the bound
    max(1e-3, 4 x that) = 1e-3 (see LRELU_CPU_NORMWISE)."""
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, p, ref, x, y, labels, w = grad_case(family, case, act, precision)
    model = mutils.create_model(cfg)
    model.load_state_dict(p)
    model = model.to(dev()).eval()
    xg = x.to(dev()).requires_grad_(True)
    out = model({'x': xg, 'y': y.to(dev())}, labels.to(dev())) if y is not None else model(xg, labels.to(dev()))
    g, = torch.autograd.grad((out * w.to(dev())).sum(), xg)
    r, gr = oracle_input_grad(ref, p, x, w, torch.float64)
    assert rel(out, r) <= TOL
    if act == 'lrelu':
        err, bound = normwise(g, gr), max(TOL, 4 * LRELU_CPU_NORMWISE[case])
        print('input gradient %s %s %s: %.3e norm-wise (bound %.1e)' % (case, act, precision, err, bound))
    else:
        err, bound = rel(g, gr), TOL
        print('input gradient %s %s %s: %.3e max-abs (bound %.1e)' % (case, act, precision, err, bound))
    assert err <= bound, (act, case, precision, err)


# ---- training mode ------------------------------------------------------------------------------------------------------------------
# ReLU's derivative jumps like LeakyReLU's; the planned and the operator executor are both fp32 evaluations in different summation
# orders, so their parameter gradients are compared norm-wise over all parameters at max(TOL, 4 x the fp32 oracle's norm-wise
# distance from the float64 oracle on the same inputs, measured on the CPU: RELU_CPU_NORMWISE) - see LRELU_CPU_NORMWISE.
RELU_CPU_NORMWISE = {'ncsnpp_positional_plain': 7.1e-7, 'sr3_tiny': 1.6e-6}        # -> the bound is TOL for both


def train_run(family, case, act, executor):
    """-> (output, {name: gradient}) of model.train() with dropout 0 and the cotangent w of grad_case, fp32"""
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, p, ref, x, y, labels, w = grad_case(family, case, act, 'fp32')
    model = mutils.create_model(cfg)
    model.load_state_dict(p)
    model = model.to(dev()).train()
    model.train_executor = executor
    out = model({'x': x.to(dev()), 'y': y.to(dev())}, labels.to(dev())) if y is not None else model(x.to(dev()), labels.to(dev()))
    assert out.requires_grad
    assert (getattr(model, '_train_ws', None) is not None) == (executor == 'planned')      # the executor that was asked for ran
    (out * w.to(dev())).sum().backward()
    return out.detach().cpu(), {k: q.grad.detach().cpu() for k, q in model.named_parameters() if q.requires_grad}


@pytest.mark.parametrize('family,case', [('ncsnpp', 'ncsnpp_positional_plain'), ('ddpm', 'sr3_tiny')])
@pytest.mark.parametrize('act', ['elu', 'relu'])
def test_training_mode_planned_vs_operators(oracle64, act, family, case):
    """model.train() with dropout 0: every parameter gradient of the planned training graph (train_graph.h carries the network's
    activation) against autograd over the differentiable operators, and the output and the loss (out . w) against the float64 oracle.
    ELU: per parameter, at the bound of the gradient tests (1e-3 of the parameter's gradient scale, tests/test_ncsnpp.py:
    test_training_mode_gradients_vs_oracle_autograd).  ReLU: norm-wise over all parameters (see RELU_CPU_NORMWISE)."""
    cfg, p, ref, x, y, labels, w = grad_case(family, case, act)
    out_p, g_p = train_run(family, case, act, 'planned')
    out_o, g_o = train_run(family, case, act, 'operators')
    with torch.no_grad():
        r = ref(widen(p), x.double())
    assert rel(out_p, r) <= 2e-5 and rel(out_o, r) <= 2e-5
    loss_ref = float((r * w.double()).sum())
    for o in (out_p, out_o):          # (the bound test_gpu_training.py:test_training_loss_and_grads_vs_reference holds the loss to)
        assert abs(float((o.double() * w.double()).sum()) - loss_ref) <= 1e-4 * abs(loss_ref)
    assert sorted(g_p) == sorted(g_o) and len(g_p) > 20
    if act == 'relu':
        num = np.sqrt(sum(float((g_p[k].double() - g_o[k].double()).pow(2).sum()) for k in g_o))
        den = np.sqrt(sum(float(g_o[k].double().pow(2).sum()) for k in g_o))
        bound = max(TOL, 4 * RELU_CPU_NORMWISE[case])
        print('training %s %s planned vs operators: %.3e norm-wise (bound %.1e)' % (case, act, num / den, bound))
        assert num / den <= bound
        return
    total = float(np.sqrt(sum(float((v.double() ** 2).sum()) for v in g_o.values())))
    worst = 0.0
    for k, v in g_o.items():
        err = float((g_p[k].double() - v.double()).abs().max())
        scale = max(float(v.abs().max()), float(v.double().norm()) / np.sqrt(v.numel()))
        assert err <= TOL * scale + 1e-6 * total / np.sqrt(v.numel()), (k, err, scale)
        if scale > 1e-6 * total:
            worst = max(worst, err / scale)
    print('training %s %s planned vs operators: worst per-parameter %.3e (bound %.1e)' % (case, act, worst, TOL))
