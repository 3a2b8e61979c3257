"""Input gradient of the HIP score networks (csd_unet_backward_ex's d_x): eval-mode autograd with respect to x against the oracle's
float64 autograd, training mode against the operator-granular path, and the consistency of the new entry point."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import score_oracle as so

TOL = 1e-3          # the project's parity bound: max-abs-diff / max-abs-ref


@pytest.fixture
def oracle64(monkeypatch):
    """the oracle in float64: its two fp32 constants (the sinusoidal embedding, the FIR kernel) are widened"""
    te, fk = so.timestep_embedding, so.fir_kernel_2d
    monkeypatch.setattr(so, 'timestep_embedding', lambda *a, **k: te(*a, **k).double())
    monkeypatch.setattr(so, 'fir_kernel_2d', lambda *a, **k: fk(*a, **k).double())
    return so


# (family, case, centred override)
NETS = [('ddpm', 'uncond_tiny', None), ('ddpm', 'uncond_tiny', True), ('ddpm', 'sr3_tiny', None), ('ddpm', 'sr3_tiny', True),
        ('ncsnpp', 'ncsnpp_fourier_skip', None), ('ncsnpp', 'ncsnpp_fourier_skip', True), ('ncsnpp', 'ncsnpp_positional_plain', None),
        ('ncsnpp', 'ncsnpp_positional_plain', False)]


def build(family, case, centered, precision, dropout=0.0):
    """-> (model on the GPU, params fp32, forward(p, x, y, labels) of the oracle, x, y, labels) with x / y / labels on the CPU"""
    from conditional_score_diffusion_amd.models import utils as mutils
    if family == 'ddpm':
        cfg, B = cases.case_config(case)
        rs = np.random.RandomState(7)
        x = torch.from_numpy(rs.uniform(0, 1, size=(B,) + tuple(cfg.data.shape_x)).astype(np.float32))
        y = cases.case_y(case) if case.startswith('sr3') else None
        labels = torch.tensor([12.25, 871.0][:B])
    else:
        cfg, B, x, labels = cases.ncsnpp_case(case)
        y = None
    if centered is not None:
        cfg.data.centered = centered
    cfg.model.csd_precision = precision
    cfg.model.dropout = dropout
    model = mutils.create_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    if family == 'ddpm':
        nc = so.NetCfg.from_config(cfg)
        p = so.synth_params(so.ddpm_param_shapes(nc), 0)

        def ref(pp, xx, yy, ll):
            return so.ddpm_forward(pp, nc, torch.cat([xx, yy], dim=1) if yy is not None else xx, ll)
    else:
        p = cases.ncsnpp_params(shapes, 5)

        def ref(pp, xx, yy, ll):
            return so.ncsnpp_forward(pp, cfg, xx, ll)
    model.load_state_dict(p)
    return model.to('cuda:0'), p, ref, x, y, labels


def call(model, x, y, labels):
    return model({'x': x, 'y': y}, labels) if y is not None else model(x, labels)


def rel(a, b):
    return (a.detach().cpu().double() - b.detach().double()).abs().max().item() / b.abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('family,case,centered', NETS)
def test_eval_input_grad_vs_oracle(oracle64, family, case, centered, precision):
    model, p, ref, x, y, labels = build(family, case, centered, precision)
    model.eval()
    dev = torch.device('cuda:0')
    out_ch = model.out_channels
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((x.shape[0], out_ch) + tuple(x.shape[2:])).astype(np.float32))
    xg = x.to(dev).requires_grad_(True)
    out = call(model, xg, y.to(dev) if y is not None else None, labels.to(dev))
    g, = torch.autograd.grad((out * w.to(dev)).sum(), xg)
    x64 = x.double().requires_grad_(True)
    p64 = {k: v.double() for k, v in p.items()}
    r = ref(p64, x64, y.double() if y is not None else None, labels.double())
    gr, = torch.autograd.grad((r * w.double()).sum(), x64)
    err = rel(g, gr)
    print('input-gradient parity %s %s centered=%s %s: %.2e' % (family, case, centered, precision, err))
    assert err <= TOL, (family, case, centered, precision, err)
    # the value itself is the network's (the training graph with dropout 0)
    assert rel(out, r) <= TOL


@pytest.mark.gpu
def test_eval_without_requires_grad_keeps_the_inference_path():
    model, _, _, x, y, labels = build('ddpm', 'uncond_tiny', None, 'fp32')
    model.eval()
    dev = torch.device('cuda:0')
    out = call(model, x.to(dev), None, labels.to(dev))
    assert not out.requires_grad and out.grad_fn is None


@pytest.mark.gpu
def test_y_requires_grad_raises():
    model, _, _, x, y, labels = build('ddpm', 'sr3_tiny', None, 'fp32')
    model.eval()
    dev = torch.device('cuda:0')
    with pytest.raises(NotImplementedError):
        call(model, x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True), labels.to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize('family,case,centered', [('ddpm', 'uncond_tiny', None), ('ddpm', 'sr3_tiny', None),
                                                  ('ncsnpp', 'ncsnpp_fourier_skip', None), ('ncsnpp', 'ncsnpp_positional_plain', None)])
def test_train_mode_dx_matches_operator_path(family, case, centered):
    dev = torch.device('cuda:0')
    grads = {}
    for executor in ('planned', 'operators'):
        model, _, _, x, y, labels = build(family, case, centered, 'fp32')
        model.train_executor = executor
        model.train_layout = 'nchw'             # (the operator path's first conv takes its data gradient in NCHW)
        if executor == 'planned':
            model.train_layout = 'nhwc'
        model.train()
        w = torch.from_numpy(np.random.RandomState(3).standard_normal((x.shape[0], model.out_channels) + tuple(x.shape[2:])).astype(
            np.float32)).to(dev)
        xg = x.to(dev).requires_grad_(True)
        out = call(model, xg, y.to(dev) if y is not None else None, labels.to(dev))
        (out * w).sum().backward()
        assert xg.grad is not None, executor
        grads[executor] = xg.grad.detach().cpu()
    err = rel(grads['planned'], grads['operators'].double())
    assert err <= TOL, (family, case, err)


@pytest.mark.gpu
def test_train_mode_without_input_grad_returns_none():
    model, _, _, x, y, labels = build('ddpm', 'uncond_tiny', None, 'fp32')
    model.train()
    dev = torch.device('cuda:0')
    xg = x.to(dev)
    out = call(model, xg, None, labels.to(dev))
    out.sum().backward()
    assert xg.grad is None
    assert all(p.grad is not None for p in model.parameters() if p.requires_grad)


def _planned(model, x, y, labels, B):
    """csd_unet_train_forward into a private workspace; -> (table, ws, d_out)"""
    from conditional_score_diffusion_amd._lib import check, current_stream, lib, ptr
    dev = x.device
    params = model._train_params()
    table = (ctypes.c_void_p * len(params))(*[q.data_ptr() for q in params])
    ws = torch.empty(lib().csd_unet_train_workspace_bytes(model._h, B, 0.0), dtype=torch.uint8, device=dev)
    out = torch.empty(B, model.out_channels, model.image_size, model.image_size, device=dev)
    check(lib().csd_unet_train_forward(model._h, table, ptr(ws), ws.numel(), ptr(x), ptr(y), ptr(labels), ptr(out), B, 0.0, 0, 1,
                                       current_stream(dev)), 'train_forward')
    return params, table, ws, out


@pytest.mark.gpu
@pytest.mark.parametrize('family,case', [('ddpm', 'sr3_tiny'), ('ncsnpp', 'ncsnpp_fourier_skip')])
def test_backward_ex_consistency(family, case):
    from conditional_score_diffusion_amd._lib import check, current_stream, lib, ptr
    model, _, _, x, y, labels = build(family, case, None, 'fp16x3')
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(5)
    B0 = 4
    S, cx, cy = model.image_size, model.x_channels, model.y_channels
    X = torch.from_numpy(rs.uniform(-1, 1, size=(B0, cx, S, S)).astype(np.float32)).to(dev)
    Y = torch.from_numpy(rs.uniform(0, 1, size=(B0, cy, S, S)).astype(np.float32)).to(dev) if cy else None
    L = torch.tensor([3.0, 120.5, 600.0, 998.0][:B0], device=dev) if family == 'ddpm' else torch.tensor([-2.0, 0.5, 1.5, 3.0], device=dev)
    D = torch.from_numpy(rs.standard_normal((B0, model.out_channels, S, S)).astype(np.float32)).to(dev)
    s = current_stream(dev)

    def run(mode, B=B0):
        xb, yb, lb, db = X[:B].contiguous(), (Y[:B].contiguous() if cy else None), L[:B].contiguous(), D[:B].contiguous()
        params, table, ws, _ = _planned(model, xb, yb, lb, B)
        gr = [torch.empty_like(q) for q in params] if mode != 'dx' else None
        gt = (ctypes.c_void_p * len(gr))(*[g.data_ptr() for g in gr]) if gr else None
        dx = torch.empty(B, cx, S, S, device=dev) if mode != 'grads' else None
        if mode == 'legacy':
            check(lib().csd_unet_backward(model._h, table, gt, ptr(ws), ws.numel(), ptr(db), B, 1, s), 'backward')
            dx = None
        else:
            check(lib().csd_unet_backward_ex(model._h, table, gt, ptr(dx), ptr(ws), ws.numel(), ptr(db), B, 1, s), 'backward_ex')
        torch.cuda.synchronize()
        return gr, dx

    g_legacy, _ = run('legacy')
    g_both, dx_both = run('both')
    _, dx_only = run('dx')
    assert torch.equal(dx_only, dx_both)                       # d_x does not depend on whether parameter gradients are formed
    for a, b in zip(g_legacy, g_both):
        assert torch.equal(a, b)                               # parameter gradients unchanged by d_x
    _, dx_one = run('dx', B=1)
    assert rel(dx_one[0], dx_only[0].cpu().double()) <= 1e-5   # row 0 of B = 4 = the B = 1 result
    assert dx_only.abs().max().item() > 0


@pytest.mark.gpu
def test_backward_ex_needs_an_output():
    from conditional_score_diffusion_amd._lib import current_stream, lib, ptr
    model, _, _, x, y, labels = build('ddpm', 'uncond_tiny', None, 'fp32')
    dev = torch.device('cuda:0')
    xb, lb = x.to(dev).contiguous(), labels.to(dev).contiguous()
    params, table, ws, out = _planned(model, xb, None, lb, xb.shape[0])
    rc = lib().csd_unet_backward_ex(model._h, table, None, None, ptr(ws), ws.numel(), ptr(torch.ones_like(out)), xb.shape[0], 1,
                                    current_stream(dev))
    assert rc != 0
