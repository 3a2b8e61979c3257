"""progressive_input = 'residual' on the planned NCSN++ graph (MI355X): the FIR pyramid convolution alone (csd_fir_pyr_conv) against
float64 torch, input gradients against the oracle's float64 autograd, planned training against the operator twin, batch independence,
the fused PC loop and the probability-flow likelihood (fused against the generic autograd path; the network's input gradient itself is
pinned to the oracle above - an oracle-driven ODE solve of this network takes many minutes on the host)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import score_oracle as so

DEV = torch.device('cuda:0')
ASYM = (1.0, 2.0, 4.0, 0.5)


def pyr_ref64(x, w, b, res, taps, scale):
    """layerspp.Downsample(with_conv=True) in float64 on NCHW: conv_downsample_2d (upfirdn2d = depthwise correlation with the flipped
    normalised FIR on the (2, 2)-padded input, then a VALID stride-2 conv) or, taps None, F.pad(0, 1, 0, 1) + stride-2 conv"""
    x, w = x.double(), w.double()
    C = x.shape[1]
    if taps is None:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    else:
        k = torch.tensor(taps, dtype=torch.float64)
        k2 = torch.outer(k, k)
        k2 = torch.flip(k2 / k2.sum(), [0, 1])
        z = F.conv2d(F.pad(x, (2, 2, 2, 2)), k2[None, None].repeat(C, 1, 1, 1), groups=C)
        y = F.conv2d(z, w, stride=2)
    if b is not None:
        y = y + b.double()[None, :, None, None]
    if res is not None:
        y = y + res.double()
    return y * scale


SHAPES = [(3, 128, 32, 3), (6, 128, 32, 1), (3, 256, 16, 130), (128, 256, 16, 3), (256, 256, 8, 3), (128, 128, 4, 130), (256, 128, 4, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('taps', [(1, 3, 3, 1), ASYM, None], ids=['fir1331', 'asym', 'nofir'])
@pytest.mark.parametrize('with_res,scale', [(False, 1.0), (True, 1.0 / np.sqrt(2.0))], ids=['plain', 'residual'])
@pytest.mark.parametrize('Cin,Cout,S,B', SHAPES)
def test_fir_pyr_conv_vs_float64(Cin, Cout, S, B, taps, with_res, scale):
    from conditional_score_diffusion_amd import ops
    rs = np.random.RandomState(Cin * 7 + Cout + S + B)
    x = torch.from_numpy(rs.standard_normal((B, Cin, S, S)).astype(np.float32) * 2.0)
    w = torch.from_numpy((rs.uniform(-1, 1, (Cout, Cin, 3, 3)) / np.sqrt(9.0 * Cin)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(Cout).astype(np.float32))
    res = torch.from_numpy(rs.standard_normal((B, Cout, S // 2, S // 2)).astype(np.float32)) if with_res else None
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)        # noqa: E731
    args = (nhwc(x), w.to(DEV), b.to(DEV), nhwc(res) if res is not None else None)
    got = ops.fir_pyr_conv(*args, fir_kernel=taps, out_scale=scale)
    again = ops.fir_pyr_conv(*args, fir_kernel=taps, out_scale=scale)
    torch.cuda.synchronize()
    ref = pyr_ref64(x, w, b, res, taps, scale).permute(0, 2, 3, 1)
    err = (got.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 2e-6 * max(1.0, np.sqrt(9.0 * Cin) / 8.0), err
    assert torch.equal(got, again)


@pytest.mark.gpu
def test_fir_pyr_conv_rejects_bad_shapes():
    from conditional_score_diffusion_amd import ops
    x = torch.randn(2, 8, 8, 3, device=DEV)
    w = torch.randn(16, 4, 3, 3, device=DEV)
    with pytest.raises(RuntimeError):
        ops.fir_pyr_conv(x, w)
    with pytest.raises(RuntimeError):
        ops.fir_pyr_conv(torch.randn(2, 7, 7, 4, device=DEV), w)
    x4 = torch.randn(2, 8, 8, 4, device=DEV)
    with pytest.raises(RuntimeError):                 # a short bias would be read past its end
        ops.fir_pyr_conv(x4, w, torch.zeros(15, device=DEV))
    with pytest.raises(RuntimeError):
        ops.fir_pyr_conv(x4, w, res=torch.zeros(2, 4, 4, 15, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------------------
def paired_residual_config():
    return cases.make_ncsnpp_config(name='ncsnpp_paired', channels=6, nf=32, ch_mult=(1, 2), attn_resolutions=(16,),
                                    progressive='none', progressive_input='residual')


def build(case, centered=None, precision='fp32', name=None):
    """-> (model on the GPU, params, cfg, x, labels); case None: the paired residual config"""
    from conditional_score_diffusion_amd.models import utils as mutils
    if case is None:
        cfg = paired_residual_config()
        B = 2
        rs = np.random.RandomState(321)
        x = torch.from_numpy(rs.uniform(0, 1, size=(B, 6, 16, 16)).astype(np.float32) * 3.0 - 1.0)
        labels = torch.from_numpy(np.log(np.array([0.02, 7.5], np.float32)))
    else:
        cfg, B, x, labels = cases.ncsnpp_case(case)
    if centered is not None:
        cfg.data.centered = centered
    cfg.model.csd_precision = precision
    cfg.model.dropout = 0.0
    if name is not None:
        cfg.model.name = name
    model = mutils.create_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    p = cases.ncsnpp_params(shapes, 5)
    model.load_state_dict(p)
    return model.to(DEV), p, cfg, x, labels


def call(model, cfg, x, labels):
    if cfg.model.name.startswith('ncsnpp_paired'):
        r = model({'x': x[:, :3], 'y': x[:, 3:]}, labels)
        return torch.cat([r['x'], r['y']], dim=1)
    return model(x, labels)


def rel(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item() / b.detach().cpu().double().abs().max().item()


@pytest.fixture
def oracle64(monkeypatch):
    te, fk = so.timestep_embedding, so.fir_kernel_2d
    monkeypatch.setattr(so, 'timestep_embedding', lambda *a, **k: te(*a, **k).double())
    monkeypatch.setattr(so, 'fir_kernel_2d', lambda *a, **k: fk(*a, **k).double())
    return so


@pytest.mark.gpu
@pytest.mark.parametrize('case,centered', [('ncsnpp_residual_input', None), ('ncsnpp_residual_input', True),
                                           ('ncsnpp_nofir_residual', None), ('ncsnpp_nofir_residual', True), (None, None)])
def test_eval_input_grad_vs_oracle(oracle64, case, centered):
    model, p, cfg, x, labels = build(case, centered)
    model.eval()
    paired = case is None
    w = torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(x.shape)).astype(np.float32))
    if paired:
        xg = x[:, :3].to(DEV).requires_grad_(True)
        r = model({'x': xg, 'y': x[:, 3:].to(DEV)}, labels.to(DEV))
        out = torch.cat([r['x'], r['y']], dim=1)
    else:
        xg = x.to(DEV).requires_grad_(True)
        out = model(xg, labels.to(DEV))
    g, = torch.autograd.grad((out * w.to(DEV)).sum(), xg)
    x64 = x.double()
    xr = (x64[:, :3] if paired else x64).clone().requires_grad_(True)
    inp = torch.cat([xr, x64[:, 3:]], dim=1) if paired else xr
    p64 = {k: v.double() for k, v in p.items()}
    ref = so.ncsnpp_forward(p64, cfg, inp, labels.double())
    gr, = torch.autograd.grad((ref * w.double()).sum(), xr)
    err = rel(g, gr)
    print('residual input-gradient parity %s centered=%s: %.2e' % (case, centered, err))
    assert err <= 1e-3, err
    assert rel(out, ref) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['ncsnpp_residual_input', 'ncsnpp_nofir_residual'])
def test_train_mode_dx_matches_operator_path(case):
    grads = {}
    for executor in ('planned', 'operators'):
        model, _, cfg, x, labels = build(case)
        model.train_executor = executor
        model.train()
        w = torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(x.shape)).astype(np.float32)).to(DEV)
        xg = x.to(DEV).requires_grad_(True)
        (model(xg, labels.to(DEV)) * w).sum().backward()
        assert xg.grad is not None, executor
        grads[executor] = xg.grad.detach().cpu()
    assert rel(grads['planned'], grads['operators']) <= 1e-3


@pytest.mark.gpu
def test_planned_training_of_the_paired_residual_config_matches_the_operator_twin():
    grads = {}
    for executor in ('planned', 'operators'):
        model, _, cfg, x, labels = build(None)
        model.train_executor = executor
        model.train()
        w = torch.from_numpy(np.random.RandomState(2).standard_normal(tuple(x.shape)).astype(np.float32)).to(DEV)
        out = call(model, cfg, x.to(DEV), labels.to(DEV))
        assert (getattr(model, '_train_ws', None) is not None) == (executor == 'planned')
        (out * w).sum().backward()
        grads[executor] = {k: q.grad.detach().cpu().double() for k, q in model.named_parameters() if q.requires_grad}
    ref = grads['operators']
    total = float(np.sqrt(sum(float((g ** 2).sum()) for g in ref.values())))
    assert set(grads['planned']) == set(ref) and len(ref) > 20
    for k, r in ref.items():
        g = grads['planned'][k]
        scale = max(float(r.abs().max()), float(r.norm()) / np.sqrt(r.numel()))
        assert float((g - r).abs().max()) <= 1e-3 * scale + 1e-6 * total / np.sqrt(r.numel()), (k, float((g - r).abs().max()), scale)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['ncsnpp_residual_input', 'cifar_like'])
def test_batch_of_65_and_69_returns_the_bits_of_batches_of_8(case):
    from conditional_score_diffusion_amd.models import utils as mutils
    if case == 'cifar_like':
        cfg = cases.make_ncsnpp_config(nf=32, ch_mult=(1, 2, 2, 2), attn_resolutions=(16,), image_size=32, progressive='none',
                                       progressive_input='residual')
    else:
        cfg, _, _, _ = cases.ncsnpp_case(case)
    cfg.model.csd_precision = 'fp16x3'
    model = mutils.create_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(cases.ncsnpp_params(shapes, 5))
    model = model.to(DEV).eval()
    S = cfg.data.image_size
    for B in (65, 69):
        rs = np.random.RandomState(B)
        x = torch.from_numpy(rs.uniform(-1, 1, size=(B, 3, S, S)).astype(np.float32)).to(DEV)
        labels = torch.from_numpy(np.log(rs.uniform(0.02, 30, size=B)).astype(np.float32)).to(DEV)
        with torch.no_grad():
            full = model(x, labels).clone()
            again = model(x, labels).clone()
            parts = torch.cat([model(x[i:i + 8], labels[i:i + 8]) for i in range(0, B, 8)])
        assert torch.equal(full, again)
        assert torch.equal(full, parts), (case, B, (full - parts).abs().max().item())


@pytest.mark.gpu
def test_fused_pc_loop_on_residual_ncsnpp_vs_oracle():
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import correctors, predictors, unconditional
    model, p, cfg, _, _ = build('ncsnpp_residual_input', precision='fp16x3')
    model.eval()
    B = 2
    smin, smax, P = 0.01, 50., 6
    sde = sde_lib.VESDE(sigma_min=smin, sigma_max=smax, N=1000)
    shape = (B, 3, 16, 16)
    tp = cases.tape([shape] * (1 + 2 * P), seed=21)
    fn = unconditional.get_pc_sampler(sde, shape, predictors.get_predictor('reverse_diffusion'),
                                      correctors.get_corrector('langevin'), snr=0.075, p_steps=P, c_steps=1, continuous=True,
                                      denoise=True, eps=1e-5)
    got, info = fn(model, noise_tape=tp)             # noise_tape is only accepted by the fused path
    ve = so.VE(smin, smax, 1000)

    def score_fn(x, t):
        std = ve.std(t)
        return so.ncsnpp_forward(p, cfg, x, torch.log(std)) / std[:, None, None, None]

    with torch.no_grad():
        ref = so.pc_sample_unconditional(score_fn, shape, so.NoiseTape(tp), ve, p_steps=P, snr=0.075, eps=1e-5, denoise=True)
    assert (got.cpu() - ref).abs().max().item() / smax < 2e-4


class _Generic(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net
        self.embedding_type = getattr(net, 'embedding_type', 'positional')

    def forward(self, x, labels):
        return self.net(x, labels)


def _agree(r1, r2):
    (b1, z1, n1), (b2, z2, n2) = r1, r2
    assert (b1.cpu().double() - b2.cpu().double()).abs().max().item() <= 1e-3, (b1, b2)
    zr = (z1.cpu().double() - z2.cpu().double()).abs().max().item() / z2.cpu().double().abs().max().item()
    assert zr <= 1e-3, zr
    assert abs(n1 - n2) <= max(12, 0.02 * n2), (n1, n2)


@pytest.mark.gpu
@pytest.mark.parametrize('sde_name,case', [('ve', 'ncsnpp_residual_input'), ('vp', 'ncsnpp_nofir_residual')])
def test_likelihood_of_the_residual_ncsnpp(sde_name, case):
    """VE on the Fourier-embedded NCSN++ (labels log sigma), VP on the positional DDPM++ form (labels 999 t), as the reference pairs them"""
    from conditional_score_diffusion_amd import likelihood, sde_lib
    model, p, cfg, x, labels = build(case)
    model.eval()
    rs = np.random.RandomState(17)
    x = torch.from_numpy(rs.uniform(0, 1, size=tuple(x.shape)).astype(np.float32))
    e = torch.from_numpy((rs.randint(0, 2, size=x.shape) * 2 - 1).astype(np.float32))
    sde = {'ve': lambda: sde_lib.VESDE(0.01, 5.0, 1000), 'vp': lambda: sde_lib.VPSDE(0.1, 20., 1000)}[sde_name]()
    fn = likelihood.get_likelihood_fn(sde, lambda v: v, rtol=1e-6, atol=1e-6, eps=1e-3)
    fused = fn(model, x.to(DEV), epsilon=e.to(DEV))
    generic = fn(_Generic(model), x.to(DEV), epsilon=e.to(DEV))
    assert np.isfinite(fused[0].cpu().numpy()).all()
    _agree(fused, generic)
