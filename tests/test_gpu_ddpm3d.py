"""-m gpu: the 3-D DDPM score networks (models/ddpm3d.py) and their operators (csrc/conv3d.hip).

Operator references: torch on the CPU in float64 (F.conv3d, F.avg_pool3d, F.interpolate).  Network references: the reference's own
outputs (tests/golden/ddpm3d.npz, written by tools/make_ddpm3d_goldens.py) and, for the ELU network, the float64 restatement
ddpm3d_cases.forward64.  Error = max-abs-diff / max-abs-ref.

Bounds:
  conv3d_block   3e-6 * max(1, sqrt(27 * Cin) / 8): the conv2d bound of test_gpu_ops.py at the 3-D reduction length, with the 3e-6 base
                 that conv3x3_block gets for its fused prologue.  torch's own fp32 F.conv3d on the CPU stays within it on every shape
                 of the sweep (worst 0.08 of the bound, test_torch_fp32_conv3d_within_bound).
  padding        1e-5 (a kernel that activates its padding misses by O(1)); pool 1e-6; upsample, repeatability: bitwise
  network        1e-4 (the bound tests/test_gpu_network.py holds the tiny 2-D networks to; the fp32 reference sits 5e-7 .. 9e-7 from float64)
  sampling       1e-3 (the project's trajectory parity bound)

Worst errors measured on the MI355X next to their bounds (the case with the largest error / bound ratio of each group):

  group                                                  fp32                 fp16x3               bound
  conv3d_block sweep (error / bound)                     2.0e-06 (0.11)   1.8e-07 (0.06)   3e-6 * max(1, sqrt(27 Cin) / 8)
  padding after the prologue                             5.5e-06             3.5e-07             1e-5
  avg_pool3d_2 (nearest_up2_3d: bitwise)                 1.8e-07                                  1e-6
  groupnorm_scale_shift against F.group_norm             6.1e-08                                  3e-6
  network forward vs reference, case A                   1.9e-06             1.2e-06             1e-4
                                case B                   1.9e-06             1.3e-06             1e-4
                                case C                   1.1e-06             9.3e-07             1e-4
  ELU network (case A) vs float64 restatement            1.6e-06             1.2e-06             1e-4
  PC sampling vs reference, S1 (cVESDE, SR3)                                  3.9e-07             1e-3
                            S2 (two-SDE pair)                                 5.1e-07             1e-3
  repeatability, batch independence, out-of-domain: exact checks
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddpm3d_cases as dc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


_ACT64 = {'none': lambda v: v, 'swish': F.silu, 'relu': F.relu, 'elu': F.elu, 'lrelu': lambda v: F.leaky_relu(v, 0.2)}

# B, (D, H, W), C0, C1, Cout, norm, bias, temb, res, out_scale, act
SWEEP = [
    (1, (1, 1, 1), 32, 0, 32, True, True, False, False, 1.0, 'swish'),          # extent 1
    (3, (2, 2, 2), 64, 0, 2, True, True, False, False, 1.0, 'swish'),           # extent 2, the paired head
    (1, (12, 12, 2), 128, 0, 32, True, False, True, False, 1.0, 'swish'),       # the bottom level of 96 x 96 x 16: the 8 x 8 x 2 brick
    (3, (3, 5, 2), 64, 32, 64, True, True, True, False, 1.0, 'swish'),          # ragged, virtual concat 96 = 64 | 32
    (1, (5, 7, 3), 1, 0, 32, False, True, False, False, 1.0, 'none'),           # the stem: K padded with zeros / direct kernel
    (3, (5, 7, 3), 2, 0, 64, False, False, False, False, 1.0, 'none'),
    (1, (9, 17, 16), 64, 0, 64, True, True, True, True, 0.70710678, 'swish'),   # 4 K chunks, 2 cout tiles, 36 bricks, everything on
    (3, (5, 7, 3), 32, 0, 96, False, True, False, True, 1.0, 'none'),           # the shortcut form (no prologue), 3 cout tiles
    (1, (3, 5, 2), 32, 0, 1, True, True, False, False, 1.0, 'elu'),             # the 1-channel head, another activation
    (1, (5, 7, 3), 96, 0, 96, True, True, True, True, 1.0, 'lrelu'),
    (3, (2, 2, 2), 128, 0, 64, False, False, True, False, 0.5, 'none'),
]


def conv_case(spec, seed=0):
    B, vol, C0, C1, Cout, norm, bias, temb, res, out_scale, act = spec
    Cin = C0 + C1
    rs = np.random.RandomState(100 + seed)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))    # noqa: E731
    d = dict(x0=2.0 * t(B, *vol, C0), x1=2.0 * t(B, *vol, C1) if C1 else None,
             w=t(Cout, Cin, 3, 3, 3) * float(np.sqrt(2.0 / (27 * (Cin + Cout)))),
             bias=0.1 * t(Cout) if bias else None, nscale=1.0 + 0.3 * t(B, Cin) if norm else None, nshift=0.5 * t(B, Cin) if norm else None,
             temb=0.3 * t(B, Cout + 5) if temb else None, res=t(B, *vol, Cout) if res else None)
    return d


def conv_ref64(d, spec):
    B, vol, C0, C1, Cout, norm, bias, temb, res, out_scale, act = spec
    x = d['x0'] if d['x1'] is None else torch.cat([d['x0'], d['x1']], dim=-1)
    x = x.double()
    if norm:
        x = _ACT64[act](x * d['nscale'].double()[:, None, None, None, :] + d['nshift'].double()[:, None, None, None, :])
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), d['w'].double(), None if d['bias'] is None else d['bias'].double(), padding=1)
    y = y.permute(0, 2, 3, 4, 1)
    if temb:
        y = y + d['temb'].double()[:, None, None, None, :Cout]
    if res:
        y = y + d['res'].double()
    return y * out_scale


def conv_gpu(d, spec, precision):
    from conditional_score_diffusion_amd import ops
    B, vol, C0, C1, Cout, norm, bias, temb, res, out_scale, act = spec
    g = {k: (None if v is None else v.to(dev())) for k, v in d.items()}
    return ops.conv3d_block(g['x0'], g['w'], g['bias'], x1=g['x1'], nscale=g['nscale'], nshift=g['nshift'], act=act if norm else 'swish',
                            temb=g['temb'], res=g['res'], out_scale=out_scale, precision=precision)


def conv_bound(spec):
    return 3e-6 * max(1.0, np.sqrt(27 * (spec[2] + spec[3])) / 8)


@pytest.fixture(scope='module')
def sweep_refs():
    out = []
    for spec in SWEEP:
        d = conv_case(spec)
        out.append((d, conv_ref64(d, spec)))
    return out


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('idx', range(len(SWEEP)))
def test_conv3d_block_sweep(sweep_refs, idx, precision):
    spec = SWEEP[idx]
    d, ref = sweep_refs[idx]
    y = conv_gpu(d, spec, precision)
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.isfinite(y).all()
    e, b = rel(y, ref), conv_bound(spec)
    print('conv3d_block %s B=%d %s C=%d+%d->%d: %.3e (bound %.3e, ratio %.2f)' % (precision, spec[0], spec[1], spec[2], spec[3], spec[4], e, b, e / b))
    assert e < b


def test_torch_fp32_conv3d_within_bound(sweep_refs):
    """the bound is not tighter than fp32 itself: torch's own fp32 evaluation on the CPU stays within it"""
    worst = 0.0
    for spec, (d, ref) in zip(SWEEP, sweep_refs):
        B, vol, C0, C1, Cout, norm, bias, temb, res, out_scale, act = spec
        x = d['x0'] if d['x1'] is None else torch.cat([d['x0'], d['x1']], dim=-1)
        if norm:
            x = {'swish': F.silu, 'elu': F.elu, 'lrelu': lambda v: F.leaky_relu(v, 0.2), 'relu': F.relu}[act](
                x * d['nscale'][:, None, None, None, :] + d['nshift'][:, None, None, None, :])
        y = F.conv3d(x.permute(0, 4, 1, 2, 3), d['w'], d['bias'], padding=1).permute(0, 2, 3, 4, 1)
        if temb:
            y = y + d['temb'][:, None, None, None, :Cout]
        if res:
            y = y + d['res']
        worst = max(worst, rel(y * out_scale, ref) / conv_bound(spec))
    print('torch fp32 F.conv3d, worst error / bound over the sweep: %.2f' % worst)
    assert worst < 1.0


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('vol,cin,cout', [((3, 5, 2), 32, 32), ((5, 9, 5), 16, 2), ((2, 2, 2), 4, 3)])
def test_padding_applied_after_prologue(vol, cin, cout, precision):
    """constant input, large positive shift, weight of ones: every output = (taps inside the volume) * Cin * act(c + shift)"""
    from conditional_score_diffusion_amd import ops
    B = 2
    x = torch.full((B,) + vol + (cin,), 0.25, device=dev())
    w = torch.ones(cout, cin, 3, 3, 3, device=dev())
    ns = torch.ones(B, cin, device=dev())
    nh = torch.full((B, cin), 4.0, device=dev())
    y = ops.conv3d_block(x, w, nscale=ns, nshift=nh, act='swish', precision=precision)
    count = F.conv3d(torch.ones(1, 1, *vol, dtype=torch.float64), torch.ones(1, 1, 3, 3, 3, dtype=torch.float64), padding=1)[0, 0]
    val = float(F.silu(torch.tensor(4.25, dtype=torch.float64)))
    ref = (count * cin * val)[None, ..., None].expand(B, *vol, cout)
    e = rel(y, ref)
    print('padding %s %s %d->%d: %.3e' % (precision, vol, cin, cout, e))
    assert e < 1e-5
    # and element-wise at the corner, where only 8 (or fewer) of the 27 taps are inside
    corner = float(y[0, 0, 0, 0, 0]) / (cin * val)
    assert abs(corner - float(count[0, 0, 0])) < 1e-3


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_repeatable_and_batch_independent(precision):
    spec = (3, (5, 7, 3), 64, 32, 64, True, True, True, True, 0.70710678, 'swish')
    d = conv_case(spec, seed=7)
    y1 = conv_gpu(d, spec, precision)
    y2 = conv_gpu(d, spec, precision)
    assert torch.equal(y1, y2)
    one = {k: (v[1:2].contiguous() if v is not None and k not in ('w', 'bias') else v) for k, v in d.items()}
    y_one = conv_gpu(one, (1,) + spec[1:], precision)
    assert torch.equal(y_one[0], y1[1])


def test_out_of_domain_raises_and_writes_nothing():
    from conditional_score_diffusion_amd import _lib, ops
    from conditional_score_diffusion_amd._lib import current_stream, lib, ptr
    B, vol, C0, C1, Cout = 1, (3, 5, 2), 24, 16, 32
    x0 = torch.randn(B, *vol, C0, device=dev())
    x1 = torch.randn(B, *vol, C1, device=dev())
    w = torch.randn(Cout, C0 + C1, 3, 3, 3, device=dev())
    with pytest.raises(RuntimeError, match='multiples of 16'):
        ops.conv3d_block(x0, w, x1=x1)
    for prec in ('fp32', 'fp16x3'):
        y = torch.full((B,) + vol + (Cout,), -7.0, device=dev())
        sc = torch.empty(int(lib().csd_conv3d_block_scratch_bytes(C0 + C1, Cout)), dtype=torch.uint8, device=dev())
        rc = lib().csd_conv3d_block(ptr(x0), ptr(x1), ptr(w), None, None, None, 1, None, 0, None, 1.0, ptr(y), B, C0, C1, Cout, *vol,
                                    _lib.PREC_IDS[prec], ptr(sc), current_stream(dev()))
        torch.cuda.synchronize()
        assert rc == -1                       # CSD_ERR_INVALID
        assert bool((y == -7.0).all())
    # the two precisions that are not provided name the two that are
    x = torch.randn(1, 2, 2, 2, 32, device=dev())
    w = torch.randn(32, 32, 3, 3, 3, device=dev())
    for prec in ('fp16', 'fp16f8'):
        with pytest.raises(RuntimeError, match=r'fp16x3.*fp32'):
            ops.conv3d_block(x, w, precision=prec)


@pytest.mark.parametrize('vol,C', [((2, 2, 2), 32), ((4, 6, 2), 64), ((6, 10, 4), 3), ((12, 20, 8), 32)])
def test_pool_and_upsample(vol, C):
    from conditional_score_diffusion_amd import ops
    B = 2
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((B,) + vol + (C,)).astype(np.float32))
    xg = x.to(dev())
    up = ops.nearest_up2_3d(xg)
    ref_up = F.interpolate(x.permute(0, 4, 1, 2, 3), scale_factor=2, mode='nearest').permute(0, 2, 3, 4, 1)
    assert torch.equal(up.cpu(), ref_up)
    pool = ops.avg_pool3d_2(xg)
    ref_pool = F.avg_pool3d(x.double().permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1)
    e = rel(pool, ref_pool)
    print('avg_pool3d_2 %s C=%d: %.3e' % (vol, C, e))
    assert tuple(pool.shape) == tuple(ref_pool.shape) and e < 1e-6
    with pytest.raises(RuntimeError, match='even'):
        ops.avg_pool3d_2(xg[:, :, :, :1].contiguous())


def test_groupnorm_scale_shift():
    from conditional_score_diffusion_amd import ops
    rs = np.random.RandomState(9)
    B, vol, C0, C1 = 3, (3, 5, 2), 64, 32
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))    # noqa: E731
    x0, x1, gamma, beta = 2.0 * t(B, *vol, C0) + 0.5, t(B, *vol, C1), 1.0 + 0.1 * t(C0 + C1), 0.1 * t(C0 + C1)
    ns, nh = ops.groupnorm_scale_shift(x0.to(dev()), gamma.to(dev()), beta.to(dev()), x1=x1.to(dev()))
    x = torch.cat([x0, x1], dim=-1).double()
    ref = F.group_norm(x.permute(0, 4, 1, 2, 3), 32, gamma.double(), beta.double(), eps=1e-6).permute(0, 2, 3, 4, 1)
    got = x * ns.cpu().double()[:, None, None, None, :] + nh.cpu().double()[:, None, None, None, :]
    e = rel(got, ref)
    print('groupnorm_scale_shift: %.3e' % e)
    assert e < 3e-6


# ---- networks ---------------------------------------------------------------------------------------------------------------------
def build(case, precision, nonlinearity='swish'):
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = dc.make_config(case, nonlinearity=nonlinearity, precision=precision)
    model = mutils.create_model(cfg)
    p = dc.params(case)
    model.load_state_dict(p)
    return cfg, p, model.to(dev()).eval()


def gpu_inputs(case):
    x, y, labels = dc.case_inputs(case)
    return x.to(dev()), None if y is None else y.to(dev()), labels.to(dev())


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', sorted(dc.CASES))
def test_network_forward_vs_reference(case, precision):
    cfg, p, model = build(case, precision)
    out = dc.call(model, case, *gpu_inputs(case))
    ref = torch.from_numpy(dc.golden()['out_' + case])
    assert tuple(out.shape) == tuple(ref.shape) and torch.isfinite(out).all()
    e = rel(out, ref)
    print('network %s %s vs reference: %.3e' % (case, precision, e))
    assert e < 1e-4


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_network_forward_elu_vs_float64(precision):
    case = 'A'
    cfg, p, model = build(case, precision, nonlinearity='elu')
    out = dc.call(model, case, *gpu_inputs(case))
    ref = dc.forward64(p, case, *dc.case_inputs(case), nonlinearity='elu')
    swish = dc.forward64(p, case, *dc.case_inputs(case), nonlinearity='swish')
    assert rel(swish, ref) > 1e-2                      # (the activation matters on this network)
    e = rel(out, ref)
    print('network %s elu %s vs float64: %.3e' % (case, precision, e))
    assert e < 1e-4


@pytest.mark.parametrize('run', sorted(dc.SAMPLER_RUNS))
def test_pc_sampling_vs_reference(run):
    """the project's get_pc_conditional_sampler (step-by-step loop: the 3-D classes are not fusable) on 5-D tensors, with torch.randn /
    torch.randn_like reading the tape the reference's run read"""
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import conditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    g = dc.golden()
    if 'run_' + run not in g.files:
        pytest.fail('tests/golden/ddpm3d.npz has no run_%s' % run)
    case = dc.SAMPLER_RUNS[run]
    cfg, p, model = build(case, 'fp16x3')
    sx = sde_lib.cVESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    sde = {'x': sx, 'y': sde_lib.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX_Y, dc.N_SCALES)} if cfg.model.name == 'ddpm3D_paired' else sx
    _, y, _ = gpu_inputs(case)
    shape = (y.shape[0],) + tuple(cfg.data.shape_x)
    tape = dc.sampler_tape(run)
    it = iter(tape)
    o_randn, o_like = torch.randn, torch.randn_like

    def nxt(shp, device=None):
        z = next(it)
        assert tuple(z.shape) == tuple(shp), (tuple(z.shape), tuple(shp))
        return z.clone() if device is None else z.to(device)

    torch.randn = lambda *s, **k: nxt(s[0] if len(s) == 1 and not isinstance(s[0], int) else s, k.get('device'))
    torch.randn_like = lambda t, **k: nxt(t.shape, t.device)
    try:
        sampler = conditional.get_pc_conditional_sampler(sde, shape, get_predictor('conditional_reverse_diffusion'),
                                                         get_corrector('conditional_langevin'), snr=dc.SNR, p_steps=dc.P_STEPS, c_steps=1,
                                                         continuous=True, denoise=True, eps=dc.EPS)
        out, _ = sampler(model, y)
    finally:
        torch.randn, torch.randn_like = o_randn, o_like
    assert next(it, None) is None                      # every draw of the reference's run was consumed
    ref = torch.from_numpy(g['run_' + run])
    assert out.dim() == 5 and tuple(out.shape) == shape and torch.isfinite(out).all()
    e = rel(out, ref)
    print('sampling %s (%s): %.3e' % (run, cfg.model.name, e))
    assert e < 1e-3


def test_unconditional_sampler_runs_on_volumes():
    """VESDE + ddpm3D through get_pc_sampler's step-by-step loop: finite, 5-D"""
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import unconditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    cfg, p, model = build('C', 'fp16x3')
    sde = sde_lib.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    shape = (2,) + tuple(cfg.data.shape_x)
    torch.manual_seed(0)
    sampler = unconditional.get_pc_sampler(sde, shape, get_predictor('reverse_diffusion'), get_corrector('langevin'), snr=dc.SNR, p_steps=dc.P_STEPS,
                                           c_steps=1, continuous=True, denoise=True, eps=dc.EPS)
    out = sampler(model)
    out = out[0] if isinstance(out, (tuple, list)) else out
    assert out.dim() == 5 and tuple(out.shape) == shape and torch.isfinite(out).all()
