"""The training-side kernels (csrc/backward.hip, wgrad_bf16.hip, train_nhwc.hip, optim.hip and the data-gradient use of the forward
convolutions) one operator at a time, at the shapes the full-size SR3-160 training step runs and at the ragged / rectangular /
split-K-edge shapes no network-level test reaches.  Every reference is plain torch or numpy in float64 on the CPU (gradients: torch
autograd of the float64 forward); the metric for tensors is the project's  max|got - ref| / max|ref|  per output tensor.

The case lists and reference builders of this file are imported by tests/test_train_ops_sensitivity.py, which shows on the CPU that
float32 torch passes every bound below and that a set of subtly wrong references (H/W swapped, a lost K-split, an unflipped weight,
GroupNorm statistics over one channel too many, an unscaled softmax, Adam without bias correction) miss them by more than 10x.

Worst error measured on the MI355X per family, beside its bound (every figure is printed by the test that asserts it):

==============================================  ==========  =======================================================
family                                          worst       bound
==============================================  ==========  =======================================================
conv fp32: y / dx / dw / db                     2.0e-6      1e-5
conv fp16x3: y / dx / db                        1.3e-6      1e-5
conv fp16x3: dw (split-bf16, dy * 1e-4)         2.8e-5      5e-5
conv fp16x3: dw (bf16 resampling rebuild)       2.9e-5      5e-5
GroupNorm(+act): y                              1.3e-7      1e-5
GroupNorm(+act): dx / dgamma / dbeta            2.9e-7      2e-5
attention: out                                  1.6e-6      1e-5
attention: dq / dk / dv                         1.5e-6      2e-5
csd_bgemm                                       1.0e-6      1e-5
fp64 reductions (error / derived bound)         0 (exact)   1 (bound: 2^-24 |ref| + n 2^-52 sum|x|)
csd_sumpool2_nhwc (error / bound)               0.75        1 (bound: 2 fp32 ulps of sum|terms|)
zero-insert / nearest-up2 / bias-add            bit-equal   bit-equal
csd_upfirdn2d, anisotropic                      6.0e-8      1e-6
csd_adam_step: param / m / v / ema              7.1e-8      16 * 2^-24 = 9.5e-7
csd_global_norm (relative)                      3.3e-8      2^-23 = 1.2e-7
csd_ema_update                                  4.9e-8      4 * 2^-24 = 2.4e-7
==============================================  ==========  =======================================================
"""
import collections
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_network import dev

pytestmark = pytest.mark.gpu

F64 = torch.float64


def rel(got, ref):
    """the project's tensor metric: max|got - ref| / max|ref|"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check(family, what, err, bound):
    """print the figure (the module docstring's table is filled from these lines), then assert it"""
    print('[train-ops] %s | %s | err %.3e | bound %.3e' % (family, what, err, bound))
    assert err < bound, (family, what, err, bound)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def to_nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# =====================================================================================================================
# 1. convolution backward
# =====================================================================================================================
IN_NHWC, OUT_NHWC = 1, 2
# S / per: the K-split schedule of the fp32 weight gradient (`wgrad_splits` in csrc/backward.hip, restated by wgrad_splits() below;
# the sensitivity file asserts that the restatement gives these values).  nhwc: the layout flags of the grad_ops_nhwc variant.
ConvCase = collections.namedtuple('ConvCase', 'n B Cin Cout H W k stride up2 S per nhwc')
CONV_CASES = [
    ConvCase(1, 7, 96, 96, 20, 20, 3, 1, False, 35, 4, 3),     # full-size 20^2 level at the 8-way batch: S = 35, per = 4
    ConvCase(2, 3, 288, 288, 5, 5, 3, 1, False, 1, 15, 3),     # S = 1 (per = 15: all rows in one split)
    ConvCase(3, 3, 96, 96, 10, 10, 3, 1, False, 4, 8, 3),      # S = 4, per = 8 over 30 rows: last split has 6 rows, splits straddle samples
    ConvCase(4, 5, 40, 72, 9, 7, 3, 1, False, 4, 12, 3),       # odd, rectangular, channels not a multiple of 32; S = 4, per = 12, last split 9 rows
    ConvCase(5, 2, 192, 96, 10, 10, 1, 1, False, 2, 10, 3),    # NIN; S = 2, per = 10
    ConvCase(6, 1, 6, 96, 40, 24, 3, 1, False, 10, 4, OUT_NHWC),   # stem, rectangular, the only B = 1 row (NCHW in -> NHWC out); S = 10, per = 4
    ConvCase(7, 2, 96, 3, 24, 40, 3, 1, False, 12, 4, IN_NHWC),    # head (NHWC in -> NCHW out); S = 12, per = 4
    ConvCase(8, 3, 64, 64, 12, 20, 3, 2, False, 2, 9, 3),      # rectangular Downsample; S = 2, per = 9 over 18 output rows
    ConvCase(9, 2, 64, 96, 6, 10, 3, 1, True, 6, 4, 3),        # rectangular Upsample; S = 6, per = 4 over 24 output rows
    ConvCase(10, 2, 32, 128, 20, 12, 3, 2, False, 2, 19, 3),   # quad-schedule stride 2 with Cout % 128; S = 2, per = 19 over 20 rows: a one-row last split
    ConvCase(11, 2, 96, 192, 10, 6, 3, 1, True, 6, 7, 3),      # quad-schedule up2 with Cout % 96; S = 6, per = 7 over 40 rows: last split 5 rows
]
CONV_IDS = ['case%d' % c.n for c in CONV_CASES]
DY_SMALL = 1e-4          # the split-bf16 weight gradient is fed small gradients, as test_split_bf16_weight_gradient does


def wgrad_splits(B, OH, OW, Cin, Cout, ksize=3):
    """(S, per) of `wgrad_splits` in csrc/backward.hip (default schedule): K-splits are runs of the B * OH output rows"""
    cdiv = lambda a, b: (a + b - 1) // b
    nrows = B * OH
    tiles = cdiv(Cout, 32) * cdiv(Cin, 32)
    S = max(1, 1024 // tiles)
    min_rows = max(4, cdiv(64, OW))
    S = min(S, max(1, nrows // min_rows))
    per = cdiv(nrows, S)
    S = cdiv(nrows, per)
    for p2 in range(per, max(min_rows, per - 8) - 1, -1):
        s2 = cdiv(nrows, p2)
        if (s2 * tiles) % 8 == 0:
            per, S = p2, s2
            break
    return S, per


def conv_out_hw(c):
    s = 2 if c.up2 else 1
    return c.H * s // c.stride, c.W * s // c.stride


@functools.lru_cache(maxsize=None)
def conv_inputs(c):
    """float32 inputs (exactly what the kernels get): activations with a mean offset, everything else random and non-symmetric"""
    g = gen(1000 + c.n)
    OH, OW = conv_out_hw(c)
    x = randn(g, c.B, c.Cin, c.H, c.W) * 1.5 + 0.2
    w = randn(g, c.Cout, c.Cin, c.k, c.k) * (2.0 / math.sqrt(c.Cin * c.k * c.k))
    b = randn(g, c.Cout)
    dy = randn(g, c.B, c.Cout, OH, OW) + 0.3
    return {'x': x, 'w': w, 'b': b, 'dy': dy, 'dy_small': dy * DY_SMALL}


def conv_forward(x, w, b, c):
    """the reference convolution in the dtype of its operands (models/layers.py: ddpm_conv3x3 / NIN, Downsample, Upsample)"""
    u = F.interpolate(x, scale_factor=2, mode='nearest') if c.up2 else x
    if c.stride == 2:
        return F.conv2d(F.pad(u, (0, 1, 0, 1)), w, b, stride=2)
    return F.conv2d(u, w, b, padding=c.k // 2)


def conv_reference_of(inp, c, dtype=F64):
    """y, dx, dw, db (and dw for the small dy) by autograd of conv_forward in `dtype`"""
    x, w, b = (inp[k].detach().clone().to(dtype).requires_grad_(True) for k in ('x', 'w', 'b'))          # (never the cached inputs themselves)
    y = conv_forward(x, w, b, c)
    dx, dw, db = torch.autograd.grad(y, [x, w, b], inp['dy'].to(dtype), retain_graph=True)
    dw_small, = torch.autograd.grad(y, [w], inp['dy_small'].to(dtype))
    return {'y': y.detach(), 'dx': dx, 'dw': dw, 'db': db, 'dw_small': dw_small}


@functools.lru_cache(maxsize=None)
def conv_reference(c):
    return conv_reference_of(conv_inputs(c), c)


def conv_bounds(c, precision):
    """(bound of y / dx / db, bound of dw, does dw use the small dy).  fp32: the exact-fp32 MFMA kernels, 1e-5 everywhere.  fp16x3:
    forward and data gradient are fp32-class (1e-5, as test_nhwc_conv_on_the_quad_schedule); the weight gradient runs split-bf16
    operands: 5e-5 - with dy * 1e-4 on the stride-1 kernel, with dy as it is through the resampling rebuild (max(1e-5, 5e-5))"""
    if precision == 'fp32':
        return 1e-5, 1e-5, False
    resample = c.stride == 2 or c.up2
    return 1e-5, max(1e-5, 5e-5), not resample


def _run_conv_gpu(c, layout, precision):
    inp = conv_inputs(c)
    d = dev()
    wd, bd = inp['w'].to(d).requires_grad_(True), inp['b'].to(d).requires_grad_(True)
    kw = dict(stride=c.stride, downsample_pad=c.stride == 2, up2=c.up2, precision=precision)
    if layout == 'nchw':
        from conditional_score_diffusion_amd import grad_ops as G
        xd = inp['x'].to(d).requires_grad_(True)
        out = G.conv2d(xd, wd, bd, **kw)
        put, get_y, get_dx = (lambda t: t.to(d)), (lambda t: t), (lambda t: t)
    else:
        from conditional_score_diffusion_amd import grad_ops_nhwc as G
        in_nhwc, out_nhwc = bool(c.nhwc & IN_NHWC), bool(c.nhwc & OUT_NHWC)
        xd = (to_nhwc(inp['x']) if in_nhwc else inp['x']).to(d)
        xd.requires_grad_(in_nhwc)          # (the data gradient of the NCHW-input stem is not part of the training graph)
        out = G.conv2d(xd, wd, bd, layout=c.nhwc, **kw)
        put = (lambda t: to_nhwc(t).to(d)) if out_nhwc else (lambda t: t.to(d))
        get_y = to_nchw if out_nhwc else (lambda t: t)
        get_dx = to_nchw if in_nhwc else (lambda t: t)
    got = {'y': get_y(out.detach())}
    out.backward(put(inp['dy']), retain_graph=True)
    got['dw'], got['db'] = wd.grad.clone(), bd.grad.clone()
    if xd.grad is not None:
        got['dx'] = get_dx(xd.grad)
    got['dw_small'], = torch.autograd.grad(out, [wd], put(inp['dy_small']))
    return got


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('c', CONV_CASES, ids=CONV_IDS)
def test_conv_backward(c, layout, precision):
    """grad_ops.conv2d (NCHW ABI) and grad_ops_nhwc.conv2d: forward, data gradient (flipped / transposed weight packing, zero-insert
    and 2x2 sum for the resampling forms), weight gradient (split-K schedule at its edges; split-bf16 and its resampling rebuild in
    'fp16x3') and bias gradient"""
    ref = conv_reference(c)
    got = _run_conv_gpu(c, layout, precision)
    tol, tol_dw, small = conv_bounds(c, precision)
    fam = 'conv %s' % precision
    tag = 'case%d %s' % (c.n, layout)
    check(fam, tag + ' y', rel(got['y'], ref['y']), tol)
    if 'dx' in got:
        check(fam, tag + ' dx', rel(got['dx'], ref['dx']), tol)
    else:
        assert layout == 'nhwc' and not c.nhwc & IN_NHWC
    check(fam, tag + ' db', rel(got['db'], ref['db']), tol)
    if precision == 'fp32':
        check(fam, tag + ' dw', rel(got['dw'], ref['dw']), tol_dw)
        check(fam, tag + ' dw(small dy)', rel(got['dw_small'], ref['dw_small']), tol_dw)
    elif small:
        check(fam + ' dw split-bf16', tag + ' dw(small dy)', rel(got['dw_small'], ref['dw_small']), tol_dw)
    else:
        check(fam + ' dw bf16 resampling rebuild', tag + ' dw', rel(got['dw'], ref['dw']), tol_dw)


# =====================================================================================================================
# 2. GroupNorm(+act) backward
# =====================================================================================================================
GNCase = collections.namedtuple('GNCase', 'n B C H W groups act')
GN_CASES = [
    GNCase(1, 7, 288, 5, 5, 32, 'swish'),       # 9 channels per group; HW = 25 is less than a workgroup
    GNCase(2, 2, 192, 10, 10, 32, 'swish'),
    GNCase(3, 1, 576, 10, 10, 32, 'swish'),     # the up path's concat width; one pixel row per workgroup in gn_bwd_stats_nhwc_kernel
    GNCase(4, 2, 16, 12, 20, 4, 'swish'),       # NCSN++'s min(C/4, 32) groups; rectangular
    GNCase(5, 2, 128, 40, 40, 32, 'none'),      # many pixel chunks
    GNCase(6, 2, 32, 2, 2, 32, 'swish'),        # fewer pixels than pixel rows
    GNCase(7, 2, 64, 7, 9, 32, 'relu'),
    GNCase(8, 2, 64, 7, 9, 32, 'lrelu'),
    GNCase(9, 2, 64, 7, 9, 32, 'elu'),
]
GN_IDS = ['case%d_%s' % (c.n, c.act) for c in GN_CASES]
GN_EPS = 1e-6
GN_TOL_Y, GN_TOL_GRAD = 1e-5, 2e-5


def act_fn(u, act):
    if act == 'swish':
        return F.silu(u)
    if act == 'relu':
        return F.relu(u)
    if act == 'lrelu':
        return F.leaky_relu(u, 0.2)
    if act == 'elu':
        return F.elu(u)
    assert act == 'none'
    return u


@functools.lru_cache(maxsize=None)
def gn_inputs(c):
    g = gen(2000 + c.n)
    return {'x': randn(g, c.B, c.C, c.H, c.W) * 3 + 0.7, 'gamma': randn(g, c.C) * 0.5 + 1.0, 'beta': randn(g, c.C) * 0.3,
            'dy': randn(g, c.B, c.C, c.H, c.W) + 0.2}


def gn_forward(x, gamma, beta, c):
    return act_fn(F.group_norm(x, c.groups, gamma, beta, eps=GN_EPS), c.act)


def gn_reference_of(inp, c, dtype=F64, forward=gn_forward):
    x, ga, be = (inp[k].detach().clone().to(dtype).requires_grad_(True) for k in ('x', 'gamma', 'beta'))
    y = forward(x, ga, be, c)
    dx, dg, db = torch.autograd.grad(y, [x, ga, be], inp['dy'].to(dtype))
    return {'y': y.detach(), 'dx': dx, 'dgamma': dg, 'dbeta': db}


@functools.lru_cache(maxsize=None)
def gn_reference(c):
    return gn_reference_of(gn_inputs(c), c)


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('c', GN_CASES, ids=GN_IDS)
def test_groupnorm_act_backward(c, layout):
    """csd_groupnorm_act + csd_groupnorm_act_backward (one workgroup per (sample, group)) and the three-kernel NHWC backward"""
    inp, ref = gn_inputs(c), gn_reference(c)
    d = dev()
    gd, bd = inp['gamma'].to(d).requires_grad_(True), inp['beta'].to(d).requires_grad_(True)
    if layout == 'nchw':
        from conditional_score_diffusion_amd import grad_ops as G
        xd = inp['x'].to(d).requires_grad_(True)
        out = G.groupnorm_act(xd, gd, bd, c.groups, GN_EPS, c.act)
        out.backward(inp['dy'].to(d))
        y, dx = out.detach(), xd.grad
    else:
        from conditional_score_diffusion_amd import grad_ops_nhwc as G
        xd = to_nhwc(inp['x']).to(d).requires_grad_(True)
        out = G.groupnorm_act(xd, gd, bd, c.groups, GN_EPS, c.act)
        out.backward(to_nhwc(inp['dy']).to(d))
        y, dx = to_nchw(out.detach()), to_nchw(xd.grad)
    tag = 'case%d %s %s' % (c.n, c.act, layout)
    check('groupnorm y', tag, rel(y, ref['y']), GN_TOL_Y)
    check('groupnorm grad', tag + ' dx', rel(dx, ref['dx']), GN_TOL_GRAD)
    check('groupnorm grad', tag + ' dgamma', rel(gd.grad, ref['dgamma']), GN_TOL_GRAD)
    check('groupnorm grad', tag + ' dbeta', rel(bd.grad, ref['dbeta']), GN_TOL_GRAD)


# =====================================================================================================================
# 3. attention backward
# =====================================================================================================================
AttnCase = collections.namedtuple('AttnCase', 'B L C peaked')
ATTN_NHWC_CASES = [AttnCase(3, 400, 192, False), AttnCase(2, 100, 288, False), AttnCase(7, 25, 288, False),
                   AttnCase(2, 129, 96, False), AttnCase(2, 37, 32, False),
                   AttnCase(2, 400, 64, True)]      # peaked softmax: inputs x 2, the last key is 3 x query 0
ATTN_NCHW_CASES = [(2, 64, 16, 8), (3, 192, 20, 20)]       # B, C, H, W
ATTN_TOL_Y, ATTN_TOL_GRAD = 1e-5, 2e-5


@functools.lru_cache(maxsize=None)
def attn_inputs(c):
    """the packed [B, L, 3C] tensor (q | k | v per pixel) and d out [B, L, C]"""
    g = gen(3000 + c.L + c.C + c.B)
    if c.peaked:
        qkv = randn(g, c.B, c.L, 3 * c.C) * 2
        qkv[:, c.L - 1, c.C:2 * c.C] = qkv[:, 0, :c.C] * 3          # as test_attention_core_in_every_precision_mode
    else:
        qkv = randn(g, c.B, c.L, 3 * c.C) + 0.1
    return {'qkv': qkv, 'do': randn(g, c.B, c.L, c.C) + 0.2}


def attn_forward(q, k, v, C, scale=True):
    """models/layers.py:584-588 on [B, L, C] operands"""
    s = torch.einsum('bqc,bkc->bqk', q, k)
    if scale:
        s = s * (int(C) ** (-0.5))
    return torch.einsum('bqk,bkc->bqc', torch.softmax(s, dim=-1), v)


def attn_reference_of(inp, c, dtype=F64, scale=True):
    q, k, v = (t.detach().clone().to(dtype).requires_grad_(True) for t in inp['qkv'].split(c.C, dim=2))
    out = attn_forward(q, k, v, c.C, scale)
    dq, dk, dv = torch.autograd.grad(out, [q, k, v], inp['do'].to(dtype))
    return {'out': out.detach(), 'dq': dq, 'dk': dk, 'dv': dv}


@functools.lru_cache(maxsize=None)
def attn_reference(c):
    return attn_reference_of(attn_inputs(c), c)


def _check_attention(tag, got, ref):
    check('attention out', tag, rel(got['out'], ref['out']), ATTN_TOL_Y)
    for k in ('dq', 'dk', 'dv'):
        check('attention grad', tag + ' ' + k, rel(got[k], ref[k]), ATTN_TOL_GRAD)


@pytest.mark.parametrize('c', ATTN_NHWC_CASES, ids=lambda c: 'B%d_L%d_C%d%s' % (c.B, c.L, c.C, '_peaked' if c.peaked else ''))
def test_attention_backward_packed(c):
    """csd_attention_nhwc + csd_attention_backward_nhwc on the packed qkv tensor: the L = 400 / 100 / 25 levels of SR3-160 at their
    widths, key counts that are no multiple of a tile, a dominating late key"""
    from conditional_score_diffusion_amd import grad_ops_nhwc as G
    inp, ref = attn_inputs(c), attn_reference(c)
    qkv = inp['qkv'].reshape(c.B, c.L, 1, 3 * c.C).to(dev()).requires_grad_(True)
    out = G.attention(qkv)
    out.backward(inp['do'].reshape(c.B, c.L, 1, c.C).to(dev()))
    dq, dk, dv = qkv.grad.reshape(c.B, c.L, 3 * c.C).split(c.C, dim=2)
    _check_attention('packed B%d L%d C%d%s' % (c.B, c.L, c.C, ' peaked' if c.peaked else ''),
                     {'out': out.detach().reshape(c.B, c.L, c.C), 'dq': dq, 'dk': dk, 'dv': dv}, ref)


@pytest.mark.parametrize('B,C,H,W', ATTN_NCHW_CASES)
def test_attention_backward_nchw(B, C, H, W):
    """csd_attention + csd_attention_backward on q, k, v [B, C, H, W], one of them rectangular"""
    from conditional_score_diffusion_amd import grad_ops as G
    c = AttnCase(B, H * W, C, False)
    inp, ref = attn_inputs(c), attn_reference(c)
    plane = lambda t: t.transpose(1, 2).reshape(B, C, H, W).contiguous()          # [B, L, C] -> [B, C, H, W]
    back = lambda t: t.reshape(B, C, H * W).transpose(1, 2)
    q, k, v = (plane(t).to(dev()).requires_grad_(True) for t in inp['qkv'].split(C, dim=2))
    out = G.attention(q, k, v)
    out.backward(plane(inp['do']).to(dev()))
    _check_attention('nchw B%d C%d %dx%d' % (B, C, H, W),
                     {'out': back(out.detach()), 'dq': back(q.grad), 'dk': back(k.grad), 'dv': back(v.grad)}, ref)


# =====================================================================================================================
# 4. csd_bgemm on raw storage
# =====================================================================================================================
BGEMM_SHAPES = [(1, 1, 1), (64, 64, 16), (65, 63, 17), (400, 400, 192), (288, 400, 400), (5, 2048, 384)]
BGEMM_BATCH, BGEMM_ALPHA, BGEMM_TOL = 3, 0.37, 1e-5
SENTINEL = -12345.5


def bgemm_layouts(M, N, K):
    """name -> (A: (m stride, k stride, z stride, base offset), B: (k stride, n stride, z, offset), C: (m stride, n stride, z, offset)).
    The four loader orders on compact operands with padded, distinct z-strides; the packed-qkv form (row stride 3 * extent, the base
    pointer offset into the row); a transposed output."""
    out = {}
    for an, (sam, sak) in (('Am', (1, M)), ('Ak', (K, 1))):
        for bn, (sbk, sbn) in (('Bn', (N, 1)), ('Bk', (1, K))):
            out[an + bn] = ((sam, sak, M * K + 5, 0), (sbk, sbn, K * N + 3, 0), (N, 1, M * N + 7, 0))
    out['packed'] = ((3 * K, 1, 3 * K * M, K), (1, 3 * K, 3 * K * N, 2 * K), (3 * N, 1, 3 * N * M, N))
    out['Ct'] = ((K, 1, M * K + 5, 0), (N, 1, K * N + 3, 0), (1, M, M * N + 7, 0))
    return out


def _index(n0, n1, s0, s1, sz, off):
    z, i, j = torch.arange(BGEMM_BATCH).view(-1, 1, 1), torch.arange(n0).view(1, -1, 1), torch.arange(n1).view(1, 1, -1)
    return off + z * sz + i * s0 + j * s1


@pytest.mark.parametrize('order', ['AmBn', 'AmBk', 'AkBn', 'AkBk', 'packed', 'Ct'])
@pytest.mark.parametrize('M,N,K', BGEMM_SHAPES)
def test_bgemm(M, N, K, order):
    """csd_bgemm with arbitrary strides: every loader order, partial tiles in M, N and K, batch 3 with distinct z-strides, alpha, the
    row stride 3 * extent of the packed qkv calls, a transposed output; nothing outside the addressed output set is written"""
    from conditional_score_diffusion_amd import grad_ops as G
    la, lb, lc = bgemm_layouts(M, N, K)[order]
    ia, ib, ic = _index(M, K, *la), _index(K, N, *lb), _index(M, N, *lc)
    g = gen(4000 + M + N + K)
    a_flat, b_flat = randn(g, int(ia.max()) + 9) + 0.2, randn(g, int(ib.max()) + 9) + 0.2
    c_flat = torch.full((int(ic.max()) + 65,), SENTINEL)
    ref = BGEMM_ALPHA * torch.einsum('zmk,zkn->zmn', a_flat.double()[ia], b_flat.double()[ib])
    ad, bd, cd = a_flat.to(dev()), b_flat.to(dev()), c_flat.to(dev())
    G.bgemm(ad[la[3]:], bd[lb[3]:], cd[lc[3]:], M, N, K, la[:2], lb[:2], lc[:2], batch=BGEMM_BATCH, z=(la[2], lb[2], lc[2]),
            alpha=BGEMM_ALPHA)
    got = cd.cpu()
    check('bgemm', '%dx%dx%d %s' % (M, N, K, order), rel(got[ic], ref), BGEMM_TOL)
    untouched = torch.ones(got.numel(), dtype=torch.bool)
    untouched[ic.reshape(-1)] = False
    assert untouched.any() and bool((got[untouched] == SENTINEL).all())


# =====================================================================================================================
# 5. reductions with an fp64 contract
# =====================================================================================================================
def cancelling(rs, shape, axis):
    """1000 + randn with alternating signs along `axis`: the sum is small against sum|x|, so an fp32 accumulation fails"""
    x = (1000.0 + rs.standard_normal(shape)).astype(np.float32)
    sign = np.where(np.arange(shape[axis]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return x * sign.reshape([-1 if i == axis else 1 for i in range(len(shape))])


def fp64_sum_excess(got, x, axis):
    """max over the outputs of |got - ref| / (2^-24 |ref| + n 2^-52 sum|x|): fp64 accumulation in any order, then one rounding to
    fp32, keeps this at or below 1"""
    x64 = x.astype(np.float64)
    ref = x64.sum(axis=axis)
    bound = 2.0 ** -24 * np.abs(ref) + x.shape[axis] * 2.0 ** -52 * np.abs(x64).sum(axis=axis)
    return float((np.abs(got.astype(np.float64) - ref) / bound).max())


def fp32_sum(x, axis):
    """what the same reduction gives when it accumulates in float32 (the sanity check: it must NOT meet the bound).  The reduced axis
    is made the contiguous one first: torch's float32 sum over an outer axis comes out exact on this data, its vectorised sum over
    the inner axis keeps same-sign partial sums of several thousand per lane and rounds them"""
    inner = np.ascontiguousarray(np.moveaxis(x, axis, -1))
    return torch.from_numpy(inner).sum(dim=-1, dtype=torch.float32).numpy()


def test_sum_inner_accumulates_in_fp64():
    from conditional_score_diffusion_amd.grad_ops import _sum_inner
    rs = np.random.RandomState(51)
    fp32_fails = 0
    for rows in (1, 7, 2016):
        for inner in (1, 25, 400, 6400):
            x = cancelling(rs, (rows, inner), 1)
            got = _sum_inner(torch.from_numpy(x).to(dev()), rows).cpu().numpy()
            check('fp64 reductions', 'sum_inner %dx%d' % (rows, inner), fp64_sum_excess(got, x, 1), 1.0 + 1e-12)
            fp32_fails += fp64_sum_excess(fp32_sum(x, 1), x, 1) > 1.0
    assert fp32_fails > 0, 'the data does not tell an fp32 accumulation from an fp64 one'


def test_sum_rows_accumulates_in_fp64():
    from conditional_score_diffusion_amd.grad_ops import _sum_rows
    rs = np.random.RandomState(52)
    fp32_fails = 0
    for R in (1, 7, 64, 2048):
        for C in (3, 96, 100, 288):
            x = cancelling(rs, (R, C), 0)
            got = _sum_rows(torch.from_numpy(x).to(dev())).cpu().numpy()
            check('fp64 reductions', 'sum_rows %dx%d' % (R, C), fp64_sum_excess(got, x, 0), 1.0 + 1e-12)
            fp32_fails += fp64_sum_excess(fp32_sum(x, 0), x, 0) > 1.0
    assert fp32_fails > 0, 'the data does not tell an fp32 accumulation from an fp64 one'


@pytest.mark.parametrize('C', [4, 96, 288, 1024])
@pytest.mark.parametrize('B', [1, 7, 64])
def test_sum_pixels_nhwc_accumulates_in_fp64(B, C):
    from conditional_score_diffusion_amd.grad_ops_nhwc import _sum_pixels
    rs = np.random.RandomState(53 + B + C)
    fp32_fails = 0
    for HW in (1, 25, 1600):
        x = cancelling(rs, (B, HW, C), 1)
        got = _sum_pixels(torch.from_numpy(x).to(dev()).view(B, HW, 1, C)).cpu().numpy()
        check('fp64 reductions', 'sum_pixels B%d HW%d C%d' % (B, HW, C), fp64_sum_excess(got, x, 1), 1.0 + 1e-12)
        fp32_fails += fp64_sum_excess(fp32_sum(x, 1), x, 1) > 1.0
    assert fp32_fails > 0, 'the data does not tell an fp32 accumulation from an fp64 one'


# =====================================================================================================================
# 6. resampling helpers
# =====================================================================================================================
RESAMPLE_SHAPES = [(1, 3, 5, 4), (3, 10, 6, 36), (2, 20, 20, 288)]       # B, h, w, C


def zero_insert_reference(dy):
    B, h, w, C = dy.shape
    z = dy.new_zeros(B, 2 * h, 2 * w, C)
    z[:, 1::2, 1::2] = dy
    return z


def sumpool2_terms(x):
    """the four terms of every 2x2 block sum of x [B, 2h, 2w, C]"""
    return torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]])


def nearest_up2_reference(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


@pytest.mark.parametrize('B,h,w,C', RESAMPLE_SHAPES)
def test_resampling_helpers(B, h, w, C):
    """csd_zero_insert_odd_nhwc, csd_nearest_up2 and csd_bias_add_nhwc move or add single values: bit-equal to torch;
    csd_sumpool2_nhwc adds four: within 2 fp32 ulps of sum|terms|"""
    from conditional_score_diffusion_amd import grad_ops_nhwc as GN, ops
    from conditional_score_diffusion_amd._lib import check as ok, current_stream, lib, ptr
    g = gen(6000 + h + w + C)
    d = dev()
    small, big, bias = randn(g, B, h, w, C) + 0.2, randn(g, B, 2 * h, 2 * w, C) + 0.2, randn(g, B, C)
    z = torch.full((B, 2 * h, 2 * w, C), SENTINEL, device=d)
    sd = small.to(d)
    ok(lib().csd_zero_insert_odd_nhwc(ptr(sd), ptr(z), B, h, w, C, current_stream(d)), 'zero_insert_odd_nhwc')
    assert torch.equal(z.cpu(), zero_insert_reference(small))
    planes = small.permute(0, 3, 1, 2).contiguous()                      # [B, C, h, w]: csd_nearest_up2 is an NCHW operator
    assert torch.equal(ops.nearest_up2(planes.to(d)).cpu(), nearest_up2_reference(planes))
    assert torch.equal(GN.bias_add(sd, bias.to(d)).cpu(), small + bias[:, None, None, :])
    pooled = torch.full((B, h, w, C), SENTINEL, device=d)
    bd = big.to(d)
    ok(lib().csd_sumpool2_nhwc(ptr(bd), ptr(pooled), B, h, w, C, current_stream(d)), 'sumpool2_nhwc')
    terms = sumpool2_terms(big.double())
    bound = 2 * np.spacing(terms.abs().sum(0).numpy().astype(np.float32)).astype(np.float64)
    err = (pooled.cpu().double() - terms.sum(0)).abs().numpy()
    check('sumpool2', 'B%d %dx%d C%d' % (B, h, w, C), float((err / bound).max()), 1.0 + 1e-12)


# =====================================================================================================================
# 7. csd_upfirdn2d on the raw ABI with anisotropic arguments
# =====================================================================================================================
def upfirdn2d_reference(x, k, up, down, pad):
    """zero-stuff by (up_x, up_y), pad or crop by (x0, x1, y0, y1), correlate with the flipped taps, decimate by (down_x, down_y)"""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    N, C, H, W = x.shape
    z = x.new_zeros(N, C, H * uy, W * ux)
    z[:, :, ::uy, ::ux] = x
    z = F.pad(z, (max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)))
    z = z[:, :, max(-py0, 0):z.shape[2] - max(-py1, 0), max(-px0, 0):z.shape[3] - max(-px1, 0)]
    out = F.conv2d(z.reshape(N * C, 1, z.shape[2], z.shape[3]), k.flip(0, 1)[None, None])
    return out.reshape(N, C, out.shape[2], out.shape[3])[:, :, ::dy, ::dx]


UPFIRDN_UP, UPFIRDN_DOWN = (2, 1), (1, 2)
UPFIRDN_PADS = [(2, 1, 0, 3), (1, -1, 1, -1)]


def upfirdn_inputs():
    g = gen(7000)
    return randn(g, 2, 5, 9, 12) + 0.2, randn(g, 4, 2) + 0.1


@pytest.mark.parametrize('pad', UPFIRDN_PADS)
def test_upfirdn2d_anisotropic(pad):
    """up (2, 1), down (1, 2), four different pads (two of them crops), a 4 x 2 kernel on a 9 x 12 map: every x / y argument pair of
    the ABI differs.  1e-6 as test_upfirdn2d: at most 8 fp32 products per output"""
    from conditional_score_diffusion_amd import ops
    x, k = upfirdn_inputs()
    ref = upfirdn2d_reference(x.double(), k.double(), UPFIRDN_UP, UPFIRDN_DOWN, pad)
    out = ops._upfirdn2d_raw(x.to(dev()), k.to(dev()), UPFIRDN_UP, UPFIRDN_DOWN, pad)
    check('upfirdn2d', 'pad %s' % (pad,), rel(out, ref), 1e-6)


# =====================================================================================================================
# 8. optimizer kernels
# =====================================================================================================================
OPT_SIZES = [1, 3, 1023, 262147, 4194309]       # the last: just past 16384 * 256, a second grid-stride sweep with a tail
f32 = lambda v: float(np.float32(v))             # a hyper-parameter as it crosses the C ABI (a float argument)
AdamCfg = collections.namedtuple('AdamCfg', 'clip wd ema step')
# clip: 'active' (max_norm = norm / 4), 'inactive' (4 * norm), 'negative' (max_norm < 0), 'null' (grad_norm = NULL).  The eight rows
# are a pairwise covering of clip x weight_decay x ema x step: every pair of values of two factors occurs in some row
ADAM_CFGS = [AdamCfg('active', 0.01, True, 1), AdamCfg('inactive', 0.0, True, 100000), AdamCfg('negative', 0.01, False, 100000),
             AdamCfg('null', 0.0, False, 1), AdamCfg('active', 0.0, False, 100000), AdamCfg('null', 0.01, True, 100000),
             AdamCfg('inactive', 0.01, False, 1), AdamCfg('negative', 0.0, True, 1)]
ADAM_HYPER = dict(lr=f32(1e-2), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), ema_decay=f32(0.999))
# param, exp_avg, exp_avg_sq and ema are each the end of a chain of at most ~12 fp32 roundings (clip, decay, two moment updates, sqrt,
# two divisions, the update, the EMA), each at most 2^-24 of an intermediate no larger than the tensor's own max: 16 * 2^-24
ADAM_TOL = 16 * 2.0 ** -24
EMA_TOL = 4 * 2.0 ** -24          # ema - (ema - p) * (1 - decay): three roundings
NORM_TOL = 2.0 ** -23             # fp64 accumulation, a sqrt and one rounding to fp32


@functools.lru_cache(maxsize=2)
def opt_state(n):
    rs = np.random.RandomState(8000 + n % 1000)
    r = lambda: rs.standard_normal(n).astype(np.float32)
    return {'param': r() + 0.2, 'grad': r() * 3 + 0.1, 'exp_avg': r() * 0.5, 'exp_avg_sq': np.abs(r()) + 0.01, 'ema': r() + 0.2}


def adam_clip_args(cfg, grad):
    """(grad_norm as the device scalar holds it or None, max_norm)"""
    norm = f32(np.sqrt((grad.astype(np.float64) ** 2).sum()))
    return {'active': (norm, f32(norm / 4)), 'inactive': (norm, f32(norm * 4)), 'negative': (norm, -1.0), 'null': (None, 1.0)}[cfg.clip]


def adam_reference(st, cfg, bias_correction=True):
    """one step of clip_grad_norm_ + torch.optim.Adam + the EMA of models/ema.py in float64"""
    h = ADAM_HYPER
    p, g, m, v = (st[k].astype(np.float64) for k in ('param', 'grad', 'exp_avg', 'exp_avg_sq'))
    norm, max_norm = adam_clip_args(cfg, st['grad'])
    if norm is not None and max_norm >= 0:
        g = g * min(max_norm / (norm + f32(1e-6)), 1.0)
    wd = f32(cfg.wd)
    if wd != 0:
        g = g + wd * p
    m = h['beta1'] * m + (1 - h['beta1']) * g
    v = h['beta2'] * v + (1 - h['beta2']) * g * g
    bc1 = 1 - h['beta1'] ** cfg.step if bias_correction else 1.0
    bc2 = 1 - h['beta2'] ** cfg.step if bias_correction else 1.0
    p = p - (h['lr'] / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + h['eps'])
    out = {'param': p, 'exp_avg': m, 'exp_avg_sq': v}
    if cfg.ema:
        e = st['ema'].astype(np.float64)
        out['ema'] = e - (1 - h['ema_decay']) * (e - p)
    return out


def np_rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize('cfg', ADAM_CFGS, ids=lambda c: '%s_wd%g_%s_step%d' % (c.clip, c.wd, 'ema' if c.ema else 'noema', c.step))
@pytest.mark.parametrize('n', OPT_SIZES)
def test_adam_step(n, cfg):
    """csd_adam_step on the raw ABI against the float64 restatement"""
    from conditional_score_diffusion_amd._lib import check as ok, current_stream, lib, ptr
    st = opt_state(n)
    ref = adam_reference(st, cfg)
    d = dev()
    t = {k: torch.from_numpy(v).to(d) for k, v in st.items()}
    norm, max_norm = adam_clip_args(cfg, st['grad'])
    norm_t = None if norm is None else torch.tensor([norm], dtype=torch.float32, device=d)
    h = ADAM_HYPER
    ok(lib().csd_adam_step(ptr(t['param']), ptr(t['grad']), ptr(t['exp_avg']), ptr(t['exp_avg_sq']), ptr(t['ema']) if cfg.ema else None,
                           ptr(norm_t), n, cfg.step, h['lr'], h['beta1'], h['beta2'], h['eps'], f32(cfg.wd), max_norm, h['ema_decay'],
                           current_stream(d)), 'adam_step')
    for k, r in ref.items():
        check('adam_step', 'n=%d %s %s' % (n, '/'.join(str(v) for v in cfg), k), np_rel(t[k].cpu().numpy(), r), ADAM_TOL)
    assert np.array_equal(t['grad'].cpu().numpy(), st['grad'])
    if not cfg.ema:
        assert np.array_equal(t['ema'].cpu().numpy(), st['ema'])


@pytest.mark.parametrize('n', OPT_SIZES)
def test_global_norm_and_ema_update(n):
    """csd_global_norm (float4 body + scalar tail over 1024 workgroups) and csd_ema_update at the same sizes"""
    from conditional_score_diffusion_amd._lib import check as ok, current_stream, lib, ptr
    st = opt_state(n)
    d = dev()
    a = torch.from_numpy(st['grad']).to(d)
    out = torch.zeros(1, device=d)
    sc = torch.empty(int(lib().csd_global_norm_scratch_bytes()), dtype=torch.uint8, device=d)
    ok(lib().csd_global_norm(ptr(a), ptr(out), n, ptr(sc), current_stream(d)), 'global_norm')
    ref = float(np.sqrt((st['grad'].astype(np.float64) ** 2).sum()))
    check('global_norm', 'n=%d' % n, abs(float(out.cpu()[0]) - ref) / ref, NORM_TOL)
    ema, p = torch.from_numpy(st['ema']).to(d), torch.from_numpy(st['param']).to(d)
    decay = f32(0.999)
    ok(lib().csd_ema_update(ptr(ema), ptr(p), n, decay, current_stream(d)), 'ema_update')
    e64, p64 = st['ema'].astype(np.float64), st['param'].astype(np.float64)
    check('ema_update', 'n=%d' % n, np_rel(ema.cpu().numpy(), e64 - (1 - decay) * (e64 - p64)), EMA_TOL)
    assert np.array_equal(p.cpu().numpy(), st['param'])


# =====================================================================================================================
# 9. dropout
# =====================================================================================================================
DROPOUT_SIZES = [1, 3, 5, 1027, 65541]


def _dropout(x, p, n):
    from conditional_score_diffusion_amd._lib import check as ok, current_stream, lib, ptr
    out, mask = torch.full_like(x[:n], SENTINEL), torch.full_like(x[:n], SENTINEL)
    ok(lib().csd_dropout(ptr(x), ptr(out), ptr(mask), p, 1234, 7, n, current_stream(x.device)), 'dropout')
    return out.cpu(), mask.cpu()


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropout_mask(p):
    """the mask holds 0 and 1 / (1 - p) only, out = x * mask exactly, the keep rate is 1 - p, and the generator is counter-based: a
    call of n = k elements gives the first k mask values of a longer one"""
    x = (randn(gen(9000), DROPOUT_SIZES[-1]) + 0.2)
    xd = x.to(dev())
    p32 = np.float32(p)
    keep = float(np.float32(1) / (np.float32(1) - p32))
    masks = {}
    for n in DROPOUT_SIZES:
        out, mask = _dropout(xd, float(p32), n)
        assert bool(((mask == 0) | (mask == keep)).all()), (n, p, mask.unique())
        assert torch.equal(out, x[:n] * mask)
        masks[n] = mask
    long = masks[DROPOUT_SIZES[-1]]
    for n in DROPOUT_SIZES[:-1]:
        assert torch.equal(masks[n], long[:n])
    n = DROPOUT_SIZES[-1]
    rate = float((long != 0).double().mean())
    assert abs(rate - (1 - p)) < 5 * math.sqrt(p * (1 - p) / n), (rate, p)
