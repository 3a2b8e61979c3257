"""-m gpu: results do not depend on what the caller-owned device buffers held, and nothing is written outside them.

include/csd.h promises nothing about the contents of the buffers a caller hands over (packed weights, activation / training
workspace, sampler / likelihood / ODE / per-operator scratch, result tensors); the package hands all of them over uninitialised.  Every
case here runs twice in one process through the allocation seam of tests/guarded.py - first with every such buffer filled with 0x00,
then with 0xFF (a NaN in every fp32 / fp16 / fp64 / e4m3 lane) - and asserts

  (a) the outputs of the two runs are bitwise equal (the library is bitwise repeatable: no tolerance),
  (b) every output element is finite and no byte of the 1 MiB guards around any buffer changed, in either run,
  (c) the baseline output meets the parity assertion of the operator's existing test, at that test's bound (imported or restated
      beside its source), and
  (d) the sizing entries that tests/guarded.py lists for the test really sized a buffer of the run.

The fill is applied where the contract allows it: the packed buffer before csd_unet_pack, the training workspace before the forward
(it survives until the backward), the sampler scratch before step 0, the ODE / likelihood / optimiser scratch before the object's first
use.

Audit (read before the first poisoned run): what the library reads from a caller-owned buffer before writing it would have to be data
only - a poisoned index would be an out-of-range access, not a NaN.
  * per-operator scratch (csd_conv_scratch_bytes, ..._wgrad_..., attention, groupnorm, fir_pyr, conv3x3_block, conv3d_*, sum_pixels,
    global_norm, update, ode, pf_ode): fp16 / fp32 / fp64 operand planes, packed weights and reduction partials, each written by a
    pack / split / partial kernel of the same call before the consumer reads it.  No kernel of csrc/ takes an index, a count or a
    pointer from global memory: every index table (otab / btab / vtab / stab) lives in LDS and is built by the workgroup that uses
    it; loop bounds and strides are kernel arguments computed on the host.
  * packed weights (csd_unet_packed_bytes): float / half / e4m3 data laid out by host-computed offsets (unet_layout.h); padding lanes
    and prefetch slack are zeroed by the pack kernels or a zero-fill launch of the same csd_unet_pack call.
  * activation and training workspace: fp32 / fp16 activations, GroupNorm partials (fp64), dropout masks; arena offsets live in the
    host-side plan, the record of a training forward in a host-side map keyed by the workspace address.
  * sampler scratch (csd_pc_scratch_bytes / csd_pc_inpaint_scratch_bytes): float state, noise, norm partials (fp64) and ONE control
    word, the non-finite flag, which csd_pc_sample / step 0 of csd_pc_step_begin clear with hipMemsetAsync before any kernel reads it.
  * the library has no atomics, tickets or spin-waits on memory.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _flatten(out):
    if isinstance(out, torch.Tensor):
        return {'out': out}
    if isinstance(out, dict):
        return out
    return {'out%d' % i: t for i, t in enumerate(out)}


@pytest.fixture
def fills(request):
    """fills(run, setup=None) -> the baseline outputs {name: CPU tensor}: ``run()`` (a tensor, a tuple or a dict of GPU tensors)
    once per fill, with assertions (a), (b) and (d) of the module docstring; ``setup()`` runs inside the seam before ``run``."""
    entries = guarded.entries_of(request.node.originalname, request.node.name)

    def two_fills(run, setup=None):
        outs = []
        for fill in (0x00, 0xFF):
            with guarded.seam(fill) as rec:
                if setup is not None:
                    setup()
                got = _flatten(run())
                torch.cuda.synchronize()
                got = {k: v.detach().cpu().clone() for k, v in got.items() if v is not None}
            rec.check_guards()
            assert rec.checks, 'no buffer of this run came through the seam'
            for k, v in got.items():
                assert bool(torch.isfinite(v).all()), 'fill 0x%02X: %s holds %d non-finite elements' % (fill, k, int((~torch.isfinite(v)).sum()))
            rec.assert_sized_by(entries)
            outs.append(got)
        assert set(outs[0]) == set(outs[1])
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), '%s depends on the previous contents of a buffer: %d elements differ' % (
                k, int((outs[0][k] != outs[1][k]).sum()))
        return outs[0]

    return two_fills


# =====================================================================================================================
# operators through ops / grad_ops*
# =====================================================================================================================
import test_gpu_ops as T_ops  # noqa: E402

CONV_CASES = [c for c in T_ops.CONV_CASES if c[3] not in (40, 160)]


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3', 'fp16'])
@pytest.mark.parametrize('B,Cin,Cout,H,ks,stride,up2', CONV_CASES)
def test_conv2d(fills, B, Cin, Cout, H, ks, stride, up2, precision):
    """the fp32 kernel, conv16, the quad kernel, pw16, stride 2 and up2; (c): test_gpu_ops.test_conv2d / test_conv2d_fp16_mfma"""
    from conditional_score_diffusion_amd import ops
    x = T_ops.rnd(B, Cin, H, H, seed=1)
    w = T_ops.rnd(Cout, Cin, ks, ks, seed=2, scale=(1.0 / (Cin * ks * ks)) ** 0.5)
    b = T_ops.rnd(Cout, seed=3, scale=0.1)
    f = (lambda t: t) if precision == 'fp32' else (lambda t: t.double())          # (the fp32 test compares with fp32 torch)
    xin = F.interpolate(x, scale_factor=2, mode='nearest') if up2 else x
    if stride == 2:
        ref = F.conv2d(F.pad(f(xin), (0, 1, 0, 1)), f(w), f(b), stride=2)
    else:
        ref = F.conv2d(f(xin), f(w), f(b), padding=ks // 2)
    xd, wd, bd = x.to(dev()), w.to(dev()), b.to(dev())
    out = fills(lambda: ops.conv2d(xd, wd, bd, stride=stride, downsample_pad=(stride == 2), up2=up2, precision=precision))['out']
    if precision == 'fp32':
        assert rel(out, ref) < 2e-6 * max(1, (Cin * ks * ks) ** 0.5 / 8)
    else:
        assert rel(out, ref) < {'fp16x3': 2e-6, 'fp16': 2e-3}[precision] * max(1, (Cin * 9) ** 0.5 / 8)


@pytest.mark.parametrize('precision,tol', [('fp16x3', 1e-5), ('fp16', 3e-3)])
@pytest.mark.parametrize('B,Cin,Cout,H,stride,up2', [(2, 64, 96, 12, 1, False), (3, 128, 128, 16, 1, False), (2, 32, 128, 8, 2, False),
                                                     (2, 96, 256, 8, 1, True), (1, 256, 192, 5, 1, False)])
def test_conv2d_nhwc(fills, B, Cin, Cout, H, stride, up2, precision, tol):
    """csd_conv2d_ex on NHWC tensors: conv_xk without a prologue / the quad schedule with pre-split planes, forward and the data gradient
    through the transposed weight packing; (c): test_gpu_training.test_nhwc_conv_on_the_quad_schedule"""
    from conditional_score_diffusion_amd import grad_ops_nhwc as G
    from test_gpu_training import rnd
    rs = np.random.RandomState(41)
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()          # noqa: E731
    to_nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()          # noqa: E731
    x, w, b = rnd(rs, B, Cin, H, H), rnd(rs, Cout, Cin, 3, 3) * 0.05, rnd(rs, Cout)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    u = F.interpolate(xr, scale_factor=2, mode='nearest') if up2 else xr
    ref = F.conv2d(F.pad(u, (0, 1, 0, 1)), wr, br, stride=2) if stride == 2 else F.conv2d(u, wr, br, padding=1)
    dy = rnd(rs, *ref.shape)
    ref.backward(dy)

    def run():
        xd, wd, bd = to_nhwc(x).to(dev()).requires_grad_(True), w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
        out = G.conv2d(xd, wd, bd, stride=stride, downsample_pad=stride == 2, up2=up2, precision=precision)
        out.backward(to_nhwc(dy).to(dev()))
        return {'y': out, 'dx': xd.grad, 'dw': wd.grad, 'db': bd.grad}

    got = fills(run)
    assert rel(to_nchw(got['y']), ref) < tol
    assert rel(to_nchw(got['dx']), xr.grad) < tol
    assert rel(got['dw'], wr.grad) < max(tol, 5e-5)
    assert rel(got['db'], br.grad) < 1e-5


# (B, H, W, C0, C1, Cout, norm, res): a 16 x 16-tile shape of test_conv3x3_block_fused_prologue and a ragged one of
# test_conv3x3_block_ragged_tiles_fp16x3 (ragged tiles exist in fp16x3 only)
BLOCK_CASES = [((3, 16, 48, 96, 96, 96, True, True), 'fp16x3', 3e-6), ((3, 16, 48, 96, 96, 96, True, True), 'fp16f8', 1e-4),
               ((1, 40, 56, 96, 96, 192, True, False), 'fp16x3', 3e-6)]


@pytest.mark.parametrize('shape,precision,tol', BLOCK_CASES)
def test_conv3x3_block(fills, shape, precision, tol):
    """csd_conv3x3_block with the per-tile statistics requested; (c): the output and statistics bounds of test_gpu_ops.
    test_conv3x3_block_fused_prologue (16 | H, W) and test_conv3x3_block_ragged_tiles_fp16x3"""
    from conditional_score_diffusion_amd import ops
    B, H, W, C0, C1, Cout, norm, res = shape
    rs = np.random.RandomState(40)
    d = dev()
    Cin = C0 + C1
    x = torch.from_numpy(rs.randn(B, H, W, Cin).astype(np.float32) * 2.0 + 0.3)
    w = torch.from_numpy((rs.randn(Cout, Cin, 3, 3) / (3.0 * Cin ** 0.5)).astype(np.float32))
    bias = torch.from_numpy(rs.randn(Cout).astype(np.float32))
    sc = torch.from_numpy((rs.rand(B, Cin) + 0.5).astype(np.float32)) if norm else None
    sh = torch.from_numpy((rs.randn(B, Cin) * 0.5).astype(np.float32)) if norm else None
    rv = torch.from_numpy((rs.randn(B, H, W, Cout) * 3.0).astype(np.float32)) if res else None
    opt = lambda t: None if t is None else t.to(d)      # noqa: E731
    args = (x[..., :C0].contiguous().to(d), w.to(d), bias.to(d))
    kw = dict(x1=x[..., C0:].contiguous().to(d) if C1 else None, nscale=opt(sc), nshift=opt(sh), res=opt(rv), out_scale=0.75,
              precision=precision, want_stats=True)
    got = fills(lambda: dict(zip(('y', 'stats'), ops.conv3x3_block(*args, **kw))))
    xd = x.double()
    if norm:
        xd = F.silu(xd * sc.double()[:, None, None, :] + sh.double()[:, None, None, :])
    ref = F.conv2d(xd.permute(0, 3, 1, 2), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    if rv is not None:
        ref = ref + rv.double()
    ref = ref * 0.75
    yc = got['y'].double()
    assert rel(yc, ref) < tol
    ty, tx = (H + 15) // 16, (W + 15) // 16
    st = got['stats'].reshape(B, ty, tx, Cout, 2)
    worst = 0.0
    for i in range(ty):
        for j in range(tx):
            blk = yc[:, 16 * i:16 * i + 16, 16 * j:16 * j + 16, :]
            worst = max(worst, (st[:, i, j, :, 0] - blk.sum((1, 2))).abs().max().item(),
                        (st[:, i, j, :, 1] - (blk * blk).sum((1, 2))).abs().max().item() * 0.1)
    assert worst < 1e-5 * float((yc * yc).sum((1, 2)).max()), worst


@pytest.mark.parametrize('B,C,H,G,act', [(3, 96, 5, 32, 'none'), (2, 288, 5, 32, 'swish')])
def test_groupnorm_act(fills, B, C, H, G, act):
    """(c): test_gpu_ops.test_groupnorm_act"""
    from conditional_score_diffusion_amd import ops
    x = T_ops.rnd(B, C, H, H, seed=4) * 3 + 0.7
    ga, be = 1 + 0.1 * T_ops.rnd(C, seed=5), 0.1 * T_ops.rnd(C, seed=6)
    ref = F.group_norm(x, G, ga, be, eps=1e-6)
    ref = F.silu(ref) if act == 'swish' else ref
    xd, gd, bd = x.to(dev()), ga.to(dev()), be.to(dev())
    out = fills(lambda: ops.groupnorm_act(xd, gd, bd, groups=G, eps=1e-6, act=act))['out']
    assert rel(out, ref) < 5e-6


@pytest.mark.parametrize('B,C,H,W', [(2, 64, 5, 5), (2, 32, 37, 1), (1, 192, 20, 20)], ids=['L25', 'L37', 'L400'])
def test_attention(fills, B, C, H, W):
    """(c): test_gpu_ops.test_attention (fp64 softmax reference, 1e-5)"""
    from conditional_score_diffusion_amd import ops
    q, k, v = T_ops.rnd(B, C, H, W, seed=7), T_ops.rnd(B, C, H, W, seed=8), T_ops.rnd(B, C, H, W, seed=9)
    s = torch.einsum('bchw,bcij->bhwij', q.double(), k.double()) * (int(C) ** (-0.5))
    s = F.softmax(s.reshape(B, H, W, H * W), dim=-1).reshape(B, H, W, H, W)
    ref = torch.einsum('bhwij,bcij->bchw', s, v.double())
    qd, kd, vd = q.to(dev()), k.to(dev()), v.to(dev())
    out = fills(lambda: ops.attention(qd, kd, vd))['out']
    assert rel(out, ref) < 1e-5


@pytest.mark.parametrize('taps,with_res,scale', [((1, 3, 3, 1), True, 1.0 / np.sqrt(2.0)), (None, False, 1.0)], ids=['fir_residual', 'nofir'])
def test_fir_pyr_conv(fills, taps, with_res, scale):
    """(c): test_gpu_ncsnpp_residual.test_fir_pyr_conv_vs_float64, its first shape"""
    from conditional_score_diffusion_amd import ops
    from test_gpu_ncsnpp_residual import SHAPES, pyr_ref64
    Cin, Cout, S, B = SHAPES[0]
    rs = np.random.RandomState(Cin * 7 + Cout + S + B)
    x = torch.from_numpy(rs.standard_normal((B, Cin, S, S)).astype(np.float32) * 2.0)
    w = torch.from_numpy((rs.uniform(-1, 1, (Cout, Cin, 3, 3)) / np.sqrt(9.0 * Cin)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(Cout).astype(np.float32))
    res = torch.from_numpy(rs.standard_normal((B, Cout, S // 2, S // 2)).astype(np.float32)) if with_res else None
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev())        # noqa: E731
    args = (nhwc(x), w.to(dev()), b.to(dev()), nhwc(res) if res is not None else None)
    out = fills(lambda: ops.fir_pyr_conv(*args, fir_kernel=taps, out_scale=scale))['out']
    ref = pyr_ref64(x, w, b, res, taps, scale).permute(0, 2, 3, 1)
    assert rel(out, ref) < 2e-6 * max(1.0, np.sqrt(9.0 * Cin) / 8.0)


def test_upfirdn2d(fills):
    """(c): test_gpu_ops.test_upfirdn2d, its first case"""
    import score_oracle as so
    from conditional_score_diffusion_amd import ops
    up, down, pad = 2, 1, (2, 1)
    x = T_ops.rnd(2, 5, 12, 12, seed=11)
    k1 = torch.tensor([1., 3., 3., 1.])
    k = torch.outer(k1, k1)
    k = k / k.sum() * (up ** 2)
    xd, kd = x.to(dev()), k.to(dev())
    out = fills(lambda: ops.upfirdn2d(xd, kd, up, down, pad))['out']
    assert rel(out, so.upfirdn2d_ref(x, k, up, down, pad)) < 1e-6


def test_linear(fills):
    """(c): test_gpu_ops.test_linear_ragged_shapes at B = 70, K = 300, N = 37"""
    from conditional_score_diffusion_amd import ops
    B, K, N = 70, 300, 37
    x, w, b = T_ops.rnd(B, K, seed=K + B), T_ops.rnd(N, K, seed=N) * (K ** -0.5), T_ops.rnd(N, seed=3)
    ref = F.silu(x.double()) @ w.double().t() + b.double()
    xd, wd, bd = x.to(dev()), w.to(dev()), b.to(dev())
    out = fills(lambda: ops.linear(xd, wd, bd, act_in='swish'))['out']
    assert rel(out, ref) < 1e-5


def test_langevin_step(fills):
    """(c): test_gpu_ops.test_update_kernels"""
    import score_oracle as so
    from conditional_score_diffusion_amd import ops
    B = 3
    x, net, z = T_ops.rnd(B, 3, 20, 20, seed=1) * 50, T_ops.rnd(B, 3, 20, 20, seed=2), T_ops.rnd(B, 3, 20, 20, seed=3)
    std, snr = 37.5, 0.15
    xr, xmr = so.langevin_update(net / std, x, z, snr)
    nd, zd = net.to(dev()), z.to(dev())
    got = fills(lambda: dict(zip(('x', 'x_mean'), ops.langevin_step(x.to(dev()).clone(), nd, zd, std, snr))))
    assert rel(got['x'], xr) < 1e-6 and rel(got['x_mean'], xmr) < 1e-6


def test_row_norms(fills):
    """(c): test_gpu_steps (torch.allclose against torch.norm, rtol 1e-6)"""
    from conditional_score_diffusion_amd import ops
    n = T_ops.rnd(5, 3, 16, 16, seed=21)
    nd = n.to(dev())
    out = fills(lambda: ops.row_norms(nd))['out']
    assert torch.allclose(out, torch.norm(n.reshape(5, -1), dim=-1), rtol=1e-6)


# ---- the backward operators of tests/test_gpu_train_ops.py: one ragged case each -------------------------------------------
@pytest.mark.parametrize('schedule', ['default', 'ab'])
@pytest.mark.parametrize('layout,precision', [('nchw', 'fp32'), ('nhwc', 'fp32'), ('nhwc', 'fp16x3')])
def test_conv_backward(fills, monkeypatch, layout, precision, schedule):
    """forward, data gradient, csd_conv2d_wgrad (fp32 and split-bf16, the default and the A/B schedule kept behind an environment
    switch) and the bias gradient at the odd, rectangular case 4 of test_gpu_train_ops (channels no multiple of 32, a short last
    K split); (c): test_gpu_train_ops.test_conv_backward"""
    import test_gpu_train_ops as T
    c = T.CONV_CASES[3]
    if schedule == 'ab':
        monkeypatch.setenv('CSD_WGRAD_WIDE' if precision == 'fp32' else 'CSD_WGRAD_GATHER', '1')
    ref = T.conv_reference(c)
    got = fills(lambda: T._run_conv_gpu(c, layout, precision))
    tol, tol_dw, small = T.conv_bounds(c, precision)
    assert rel(got['y'], ref['y']) < tol and rel(got['dx'], ref['dx']) < tol and rel(got['db'], ref['db']) < tol
    if precision == 'fp32':
        assert rel(got['dw'], ref['dw']) < tol_dw and rel(got['dw_small'], ref['dw_small']) < tol_dw
    else:
        assert small and rel(got['dw_small'], ref['dw_small']) < tol_dw


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_groupnorm_act_backward(fills, layout):
    """case 4 of test_gpu_train_ops (4 groups, rectangular 12 x 20); (c): test_gpu_train_ops.test_groupnorm_act_backward"""
    import test_gpu_train_ops as T
    c = T.GN_CASES[3]
    inp, ref = T.gn_inputs(c), T.gn_reference(c)
    d = dev()

    def run():
        gd, bd = inp['gamma'].to(d).requires_grad_(True), inp['beta'].to(d).requires_grad_(True)
        if layout == 'nchw':
            from conditional_score_diffusion_amd import grad_ops as G
            xd = inp['x'].to(d).requires_grad_(True)
            out = G.groupnorm_act(xd, gd, bd, c.groups, T.GN_EPS, c.act)
            out.backward(inp['dy'].to(d))
            return {'y': out, 'dx': xd.grad, 'dgamma': gd.grad, 'dbeta': bd.grad}
        from conditional_score_diffusion_amd import grad_ops_nhwc as G
        xd = T.to_nhwc(inp['x']).to(d).requires_grad_(True)
        out = G.groupnorm_act(xd, gd, bd, c.groups, T.GN_EPS, c.act)
        out.backward(T.to_nhwc(inp['dy']).to(d))
        return {'y': T.to_nchw(out.detach()), 'dx': T.to_nchw(xd.grad), 'dgamma': gd.grad, 'dbeta': bd.grad}

    got = fills(run)
    assert rel(got['y'], ref['y']) < T.GN_TOL_Y
    for k in ('dx', 'dgamma', 'dbeta'):
        assert rel(got[k], ref[k]) < T.GN_TOL_GRAD, k


def test_attention_backward_packed(fills):
    """L = 129 (no multiple of a key tile), C = 96; (c): test_gpu_train_ops.test_attention_backward_packed"""
    import test_gpu_train_ops as T
    from conditional_score_diffusion_amd import grad_ops_nhwc as G
    c = T.ATTN_NHWC_CASES[3]
    inp, ref = T.attn_inputs(c), T.attn_reference(c)

    def run():
        qkv = inp['qkv'].reshape(c.B, c.L, 1, 3 * c.C).to(dev()).requires_grad_(True)
        out = G.attention(qkv)
        out.backward(inp['do'].reshape(c.B, c.L, 1, c.C).to(dev()))
        return {'out': out, 'dqkv': qkv.grad}

    got = fills(run)
    dq, dk, dv = got['dqkv'].reshape(c.B, c.L, 3 * c.C).split(c.C, dim=2)
    assert rel(got['out'].reshape(c.B, c.L, c.C), ref['out']) < T.ATTN_TOL_Y
    for k, g in (('dq', dq), ('dk', dk), ('dv', dv)):
        assert rel(g, ref[k]) < T.ATTN_TOL_GRAD, k


def test_attention_backward_nchw(fills):
    """the rectangular 16 x 8 case; (c): test_gpu_train_ops.test_attention_backward_nchw"""
    import test_gpu_train_ops as T
    from conditional_score_diffusion_amd import grad_ops as G
    B, C, H, W = T.ATTN_NCHW_CASES[0]
    c = T.AttnCase(B, H * W, C, False)
    inp, ref = T.attn_inputs(c), T.attn_reference(c)
    plane = lambda t: t.transpose(1, 2).reshape(B, C, H, W).contiguous()          # noqa: E731
    back = lambda t: t.reshape(B, C, H * W).transpose(1, 2)                        # noqa: E731

    def run():
        q, k, v = (plane(t).to(dev()).requires_grad_(True) for t in inp['qkv'].split(C, dim=2))
        out = G.attention(q, k, v)
        out.backward(plane(inp['do']).to(dev()))
        return {'out': out, 'dq': q.grad, 'dk': k.grad, 'dv': v.grad}

    got = fills(run)
    assert rel(back(got['out']), ref['out']) < T.ATTN_TOL_Y
    for k in ('dq', 'dk', 'dv'):
        assert rel(back(got[k]), ref[k]) < T.ATTN_TOL_GRAD, k


def test_sum_pixels_nhwc(fills):
    """B = 7, HW = 25, C = 96; (c): test_gpu_train_ops.test_sum_pixels_nhwc_accumulates_in_fp64 (the derived fp64-accumulation bound)"""
    import test_gpu_train_ops as T
    from conditional_score_diffusion_amd.grad_ops_nhwc import _sum_pixels
    B, HW, C = 7, 25, 96
    x = T.cancelling(np.random.RandomState(53 + B + C), (B, HW, C), 1)
    xd = torch.from_numpy(x).to(dev()).view(B, HW, 1, C)
    out = fills(lambda: _sum_pixels(xd))['out']
    assert T.fp64_sum_excess(out.numpy(), x, 1) <= 1.0 + 1e-12


def test_global_norm(fills):
    """csd_global_norm through FusedAdam.grad_norm (the optimiser keeps its scratch: it is filled before the object's first use), a size
    with a scalar tail; (c): test_gpu_train_ops.test_global_norm_and_ema_update (2^-23 relative)"""
    import test_gpu_train_ops as T
    from conditional_score_diffusion_amd import optim
    n = 1027
    grad = np.random.RandomState(8000 + n).standard_normal(n).astype(np.float32) * 3 + 0.1
    assert n % 4

    def run():
        opt = optim.FusedAdam([torch.nn.Parameter(torch.zeros(n, device=dev()))])
        assert opt.flat.numel >= n
        opt.flat.grad[:n].copy_(torch.from_numpy(grad))
        return opt.grad_norm()

    out = fills(run)['out']
    ref = float(np.sqrt((grad.astype(np.float64) ** 2).sum()))
    assert abs(float(out[0]) - ref) / ref < T.NORM_TOL


# ---- the 3-D set: the first sweep entries of tests/test_gpu_ddpm3d*.py --------------------------------------------------------
@pytest.mark.parametrize('idx,precision', [(3, 'fp32'), (3, 'fp16x3'), (4, 'fp16x3'), (0, 'fp16x3')],
                         ids=['two_sources_direct', 'two_sources_mfma', 'stem', 'extent1'])
def test_conv3d_block(fills, idx, precision):
    """csd_conv3d_block in its direct (fp32) and MFMA (fp16x3) form on the two-source ragged layer of the sweep, the 1-channel stem and
    the extent-1 volume; (c): test_gpu_ddpm3d.test_conv3d_block_sweep"""
    import test_gpu_ddpm3d as T
    spec = T.SWEEP[idx]
    d = T.conv_case(spec)
    out = fills(lambda: T.conv_gpu(d, spec, precision))['out']
    assert rel(out, T.conv_ref64(d, spec)) < T.conv_bound(spec)


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_conv3d_gradients(fills, precision):
    """csd_conv3d_wgrad, csd_conv3d_dgrad_scale + the data-gradient convolution, the bias gradient at the first sweep entries with more
    than one voxel; (c): test_gpu_ddpm3d_train.test_conv3d_gradients_sweep"""
    import ddpm3d_train_cases as tc
    import test_gpu_ddpm3d_train as T
    for idx in (1, 4):
        B, vol, Cin, Cout = tc.SWEEP[idx]
        rdx, rdw, rdb = tc.op_ref(idx)
        got = fills(lambda: dict(zip(('dx', 'dw', 'db'), T._gpu_conv_grads(tc.op_case(idx), 1.0, precision))))
        assert tc.rel(got['dx'], rdx) < tc.dx_bound(Cout), idx
        assert tc.rel(got['dw'], rdw) < tc.DW_BOUND[precision], idx
        assert tc.rel(got['db'], rdb) < tc.DB_BOUND, idx


def test_groupnorm_scale_shift(fills):
    """(c): test_gpu_ddpm3d.test_groupnorm_scale_shift"""
    from conditional_score_diffusion_amd import ops
    rs = np.random.RandomState(9)
    B, vol, C0, C1 = 3, (3, 5, 2), 64, 32
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))    # noqa: E731
    x0, x1, gamma, beta = 2.0 * t(B, *vol, C0) + 0.5, t(B, *vol, C1), 1.0 + 0.1 * t(C0 + C1), 0.1 * t(C0 + C1)
    args = (x0.to(dev()), gamma.to(dev()), beta.to(dev()))
    x1d = x1.to(dev())
    got = fills(lambda: dict(zip(('ns', 'nh'), ops.groupnorm_scale_shift(*args, x1=x1d))))
    x = torch.cat([x0, x1], dim=-1).double()
    ref = F.group_norm(x.permute(0, 4, 1, 2, 3), 32, gamma.double(), beta.double(), eps=1e-6).permute(0, 2, 3, 4, 1)
    out = x * got['ns'].double()[:, None, None, None, :] + got['nh'].double()[:, None, None, None, :]
    assert rel(out, ref) < 3e-6


def test_pool_and_upsample_3d(fills):
    """(c): test_gpu_ddpm3d.test_pool_and_upsample, its first ragged volume"""
    from conditional_score_diffusion_amd import ops
    B, vol, C = 2, (4, 6, 2), 64
    x = torch.from_numpy(np.random.RandomState(5).standard_normal((B,) + vol + (C,)).astype(np.float32))
    xg = x.to(dev())
    got = fills(lambda: {'up': ops.nearest_up2_3d(xg), 'pool': ops.avg_pool3d_2(xg)})
    assert torch.equal(got['up'], F.interpolate(x.permute(0, 4, 1, 2, 3), scale_factor=2, mode='nearest').permute(0, 2, 3, 4, 1))
    assert rel(got['pool'], F.avg_pool3d(x.double().permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1)) < 1e-6


# =====================================================================================================================
# networks: pack + forward
# =====================================================================================================================
import cases  # noqa: E402
import score_oracle as so  # noqa: E402
import test_gpu_network as T_net  # noqa: E402
from test_gpu_activations import oracle64  # noqa: E402,F401  (fixture: the oracle in float64)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRECISIONS = ['fp32', 'fp16x3', 'fp16f8', 'fp16']
# net1 of the tiny cases against the reference's fixture: test_forward_and_score_vs_golden (fp32) and test_fp16_mfma_modes_vs_golden
TINY_TOL = {'fp32': 1e-4, 'fp16x3': 1e-4, 'fp16f8': 3e-4, 'fp16': 2e-2}


def flat(r):
    return torch.cat([r['x'], r['y']], dim=1) if isinstance(r, dict) else r


def _forward(fills, model, *args):
    """pack + forward through the seam: packed weights, workspace and the result are guarded and filled in both runs"""
    def run():
        with torch.no_grad():
            return flat(model(*args))
    return fills(run, setup=lambda: guarded.reset_model_buffers(model))['out']


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(cases.CASES))
def test_network_forward(fills, case, precision):
    """sr3_tiny, cmde_tiny, uncond_tiny in every arithmetic mode; (c): net1 of tests/golden/<case>.npz at the bounds of
    test_gpu_network.test_forward_and_score_vs_golden / test_fp16_mfma_modes_vs_golden (the same number formats on uncond_tiny)"""
    g = np.load(os.path.join(GOLDEN, case + '.npz'))
    cfg, nc, p, model = T_net.build(case, precision)
    sde = T_net.sdes_for(cfg)
    x = torch.from_numpy(g['x1']).to(dev())
    B = x.shape[0]
    t = torch.ones(B, device=dev()) * 0.5
    if cfg.model.name == 'ddpm':
        args = (x, sde.marginal_prob(x, t)[1])
    else:
        args = ({'x': x, 'y': cases.case_y(case).to(dev())}, t * (cfg.model.num_scales - 1))
    out = _forward(fills, model, *args)
    assert T_net.rel(out.numpy(), g['net1']) < TINY_TOL[precision]


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('fp16x3', 2e-5), ('fp16f8', 2e-4), ('fp16', 5e-3)])
@pytest.mark.parametrize('case', list(cases.NCSNPP_CASES))
def test_ncsnpp_forward(fills, case, precision, tol):
    """the tiny NCSN++ cases, the residual input pyramid among them; (c): test_ncsnpp.test_forward_vs_reference"""
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B, x, labels = cases.ncsnpp_case(case)
    cfg.model.csd_precision = precision
    model = mutils.create_model(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(cases.ncsnpp_params(shapes, 5))
    model = model.to(dev()).eval()
    x, labels = x.to(dev()), labels.to(dev())
    args = ({'x': x[:, :3].contiguous(), 'y': x[:, 3:].contiguous()}, labels) if cfg.model.name == 'ncsnpp_paired' else (x, labels)
    out = _forward(fills, model, *args)
    ref = torch.from_numpy(np.load(os.path.join(GOLDEN, 'ncsnpp.npz'))[case + '_out'])
    assert rel(out, ref) < tol


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('fp16x3', 2e-5), ('fp16f8', 2e-4), ('fp16', 5e-3)])
def test_nf96_network_forward(fills, precision, tol):
    """nf = 96, 32 x 32, B = 3: stem, conv_xk, tap-form head; (c): test_gpu_network.test_nf96_batch_unmasked_tiles"""
    cfg = cases.make_config(name='ddpm_paired_SR3', nf=96, ch_mult=(1, 1), num_res_blocks=1, attn_resolutions=(), image_size=32)
    cfg, nc, p, model = T_net.build(cfg, precision)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.standard_normal((3, 3, 32, 32)).astype(np.float32) * 5)
    y = torch.from_numpy(rs.uniform(0, 1, (3, 3, 32, 32)).astype(np.float32))
    lab = torch.tensor([500., 20., 900.])
    with torch.no_grad():
        ref = so.paired_forward(p, nc, x, y, lab, True)
    out = _forward(fills, model, {'x': x.to(dev()), 'y': y.to(dev())}, lab.to(dev()))
    assert T_net.rel(out.numpy(), ref.numpy()) < tol


@pytest.mark.parametrize('precision,tol', [('fp16x3', 3e-5), ('fp16f8', 3e-4), ('fp16', 5e-3), ('fp32', 3e-5)])
def test_nf128_network_forward(fills, precision, tol):
    """nf = 128, 16 x 16: quad groups of four cout tiles; (c): test_gpu_network.test_nf128_network_vs_oracle"""
    cfg = cases.make_config(name='ddpm_paired', nf=128, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(8,), image_size=16)
    cfg, nc, p, model = T_net.build(cfg, precision)
    rs = np.random.RandomState(77)
    x = torch.from_numpy(rs.uniform(-1, 2, size=(3, 3, 16, 16)).astype(np.float32))
    y = torch.from_numpy(rs.uniform(0, 1, size=(3, 3, 16, 16)).astype(np.float32))
    labels = torch.tensor([3.0, 420.5, 998.0])
    with torch.no_grad():
        ref = flat(so.paired_forward(p, nc, x, y, labels, sr3=False))
    out = _forward(fills, model, {'x': x.to(dev()), 'y': y.to(dev())}, labels.to(dev()))
    assert (out - ref).abs().max().item() <= tol * ref.abs().max().item()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_elu_network_forward(fills, oracle64, precision):  # noqa: F811
    """a non-SiLU network: its head runs on the ordinary 3 x 3 path; (c): test_gpu_activations.test_ddpm_forward_vs_oracle64"""
    import test_gpu_activations as T
    cfg, B, sr3, tols = T.ddpm_shape('sr3_tiny')
    nc, p, model = T.ddpm_model(cfg, 'elu', precision)
    x, y, labels = T.ddpm_inputs(cfg, B)
    out = _forward(fills, model, {'x': x.to(dev()), 'y': y.to(dev())}, labels.to(dev()))
    assert rel(out, T.ddpm_ref64('sr3_tiny', 'elu')) < tols[precision]


def test_network_forward_two_batch_chunks(fills):
    """sr3_tiny at B = 65: two batch chunks on two streams, each with a private workspace block; (c): every sample carries the bits of
    the unchunked plan (test_gpu_network.test_batch_chunk_plan_returns_the_bits_of_the_unchunked_plan)"""
    case, B = 'sr3_tiny', 65
    cfg, nc, p, model = T_net.build(case, precision='fp16x3')
    g = torch.Generator().manual_seed(11)
    x = (torch.randn((B,) + tuple(cfg.data.shape_x), generator=g) * 20).to(dev())
    lab = (torch.rand(B, generator=g) * 900 + 50).to(dev())
    y = cases.case_y(case, B=B).to(dev())
    inp = lambda sl: {'x': x[sl].contiguous(), 'y': y[sl].contiguous()}      # noqa: E731
    full = _forward(fills, model, inp(slice(0, B)), lab)
    guarded.reset_model_buffers(model)
    with torch.no_grad():
        parts = [model(inp(slice(i, min(i + 8, B))), lab[i:i + 8].contiguous()) for i in range(0, B, 8)]
    assert torch.equal(full, torch.cat(parts).cpu())
    assert model.stats(B)[0] > model.stats(8)[0] + 20


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('case', ['B', 'C'])
def test_ddpm3d_forward(fills, case, precision):
    """the 3-D networks run operator by operator: every scratch and result of every layer is guarded;
    (c): test_gpu_ddpm3d.test_network_forward_vs_reference"""
    import ddpm3d_cases as dc
    import test_gpu_ddpm3d as T
    cfg, p, model = T.build(case, precision)
    inputs = T.gpu_inputs(case)
    out = fills(lambda: dc.call(model, case, *inputs))['out']
    assert rel(out, torch.from_numpy(dc.golden()['out_' + case])) < 1e-4


# =====================================================================================================================
# sampling: the scratch is filled before step 0 (it carries state across the steps)
# =====================================================================================================================
def _cond_sampler(cfg, sde, B, P, **kw):
    from conditional_score_diffusion_amd.sampling import conditional
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    return conditional.get_pc_conditional_sampler(sde, (B,) + tuple(cfg.data.shape_x), get_predictor(cfg.sampling.predictor),
                                                  get_corrector(cfg.sampling.corrector), snr=cfg.sampling.snr, p_steps=P,
                                                  c_steps=1, continuous=True, denoise=True, eps=1e-5, **kw)


@pytest.mark.parametrize('kind', ['sr3_tape_record', 'cmde_use_path', 'vp_langevin'])
def test_pc_sampling(fills, kind):
    """csd_pc_sample on the tiny networks, the recording (itself a guarded, filled result) requested on sr3_tiny.  The runs are the
    ones the reference's fixtures hold (there is none of 3 steps): 10 steps of sr3_tiny, 4 steps of the bridge sampler, 6 steps of
    VP reverse diffusion + Langevin; (c): test_gpu_network.test_pc_trajectory_vs_golden, test_use_path_on_the_fused_loop_vs_golden,
    test_gpu_vp_sampling.test_fused_loop_vs_reference_runs"""
    reset = lambda: guarded.reset_model_buffers(model)          # noqa: E731
    if kind == 'sr3_tape_record':
        case, P = 'sr3_tiny', 10
        g = np.load(os.path.join(GOLDEN, case + '.npz'))
        cfg, nc, p, model = T_net.build(case)
        sde = T_net.sdes_for(cfg)
        y = cases.case_y(case).to(dev())
        tape = cases.tape(cases.pc_tape_shapes(case, P))
        fn = _cond_sampler(cfg, sde, y.shape[0], P)

        def run():
            res, info = fn(model, y, show_evolution=True, noise_tape=tape)
            return {'x': res, 'evolution': info['evolution']['x']}

        got = fills(run, setup=reset)
        smax = cfg.model.sigma_max_x
        assert T_net.rel(got['x'].numpy(), g['pc10'], floor=smax) < 2e-4
        assert np.abs(got['evolution'].numpy() - g['pc10_evolution']).max() / smax < 2e-4
    elif kind == 'cmde_use_path':
        g = np.load(os.path.join(GOLDEN, 'use_path.npz'))
        cfg, nc, p, model = T_net.build('cmde_tiny')
        sde = T_net.sdes_for(cfg)
        y = cases.case_y('cmde_tiny').to(dev())
        B, P = y.shape[0], 4
        xs, ys = (B,) + tuple(cfg.data.shape_x), (B,) + tuple(cfg.data.shape_y)
        tp = cases.tape([xs, ys] + [ys, xs, xs] * P, seed=7)
        fn = _cond_sampler(cfg, sde, B, P, use_path=True)
        got = fills(lambda: fn(model, y, noise_tape=tp)[0], setup=reset)
        assert np.abs(got['out'].numpy() - g['out']).max() / float(sde['x'].sigma_max) < 2e-4
    else:
        import test_gpu_vp_sampling as T
        name, case, scls, pred, corr, continuous, pf = T.RUNS[0]
        assert corr == 'langevin' and scls == 'VPSDE'
        cfg, nc, p, model = T_net.build(case)
        xs, sample = T._sampler(cfg, case, T.vp_sde(scls), pred, corr, continuous, pf, 6)
        tape = cases.tape([xs] * (1 + 2 * 6))
        got = fills(lambda: sample(model, noise_tape=tape)[0], setup=reset)
        assert T_net.rel(got['out'].numpy(), np.load(T.GOLD)['run_' + name], floor=1.0) < 2e-4


def test_pc_inpainting(fills):
    """csd_pc_inpaint_sample on uncond_tiny; (c): test_gpu_inpaint_fused.test_device_loop_vs_the_reference_run (fp32)"""
    import test_gpu_inpaint_fused as T
    from conditional_score_diffusion_amd import sde_lib
    g = np.load(os.path.join(GOLDEN, 'inpaint.npz'))
    cfg, B, data, mask, tape = T.inputs()
    _, _, _, model = T_net.build('uncond_tiny')
    sde = sde_lib.VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, 12)
    fn = T.inpainter(sde, 'reverse_diffusion', 'langevin', snr=0.15, eps=1e-5)
    dd, md = data.to(dev()), mask.to(dev())
    x = fills(lambda: fn(model, dd, md, noise_tape=tape)[0], setup=lambda: guarded.reset_model_buffers(model))['out']
    assert float(((x - data) * mask).abs().max()) == 0.0
    assert float(np.abs(x.numpy() - g['x']).max()) <= 2e-4 * float(cfg.model.sigma_max_x)


def test_pc_step_forms(fills):
    """csd_pc_step_begin / csd_pc_step_end on sr3_tiny: the scratch is filled before step 0 only and carries the state from there;
    (c): the shard run of tests/golden/sharded_modes.npz and the one-call form (test_gpu_sharded.
    test_per_shard_and_global_norm_modes_vs_reference)"""
    case, P, B = 'sr3_tiny', 10, 4
    g = np.load(os.path.join(GOLDEN, 'sharded_modes.npz'))
    cfg, nc, p, model = T_net.build(case)
    sde = T_net.sdes_for(cfg)
    smax = float(sde.sigma_max)
    y = cases.case_y(case, B=B).to(dev())[:2].contiguous()
    tape = [t[:2] for t in cases.tape(cases.pc_tape_shapes(case, P, B=B), seed=91)]
    fn = _cond_sampler(cfg, sde, 2, P)
    b = fills(lambda: fn(model, y, noise_tape=tape, global_norm=(lambda s: None, 2))[0],
              setup=lambda: guarded.reset_model_buffers(model))['out']
    guarded.reset_model_buffers(model)
    a = fn(model, y, noise_tape=tape)[0].cpu()
    assert np.abs(a.numpy() - g[case + '_shard0']).max() / smax < 2e-4
    assert np.abs(a.numpy() - b.numpy()).max() / smax < 1e-6


# =====================================================================================================================
# training: the workspace is filled before the forward and must survive until the backward
# =====================================================================================================================
def test_planned_training(fills, oracle64):  # noqa: F811
    """planned forward + backward of sr3_tiny, dropout 0: the loss and every parameter gradient of the training loss, then d loss / d x of
    a weighted sum of the outputs; (c): tests/golden/grads.npz (test_gpu_training.test_training_loss_and_grads_vs_reference) and the
    oracle's float64 input gradient (test_gpu_input_grad: 1e-3)"""
    import test_gpu_input_grad as T_ig
    import test_gpu_training as T
    from test_oracle_golden import check_grads_vs_fixture

    def run():
        loss, grads, model = T._hip_loss_and_grads('sr3_tiny')
        assert model.train_executor == 'planned'
        out = dict(grads)
        out['<loss>'] = torch.tensor([loss], dtype=torch.float64)
        return out

    got = fills(run)
    loss = float(got.pop('<loss>')[0])
    check_grads_vs_fixture(np.load(os.path.join(GOLDEN, 'grads.npz')), 'sr3_tiny', loss, got, 1e-3)

    model, p, ref, x, y, labels = T_ig.build('ddpm', 'sr3_tiny', None, 'fp32')
    model.train()
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((x.shape[0], model.out_channels) + tuple(x.shape[2:])).astype(np.float32))

    def run_dx():
        model.zero_grad(set_to_none=True)
        xg = x.to(dev()).requires_grad_(True)
        out = T_ig.call(model, xg, y.to(dev()), labels.to(dev()))
        (out * w.to(dev())).sum().backward()
        grads = {k: v.grad for k, v in model.named_parameters()}
        grads['<x>'], grads['<out>'] = xg.grad, out
        return grads

    got = fills(run_dx, setup=lambda: guarded.reset_model_buffers(model))
    x64 = x.double().requires_grad_(True)
    r = ref({k: v.double() for k, v in p.items()}, x64, y.double(), labels.double())
    gr, = torch.autograd.grad((r * w.double()).sum(), x64)
    assert T_ig.rel(got['<x>'], gr) <= T_ig.TOL and T_ig.rel(got['<out>'], r) <= T_ig.TOL


def test_eval_input_gradient(fills, oracle64):  # noqa: F811
    """the eval-mode input-gradient path (a private training workspace per forward); (c): test_gpu_input_grad.test_eval_input_grad_vs_oracle"""
    import test_gpu_input_grad as T
    model, p, ref, x, y, labels = T.build('ddpm', 'sr3_tiny', None, 'fp16x3')
    model.eval()
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((x.shape[0], model.out_channels) + tuple(x.shape[2:])).astype(np.float32))

    def run():
        xg = x.to(dev()).requires_grad_(True)
        out = T.call(model, xg, y.to(dev()), labels.to(dev()))
        g, = torch.autograd.grad((out * w.to(dev())).sum(), xg)
        return {'dx': g, 'out': out}

    got = fills(run, setup=lambda: guarded.reset_model_buffers(model))
    x64 = x.double().requires_grad_(True)
    r = ref({k: v.double() for k, v in p.items()}, x64, y.double(), labels.double())
    gr, = torch.autograd.grad((r * w.double()).sum(), x64)
    assert T.rel(got['dx'], gr) <= T.TOL and T.rel(got['out'], r) <= T.TOL


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('fp16x3', 2e-4)])
def test_ddpm3d_training(fills, precision, tol):
    """ddpm3D case B in training mode, dropout 0: every parameter gradient and the input gradient;
    (c): test_gpu_ddpm3d_train.test_network_gradients_vs_float64"""
    import ddpm3d_cases as dc
    import ddpm3d_train_cases as tc
    import test_gpu_ddpm3d_train as T
    case = 'B'
    cfg, model = T.build(case, precision)
    x, y, labels = T.gpu_inputs(case)
    val, rg, rdx = tc.net_ref(case)
    model.train()
    gw = tc.net_g(case).to(dev())

    def run():
        model.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        out = dc.call(model, case, xg, y, labels)
        (out * gw).sum().backward()
        got = {k: v.grad for k, v in model.named_parameters()}
        got['<x>'] = xg.grad
        return got

    got = fills(run)
    ref = dict(rg)
    ref['<x>'] = rdx
    assert set(got) == set(ref)
    worst, where = tc.grad_check(got, ref, tol, 1e-7)
    assert worst <= 1.0, where


# =====================================================================================================================
# likelihood and the device-resident RK45: the scratch is filled before the object's first use
# =====================================================================================================================
def test_likelihood(fills):
    """the fused probability-flow right-hand side (training workspace + csd_pf_ode scratch, both held for the whole solve);
    (c): the generic autograd path, test_gpu_likelihood.test_fused_likelihood_matches_generic_and_oracle"""
    import test_gpu_likelihood as T
    from conditional_score_diffusion_amd import likelihood, sde_lib
    cfg, model, oracle, x, e = T._uncond()
    sde = sde_lib.VESDE(0.01, 5.0, 1000)
    fn = likelihood.get_likelihood_fn(sde, lambda v: v, **T.TOL)
    xd, ed = x.to(dev()), e.to(dev())
    nfe = []

    def run():
        bpd, z, n = fn(model, xd, epsilon=ed)
        nfe.append(n)
        return {'bpd': bpd, 'z': z}

    got = fills(run, setup=lambda: guarded.reset_model_buffers(model))
    assert nfe[0] == nfe[1]
    T._agree((got['bpd'], got['z'], nfe[0]), fn(T.Generic(model), xd, epsilon=ed))


def test_device_rk45(fills):
    """ode_solver.DeviceBackend (csd_ode_combine / csd_ode_error_sumsq / csd_ode_scaled_sumsq with their reduction scratch) on the
    analytic problem; (c): test_gpu_ode_rk45.test_device_solver_matches_scipy"""
    import test_gpu_ode_rk45 as T
    from conditional_score_diffusion_amd import ode_solver as osv
    from test_ode_solver_host import scipy_reference
    n, t0, t1, tol = 1001, 1.0, 1e-3, 1e-6
    want_y, want_nfev, want_steps = scipy_reference(n, t0, t1, tol)
    rs = np.random.RandomState(3)
    lam, w, y0 = T._T(rs.uniform(0.1, 3.0, size=n)), T._T(rs.uniform(0.0, 20.0, size=n)), T._T(3.0 * rs.standard_normal(n))
    d = math.copysign(1.0, t1 - t0)
    counts = []

    def rhs(t, y, x32, k_out):
        k_out.copy_(d * (-lam * y + 5.0 * torch.sin(w * t) + 0.3 * torch.roll(y, 1) ** 2 / (1.0 + y * y)))

    def run():
        res = osv.solve(rhs, osv.DeviceBackend(y0), t0, t1, tol, tol)
        counts.append((res.nfev, res.n_accepted))
        return res.y

    y = fills(run)['out']
    assert counts[0] == counts[1] == (want_nfev, want_steps)
    assert np.abs(y.numpy() - want_y).max() / np.abs(want_y).max() <= 1e-12
