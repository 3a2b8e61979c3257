"""Would tests/test_gpu_train_ops.py notice a subtly wrong kernel?  Answered on the CPU, with its own case lists, inputs, reference
builders and bounds:

1. float32 CPU torch (numpy for the optimizer) passes every family's bound against the float64 reference - the bounds leave room for
   a correct fp32 implementation, and the calibration stays live;
2. references that are wrong in the ways a kernel can be wrong miss the bound by 10x or more: H and W swapped at the ABI on the
   rectangular cases, the rows of the last K-split lost, a data gradient with the weight not flipped, GroupNorm statistics over one
   channel too many or too few, a softmax without its C^-1/2 scale, Adam without bias correction.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_train_ops as T

MARGIN = 10.0
RECT_CONV = [c for c in T.CONV_CASES if c.H != c.W]


def missed(mutant, ref, bound):
    return T.rel(mutant, ref) >= MARGIN * bound


# ---------------------------------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', T.CONV_CASES, ids=T.CONV_IDS)
def test_split_schedule_table(c):
    """the S / per columns of the case list are what the library's schedule gives for the case, and say what the comments claim"""
    OH, OW = T.conv_out_hw(c)
    assert T.wgrad_splits(c.B, OH, OW, c.Cin, c.Cout, c.k) == (c.S, c.per)
    assert (c.S - 1) * c.per < c.B * OH <= c.S * c.per


def test_split_schedule_edges_are_covered():
    by = {c.n: c for c in T.CONV_CASES}
    assert (by[1].S, by[1].per) == (35, 4)
    assert by[2].S == 1
    assert (by[3].S, by[3].per) == (4, 8) and 3 * 10 - 3 * 8 == 6 and by[3].per % 10 != 0          # short last split, straddles samples
    assert (by[4].S, by[4].per) == (4, 12) and 5 * 9 - 3 * 12 == 9


@pytest.mark.parametrize('c', T.CONV_CASES, ids=T.CONV_IDS)
def test_conv_fp32_torch_passes(c):
    ref, f32 = T.conv_reference(c), T.conv_reference_of(T.conv_inputs(c), c, torch.float32)
    for k in ('y', 'dx', 'dw', 'db', 'dw_small'):
        assert T.rel(f32[k], ref[k]) < 1e-5 / 4, k          # (a quarter of the tightest bound of the family)


def _swap_hw(c):
    """the reference of a kernel that takes the map as W x H: same memory in, same memory out"""
    OH, OW = T.conv_out_hw(c)
    inp = T.conv_inputs(c)
    t = c._replace(H=c.W, W=c.H)
    mut = dict(inp, x=inp['x'].reshape(c.B, c.Cin, c.W, c.H))
    for k in ('dy', 'dy_small'):
        mut[k] = inp[k].reshape(c.B, c.Cout, OW, OH)
    out = T.conv_reference_of(mut, t)
    out['y'] = out['y'].reshape(c.B, c.Cout, OH, OW)
    out['dx'] = out['dx'].reshape(c.B, c.Cin, c.H, c.W)
    return out


@pytest.mark.parametrize('c', RECT_CONV, ids=['case%d' % c.n for c in RECT_CONV])
def test_conv_with_h_and_w_swapped_fails(c):
    ref, mut = T.conv_reference(c), _swap_hw(c)
    for precision in ('fp32', 'fp16x3'):
        tol, tol_dw, small = T.conv_bounds(c, precision)
        assert missed(mut['y'], ref['y'], tol) and missed(mut['dx'], ref['dx'], tol)
        if c.k == 3:                                         # (a 1 x 1 weight gradient sums over all pixels: no H / W in it)
            assert missed(mut['dw_small'], ref['dw_small'], tol_dw) and missed(mut['dw'], ref['dw'], tol_dw)


def _dw_without_rows(c, keep_row):
    """dw with the output rows r = b * OH + oy for which keep_row(b, oy) is False dropped from the sum"""
    OH, OW = T.conv_out_hw(c)
    inp = T.conv_inputs(c)
    mask = torch.tensor([[1.0 if keep_row(b, oy) else 0.0 for oy in range(OH)] for b in range(c.B)]).view(c.B, 1, OH, 1)
    mut = dict(inp, dy=inp['dy'] * mask, dy_small=inp['dy_small'] * mask)
    return T.conv_reference_of(mut, c)


@pytest.mark.parametrize('c', T.CONV_CASES, ids=T.CONV_IDS)
def test_conv_without_the_last_k_split_fails(c):
    OH, OW = T.conv_out_hw(c)
    ref = T.conv_reference(c)
    mut = _dw_without_rows(c, lambda b, oy: b * OH + oy < (c.S - 1) * c.per)
    for precision in ('fp32', 'fp16x3'):
        tol_dw = T.conv_bounds(c, precision)[1]
        assert missed(mut['dw'], ref['dw'], tol_dw) and missed(mut['dw_small'], ref['dw_small'], tol_dw)
    if c.stride == 2:
        # the bf16 resampling rebuild splits the rows of the FINE grid (dy row oy sits on fine row 2 * oy + 1 of H rows per sample)
        S2, per2 = T.wgrad_splits(c.B, c.H, c.W, c.Cin, c.Cout, 3)
        mut = _dw_without_rows(c, lambda b, oy: b * c.H + 2 * oy + 1 < (S2 - 1) * per2)
        assert missed(mut['dw'], ref['dw'], T.conv_bounds(c, 'fp16x3')[1])


@pytest.mark.parametrize('c', [c for c in T.CONV_CASES if c.k == 3 and c.stride == 1 and not c.up2],
                         ids=lambda c: 'case%d' % c.n)
def test_conv_data_gradient_without_the_flip_fails(c):
    inp, ref = T.conv_inputs(c), T.conv_reference(c)
    dy, w = inp['dy'].double(), inp['w'].double()
    flipped = F.conv2d(dy, w.flip(2, 3).transpose(0, 1), padding=1)          # what the data-gradient kernels compute
    assert T.rel(flipped, ref['dx']) < 1e-12
    assert missed(F.conv2d(dy, w.transpose(0, 1), padding=1), ref['dx'], 1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------
def _gn_forward_with_stats_over(extra):
    """GroupNorm whose group statistics run over cpg + extra channels"""
    def forward(x, gamma, beta, c):
        C = x.shape[1]
        cpg = C // c.groups
        xh = []
        for g in range(c.groups):
            lo = g * cpg
            s = x[:, lo:min(C, lo + cpg + extra)]
            mean = s.mean(dim=(1, 2, 3), keepdim=True)
            var = s.var(dim=(1, 2, 3), unbiased=False, keepdim=True)
            xh.append((x[:, lo:lo + cpg] - mean) / torch.sqrt(var + T.GN_EPS))
        return T.act_fn(torch.cat(xh, 1) * gamma[None, :, None, None] + beta[None, :, None, None], c.act)
    return forward


@pytest.mark.parametrize('c', T.GN_CASES, ids=T.GN_IDS)
def test_groupnorm_calibration_and_wrong_group_width(c):
    inp, ref = T.gn_inputs(c), T.gn_reference(c)
    bounds = {'y': T.GN_TOL_Y, 'dx': T.GN_TOL_GRAD, 'dgamma': T.GN_TOL_GRAD, 'dbeta': T.GN_TOL_GRAD}
    f32 = T.gn_reference_of(inp, c, torch.float32)
    for k, b in bounds.items():
        assert T.rel(f32[k], ref[k]) < b / 4, k
    same = T.gn_reference_of(inp, c, forward=_gn_forward_with_stats_over(0))
    for k in bounds:
        assert T.rel(same[k], ref[k]) < 1e-11, k
    for extra in ((1, -1) if c.C // c.groups > 1 else (1,)):
        mut = T.gn_reference_of(inp, c, forward=_gn_forward_with_stats_over(extra))
        for k in ('y', 'dx', 'dgamma'):          # (dbeta = sum dy act'(u) does not see the statistics when there is no activation)
            assert missed(mut[k], ref[k], bounds[k]), (extra, k)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
ATTN = T.ATTN_NHWC_CASES + [T.AttnCase(B, H * W, C, False) for (B, C, H, W) in T.ATTN_NCHW_CASES]


@pytest.mark.parametrize('c', ATTN, ids=lambda c: 'B%d_L%d_C%d%s' % (c.B, c.L, c.C, '_peaked' if c.peaked else ''))
def test_attention_calibration_and_missing_scale(c):
    inp, ref = T.attn_inputs(c), T.attn_reference(c)
    bounds = {'out': T.ATTN_TOL_Y, 'dq': T.ATTN_TOL_GRAD, 'dk': T.ATTN_TOL_GRAD, 'dv': T.ATTN_TOL_GRAD}
    f32 = T.attn_reference_of(inp, c, torch.float32)
    mut = T.attn_reference_of(inp, c, scale=False)
    for k, b in bounds.items():
        assert T.rel(f32[k], ref[k]) < b / 4, k
        assert missed(mut[k], ref[k], b), k


# ---------------------------------------------------------------------------------------------------------------------
# bgemm, reductions, resampling helpers, upfirdn2d
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,K', T.BGEMM_SHAPES)
def test_bgemm_fp32_torch_passes(M, N, K):
    g = T.gen(4000 + M + N + K)
    a, b = T.randn(g, 3, M, K) + 0.2, T.randn(g, 3, K, N) + 0.2
    assert T.rel(T.BGEMM_ALPHA * torch.bmm(a, b), T.BGEMM_ALPHA * torch.bmm(a.double(), b.double())) < T.BGEMM_TOL / 4


def test_bgemm_layouts_address_distinct_elements():
    """every layout of the GPU test maps (z, m, n) / (z, m, k) / (z, k, n) to distinct storage elements"""
    for (M, N, K) in T.BGEMM_SHAPES:
        for name, (la, lb, lc) in T.bgemm_layouts(M, N, K).items():
            for idx in (T._index(M, K, *la), T._index(K, N, *lb), T._index(M, N, *lc)):
                assert idx.unique().numel() == idx.numel(), (M, N, K, name)


@pytest.mark.parametrize('shape,axis', [((2016, 6400), 1), ((7, 400), 1), ((2048, 288), 0), ((64, 100), 0), ((7, 1600, 96), 1)])
def test_cancelling_data_separates_fp32_from_fp64_accumulation(shape, axis):
    x = T.cancelling(np.random.RandomState(5), shape, axis)
    exact = x.astype(np.float64).sum(axis=axis).astype(np.float32)          # fp64 accumulation, one rounding
    assert T.fp64_sum_excess(exact, x, axis) <= 1.0
    assert T.fp64_sum_excess(T.fp32_sum(x, axis), x, axis) > MARGIN
    if shape[axis] >= 400:
        # a kernel that adds in float32 one element after the other keeps its partial sums near 1000 and is exact on short runs of
        # this data; from a few hundred elements on the partial sums drift past 1024, where odd multiples of 2^-14 are rounded
        inner = np.ascontiguousarray(np.moveaxis(x, axis, -1))
        sequential = np.cumsum(inner, axis=-1, dtype=np.float32)[..., -1]
        assert T.fp64_sum_excess(sequential, inner, inner.ndim - 1) > MARGIN


@pytest.mark.parametrize('B,h,w,C', [s for s in T.RESAMPLE_SHAPES if s[1] != s[2]])
def test_resampling_helpers_with_h_and_w_swapped_fail(B, h, w, C):
    g = T.gen(6000 + h + w + C)
    small, big = T.randn(g, B, h, w, C) + 0.2, T.randn(g, B, 2 * h, 2 * w, C) + 0.2
    assert not torch.equal(T.zero_insert_reference(small.reshape(B, w, h, C)).reshape(B, 2 * h, 2 * w, C), T.zero_insert_reference(small))
    planes = small.permute(0, 3, 1, 2).contiguous()
    assert not torch.equal(T.nearest_up2_reference(planes.reshape(B, C, w, h)).reshape(B, C, 2 * h, 2 * w), T.nearest_up2_reference(planes))
    terms = T.sumpool2_terms(big.double())
    swapped = T.sumpool2_terms(big.double().reshape(B, 2 * w, 2 * h, C)).sum(0).reshape(B, h, w, C)
    bound = 2 * np.spacing(terms.abs().sum(0).numpy().astype(np.float32)).astype(np.float64)
    assert float(((swapped - terms.sum(0)).abs().numpy() / bound).max()) > MARGIN
    f32 = T.sumpool2_terms(big).sum(0)                                      # float32 torch passes
    assert float(((f32.double() - terms.sum(0)).abs().numpy() / bound).max()) <= 1.0


@pytest.mark.parametrize('pad', T.UPFIRDN_PADS)
def test_upfirdn2d_calibration_and_wrong_axes(pad):
    x, k = T.upfirdn_inputs()
    ref = T.upfirdn2d_reference(x.double(), k.double(), T.UPFIRDN_UP, T.UPFIRDN_DOWN, pad)
    assert T.rel(T.upfirdn2d_reference(x, k, T.UPFIRDN_UP, T.UPFIRDN_DOWN, pad), ref) < 1e-6 / 4
    unflipped = T.upfirdn2d_reference(x.double(), k.double().flip(0, 1), T.UPFIRDN_UP, T.UPFIRDN_DOWN, pad)
    assert missed(unflipped, ref, 1e-6)
    xy = (pad[2], pad[3], pad[0], pad[1])                                   # the x pads applied to y and the y pads to x
    if xy != pad:
        other = T.upfirdn2d_reference(x.double(), k.double(), T.UPFIRDN_UP, T.UPFIRDN_DOWN, xy)
        assert other.shape != ref.shape or missed(other, ref, 1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------------------------------
def _adam_fp32(st, cfg):
    """the same step in float32 numpy arithmetic"""
    h = {k: np.float32(v) for k, v in T.ADAM_HYPER.items()}
    one = np.float32(1)
    p, g, m, v = (st[k].copy() for k in ('param', 'grad', 'exp_avg', 'exp_avg_sq'))
    norm, max_norm = T.adam_clip_args(cfg, st['grad'])
    if norm is not None and max_norm >= 0:
        g = g * np.minimum(np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6)), one)
    if cfg.wd != 0:
        g = g + np.float32(cfg.wd) * p
    m = h['beta1'] * m + (one - h['beta1']) * g
    v = h['beta2'] * v + (one - h['beta2']) * g * g
    bc1 = np.float32(1 - float(h['beta1']) ** cfg.step)
    bc2s = np.float32(np.sqrt(1 - float(h['beta2']) ** cfg.step))
    p = p - (h['lr'] / bc1) * (m / (np.sqrt(v) / bc2s + h['eps']))
    out = {'param': p, 'exp_avg': m, 'exp_avg_sq': v}
    if cfg.ema:
        out['ema'] = st['ema'] - (st['ema'] - p) * (one - h['ema_decay'])
    assert all(a.dtype == np.float32 for a in out.values())
    return out


@pytest.mark.parametrize('cfg', T.ADAM_CFGS, ids=lambda c: '%s_wd%g_%s_step%d' % (c.clip, c.wd, 'ema' if c.ema else 'noema', c.step))
def test_adam_calibration_and_missing_bias_correction(cfg):
    for n in (3, 1023, 262147):
        st = T.opt_state(n)
        ref = T.adam_reference(st, cfg)
        for k, v in _adam_fp32(st, cfg).items():
            assert T.np_rel(v, ref[k]) < T.ADAM_TOL / 4, (n, k)
        if cfg.step == 1:          # (at step 100000 both corrections are 1 to the last bit: nothing to miss)
            mut = T.adam_reference(st, cfg, bias_correction=False)
            assert T.np_rel(mut['param'], ref['param']) >= MARGIN * T.ADAM_TOL
            if cfg.ema:
                assert T.np_rel(mut['ema'], ref['ema']) >= MARGIN * T.ADAM_TOL
        e64, p64 = st['ema'].astype(np.float64), st['param'].astype(np.float64)
        d = np.float32(0.999)
        assert T.np_rel(st['ema'] - (st['ema'] - st['param']) * (np.float32(1) - d), e64 - (1 - float(d)) * (e64 - p64)) < T.EMA_TOL / 4
