"""The differentiable layer operators of the 3-D DDPM networks on channels-last volumes ([B, D, H, W, C] fp32, contiguous).

``torch.autograd.Function`` shells in the style of grad_ops_nhwc: autograd records the graph, every gradient is a HIP kernel behind the
C ABI (include/csd.h):

=====================  ==============================================================================================================
conv3d (3x3x3)         forward csd_conv3d_block without prologue;
                       dX = csd_conv3d_block(dY * 2^k; flip(W)^T) / 2^k with the per-sample power of two of csd_conv3d_dgrad_scale
                       (the forward kernel's fp16 hi | lo operands made scale invariant; the multiply and csd_scale_rows are exact);
                       dW = csd_conv3d_wgrad (split bf16 / fp32);  db = csd_sum_pixels_nhwc + csd_sum_rows
groupnorm_act          csd_groupnorm_act_nhwc / csd_groupnorm_act_backward_nhwc with S = D*H*W
avg_pool3d_2           backward = csd_nearest_up2_3d_ndhwc / 8
nearest_up2_3d         backward = csd_avgpool3d_2_ndhwc * 8
bias_add               csd_bias_add_nhwc;  dbias[b, c] = csd_sum_pixels_nhwc
linear, axpby, dropout grad_ops (layout free)
=====================  ==============================================================================================================

torch moves data only (the flipped / transposed weight of the data gradient is a copy).  There is no CPU fallback: every function
requires float32 GPU tensors.
"""
import torch

from . import _lib, grad_ops_nhwc, ops
from ._lib import check, current_stream, lib, ptr, require_gpu_tensor
from .grad_ops import _sum_inner, _sum_rows, axpby, dropout, linear  # noqa: F401  (layout-free operators are shared)

_PRECISIONS = ('fp32', 'f32', 'fp16x3')


def conv3d_wgrad(a, dy, precision='fp16x3'):
    """dw [Cout, Cin, 3, 3, 3] = sum over b, voxels of dy[b, v, co] * a[b, v + tap, ci] (csd_conv3d_wgrad); a [B,D,H,W,Cin], dy [B,D,H,W,Cout]."""
    require_gpu_tensor(a, 'a')
    require_gpu_tensor(dy, 'dy')
    a, dy = a.contiguous(), dy.contiguous()
    if a.dim() != 5 or dy.dim() != 5 or tuple(a.shape[:4]) != tuple(dy.shape[:4]):
        raise RuntimeError('conv3d_wgrad: a %s and dy %s are not [B, D, H, W, C] of one volume' % (tuple(a.shape), tuple(dy.shape)))
    if precision not in _PRECISIONS:
        raise ValueError("conv3d_wgrad: precision %r is not 'fp32' or 'fp16x3'" % (precision,))
    B, D, H, W, Cin = a.shape
    Cout = dy.shape[4]
    prec = _lib.PREC_IDS[precision]
    dw = ops._out((Cout, Cin, 3, 3, 3), torch.float32, a.device)
    sc = ops._scratch(lib().csd_conv3d_wgrad_scratch_bytes(B, Cin, Cout, D, H, W, prec), a.device)
    check(lib().csd_conv3d_wgrad(ptr(a), ptr(dy), ptr(dw), B, Cin, Cout, D, H, W, prec, ptr(sc), current_stream(a.device)), 'conv3d_wgrad')
    return dw


def conv3d_dgrad(dy, weight, precision='fp16x3'):
    """dx [B,D,H,W,Cin] of y = conv3d(x, weight [Cout,Cin,3,3,3]) given dy [B,D,H,W,Cout]: the convolution of dy with the flipped,
    transposed weight, scale invariant (see the module docstring)."""
    require_gpu_tensor(dy, 'dy')
    dy = dy.contiguous()
    B, D, H, W, Cout = dy.shape
    wt = weight.flip(2, 3, 4).transpose(0, 1).contiguous()               # [Cin, Cout, 3, 3, 3]: data movement only
    dev = dy.device
    rowscale = ops._out(B, torch.float32, dev)
    nscale = ops._out((B, Cout), torch.float32, dev)
    nshift = ops._out((B, Cout), torch.float32, dev)
    sc = ops._scratch(lib().csd_conv3d_dgrad_scale_scratch_bytes(B), dev)
    check(lib().csd_conv3d_dgrad_scale(ptr(dy), ptr(rowscale), ptr(nscale), ptr(nshift), B, dy.numel() // B, Cout, ptr(sc),
                                       current_stream(dev)), 'conv3d_dgrad_scale')
    dx = ops.conv3d_block(dy, wt, None, nscale=nscale, nshift=nshift, act='none', precision=precision)
    check(lib().csd_scale_rows(ptr(dx), ptr(dx), ptr(rowscale), 1, B, dx.numel() // B, current_stream(dev)), 'scale_rows')
    return dx


def _sum_voxels(x):
    """[B, D, H, W, C] -> [B, C]"""
    B, C = x.shape[0], x.shape[-1]
    S = x.numel() // (B * C)
    if C % 4 or C > 1024:
        return _sum_inner(x.reshape(B, S, C).transpose(1, 2).contiguous(), B * C).view(B, C)
    return grad_ops_nhwc._sum_pixels(x.view(B, 1, S, C))


class _Conv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, precision):
        ctx.save_for_backward(x, weight)
        ctx.cfg = (precision, bias is not None)
        return ops.conv3d_block(x, weight, bias, precision=precision)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        precision, has_bias = ctx.cfg
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = conv3d_dgrad(dy, weight, precision)
        if ctx.needs_input_grad[1]:
            dw = conv3d_wgrad(x, dy, precision)
        if has_bias and ctx.needs_input_grad[2]:
            db = _sum_rows(_sum_voxels(dy))
        return dx, dw, db, None


def conv3d(x, weight, bias=None, precision='fp16x3'):
    """3x3x3 convolution, stride 1, zero padding 1: x [B,D,H,W,Cin], weight [Cout,Cin,3,3,3] -> [B,D,H,W,Cout]."""
    if precision not in _PRECISIONS:
        raise ValueError("conv3d: precision %r is not 'fp32' or 'fp16x3'" % (precision,))
    require_gpu_tensor(x, 'x')
    require_gpu_tensor(weight, 'weight')
    return _Conv3d.apply(x.contiguous(), weight.contiguous(), None if bias is None else bias.contiguous(), precision)


def groupnorm_act(x, gamma, beta, groups=32, eps=1e-6, act='none'):
    """act(GroupNorm(x)) on [B, D, H, W, C]: the NHWC operator on [B, 1, S, C], S = D*H*W."""
    require_gpu_tensor(x, 'x')
    shp = x.shape
    x = x.contiguous()
    y = grad_ops_nhwc.groupnorm_act(x.view(shp[0], 1, -1, shp[-1]), gamma, beta, groups, eps, act)
    return y.view(shp)


class _AvgPool3d2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.avg_pool3d_2(x)

    @staticmethod
    def backward(ctx, dy):
        return ops.axpby(ops.nearest_up2_3d(dy.contiguous()), None, alpha=0.125)


def avg_pool3d_2(x):
    require_gpu_tensor(x, 'x')
    return _AvgPool3d2.apply(x.contiguous())


class _NearestUp2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.nearest_up2_3d(x)

    @staticmethod
    def backward(ctx, dy):
        return ops.axpby(ops.avg_pool3d_2(dy.contiguous()), None, alpha=8.0)


def nearest_up2_3d(x):
    require_gpu_tensor(x, 'x')
    return _NearestUp2.apply(x.contiguous())


def bias_add(x, bias):
    """x [B, D, H, W, C] + bias[b, c] (the time-embedding add of the residual blocks)"""
    require_gpu_tensor(x, 'x')
    shp = x.shape
    x = x.contiguous()
    return grad_ops_nhwc.bias_add(x.view(shp[0], 1, -1, shp[-1]), bias).view(shp)
