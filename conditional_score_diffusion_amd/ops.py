"""Thin tensor-level wrappers over the per-operator C ABI (include/csd.h).

Tensors are containers only: every function checks that its operands are contiguous fp32 GPU
tensors, allocates the output / scratch with torch, and enqueues the HIP kernels on the current
stream.  No torch arithmetic happens here.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, current_stream, lib, ptr, require_gpu_tensor


def _scratch(nbytes, device):
    """A caller-owned byte buffer (scratch, workspace, packed weights) of exactly the size a ``csd_*_bytes`` entry declared.  A declared
    size of 0 (the operator is expected to refuse the call) still gets an address.  Every such buffer of the package comes from here."""
    return torch.empty(int(nbytes) or 256, dtype=torch.uint8, device=device)


def _out(shape, dtype, device):
    """A result tensor that the library writes in full (never reads).  Every output of the package comes from here."""
    return torch.empty(shape, dtype=dtype, device=device)


def _c(t, name):
    require_gpu_tensor(t, name)
    return t.contiguous()


def groupnorm_act(x, gamma, beta, groups=32, eps=1e-6, act='none'):
    """act(GroupNorm(x)) - nn.GroupNorm + get_act (models/layers.py:571,638,646)."""
    x, gamma, beta = _c(x, 'x'), _c(gamma, 'gamma'), _c(beta, 'beta')
    B, C, H, W = x.shape
    y = _out(x.shape, x.dtype, x.device)
    sc = _scratch(lib().csd_groupnorm_scratch_bytes(B, C, H, W), x.device)
    check(lib().csd_groupnorm_act(ptr(x), ptr(gamma), ptr(beta), ptr(y), B, C, H, W, groups, eps,
                                  _lib.ACT_IDS[act], ptr(sc), current_stream(x.device)), 'groupnorm_act')
    return y


def conv2d(x, weight, bias=None, stride=1, downsample_pad=False, up2=False, precision='fp32'):
    """3x3 / 1x1 convolution, weight OIHW (models/layers.py:100-132); ``stride=2,
    downsample_pad=True`` is the reference Downsample (pad (0,1,0,1), models/layers.py:619-625);
    ``up2`` applies nearest x2 first (models/layers.py:600-604)."""
    x, weight = _c(x, 'x'), _c(weight, 'weight')
    if bias is not None:
        bias = _c(bias, 'bias')
    B, Cin, H, W = x.shape
    Cout, Cin_w, kh, kw = weight.shape
    if Cin_w != Cin or kh != kw:
        raise RuntimeError('conv2d: weight %s does not match input channels %d' % (tuple(weight.shape), Cin))
    OH = (H * (2 if up2 else 1)) // stride
    OW = (W * (2 if up2 else 1)) // stride
    y = _out((B, Cout, OH, OW), torch.float32, x.device)
    sc = _scratch(lib().csd_conv_scratch_bytes(B, Cin, Cout, H, W, kh, int(up2)), x.device)
    check(lib().csd_conv2d(ptr(x), ptr(weight), ptr(bias), ptr(y), B, Cin, Cout, H, W, kh, stride,
                           1 if downsample_pad else 0, int(up2), _lib.PREC_IDS[precision], ptr(sc),
                           current_stream(x.device)), 'conv2d')
    return y


def fir_pyr_conv(x, weight, bias=None, res=None, fir_kernel=(1, 3, 3, 1), out_scale=1.0):
    """The 'residual' input pyramid of NCSN++ (layerspp.Downsample(with_conv=True), layerspp.py:129-163) on NHWC fp32 tensors:
    ``(Downsample(x) + res) * out_scale``.  x [B, H, H, P] with P >= Cin floats per pixel (the first Cin are read: the padded assembled
    input of a network is such a tensor), weight [Cout, Cin, 3, 3] OIHW, res [B, H/2, H/2, Cout] or None.
    ``fir_kernel`` (4 taps): conv_downsample_2d (FIR with pads (2, 2), then a VALID stride-2 conv); None: fir = False
    (F.pad(0, 1, 0, 1) + stride-2 conv).  csd_fir_pyr_conv.  Returns [B, H/2, H/2, Cout]."""
    import ctypes
    x, weight = _c(x, 'x'), _c(weight, 'weight')
    B, H, W, pix = x.shape
    Cout, Cin = weight.shape[0], weight.shape[1]
    if H != W or H % 2 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or Cin > pix:
        raise RuntimeError('fir_pyr_conv: x %s / weight %s do not match' % (tuple(x.shape), tuple(weight.shape)))
    if bias is not None:
        bias = _c(bias, 'bias')
        if tuple(bias.shape) != (Cout,):
            raise RuntimeError('fir_pyr_conv: bias %s is not [Cout] = [%d]' % (tuple(bias.shape), Cout))
    if res is not None:
        res = _c(res, 'res')
        if tuple(res.shape) != (B, H // 2, H // 2, Cout):
            raise RuntimeError('fir_pyr_conv: res %s is not [B, H/2, H/2, Cout]' % (tuple(res.shape),))
    if any(t is not None and t.device != x.device for t in (weight, bias, res)):
        raise RuntimeError('fir_pyr_conv: x, weight, bias and res must be on one device')
    taps = None
    if fir_kernel is not None:
        if len(fir_kernel) != 4:
            raise NotImplementedError('fir_pyr_conv: 4-tap FIR kernels only')
        taps = (ctypes.c_float * 4)(*[float(v) for v in fir_kernel])
    y = _out((B, H // 2, H // 2, Cout), torch.float32, x.device)
    sc = _scratch(lib().csd_fir_pyr_conv_scratch_bytes(Cin, Cout), x.device)
    check(lib().csd_fir_pyr_conv(ptr(x), ptr(weight), ptr(bias), ptr(res), ptr(y), B, Cin, Cout, H, pix,
                                 ctypes.cast(taps, ctypes.c_void_p) if taps is not None else None, float(out_scale), ptr(sc),
                                 current_stream(x.device)), 'fir_pyr_conv')
    return y


def fir_resample_nhwc(x, fir_kernel=(1, 3, 3, 1), up=False):
    """FIR resampling by 2 of an NHWC fp32 tensor [B, H, W, C] with a separable 4-tap kernel: upsample_2d / downsample_2d of
    models/up_or_down_sampling.py:196-257 as the NCSN++ plans run them (csd_fir_resample_nhwc).  Returns [B, 2H, 2W, C] or
    [B, H/2, W/2, C]."""
    import ctypes
    x = _c(x, 'x')
    B, H, W, C = x.shape
    if len(fir_kernel) != 4:
        raise NotImplementedError('fir_resample_nhwc: 4-tap FIR kernels only')
    taps = (ctypes.c_float * 4)(*[float(v) for v in fir_kernel])
    y = _out((B, 2 * H, 2 * W, C) if up else (B, H // 2, W // 2, C), torch.float32, x.device)
    check(lib().csd_fir_resample_nhwc(ptr(x), ptr(y), B, H, W, C, ctypes.cast(taps, ctypes.c_void_p), int(bool(up)),
                                      current_stream(x.device)), 'fir_resample_nhwc')
    return y


def input_conv(x, y, weight, bias, y_noise=None, y_sigma=0.0, centered=False, precision='fp16x3', fused=True, want_stats=False, y_scale=0):
    """The DDPM family's first layer (models/ddpm.py:163-168, :283 and the first conv3x3): conv3x3(2 cat(x, y + y_sigma y_noise) - 1) on
    NCHW fp32 x [B, Cx, S, S], y [B, Cy, S, S] or None; weight [Cout, Cx + Cy, 3, 3], bias [Cout]; up to 32 input channels.
    ``fused``: the one-launch layer of csrc/stem.hip; otherwise the assembled, padded input and the generic convolution (what a
    network's plan runs where the fused layer does not apply).  csd_input_conv.  Returns out [B, S, S, Cout] NHWC (and, fused with
    ``want_stats``, the (sum, sum of squares) of every 16 x 8 tile of it).  ``y_scale = K >= 2``: y (and y_noise) are
    [B, Cy, S / K, S / K] and the layer sees the bilinear upsample of y + y_sigma y_noise - the first layer of the Kx super-resolution
    networks (csd_input_conv_kx; up to 8 channels)."""
    x, weight, bias = _c(x, 'x'), _c(weight, 'weight'), _c(bias, 'bias')
    B, Cx, S, S2 = x.shape
    Cy = 0
    K = int(y_scale)
    if K and (K < 2 or S % K or y is None):
        raise RuntimeError('input_conv: y_scale = %d needs y and a scale >= 2 that divides S = %d' % (K, S))
    sy = S // K if K else S
    if y is not None:
        y = _c(y, 'y')
        Cy = y.shape[1]
        if tuple(y.shape) != (B, Cy, sy, sy):
            raise RuntimeError('input_conv: y %s does not match x %s' % (tuple(y.shape), tuple(x.shape)))
    Cout = weight.shape[0]
    if S != S2 or tuple(weight.shape) != (Cout, Cx + Cy, 3, 3) or tuple(bias.shape) != (Cout,):
        raise RuntimeError('input_conv: x %s / weight %s / bias %s do not match' % (tuple(x.shape), tuple(weight.shape), tuple(bias.shape)))
    if y_noise is not None:
        y_noise = _c(y_noise, 'y_noise')
        if y is None or tuple(y_noise.shape) != tuple(y.shape):
            raise RuntimeError('input_conv: y_noise must have the shape of y')
    out = _out((B, S, S, Cout), torch.float32, x.device)
    stats = _out((B * (S // 16) * (S // 8), Cout, 2), torch.float64, x.device) if want_stats else None
    if Cx + Cy > 32:
        raise RuntimeError('input_conv: at most 32 input channels (got %d + %d)' % (Cx, Cy))
    sc = _scratch(lib().csd_conv_scratch_bytes(B, 32, Cout, S, S, 3, 0), x.device)      # (the 32-channel convolution's: include/csd.h)
    if K:
        check(lib().csd_input_conv_kx(ptr(x), ptr(y), ptr(y_noise), float(y_sigma), ptr(weight), ptr(bias), ptr(out), ptr(stats), B, Cx,
                                      Cy, Cout, S, K, int(bool(centered)), _lib.PREC_IDS[precision], int(bool(fused)), ptr(sc),
                                      current_stream(x.device)), 'input_conv_kx')
        return (out, stats) if want_stats else out
    check(lib().csd_input_conv(ptr(x), ptr(y), ptr(y_noise), float(y_sigma), ptr(weight), ptr(bias), ptr(out), ptr(stats), B, Cx, Cy,
                               Cout, S, int(bool(centered)), _lib.PREC_IDS[precision], int(bool(fused)), ptr(sc),
                               current_stream(x.device)), 'input_conv')
    return (out, stats) if want_stats else out


def conv3x3_block(x0, weight, bias=None, x1=None, nscale=None, nshift=None, temb=None, res=None, out_scale=1.0,
                  precision='fp16x3', want_stats=False):
    """The ResnetBlock convolution with its prologue fused (models/layers.py:632-675): y = Conv3x3(SiLU(x*nscale + nshift))
    (+ bias + temb[:, None, None, :] + res) * out_scale on NHWC fp32 tensors; x = x0 (| x1: virtual concat).  csd_conv3x3_block.
    Returns y [B,H,W,Cout] (and the per-tile (sum, sum of squares) partials of y when ``want_stats``)."""
    x0, weight = _c(x0, 'x0'), _c(weight, 'weight')
    B, H, W, C0 = x0.shape
    C1 = 0
    if x1 is not None:
        x1 = _c(x1, 'x1')
        C1 = x1.shape[3]
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, C0 + C1, 3, 3):
        raise RuntimeError('conv3x3_block: weight %s does not match %d input channels' % (tuple(weight.shape), C0 + C1))
    opt = [None if t is None else _c(t, 't') for t in (bias, nscale, nshift, temb, res)]
    bias, nscale, nshift, temb, res = opt
    y = _out((B, H, W, Cout), torch.float32, x0.device)
    stats = _out((B * ((H + 15) // 16) * ((W + 15) // 16), Cout, 2), torch.float64, x0.device) if want_stats else None
    sc = _scratch(lib().csd_conv3x3_block_scratch_bytes(C0 + C1, Cout), x0.device)
    check(lib().csd_conv3x3_block(ptr(x0), ptr(x1), ptr(weight), ptr(bias), ptr(nscale), ptr(nshift), ptr(temb),
                                  temb.shape[1] if temb is not None else 0, ptr(res), float(out_scale), ptr(y), ptr(stats),
                                  B, C0, C1, Cout, H, W, _lib.PREC_IDS[precision], ptr(sc), current_stream(x0.device)),
          'conv3x3_block')
    return (y, stats) if want_stats else y


def conv3d_block(x0, weight, bias=None, x1=None, nscale=None, nshift=None, act='swish', temb=None, res=None, out_scale=1.0,
                 precision='fp16x3'):
    """The 3-D ResnetBlock convolution with its prologue fused (models/layers.py:632-675 with dim = 3): y = (Conv3x3x3(act(x*nscale +
    nshift)) + bias + temb[:, None, None, None, :] + res) * out_scale on channels-last fp32 tensors [B,D,H,W,C]; x = x0 (| x1: virtual
    concat); weight [Cout, C0+C1, 3, 3, 3].  nscale = nshift = None: the convolution reads x as it is.  csd_conv3d_block."""
    x0, weight = _c(x0, 'x0'), _c(weight, 'weight')
    if x0.dim() != 5:
        raise RuntimeError('conv3d_block: x0 %s is not [B, D, H, W, C]' % (tuple(x0.shape),))
    B, D, H, W, C0 = x0.shape
    C1 = 0
    if x1 is not None:
        x1 = _c(x1, 'x1')
        if tuple(x1.shape[:4]) != (B, D, H, W):
            raise RuntimeError('conv3d_block: x1 %s does not match x0 %s' % (tuple(x1.shape), tuple(x0.shape)))
        C1 = x1.shape[4]
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, C0 + C1, 3, 3, 3):
        raise RuntimeError('conv3d_block: weight %s does not match %d input channels' % (tuple(weight.shape), C0 + C1))
    if precision not in _lib.PREC_IDS or act not in _lib.ACT_IDS:
        raise ValueError('conv3d_block: unknown precision %r or activation %r' % (precision, act))
    bias, nscale, nshift, temb, res = [None if t is None else _c(t, 't') for t in (bias, nscale, nshift, temb, res)]
    for t, shp, name in ((bias, (Cout,), 'bias'), (nscale, (B, C0 + C1), 'nscale'), (nshift, (B, C0 + C1), 'nshift'),
                         (res, (B, D, H, W, Cout), 'res')):
        if t is not None and tuple(t.shape) != shp:
            raise RuntimeError('conv3d_block: %s %s is not %s' % (name, tuple(t.shape), shp))
    if temb is not None and (temb.dim() != 2 or temb.shape[0] != B):
        raise RuntimeError('conv3d_block: temb %s is not [B, >= Cout]' % (tuple(temb.shape),))
    if any(t is not None and t.device != x0.device for t in (weight, x1, bias, nscale, nshift, temb, res)):
        raise RuntimeError('conv3d_block: every operand must be on one device')
    y = _out((B, D, H, W, Cout), torch.float32, x0.device)
    sc = _scratch(lib().csd_conv3d_block_scratch_bytes(C0 + C1, Cout), x0.device)
    check(lib().csd_conv3d_block(ptr(x0), ptr(x1), ptr(weight), ptr(bias), ptr(nscale), ptr(nshift), _lib.ACT_IDS[act], ptr(temb),
                                 temb.shape[1] if temb is not None else 0, ptr(res), float(out_scale), ptr(y), B, C0, C1, Cout, D, H, W,
                                 _lib.PREC_IDS[precision], ptr(sc), current_stream(x0.device)), 'conv3d_block')
    return y


def avg_pool3d_2(x):
    """nn.AvgPool3d(2, 2) (models/layers.py:617) on a channels-last volume [B,D,H,W,C] -> [B,D/2,H/2,W/2,C]."""
    x = _c(x, 'x')
    B, D, H, W, C = x.shape
    y = _out((B, D // 2, H // 2, W // 2, C), torch.float32, x.device)
    check(lib().csd_avgpool3d_2_ndhwc(ptr(x), ptr(y), B, D, H, W, C, current_stream(x.device)), 'avg_pool3d_2')
    return y


def nearest_up2_3d(x):
    """F.interpolate(x, 2 * size, mode='nearest') (models/layers.py:601) on a channels-last volume [B,D,H,W,C]."""
    x = _c(x, 'x')
    B, D, H, W, C = x.shape
    y = _out((B, 2 * D, 2 * H, 2 * W, C), torch.float32, x.device)
    check(lib().csd_nearest_up2_3d_ndhwc(ptr(x), ptr(y), B, D, H, W, C, current_stream(x.device)), 'nearest_up2_3d')
    return y


def groupnorm_scale_shift(x0, gamma, beta, x1=None, groups=32, eps=1e-6):
    """GroupNorm statistics of x = x0 (| x1) on channels-last tensors [B, ..., C] without the normalised tensor: (nscale, nshift), each
    [B, C0+C1] = rstd*gamma and beta - mean*rstd*gamma - the prologue operands of conv3d_block / conv3x3_block."""
    x0, gamma, beta = _c(x0, 'x0'), _c(gamma, 'gamma'), _c(beta, 'beta')
    B, C0 = x0.shape[0], x0.shape[-1]
    S = x0.numel() // max(B * C0, 1)
    C1 = 0
    if x1 is not None:
        x1 = _c(x1, 'x1')
        C1 = x1.shape[-1]
        if tuple(x1.shape[:-1]) != tuple(x0.shape[:-1]):
            raise RuntimeError('groupnorm_scale_shift: x1 %s does not match x0 %s' % (tuple(x1.shape), tuple(x0.shape)))
    if tuple(gamma.shape) != (C0 + C1,) or tuple(beta.shape) != (C0 + C1,):
        raise RuntimeError('groupnorm_scale_shift: gamma / beta are not [%d]' % (C0 + C1))
    nscale = _out((B, C0 + C1), torch.float32, x0.device)
    nshift = _out(nscale.shape, nscale.dtype, nscale.device)
    sc = _scratch(lib().csd_groupnorm_scale_shift_scratch_bytes(B, C0 + C1, S, groups), x0.device)
    check(lib().csd_groupnorm_scale_shift(ptr(x0), ptr(x1), ptr(gamma), ptr(beta), ptr(nscale), ptr(nshift), B, C0, C1, S, groups,
                                          float(eps), ptr(sc), current_stream(x0.device)), 'groupnorm_scale_shift')
    return nscale, nshift


def attention(q, k, v):
    """softmax(q.k C^-1/2) v over H*W positions (models/layers.py:584-588)."""
    q, k, v = _c(q, 'q'), _c(k, 'k'), _c(v, 'v')
    B, C, H, W = q.shape
    out = _out(q.shape, q.dtype, q.device)
    sc = _scratch(lib().csd_attention_scratch_bytes(B, C, H, W), q.device)
    check(lib().csd_attention(ptr(q), ptr(k), ptr(v), ptr(out), B, C, H, W, ptr(sc), current_stream(q.device)),
          'attention')
    return out


def _upfirdn2d_raw(x, kernel, up, down, pad4):
    """csd_upfirdn2d with per-axis factors and four pads (x0, x1, y0, y1); negative pads crop."""
    x, kernel = _c(x, 'x'), _c(kernel, 'kernel')
    N, C, H, W = x.shape
    kh, kw = kernel.shape
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad4
    OH = (H * uy + py0 + py1 - kh) // dy + 1
    OW = (W * ux + px0 + px1 - kw) // dx + 1
    out = _out((N, C, OH, OW), torch.float32, x.device)
    check(lib().csd_upfirdn2d(ptr(x), ptr(kernel), ptr(out), N, C, H, W, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1,
                              current_stream(x.device)), 'upfirdn2d')
    return out


class _UpFirDn2dBackward(torch.autograd.Function):
    """grad_input = upfirdn2d(grad_output, flip(kernel), up=down, down=up, pad=g_pad) (op/upfirdn2d.py:20-85)."""

    @staticmethod
    def forward(ctx, grad_output, kernel, grad_kernel, up, down, pad, g_pad, in_size, out_size):
        ctx.save_for_backward(kernel)
        ctx.up, ctx.down, ctx.pad, ctx.in_size, ctx.out_size = up, down, pad, in_size, out_size
        g = _upfirdn2d_raw(grad_output.reshape(in_size[0], in_size[1], out_size[0], out_size[1]), grad_kernel, down, up, g_pad)
        return g.view(in_size)

    @staticmethod
    def backward(ctx, gradgrad_input):
        kernel, = ctx.saved_tensors
        gg = _upfirdn2d_raw(gradgrad_input.contiguous(), kernel, ctx.up, ctx.down, ctx.pad)
        return gg, None, None, None, None, None, None, None, None


class _UpFirDn2d(torch.autograd.Function):
    """Differentiable upfirdn2d, same autograd structure as the reference's UpFirDn2d (op/upfirdn2d.py:88-145)."""

    @staticmethod
    def forward(ctx, x, kernel, up, down, pad):
        ux, uy = up
        dx, dy = down
        px0, px1, py0, py1 = pad
        kh, kw = kernel.shape
        _, _, in_h, in_w = x.shape
        out = _upfirdn2d_raw(x, kernel, up, down, pad)
        out_h, out_w = out.shape[2], out.shape[3]
        ctx.save_for_backward(kernel, torch.flip(kernel, [0, 1]))
        ctx.in_size, ctx.out_size, ctx.up, ctx.down, ctx.pad = tuple(x.shape), (out_h, out_w), up, down, pad
        ctx.g_pad = (kw - px0 - 1, in_w * ux - out_w * dx + px0 - ux + 1,
                     kh - py0 - 1, in_h * uy - out_h * dy + py0 - uy + 1)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        kernel, grad_kernel = ctx.saved_tensors
        g = _UpFirDn2dBackward.apply(grad_output.contiguous(), kernel, grad_kernel, ctx.up, ctx.down, ctx.pad, ctx.g_pad,
                                     ctx.in_size, ctx.out_size)
        return g, None, None, None, None


def upfirdn2d(x, kernel, up=1, down=1, pad=(0, 0)):
    """Same call signature as the reference's op.upfirdn2d (op/upfirdn2d.py:147-158); differentiable w.r.t. ``x`` with
    the reference's backward (the same FIR kernel flipped, up/down swapped, pads g_pad)."""
    return _UpFirDn2d.apply(x, kernel, (up, up), (down, down), (pad[0], pad[1], pad[0], pad[1]))


def fused_leaky_relu(x, bias, negative_slope=0.2, scale=2 ** 0.5):
    """Forward of op.fused_leaky_relu (op/fused_act.py:86-97): lrelu(x + b[c]) * scale."""
    x, bias = _c(x, 'x'), _c(bias, 'bias')
    out = _out(x.shape, x.dtype, x.device)
    inner = 1
    for s in x.shape[2:]:
        inner *= s
    check(lib().csd_fused_bias_act(ptr(x), ptr(bias), None, ptr(out), x.numel(), x.shape[1], inner, 3, 0,
                                   negative_slope, scale, current_stream(x.device)), 'fused_bias_act')
    return out


def nearest_up2(x):
    x = _c(x, 'x')
    N, C, H, W = x.shape
    out = _out((N, C, 2 * H, 2 * W), torch.float32, x.device)
    check(lib().csd_nearest_up2(ptr(x), ptr(out), N, C, H, W, current_stream(x.device)), 'nearest_up2')
    return out


def timestep_embedding(t, dim):
    t = _c(t, 't')
    out = _out((t.shape[0], dim), torch.float32, t.device)
    check(lib().csd_timestep_embedding(ptr(t), ptr(out), t.shape[0], dim, current_stream(t.device)),
          'timestep_embedding')
    return out


def linear(x, weight, bias=None, act_in='none'):
    """act_in(x) @ weight.T + bias on [B, K] (nn.Linear; the reference applies the activation to the INPUT of the
    second temb layer and of every Dense_0: models/ncsnpp.py:257-263, layerspp.py:253-255)."""
    x, weight = _c(x, 'x'), _c(weight, 'weight')
    if bias is not None:
        bias = _c(bias, 'bias')
    B, K = x.shape
    N = weight.shape[0]
    out = _out((B, N), torch.float32, x.device)
    check(lib().csd_linear(ptr(x), ptr(weight), ptr(bias), ptr(out), B, K, N, _lib.ACT_IDS[act_in],
                           current_stream(x.device)), 'linear')
    return out


def fourier_embedding(t, W):
    """GaussianFourierProjection (models/layerspp.py:32-41): [sin(2 pi W t), cos(2 pi W t)]."""
    t, W = _c(t, 't'), _c(W, 'W')
    out = _out((t.shape[0], 2 * W.shape[0]), torch.float32, t.device)
    check(lib().csd_fourier_embedding(ptr(t), ptr(W), ptr(out), t.shape[0], W.shape[0], current_stream(t.device)),
          'fourier_embedding')
    return out


def axpby(a, b=None, alpha=1.0, beta=1.0, gamma=0.0, post=1.0):
    """(alpha*a + beta*b + gamma) * post, elementwise (b optional)."""
    a = _c(a, 'a')
    if b is not None:
        b = _c(b, 'b')
        if b.shape != a.shape:
            raise RuntimeError('axpby: shapes %s and %s differ' % (tuple(a.shape), tuple(b.shape)))
    out = _out(a.shape, a.dtype, a.device)
    check(lib().csd_axpby(ptr(a), ptr(b), ptr(out), float(alpha), float(beta), float(gamma), float(post), a.numel(),
                          current_stream(a.device)), 'axpby')
    return out


def _planes(t, name, scale):
    t = _c(t, name)
    if t.dim() < 2 or t.shape[-1] != t.shape[-2]:
        raise RuntimeError('%s must be [..., side, side] (got %s)' % (name, tuple(t.shape)))
    if int(scale) < 2:
        raise RuntimeError('%s: scale must be at least 2 (got %r)' % (name, scale))
    return t, int(t.shape[-1]), int(scale), t.numel() // (t.shape[-1] * t.shape[-2])


def bilinear_up(y, scale):
    """``F.interpolate(y, scale_factor=K, mode='bilinear', align_corners=False)`` for an integer K >= 2 on [..., s, s]: the upsample of
    csd_unet_config.y_scale (the same device function as the network's input kernels - csrc/common.h: bilin_up)."""
    y, side, K, n = _planes(y, 'y', scale)
    out = _out(tuple(y.shape[:-2]) + (side * K, side * K), torch.float32, y.device)
    check(lib().csd_bilinear_up(ptr(y), ptr(out), n, side, K, current_stream(y.device)), 'bilinear_up')
    return out


def bilinear_down_adjoint(g, scale):
    """the transpose of ``bilinear_down``: [..., s, s] -> [..., K s, K s], a quarter of g at the four centre pixels of each K x K block
    (K odd: g at the centre pixel), zero elsewhere"""
    g, side, K, n = _planes(g, 'g', scale)
    out = _out(tuple(g.shape[:-2]) + (side * K, side * K), torch.float32, g.device)
    check(lib().csd_bilinear_down_adjoint(ptr(g), ptr(out), n, side * K, K, current_stream(g.device)), 'bilinear_down_adjoint')
    return out


class _BilinearDown(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, K):
        ctx.K = K
        v, side, K, n = _planes(v, 'v', K)
        if side % K:
            raise RuntimeError('bilinear_down: scale %d must divide the side %d' % (K, side))
        out = _out(tuple(v.shape[:-2]) + (side // K, side // K), torch.float32, v.device)
        check(lib().csd_bilinear_down(ptr(v), ptr(out), n, side, K, current_stream(v.device)), 'bilinear_down')
        return out

    @staticmethod
    def backward(ctx, g):
        return bilinear_down_adjoint(g, ctx.K), None


def bilinear_down(v, scale):
    """``F.interpolate(v, size=S // K, mode='bilinear', align_corners=False)`` (no antialias) for an integer K >= 2 that divides S, on
    [..., S, S]: the mean of the 2 x 2 block at rows / columns K i + K / 2 - 1, K i + K / 2 (K even) or the pixel K i + (K - 1) / 2
    (K odd) - the downsample of csd_unet_config.y_scale (csrc/common.h: bilin_down).  Differentiable (``bilinear_down_adjoint``)."""
    return _BilinearDown.apply(v, int(scale))


def bias_add_nchw(x, bias, act='none'):
    """act(x + bias[:, :, None, None]) with bias [B, C] (or [C])."""
    x, bias = _c(x, 'x'), _c(bias, 'bias')
    B, C = x.shape[0], x.shape[1]
    inner = x.numel() // (B * C)
    stride = C if bias.dim() == 2 else 0
    out = _out(x.shape, x.dtype, x.device)
    check(lib().csd_bias_add_nchw(ptr(x), ptr(bias), ptr(out), B, C, inner, stride, _lib.ACT_IDS[act],
                                  current_stream(x.device)), 'bias_add_nchw')
    return out


def randn(shape, seed, stream_id, device):
    """Counter-based standard normals (Philox4x32-10): same (seed, stream_id) -> same tensor."""
    out = _out(shape, torch.float32, device)
    check(lib().csd_randn(ptr(out), out.numel(), int(seed), int(stream_id), current_stream(out.device)), 'randn')
    return out


def _addr(t, name):
    """device address of a float32 GPU tensor whose elements lie densely in memory (a view at any 4-byte offset is fine)"""
    _lib.require_gpu_tensor(t, name)
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)
    return ctypes.c_void_p(t.data_ptr())


def inpaint_blend(x, data, mask, z=None, mean_scale=1.0, std=0.0, seed=0, stream_id=0, x_mean=True):
    """In-place re-imposition of the known pixels (sampling/unconditional.py:268-271), one kernel:
    ``masked_mean = mean_scale*data; masked = masked_mean + std*z; x = x*(1 - mask) + masked*mask;
    x_mean = x*(1 - mask) + masked_mean*mask`` (x_mean from the new x); returns ``(x, x_mean)``, ``x_mean=False``: ``(x, None)``.

    ``z=None``: the normals of ``randn(shape, seed, stream_id)`` are made in registers (bit-identical to passing that tensor); with
    ``std == 0`` nothing is drawn.  ``mask`` has ``x``'s shape and may hold any value in [0, 1].  The tensors may be views at any
    element offset: 16-byte accesses are used when every address allows them."""
    tensors = [('x', x), ('data', data), ('mask', mask)] + ([('z', z)] if z is not None else [])
    for name, t in tensors[1:]:
        if t.shape != x.shape:
            raise RuntimeError('inpaint_blend: %s has shape %s, x has %s' % (name, tuple(t.shape), tuple(x.shape)))
    xm = _out(x.shape, x.dtype, x.device) if x_mean else None
    check(lib().csd_inpaint_blend(_addr(x, 'x'), ptr(xm), _addr(data, 'data'), _addr(mask, 'mask'),
                                  _addr(z, 'z') if z is not None else None, float(mean_scale), float(std), x.numel(), int(seed),
                                  int(stream_id), current_stream(x.device)), 'inpaint_blend')
    return x, xm


def _color_matrix(matrix):
    """the host 3 x 3 fp32 array the colorization entries take (None: the library's default, the reference's M)"""
    if matrix is None:
        return None
    m = torch.as_tensor(matrix, dtype=torch.float32).cpu().contiguous()
    if tuple(m.shape) != (3, 3):
        raise RuntimeError('colorization matrix must be 3 x 3 (decouple(v)[j] = sum_i v[i] * M[i][j]), got %s' % (tuple(m.shape),))
    return (ctypes.c_float * 9)(*[float(v) for v in m.flatten()])


def _color_state(x, gray0, who):
    _lib.require_gpu_tensor(x, 'x')
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError('%s: the state must be [B, 3, H, W] (got %s): the decoupled space has three channels' % (who, tuple(x.shape)))
    B, _, H, W = x.shape
    if tuple(gray0.shape) != (B, 1, H, W):
        raise RuntimeError('%s: gray0 has shape %s, the state %s needs %s' % (who, tuple(gray0.shape), tuple(x.shape), (B, 1, H, W)))
    return B, H * W


def colorize_gray0(gray, matrix=None):
    """Channel 0 of ``decouple(gray)``: [B, 3, H, W] -> [B, 1, H, W], ``(gray[:, 0]*M[0][0] + gray[:, 1]*M[1][0]) + gray[:, 2]*M[2][0]``.
    The colorizers compute it once per call."""
    _lib.require_gpu_tensor(gray, 'gray')
    if gray.dim() != 4 or gray.shape[1] != 3:
        raise RuntimeError('colorize_gray0: the gray-scale image must be [B, 3, H, W] (got %s)' % (tuple(gray.shape),))
    B, _, H, W = gray.shape
    out = _out((B, 1, H, W), torch.float32, gray.device)
    check(lib().csd_colorize_gray0(_addr(gray, 'gray'), ptr(out), B, H * W, _color_matrix(matrix), current_stream(gray.device)),
          'colorize_gray0')
    return out


def colorize_start(x, gray0, matrix=None):
    """In place: the prior ``x`` [B, 3, H, W] becomes the colorizer's initial state ``couple(decouple(gray)*mask +
    decouple(prior*(1 - mask)))`` (controllable_generation.py:180-182; mask = 1 on channel 0, the prior masked in image space)."""
    B, hw = _color_state(x, gray0, 'colorize_start')
    check(lib().csd_colorize_blend(_addr(x, 'x'), None, _addr(gray0, 'gray0'), None, 1.0, 0.0, B, hw, 1, _color_matrix(matrix), None,
                                   0, 0, current_stream(x.device)), 'colorize_blend')
    return x


def colorize_blend(x, gray0, z=None, mean_scale=1.0, std=0.0, seed=0, stream_id=0, x_mean=True, matrix=None):
    """In-place re-imposition of the gray channel (controllable_generation.py:150-153), one kernel.  With ``decouple(v)[j] = sum_i v[i] *
    M[i][j]`` and ``couple`` the same contraction with the inverse: ``masked_mean = mean_scale*gray0; masked = masked_mean + z[:, :1]*std;
    x = couple(cat(masked, decouple(x)[:, 1:])); x_mean = couple(cat(masked_mean, decouple(x)[:, 1:]))`` (x_mean from the new x);
    returns ``(x, x_mean)``, ``x_mean=False``: ``(x, None)``.

    ``x`` is [B, 3, H, W], ``gray0`` [B, 1, H, W] (``colorize_gray0``).  ``z`` has ``x``'s shape; only its channel 0 is read.
    ``z=None``: those elements of ``randn(x.shape, seed, stream_id)`` are made in registers (bit-identical to passing that tensor);
    with ``std == 0`` nothing is drawn.  ``matrix=None`` is the reference's M; its inverse is the float64 inverse rounded once.  A matrix
    with max |M M^T - I| > 1e-6 is refused.  The tensors may be views at any element offset: 16-byte accesses are used when every
    address and H*W allow them."""
    B, hw = _color_state(x, gray0, 'colorize_blend')
    if z is not None and z.shape != x.shape:
        raise RuntimeError('colorize_blend: z has shape %s, x has %s' % (tuple(z.shape), tuple(x.shape)))
    xm = _out(x.shape, x.dtype, x.device) if x_mean else None
    check(lib().csd_colorize_blend(_addr(x, 'x'), ptr(xm), _addr(gray0, 'gray0'), _addr(z, 'z') if z is not None else None,
                                   float(mean_scale), float(std), B, hw, 0, _color_matrix(matrix), None, int(seed), int(stream_id),
                                   current_stream(x.device)), 'colorize_blend')
    return x, xm


def _band_matrix(matrix):
    """the host 4 x 4 fp32 array csd_band_split / csd_band_merge take (None: the library's orthonormal Haar matrix)"""
    if matrix is None:
        return None
    m = torch.as_tensor(matrix, dtype=torch.float32).cpu().contiguous()
    if tuple(m.shape) != (4, 4):
        raise RuntimeError('band matrix must be 4 x 4 (rows = bands, columns = 2 dy + dx), got %s' % (tuple(m.shape),))
    return (ctypes.c_float * 16)(*[float(v) for v in m.flatten()])


def _sample_ld(t, name):
    """floats between consecutive samples of a float32 GPU tensor [B, C, H, W] whose samples are dense (a channel slice of a wider
    contiguous tensor qualifies: the library takes a per-sample stride)"""
    _lib.require_gpu_tensor(t, name)
    if t.dim() != 4:
        raise RuntimeError('%s must be [B, C, H, W] (got %s)' % (name, tuple(t.shape)))
    B, C, H, W = t.shape
    if t.numel() == 0 or tuple(t.stride()[1:]) != (H * W, W, 1) or (B > 1 and t.stride(0) < C * H * W):
        raise RuntimeError('%s must have dense samples: strides (ld, H*W, W, 1) with ld >= C*H*W (got %s for %s)'
                           % (name, tuple(t.stride()), tuple(t.shape)))
    return int(t.stride(0)) if B > 1 else C * H * W


def band_split(x, matrix=None):
    """Image [B, C, 2S, 2S] -> its four bands [B, 4C, S, S], band-major (channel C*k + c is band k of image channel c): the 2x2-block,
    stride-2 orthogonal transform of the Haar multi-scale models, ``band_k = sum_{dy,dx} matrix[k][2dy + dx] * x[2i + dy, 2j + dx]``.
    ``matrix=None`` is the orthonormal Haar matrix (include/csd.h, csd_band_split, spells it out and says why it is an argument: the
    order and signs of the reference layer's bands 1 - 3 could not be checked against iunets).  A matrix with max |M M^T - I| > 1e-6 and
    an odd image side are refused."""
    ld = _sample_ld(x, 'x')
    B, C, H, W = x.shape
    if H != W or H % 2:
        raise RuntimeError('band_split: the image side must be even and the image square (got %d x %d)' % (H, W))
    S = H // 2
    out = _out((B, 4 * C, S, S), torch.float32, x.device)
    check(lib().csd_band_split(ctypes.c_void_p(x.data_ptr()), ld, ptr(out), 4 * C * S * S, B, C, S, _band_matrix(matrix),
                               current_stream(x.device)), 'band_split')
    return out


def band_merge(lo, hi, matrix=None, out=None):
    """The transpose (= inverse) of ``band_split``: low band ``lo`` [B, C, S, S] and detail bands ``hi`` [B, 3C, S, S] -> the image
    [B, C, 2S, 2S].  ``lo`` / ``hi`` may be channel slices of wider tensors (no cat is needed), and ``out`` may be given: a float32
    tensor or channel slice [B, C, 2S, 2S] with dense samples, e.g. ``buf[:, :C]`` of a [B, 4C, 2S, 2S] buffer, whose other channels
    stay untouched."""
    lo_ld, hi_ld = _sample_ld(lo, 'lo'), _sample_ld(hi, 'hi')
    B, C, S, W = lo.shape
    if S != W or tuple(hi.shape) != (B, 3 * C, S, S):
        raise RuntimeError('band_merge: lo %s needs hi [B, 3C, S, S], got %s' % (tuple(lo.shape), tuple(hi.shape)))
    if out is None:
        out = _out((B, C, 2 * S, 2 * S), torch.float32, lo.device)
    elif tuple(out.shape) != (B, C, 2 * S, 2 * S):
        raise RuntimeError('band_merge: out has shape %s, the image is %s' % (tuple(out.shape), (B, C, 2 * S, 2 * S)))
    x_ld = _sample_ld(out, 'out')
    check(lib().csd_band_merge(ctypes.c_void_p(lo.data_ptr()), lo_ld, ctypes.c_void_p(hi.data_ptr()), hi_ld,
                               ctypes.c_void_p(out.data_ptr()), x_ld, B, C, S, _band_matrix(matrix), current_stream(lo.device)), 'band_merge')
    return out


def scale_rows(x, scale, divide=False):
    """x[b] * scale[b] (or / scale[b]) - divide_by_sigmas (models/utils.py:50-74)."""
    x, scale = _c(x, 'x'), _c(scale, 'scale')
    out = _out(x.shape, x.dtype, x.device)
    B = x.shape[0]
    check(lib().csd_scale_rows(ptr(out), ptr(x), ptr(scale), int(divide), B, x.numel() // B,
                               current_stream(x.device)), 'scale_rows')
    return out


def dsm_perturb(x, std, m=None, z=None, seed=0, stream_id=0):
    """``x_t[b] = m[b] * x[b] + std[b] * z[b]`` in one kernel with the three roundings of ``losses._perturb`` (bitwise that route).
    ``m``, ``std``: device [B]; ``m=None``: 1 (the VE SDEs).  ``z=None``: the normals of ``randn(x.shape, seed, stream_id)`` made in
    registers (bit-identical to passing that tensor)."""
    x, std = _c(x, 'x'), _c(std, 'std')
    B = x.shape[0]
    tensors = [('std', std, (B,))] + ([('m', _c(m, 'm'), (B,))] if m is not None else []) + \
              ([('z', _c(z, 'z'), tuple(x.shape))] if z is not None else [])
    for name, t, shape in tensors:
        if tuple(t.shape) != shape:
            raise RuntimeError('dsm_perturb: %s has shape %s, expected %s' % (name, tuple(t.shape), shape))
    out = _out(x.shape, x.dtype, x.device)
    check(lib().csd_dsm_perturb(ptr(out), ptr(x), ptr(m.contiguous()) if m is not None else None, ptr(std),
                                ptr(z.contiguous()) if z is not None else None, B, x.numel() // B, int(seed), int(stream_id),
                                current_stream(x.device)), 'dsm_perturb')
    return out


def dsm_residual(net, segments, seed=0, want_d_out=True):
    """The weighted denoising score-matching residual over 1 or 2 segments of the network's flat per-sample output rows (include/csd.h:
    csd_dsm_residual).  ``net`` [B, ...] contiguous; ``segments``: dicts with ``offset``, ``length`` (floats inside a row), ``a``, ``b``,
    ``w`` (device [B]) and either ``z`` (device [B, length]) or ``stream_id`` (the Philox fill of ``(seed, stream_id)``).
    Returns ``(loss, loss_rows, d_out)``: a [1] float32 tensor = sum_b loss_rows[b], the [B] float64 per-sample values, and
    ``2 w a (a h + b z)`` in ``net``'s shape (zeros outside the segments; None with ``want_d_out=False``)."""
    net = _c(net, 'net')
    B = net.shape[0]
    segs = (_lib.DsmSegment * max(len(segments), 1))()
    keep = []
    for k, s in enumerate(segments[:len(segs)]):
        c = [_c(s[n], n) for n in ('a', 'b', 'w')]
        for n, t in zip('abw', c):
            if tuple(t.shape) != (B,):
                raise RuntimeError('dsm_residual: %s of segment %d has shape %s, expected (%d,)' % (n, k, tuple(t.shape), B))
        z = s.get('z')
        if z is not None:
            z = _c(z, 'z')
            if z.numel() != B * int(s['length']):
                raise RuntimeError('dsm_residual: z of segment %d has %d elements, expected %d' % (k, z.numel(), B * int(s['length'])))
        keep += c + [z]
        segs[k].offset, segs[k].length = int(s['offset']), int(s['length'])
        segs[k].a, segs[k].b, segs[k].w = (t.data_ptr() for t in c)
        segs[k].z = z.data_ptr() if z is not None else None
        segs[k].stream_id = int(s.get('stream_id', 0))
    dev = net.device
    d_out = _out(net.shape, torch.float32, dev) if want_d_out else None
    partials = _out(B * max(len(segments), 1) * _lib.DSM_PARTS, torch.float64, dev)
    rows, loss = _out(B, torch.float64, dev), _out(1, torch.float32, dev)
    check(lib().csd_dsm_residual(ptr(net), net.numel() // B, segs, len(segments), ptr(d_out), ptr(partials), ptr(rows), ptr(loss), B,
                                 int(seed), current_stream(dev)), 'dsm_residual')
    return loss, rows, d_out


def langevin_step(x, net, z, std, snr, alpha=1.0):
    """In-place Langevin corrector update (sampling/correctors.py:51-78,88-108); ``alpha`` = sde.alphas[timestep] for the VP / subVP
    SDEs, 1 for the VE SDEs; returns (x, x_mean)."""
    x, net, z = _c(x, 'x'), _c(net, 'net'), _c(z, 'z')
    B = x.shape[0]
    x_mean = _out(x.shape, x.dtype, x.device)
    sc = _scratch(lib().csd_update_scratch_bytes(B), x.device)
    check(lib().csd_langevin_step(ptr(x), ptr(x_mean), ptr(net), ptr(z), float(std), float(snr), float(alpha), B,
                                  x.numel() // B, ptr(sc), current_stream(x.device)), 'langevin_step')
    return x, x_mean


def row_norms(x):
    """||x_b||_2 per sample -> [B] (fp64 accumulation on the device)."""
    x = _c(x, 'x')
    B = x.shape[0]
    out = _out(B, torch.float32, x.device)
    check(lib().csd_row_norms(ptr(x), ptr(out), B, x.numel() // B, current_stream(x.device)), 'row_norms')
    return out


def affine_noise_step(x, score, z, p, a, c):
    """In-place x_mean = p*x + a*score; x = x_mean + c*z (Euler-Maruyama / ancestral / annealed-Langevin updates)."""
    x, score, z = _c(x, 'x'), _c(score, 'score'), _c(z, 'z')
    x_mean = _out(x.shape, x.dtype, x.device)
    check(lib().csd_affine_noise_step(ptr(x), ptr(x_mean), ptr(score), ptr(z), float(p), float(a), float(c),
                                      x.numel(), current_stream(x.device)), 'affine_noise_step')
    return x, x_mean


def reverse_diffusion_step(x, net, z, std, G, drift=None, probability_flow=False):
    """In-place reverse-diffusion predictor update (sampling/predictors.py:84-89,97-102).

    ``drift``: None for an SDE without forward drift (VE), else ``(a, b, sub_x)`` with the discretised forward drift
    f = (a*x)*b, minus x when ``sub_x`` (VP: (sqrt(alpha_i), 1, True); sub-VP: (phi(t), dt, False)).  ``probability_flow``: the
    reverse ODE (half the score term, no noise; ``z`` is still read).  Without either, the VE kernel runs as before."""
    x, net, z = _c(x, 'x'), _c(net, 'net'), _c(z, 'z')
    B = x.shape[0]
    x_mean = _out(x.shape, x.dtype, x.device)
    if drift is None and not probability_flow:
        check(lib().csd_reverse_diffusion_step(ptr(x), ptr(x_mean), ptr(net), ptr(z), float(std), float(G), B,
                                               x.numel() // B, current_stream(x.device)), 'reverse_diffusion_step')
        return x, x_mean
    a, b, sub_x = drift if drift is not None else (0.0, 0.0, False)
    form = 0 if drift is None else (2 if sub_x else 1)
    check(lib().csd_reverse_diffusion_step_ex(ptr(x), ptr(x_mean), ptr(net), ptr(z), float(std), float(G), float(a), float(b), form,
                                              0.5 if probability_flow else 1.0, 0.0 if probability_flow else float(G), B,
                                              x.numel() // B, current_stream(x.device)), 'reverse_diffusion_step_ex')
    return x, x_mean
