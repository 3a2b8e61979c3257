"""DDPM-family score networks as thin adapters over the HIP graph executor.

Registers the reference's names ``ddpm``, ``ddpm_paired_SR3``, ``ddpm_paired``, ``ddpm_2xSR`` and ``ddpm_KxSR``
(models/ddpm.py:80,275,287,300,316) with the reference's constructor / call signatures:

    model = create_model(config)              # cls(config)
    out = model(x | {'x': x, 'y': y}, labels) # Tensor | {'x': .., 'y': ..}

The nn.Module holds ONLY the parameters, named exactly like the reference ``state_dict``
(``all_modules.{i}.Conv_0.weight`` ...; conv OIHW, NIN ``W`` [in,out], Linear [out,in]) so that
reference checkpoints load with ``load_state_dict``; the parameter table itself comes from the
library (csd_unet_param_info), which rebuilds the module list from the config the way
``DDPM.__init__`` does.  ``forward`` hands raw device pointers to ``csd_unet_forward``; all
arithmetic runs in libcsd_hip.so.  There is no PyTorch fallback.  The operator-granular training
executors (``train_executor = 'operators'``: ``_TrainOpsNHWC`` / ``_TrainOpsNCHW``, the yardstick of the
planned training graph) are executors of ``topology.run_unet`` on ``topology.build_modules``' list.
"""
import ctypes
import math
import os

import torch
import torch.nn as nn

from .. import _lib, grad_ops, grad_ops_nhwc, ops
from .._lib import check, current_stream, lib, ptr, require_gpu_tensor
from . import utils
from .topology import Executor, build_modules, run_unet


class _Node(nn.Module):
    """Parameter container: gives nested state_dict keys (``3.Conv_0.weight``)."""


def _fan_avg_uniform(shape, scale, is_nin):
    """``default_init(scale)`` = variance_scaling(scale, 'fan_avg', 'uniform') with the reference's
    default axes in_axis=1, out_axis=0 (models/layers.py:54-91)."""
    rf = 1
    for s in shape[2:]:
        rf *= s
    fan_in, fan_out = shape[1] * rf, shape[0] * rf
    var = (1e-10 if scale == 0 else scale) / ((fan_in + fan_out) / 2.0)
    return (torch.rand(*shape) * 2. - 1.) * math.sqrt(3 * var)


def _model_key(config, key, default):
    """config.model.<key>, or `default` where the config does not set it"""
    m = config.model
    v = m.get(key, None) if hasattr(m, 'get') else getattr(m, key, None)
    return default if v is None else v


def _precision(config, precision):
    """arithmetic of the 3x3 contractions: the constructor argument, else config.model.csd_precision, else $CSD_PRECISION, else
    'fp16x3'.  'fp32' (exact fp32 MFMA), 'fp16x3' (split-fp16 operands, three fp16 MFMAs per product: fp32-class accuracy - the
    DEFAULT: a model built from an unchanged reference config computes in the reference's precision class), 'fp16f8' (split operands,
    correction products with e4m3 operands on the fp8 matrix cores: 1e-5-class accuracy on the tested weights, opt-in), 'fp16' (opt-in,
    not certified).  Not a reference key."""
    if precision is None:
        precision = _model_key(config, 'csd_precision', None)
    if precision is None:
        precision = os.environ.get('CSD_PRECISION', 'fp16x3')
    if precision not in _lib.PREC_IDS:
        raise ValueError('unknown csd precision %r (choose from %s)' % (precision, sorted(_lib.PREC_IDS)))
    return precision


def _activation(config):
    """config.model.nonlinearity as a name of _lib.ACT_IDS (models/layers.py:29-41)"""
    act = config.model.nonlinearity.lower()
    if act not in _lib.ACT_IDS or act == 'none':
        raise NotImplementedError('activation function does not exist!')
    return act


class _HandleSurface:
    """What a network that owns a ``csd_unet`` handle offers to its callers (``sampling/fused.py``, the likelihood, the benches): the
    handle ``_h`` (``_create_unet``), the library's parameter table, the packed weights ``_packed`` (``_ensure_packed()`` packs again
    when a parameter moved or changed), the activation workspace ``_workspace(B)``, the evaluation ``_unet_forward`` and ``stats(B)``.
    Expects ``_param_names``, ``y_channels`` and ``device`` on the instance.  Every byte buffer comes from ``ops._scratch``."""

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                lib().csd_unet_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _create_unet(self, cfg):
        """the handle of a filled csd_unet_config; nothing is packed yet"""
        self._cfg, self._h = cfg, ctypes.c_void_p()
        check(lib().csd_unet_create(ctypes.byref(cfg), ctypes.byref(self._h)), 'unet_create')
        self._packed = self._packed_key = self._ws = None

    def _param_table(self):
        """[(state_dict name, shape)] as the library rebuilt it from the config (up to 5 dimensions: the 3-D conv weights)"""
        out = []
        name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 5)()
        for i in range(lib().csd_unet_num_params(self._h)):
            check(lib().csd_unet_param_info(self._h, i, ctypes.byref(name), ctypes.byref(ndim), shape), 'param_info')
            out.append((name.value.decode(), tuple(shape[j] for j in range(ndim.value))))
        return out

    def _unet_forward(self, x, y, labels, out_shape, y_noise=None, y_sigma=0.0):
        """one csd_unet_forward on inputs whose shapes the caller has checked"""
        B = x.shape[0]
        if self.y_channels:
            y = y.contiguous()
        self._ensure_packed()
        ws = self._workspace(B)
        out = ops._out(out_shape, torch.float32, x.device)
        check(lib().csd_unet_forward(self._h, ptr(self._packed), ptr(ws), ws.numel(), ptr(x.contiguous()),
                                     ptr(y) if self.y_channels else None, ptr(labels), ptr(out), B,
                                     ptr(y_noise) if y_noise is not None else None, float(y_sigma),
                                     current_stream(x.device)), 'unet_forward')
        return out

    # -- packing -----------------------------------------------------------------------------------
    def _ensure_packed(self):
        params = dict(self.named_parameters())
        key = (_lib.WEIGHT_EPOCH[0],) + tuple((p.data_ptr(), p._version) for p in params.values())
        if self._packed is not None and key == self._packed_key:
            return
        dev = self.device
        if dev.type != 'cuda':
            raise RuntimeError('the HIP score network runs on the MI355X only: move the model with .to("cuda") '
                               '(parameters are on %s); there is no CPU fallback' % dev)
        for name in self._param_names:
            p = params[name]
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError('parameter %s must be contiguous float32' % name)
            check(lib().csd_unet_set_param(self._h, name.encode(), ctypes.c_void_p(p.data_ptr()), p.numel()),
                  'set_param')
        nbytes = lib().csd_unet_packed_bytes(self._h)
        if self._packed is None or self._packed.numel() < nbytes or self._packed.device != dev:
            self._packed = ops._scratch(nbytes, dev)
        check(lib().csd_unet_pack(self._h, ptr(self._packed), current_stream(dev)), 'unet_pack')
        self._packed_key = key

    def _workspace(self, B):
        need = lib().csd_unet_workspace_bytes(self._h, B)
        if need == 0:
            raise RuntimeError('libcsd_hip: cannot plan batch %d: %s' % (B, lib().csd_last_error().decode()))
        if self._ws is None or self._ws.numel() < need or self._ws.device != self.device:
            self._ws = ops._scratch(need, self.device)
        return self._ws

    # -- the planned training graph (csd_unet_train_forward / csd_unet_backward*): what the autograd nodes _PlannedNet and
    # _InputGradNet ask of a model beside ``_h``, ``_param_names``, ``_dropout``, ``dropout_seed``, ``_train_calls`` and the shapes
    # ``_x_shape(B)`` / ``_out_shape(B)`` of one call's x (and d_x) and output ------------------------------------------------------
    _train_ws = None
    _train_ws_busy = False         # a forward whose backward has not run yet holds the shared training workspace
    _train_ws_owner = None         # ... identified by its call index

    def _train_workspace(self, B):
        need = lib().csd_unet_train_workspace_bytes(self._h, B, self._dropout)
        if need == 0:
            raise RuntimeError('libcsd_hip: cannot plan the training graph at batch %d: %s' % (B, lib().csd_last_error().decode()))
        if self._train_ws is None or self._train_ws.numel() < need or self._train_ws.device != self.device:
            self._train_ws = None
            self._train_ws = ops._scratch(need, self.device)
        return self._train_ws

    def _train_params(self):
        params = dict(self.named_parameters())
        return [params[name] for name in self._param_names]

    def stats(self, B):
        """(kernel launches, algorithmic FLOPs, algorithmic bytes) of one evaluation at batch B."""
        n, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        check(lib().csd_unet_stats(self._h, B, ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by)), 'unet_stats')
        return n.value, fl.value, by.value


class HipUNet(nn.Module, _HandleSurface):
    """Base adapter. Subclasses fix (x_channels, y_channels) conventions."""

    arch = 0
    x_squeeze = 0          # 1: x is the high-resolution image [B, x_channels / 4, 2S, 2S] (csd_unet_config.x_squeeze; DDPM_2xSR)
    y_scale = 0            # K >= 2: y is the low-resolution image [B, y_channels, S / K, S / K] (csd_unet_config.y_scale; the KxSR classes)

    def __init__(self, config, precision=None):
        super().__init__()
        m, d = config.model, config.data
        self.precision = precision = _precision(config, precision)
        self.nf = m.nf
        self.num_res_blocks = m.num_res_blocks
        self.attn_resolutions = tuple(m.attn_resolutions)
        self.num_resolutions = len(m.ch_mult)
        self.conditional = bool(m.conditional)
        self.centered = bool(d.centered)
        self.image_size = int(d.effective_image_size)
        self.out_channels = int(self._out_channels(config))
        self.x_channels, self.y_channels = self._channels(config)
        self._act_name = act = _activation(config)
        self._train_calls = 0
        self.train_layout = os.environ.get('CSD_TRAIN_LAYOUT', 'nhwc')     # 'nhwc' | 'nchw' (see _train_forward)
        self.train_executor = os.environ.get('CSD_TRAIN_EXECUTOR', 'planned')   # 'planned' (csd_unet_backward) | 'operators' (autograd)
        self._train_ws = None
        self._train_ws_busy = False        # a forward whose backward has not run yet holds the shared training workspace
        self._train_ws_owner = None        # ... identified by its call index
        self.dropout_seed = int(getattr(config, 'seed', 0) or 0)   # Philox key of the dropout masks
        cfg = _lib.UNetConfig()
        cfg.arch = self.arch
        cfg.nf = m.nf
        cfg.n_levels = len(m.ch_mult)
        for i, v in enumerate(m.ch_mult):
            cfg.ch_mult[i] = int(v)
        cfg.num_res_blocks = m.num_res_blocks
        cfg.n_attn = len(m.attn_resolutions)
        for i, v in enumerate(m.attn_resolutions):
            cfg.attn_resolutions[i] = int(v)
        cfg.image_size = self.image_size
        cfg.x_channels, cfg.y_channels, cfg.out_channels = self.x_channels, self.y_channels, self.out_channels
        cfg.resamp_with_conv = int(bool(m.resamp_with_conv))
        cfg.conditional = int(self.conditional)
        cfg.centered = int(self.centered)
        cfg.act = _lib.ACT_IDS[act]
        cfg.precision = _lib.PREC_IDS[precision]
        cfg.x_squeeze = int(self.x_squeeze)
        cfg.y_scale = int(self.y_scale)
        self._extra_config(cfg, config)
        self._create_unet(cfg)
        self._dropout = float(_model_key(config, 'dropout', 0.0))
        self._build_params()

    # -- parameters ------------------------------------------------------------------------------
    def _channels(self, config):
        raise NotImplementedError

    def _out_channels(self, config):
        return config.model.output_channels

    def _extra_config(self, cfg, config):
        """hook: architecture-specific fields of csd_unet_config"""

    def _build_params(self):
        table = self._param_table()
        last_idx = max(int(k.split('.')[1]) for k, _ in table)
        nodes = {}
        for key, shape in table:
            parts = key.split('.')           # all_modules, idx, [sub], leaf
            idx = int(parts[1])
            node = nodes.setdefault(idx, _Node())
            for sub in parts[2:-1]:
                if not hasattr(node, sub):
                    node.add_module(sub, _Node())
                node = getattr(node, sub)
            leaf = parts[-1]
            if len(shape) >= 2:
                is_nin = leaf == 'W'
                if 'Conv_1' in key or 'NIN_3' in key or (idx == last_idx and len(shape) == 4):
                    scale = 0.          # init_scale=0 -> 1e-10 (models/layers.py:648,575; ddpm.py:146)
                elif is_nin:
                    scale = 0.1         # NIN default init_scale (models/layers.py:556)
                else:
                    scale = 1.
                val = _fan_avg_uniform(shape, scale, is_nin)
            elif leaf == 'weight':      # GroupNorm gamma
                val = torch.ones(shape)
            else:
                val = torch.zeros(shape)
            node.register_parameter(leaf, nn.Parameter(val))
        self.all_modules = nn.ModuleList([nodes[i] for i in sorted(nodes)])
        assert sorted(nodes) == list(range(len(nodes)))
        self._param_names = [k for k, _ in table]

    @property
    def device(self):
        return next(self.parameters()).device

    # -- shapes at the library boundary ------------------------------------------------------------
    def _x_shape(self, B):
        """x (and d_x) of one call: [B, x_channels, S, S], or the image [B, x_channels / 4, 2S, 2S] of a squeezed network"""
        S = self.image_size
        return (B, self.x_channels // 4, 2 * S, 2 * S) if self.x_squeeze else (B, self.x_channels, S, S)

    def _y_shape(self, B):
        """y of one call: [B, y_channels, S, S], or [B, y_channels, S / K, S / K] with y_scale = K"""
        s = self.image_size // self.y_scale if self.y_scale else self.image_size
        return (B, self.y_channels, s, s)

    def _out_shape(self, B):
        """the buffer csd_unet_forward / csd_unet_train_forward write: [B, out_channels, S, S]; a squeezed network's is flat per sample
        (the x block in image layout, then the other channels at S x S - ``DDPM_2xSR._split``), and so is a y_scale network's (the x
        block, then the other channels at S / K - ``_KxSR._split``)"""
        S = self.image_size
        if self.y_scale:
            s = S // self.y_scale
            return (B, self.x_channels * S * S + (self.out_channels - self.x_channels) * s * s)
        return (B, self.out_channels * S * S) if self.x_squeeze else (B, self.out_channels, S, S)

    # -- evaluation --------------------------------------------------------------------------------
    def _run(self, x, y, labels, y_noise=None, y_sigma=0.0):
        require_gpu_tensor(x, 'x')
        if self.training and torch.is_grad_enabled():
            if y_noise is not None:
                raise RuntimeError('the fused y-perturbation is a sampling feature; perturb y before a training step')
            return self._train_forward(x, y, labels)
        if torch.is_grad_enabled() and x.requires_grad:
            if y_noise is not None:
                raise RuntimeError('the fused y-perturbation is a sampling feature; it has no input gradient')
            return self._input_grad_forward(x, y, labels)
        labels = self._check_io(x, y, labels)
        return self._unet_forward(x, y, labels, self._out_shape(x.shape[0]), y_noise, y_sigma)

    def _check_io(self, x, y, labels):
        """shapes of one call's x, y, labels; returns the labels as a contiguous float32 tensor on x's device"""
        B, S = x.shape[0], self.image_size
        if tuple(x.shape) != self._x_shape(B):
            raise RuntimeError('x has shape %s, expected %s' % (tuple(x.shape), self._x_shape(B)))
        if self.y_channels:
            require_gpu_tensor(y, 'y')
            if tuple(y.shape) != self._y_shape(B):
                raise RuntimeError('y has shape %s, expected %s' % (tuple(y.shape), self._y_shape(B)))
        labels = labels.to(device=x.device, dtype=torch.float32).contiguous()
        if labels.shape != (B,):
            raise RuntimeError('labels must have shape [%d]' % B)
        return labels

    # -- eval-mode autograd with respect to x: the planned training graph without dropout, an input-only backward ------------------
    def _input_grad_forward(self, x, y, labels):
        """``model.eval()`` with ``x.requires_grad`` under autograd: ONE node whose forward is csd_unet_train_forward with dropout 0
        (the activations stay in a private workspace) and whose backward is csd_unet_backward_ex(grads = NULL, d_x): the data gradient
        only, no parameter gradient.  Only x is differentiated (y is the condition)."""
        if y is not None and y.requires_grad:
            raise NotImplementedError('the HIP score network differentiates its input x only; y takes no gradient')
        if self.arch == 0 and not self._cfg.resamp_with_conv:
            raise NotImplementedError('input gradients with resamp_with_conv=False are not provided')
        labels = self._check_io(x, y, labels)
        self._xgrad_calls = getattr(self, '_xgrad_calls', 0) + 1
        return _InputGradNet.apply(self, x.contiguous(), y.detach().contiguous() if self.y_channels else None, labels.detach(),
                                   self._xgrad_calls)

    # -- training-mode evaluation: ONE planned graph behind the C ABI (csd_unet_train_forward / csd_unet_backward) -------------------
    def _train_forward_planned(self, x, y, labels):
        """``model.train()`` + autograd as ONE node: the forward is csd_unet_train_forward (the reference's layer sequence,
        models/ddpm.py:149-213, dropout on, activations kept in a library workspace), the backward csd_unet_backward (every
        parameter gradient from one call).  ``self.grad_sink``: when a Trainer owns the flat gradient buffer the gradients are
        written straight into ``p.grad`` (which it zeroed) and autograd is handed nothing to accumulate."""
        labels = self._check_io(x, y, labels)
        self._train_calls += 1
        return _PlannedNet.apply(self, x.contiguous(), y.contiguous() if self.y_channels else None, labels, *self._train_params())

    # -- training-mode evaluation: differentiable, operator-granular ------------------------------------------
    def _train_forward(self, x, y, labels):
        """``model.train()`` + autograd: the reference forward (models/ddpm.py:149-213) layer by layer on differentiable HIP
        operators (forward AND backward kernels behind include/csd.h), with ``nn.Dropout`` active (models/layers.py:647,662).
        The planned graph executor (csd_unet_forward) stays the inference path; this one keeps every activation that a
        gradient needs.  ``self.train_layout``: 'nhwc' (default) keeps activations in the library's layout between layers
        (grad_ops_nhwc: no layout change anywhere but the network's NCHW input and output), 'nchw' runs every layer through
        the NCHW per-operator ABI (grad_ops)."""
        if not self._cfg.resamp_with_conv:
            raise NotImplementedError('training with resamp_with_conv=False is not provided')
        if self.train_executor == 'planned' and self.arch == 0 and self.train_layout == 'nhwc':
            return self._train_forward_planned(x, y, labels)
        if self.x_squeeze:
            raise NotImplementedError('a squeezed network (ddpm_2xSR) trains on the planned graph only (CSD_TRAIN_EXECUTOR=planned, '
                                      'CSD_TRAIN_LAYOUT=nhwc)')
        if self.y_scale:
            raise NotImplementedError('a network with y_scale (ddpm_KxSR) trains on the planned graph only (CSD_TRAIN_EXECUTOR=planned, '
                                      'CSD_TRAIN_LAYOUT=nhwc)')
        labels = self._check_io(x, y, labels)
        self._train_calls += 1
        ex = (_TrainOpsNHWC if self.train_layout == 'nhwc' else _TrainOpsNCHW)(self)
        h = torch.cat([x, y], dim=1) if self.y_channels else x
        temb = ops.timestep_embedding(labels, self.nf) if self.conditional else None
        if not self.centered:
            h = ex.O.axpby(h, None, 2.0, 0.0, -1.0, 1.0)
        return run_unet(self._topology(), self.all_modules, ex, h, temb)

    def _topology(self):
        """the module list of this DDPM-family network (arch 0), as csrc/unet.hip builds it from the same config"""
        c = self._cfg
        return build_modules('ddpm', c.nf, c.ch_mult[:c.n_levels], c.num_res_blocks, self.x_channels + self.y_channels, self.out_channels,
                             [l for l in range(c.n_levels) if self.image_size >> l in self.attn_resolutions], self.conditional)


class _TrainOpsNCHW(Executor):
    """Executor of ``topology.run_unet`` for the training mode of the 2-D DDPM family: the arithmetic of each module of the reference
    forward (models/ddpm.py:149-213) on the differentiable NCHW operators of grad_ops.  One object per forward: it counts the dropout
    sites, whose Philox stream ids are ``(model._train_calls << 16) + k``, k = 1, 2, ... in module order."""

    O = grad_ops
    bias_add = staticmethod(grad_ops.bias_add_nchw)

    def __init__(self, model):
        self.model, self.prec, self.act, self.drops = model, model.precision, model._act_name, 0

    def qkv_attention(self, node, t):
        O, p = self.O, self.prec
        return O.attention(O.nin(t, node.NIN_0.W, node.NIN_0.b, p), O.nin(t, node.NIN_1.W, node.NIN_1.b, p),
                           O.nin(t, node.NIN_2.W, node.NIN_2.b, p))

    def stem(self, node, m, x):
        return self.O.conv2d(x, node.weight, node.bias, precision=self.prec)

    head_conv = stem

    def res(self, node, m, h, temb):
        O, act, model = self.O, self.act, self.model
        t = O.groupnorm_act(h, node.GroupNorm_0.weight, node.GroupNorm_0.bias, 32, 1e-6, act)
        t = O.conv2d(t, node.Conv_0.weight, node.Conv_0.bias, precision=self.prec)
        if temb is not None:
            t = self.bias_add(t, O.linear(temb, node.Dense_0.weight, node.Dense_0.bias, act_in=act))
        t = O.groupnorm_act(t, node.GroupNorm_1.weight, node.GroupNorm_1.bias, 32, 1e-6, act)
        self.drops += 1
        t = O.dropout(t, model._dropout, model.dropout_seed, (model._train_calls << 16) + self.drops)
        t = O.conv2d(t, node.Conv_1.weight, node.Conv_1.bias, precision=self.prec)
        if m.cin != m.cout:
            h = O.nin(h, node.NIN_0.W, node.NIN_0.b, self.prec)
        return O.axpby(h, t)

    def attn(self, node, m, h):
        O = self.O
        t = O.groupnorm_act(h, node.GroupNorm_0.weight, node.GroupNorm_0.bias, 32, 1e-6, 'none')
        return O.axpby(h, O.nin(self.qkv_attention(node, t), node.NIN_3.W, node.NIN_3.b, self.prec))

    def downsample(self, node, m, h, temb):
        return self.O.conv2d(h, node.Conv_0.weight, node.Conv_0.bias, stride=2, downsample_pad=True, precision=self.prec)

    def upsample(self, node, m, h, temb):
        return self.O.conv2d(h, node.Conv_0.weight, node.Conv_0.bias, up2=True, precision=self.prec)

    def gn(self, node, m, h):
        return self.O.groupnorm_act(h, node.weight, node.bias, 32, 1e-6, self.act)


class _TrainOpsNHWC(_TrainOpsNCHW):
    """... on grad_ops_nhwc: activations stay in the library's layout [B, H, W, C] between layers; only the first convolution (NCHW
    in) and the last (NCHW out) change it."""

    O, cdim = grad_ops_nhwc, 3
    bias_add = staticmethod(grad_ops_nhwc.bias_add)

    def qkv_attention(self, node, t):
        """q | k | v from ONE 1x1 contraction (weights concatenated: data movement), packed per pixel"""
        W = torch.cat([node.NIN_0.W, node.NIN_1.W, node.NIN_2.W], dim=1)
        b = torch.cat([node.NIN_0.b, node.NIN_1.b, node.NIN_2.b])
        return self.O.attention(self.O.nin(t, W, b, self.prec))

    def stem(self, node, m, x):
        return self.O.conv2d(x, node.weight, node.bias, precision=self.prec, layout=self.O.OUT_NHWC)

    def head_conv(self, node, m, h):
        return self.O.conv2d(h, node.weight, node.bias, precision=self.prec, layout=self.O.IN_NHWC)


def _release_shared_ws(model_ref, owner):
    """the forward that held the model's shared training workspace is done with it (its backward ran, or its graph was dropped).
    Ownership is keyed by the forward's call index, not by the buffer: the graph of iteration N is usually freed only after
    iteration N + 1's forward has taken the (same) workspace, and a release keyed by the pointer would then free it under the new owner."""
    model = model_ref()
    if model is not None and model._train_ws_busy and getattr(model, '_train_ws_owner', None) == owner:
        model._train_ws_busy = False
        model._train_ws_owner = None


def _release_private_ws(model_ref, handle, ws_ptr, call):
    """a monitoring forward's private workspace is about to be freed: drop the library's record of THAT forward (by call index: a late
    finalizer must not erase the record of a newer forward that was handed the same address - csd_unet_train_release_call)"""
    model = model_ref()
    if model is not None and getattr(model, '_h', None) is handle and handle is not None:
        lib().csd_unet_train_release_call(handle, ctypes.c_void_p(ws_ptr), ctypes.c_uint64(call))


class _PlannedNet(torch.autograd.Function):
    """The whole training-mode network as one autograd node over csd_unet_train_forward / csd_unet_backward."""

    @staticmethod
    def forward(ctx, model, x, y, labels, *params):
        B = x.shape[0]
        for name, p in zip(model._param_names, params):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != x.device:
                raise RuntimeError('parameter %s must be contiguous float32 on %s' % (name, x.device))
        # the shared training workspace belongs to ONE live forward; a second one (e.g. a monitoring forward between a training
        # forward and its backward) gets a workspace of its own, released with its autograd context
        shared = not model._train_ws_busy
        ws = model._train_workspace(B) if shared else ops._scratch(
            lib().csd_unet_train_workspace_bytes(model._h, B, model._dropout), x.device)
        table = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
        out = ops._out(model._out_shape(B), torch.float32, x.device)
        check(lib().csd_unet_train_forward(model._h, table, ptr(ws), ws.numel(), ptr(x), ptr(y) if y is not None else None,
                                           ptr(labels), ptr(out), B, model._dropout, model.dropout_seed, model._train_calls,
                                           current_stream(x.device)), 'unet_train_forward')
        ctx.model, ctx.table, ctx.ws, ctx.B, ctx.call = model, table, ws, B, model._train_calls
        ctx.fin = None
        if shared:
            model._train_ws_busy = True
            model._train_ws_owner = ctx.call
            import weakref
            ctx.fin = weakref.finalize(ctx, _release_shared_ws, weakref.ref(model), ctx.call)
        else:
            import weakref
            weakref.finalize(ctx, _release_private_ws, weakref.ref(model), model._h, ws.data_ptr(), ctx.call)
        ctx.shapes = [(p.shape, p.numel()) for p in params]
        # direct mode: the backward writes straight into the parameters' .grad views (the flat gradient buffer).  A parameter that
        # takes no gradient (the fixed Gaussian-Fourier W of NCSN++) has none: the library still writes one - into a throw-away buffer
        ctx.sink = [p.grad if p.requires_grad else False for p in params] if getattr(model, 'grad_sink', False) else None
        return out

    @staticmethod
    def backward(ctx, dout):
        model, B = ctx.model, ctx.B
        dout = dout.contiguous()
        direct = ctx.sink is not None and all(g is False or (g is not None and g.is_contiguous() and g.data_ptr() % 16 == 0)
                                              for g in ctx.sink)
        # (distributed.GradSync reads this: the gradient-ready events of the planned backward describe the FINAL gradients only
        # when the kernels wrote .grad themselves; otherwise autograd's accumulation runs after them)
        model._last_backward_direct = direct
        if direct:
            grads = [ops._out(shape, torch.float32, dout.device) if g is False else g
                     for g, (shape, _) in zip(ctx.sink, ctx.shapes)]
        else:
            offs = [0]
            for _, n in ctx.shapes:
                offs.append(offs[-1] + (n + 3) // 4 * 4)
            flat = ops._out(offs[-1], torch.float32, dout.device)
            grads = [flat[o:o + n].view(shape) for o, (shape, n) in zip(offs, ctx.shapes)]
        gtable = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        # d loss / d x from the same call when autograd asks for it (csd_unet_backward_ex: the parameter gradients are unchanged)
        dx = ops._out(model._x_shape(B), torch.float32, dout.device) if ctx.needs_input_grad[1] else None
        # gradient accumulation (train.Trainer sets both before each backward of a window; absent: one backward per step, as ever):
        # in direct mode the kernels ADD to the .grad views from the window's second micro-batch on, and only the window's last
        # backward records the gradient-ready events.  Off direct mode autograd accumulates the returned gradients itself.
        acc = 1 if direct and getattr(model, 'grad_accumulate', False) else 0
        marks = 1 if getattr(model, 'grad_marks', True) else 0
        check(lib().csd_unet_backward_acc(model._h, ctx.table, gtable, ptr(dx), ptr(ctx.ws), ctx.ws.numel(), ptr(dout), B, ctx.call,
                                          acc, marks, current_stream(dout.device)), 'unet_backward')
        if ctx.fin is not None:         # (the backward releases the workspace itself; the finalizer of this context must not fire later)
            ctx.fin.detach()
            _release_shared_ws(lambda: model, ctx.call)
        if direct:
            return (None, dx, None, None) + (None,) * len(grads)
        return (None, dx, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:]))


class _InputGradNet(torch.autograd.Function):
    """The eval-mode network as one autograd node with respect to x: csd_unet_train_forward (dropout 0) / csd_unet_backward_ex with
    grads = NULL.  Each forward owns a workspace; its record in the library is dropped after the backward (or with the context)."""

    @staticmethod
    def forward(ctx, model, x, y, labels, call):
        B = x.shape[0]
        params = model._train_params()
        for name, p in zip(model._param_names, params):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != x.device:
                raise RuntimeError('parameter %s must be contiguous float32 on %s' % (name, x.device))
        need = lib().csd_unet_train_workspace_bytes(model._h, B, 0.0)
        if need == 0:
            raise RuntimeError('libcsd_hip: cannot plan the input-gradient graph at batch %d: %s' % (B, lib().csd_last_error().decode()))
        ws = ops._scratch(need, x.device)
        table = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
        out = ops._out(model._out_shape(B), torch.float32, x.device)
        check(lib().csd_unet_train_forward(model._h, table, ptr(ws), ws.numel(), ptr(x), ptr(y), ptr(labels), ptr(out), B, 0.0,
                                           model.dropout_seed, call, current_stream(x.device)), 'unet_train_forward')
        import weakref
        ctx.model, ctx.params, ctx.table, ctx.ws, ctx.B, ctx.call = model, params, table, ws, B, call
        ctx.fin = weakref.finalize(ctx, _release_private_ws, weakref.ref(model), model._h, ws.data_ptr(), call)
        return out

    @staticmethod
    def backward(ctx, dout):
        model, B = ctx.model, ctx.B
        dout = dout.contiguous()
        dx = ops._out(model._x_shape(B), torch.float32, dout.device)
        check(lib().csd_unet_backward_ex(model._h, ctx.table, None, ptr(dx), ptr(ctx.ws), ctx.ws.numel(), ptr(dout), B, ctx.call,
                                         current_stream(dout.device)), 'unet_backward_ex')
        ctx.fin()
        return None, dx, None, None, None


@utils.register_model(name='ddpm')
class DDPM(HipUNet):
    """Unconditional DDPM U-Net: ``model(x, labels) -> Tensor`` (models/ddpm.py:80-213)."""

    # (configs that leave model.input_channels / output_channels out - configs/ve/haarflow/*.py: the 12 Haar bands - name the image's
    # channels in data.num_channels)
    def _channels(self, config):
        return int(_model_key(config, 'input_channels', config.data.num_channels)), 0

    def _out_channels(self, config):
        return _model_key(config, 'output_channels', config.data.num_channels)

    def forward(self, x, labels):
        return self._run(x, None, labels)


class _Paired(HipUNet):
    def _channels(self, config):
        cx = int(config.data.shape_x[0])
        return cx, int(config.model.input_channels) - cx


@utils.register_model(name='ddpm_paired_SR3')
class DDPM_paired_SR3(_Paired):
    """CDE / SR3 estimator: net(cat(x, y)) -> score_x (models/ddpm.py:275-285)."""

    def forward(self, input_dict, labels):
        return self._run(input_dict['x'], input_dict['y'], labels)


@utils.register_model(name='ddpm_paired')
class DDPM_paired(_Paired):
    """CMDE / VS-CMDE estimator: net(cat(x, y)) -> {'x': .., 'y': ..} (models/ddpm.py:287-298)."""

    def forward(self, input_dict, labels):
        out = self._run(input_dict['x'], input_dict['y'], labels)
        c = self.x_channels
        return {'x': out[:, :c], 'y': out[:, c:]}


class _Squeeze2x:
    """The 2x super-resolution wrappers (models/ddpm.py:39-52,300-314, models/ncsnpp.py:403-432) over a paired network: the U-Net behind
    a parameter-free space-to-depth squeeze of x.  ``forward({'x': [B, cx, 2S, 2S], 'y': [B, cy, S, S]}, labels) -> {'x': [B, cx, 2S, 2S],
    'y': [B, cy, S, S]}`` with S = data.effective_image_size.  The squeeze is addressing inside the library's boundary kernels
    (csd_unet_config.x_squeeze): no squeezed copy of x, and the returned ``'x'`` is a view of the buffer the network wrote."""

    x_squeeze = 1

    @staticmethod
    def _sq_validate(config, name):
        d = config.data
        hi, S, lo = int(d.shape_x[1]), int(d.effective_image_size), int(d.shape_y[1])
        if not (hi == 2 * S == 2 * lo and int(d.shape_x[2]) == hi and int(d.shape_y[2]) == lo):
            raise ValueError('%s: the image side data.shape_x[1] = %d must be twice data.effective_image_size = %d and twice '
                             'data.shape_y[1] = %d (square images)' % (name, hi, S, lo))

    def _split(self, out):
        B, S = out.shape[0], self.image_size
        n = self.x_channels * S * S
        return {'x': out[:, :n].view(self._x_shape(B)), 'y': out[:, n:].view(B, self.out_channels - self.x_channels, S, S)}

    def forward(self, input_dict, labels):
        return self._split(self._run(input_dict['x'], input_dict['y'], labels))


@utils.register_model(name='ddpm_2xSR')
class DDPM_2xSR(_Squeeze2x, _Paired):
    """One 2x stage of the sequential super-resolution cascades (models/ddpm.py:39-52,300-314): the DDPM U-Net behind the squeeze of x
    (_Squeeze2x).  The parameters are the reference ``DDPM_2xSR``'s (the squeeze has none)."""

    def __init__(self, config, precision=None):
        self._sq_validate(config, 'ddpm_2xSR')
        super().__init__(config, precision)

    def _channels(self, config):
        cx = 4 * int(config.data.shape_x[0])
        return cx, int(config.model.input_channels) - cx


class _KxSR:
    """The direct Kx super-resolution wrappers (models/ddpm.py:316-331, models/ncsnpp.py:435-450) over a paired network: with
    S = data.target_resolution and K = data.scale, ``forward({'x': [B, cx, S, S], 'y': [B, cy, S / K, S / K]}, labels) ->
    {'x': [B, cx, S, S], 'y': [B, cy, S / K, S / K]}``: the network sees the bilinear upsample of y and its y output is resized back.
    Both resizes are ``F.interpolate(mode='bilinear', align_corners=False)`` without antialiasing - torchvision's ``Resize`` on tensors
    when the reference was written - and live in the library's boundary kernels (csd_unet_config.y_scale): no upsampled copy of y.
    The low-resolution side is ``target_resolution // scale`` (``data.shape_y`` of the direct configs still names S and only feeds
    sigma_max_y).  No parameters beyond the paired network's."""

    def _kx_validate(self, config, name):
        d = config.data
        S, K = int(d.target_resolution), int(d.scale)
        if not (S == int(d.effective_image_size) == int(d.shape_x[1]) == int(d.shape_x[2])):
            raise ValueError('%s: data.target_resolution = %d, data.effective_image_size = %d and data.shape_x[1:] = %s must name one '
                             'square side' % (name, S, int(d.effective_image_size), list(d.shape_x[1:])))
        if K < 2:
            raise ValueError('%s: data.scale = %d must be at least 2' % (name, K))
        if S % K:
            raise ValueError('%s: data.scale = %d must divide data.target_resolution = %d' % (name, K, S))
        object.__setattr__(self, 'y_scale', K)

    def _split(self, out):
        B, S = out.shape[0], self.image_size
        s, n = S // self.y_scale, self.x_channels * S * S
        return {'x': out[:, :n].view(self._x_shape(B)), 'y': out[:, n:].view(B, self.out_channels - self.x_channels, s, s)}

    def forward(self, input_dict, labels):
        return self._split(self._run(input_dict['x'], input_dict['y'], labels))


@utils.register_model(name='ddpm_KxSR')
class DDPM_KxSR(_KxSR, _Paired):
    """``ddpm_KxSR`` (models/ddpm.py:316-331; configs/ve/srflow/celebAHQ160/direct/8x.py)."""

    def __init__(self, config, precision=None):
        self._kx_validate(config, 'ddpm_KxSR')
        super().__init__(config, precision)
