"""3-D DDPM score networks (reference models/ddpm3D.py:38-196) on the per-operator C ABI.

Registers ``ddpm3D``, ``ddpm3D_paired`` and ``ddpm3D_paired_SR3`` with the reference's constructor / call signatures and the
reference's ``state_dict`` keys and shapes (``all_modules.{i}.{GroupNorm_0,Conv_0,Dense_0,GroupNorm_1,Conv_1,Conv_2}.{weight,bias}``,
conv weights [Cout, Cin, 3, 3, 3]); the parameter-free Downsample / Upsample entries keep their places in the module list, so the indices
are the reference's.  The networks are the DDPM U-Net on nn.Conv3d without attention: 2x2x2 average-pool downsampling, nearest x2
upsampling, a 3x3x3 convolution as the shortcut of every residual block whose channel count changes (``conv_shortcut=True``).

This is an operator-granular executor like ``ncsnpp_ops`` (``_EvalOps3D`` on ``topology.run_unet``, the module list from
``topology.build_modules``): one C-ABI call per layer, channels-last [B, D, H, W, C] inside.  The
NCDHW <-> NDHWC change happens at the boundary only, where the tensors have 1 or 2 channels (a torch copy); everything else is a HIP
kernel: csd_conv3d_block with the GroupNorm affine + activation fused into its staging and bias / time embedding / residual into its
epilogue (the up path's concatenation is virtual: two sources, no copy), csd_groupnorm_scale_shift, csd_avgpool3d_2_ndhwc,
csd_nearest_up2_3d_ndhwc, csd_timestep_embedding, csd_linear, csd_axpby.  There is no PyTorch fallback.  One data movement besides the
boundary is torch's: an up block whose concatenated input is as wide as its ``out_ch`` has no Conv_2, so the concatenated tensor itself
is the residual and is materialised with one ``torch.cat`` (no arithmetic; no reference config has such a ``ch_mult``).

Arithmetic: ``config.model.csd_precision`` / ``$CSD_PRECISION``, 'fp16x3' (default) or 'fp32'.

Refused, with the reason (never a silent fallback):
  ``resamp_with_conv=True``   the reference itself fails there (Upsample builds a 2-D convolution and Downsample pads two of the three
                              dimensions: a conv2d on a 5-D tensor)
  ``conditional=False``       the reference raises NameError (its module list is only created under ``if conditional``)
  an odd extent at a pooled level, precisions other than fp32 / fp16x3 (ValueError)
  training mode and input gradients on CPU tensors (there is no CPU path); the likelihood of the 3-D networks is not provided
By default sampling runs on the step-by-step predictor / corrector loop (``sampling.fused.fusable`` is False for a default model).

The planned path (opt-in: ``config.model.csd_planned = True``, the constructor argument ``planned=True`` or ``$CSD_PLANNED=1``): the model
creates a ``csd_unet`` handle (``csd_unet_config.arch = 2``) for the volume ``config.data.shape_x[1:]`` at construction.  In eval mode
without input gradients ``forward`` is then ONE ``csd_unet_forward``: the weights are packed once (and again when a parameter changes),
every buffer lies at a fixed offset of one workspace, x and y go in separately as NCDHW (no torch ``cat`` / ``permute`` / ``axpby``), the
result is bitwise the operator path's.  ``sampling.fused.fusable`` accepts such a model, so the PC samplers run volumes on the fused
device loop (``csd_pc_sample``).  A forward on another volume raises ValueError (the operator path accepts any volume); construction
refuses what the library refuses (an odd pooled extent of the configured volume, a ``ch_mult`` whose up path has a block without
Conv_2).  Training mode and input gradients keep the autograd executor.  Inpainting, the likelihood and the ODE sampler on the device are not
provided for the 3-D networks.  Making the planned path the default is a separate, later decision.

The planned training graph (opt-in: ``config.model.csd_planned_train = True``, the constructor argument ``planned_train=True`` or
``$CSD_PLANNED_TRAIN=1``; off by default, and then nothing below applies): the model creates the ``arch = 2`` handle (also when ``planned``
is off) and, on GPU tensors, training mode and eval mode with ``x.requires_grad`` are ONE autograd node over csd_unet_train_forward /
csd_unet_backward_acc (``ddpm._PlannedNet`` / ``ddpm._InputGradNet``, csrc/train_graph3d.h) instead of the ``_GradOps3D`` graph: the same
kernels and dropout masks (the same Philox stream ids), activations in a workspace sized by a dry run, every parameter gradient written -
or, in a ``train.Trainer`` accumulation window, added - straight to its ``.grad`` view, gradient-ready marks for ``distributed.GradSync``
(``train_executor == 'planned'``), and ``losses.csd_fused_loss`` on volumes (``_run``).  A volume other than the configured one raises
ValueError.  ``planned`` still decides how eval mode without gradients runs.

Training and input gradients (GPU tensors): in training mode, and in eval mode when ``x.requires_grad`` under autograd, the forward is
the differentiable, operator-granular one (``_GradOps3D``, the same walk): the layers of ResnetBlockDDPM as grad_ops_3d / grad_ops autograd nodes
(GroupNorm + act -> Conv_0 -> + Dense_0(act(temb)) -> GroupNorm + act -> Dropout_0 -> Conv_1, + the shortcut), whose backward passes
are HIP kernels: csd_conv3d_wgrad (split bf16 / fp32), the scale-invariant data gradient on csd_conv3d_block,
csd_groupnorm_act_backward_nhwc, the pooling / upsampling adjoints.  The up path's concatenation is a ``torch.cat`` there (data
movement; autograd splits the gradient), the boundary permutes stay torch.  Dropout masks are a pure function of the Philox key
``dropout_seed`` and the stream id ``_train_calls << 16 | index`` (the scheme of ddpm.py's operator path); dropout is off in eval
mode.  For the paired classes only ``x`` takes a gradient.  The inference forward is not touched by any of this.
"""
import os

import torch
import torch.nn as nn

from .. import _lib, grad_ops_3d, ops
from .._lib import require_gpu_tensor
from . import utils
from .ddpm import _HandleSurface, _InputGradNet, _Node, _PlannedNet, _activation, _fan_avg_uniform, _model_key, _precision
from .topology import Executor, build_modules, run_unet

_PRECISIONS = ('fp32', 'f32', 'fp16x3')


class DDPM3D(nn.Module, _HandleSurface):
    """``ddpm3D`` (models/ddpm3D.py:38-171): model(x [B, C, D, H, W], labels [B]) -> [B, output_channels, D, H, W]."""

    def __init__(self, config, precision=None, planned=None, planned_train=None):
        super().__init__()
        m, d = config.model, config.data
        precision = _precision(config, precision)
        if precision not in _PRECISIONS:
            raise ValueError("the 3-D networks run in 'fp32' or 'fp16x3' (csd_conv3d_block has no %r arithmetic)" % (precision,))
        self.precision = precision
        self.config = config
        self.act = _activation(config)
        if bool(m.resamp_with_conv):
            raise NotImplementedError('ddpm3D: resamp_with_conv=True is not provided - the reference fails there too (its Upsample '
                                      'builds a 2-D convolution, its Downsample pads 2 of the 3 dimensions: conv2d on a 5-D tensor)')
        if not bool(m.conditional):
            raise NotImplementedError('ddpm3D: conditional=False is not provided - the reference raises NameError there (its module '
                                      'list only exists under `if conditional`)')
        self.nf = nf = m.nf
        ch_mult = tuple(m.ch_mult)
        self.num_res_blocks = m.num_res_blocks
        self.num_resolutions = len(ch_mult)
        self.conditional = True
        self.centered = bool(d.centered)
        self.embedding_type = 'positional'
        self.input_channels = m.input_channels
        self.output_channels = m.output_channels
        if nf % 32:
            raise ValueError('ddpm3D: nf = %d is not divisible into the 32 GroupNorm groups' % nf)
        self._dropout = float(_model_key(config, 'dropout', 0.0))
        self._train_calls = 0
        self.dropout_seed = int(getattr(config, 'seed', 0) or 0)   # Philox key of the dropout masks
        self._topology = build_modules('ddpm3d', nf, ch_mult, m.num_res_blocks, self.input_channels, self.output_channels)
        self.all_modules = nn.ModuleList([self._make_node(mod.kind, mod) for mod in self._topology])   # (list order: the RNG's too)
        if planned is None:
            planned = _model_key(config, 'csd_planned', None)
        if planned is None:
            planned = os.environ.get('CSD_PLANNED', '0').strip().lower() not in ('', '0', 'false', 'no', 'off')
        self.planned = bool(planned)
        if planned_train is None:
            planned_train = _model_key(config, 'csd_planned_train', None)
        if planned_train is None:
            planned_train = os.environ.get('CSD_PLANNED_TRAIN', '0').strip().lower() not in ('', '0', 'false', 'no', 'off')
        self.planned_train = bool(planned_train)
        self._h = self._packed = self._packed_key = self._ws = None
        if self.planned or self.planned_train:
            self._create_handle(config)
        if self.planned_train:
            self.train_executor = 'planned'           # (train.Trainer, distributed.GradSync: direct gradient writes, marks, accumulation)

    # ---- the planned path: one csd_unet handle (arch 2) for the configured volume ----
    def _channels(self, config):
        """(x channels, y channels) of the network input"""
        return int(config.model.input_channels), 0

    def _create_handle(self, config):
        m, d = config.model, config.data
        vol = tuple(int(v) for v in d.shape_x[1:])
        if len(vol) != 3:
            raise ValueError('ddpm3D (planned): config.data.shape_x = %s is not [C, D, H, W]' % (list(d.shape_x),))
        for lvl in range(self.num_resolutions - 1):
            if any((e >> lvl) % 2 or (e >> lvl) < 2 for e in vol):
                raise ValueError('ddpm3D (planned): the configured volume %s has an odd extent at level %d, which the 2x2x2 average pool '
                                 'cannot halve' % (vol, lvl))
        self.volume = vol
        self.x_channels, self.y_channels = self._channels(config)
        if self.x_channels + self.y_channels != self.input_channels:
            raise ValueError('ddpm3D (planned): shape_x[0] + shape_y[0] = %d + %d channels, the network takes input_channels = %d'
                             % (self.x_channels, self.y_channels, self.input_channels))
        cfg = _lib.UNetConfig()
        cfg.arch = 2
        cfg.nf = self.nf
        cfg.n_levels = self.num_resolutions
        for i, v in enumerate(m.ch_mult):
            cfg.ch_mult[i] = int(v)
        cfg.num_res_blocks = self.num_res_blocks
        cfg.x_channels, cfg.y_channels, cfg.out_channels = self.x_channels, self.y_channels, int(self.output_channels)
        cfg.resamp_with_conv, cfg.conditional, cfg.centered = 0, 1, int(self.centered)
        cfg.act = _lib.ACT_IDS[self.act]
        cfg.precision = _lib.PREC_IDS[self.precision]
        for i in range(3):
            cfg.vol[i] = vol[i]
        cfg.planned_train = int(self.planned_train)   # (0: the training entries refuse the handle, as they always did)
        self._create_unet(cfg)
        # the library rebuilds the module list from the config: its parameter table must be this module's state_dict
        table = self._param_table()
        if table != [(k, tuple(p.shape)) for k, p in self.named_parameters()]:
            raise RuntimeError('ddpm3D (planned): the library\'s parameter table differs from the module\'s state_dict')
        self._param_names = [k for k, _ in table]

    def _use_plan(self, x):
        """eval mode without input gradients: the planned evaluation; training mode and x.requires_grad keep the autograd executor"""
        want_grad = torch.is_grad_enabled() and x.requires_grad
        return self.planned and not ((self.training and torch.is_grad_enabled()) or want_grad)

    # ---- the planned training graph (``planned_train``): the handle's csd_unet_train_forward / csd_unet_backward* behind ddpm.py's nodes ----
    def _use_train_graph(self, x):
        """training mode, or eval mode with ``x.requires_grad``, under autograd on GPU tensors (CPU tensors keep the existing refusal)"""
        grad = torch.is_grad_enabled() and (self.training or x.requires_grad)
        return self.planned_train and grad and x.is_cuda

    def _x_shape(self, B):
        return (B, self.x_channels) + self.volume

    def _out_shape(self, B):
        return (B, int(self.output_channels)) + self.volume

    def _train_graph_forward(self, x, y, labels):
        """ONE autograd node: ``_PlannedNet`` in training mode (dropout on, every parameter gradient from csd_unet_backward_acc), else
        ``_InputGradNet`` (dropout 0, the data gradient only).  Only x is differentiated (y is the condition)."""
        if y is not None and y.requires_grad:             # (the operator path differentiates through its torch.cat; this node does not)
            raise NotImplementedError('ddpm3D (planned_train): the network differentiates its input x only; y takes no gradient')
        x, y, labels = self._check_planned_io(x, y, labels)
        if self.training:
            self._train_calls += 1
            return _PlannedNet.apply(self, x, y, labels, *self._train_params())
        self._xgrad_calls = getattr(self, '_xgrad_calls', 0) + 1
        return _InputGradNet.apply(self, x, None if y is None else y.detach(), labels.detach(), self._xgrad_calls)

    def _run(self, x, y, labels):
        """the network on separate x and y -> the raw output [B, output_channels, D, H, W] (``losses.csd_fused_loss``), on the handle"""
        if self._h is None:
            raise NotImplementedError('ddpm3D: _run needs the csd_unet handle (planned=True or planned_train=True)')
        if self._use_train_graph(x):
            return self._train_graph_forward(x, y, labels)
        if torch.is_grad_enabled() and (self.training or x.requires_grad):
            raise NotImplementedError('ddpm3D: gradients through _run need planned_train=True and GPU tensors')
        return self._planned_forward(x, y, labels)

    def _check_planned_io(self, x, y, labels):
        """shapes of one call on the handle; returns contiguous float32 x, y (or None), labels"""
        vol = self.volume
        if x.dim() != 5 or x.shape[1] != self.x_channels:
            raise ValueError('ddpm3D: input %s is not [B, %d, D, H, W]' % (tuple(x.shape), self.x_channels))
        if tuple(x.shape[2:]) != vol:
            raise ValueError('ddpm3D (planned): the input volume %s is not the configured volume %s (config.data.shape_x[1:]), for which '
                             'the plan was made; the operator path (csd_planned = False) accepts any volume' % (tuple(x.shape[2:]), vol))
        require_gpu_tensor(x, 'x')
        require_gpu_tensor(labels, 'labels')
        B = x.shape[0]
        if self.y_channels:
            require_gpu_tensor(y, 'y')
            if tuple(y.shape) != (B, self.y_channels) + vol:
                raise ValueError('ddpm3D: y %s is not %s' % (tuple(y.shape), (B, self.y_channels) + vol))
            y = y.float().contiguous()
        else:
            y = None
        labels = labels.to(dtype=torch.float32).contiguous()
        if tuple(labels.shape) != (B,):
            raise ValueError('ddpm3D: labels must have shape [%d]' % B)
        return x.float().contiguous(), y, labels

    def _planned_forward(self, x, y, labels):
        """one csd_unet_forward: x [B, Cx, D, H, W], y [B, Cy, D, H, W] or None -> [B, output_channels, D, H, W]"""
        x, y, labels = self._check_planned_io(x, y, labels)
        return self._unet_forward(x, y, labels, self._out_shape(x.shape[0]))

    # ---- parameters: names, shapes and initialisation of the reference ----
    def _make_node(self, kind, a):
        node = _Node()

        def sub(name, weight, nbias):
            c = _Node()
            c.register_parameter('weight', nn.Parameter(weight))
            c.register_parameter('bias', nn.Parameter(torch.zeros(nbias)))
            node.add_module(name, c)

        if kind == 'linear':
            node.register_parameter('weight', nn.Parameter(_fan_avg_uniform((a.cout, a.cin), 1., False)))
            node.register_parameter('bias', nn.Parameter(torch.zeros(a.cout)))
        elif kind == 'conv':
            node.register_parameter('weight', nn.Parameter(_fan_avg_uniform((a.cout, a.cin, 3, 3, 3), a.init_scale, False)))
            node.register_parameter('bias', nn.Parameter(torch.zeros(a.cout)))
        elif kind == 'gn':
            node.register_parameter('weight', nn.Parameter(torch.ones(a.cin)))
            node.register_parameter('bias', nn.Parameter(torch.zeros(a.cin)))
        elif kind == 'res':                               # ResnetBlockDDPM(dim=3, conv_shortcut=True), models/layers.py:634-656
            cin, cout = a.cin, a.cout
            sub('GroupNorm_0', torch.ones(cin), cin)
            sub('Conv_0', _fan_avg_uniform((cout, cin, 3, 3, 3), 1., False), cout)
            sub('Dense_0', _fan_avg_uniform((cout, self.nf * 4), 1., False), cout)
            sub('GroupNorm_1', torch.ones(cout), cout)
            sub('Conv_1', _fan_avg_uniform((cout, cout, 3, 3, 3), 0., False), cout)
            if cin != cout:
                sub('Conv_2', _fan_avg_uniform((cout, cin, 3, 3, 3), 1., False), cout)
        elif kind not in ('down', 'up'):                  # Downsample / Upsample without a convolution hold no parameter
            raise AssertionError(kind)
        return node

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def _mods(self):
        """the module list as (kind, attributes) pairs"""
        return [(mod.kind, vars(mod)) for mod in self._topology]

    # ---- forward: DDPM3D.forward (models/ddpm3D.py:107-171) ----
    def forward(self, x, labels):
        if self._use_train_graph(x):
            return self._train_graph_forward(x, None, labels)
        if self._use_plan(x) and not (self.training and not x.is_cuda):
            return self._planned_forward(x, None, labels)
        want_grad = torch.is_grad_enabled() and x.requires_grad
        if (self.training or want_grad) and not x.is_cuda:
            if self.training:
                raise NotImplementedError('ddpm3D: training mode is not provided on CPU tensors (the 3-D backward operators are HIP kernels, '
                                          'there is no CPU path); move the model and the batch to the GPU, or call model.eval()')
            raise NotImplementedError('ddpm3D: input gradients are not provided on CPU tensors (the 3-D backward operators are HIP '
                                      'kernels, there is no CPU path)')
        if x.dim() != 5 or x.shape[1] != self.input_channels:
            raise ValueError('ddpm3D: input %s is not [B, %d, D, H, W]' % (tuple(x.shape), self.input_channels))
        ext = tuple(x.shape[2:])
        for lvl in range(self.num_resolutions - 1):
            if any((e >> lvl) % 2 or (e >> lvl) < 2 for e in ext):
                raise ValueError('ddpm3D: volume %s has an odd extent at level %d, which the 2x2x2 average pool cannot halve' % (ext, lvl))
        require_gpu_tensor(x, 'x')
        require_gpu_tensor(labels, 'labels')
        grad = (self.training and torch.is_grad_enabled()) or want_grad
        if grad:
            self._train_calls += 1
        ex = _GradOps3D(self) if grad else _EvalOps3D(self)
        with torch.set_grad_enabled(grad):
            temb = ops.timestep_embedding(labels.contiguous().float(), self.nf)
            h = x.float().permute(0, 2, 3, 4, 1).contiguous()            # NCDHW -> NDHWC (1 or 2 channels)
            if not self.centered:
                h = ex.O.axpby(h, None, alpha=2.0, gamma=-1.0)
            h = run_unet(self._topology, self.all_modules, ex, h, temb)
            return h.permute(0, 4, 1, 2, 3).contiguous()                 # NDHWC -> NCDHW


class _Ops3D(Executor):
    """What the two executors of the 3-D networks share: channels-last activations and the parameter-free resampling.  One object per
    forward: it counts the dropout sites."""

    cdim = -1

    def __init__(self, model):
        self.model, self.p, self.act, self.drops = model, model.precision, model.act, 0

    def downsample(self, node, m, h, temb):
        return self.O.avg_pool3d_2(h)

    def upsample(self, node, m, h, temb):
        return self.O.nearest_up2_3d(h)


class _EvalOps3D(_Ops3D):
    """Executor of ``topology.run_unet`` without autograd: the modules of DDPM3D.forward (models/ddpm3D.py:107-171) on the forward
    operators, every GroupNorm + activation as a per-channel scale / shift in the staging of the convolution behind it"""

    O = ops

    def stem(self, node, m, h):
        return ops.conv3d_block(h, node.weight, node.bias, precision=self.p)

    def res(self, node, m, x0, temb, x1=None):
        """ResnetBlockDDPM.forward (models/layers.py:658-675) on x = x0 (| x1)."""
        p = self.p
        ns, nh = ops.groupnorm_scale_shift(x0, node.GroupNorm_0.weight, node.GroupNorm_0.bias, x1=x1)
        t = ops.linear(temb, node.Dense_0.weight, node.Dense_0.bias, act_in=self.act)
        h = ops.conv3d_block(x0, node.Conv_0.weight, node.Conv_0.bias, x1=x1, nscale=ns, nshift=nh, act=self.act, temb=t, precision=p)
        ns, nh = ops.groupnorm_scale_shift(h, node.GroupNorm_1.weight, node.GroupNorm_1.bias)
        if m.cin != m.cout:
            x = ops.conv3d_block(x0, node.Conv_2.weight, node.Conv_2.bias, x1=x1, precision=p)
        else:
            x = x0 if x1 is None else torch.cat([x0, x1], dim=-1)      # (a concatenated input whose width equals out_ch: a copy)
        return ops.conv3d_block(h, node.Conv_1.weight, node.Conv_1.bias, nscale=ns, nshift=nh, act=self.act, res=x, precision=p)

    def up_block(self, node, m, h, skip, temb):
        return self.res(node, m, h, temb, x1=skip)          # (the concatenation is virtual: two sources)

    def gn(self, node, m, h):
        return (h, *ops.groupnorm_scale_shift(h, node.weight, node.bias))

    def head_conv(self, node, m, h_ns_nh):
        h, ns, nh = h_ns_nh
        return ops.conv3d_block(h, node.weight, node.bias, nscale=ns, nshift=nh, act=self.act, precision=self.p)


class _GradOps3D(_Ops3D):
    """... as autograd nodes (grad_ops_3d / grad_ops), for training mode and for eval mode with ``x.requires_grad``: the same layers and
    the same convolution kernels without the fused prologue (GroupNorm + act is its own node, whose output the weight gradient needs),
    dropout in training mode, ``torch.cat`` for the skips (data movement; autograd splits the gradient).  The Philox stream ids of the
    dropout sites are ``(model._train_calls << 16) + k``, k = 1, 2, ... in module order."""

    O = grad_ops_3d

    def stem(self, node, m, h):
        return self.O.conv3d(h, node.weight, node.bias, self.p)

    head_conv = stem

    def res(self, node, m, h, temb):
        G, act, p, model = self.O, self.act, self.p, self.model
        t = G.groupnorm_act(h, node.GroupNorm_0.weight, node.GroupNorm_0.bias, act=act)
        t = G.conv3d(t, node.Conv_0.weight, node.Conv_0.bias, p)
        t = G.bias_add(t, G.linear(temb, node.Dense_0.weight, node.Dense_0.bias, act_in=act))
        t = G.groupnorm_act(t, node.GroupNorm_1.weight, node.GroupNorm_1.bias, act=act)
        self.drops += 1
        t = G.dropout(t, model._dropout if model.training else 0.0, model.dropout_seed, (model._train_calls << 16) + self.drops)
        t = G.conv3d(t, node.Conv_1.weight, node.Conv_1.bias, p)
        if m.cin != m.cout:
            h = G.conv3d(h, node.Conv_2.weight, node.Conv_2.bias, p)
        return G.axpby(h, t)

    def gn(self, node, m, h):
        return self.O.groupnorm_act(h, node.weight, node.bias, act=self.act)


class _Paired3D(DDPM3D):
    def _channels(self, config):
        return int(config.data.shape_x[0]), int(config.data.shape_y[0])

    def _paired(self, x, y, labels):
        """the network on (x, y): planned, x and y go to the library separately; else the concatenated input on the operator path"""
        if self._use_train_graph(x):
            return self._train_graph_forward(x, y, labels)
        if self._use_plan(x) and not (self.training and not x.is_cuda):
            return self._planned_forward(x, y, labels)
        return DDPM3D.forward(self, torch.cat((x, y), dim=1), labels)


class DDPM3D_paired(_Paired3D):
    """``ddpm3D_paired`` (models/ddpm3D.py:173-184): concatenates x and y, returns both halves."""

    def forward(self, input_dict, labels):
        x, y = input_dict['x'], input_dict['y']
        xc = x.size(1)
        out = self._paired(x, y, labels)
        return {'x': out[:, :xc], 'y': out[:, xc:]}


class DDPM3D_paired_SR3(_Paired3D):
    """``ddpm3D_paired_SR3`` (models/ddpm3D.py:186-196): concatenates x and y, returns the score of x."""

    def forward(self, input_dict, labels):
        return self._paired(input_dict['x'], input_dict['y'], labels)


utils.register_model(DDPM3D, name='ddpm3D')
utils.register_model(DDPM3D_paired, name='ddpm3D_paired')
utils.register_model(DDPM3D_paired_SR3, name='ddpm3D_paired_SR3')
