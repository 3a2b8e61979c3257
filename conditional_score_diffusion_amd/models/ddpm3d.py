"""3-D DDPM score networks (reference models/ddpm3D.py:38-196) on the per-operator C ABI.

Registers ``ddpm3D``, ``ddpm3D_paired`` and ``ddpm3D_paired_SR3`` with the reference's constructor / call signatures and the
reference's ``state_dict`` keys and shapes (``all_modules.{i}.{GroupNorm_0,Conv_0,Dense_0,GroupNorm_1,Conv_1,Conv_2}.{weight,bias}``,
conv weights [Cout, Cin, 3, 3, 3]); the parameter-free Downsample / Upsample entries keep their places in the module list, so the indices
are the reference's.  The networks are the DDPM U-Net on nn.Conv3d without attention: 2x2x2 average-pool downsampling, nearest x2
upsampling, a 3x3x3 convolution as the shortcut of every residual block whose channel count changes (``conv_shortcut=True``).

This is an operator-granular executor like ``ncsnpp_ops``: one C-ABI call per layer, channels-last [B, D, H, W, C] inside.  The
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
Conv_2).  Training mode and input gradients keep ``_grad_forward``.  Inpainting, the likelihood and the ODE sampler on the device are not
provided for the 3-D networks.  Making the planned path the default is a separate, later decision.

Training and input gradients (GPU tensors): in training mode, and in eval mode when ``x.requires_grad`` under autograd, the forward is
the differentiable, operator-granular one (``_grad_forward``): the layers of ResnetBlockDDPM as grad_ops_3d / grad_ops autograd nodes
(GroupNorm + act -> Conv_0 -> + Dense_0(act(temb)) -> GroupNorm + act -> Dropout_0 -> Conv_1, + the shortcut), whose backward passes
are HIP kernels: csd_conv3d_wgrad (split bf16 / fp32), the scale-invariant data gradient on csd_conv3d_block,
csd_groupnorm_act_backward_nhwc, the pooling / upsampling adjoints.  The up path's concatenation is a ``torch.cat`` there (data
movement; autograd splits the gradient), the boundary permutes stay torch.  Dropout masks are a pure function of the Philox key
``dropout_seed`` and the stream id ``_train_calls << 16 | index`` (the scheme of ddpm.py's operator path); dropout is off in eval
mode.  For the paired classes only ``x`` takes a gradient.  The inference forward is not touched by any of this.
"""
import ctypes
import os

import torch
import torch.nn as nn

from .. import _lib, ops
from .._lib import check, current_stream, lib, ptr, require_gpu_tensor
from . import utils
from .ddpm import _HandleSurface, _Node, _fan_avg_uniform

_PRECISIONS = ('fp32', 'f32', 'fp16x3')


class DDPM3D(nn.Module, _HandleSurface):
    """``ddpm3D`` (models/ddpm3D.py:38-171): model(x [B, C, D, H, W], labels [B]) -> [B, output_channels, D, H, W]."""

    def __init__(self, config, precision=None, planned=None):
        super().__init__()
        m, d = config.model, config.data
        get = (lambda k, dflt=None: m.get(k, dflt)) if hasattr(m, 'get') else (lambda k, dflt=None: getattr(m, k, dflt))
        if precision is None:
            precision = get('csd_precision') or os.environ.get('CSD_PRECISION', 'fp16x3')
        if precision not in _lib.PREC_IDS:
            raise ValueError('unknown csd precision %r (choose from %s)' % (precision, sorted(_lib.PREC_IDS)))
        if precision not in _PRECISIONS:
            raise ValueError("the 3-D networks run in 'fp32' or 'fp16x3' (csd_conv3d_block has no %r arithmetic)" % (precision,))
        self.precision = precision
        self.config = config
        self.act = m.nonlinearity.lower()
        if self.act not in _lib.ACT_IDS or self.act == 'none':
            raise NotImplementedError('activation function does not exist!')
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
        self._dropout = float(get('dropout', 0.0) or 0.0)
        self._train_calls = 0
        self.dropout_seed = int(getattr(config, 'seed', 0) or 0)   # Philox key of the dropout masks

        # ---- module list, in the order of DDPM3D.__init__ (models/ddpm3D.py:56-105) ----
        mods = [('linear', dict(cin=nf, cout=nf * 4)), ('linear', dict(cin=nf * 4, cout=nf * 4)),
                ('conv', dict(cin=self.input_channels, cout=nf, init_scale=1.))]
        hs_c = [nf]
        in_ch = nf
        for i_level in range(self.num_resolutions):
            for _ in range(self.num_res_blocks):
                out_ch = nf * ch_mult[i_level]
                mods.append(('res', dict(cin=in_ch, cout=out_ch)))
                in_ch = out_ch
                hs_c.append(in_ch)
            if i_level != self.num_resolutions - 1:
                mods.append(('down', {}))
                hs_c.append(in_ch)
        in_ch = hs_c[-1]
        mods.append(('res', dict(cin=in_ch, cout=in_ch)))
        mods.append(('res', dict(cin=in_ch, cout=in_ch)))
        for i_level in reversed(range(self.num_resolutions)):
            for _ in range(self.num_res_blocks + 1):
                out_ch = nf * ch_mult[i_level]
                mods.append(('res', dict(cin=in_ch + hs_c.pop(), cout=out_ch)))
                in_ch = out_ch
            if i_level != 0:
                mods.append(('up', {}))
        assert not hs_c
        mods.append(('gn', dict(c=in_ch)))
        mods.append(('conv', dict(cin=in_ch, cout=self.output_channels, init_scale=0.)))
        self._mods = mods
        self.all_modules = nn.ModuleList([self._make_node(k, a) for k, a in mods])
        if planned is None:
            planned = get('csd_planned')
        if planned is None:
            planned = os.environ.get('CSD_PLANNED', '0').strip().lower() not in ('', '0', 'false', 'no', 'off')
        self.planned = bool(planned)
        self._h = self._packed = self._packed_key = self._ws = None
        if self.planned:
            self._create_handle(config)

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
        self._cfg = cfg
        h = ctypes.c_void_p()
        check(lib().csd_unet_create(ctypes.byref(cfg), ctypes.byref(h)), 'unet_create')
        self._h = h
        # the library rebuilds the module list from the config: its parameter table must be this module's state_dict
        name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 5)()
        table = []
        for i in range(lib().csd_unet_num_params(h)):
            check(lib().csd_unet_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape), 'param_info')
            table.append((name.value.decode(), tuple(shape[j] for j in range(ndim.value))))
        mine = [(k, tuple(p.shape)) for k, p in self.named_parameters()]
        if table != mine:
            raise RuntimeError('ddpm3D (planned): the library\'s parameter table differs from the module\'s state_dict')
        self._param_names = [k for k, _ in table]

    def _use_plan(self, x):
        """eval mode without input gradients: the planned evaluation; training mode and x.requires_grad keep _grad_forward"""
        want_grad = torch.is_grad_enabled() and x.requires_grad
        return self.planned and not ((self.training and torch.is_grad_enabled()) or want_grad)

    def _planned_forward(self, x, y, labels):
        """one csd_unet_forward: x [B, Cx, D, H, W], y [B, Cy, D, H, W] or None -> [B, output_channels, D, H, W]"""
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
            y = y.contiguous()
        labels = labels.contiguous()
        if tuple(labels.shape) != (B,):
            raise ValueError('ddpm3D: labels must have shape [%d]' % B)
        self._ensure_packed()
        ws = self._workspace(B)
        out = ops._out((B, int(self.output_channels)) + vol, torch.float32, x.device)
        check(lib().csd_unet_forward(self._h, ptr(self._packed), ptr(ws), ws.numel(), ptr(x.contiguous()), ptr(y) if self.y_channels else None,
                                     ptr(labels), ptr(out), B, None, 0.0, current_stream(x.device)), 'unet_forward')
        return out

    # ---- parameters: names, shapes and initialisation of the reference ----
    def _make_node(self, kind, a):
        node = _Node()

        def sub(name, weight, nbias):
            c = _Node()
            c.register_parameter('weight', nn.Parameter(weight))
            c.register_parameter('bias', nn.Parameter(torch.zeros(nbias)))
            node.add_module(name, c)

        if kind == 'linear':
            node.register_parameter('weight', nn.Parameter(_fan_avg_uniform((a['cout'], a['cin']), 1., False)))
            node.register_parameter('bias', nn.Parameter(torch.zeros(a['cout'])))
        elif kind == 'conv':
            node.register_parameter('weight', nn.Parameter(_fan_avg_uniform((a['cout'], a['cin'], 3, 3, 3), a['init_scale'], False)))
            node.register_parameter('bias', nn.Parameter(torch.zeros(a['cout'])))
        elif kind == 'gn':
            node.register_parameter('weight', nn.Parameter(torch.ones(a['c'])))
            node.register_parameter('bias', nn.Parameter(torch.zeros(a['c'])))
        elif kind == 'res':                               # ResnetBlockDDPM(dim=3, conv_shortcut=True), models/layers.py:634-656
            cin, cout = a['cin'], a['cout']
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

    # ---- blocks ----
    def _res(self, node, a, x0, x1, temb):
        """ResnetBlockDDPM.forward (models/layers.py:658-675) on x = x0 (| x1)."""
        p = self.precision
        ns, nh = ops.groupnorm_scale_shift(x0, node.GroupNorm_0.weight, node.GroupNorm_0.bias, x1=x1)
        t = ops.linear(temb, node.Dense_0.weight, node.Dense_0.bias, act_in=self.act)
        h = ops.conv3d_block(x0, node.Conv_0.weight, node.Conv_0.bias, x1=x1, nscale=ns, nshift=nh, act=self.act, temb=t, precision=p)
        ns, nh = ops.groupnorm_scale_shift(h, node.GroupNorm_1.weight, node.GroupNorm_1.bias)
        if a['cin'] != a['cout']:
            x = ops.conv3d_block(x0, node.Conv_2.weight, node.Conv_2.bias, x1=x1, precision=p)
        else:
            x = x0 if x1 is None else torch.cat([x0, x1], dim=-1)      # (a concatenated input whose width equals out_ch: a copy)
        return ops.conv3d_block(h, node.Conv_1.weight, node.Conv_1.bias, nscale=ns, nshift=nh, act=self.act, res=x, precision=p)

    # ---- forward: DDPM3D.forward (models/ddpm3D.py:107-171) ----
    def forward(self, x, labels):
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
        mods, nodes = self._mods, self.all_modules
        if (self.training and torch.is_grad_enabled()) or want_grad:
            return self._grad_forward(x, labels)
        with torch.no_grad():
            temb = ops.timestep_embedding(labels.contiguous().float(), self.nf)
            temb = ops.linear(temb, nodes[0].weight, nodes[0].bias)
            temb = ops.linear(temb, nodes[1].weight, nodes[1].bias, act_in=self.act)
            h = x.float().permute(0, 2, 3, 4, 1).contiguous()            # NCDHW -> NDHWC (1 or 2 channels)
            if not self.centered:
                h = ops.axpby(h, None, alpha=2.0, gamma=-1.0)
            i = 2
            hs = [ops.conv3d_block(h, nodes[i].weight, nodes[i].bias, precision=self.precision)]
            i += 1
            for i_level in range(self.num_resolutions):
                for _ in range(self.num_res_blocks):
                    hs.append(self._res(nodes[i], mods[i][1], hs[-1], None, temb))
                    i += 1
                if i_level != self.num_resolutions - 1:
                    hs.append(ops.avg_pool3d_2(hs[-1]))
                    i += 1
            h = hs[-1]
            for _ in range(2):
                h = self._res(nodes[i], mods[i][1], h, None, temb)
                i += 1
            for i_level in reversed(range(self.num_resolutions)):
                for _ in range(self.num_res_blocks + 1):
                    h = self._res(nodes[i], mods[i][1], h, hs.pop(), temb)
                    i += 1
                if i_level != 0:
                    h = ops.nearest_up2_3d(h)
                    i += 1
            assert not hs
            ns, nh = ops.groupnorm_scale_shift(h, nodes[i].weight, nodes[i].bias)
            i += 1
            h = ops.conv3d_block(h, nodes[i].weight, nodes[i].bias, nscale=ns, nshift=nh, act=self.act, precision=self.precision)
            i += 1
            assert i == len(nodes)
            return h.permute(0, 4, 1, 2, 3).contiguous()                 # NDHWC -> NCDHW


    # ---- the differentiable forward: training mode, or eval mode with x.requires_grad ----
    def _grad_forward(self, x, labels):
        """The forward above as autograd nodes (grad_ops_3d / grad_ops): same layers, same kernels for the convolutions (without the
        fused prologue: GroupNorm + act is its own node, whose output the weight gradient needs), dropout in training mode."""
        from .. import grad_ops_3d as G
        mods, nodes, p, act = self._mods, self.all_modules, self.precision, self.act
        drop_p = self._dropout if self.training else 0.0
        self._train_calls += 1
        drop = [0]

        def res(node, a, h, temb):
            t = G.groupnorm_act(h, node.GroupNorm_0.weight, node.GroupNorm_0.bias, act=act)
            t = G.conv3d(t, node.Conv_0.weight, node.Conv_0.bias, p)
            t = G.bias_add(t, G.linear(temb, node.Dense_0.weight, node.Dense_0.bias, act_in=act))
            t = G.groupnorm_act(t, node.GroupNorm_1.weight, node.GroupNorm_1.bias, act=act)
            drop[0] += 1
            t = G.dropout(t, drop_p, self.dropout_seed, (self._train_calls << 16) + drop[0])
            t = G.conv3d(t, node.Conv_1.weight, node.Conv_1.bias, p)
            if a['cin'] != a['cout']:
                h = G.conv3d(h, node.Conv_2.weight, node.Conv_2.bias, p)
            return G.axpby(h, t)

        temb = ops.timestep_embedding(labels.contiguous().float(), self.nf)
        temb = G.linear(temb, nodes[0].weight, nodes[0].bias)
        temb = G.linear(temb, nodes[1].weight, nodes[1].bias, act_in=act)
        h = x.float().permute(0, 2, 3, 4, 1).contiguous()                # NCDHW -> NDHWC (1 or 2 channels)
        if not self.centered:
            h = G.axpby(h, None, alpha=2.0, gamma=-1.0)
        i = 2
        hs = [G.conv3d(h, nodes[i].weight, nodes[i].bias, p)]
        i += 1
        for i_level in range(self.num_resolutions):
            for _ in range(self.num_res_blocks):
                hs.append(res(nodes[i], mods[i][1], hs[-1], temb))
                i += 1
            if i_level != self.num_resolutions - 1:
                hs.append(G.avg_pool3d_2(hs[-1]))
                i += 1
        h = hs[-1]
        for _ in range(2):
            h = res(nodes[i], mods[i][1], h, temb)
            i += 1
        for i_level in reversed(range(self.num_resolutions)):
            for _ in range(self.num_res_blocks + 1):
                h = res(nodes[i], mods[i][1], torch.cat([h, hs.pop()], dim=-1), temb)      # data movement; autograd splits the gradient
                i += 1
            if i_level != 0:
                h = G.nearest_up2_3d(h)
                i += 1
        assert not hs
        h = G.groupnorm_act(h, nodes[i].weight, nodes[i].bias, act=act)
        i += 1
        h = G.conv3d(h, nodes[i].weight, nodes[i].bias, p)
        i += 1
        assert i == len(nodes)
        return h.permute(0, 4, 1, 2, 3).contiguous()                     # NDHWC -> NCDHW


class _Paired3D(DDPM3D):
    def _channels(self, config):
        return int(config.data.shape_x[0]), int(config.data.shape_y[0])

    def _paired(self, x, y, labels):
        """the network on (x, y): planned, x and y go to the library separately; else the concatenated input on the operator path"""
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
