"""The U-Net of the three families, described once: ``build_modules`` writes the reference's module list as ``Module`` records and
``run_unet`` walks it.  This is the Python counterpart of ``build_modules`` / ``build_modules3d`` in csrc/unet.hip and csrc/unet3d.h
(same roles, same order); ``build_modules`` is the only Python code that knows the order of the network and ``run_unet`` the only one
that keeps a skip stack.  The operator-granular executors (models/ddpm.py, ncsnpp.py, ddpm3d.py) supply the arithmetic: one method
per role, no loop over levels and no running module index."""
from dataclasses import dataclass

import torch


@dataclass
class Module:
    kind: str                 # 'fourier' | 'linear' | 'conv' | 'res' | 'attn' | 'down' | 'up' | 'gn' | 'combine' | 'pyr_down'
    role: str                 # the Role names of csrc/unet.hip, lower case
    level: int
    cin: int                  # attn / down / up / gn: "channels"; combine: the pyramid's (dim1); fourier: embedding size
    cout: int                 # combine: the level's channels (dim2)
    skip: int = 0             # up_block: channels of the skip tensor it pops (its input is h | skip: cin - skip, skip)
    up: bool = False          # BigGAN block: FIR resampling of h and x inside the block
    down: bool = False
    push: bool = False        # its output goes on the skip stack
    init_scale: float = 1.    # 'conv': variance scale of the weight initialisation


def build_modules(family, nf, ch_mult, num_res_blocks, in_channels, out_channels, attn_levels=(), conditional=True, fourier=False,
                  progressive='none', progressive_input='none', init_scale=0.):
    """The module list of ``DDPM.__init__`` (models/ddpm.py:96-147; family 'ddpm'), ``NCSNpp.__init__`` with BigGAN blocks
    (models/ncsnpp.py:44-236; 'ncsnpp') or ``DDPM3D.__init__`` (models/ddpm3D.py:56-105; 'ddpm3d'), in the reference's order.
    ``attn_levels``: the levels whose side is in ``attn_resolutions``.  One U-Net; the families differ in the Fourier entry, in how a
    level is left ('down' / 'up' modules vs. BigGAN down / up blocks), in the middle attention (none in 3-D), in the input pyramid
    behind a downsample and in the output pyramid in front of an upsample."""
    assert family in ('ddpm', 'ncsnpp', 'ddpm3d')
    pp, last = family == 'ncsnpp', len(ch_mult) - 1
    pyr_out = progressive == 'output_skip'
    mods = []

    def add(kind, role, level, cin, cout, **kw):
        mods.append(Module(kind, role, level, cin, cout, **kw))

    if fourier:
        add('fourier', 'emb_fourier', 0, nf, 2 * nf)
    if conditional:
        add('linear', 'emb_linear0', 0, 2 * nf if fourier else nf, 4 * nf)
        add('linear', 'emb_linear1', 0, 4 * nf, 4 * nf)
    add('conv', 'stem', 0, in_channels, nf, push=True)
    hs_c = [nf]                # channels on the skip stack
    in_ch, pyr_ch = nf, in_channels
    for l in range(last + 1):
        for _ in range(num_res_blocks):
            add('res', 'down_block', l, in_ch, nf * ch_mult[l])
            in_ch = nf * ch_mult[l]
            if l in attn_levels:
                add('attn', 'attn', l, in_ch, in_ch)
            mods[-1].push = True
            hs_c.append(in_ch)
        if l != last:
            add('res' if pp else 'down', 'downsample', l, in_ch, in_ch, down=pp)
            if progressive_input == 'input_skip':
                add('combine', 'combine', l + 1, in_channels, in_ch)
            elif progressive_input == 'residual':                          # ncsnpp.py:171-173
                add('pyr_down', 'pyr_down', l, pyr_ch, in_ch)
                pyr_ch = in_ch
            mods[-1].push = True
            hs_c.append(in_ch)
    add('res', 'mid_res_in', last, in_ch, in_ch)
    if family != 'ddpm3d':
        add('attn', 'mid_attn', last, in_ch, in_ch)
    add('res', 'mid_res_out', last, in_ch, in_ch)
    for l in reversed(range(last + 1)):
        for _ in range(num_res_blocks + 1):
            skip = hs_c.pop()
            add('res', 'up_block', l, in_ch + skip, nf * ch_mult[l], skip=skip)
            in_ch = nf * ch_mult[l]
        if l in attn_levels:
            add('attn', 'attn', l, in_ch, in_ch)
        if pyr_out:
            add('gn', 'pyr_gn', l, in_ch, in_ch)
            add('conv', 'pyr_conv', l, in_ch, out_channels, init_scale=init_scale)
        if l != 0:
            add('res' if pp else 'up', 'upsample', l, in_ch, in_ch, up=pp)
    assert not hs_c
    if not pyr_out:
        add('gn', 'head_gn', 0, in_ch, in_ch)
        add('conv', 'head_conv', 0, in_ch, out_channels, init_scale=init_scale)
    return mods


def run_unet(mods, nodes, ex, x, temb):
    """One evaluation of the network ``mods`` (parameters: ``nodes``, one per module) on the executor ``ex``: ``x`` is the network
    input as the stem takes it, ``temb`` what the first embedding module takes (the label, or its positional embedding).  Everything
    that is topology lives here - the skip stack, the input / output pyramid state of NCSN++.  ``ex`` does the arithmetic of one
    module per call, ``ex.<what>(node, module, ...)``: emb_fourier, emb_linear, stem, res, up_block, attn, downsample, upsample,
    combine, pyr_down, gn, pyr_conv, head_conv (the module tells a method its role where two roles share one)."""
    assert len(mods) == len(nodes)
    hs = []
    h, pyr_in, pyr_out = None, x, None
    for m, node in zip(mods, nodes):
        r = m.role
        if r in ('down_block', 'mid_res_out'):
            h = ex.res(node, m, h, temb)
        elif r == 'mid_res_in':                     # reads the top of the stack, which stays
            h = ex.res(node, m, hs[-1], temb)
        elif r == 'up_block':
            h = ex.up_block(node, m, h, hs.pop(), temb)
        elif r in ('attn', 'mid_attn'):
            h = ex.attn(node, m, h)
        elif r in ('downsample', 'upsample'):
            h = getattr(ex, r)(node, m, h, temb)
        elif r == 'stem':
            h = ex.stem(node, m, x)
        elif r == 'combine':                        # 'input_skip': the resampled image joins h; the pyramid stays the image
            pyr_in, h = ex.combine(node, m, pyr_in, h)
        elif r == 'pyr_down':                       # 'residual': the pyramid is the running sum (ncsnpp.py:302-309)
            pyr_in = h = ex.pyr_down(node, m, pyr_in, h)
        elif r == 'pyr_gn':                         # the output pyramid is a side branch: h goes on to the upsample
            ph = ex.gn(node, m, h)
        elif r == 'pyr_conv':
            pyr_out = ex.pyr_conv(node, m, ph, pyr_out)
        elif r == 'head_gn':
            h = ex.gn(node, m, h)
        elif r == 'head_conv':
            h = ex.head_conv(node, m, h)
        elif r == 'emb_fourier':
            temb = ex.emb_fourier(node, m, temb)
        else:
            assert r in ('emb_linear0', 'emb_linear1'), r
            temb = ex.emb_linear(node, m, temb)
        if m.push:
            hs.append(h)
    assert not hs
    return h if pyr_out is None else pyr_out


class Executor:
    """What the operator executors share.  ``O`` is their operator module (ops, grad_ops, ...), ``act`` the activation's name, ``cdim``
    the channel axis of an activation."""

    cdim = 1

    def emb_linear(self, node, m, temb):            # (the second Linear takes act(temb): models/ddpm.py:157-158)
        return self.O.linear(temb, node.weight, node.bias, act_in=self.act if m.role == 'emb_linear1' else 'none')

    def up_block(self, node, m, h, skip, temb):
        return self.res(node, m, torch.cat([h, skip], dim=self.cdim), temb)


