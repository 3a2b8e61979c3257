"""Seeded parity cases of the DDPM family on images with more than 8 channels, shared by tools/make_wide_goldens.py (which runs the
imported reference on them) and the tests (tests/test_wide_host.py, tests/test_gpu_wide.py).  Inputs, labels and noise tapes are
regenerated from seeds on either side, the parameters come from score_oracle.synth_params(shapes, 0); tests/golden/wide_channels.npz
holds the reference's outputs only.

    case  model            channels        size  nf  ch_mult    attention  what it exercises
    W1    ddpm_paired      16 + 16 -> 32   16    32  (1, 2)     (8,)       two full 16-channel K groups, a 32-channel head, y + sigma z on 16 channels
    W1c   as W1 with data.centered = True
    W2    ddpm             12              16    32  (1, 1, 2)  -          pad 12 -> 16, unconditional (inpainting, likelihood)
    W3    ddpm_paired_SR3  6 + 3 -> 6      20    32  (1, 2)     (10,)      just over the old limit; 20 is no multiple of 16
    W4    ddpm_paired      5 + 12 -> 17    24    32  (1, 2)     -          pad 17 -> 32, the x | y boundary inside a 16-channel group
    W5    ddpm_paired_SR3  16 + 16 -> 16   16    64  (1, 2)     -          nf 64 at 32 padded channels: the plan keeps assemble + generic convolution
    W6    ddpm             12              32    64  (1, 2)     -          nf 64: the fused wide first layer (stem_wide_kernel) in the plan, 8 tiles per sample

All with one residual block per level and B = 2.  W5 / W6 exist because the fused first layer needs nf % 64 == 0 (or % 96): at nf 32
the plan runs the assemble pass at the padded width and the generic convolution, which W1 - W4 cover.  The wide kernel at 32 padded
channels is reached through ops.input_conv (tests/test_gpu_wide.py: the first layer as an operator).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'oracle')) if p not in sys.path]
import cases  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'wide_channels.npz')
B = 2

CASES = {
    # name: (model, x channels, y channels, image size, nf, ch_mult, attention resolutions, centered)
    'W1': ('ddpm_paired', 16, 16, 16, 32, (1, 2), (8,), False),
    'W1c': ('ddpm_paired', 16, 16, 16, 32, (1, 2), (8,), True),
    'W2': ('ddpm', 12, 0, 16, 32, (1, 1, 2), (), False),
    'W3': ('ddpm_paired_SR3', 6, 3, 20, 32, (1, 2), (10,), False),
    'W4': ('ddpm_paired', 5, 12, 24, 32, (1, 2), (), False),
    'W5': ('ddpm_paired_SR3', 16, 16, 16, 64, (1, 2), (), False),
    'W6': ('ddpm', 12, 0, 32, 64, (1, 2), (), False),
}
ISSUE_CASES = ['W1', 'W2', 'W3', 'W4']            # the four shapes every layer is tested on
FORWARD_TIMES = [1.0, 1e-5]                       # both ends of the noise schedule
ONE_TIME_CASES = ['W1c', 'W5', 'W6']             # the fixture holds their network output at FORWARD_TIMES[0] only (the file stays small)
P_STEPS = 3
SAMPLER_CASES = ['W1', 'W3']                      # W1: the two-SDE VE pair (y + sigma z on 16 channels), W3: cVESDE
TRAIN_CASES = ['W1', 'W3']
INPAINT_N = 6                                     # VESDE steps of the inpainting run on W2
# sigma_max_x is the reference configs' sqrt(prod(shape_x)) (cases.make_config); the Haar mask: the first three channels are known
HAAR_KNOWN = 3


def make_config(case, precision=None):
    name, xc, yc, S, nf, ch_mult, attn, centered = CASES[case]
    cfg = cases.make_config(name=name, nf=nf, ch_mult=ch_mult, num_res_blocks=1, attn_resolutions=attn, image_size=S, x_ch=xc,
                            y_ch=yc if yc else xc)
    if name == 'ddpm':
        cfg.data.num_channels = xc
    cfg.data.centered = centered
    if precision is not None:
        cfg.model.csd_precision = precision
    return cfg


def case_y(case):
    """the condition image in [0, 1): a uniform draw with a zeroed square, as cases.case_y makes it for the paired networks"""
    name, xc, yc, S, nf, ch_mult, attn, centered = CASES[case]
    if not yc:
        return None
    rs = np.random.RandomState(123)
    y = rs.uniform(0, 1, size=(B, yc, S, S)).astype(np.float32)
    y[:, :, S // 4:S // 4 + S // 2, S // 4:S // 4 + S // 2] = 0.
    return torch.from_numpy(y)


def forward_inputs(case):
    """[(x, t)] for FORWARD_TIMES: x = sigma(t) N(0, 1) + 0.5, the draws of oracle/make_goldens.py:gen_network_case"""
    cfg = make_config(case)
    m = cfg.model
    rs = np.random.RandomState(7)
    xs = (B,) + tuple(cfg.data.shape_x)
    out = []
    for tval in FORWARD_TIMES:
        sig = float(m.sigma_min_x * (m.sigma_max_x / m.sigma_min_x) ** tval)
        out.append((torch.from_numpy((rs.standard_normal(xs) * sig + 0.5).astype(np.float32)), torch.ones(B) * tval))
    return out


def pc_tape(case, p_steps=P_STEPS):
    """the normals of a PC run in draw order: the prior, then per step and phase (corrector, predictor) [z_y of the two-SDE pair,] z_x"""
    cfg = make_config(case)
    xs, ys = (B,) + tuple(cfg.data.shape_x), (B,) + tuple(cfg.data.shape_y)
    per_phase = [ys, xs] if cfg.model.name == 'ddpm_paired' else [xs]
    return cases.tape([xs] + (per_phase + per_phase) * p_steps)


def inpaint_inputs():
    """W2 with the Haar channel mask [1, 12, 1, 1] = (1, 1, 1, 0, ..., 0): data in [0, 1), the mask, the tape (prior + 4 draws per step)"""
    cfg = make_config('W2')
    S, C = cfg.data.image_size, CASES['W2'][1]
    rs = np.random.RandomState(77)
    data = torch.from_numpy(rs.uniform(0, 1, size=(B, C, S, S)).astype(np.float32))
    mask = torch.zeros(1, C, 1, 1)
    mask[:, :HAAR_KNOWN] = 1.
    return cfg, data, mask, cases.tape([(B, C, S, S)] * (1 + 4 * INPAINT_N), 23)


def grad_inputs(case):
    """the training-loss inputs (cases.grad_case's recipe): config with dropout off, data batch in [0, 1), fixed times, the loss's tape"""
    cfg = make_config(case)
    cfg.model.dropout = 0.0
    rs = np.random.RandomState(11)
    xs, ys = (B,) + tuple(cfg.data.shape_x), (B,) + tuple(cfg.data.shape_y)
    x = torch.from_numpy(rs.uniform(0, 1, size=xs).astype(np.float32))
    t = torch.tensor([0.83, 0.21][:B])
    shapes = [ys, xs] if cfg.model.name == 'ddpm_paired' else [xs]
    return cfg, x, case_y(case), t, cases.tape(shapes, 3)


def dx_inputs(case):
    """eval-mode input gradient: x in [0, 1), labels, and the cotangent w of the scalar (out * w).sum()"""
    cfg = make_config(case)
    rs = np.random.RandomState(7)
    x = torch.from_numpy(rs.uniform(0, 1, size=(B,) + tuple(cfg.data.shape_x)).astype(np.float32))
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((B, cfg.model.output_channels) + tuple(x.shape[2:])).astype(np.float32))
    return cfg, x, case_y(case), torch.tensor([12.25, 871.0][:B]), w


def params(cfg, seed=0):
    import score_oracle as so
    return so.synth_params(so.ddpm_param_shapes(so.NetCfg.from_config(cfg)), seed)


def call(model, cfg, x, y, labels):
    """model output as one tensor (the paired network's two halves concatenated back)"""
    if cfg.model.name == 'ddpm':
        return model(x, labels)
    out = model({'x': x, 'y': y}, labels)
    return torch.cat([out['x'], out['y']], dim=1) if isinstance(out, dict) else out


def golden():
    return np.load(GOLDEN)


# ---- float64 restatement of the forward (models/ddpm.py:149-213 behind the wrappers of :275-298), from the state_dict alone.  `mangle`
# restates it WRONGLY on purpose, for the sensitivity checks of tests/test_wide_host.py:
#   'swap'  the x and y channel blocks of the assembled input change places
#   'drop'  the assembled channels from 8 on are zero (what a build that kept the 8-channel input width would see)
#   'pad'   the channels that pad the input to the next multiple of 16 hold ones and meet weights (the mean of the real weights of their
#           cout and tap) instead of zeros - what reading the padding of the input and of the packed weight as data would give ----
def forward64(p, cfg, x, y, labels, mangle=None):
    m = cfg.model
    nf, ch_mult, attn_res, S = m.nf, tuple(m.ch_mult), tuple(m.attn_resolutions), cfg.data.image_size
    p = {k: v.double() for k, v in p.items()}
    xc = x.shape[1]
    h = (torch.cat([x, y], dim=1) if y is not None else x).double()
    if not cfg.data.centered:
        h = 2 * h - 1.
    w0, b0 = p['all_modules.2.weight'], p['all_modules.2.bias']
    if mangle == 'swap':
        h = torch.cat([h[:, xc:], h[:, :xc]], dim=1) if y is not None else torch.flip(h, dims=[1])
    elif mangle == 'drop':
        h = h.clone()
        h[:, 8:] = 0.
    elif mangle == 'pad':
        c = h.shape[1]
        npad = (c + 15) // 16 * 16 - c
        npad = npad if npad else 16                # (a full group: the next 16 channels of a wider read)
        h = torch.cat([h, torch.ones(h.shape[0], npad, S, S, dtype=h.dtype)], dim=1)
        w0 = torch.cat([w0, w0.mean(dim=1, keepdim=True).expand(-1, npad, -1, -1)], dim=1)
    else:
        assert mangle is None, mangle

    def P(i, s):
        return p['all_modules.%d.%s' % (i, s)]

    def gn(i, s, v):
        pre = s + '.' if s else ''
        return F.group_norm(v, 32, P(i, pre + 'weight'), P(i, pre + 'bias'), eps=1e-6)

    def nin(i, s, v):
        return torch.einsum('bchw,co->bohw', v, P(i, s + '.W')) + P(i, s + '.b')[None, :, None, None]

    def res(i, v, temb):
        t = F.silu(gn(i, 'GroupNorm_0', v))
        t = F.conv2d(t, P(i, 'Conv_0.weight'), P(i, 'Conv_0.bias'), padding=1)
        t = t + F.linear(F.silu(temb), P(i, 'Dense_0.weight'), P(i, 'Dense_0.bias'))[:, :, None, None]
        t = F.conv2d(F.silu(gn(i, 'GroupNorm_1', t)), P(i, 'Conv_1.weight'), P(i, 'Conv_1.bias'), padding=1)
        if ('all_modules.%d.NIN_0.W' % i) in p:
            v = nin(i, 'NIN_0', v)
        return v + t

    def attn(i, v):
        Bq, C, H, W = v.shape
        t = gn(i, 'GroupNorm_0', v)
        q, k, vv = nin(i, 'NIN_0', t), nin(i, 'NIN_1', t), nin(i, 'NIN_2', t)
        w = torch.einsum('bchw,bcij->bhwij', q, k) * (int(C) ** (-0.5))
        w = F.softmax(w.reshape(Bq, H, W, H * W), dim=-1).reshape(Bq, H, W, H, W)
        t = torch.einsum('bhwij,bcij->bchw', w, vv)
        return v + nin(i, 'NIN_3', t)

    half = nf // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float64) * -(np.log(10000.0) / (half - 1)))
    e = labels.double()[:, None] * freq[None, :]
    temb = torch.cat([torch.sin(e), torch.cos(e)], dim=1)
    temb = F.linear(temb, P(0, 'weight'), P(0, 'bias'))
    temb = F.linear(F.silu(temb), P(1, 'weight'), P(1, 'bias'))
    i = 2
    hs = [F.conv2d(h, w0, b0, padding=1)]
    i += 1
    L = len(ch_mult)
    for lvl in range(L):
        hh = res(i, hs[-1], temb)
        i += 1
        if (S >> lvl) in attn_res:
            hh = attn(i, hh)
            i += 1
        hs.append(hh)
        if lvl != L - 1:
            hs.append(F.conv2d(F.pad(hs[-1], (0, 1, 0, 1)), P(i, 'Conv_0.weight'), P(i, 'Conv_0.bias'), stride=2))
            i += 1
    h = res(i, hs[-1], temb)
    h = attn(i + 1, h)
    h = res(i + 2, h, temb)
    i += 3
    for lvl in reversed(range(L)):
        for _ in range(2):
            h = res(i, torch.cat([h, hs.pop()], dim=1), temb)
            i += 1
        if (S >> lvl) in attn_res:
            h = attn(i, h)
            i += 1
        if lvl != 0:
            h = F.interpolate(h, scale_factor=2, mode='nearest')
            h = F.conv2d(h, P(i, 'Conv_0.weight'), P(i, 'Conv_0.bias'), padding=1)
            i += 1
    assert not hs
    h = F.silu(gn(i, '', h))
    return F.conv2d(h, P(i + 1, 'weight'), P(i + 1, 'bias'), padding=1)
