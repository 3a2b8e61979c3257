"""Seeded parity cases of the 2x super-resolution networks (ddpm_2xSR: the DDPM U-Net behind a space-to-depth squeeze of x), shared by
tools/make_sr_goldens.py (which runs the imported reference on them) and the tests (tests/test_sr_host.py, tests/test_gpu_sr.py).
Inputs, labels and noise tapes are regenerated from seeds on either side, the parameters come from score_oracle.synth_params(shapes, 0);
tests/golden/sr2x.npz holds the reference's outputs only.

    case  image x      network          nf  ch_mult  attention  first-layer route (csrc/stem.hip: stem_supported / stem_planned)
    R1    3 x 32 x 32  12 + 3 at 16^2   32  (1, 2)   (8,)       assemble pass + generic convolution (nf 32)
    R2    3 x 64 x 64  12 + 3 at 32^2   64  (1, 2)   -          stem_wide_kernel, 16 padded channels, several tiles per sample
    R3    1 x 32 x 32  4 + 1 at 16^2    64  (1, 2)   -          stem_kernel (<= 8 channels)
    R4    1 x 40 x 40  4 + 1 at 20^2    32  (1, 2)   (10,)      20 is no multiple of 16 (no fused layer); data.centered = True

All with one residual block per level and B = 2; each is the smallest shape that reaches its route.  The channel order of the squeeze is
models/ddpm.py:39-52's: x'[b, 4c + 2dy + dx, i, j] = x[b, c, 2i + dy, 2j + dx].
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')) if p not in sys.path]
import cases  # noqa: E402
import wide_cases as wc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'sr2x.npz')
B = 2

CASES = {
    # name: (image channels of x, channels of y, S = side of y and of the network, nf, ch_mult, attention resolutions, centered)
    'R1': (3, 3, 16, 32, (1, 2), (8,), False),
    'R2': (3, 3, 32, 64, (1, 2), (), False),
    'R3': (1, 1, 16, 64, (1, 2), (), False),
    'R4': (1, 1, 20, 32, (1, 2), (10,), True),
}
FORWARD_TIMES = [1.0, 1e-5]                       # both ends of the noise schedule
P_STEPS = 3
SAMPLER_CASES = ['R1', 'R3']
PATH_CASE = 'R1'                                  # use_path: the bridge for y_t
TRAIN_CASE = 'R1'
ORDERS = ('ref', 'swap', 'cmajor')                # squeeze orders: the reference's, dy and dx swapped, 4 * (2dy + dx) + c


def make_config(case, precision=None, name='ddpm_2xSR'):
    """a reference-style config of one 2x stage (configs/ve/srflow/celebAHQ160/sequential/bicubic/config_160.py:81-87,103-104,140-141):
    image_size is the high-resolution side, effective_image_size the side the network runs at.  ``name='ddpm_paired'``: the same
    network WITHOUT the squeeze, on a pre-squeezed x [B, 4c, S, S] (the twin of the addressing tests and of forward64)."""
    cx, cy, S, nf, ch_mult, attn, centered = CASES[case]
    cfg = cases.make_config(name=name, nf=nf, ch_mult=ch_mult, num_res_blocks=1, attn_resolutions=attn, image_size=S, x_ch=4 * cx, y_ch=cy)
    d, m = cfg.data, cfg.model
    d.centered = centered
    d.num_channels = 4 * cx + cy
    m.input_channels = m.output_channels = d.num_channels
    if name == 'ddpm_2xSR':
        d.image_size = 2 * S
        d.effective_image_size = S
        d.shape_x = [cx, 2 * S, 2 * S]
        d.shape_y = [cy, S, S]
    # (both names: sigma_max of the IMAGE shapes, as the reference configs set them)
    m.sigma_max_x = m.sigma_max = float(np.sqrt(4 * cx * S * S))
    m.sigma_max_y = float(np.sqrt(cy * S * S))
    if precision is not None:
        m.csd_precision = precision
    return cfg


def squeeze(x, order='ref'):
    """[B, C, 2S, 2S] -> [B, 4C, S, S]; 'ref' is SqueezeBlock.forward, the others are wrong on purpose (tests/test_sr_host.py)"""
    Bq, C, H, W = x.shape
    z = x.reshape(Bq, C, H // 2, 2, W // 2, 2)                  # b, c, i, dy, j, dx
    perm = {'ref': (0, 1, 3, 5, 2, 4), 'swap': (0, 1, 5, 3, 2, 4), 'cmajor': (0, 3, 5, 1, 2, 4)}[order]
    return z.permute(*perm).reshape(Bq, 4 * C, H // 2, W // 2)


def unsqueeze(z, order='ref'):
    """the inverse of squeeze(., order): [B, 4C, S, S] -> [B, C, 2S, 2S]"""
    Bq, C4, H, W = z.shape
    C = C4 // 4
    if order == 'ref':
        v = z.reshape(Bq, C, 2, 2, H, W).permute(0, 1, 4, 2, 5, 3)          # b, c, dy, dx, i, j -> b, c, i, dy, j, dx
    elif order == 'swap':
        v = z.reshape(Bq, C, 2, 2, H, W).permute(0, 1, 4, 3, 5, 2)          # b, c, dx, dy, i, j
    else:
        v = z.reshape(Bq, 2, 2, C, H, W).permute(0, 3, 4, 1, 5, 2)          # b, dy, dx, c, i, j
    return v.reshape(Bq, C, 2 * H, 2 * W)


def case_y(case):
    """the low-resolution condition in [0, 1): a uniform draw with a zeroed square (wide_cases.case_y's recipe)"""
    cx, cy, S = CASES[case][:3]
    rs = np.random.RandomState(123)
    y = rs.uniform(0, 1, size=(B, cy, S, S)).astype(np.float32)
    y[:, :, S // 4:S // 4 + S // 2, S // 4:S // 4 + S // 2] = 0.
    return torch.from_numpy(y)


def forward_inputs(case):
    """[(x, t)] for FORWARD_TIMES: the image x = sigma(t) N(0, 1) + 0.5"""
    cfg = make_config(case)
    m = cfg.model
    rs = np.random.RandomState(7)
    xs = (B,) + tuple(cfg.data.shape_x)
    out = []
    for tval in FORWARD_TIMES:
        sig = float(m.sigma_min_x * (m.sigma_max_x / m.sigma_min_x) ** tval)
        out.append((torch.from_numpy((rs.standard_normal(xs) * sig + 0.5).astype(np.float32)), torch.ones(B) * tval))
    return out


def labels_of(cfg, t):
    return t * (cfg.model.num_scales - 1)


def shapes(case):
    cfg = make_config(case)
    return (B,) + tuple(cfg.data.shape_x), (B,) + tuple(cfg.data.shape_y)


def pc_tape(case, p_steps=P_STEPS):
    """the normals of a two-SDE PC run in draw order: the prior, then per step and phase (corrector, predictor) z_y at S^2, z_x at (2S)^2"""
    xs, ys = shapes(case)
    return cases.tape([xs] + [ys, xs, ys, xs] * p_steps)


def path_tape(case, p_steps=P_STEPS):
    """use_path: the prior, z of y_{T + tau}; per step the bridge's z_y, the predictor's z_x, the corrector's z_x"""
    xs, ys = shapes(case)
    return cases.tape([xs, ys] + [ys, xs, xs] * p_steps, seed=7)


def grad_inputs(case):
    """the training-loss inputs (cases.grad_case's recipe): config with dropout off, image batch in [0, 1), fixed times, the loss's tape"""
    cfg = make_config(case)
    cfg.model.dropout = 0.0
    rs = np.random.RandomState(11)
    xs, ys = shapes(case)
    x = torch.from_numpy(rs.uniform(0, 1, size=xs).astype(np.float32))
    return cfg, x, case_y(case), torch.tensor([0.83, 0.21][:B]), cases.tape([ys, xs], 3)


def dx_inputs(case):
    """eval-mode input gradient: the image x in [0, 1), labels, and the cotangents (w_x, w_y) of (out_x * w_x).sum() + (out_y * w_y).sum()"""
    cfg = make_config(case)
    xs, ys = shapes(case)
    x = torch.from_numpy(np.random.RandomState(7).uniform(0, 1, size=xs).astype(np.float32))
    rs = np.random.RandomState(3)
    wx = torch.from_numpy(rs.standard_normal(xs).astype(np.float32))
    wy = torch.from_numpy(rs.standard_normal(ys).astype(np.float32))
    return cfg, x, case_y(case), torch.tensor([12.25, 871.0][:B]), wx, wy


def params(cfg, seed=0):
    return wc.params(cfg, seed)


def golden():
    return np.load(GOLDEN)


def forward64(p, case, x, y, labels, order='ref'):
    """float64 restatement of DDPM_2xSR.forward: wide_cases.forward64 (the DDPM U-Net) behind squeeze / unsqueeze -> (out_x, out_y)"""
    cfg = make_config(case, name='ddpm_paired')
    cx = 4 * CASES[case][0]
    out = wc.forward64(p, cfg, squeeze(x, order), y, labels)
    return unsqueeze(out[:, :cx], order), out[:, cx:]
