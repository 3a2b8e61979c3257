"""Seeded parity cases of the direct Kx super-resolution networks (ddpm_KxSR, ncsnpp_KxSR: a paired network behind the bilinear upsample
of the low-resolution y, its y output resized back), shared by tools/make_kxsr_goldens.py (which runs the imported reference on them) and
the tests (tests/test_kxsr_host.py, tests/test_gpu_kxsr.py).  Inputs, labels and noise tapes are regenerated from seeds on either side,
the parameters come from score_oracle.synth_params / cases.ncsnpp_params; tests/golden/kxsr.npz holds the reference's outputs only.

    case  class        x            y          K  nf  ch_mult  attention  why
    K1    ddpm_KxSR    3 x 16 x 16  3 x 4 x 4  4  32  (1, 2)   (8,)       assemble pass + generic convolution
    K2    ddpm_KxSR    3 x 32 x 32  3 x 4 x 4  8  64  (1, 2)   -          nf 64 (the shape the fused first layer takes for ddpm_paired), several
                                                                          tiles per sample, a K x K block wider than a 16-pixel tile
    K3    ddpm_KxSR    1 x 24 x 24  1 x 8 x 8  3  32  (1, 2)   -          odd K; 24 is no multiple of 16; data.centered = True
    K4    ncsnpp_KxSR  3 x 16 x 16  3 x 8 x 8  2  32  (1, 2)   (8,)       arch 1 with the embedding / progressive options of
                                                                          configs/ve/srflow/DF2K/direct/4x.py (fourier, output_skip, input_skip)

All with one residual block per level and B = 2.  Both resizes are F.interpolate(mode='bilinear', align_corners=False) WITHOUT
antialiasing: what torchvision's Resize did on tensors when the reference was written (tools/make_kxsr_goldens.py installs exactly that
as its torchvision stand-in).  As in the reference's direct configs, data.shape_y names S; the low-resolution side is
target_resolution // scale.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')) if p not in sys.path]
import cases  # noqa: E402
import wide_cases as wc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kxsr.npz')
B = 2

CASES = {
    # name: (class, channels of x, channels of y, S, K, nf, ch_mult, attention resolutions, centered)
    'K1': ('ddpm_KxSR', 3, 3, 16, 4, 32, (1, 2), (8,), False),
    'K2': ('ddpm_KxSR', 3, 3, 32, 8, 64, (1, 2), (), False),
    'K3': ('ddpm_KxSR', 1, 1, 24, 3, 32, (1, 2), (), True),
    'K4': ('ncsnpp_KxSR', 3, 3, 16, 2, 32, (1, 2), (8,), False),
}
TWIN = {'ddpm_KxSR': 'ddpm_paired', 'ncsnpp_KxSR': 'ncsnpp_paired'}
FORWARD_TIMES = [1.0, 1e-5]                       # both ends of the noise schedule
P_STEPS = 3
SAMPLER_CASES = ['K1', 'K4']
PATH_CASE = 'K1'                                  # use_path: the bridge for y_t
TRAIN_CASE = 'K1'
RESIZES = ('ref', 'corners', 'nearest')           # the reference's resize, align_corners=True, nearest (wrong on purpose)


def make_config(case, precision=None, twin=False):
    """a reference-style config of a direct Kx network (configs/ve/srflow/celebAHQ160/direct/8x.py, DF2K/direct/4x.py).  ``twin``: the
    paired network WITHOUT the resizes, on a pre-upsampled y [B, cy, S, S] (the twin of the bitwise tests and of forward64)."""
    name, cx, cy, S, K, nf, ch_mult, attn, centered = CASES[case]
    if name == 'ddpm_KxSR':
        cfg = cases.make_config(name=TWIN[name] if twin else name, nf=nf, ch_mult=ch_mult, num_res_blocks=1, attn_resolutions=attn,
                                image_size=S, x_ch=cx, y_ch=cy)
        cfg.model.input_channels = cfg.model.output_channels = cx + cy
        cfg.training.conditioning_approach = 'ours_NDV'
    else:
        cfg = cases.make_ncsnpp_config(name=TWIN[name] if twin else name, nf=nf, ch_mult=ch_mult, num_res_blocks=1, attn_resolutions=attn,
                                       image_size=S, channels=cx + cy)
        cfg.training.likelihood_weighting = cfg.training.reduce_mean = True
        cfg.sampling.predictor, cfg.sampling.corrector, cfg.sampling.snr = 'conditional_reverse_diffusion', 'conditional_langevin', 0.15
        cfg.data.shape_x, cfg.data.shape_y = [cx, S, S], [cy, S, S]
        m = cfg.model
        m.sigma_min_x = m.sigma_min_y = m.sigma_min = 5e-3
        m.sigma_max_x = m.sigma_max = float(np.sqrt(cx * S * S))
        m.sigma_max_y = 1.0
        m.input_channels = m.output_channels = cx + cy
        cfg.optim = cases.make_config().optim
        cfg.seed = 42
    d = cfg.data
    d.centered = centered
    d.target_resolution = S
    d.scale = K
    if precision is not None:
        cfg.model.csd_precision = precision
    return cfg


def low_side(case):
    return CASES[case][3] // CASES[case][4]


def shapes(case):
    """(shape of x, shape of the low-resolution y), with the batch"""
    name, cx, cy, S, K = CASES[case][:5]
    return (B, cx, S, S), (B, cy, S // K, S // K)


def resize(v, size, how='ref'):
    """the reference's Resize(size, BILINEAR) on a tensor: torch's bilinear resize, align_corners=False, no antialias; 'corners' and
    'nearest' are wrong on purpose (tests/test_kxsr_host.py)"""
    if how == 'nearest':
        return F.interpolate(v, size=(size, size), mode='nearest')
    return F.interpolate(v, size=(size, size), mode='bilinear', align_corners=(how == 'corners'))


def case_y(case):
    """the low-resolution condition in [0, 1): a uniform draw with a zeroed square (wide_cases.case_y's recipe)"""
    ys = shapes(case)[1]
    s = ys[-1]
    y = np.random.RandomState(123).uniform(0, 1, size=ys).astype(np.float32)
    y[:, :, s // 4:s // 4 + s // 2, s // 4:s // 4 + s // 2] = 0.
    return torch.from_numpy(y)


def forward_inputs(case):
    """[(x, t)] for FORWARD_TIMES: x = sigma(t) N(0, 1) + 0.5"""
    m = make_config(case).model
    rs = np.random.RandomState(7)
    xs = shapes(case)[0]
    out = []
    for tval in FORWARD_TIMES:
        sig = float(m.sigma_min_x * (m.sigma_max_x / m.sigma_min_x) ** tval)
        out.append((torch.from_numpy((rs.standard_normal(xs) * sig + 0.5).astype(np.float32)), torch.ones(B) * tval))
    return out


def labels_of(cfg, t):
    return t * (cfg.model.num_scales - 1)


def score_inputs(case):
    """the two-SDE score function's inputs: x_t, a perturbed low-resolution y_t, t in (0, 1)"""
    xs, ys = shapes(case)
    rs = np.random.RandomState(17)
    x = torch.from_numpy((rs.standard_normal(xs) * 2.0 + 0.5).astype(np.float32))
    y = case_y(case) + torch.from_numpy((rs.standard_normal(ys) * 0.3).astype(np.float32))
    return x, y, torch.tensor([0.71, 0.13][:B])


def pc_tape(case, p_steps=P_STEPS):
    """the normals of a two-SDE PC run in draw order: the prior, then per step and phase (corrector, predictor) z_y at (S / K)^2, z_x at S^2"""
    xs, ys = shapes(case)
    return cases.tape([xs] + [ys, xs, ys, xs] * p_steps)


def path_tape(case, p_steps=P_STEPS):
    """use_path: the prior, z of y_{T + tau}; per step the bridge's z_y, the predictor's z_x, the corrector's z_x"""
    xs, ys = shapes(case)
    return cases.tape([xs, ys] + [ys, xs, xs] * p_steps, seed=7)


def tape_floats(case, p_steps=P_STEPS, use_path=False):
    """elements the fused loop reads from a tape behind the prior: x draws at S^2 per channel, y draws at (S / K)^2"""
    xs, ys = shapes(case)
    nx, ny = int(np.prod(xs)), int(np.prod(ys))
    return ny + p_steps * (ny + 2 * nx) if use_path else p_steps * 2 * (ny + nx)


def grad_inputs(case):
    """the training-loss inputs (cases.grad_case's recipe): config with dropout off, x in [0, 1), fixed times, the loss's tape"""
    cfg = make_config(case)
    cfg.model.dropout = 0.0
    xs, ys = shapes(case)
    x = torch.from_numpy(np.random.RandomState(11).uniform(0, 1, size=xs).astype(np.float32))
    return cfg, x, case_y(case), torch.tensor([0.83, 0.21][:B]), cases.tape([ys, xs], 3)


def dx_inputs(case):
    """eval-mode input gradient: x in [0, 1), labels, and the cotangents (w_x, w_y) of (out_x * w_x).sum() + (out_y * w_y).sum()"""
    cfg = make_config(case)
    xs, ys = shapes(case)
    x = torch.from_numpy(np.random.RandomState(7).uniform(0, 1, size=xs).astype(np.float32))
    rs = np.random.RandomState(3)
    wx = torch.from_numpy(rs.standard_normal(xs).astype(np.float32))
    wy = torch.from_numpy(rs.standard_normal(ys).astype(np.float32))
    return cfg, x, case_y(case), torch.tensor([12.25, 871.0][:B]), wx, wy


def params(cfg, shapes_=None, seed=0):
    """DDPM family: score_oracle.synth_params on the oracle's shape table.  NCSN++: cases.ncsnpp_params on ``shapes_`` (the state_dict's
    key -> shape of the model at hand, the reference's or ours)"""
    if cfg.model.name.startswith('ddpm'):
        return wc.params(cfg, seed)
    return cases.ncsnpp_params({k: tuple(v) for k, v in shapes_.items()}, seed)


def golden():
    return np.load(GOLDEN)


def forward64(p, case, x, y, labels, how='ref'):
    """float64 restatement of the KxSR forward from the state_dict alone -> (out_x, out_y): the paired network on
    cat(x, resize(y -> S)), its y channels resized to S / K"""
    import score_oracle as so
    name, cx, cy, S, K = CASES[case][:5]
    cfg = make_config(case, twin=True)
    y_up = resize(y.double(), S, how)
    if name == 'ddpm_KxSR':
        out = wc.forward64(p, cfg, x.double(), y_up, labels)
    else:
        # the Gaussian Fourier argument ((t W) 2) pi is part of the result in fp32 (it reaches 1e5 at t (N - 1) = 999: layerspp.py:39-41),
        # so it is formed in fp32 as the reference forms it; everything behind it runs in float64, one sample at a time (the network
        # has no cross-sample operation) with W replaced by argument / (2 pi) and time_cond = 1
        pd = {k: v.double() for k, v in p.items()}
        wkey = 'all_modules.0.W'
        arg = labels.float()[:, None] * p[wkey].float()[None, :] * 2 * np.pi
        h = torch.cat([x.double(), y_up], dim=1)
        outs = []
        fir = so.fir_kernel_2d
        so.fir_kernel_2d = lambda k, gain=1.0: fir(k, gain).double()      # (the oracle's FIR taps are fp32 tensors: exact dyadic values)
        try:
            for b in range(h.shape[0]):
                pb = dict(pd)
                pb[wkey] = arg[b].double() / (2 * np.pi)
                outs.append(so.ncsnpp_forward(pb, cfg, h[b:b + 1], torch.ones(1, dtype=torch.float64)))
        finally:
            so.fir_kernel_2d = fir
        out = torch.cat(outs, dim=0)
    return out[:, :cx], resize(out[:, cx:], S // K, how)
