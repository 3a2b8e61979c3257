"""Seeded parity cases of the 3-D DDPM networks, shared by tools/make_ddpm3d_goldens.py (which runs the imported reference on them) and
the tests (which run the HIP path on them).  Inputs, labels and noise tapes are regenerated from seeds on either side, the parameters come
from score_oracle.synth_params on the state_dict shapes; tests/golden/ddpm3d.npz holds the reference's outputs and the state_dict
name / shape lists only.

    case   model               nf  ch_mult    res blocks  B  volume (D x H x W)
    A      ddpm3D_paired       32  (1, 2, 2)  1           2  12 x 20 x 8   levels 12x20x8 -> 6x10x4 -> 3x5x2; concats of 96 and 128 channels
    B      ddpm3D_paired_SR3   32  (1, 2)     1           2  6 x 10 x 4    1-channel head
    C      ddpm3D              as B, one input channel

It also holds a float64 restatement of the forward in torch (F.conv3d, F.group_norm, F.avg_pool3d, F.interpolate) for networks the
fixture does not cover (other activations).
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'oracle')) if p not in sys.path]
from conditional_score_diffusion_amd.config_dict import ConfigDict  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ddpm3d.npz')

CASES = {
    # name: (model, nf, ch_mult, num_res_blocks, B, (D, H, W), x channels, y channels)
    'A': ('ddpm3D_paired', 32, (1, 2, 2), 1, 2, (12, 20, 8), 1, 1),
    'B': ('ddpm3D_paired_SR3', 32, (1, 2), 1, 2, (6, 10, 4), 1, 1),
    'C': ('ddpm3D', 32, (1, 2), 1, 2, (6, 10, 4), 1, 0),
}
LABELS = [3., 420.5]
# sampler runs: cVESDE(0.01, 30, N = 6) (S2: the pair with VESDE(0.01, 1, N = 6) for y), conditional reverse diffusion + conditional
# Langevin, continuous, denoise
SIGMA_MIN, SIGMA_MAX, SIGMA_MAX_Y, N_SCALES, SNR, P_STEPS, EPS = 0.01, 30., 1., 6, 0.16, 3, 1e-5
SAMPLER_RUNS = {'S1': 'B', 'S2': 'A'}


def make_config(case, nonlinearity='swish', precision=None):
    """a reference-style config with the keys models/ddpm3D.py:40-105 reads (cf. configs/ve/inverse_problems/MRI_to_PET/
    MRI_to_PET_slices3D.py: no attention, average-pool / nearest resampling, centered = False)"""
    name, nf, ch_mult, nrb, B, vol, xc, yc = CASES[case]
    c = ConfigDict()
    c.training = ConfigDict(continuous=True, sde='vesde')
    c.sampling = ConfigDict(method='pc', predictor='conditional_reverse_diffusion', corrector='conditional_langevin', n_steps_each=1,
                            noise_removal=True, probability_flow=False, snr=SNR)
    c.data = ConfigDict(centered=False, shape_x=[xc] + list(vol), shape_y=[yc] + list(vol), num_channels=xc + yc)
    c.model = ConfigDict(name=name, nf=nf, ch_mult=tuple(ch_mult), num_res_blocks=nrb, dropout=0.1, resamp_with_conv=False,
                         conditional=True, nonlinearity=nonlinearity, num_scales=N_SCALES, sigma_min_x=SIGMA_MIN, sigma_max_x=SIGMA_MAX,
                         sigma_min_y=SIGMA_MIN, sigma_max_y=SIGMA_MAX_Y, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX,
                         input_channels=xc + yc, output_channels=xc + yc if name == 'ddpm3D_paired' else xc,
                         embedding_type='positional', scale_by_sigma=True)
    if precision is not None:
        c.model.csd_precision = precision
    return c, B


def case_inputs(case):
    """x ~ 5 N(0, 1), y ~ U(0, 1) (None for the unconditional network), labels"""
    name, nf, ch_mult, nrb, B, vol, xc, yc = CASES[case]
    rs = np.random.RandomState(1234)
    x = torch.from_numpy((5.0 * rs.standard_normal((B, xc) + vol)).astype(np.float32))
    y = torch.from_numpy(rs.uniform(0, 1, size=(B, yc) + vol).astype(np.float32)) if yc else None
    return x, y, torch.tensor(LABELS[:B], dtype=torch.float32)


def sampler_tape(run):
    """the normals of a sampler run in draw order: the prior, then per step and per phase (corrector, predictor) [z_y of the two-SDE
    pair,] z_x"""
    import cases
    case = SAMPLER_RUNS[run]
    name, nf, ch_mult, nrb, B, vol, xc, yc = CASES[case]
    xs, ys = (B, xc) + vol, (B, yc) + vol
    per_phase = [ys, xs] if name == 'ddpm3D_paired' else [xs]
    return cases.tape([xs] + (per_phase + per_phase) * P_STEPS)


def golden():
    return np.load(GOLDEN)


def golden_shapes(case):
    """the reference's state_dict as {name: shape}, in its order"""
    return {k: tuple(v) for k, v in json.loads(str(golden()['shapes_' + case]))}


def params(case, seed=0):
    import score_oracle as so
    return so.synth_params(golden_shapes(case), seed)


def call(model, case, x, y, labels):
    """model output as one tensor (the paired network's two halves concatenated back)"""
    if CASES[case][0] == 'ddpm3D':
        return model(x, labels)
    out = model({'x': x, 'y': y}, labels)
    return torch.cat([out['x'], out['y']], dim=1) if isinstance(out, dict) else out


# ---- float64 restatement of the forward (what models/ddpm3D.py:107-171 computes), from the state_dict alone ----
_ACTS = {'swish': F.silu, 'relu': F.relu, 'elu': F.elu, 'lrelu': lambda v: F.leaky_relu(v, 0.2)}


def forward64(p, case, x, y, labels, nonlinearity='swish', centered=False):
    name, nf, ch_mult, nrb, B, vol, xc, yc = CASES[case]
    p = {k: v.double() for k, v in p.items()}
    act = _ACTS[nonlinearity]
    h = (torch.cat([x, y], dim=1) if y is not None else x).double()

    def P(i, s):
        return p['all_modules.%d.%s' % (i, s)]

    def conv(i, s, v):
        pre = s + '.' if s else ''
        return F.conv3d(v, P(i, pre + 'weight'), P(i, pre + 'bias'), padding=1)

    def gn(i, s, v):
        pre = s + '.' if s else ''
        return F.group_norm(v, 32, P(i, pre + 'weight'), P(i, pre + 'bias'), eps=1e-6)

    def res(i, v, temb):
        t = act(gn(i, 'GroupNorm_0', v))
        t = conv(i, 'Conv_0', t) + F.linear(act(temb), P(i, 'Dense_0.weight'), P(i, 'Dense_0.bias'))[:, :, None, None, None]
        t = conv(i, 'Conv_1', act(gn(i, 'GroupNorm_1', t)))
        if ('all_modules.%d.Conv_2.weight' % i) in p:
            v = conv(i, 'Conv_2', v)
        return v + t

    half = nf // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float64) * -(np.log(10000.0) / (half - 1)))
    e = labels.double()[:, None] * freq[None, :]
    temb = torch.cat([torch.sin(e), torch.cos(e)], dim=1)
    temb = F.linear(temb, P(0, 'weight'), P(0, 'bias'))
    temb = F.linear(act(temb), P(1, 'weight'), P(1, 'bias'))
    if not centered:
        h = 2 * h - 1.
    i = 2
    hs = [conv(i, '', h)]
    i += 1
    L = len(ch_mult)
    for lvl in range(L):
        for _ in range(nrb):
            hs.append(res(i, hs[-1], temb))
            i += 1
        if lvl != L - 1:
            hs.append(F.avg_pool3d(hs[-1], 2, 2))
            i += 1
    h = hs[-1]
    for _ in range(2):
        h = res(i, h, temb)
        i += 1
    for lvl in reversed(range(L)):
        for _ in range(nrb + 1):
            h = res(i, torch.cat([h, hs.pop()], dim=1), temb)
            i += 1
        if lvl != 0:
            h = F.interpolate(h, scale_factor=2, mode='nearest')
            i += 1
    h = act(gn(i, '', h))
    return conv(i + 1, '', h)
