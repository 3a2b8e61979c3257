"""Seeded parity cases of NCSN++ on images with more than 8 channels and of ncsnpp_2xSR, shared by tools/make_ncsnpp_wide_goldens.py
(which runs the imported reference on them) and the tests (tests/test_ncsnpp_wide_host.py, tests/test_gpu_ncsnpp_wide.py).  Inputs,
labels and noise tapes are regenerated from seeds on either side, the parameters come from cases.ncsnpp_params(shapes, 5);
tests/golden/ncsnpp_wide.npz holds the reference's outputs only.

    case  model          channels            side  nf  ch_mult    attention  options                                  what it can break
    N1    ncsnpp_paired  16 + 16 -> 32       16    32  (1, 2)     (8,)       fourier, fir, output_skip, input_skip    two full 16-channel K groups, a 32-wide output pyramid, y + sigma z on 16 channels
    N1c   as N1 with data.centered = True
    N2    ncsnpp_paired  9 + 3 -> 12         16    32  (1, 1, 2)  -          fourier, fir, output_skip, residual      pad 12 -> 16 with Cin 12 under pixel stride 16 in fir_pyr_conv; two pyramid levels each way
    N2n   as N2 with fir = False, positional, progressive 'none'             progressive_input id 3, the (0, 1, 1, 0) taps
    N3    ncsnpp_paired  6 + 3 -> 9          20    32  (1, 2)     (10,)      positional, progressive none / none      just over the old limit; a 9-channel plain head; 20 is no multiple of 16
    N4    ncsnpp_paired  5 + 12 -> 17        24    32  (1, 2)     -          fourier, fir, output_skip, input_skip    pad 17 -> 32, the x | y boundary inside a K group, a 17-pitch FIR upsample
    N5    ncsnpp_2xSR    x 3 @ 32^2, y 3 @ 16^2 (12 + 3 -> 15)
                                             16    32  (1, 2)     (8,)       fourier, fir, output_skip, input_skip    squeeze addressing in the assemble pass and in the residual + scattered head store; 15-pitch pyramids
    N6    ncsnpp_paired  9 + 3 -> 12         32    64  (1, 2)     -          fourier, fir, output_skip, none          nf 64: the shape the fused wide first layer covers, without an assembled tensor beside it
    N6s   as N6 with progressive_input = 'input_skip'                        ... and with one

N2, N2n, N6 and N6s are the 12 Haar bands as the paired 9 + 3 network (the SR-flow Haar models): the unconditional ``ncsnpp`` keeps its
limit of 8 channels (csrc/unet.hip: tests/test_wide_host.py pins that refusal), so inpainting and the likelihood, which exist for
unconditional networks only, have no case here.

All with one residual block per level, skip_rescale, resblock_type 'biggan' and B = 2.  N2n runs WITHOUT the output pyramid: with
fir = False the reference's pyramid_upsample cannot run (layerspp.py:117 passes 'nearest' as F.interpolate's scale_factor; see
oracle/cases.py NCSNPP_CASES), so no reference output of 'output_skip' with fir = False exists.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')) if p not in sys.path]
import cases  # noqa: E402
import sr_cases as sc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ncsnpp_wide.npz')
B = 2
PARAM_SEED = 5

_SKIP = dict(embedding_type='fourier', progressive='output_skip', progressive_input='input_skip')
CASES = {
    # name: (model, x channels, y channels, side of the network, nf, ch_mult, attention resolutions, centered, NCSN++ options)
    'N1': ('ncsnpp_paired', 16, 16, 16, 32, (1, 2), (8,), False, _SKIP),
    'N1c': ('ncsnpp_paired', 16, 16, 16, 32, (1, 2), (8,), True, _SKIP),
    'N2': ('ncsnpp_paired', 9, 3, 16, 32, (1, 1, 2), (), False, dict(_SKIP, progressive_input='residual')),
    'N2n': ('ncsnpp_paired', 9, 3, 16, 32, (1, 1, 2), (), False,
            dict(embedding_type='positional', progressive='none', progressive_input='residual', fir=False)),
    'N3': ('ncsnpp_paired', 6, 3, 20, 32, (1, 2), (10,), False, dict(embedding_type='positional', progressive='none', progressive_input='none')),
    'N4': ('ncsnpp_paired', 5, 12, 24, 32, (1, 2), (), False, _SKIP),
    'N5': ('ncsnpp_2xSR', 12, 3, 16, 32, (1, 2), (8,), False, _SKIP),      # (x channels: of the squeezed network; the image has 3)
    'N6': ('ncsnpp_paired', 9, 3, 32, 64, (1, 2), (), False, dict(_SKIP, progressive_input='none')),
    'N6s': ('ncsnpp_paired', 9, 3, 32, 64, (1, 2), (), False, _SKIP),
}
ISSUE_CASES = ['N1', 'N2', 'N3', 'N4', 'N5']      # the fixture holds both ends of the noise schedule for these
ONE_TIME_CASES = ['N1c', 'N2n', 'N6', 'N6s']      # ... and t = FORWARD_TIMES[0] only for these
FORWARD_TIMES = [1.0, 1e-5]
P_STEPS = 3
SAMPLER_CASES = ['N1', 'N4', 'N5']                # the two-SDE VE pair {'x': cVESDE, 'y': VESDE} (N3 has no SR3 twin in the NCSN++ family)
TRAIN_CASES = ['N1', 'N4', 'N5']


def make_config(case, precision=None, name=None):
    """a reference-style config: oracle/cases.py make_ncsnpp_config plus the data shapes and noise scales of cases.make_config (the
    keys the samplers and the loss read).  ``name``: the same network under another registered name ('ncsnpp_paired' for N5: the
    network WITHOUT the squeeze, on a pre-squeezed x)."""
    model, xc, yc, S, nf, ch_mult, attn, centered, opt = CASES[case] if isinstance(case, str) else case
    name = name or model
    cfg = cases.make_ncsnpp_config(name=name, nf=nf, ch_mult=ch_mult, num_res_blocks=1, attn_resolutions=attn, image_size=S,
                                   channels=xc + yc, skip_rescale=True, centered=centered, **opt)
    d, m, t, s = cfg.data, cfg.model, cfg.training, cfg.sampling
    d.shape_x = [xc, S, S]
    d.shape_y = [yc if yc else xc, S, S]
    if name == 'ncsnpp_2xSR':
        d.image_size = 2 * S
        d.shape_x = [xc // 4, 2 * S, 2 * S]
    m.dropout = 0.1
    m.sigma_min_x = m.sigma_min = 5e-3
    m.sigma_max_x = m.sigma_max = float(np.sqrt(xc * S * S))
    m.sigma_min_y, m.sigma_max_y = 5e-3, (float(np.sqrt(yc * S * S)) if model == 'ncsnpp_2xSR' else 1.0)
    m.ema_rate = 0.999
    t.likelihood_weighting = t.reduce_mean = True
    t.conditioning_approach = 'ours_NDV'
    s.snr = 0.15
    if yc:
        s.predictor, s.corrector = 'conditional_reverse_diffusion', 'conditional_langevin'
    if precision is not None:
        m.csd_precision = precision
    return cfg


def is_paired(case):
    return CASES[case][2] > 0


def case_y(case):
    """the condition image in [0, 1): a uniform draw with a zeroed square (wide_cases.case_y's recipe)"""
    yc, S = CASES[case][2], CASES[case][3]
    if not yc:
        return None
    rs = np.random.RandomState(123)
    y = rs.uniform(0, 1, size=(B, yc, S, S)).astype(np.float32)
    y[:, :, S // 4:S // 4 + S // 2, S // 4:S // 4 + S // 2] = 0.
    return torch.from_numpy(y)


def shapes(case):
    cfg = make_config(case)
    return (B,) + tuple(cfg.data.shape_x), (B,) + tuple(cfg.data.shape_y)


def forward_inputs(case):
    """[(x, t)] for FORWARD_TIMES: x = sigma(t) N(0, 1) + 0.5 (N5: the image)"""
    m = make_config(case).model
    rs = np.random.RandomState(7)
    xs = shapes(case)[0]
    out = []
    for tval in FORWARD_TIMES:
        sig = float(m.sigma_min_x * (m.sigma_max_x / m.sigma_min_x) ** tval)
        out.append((torch.from_numpy((rs.standard_normal(xs) * sig + 0.5).astype(np.float32)), torch.ones(B) * tval))
    return out


def labels_of(case, cfg, t):
    """what the score functions hand the network (models/utils.py:156-253): t (N - 1) for the conditional estimators; for the
    unconditional continuous VE network sigma(t), its logarithm with Fourier features"""
    m = cfg.model
    if is_paired(case):
        return t * (m.num_scales - 1)
    sig = (m.sigma_min_x * (m.sigma_max_x / m.sigma_min_x) ** t).float()
    return torch.log(sig) if m.embedding_type == 'fourier' else sig


def score_of(case, cfg, net, t):
    """the reference's score of the x domain from a network output in the layout of ``call``: net_x / sigma_x(t) (models/utils.py
    divide_by_sigmas behind get_conditional_score_fn(target_domain='x')), float64; N5: as the image.  The fixture holds no score arrays
    (size limit of a committed file): tools/make_ncsnpp_wide_goldens.py asserts this restatement against the reference's own score
    function to 1e-6 on every case and time"""
    m, xc = cfg.model, CASES[case][1]
    sig = m.sigma_min_x * (m.sigma_max_x / m.sigma_min_x) ** t.double()
    sx = net[:, :xc].double() / sig[:, None, None, None]
    return sc.unsqueeze(sx) if CASES[case][0] == 'ncsnpp_2xSR' else sx


def pc_tape(case, p_steps=P_STEPS):
    """the normals of a two-SDE PC run in draw order: the prior, then per step and phase (corrector, predictor) z_y, z_x"""
    xs, ys = shapes(case)
    return cases.tape([xs] + [ys, xs, ys, xs] * p_steps)


def grad_inputs(case):
    """the training-loss inputs (cases.grad_case's recipe): config with dropout off, data batch in [0, 1), fixed times, the loss's tape"""
    cfg = make_config(case)
    cfg.model.dropout = 0.0
    rs = np.random.RandomState(11)
    xs, ys = shapes(case)
    x = torch.from_numpy(rs.uniform(0, 1, size=xs).astype(np.float32))
    return cfg, x, case_y(case), torch.tensor([0.83, 0.21][:B]), cases.tape([ys, xs] if is_paired(case) else [xs], 3)


def dx_inputs(case):
    """eval-mode input gradient: x in [0, 1), labels, and the cotangent w of the scalar (out * w).sum() over both halves of the output"""
    cfg = make_config(case)
    xs, ys = shapes(case)
    x = torch.from_numpy(np.random.RandomState(7).uniform(0, 1, size=xs).astype(np.float32))
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((B, cfg.data.num_channels) + xs[2:]).astype(np.float32))
    return cfg, x, case_y(case), torch.tensor([12.25, 871.0][:B]), w


def param_shapes(cfg):
    """name -> shape of the network's state_dict, from the library's parameter table (host only: the handle without values)"""
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ncsnpp      # noqa: F401  (registers the model names)
    with torch.device('meta'):
        model = mutils.create_model(cfg)
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


def params(cfg, shapes_=None, seed=PARAM_SEED):
    return cases.ncsnpp_params(shapes_ if shapes_ is not None else param_shapes(cfg), seed)


def call(model, case, x, y, labels):
    """model output as one tensor in the layout of the network's input: the paired halves concatenated back (N5: the image-layout x
    block squeezed again)"""
    if not is_paired(case):
        return model(x, labels)
    out = model({'x': x, 'y': y}, labels)
    ox = sc.squeeze(out['x']) if CASES[case][0] == 'ncsnpp_2xSR' else out['x']
    return torch.cat([ox, out['y']], dim=1)


def oracle_forward(p, case, x, y, labels):
    """oracle/score_oracle.py ncsnpp_forward on the case, in the layout of ``call``"""
    import score_oracle as so
    cfg = make_config(case, name='ncsnpp_paired' if CASES[case][0] == 'ncsnpp_2xSR' else None)
    if CASES[case][0] == 'ncsnpp_2xSR':
        x = sc.squeeze(x)
    return so.ncsnpp_forward(p, cfg, torch.cat([x, y], dim=1) if y is not None else x, labels)


def golden():
    return np.load(GOLDEN)


# ---- cascades with NCSN++ stages (sampling/cascade.py), two stages each at sides 8 -> 16, P_STEPS steps per stage -------------------------
#   bicubic       ncsnpp_2xSR: y 3 x 8^2 -> x 3 x 16^2 on the N5 network without attention at 8^2, then N5 (-> 3 x 32^2)
#   haar          ncsnpp_paired 9 + 3 at 8^2, then at 16^2 with attention at 8
#   mixed         bicubic with a DDPM second stage: the NCSN++ first stage of 'bicubic', then sr_cases R1 (ddpm_2xSR)
# The fixture holds the reference's samplers chained on the stage tapes for 'bicubic' (``bicubic_s<k>``).
_SQ8 = ('ncsnpp_2xSR', 12, 3, 8, 32, (1, 2), (), False, _SKIP)
CASCADE_STAGES = {
    'bicubic': [_SQ8, 'N5'],
    'haar': [('ncsnpp_paired', 9, 3, 8, 32, (1, 2), (), False, _SKIP), ('ncsnpp_paired', 9, 3, 16, 32, (1, 2), (8,), False, _SKIP)],
    'mixed': [_SQ8, 'R1'],
}
CASCADE_SPACE = {'bicubic': 'bicubic', 'haar': 'haar', 'mixed': 'bicubic'}


def stage_config(flow, k, precision=None):
    spec = CASCADE_STAGES[flow][k]
    return sc.make_config(spec, precision) if spec == 'R1' else make_config(spec, precision)


def stage_params(flow, k):
    cfg = stage_config(flow, k)
    return sc.params(cfg) if CASCADE_STAGES[flow][k] == 'R1' else params(cfg)


def stage_tape(flow, k):
    """stage k's normals in its sampler's draw order (cascade_cases.tape's layout): the prior, then per step and phase z_y, z_x for the
    two-SDE stages"""
    d = stage_config(flow, k).data
    xs = (B,) + tuple(d.shape_x)
    per_phase = [(B,) + tuple(d.shape_y), xs]
    return cases.tape([xs] + (per_phase + per_phase) * P_STEPS, seed=700 + 10 * list(CASCADE_STAGES).index(flow) + k)


def lr_input():
    """the cascade's input in [0, 1): the low-resolution image / the low band, 3 x 8^2 (cascade_cases.lr_input's recipe)"""
    rs = np.random.RandomState(321)
    y = rs.uniform(0, 1, size=(B, 3, 8, 8)).astype(np.float32)
    y[:, :, 2:6, 2:6] = 0.
    return torch.from_numpy(y)
