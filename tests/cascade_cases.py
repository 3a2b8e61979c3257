"""Seeded parity cases of the sequential super-resolution cascades (sampling/cascade.py, csd_pc_cascade_sample), shared by
tools/make_cascade_goldens.py (which runs the imported reference's samplers stage by stage on them) and the tests
(tests/test_cascade_host.py, tests/test_gpu_cascade.py).  Inputs and noise tapes are regenerated from seeds on either side, the
parameters come from score_oracle.synth_params(shapes, 0); tests/golden/cascade.npz holds the reference's outputs only: every stage's
image, ``<flow>_s<k>``.

    flow          stage 1                                          stage 2                          first-layer routes
    bicubic       sr_cases R1 (y 3 x 16^2, x 3 x 32^2, nf 32)      R2 (y 3 x 32^2, x 3 x 64^2, nf 64)  assemble + generic conv, then
                                                                                                    stem_wide_kernel with the squeeze
    haar          ddpm_paired 9 + 3 at 16^2, nf 32, (1, 2), att 8  the same at 32^2, nf 64, no att  the same two routes at 12 padded to
                                                                                                    16 channels, x | y boundary at 9
    haar_inpaint  wide_cases W2 (ddpm, 12 bands, 16^2)             W6 (12 bands, 32^2, nf 64)       mask [1, 12, 1, 1], merge into a
                                                                                                    channel slice

B = 2 and P_STEPS = 3 PC steps per stage (the conditional stages on their 1000-scale SDE pair, the inpainting stages on a VESDE with
N = 3: the reference's inpainter runs sde.N steps).

THE LINK BETWEEN HAAR STAGES IS A RESTATEMENT, NOT THE REFERENCE: the reference's transform (iunets' InvertibleDownsampling2D) cannot
be imported here, so ``merge64`` restates ``haar_backward`` in float64 torch (conv_transpose2d with the orthonormal Haar matrix HAAR,
band-major channels); the fixture tool and ``cascade64`` both use it.  The samplers on either side of the link are the reference's.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')) if p not in sys.path]
import cases  # noqa: E402
import score_oracle as so  # noqa: E402
import sr_cases as sc  # noqa: E402
import wide_cases as wc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'cascade.npz')
B = 2
P_STEPS = 3
FLOWS = ('bicubic', 'haar', 'haar_inpaint')
N_STAGES = 2
EPS = 1e-5
TRAJECTORY = 1e-3            # the project's sampler bound (tests/test_gpu_sr.py TRAJECTORY), here of the stage's sigma_max_x
# rows = bands, columns = 2 dy + dx (include/csd.h, csd_band_split)
HAAR = torch.tensor([[.5, .5, .5, .5], [.5, -.5, .5, -.5], [.5, .5, -.5, -.5], [.5, -.5, -.5, .5]], dtype=torch.float64)
HAAR_STAGES = [dict(nf=32, image_size=16, attn_resolutions=(8,)), dict(nf=64, image_size=32, attn_resolutions=())]


def stage_config(flow, k, precision=None):
    if flow == 'bicubic':
        return sc.make_config(('R1', 'R2')[k], precision)
    if flow == 'haar_inpaint':
        return wc.make_config(('W2', 'W6')[k], precision)
    cfg = cases.make_config(name='ddpm_paired', ch_mult=(1, 2), num_res_blocks=1, x_ch=9, y_ch=3, **HAAR_STAGES[k])
    if precision is not None:
        cfg.model.csd_precision = precision
    return cfg


def stage_params(flow, k):
    return wc.params(stage_config(flow, k), 0)


def sigma_max(flow, k):
    return float(stage_config(flow, k).model.sigma_max_x)


def state_shape(flow, k):
    """the state of stage k: the image of a bicubic stage, the 9 detail bands of a Haar stage, the 12 bands of an inpainting stage"""
    return (B,) + tuple(stage_config(flow, k).data.shape_x)


def cond_shape(flow, k):
    return None if flow == 'haar_inpaint' else (B,) + tuple(stage_config(flow, k).data.shape_y)


def image_shape(flow, k):
    """the image stage k hands on"""
    S = stage_config(flow, k).data.effective_image_size
    return (B, 3, 2 * S, 2 * S)


def lr_input(flow):
    """the cascade's input in [0, 1): the low-resolution image (bicubic) / the low band (both Haar forms), wide_cases.case_y's recipe"""
    rs = np.random.RandomState(321)
    y = rs.uniform(0, 1, size=(B, 3, 16, 16)).astype(np.float32)
    y[:, :, 4:12, 4:12] = 0.
    return torch.from_numpy(y)


def tape(flow, k):
    """stage k's normals in its sampler's draw order: the prior, then per step and phase (corrector, predictor) z_y, z_x for the two-SDE
    stages and z_update, z_blend for the inpainting stages"""
    xs, ys = state_shape(flow, k), cond_shape(flow, k)
    per_phase = [xs, xs] if ys is None else [ys, xs]
    return cases.tape([xs] + (per_phase + per_phase) * P_STEPS, seed=500 + 10 * FLOWS.index(flow) + k)


def golden():
    return np.load(GOLDEN)


# ---- the band link, float64 ---------------------------------------------------------------------------------------------------------------
def merge64(lo, hi, matrix=HAAR):
    """float64 restatement of haar_backward on band-major channels: [B, C, S, S] low band and [B, 3C, S, S] detail bands ->
    [B, C, 2S, 2S], x[c, 2i + dy, 2j + dx] = sum_k matrix[k][2 dy + dx] * band_k[c, i, j], as one grouped conv_transpose2d"""
    Bq, C, S, _ = lo.shape
    bands = torch.cat([lo, hi], dim=1).double().reshape(Bq, 4, C, S, S).transpose(1, 2).reshape(Bq, 4 * C, S, S)      # channel c*4 + k
    w = matrix.double().reshape(4, 1, 2, 2).repeat(C, 1, 1, 1)
    return F.conv_transpose2d(bands, w, stride=2, groups=C)


def split64(x, matrix=HAAR):
    """the transpose of merge64: [B, C, 2S, 2S] -> [B, 4C, S, S] band-major"""
    Bq, C, H, _ = x.shape
    w = matrix.double().reshape(4, 1, 2, 2).repeat(C, 1, 1, 1)
    out = F.conv2d(x.double(), w, stride=2, groups=C)                                     # channel c*4 + k
    return out.reshape(Bq, C, 4, H // 2, H // 2).transpose(1, 2).reshape(Bq, 4 * C, H // 2, H // 2)


# ---- float64 restatement of the whole cascade -----------------------------------------------------------------------------------------
def _b(v):
    return v[:, None, None, None]


def _pc64(net, ve_x, ve_y, y, tp, inpaint=None):
    """one stage: the default loop of get_pc_conditional_sampler on the VE pair (sampling/conditional.py:180-226) or get_pc_inpainter
    (sampling/unconditional.py:230-345), corrector then predictor, denoised.  State, network and updates in float64; the per-step
    scalars are the reference's fp32 expressions (score_oracle.VE), widened."""
    it = iter(tp)
    z = lambda: next(it).double()      # noqa: E731
    if inpaint is not None:
        data, mask = inpaint
        x = data * mask + z() * ve_x.sigma_max * (1. - mask)
    else:
        x = z() * ve_x.sigma_max
    ts = torch.linspace(1, EPS, P_STEPS)
    x_mean = x
    for i in range(P_STEPS):
        vec_t = torch.ones(x.shape[0]) * ts[i]
        std, G = ve_x.std(vec_t).double(), ve_x.G(vec_t).double()
        for phase in ('corrector', 'predictor'):
            y_in = y + z() * _b(ve_y.std(vec_t).double()) if ve_y is not None else None
            score = net(x, y_in, vec_t) / _b(std)
            zz = z()
            if phase == 'corrector':
                g = torch.norm(score.reshape(score.shape[0], -1), dim=-1).mean()
                n = torch.norm(zz.reshape(zz.shape[0], -1), dim=-1).mean()
                step = (0.15 * n / g) ** 2 * 2
                x_mean = x + step * score
                x = x_mean + torch.sqrt(step * 2) * zz
            else:
                x_mean = x + _b(G) ** 2 * score
                x = x_mean + _b(G) * zz
            if inpaint is not None:
                masked = data + z() * _b(std)
                x = x * (1. - mask) + masked * mask
                x_mean = x * (1. - mask) + data * mask
    assert next(it, None) is None
    return x_mean


def cascade64(flow, mangle=None):
    """float64 restatement of the whole cascade on the cases' tapes -> every stage's image.  ``mangle`` restates it WRONGLY on purpose
    (tests/test_cascade_host.py): 'bands' exchanges bands 1 and 2 in every merge (for the Haar matrix the same as exchanging dy and dx
    of the block), 'squeeze' exchanges dy and dx of the space-to-depth squeeze of the SECOND bicubic stage."""
    assert mangle in (None, 'bands', 'squeeze') and (mangle != 'squeeze' or flow == 'bicubic') and (mangle != 'bands' or flow != 'bicubic')
    matrix = HAAR[[0, 2, 1, 3]] if mangle == 'bands' else HAAR
    cur = lr_input(flow).double()
    images = []
    for k in range(N_STAGES):
        cfg, p = stage_config(flow, k), stage_params(flow, k)
        m = cfg.model
        if flow == 'haar_inpaint':
            ve = so.VE(m.sigma_min_x, m.sigma_max_x, P_STEPS)
            data = torch.cat([cur, torch.zeros(B, 9, cur.shape[2], cur.shape[3], dtype=torch.float64)], dim=1)
            mask = torch.zeros(1, 12, 1, 1, dtype=torch.float64)
            mask[:, :3] = 1.
            net = lambda x, y, t, cfg=cfg, p=p, ve=ve: wc.forward64(p, cfg, x, None, ve.std(t))      # noqa: E731  (label: sigma(t))
            bands = _pc64(net, ve, None, None, tape(flow, k), inpaint=(data, mask))
            cur = merge64(data[:, :3], bands[:, 3:], matrix)
        else:
            ve_x, ve_y = so.VE(m.sigma_min_x, m.sigma_max_x, m.num_scales), so.VE(m.sigma_min_y, m.sigma_max_y, m.num_scales)
            if flow == 'bicubic':
                order = 'swap' if (mangle == 'squeeze' and k == 1) else 'ref'
                net = lambda x, y, t, k=k, p=p, order=order: sc.forward64(p, ('R1', 'R2')[k], x, y, t * (m.num_scales - 1), order)[0]      # noqa: E731
                cur = _pc64(net, ve_x, ve_y, cur, tape(flow, k))
            else:
                net = lambda x, y, t, cfg=cfg, p=p: wc.forward64(p, cfg, x, y, t * (m.num_scales - 1))[:, :9]      # noqa: E731
                cur = merge64(cur, _pc64(net, ve_x, ve_y, cur, tape(flow, k)), matrix)
        images.append(cur)
    return images
