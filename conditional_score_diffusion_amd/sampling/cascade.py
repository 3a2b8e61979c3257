"""Sequential super-resolution cascades: the multi-scale mode of the reference (run_lib.py:113-222, ``multi_scale_test``).

``get_autoregressive_sampler(stages, coord_space, ...)`` follows run_lib.py:145-222 and returns
``sampler(lr, return_intermediate_images=False, show_evolution=False, noise_tapes=None, seed=None)``:

    'bicubic'       a low-resolution image goes through 2x stage after 2x stage (``bicubic_autoregressive_sampler``, the configs under
                    configs/ve/srflow/*/sequential/bicubic): stage k's result is stage k + 1's condition
    'haar'          the low band of a Haar pyramid has its detail bands sampled level by level (``haar_autoregressive_sampler``,
                    .../sequential/haar): a stage samples the 3C detail bands given the C-channel low band, ``haar_backward`` of the two
                    is the next level's low band
    'haar_inpaint'  the inpainting form of the same pyramid with unconditional 4C-band networks
                    (lightning_modules/HaarMultiScaleSdeGenerativeModel.py:62-89 and the ``auto_regressive_sampling`` sketch below it):
                    the known low band is bands [0, C) of the data, mask [1, 4C, 1, 1], the merge of the inpainted bands is the next
                    level's low band

It returns what the reference's inner functions return: ``(list of CPU images, [])`` with ``return_intermediate_images`` (the input
first, then every level), else ``(image, [])``.  ``show_evolution=True`` raises NotImplementedError.

Two routes, the same bits.  ``one_call=True``: every stage's loop is prepared on the host (``fused.prepare``) and ONE
csd_pc_cascade_sample enqueues all of them with the hand-over between stages on the device (csd_band_merge, the initial blend of an
inpainting stage) and one synchronisation behind the last stage; a stage that is not ``fused.fusable`` raises, naming the stage and the
reason.  ``one_call=False``: the existing per-stage samplers (``get_conditional_sampling_fn`` / ``get_pc_inpainter(device_loop=True)``)
chained in Python, one synchronisation per stage.  ``one_call=None`` picks the one call when every stage allows it.

Noise: ``noise_tapes`` is one tape per stage in that stage's existing layout (the prior first); ``seed=s`` gives stage k the Philox key
``stage_seed(s, k)``, so a cascade equals its stages run one by one with those seeds.

The band transform: ``haar_forward`` / ``haar_backward`` / ``get_dc_coefficients`` / ``get_hf_coefficients`` are the four helpers of
lightning_modules/ConditionalSdeGenerativeModel.py:207-221 over ``ops.band_split`` / ``ops.band_merge``, in the band-major channel order
the reference has after ``permute_channels(forward=True)``.  The reference's transform is iunets' InvertibleDownsampling2D(init='haar');
that library was not available here, so the order and signs of bands 1 - 3 are NOT checked against it: ``band_matrix`` (4 x 4, rows =
bands, columns = 2 dy + dx, orthogonal) replaces the built-in orthonormal Haar matrix for a caller who has that library's kernel.
"""
import ctypes

import torch

from .. import _lib, ops, sde_lib
from .._lib import check, current_stream, lib, ptr
from . import fused
from .conditional import get_conditional_sampling_fn
from .correctors import get_corrector
from .predictors import get_predictor
from .unconditional import get_pc_inpainter

COORD_SPACES = ('bicubic', 'haar', 'haar_inpaint')


def stage_seed(seed, k):
    """The Philox key of stage k (0-based) of a cascade seeded with ``seed``: distinct per stage, so no stage reuses another's noise"""
    return (int(seed) * 1000003 + 104729 * (int(k) + 1)) & 0x7FFFFFFFFFFFFFFF


# ---- the four helpers of ConditionalSdeGenerativeModel.py:207-221 -----------------------------------------------------------------------
def haar_forward(x, band_matrix=None):
    """image [B, C, 2S, 2S] -> bands [B, 4C, S, S], band-major (``haar_transform`` + ``permute_channels``)"""
    return ops.band_split(x, band_matrix)


def haar_backward(x, band_matrix=None):
    """bands [B, 4C, S, S] -> image [B, C, 2S, 2S] (``permute_channels(forward=False)`` + ``haar_transform.inverse``)"""
    if x.dim() != 4 or x.shape[1] % 4:
        raise RuntimeError('haar_backward: needs [B, 4C, S, S] bands (got %s)' % (tuple(x.shape),))
    C = x.shape[1] // 4
    return ops.band_merge(x[:, :C], x[:, C:], band_matrix)


def get_dc_coefficients(x, levels=1, band_matrix=None):
    """the low band of ``levels`` Haar steps: [B, C, S, S] -> [B, C, S / 2^levels, S / 2^levels] (run_lib.py:115-130 loops it)"""
    for _ in range(int(levels)):
        C = x.shape[1]
        x = haar_forward(x, band_matrix)[:, :C].contiguous()
    return x


def get_hf_coefficients(x, band_matrix=None):
    """the three detail bands of one Haar step: [B, C, 2S, 2S] -> [B, 3C, S, S]"""
    C = x.shape[1]
    return haar_forward(x, band_matrix)[:, C:].contiguous()


# ---- per-stage settings -----------------------------------------------------------------------------------------------------------------
def _settings(k, sde, config, coord_space, predictor, corrector, p_steps, c_steps):
    """the sampler settings of stage k as get_conditional_sampling_fn / get_inpainting_fn read them from its config, with the overrides of
    multi_scale_test applied (run_lib.py:156,181 pass predictor, corrector, p_steps, c_steps to every stage)"""
    s, m = config.sampling, config.model
    inpaint = coord_space == 'haar_inpaint'
    c_sde = sde['x'] if isinstance(sde, dict) else sde
    st = dict(predictor=get_predictor((s.predictor if predictor == 'default' else predictor).lower()),
              corrector=get_corrector((s.corrector if corrector == 'default' else corrector).lower()),
              snr=s.snr, denoise=s.noise_removal, probability_flow=s.probability_flow, continuous=config.training.continuous,
              # sampling_eps of the lightning modules' configure_sde: 1e-5 for the VE SDEs, 1e-3 for VP / sub-VP
              eps=1e-5 if isinstance(c_sde, (sde_lib.VESDE, sde_lib.cVESDE)) else 1e-3)
    if inpaint:
        # get_inpainting_fn (sampling/unconditional.py:78-91): sde.N steps, one corrector step each
        if isinstance(sde, dict):
            raise ValueError('stage %d: the inpainting form takes a single SDE, not an {x, y} pair' % k)
        if p_steps not in ('default', sde.N) or c_steps not in ('default', 1):
            raise ValueError('stage %d: the inpainter runs sde.N = %d steps with one corrector step each (get_inpainting_fn); '
                             'p_steps = %r / c_steps = %r cannot be honoured' % (k, sde.N, p_steps, c_steps))
        st.update(p_steps=sde.N, c_steps=1)
    else:
        st.update(p_steps=m.num_scales if p_steps == 'default' else p_steps, c_steps=s.n_steps_each if c_steps == 'default' else c_steps)
    return st


def _why_not_one_call(model, sde, st, inpaint, check_device=True):
    """None when csd_pc_cascade_sample can run this stage, else the reason (``check_device=False``: leave out where the model lies)"""
    from ..models.ddpm import HipUNet
    if not isinstance(model, HipUNet):
        return 'the model is a %s, not a planned 2-D HipUNet (DDPM family or NCSN++; 3-D stages are out of scope)' % type(model).__name__
    if getattr(model, 'y_scale', 0):
        return 'the Kx networks (y_scale) do not run in a cascade'
    if inpaint != (model.y_channels == 0):
        return ('the inpainting form runs unconditional networks, this one takes a %d-channel condition' % model.y_channels if inpaint
                else 'a conditional stage needs a network with a condition, this one is unconditional')
    if st['c_steps'] != 1:
        return 'c_steps = %s corrector steps per update (the device loop runs 1)' % (st['c_steps'],)
    if not fused.fusable(model, sde, st['predictor'], st['corrector'], st['c_steps'], st['probability_flow'], st['continuous']):
        return 'the device loop does not implement (%s, %s, %s, probability_flow=%s, continuous=%s)' % (
            type(sde['x'] if isinstance(sde, dict) else sde).__name__, st['predictor'].__name__, st['corrector'].__name__,
            st['probability_flow'], st['continuous'])
    if check_device and model.device.type != 'cuda':
        return 'the model is on %s, the device loop runs on the GPU' % model.device
    return None


def _check_stages(stages, coord_space):
    """shape errors a wrong stage order makes, named before anything runs: each stage's condition must be the image the stage before
    hands on"""
    if coord_space not in COORD_SPACES:
        raise NotImplementedError('%s space is not supported for autoregressive sampling (one of %s)' % (coord_space, ', '.join(COORD_SPACES)))
    if not stages:
        raise ValueError('get_autoregressive_sampler: no stages')
    for k, stage in enumerate(stages):
        if len(stage) != 3:
            raise ValueError('stage %d: a stage is a (model, sde, config) triple' % k)
    sides = []
    for k, (model, sde, config) in enumerate(stages):
        d = config.data
        if coord_space == 'haar_inpaint':
            ch, side = int(d.num_channels), int(d.image_size)
            if ch % 4:
                raise ValueError('stage %d: the inpainting form needs 4C band channels, the config has %d' % (k, ch))
        else:
            if not isinstance(sde, dict):
                raise ValueError('stage %d: a conditional stage takes the SDE pair {"x": ..., "y": ...}' % k)
            (cx, sx), (cy, sy) = (int(d.shape_x[0]), int(d.shape_x[-1])), (int(d.shape_y[0]), int(d.shape_y[-1]))
            if coord_space == 'bicubic' and (cx != cy or sx != 2 * sy):
                raise ValueError('stage %d: a bicubic stage maps y [%d, %d, %d] to x of the same channels at twice the side, its config '
                                 'has x %s' % (k, cy, sy, sy, list(d.shape_x)))
            if coord_space == 'haar' and (cx != 3 * cy or sx != sy):
                raise ValueError('stage %d: a Haar stage samples the 3C detail bands of its C-channel low band at the same side, its '
                                 'config has x %s, y %s' % (k, list(d.shape_x), list(d.shape_y)))
            side = sy
        sides.append(side)
    for k in range(1, len(sides)):
        if sides[k] != 2 * sides[k - 1]:
            raise ValueError('stages must be in low-to-high order, each at twice the side of the one before: stage %d runs at %d, stage %d '
                             'at %d' % (k - 1, sides[k - 1], k, sides[k]))


def get_autoregressive_sampler(stages, coord_space='bicubic', predictor='default', corrector='default', p_steps='default',
                               c_steps='default', band_matrix=None, one_call=None):
    """see the module docstring; ``stages``: (model, sde or {x, y} pair, config) triples in low-to-high order"""
    _check_stages(stages, coord_space)
    stages = [tuple(s) for s in stages]
    inpaint = coord_space == 'haar_inpaint'
    settings = [_settings(k, sde, cfg, coord_space, predictor, corrector, p_steps, c_steps) for k, (_, sde, cfg) in enumerate(stages)]
    n = len(stages)
    if one_call:                                 # what does not depend on where the models lie is refused here, not at the first call
        for k, ((model, sde, _), st) in enumerate(zip(stages, settings)):
            why = _why_not_one_call(model, sde, st, inpaint, check_device=False)
            if why is not None:
                raise NotImplementedError('get_autoregressive_sampler(one_call=True): stage %d: %s' % (k, why))

    def route():
        """True: the one call; raises when ``one_call=True`` cannot be honoured"""
        if one_call is False:
            return False
        for k, ((model, sde, _), st) in enumerate(zip(stages, settings)):
            why = _why_not_one_call(model, sde, st, inpaint)
            if why is not None:
                if one_call:
                    raise NotImplementedError('get_autoregressive_sampler(one_call=True): stage %d: %s' % (k, why))
                return False
        return True

    def mask_for(data):
        C4 = data.shape[1]
        mask = torch.zeros(1, C4, 1, 1, dtype=torch.float32, device=data.device)
        mask[:, :C4 // 4] = 1.
        return mask

    def first_data(lr):
        """the inpainting form's up_sample (HaarMultiScaleSdeGenerativeModel.py:75-80): zeros with the low band in channels [0, C)"""
        B, C, S, _ = lr.shape
        data = torch.zeros(B, 4 * C, S, S, dtype=torch.float32, device=lr.device)
        data[:, :C] = lr
        return data

    def chained(lr, tapes, seeds, keep):
        """the existing per-stage samplers, one after the other"""
        images = []
        cur = lr
        for k, ((model, sde, cfg), st) in enumerate(zip(stages, settings)):
            kw = dict(noise_tape=tapes[k] if tapes is not None else None, seed=seeds[k])
            if inpaint:
                fn = get_pc_inpainter(sde, st['predictor'], st['corrector'], st['snr'], n_steps=1, probability_flow=st['probability_flow'],
                                      continuous=st['continuous'], denoise=st['denoise'], eps=st['eps'], device_loop=True)
                data = first_data(cur)
                bands, _ = fn(model, data, mask_for(data), **kw)
                C = cur.shape[1]
                cur = ops.band_merge(data[:, :C], bands[:, C:], band_matrix)
            else:
                fn = get_conditional_sampling_fn(cfg, sde, model._x_shape(cur.shape[0]), st['eps'], predictor=predictor, corrector=corrector,
                                                 p_steps=p_steps, c_steps=c_steps)
                x, _ = fn(model, cur, **kw)
                cur = x if coord_space == 'bicubic' else ops.band_merge(cur, x, band_matrix)
            if keep:
                images.append(cur)
        return cur, images

    def fused_cascade(lr, tapes, seeds, keep):
        """csd_pc_cascade_sample: every stage prepared on the host, one call"""
        dev, B = lr.device, lr.shape[0]
        preps, outs = [], []
        arr = (_lib.CascadeStage * n)()
        C = lr.shape[1]
        for k, ((model, sde, cfg), st) in enumerate(zip(stages, settings)):
            kw = dict(noise_tape=tapes[k] if tapes is not None else None, seed=seeds[k], predictor=st['predictor'],
                      corrector=st['corrector'], probability_flow=st['probability_flow'], continuous=st['continuous'])
            shape = model._x_shape(B)
            if inpaint:
                data = first_data(lr) if k == 0 else ops._out(shape, torch.float32, dev)       # (k >= 1: the library zeroes and fills it)
                prep = fused.prepare(model, sde, shape, None, st['p_steps'], st['snr'], st['eps'], st['denoise'],
                                     unconditional_label=fused.unconditional_label(model), inpaint=(data, mask_for(data)), blend=(k == 0),
                                     **kw)
            else:
                prep = fused.prepare(model, sde, shape, None, st['p_steps'], st['snr'], st['eps'], st['denoise'], **kw)
            preps.append(prep)
            g = arr[k]
            g.net, g.packed = model._h, model._packed.data_ptr()
            g.pc = ctypes.pointer(prep.p)
            g.inpaint = ctypes.pointer(prep.constraint.struct) if prep.constraint is not None else None
            g.x = prep.x.data_ptr()
            g.link = 0 if (k == 0 or coord_space == 'bicubic') else (2 if inpaint else 1)
            # the image a Haar stage hands on: a caller buffer where it is returned (the last level, every level with
            # return_intermediate_images), else a region of the scratch; link 2 writes it into the next stage's data
            side = 2 * model.image_size
            want = coord_space == 'haar' and (keep or k == n - 1) or (inpaint and k == n - 1)
            outs.append(ops._out((B, C, side, side), torch.float32, dev) if want else None)
            g.out = outs[k].data_ptr() if want else None
        ws_bytes = max(int(lib().csd_unet_workspace_bytes(m._h, B)) for m, _, _ in stages)
        pc_bytes = max((int(lib().csd_pc_scratch_bytes(m._h, B)) + 255) // 256 * 256 for m, _, _ in stages)
        hand = sum((B * C * 4 * m.image_size ** 2 * 4 + 255) // 256 * 256
                   for k, (m, _, _) in enumerate(stages) if coord_space == 'haar' and k < n - 1 and outs[k] is None)
        ws = ops._scratch(ws_bytes, dev)
        scratch = ops._scratch(pc_bytes + hand, dev)
        flags = ops._out((n,), torch.int32, dev)
        y0 = None if inpaint else lr
        sampler.stage_flags = flags              # (stage k's flag of the finiteness contract, also behind a NonFiniteError)
        check(lib().csd_pc_cascade_sample(arr, n, 0 if coord_space == 'bicubic' else (2 if inpaint else 1), ptr(y0), B, ptr(ws),
                                          ws.numel(), ptr(scratch), scratch.numel(), ptr(flags), ops._band_matrix(band_matrix),
                                          current_stream(dev)), 'pc_cascade_sample')
        if coord_space == 'bicubic':
            images = [p.x for p in preps]
        elif inpaint:
            images = [preps[k + 1].constraint.data[:, :C] for k in range(n - 1)] + [outs[-1]]
        else:
            images = outs
        del arr                                  # (it pointed into preps, alive until here; the call synchronised)
        return images[-1], (images if keep else [])

    def sampler(lr, return_intermediate_images=False, show_evolution=False, noise_tapes=None, seed=None):
        if show_evolution:
            raise NotImplementedError('show_evolution is not provided for the cascades: run the stage of interest through its own sampler')
        _lib.require_gpu_tensor(lr, 'lr')
        if noise_tapes is not None and len(noise_tapes) != n:
            raise ValueError('noise_tapes holds %d tapes, the cascade has %d stages' % (len(noise_tapes), n))
        if seed is None:
            seed = fused.fresh_seed()
        seeds = [stage_seed(seed, k) for k in range(n)]
        lr = lr.contiguous()
        with torch.no_grad():
            run = fused_cascade if route() else chained
            image, images = run(lr, noise_tapes, seeds, return_intermediate_images)
        if return_intermediate_images:
            return [lr.clone().cpu()] + [im.clone().cpu() for im in images], []
        return image, []

    return sampler
