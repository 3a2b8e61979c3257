"""PC colorization, host side (no GPU): the float64 restatement of tests/colorize_cases.py against the reference's own runs
(tests/golden/colorize.npz, tools/make_colorize_goldens.py) and its sensitivity to three wrong restatements; the draw schedule of a
colorization run as csd_pc_noise_draws lists it; the ABI struct against the header; the dispatch of ``get_pc_colorizer(device_loop=...)``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cases
import colorize_cases as cc
from conditional_score_diffusion_amd.sampling.unconditional import get_colorization_fn, get_pc_colorizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-4                                      # of sigma_max (VE) or of 1 (VP, sub-VP): DESIGN.md 4d, the inpainting row


def _err(got, name):
    ref = cc.golden()['run_' + name].astype(np.float64)
    return float(np.abs(got.numpy() - ref).max()) / cc.scale(cc.run(name)[1])


# ---- 1. the restatement and the fixture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [r[0] for r in cc.RUNS])
def test_restatement_reproduces_the_reference_runs(name):
    """measured, max |x64 - ref| / scale: ve_rd_lang 2.2e-6, ve_rd_lang_noisy 2.0e-6, vp_rd_lang 1.8e-5, ve_em_none 7.3e-6, vp_em_none
    1.5e-5, subvp_em_none 6.7e-6, ve_anc_none 1.8e-6, vp_anc_none 2.7e-5, ve_rd_none_pf 1.1e-6 - the reference's own fp32 error"""
    err = _err(cc.colorize64(name), name)
    print('%s: float64 restatement vs the reference run %.3e of scale' % (name, err))
    assert err <= BOUND


def test_restatement_reproduces_the_reference_operator():
    g = cc.golden()
    x, gray, z = cc.op_inputs()
    ms, sd = g['op_scalars']
    xn, xm = cc.blend64(x, cc.gray0_64(gray), z, ms, sd)
    for got, want in ((xn, g['op_x']), (xm, g['op_x_mean'])):
        assert np.abs(got.numpy() - want).max() / np.abs(want).max() <= 5e-6
    # channel 0 of the decoupled result is the perturbed gray channel, the others are the state's
    m, _ = cc.matrices64()
    d_new, d_old = cc.decouple64(xn, m), cc.decouple64(x, m)
    assert float((d_new[:, 0] - (ms * cc.gray0_64(gray)[:, 0] + sd * z[:, 0].double())).abs().max()) < 1e-12
    assert float((d_new[:, 1:] - d_old[:, 1:]).abs().max()) < 1e-12


MANGLED = [('ve_rd_lang', 'transpose'), ('ve_rd_lang', 'prior_order'), ('vp_rd_lang', 'transpose'), ('vp_rd_lang', 'prior_order'),
           ('vp_rd_lang', 'mean_old_x')]


@pytest.mark.parametrize('name,mangle', MANGLED)
def test_wrong_restatements_miss_the_bound_tenfold(name, mangle):
    """Measured here on the CPU (N = 4, sigma_max 27.7), max |x64 - ref| / scale over the bound 2e-4:

        mangling       ve_rd_lang                 vp_rd_lang
        transpose      5.72    = 28605 x bound    17.0 = 85089 x bound
        prior_order    3.19    = 15924 x bound    10.2 = 50847 x bound
        mean_old_x     6.5e-4  = 3.3 x bound      6.50 = 32495 x bound

    'mean_old_x' builds x_mean from the state that ENTERS the phase - the ``x`` argument of the reference's colorization_update_fn - and
    not from the re-imposed new x.  (The state after the update and before the re-imposition would be no mangling at all: the
    re-imposition changes channel 0 of the decoupled space only, so decouple(x_new)[1:] == decouple(x_updated)[1:] identically and
    the two x_mean agree to rounding, 2.2e-6 on ve_rd_lang.)  A denoised result is the x_mean of the LAST predictor phase alone, so
    this mangling shows as much as that one update moves the state: for VE, at t = eps, G = sigma_0 = sigma_min = 0.005 whatever
    sigma_max is, while ten bounds are 2e-3 sigma_max = 0.055 - a VE run cannot tell it apart at any sigma_max (measured over the VE
    runs: 1.6 .. 16.9 x bound, 0 where denoise is off); for VP the last update is of the size sqrt(beta_0) = 0.16 against ten bounds
    of 2e-3.  It is therefore measured on the VP run, where all three manglings are."""
    err = _err(cc.colorize64(name, mangle), name)
    print('%s / %s: %.3e of scale = %.1f x bound' % (name, mangle, err, err / BOUND))
    assert err > 10 * BOUND


def test_x_mean_from_the_updates_mean_is_caught():
    """x_mean built from the x_mean that the predictor returned - the state without the update's noise - instead of the re-imposed new
    x: the denoised result loses the last predictor's noise G z in channels 1 and 2.  Measured on vp_rd_lang (G = sqrt(beta_0) = 0.16 at
    the last step): 0.44 of scale = 2187 x bound."""
    err = _err(cc.colorize64('vp_rd_lang', 'mean_from_update'), 'vp_rd_lang')
    print('vp_rd_lang / mean_from_update: %.3e of scale = %.1f x bound' % (err, err / BOUND))
    assert err > 10 * BOUND


def test_mangles_leave_the_tape_length_alone():
    assert cc.MANGLES == ('transpose', 'prior_order', 'mean_old_x')
    for _, _, pred, corr, _, _ in cc.RUNS:
        assert len(cc.run_tape(pred, corr)) == 1 + 2 * cc.N + ((pred != 'none') + (corr != 'none')) * cc.N


# ---- 2. the default matrix --------------------------------------------------------------------------------------------------------------------
def test_default_matrix_is_orthonormal_with_the_gray_direction_first():
    m = np.array(cc.M, np.float32).astype(np.float64)
    assert np.abs(m @ m.T - np.eye(3)).max() <= 1e-6          # what csd_colorize_blend requires of a caller's matrix
    assert np.abs(m[:, 0] - 1 / np.sqrt(3)).max() < 1e-6      # decouple(gray)[0] = sqrt(3) * gray for equal channels
    g = cc.gray().double()
    d = cc.decouple64(g, torch.from_numpy(m))
    assert float(d[:, 1:].abs().max()) < 1e-6 and float((d[:, 0] - np.sqrt(3) * g[:, 0]).abs().max()) < 1e-6


# ---- 3. the draw schedule ---------------------------------------------------------------------------------------------------------------------
RULES = [(p, c) for p in (0, 1, 2) for c in (0, 1, 2) if (p, c) != (2, 2)]


def test_draw_rows_of_a_colorization_run():
    """2 n z_colorize draws (kind 5) behind the phases, a 'none' phase included, plus the sampler's own; one sequence, stream 1 + j"""
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd.sampling import fused
    from test_pc_draws_host import handle
    h, ex, _ = handle('uncond_tiny')
    assert fused.DRAW_KINDS[cc.Z_COLORIZE] == 'z_colorize' and fused.DRAW_KINDS[:5] == ('z_y0', 'z_y', 'zy', 'z', 'z_blend')
    for (p, c), n, B in ((r, n, B) for r in RULES for n in (1, 4) for B in (1, 2)):
        rows = [list(r) for r in fused.noise_draws(h._h, B, p, c, colorize=True, n_steps=n)]
        assert rows == cc.draw_rows(p != 2, c != 2, n, B * ex), (p, c, n, B)
        assert len(rows) == (2 + (p != 2) + (c != 2)) * n
        assert _lib.lib().csd_pc_noise_draws(h._h, B, p, c, 0, 0, 2, n, None, 0) == len(rows)
        # the same places as inpainting's z_blend
        blend = [list(r) for r in fused.noise_draws(h._h, B, p, c, inpaint=True, n_steps=n)]
        assert [[r[0], 4 if r[1] == cc.Z_COLORIZE else r[1]] + r[2:] for r in rows] == blend
    for pred, corr in {(r[2], r[3]) for r in cc.RUNS}:
        assert cc.n_draws(pred, corr) == len(cc.draw_rows(pred != 'none', corr != 'none', cc.N, 1))


def test_schedule_refusals_name_the_reason():
    import wide_cases as wc
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import fused
    from test_pc_draws_host import handle
    with torch.device('meta'):
        wide = mutils.create_model(wc.make_config('W2'))           # unconditional, 12 channels
    for h, words in ((handle('ddpm3d_B')[0], '3-D'), (handle('kxsr_K1')[0], 'y_scale'), (handle('paired_3_1')[0], 'unconditional networks only'),
                     (wide, 'x_channels = 12')):
        assert _lib.lib().csd_pc_noise_draws(h._h, 2, 0, 0, 0, 0, 2, 2, None, 0) == -1      # CSD_ERR_INVALID
        msg = _lib.lib().csd_last_error().decode()
        assert 'pc_colorize' in msg and words in msg, msg
        with pytest.raises(RuntimeError, match=words):
            fused.noise_draws(h._h, 2, 0, 0, colorize=True, n_steps=2)
    u = handle('uncond_tiny')[0]._h
    assert _lib.lib().csd_pc_noise_draws(u, 2, 0, 0, 0, 0, 3, 2, None, 0) == -1 and 'bad inpaint mode 3' in _lib.lib().csd_last_error().decode()
    with pytest.raises(NotImplementedError, match='exclude each other'):
        fused.noise_draws(u, 2, 0, 0, inpaint=True, colorize=True)


# ---- 4. the ABI ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, 'include', 'csd.h')).read()


def test_colorize_params_mirror_the_header():
    from conditional_score_diffusion_amd import _lib
    hdr = _header()
    body = hdr[hdr.index('typedef struct csd_pc_colorize_params {'):hdr.index('} csd_pc_colorize_params;')]
    fields = re.findall(r'^\s+(?:const )?[a-z0-9_]+\*? ([a-z0-9_A-Z]+);', body, flags=re.M)
    names = [n for n, _ in _lib.PCColorizeParams._fields_]
    assert names == fields == ['gray0', 'mean_scale', 'std', 'matrix', 'inv_matrix']
    assert ctypes.sizeof(_lib.PCColorizeParams) == 5 * ctypes.sizeof(ctypes.c_void_p)
    cp = _lib.PCColorizeParams()
    assert not cp.gray0 and not cp.mean_scale and not cp.std and not cp.matrix and not cp.inv_matrix
    for a, b in (('csd_pc_inpaint_sample', 'csd_pc_colorize_sample'), ('csd_pc_inpaint_step_begin', 'csd_pc_colorize_step_begin'),
                 ('csd_pc_inpaint_step_end', 'csd_pc_colorize_step_end')):
        assert len(_lib.SIGNATURES[b][1]) == len(_lib.SIGNATURES[a][1]) and hasattr(_lib.lib(), b)
    assert 'csd_colorize_blend' in _lib.SIGNATURES and 'csd_colorize_gray0' in _lib.SIGNATURES
    # the scratch of a colorization call is csd_pc_scratch_bytes: the header gives the name as an alias, the library has no second entry
    assert re.search(r'^#define csd_pc_colorize_scratch_bytes csd_pc_scratch_bytes$', hdr, flags=re.M)
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), 'csd_pc_colorize_scratch_bytes')


# ---- 5. dispatch ----------------------------------------------------------------------------------------------------------------------------------
def _colorizer(model_case, n_steps=1, device_loop=True):
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    model = mutils.create_model(cases.case_config(model_case)[0])
    fn = get_pc_colorizer(sde_lib.VESDE(0.01, 50., 4), get_predictor('reverse_diffusion'), get_corrector('langevin'), snr=0.15,
                          n_steps=n_steps, continuous=True, device_loop=device_loop)
    return fn, model, torch.zeros(2, 3, 16, 16)


def test_device_loop_refuses_what_it_does_not_cover():
    import wide_cases as wc
    from conditional_score_diffusion_amd.models import utils as mutils
    fn, model, gray = _colorizer('uncond_tiny')
    with pytest.raises(NotImplementedError, match='device loop runs on the GPU'):      # a CPU model: no silent fall-back
        fn(model, gray)
    fn, model, gray = _colorizer('sr3_tiny')
    with pytest.raises(NotImplementedError, match='unconditional network'):
        fn(model, gray)
    fn, model, gray = _colorizer('uncond_tiny', n_steps=2)
    with pytest.raises(NotImplementedError, match='n_steps = 2'):
        fn(model, gray)
    fn, _, gray = _colorizer('uncond_tiny')
    with pytest.raises(NotImplementedError, match='3-channel state'):
        fn(mutils.create_model(wc.make_config('W2')), gray)
    with pytest.raises(NotImplementedError, match='not a HipUNet'):
        fn(torch.nn.Identity(), gray)


@pytest.mark.parametrize('kw', [dict(noise_tape=[torch.zeros(1)]), dict(seed=3), dict(global_norm=(lambda s: None, 2))])
def test_device_loop_keywords_need_the_device_loop(kw):
    fn, model, gray = _colorizer('uncond_tiny', device_loop=False)
    with pytest.raises(NotImplementedError, match='device_loop=True'):
        fn(model, gray, **kw)


def test_inpaint_and_colorize_exclude_each_other():
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import fused
    _, model, gray = _colorizer('uncond_tiny')
    with pytest.raises(NotImplementedError, match='exclude each other'):
        fused.run(model, sde_lib.VESDE(0.01, 50., 4), tuple(gray.shape), None, 4, 0.15, 1e-3, True, inpaint=(gray, torch.ones_like(gray)),
                  colorize=gray)


def test_colorization_fn_reads_the_config_switch():
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg = cases.case_config('uncond_tiny')[0]
    sde = sde_lib.VESDE(0.01, 50., 4)
    model = mutils.create_model(cfg)
    gray = torch.zeros(2, 3, 16, 16)
    assert not cfg.sampling.get('csd_device_loop', False)             # the default stays the step-by-step loop
    with pytest.raises(NotImplementedError, match='device_loop=True'):      # ... which takes no seed
        get_colorization_fn(cfg, sde, 1e-5)(model, gray, seed=1)
    cfg.sampling.csd_device_loop = True
    with pytest.raises(NotImplementedError, match=r'get_pc_colorizer\(device_loop=True\): the model is on cpu'):
        get_colorization_fn(cfg, sde, 1e-5)(model, gray, seed=1)
