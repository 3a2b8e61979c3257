"""No GPU: NCSN++ with 9 .. 32 input channels and ncsnpp_2xSR on the host side - the fixture tests/golden/ncsnpp_wide.npz against the
CPU oracle's restatement (oracle/score_oracle.py ncsnpp_forward) on the cases of tests/ncsnpp_wide_cases.py, what csd_unet_create
accepts and refuses for arch 1, that every such network plans (inference and the training dry run) in the four precision modes, the
registry entry ncsnpp_2xSR with the reference's parameter table and its config validation, the fused loop's draw schedule on NCSN++
handles and the cascade's stage checks."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import ncsnpp_wide_cases as nw
import sr_cases as sc

PRECISIONS = ('fp32', 'fp16x3', 'fp16', 'fp16f8')
FORWARD_BOUND = 1e-4           # tests/test_wide_host.py FORWARD_BOUND: the fp32 / fp16x3 bound of the GPU forward tests


def _create(cfg):
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ncsnpp      # noqa: F401  (registers the model names)
    with torch.device('meta'):                                 # (the handle only: no parameter values)
        return mutils.create_model(cfg)


def _digest(model, B, dropout=0.0):
    """csd_unet_debug_digest: hashes the parameter table, the packed layout, the inference plan and the training dry run - it fails
    where any of them cannot be built"""
    from conditional_score_diffusion_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).csd_unet_debug_digest
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_uint64)]
    d = (ctypes.c_uint64 * 4)()
    rc = fn(model._h, B, float(dropout), d)
    return rc, [int(v) for v in d], _lib.lib().csd_last_error().decode()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# ---- the fixture and the CPU restatement agree before any GPU is involved -----------------------------------------------------------------
@pytest.mark.parametrize('case', list(nw.CASES))
def test_oracle_forward_reproduces_the_fixture(case):
    g = nw.golden()
    cfg = nw.make_config(case)
    p = nw.params(cfg)
    y = nw.case_y(case)
    for j, (x, t) in enumerate(nw.forward_inputs(case)):
        if j and case in nw.ONE_TIME_CASES:
            assert '%s_net%d' % (case, j) not in g.files
            break
        ref = torch.from_numpy(g['%s_net%d' % (case, j)])
        with torch.no_grad():
            got = nw.oracle_forward(p, case, x, y, nw.labels_of(case, cfg, t))
        e = _rel(got, ref)
        print('%s t[%d]: oracle vs fixture %.3e' % (case, j, e))
        assert tuple(ref.shape) == (nw.B, cfg.data.num_channels) + (nw.CASES[case][3],) * 2
        assert e < FORWARD_BOUND / 10, (case, j, e)
        assert '%s_score%d' % (case, j) not in g.files      # (derived: nw.score_of; the fixture tool asserts it against the reference)
        sx = nw.score_of(case, cfg, ref, t)
        assert tuple(sx.shape) == nw.shapes(case)[0]
        # ... and it is the project's own conditional score function around a network that returns the fixture's output
        from conditional_score_diffusion_amd import sde_lib
        from conditional_score_diffusion_amd.models import utils as mutils
        m = cfg.model
        sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}

        class Fixed(torch.nn.Module):
            def forward(self, d, labels):
                xc = nw.CASES[case][1]
                return {'x': sc.unsqueeze(ref[:, :xc]) if case == 'N5' else ref[:, :xc], 'y': ref[:, xc:]}
        sfn = mutils.get_conditional_score_fn(mutils.get_score_fn(sde, Fixed(), conditional=True, train=False, continuous=True), 'x')
        assert _rel(sfn(x, y, t), sx) < 1e-6


def test_fixture_holds_what_the_tool_lists():
    g = nw.golden()
    for case in nw.SAMPLER_CASES:
        assert tuple(g[case + '_pc'].shape) == nw.shapes(case)[0]
    for case in nw.TRAIN_CASES:
        assert len(g[case + '_names']) == len(g[case + '_norms']) == len(g[case + '_samples']) > 100
        assert not any(str(n).endswith('.W') and str(n).count('.') == 2 for n in g[case + '_names'])      # (the fixed Fourier matrix)
    assert tuple(g['N2_dx'].shape) == nw.shapes('N2')[0]
    assert tuple(g['bicubic_s0'].shape) == (nw.B, 3, 16, 16) and tuple(g['bicubic_s1'].shape) == (nw.B, 3, 32, 32)


# ---- the registry ----------------------------------------------------------------------------------------------------------------------
def test_ncsnpp_2xsr_is_registered_with_the_reference_parameter_table():
    """same keys, same order, same shapes as the reference NCSNpp_2xSR's state_dict (its SqueezeBlock has no parameters), which is
    that of ncsnpp_paired on 4 cx + cy channels"""
    model = _create(nw.make_config('N5'))
    assert type(model).__name__ == 'NCSNpp_2xSR' and model.x_squeeze == 1 and model.arch == 1
    assert (model.x_channels, model.y_channels, model.out_channels, model.image_size) == (12, 3, 15, 16)
    got = ['%s|%s' % (k, ','.join(map(str, v.shape))) for k, v in model.state_dict().items()]
    assert got == [str(s) for s in nw.golden()['N5_keys']]
    twin = _create(nw.make_config('N5', name='ncsnpp_paired'))
    assert [(k, tuple(v.shape)) for k, v in twin.state_dict().items()] == [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert model._x_shape(2) == (2, 3, 32, 32) and model._y_shape(2) == (2, 3, 16, 16)


def test_ncsnpp_2xsr_validates_its_shapes_like_ddpm_2xsr():
    for key, val in (('shape_x', [3, 30, 30]), ('shape_y', [3, 8, 8]), ('effective_image_size', 32), ('shape_x', [3, 32, 16])):
        cfg = nw.make_config('N5')
        cfg.data[key] = val
        with pytest.raises(ValueError, match=r'ncsnpp_2xSR: the image side'):
            _create(cfg)
    cfg = sc.make_config('R1')                     # (the same refusal under the DDPM name, with its own name in the message)
    cfg.data.shape_y = [3, 8, 8]
    with pytest.raises(ValueError, match=r'ddpm_2xSR: the image side'):
        _create(cfg)


def test_the_operator_twin_refuses_the_squeeze():
    model = _create(nw.make_config('N5'))
    model.train_executor = 'operators'
    with pytest.raises(NotImplementedError, match='planned graph only'):
        model._train_forward(None, None, None)


# ---- what csd_unet_create accepts and refuses for arch 1 ---------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
def test_nine_to_thirty_two_channels_create_and_plan(precision):
    """every channel count above the old limit, split x | y in two ways, over the pyramid options: parameter table, packed layout,
    inference plan and the training dry run all build"""
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    opts = [dict(), dict(progressive_input='residual'), dict(progressive='none', progressive_input='none', embedding_type='positional'),
            dict(progressive_input='residual', fir=False, progressive='none', embedding_type='positional')]
    seen = set()
    for c in range(9, 33):
        S, nf = (16, 64) if c % 2 else (20, 32)
        cfg = cases.make_ncsnpp_config(channels=c, nf=nf, ch_mult=(1, 2), attn_resolutions=(S // 2,), image_size=S, **opts[c % 4])
        cfg.model.csd_precision = precision
        for name, xc in (('ncsnpp_paired', c - 3), ('ncsnpp_paired', c // 2)):
            cfg.model.name = name
            cfg.data.shape_x, cfg.data.shape_y = [xc, S, S], [c - xc, S, S]
            model = _create(cfg)
            assert (model.x_channels, model.y_channels, model.out_channels) == (xc, c - xc, c)
            rc, d, msg = _digest(model, 2, 0.1)
            assert rc == 0, (name, c, precision, msg)
            assert l.csd_unet_workspace_bytes(model._h, 3) > 0 and l.csd_unet_packed_bytes(model._h) > 0
            assert l.csd_pc_scratch_bytes(model._h, 2) > 0 and l.csd_unet_train_workspace_bytes(model._h, 2, 0.0) > 0
            seen.add(tuple(d[1:]))
    assert len(seen) == 24                         # (layout, plan and training graph follow the channel count; the x | y split does not)


def _paired(channels, xc):
    cfg = cases.make_ncsnpp_config(name='ncsnpp_paired', channels=channels)
    cfg.data.shape_x, cfg.data.shape_y = [xc, 16, 16], [channels - xc, 16, 16]
    return cfg


def test_thirty_three_channels_are_refused_naming_the_limit():
    with pytest.raises(RuntimeError, match=r'ncsnpp: x\+y channels must be <= 32'):
        _create(_paired(33, 17))
    _create(_paired(32, 16))
    _create(_paired(9, 6))


def test_the_unconditional_network_keeps_its_limit():
    """more than 8 channels and x_squeeze are provided for the paired networks (y_channels > 0); ``ncsnpp`` without a condition keeps
    the limit and the message that tests/test_wide_host.py pins, and says where the wider networks are"""
    with pytest.raises(RuntimeError, match=r'ncsnpp: x\+y channels must be <= 8 for a network without a condition \(got 12; the paired'):
        _create(cases.make_ncsnpp_config(channels=12))
    _create(cases.make_ncsnpp_config(channels=8))


def test_x_squeeze_keeps_the_ddpm_conditions_and_kx_its_limit():
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    model = _create(nw.make_config('N5'))
    cfg = _lib.UNetConfig.from_buffer_copy(model._cfg)
    for field, val, msg in (('x_channels', 10, r'x_squeeze needs x_channels % 4 == 0'), ('x_squeeze', 2, 'x_squeeze must be 0 or 1')):
        bad = _lib.UNetConfig.from_buffer_copy(cfg)
        setattr(bad, field, val)
        if field == 'x_channels':
            bad.y_channels = 5
        h = ctypes.c_void_p()
        assert l.csd_unet_create(ctypes.byref(bad), ctypes.byref(h)) != 0
        assert __import__('re').search(msg, l.csd_last_error().decode()), l.csd_last_error().decode()
    bad = _lib.UNetConfig.from_buffer_copy(cfg)
    bad.x_channels, bad.y_channels, bad.out_channels = 4, 0, 4      # (no condition: arch 1 takes the squeeze for the paired networks)
    h = ctypes.c_void_p()
    assert l.csd_unet_create(ctypes.byref(bad), ctypes.byref(h)) != 0
    assert 'arch 1' in l.csd_last_error().decode() and 'y_channels > 0' in l.csd_last_error().decode()
    bad = _lib.UNetConfig.from_buffer_copy(cfg)
    bad.x_squeeze, bad.y_scale = 0, 2              # ncsnpp_KxSR stays at up to 8 assembled channels
    h = ctypes.c_void_p()
    assert l.csd_unet_create(ctypes.byref(bad), ctypes.byref(h)) != 0 and 'up to 8 assembled channels' in l.csd_last_error().decode()


@pytest.mark.parametrize('case', list(nw.CASES))
def test_cases_create_in_every_precision_and_size_their_scratch(case):
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    _, xc, yc, S = nw.CASES[case][:4]
    for precision in PRECISIONS:
        model = _create(nw.make_config(case, precision))
        rc, d, msg = _digest(model, nw.B, 0.0) if case != 'N5' else (0, None, '')      # (a squeezed handle has no digest: plan_digest.h)
        assert rc == 0, (case, precision, msg)
        assert l.csd_unet_workspace_bytes(model._h, nw.B) > 0
        assert l.csd_unet_train_workspace_bytes(model._h, nw.B, 0.0) > 0
        hw, oc = S * S, model.out_channels
        floats = lambda n: (n + 63) // 64 * 64      # noqa: E731  (tests/test_wide_host.py: the layout of the PC scratch)
        want = 4 * (floats(nw.B * oc * hw) + 2 * floats(nw.B * xc * hw) + 2 * floats(nw.B * max(yc, 1) * hw) + floats(nw.B))
        assert l.csd_pc_scratch_bytes(model._h, nw.B) == want + nw.B * 64 * 2 * 8 + 256


# ---- the fused loop's draw schedule and the cascade's stage checks on NCSN++ handles -----------------------------------------------------
def test_noise_draws_of_ncsnpp_handles():
    """csd_pc_noise_draws (host only): the two-SDE schedule of N1 / N5 (N5: x draws at the image's size = the squeezed size), two
    draws per phase, in tape order"""
    from conditional_score_diffusion_amd.sampling import fused
    for case in ('N1', 'N5'):
        model = _create(nw.make_config(case))
        (_, *xs), (_, *ys) = nw.shapes(case)
        ex, ey = int(np.prod(xs)), int(np.prod(ys))
        rows = fused.noise_draws(model._h, nw.B, 0, 0, std_y=True, n_steps=nw.P_STEPS)
        assert [r[3] for r in rows] == [nw.B * ey, nw.B * ex] * (2 * nw.P_STEPS)
        assert len(rows) == len(nw.pc_tape(case)) - 1
        offs = np.cumsum([0] + [r[3] for r in rows[:-1]])
        assert [r[4] for r in rows] == list(offs)
    with pytest.raises(RuntimeError, match='x_squeeze'):            # inpainting on a squeezed handle stays refused
        fused.noise_draws(_create(nw.make_config('N5'))._h, nw.B, 0, 0, inpaint=True, n_steps=2)


def _stages(flow, order=(0, 1)):
    from conditional_score_diffusion_amd import sde_lib
    out = []
    for k in order:
        cfg = nw.stage_config(flow, k)
        m = cfg.model
        sde = {'x': sde_lib.cVESDE(m.sigma_min_x, m.sigma_max_x, m.num_scales), 'y': sde_lib.VESDE(m.sigma_min_y, m.sigma_max_y, m.num_scales)}
        out.append((_create(cfg), sde, cfg))
    return out


@pytest.mark.parametrize('flow', list(nw.CASCADE_STAGES))
def test_cascade_accepts_ncsnpp_stages_for_the_one_call(flow):
    """get_autoregressive_sampler(one_call=True) refuses at construction whatever does not depend on where the models lie: NCSN++
    stages, alone and beside a DDPM stage, pass in the two conditional coordinate spaces; a wrong order is still named"""
    from conditional_score_diffusion_amd.sampling import cascade
    space = nw.CASCADE_SPACE[flow]
    p_steps = nw.P_STEPS
    stages = _stages(flow)
    assert callable(cascade.get_autoregressive_sampler(stages, space, p_steps=p_steps, one_call=True))
    for (model, sde, cfg) in stages:
        st = cascade._settings(0, sde, cfg, space, 'default', 'default', p_steps, 'default')
        assert cascade._why_not_one_call(model, sde, st, False, check_device=False) is None
    with pytest.raises(ValueError, match='low-to-high order'):
        cascade.get_autoregressive_sampler(stages[::-1], space, p_steps=p_steps, one_call=True)


def test_cascade_still_refuses_kx_and_3d_stages_and_no_longer_names_ncsnpp():
    import inspect
    import kxsr_cases
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import cascade
    from conditional_score_diffusion_amd.sampling.correctors import get_corrector
    from conditional_score_diffusion_amd.sampling.predictors import get_predictor
    st = dict(predictor=get_predictor('conditional_reverse_diffusion'), corrector=get_corrector('conditional_langevin'), c_steps=1,
              probability_flow=False, continuous=True)
    sde = {'x': sde_lib.cVESDE(5e-3, 10., 1000), 'y': sde_lib.VESDE(5e-3, 1., 1000)}
    why = cascade._why_not_one_call(_create(kxsr_cases.make_config('K1')), sde, st, False, check_device=False)
    assert why is not None and 'Kx' in why
    why = cascade._why_not_one_call(torch.nn.Linear(1, 1), sde, st, False, check_device=False)
    assert '3-D stages are out of scope' in why and 'NCSN++ and' not in why
    assert 'NCSN++ and 3-D' not in inspect.getsource(cascade._why_not_one_call)
