"""No GPU: the 2x super-resolution networks (ddpm_2xSR, csd_unet_config.x_squeeze) on the host side - the registered name, the
reference's parameter table, what construction and csd_unet_create refuse, that a zeroed x_squeeze leaves today's networks alone, that
the cases of tests/sr_cases.py plan in the four precision modes - and the fixture itself: the reference's fp32 outputs lie within the
GPU tests' forward bound of a float64 restatement behind squeeze / unsqueeze, and restatements with a WRONG squeeze order (dy and dx
swapped; 4 * (2dy + dx) + c) miss that bound by more than 10x, so the fixture tells the orders apart."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import sr_cases as sc

PRECISIONS = ('fp32', 'fp16x3', 'fp16', 'fp16f8')
FORWARD_BOUND = 1e-4          # tests/test_gpu_sr.py (tests/test_gpu_wide.py: NET_TOL of fp32 / fp16x3)


def _create(cfg, meta=True):
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ncsnpp      # noqa: F401  (registers the model names)
    if not meta:
        return mutils.create_model(cfg)
    with torch.device('meta'):                                 # (the handle only: no parameter values)
        return mutils.create_model(cfg)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _raw_create(**fields):
    """csd_unet_create on a zero-initialised csd_unet_config with the given fields -> (status, message)"""
    from conditional_score_diffusion_amd import _lib
    cfg = _lib.UNetConfig()
    base = dict(nf=32, n_levels=2, num_res_blocks=1, image_size=16, x_channels=4, y_channels=1, out_channels=5, resamp_with_conv=1,
                conditional=1, act=_lib.ACT_IDS['swish'])
    base.update(fields)
    for k, v in base.items():
        if k == 'ch_mult':
            for i, m in enumerate(v):
                cfg.ch_mult[i] = m
        elif k == 'vol':
            for i, m in enumerate(v):
                cfg.vol[i] = m
        elif k == 'fir_kernel':
            for i, m in enumerate(v):
                cfg.fir_kernel[i] = m
        else:
            setattr(cfg, k, v)
    if 'ch_mult' not in base:
        cfg.ch_mult[0], cfg.ch_mult[1] = 1, 2
    h = ctypes.c_void_p()
    l = _lib.lib()
    rc = l.csd_unet_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = l.csd_last_error().decode()
    if rc == 0:
        l.csd_unet_destroy(h)
    return rc, msg


def test_the_name_registers_and_the_adapter_reports_the_network_side():
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ddpm as ddpm
    assert mutils.get_model('ddpm_2xSR') is ddpm.DDPM_2xSR
    for case, (cx, cy, S, nf, ch_mult, attn, centered) in sc.CASES.items():
        model = _create(sc.make_config(case))
        assert (model.x_channels, model.y_channels, model.out_channels, model.image_size) == (4 * cx, cy, 4 * cx + cy, S)
        assert model.x_squeeze == 1 and model._cfg.x_squeeze == 1
        assert model._x_shape(3) == (3, cx, 2 * S, 2 * S)
        assert model._out_shape(3) == (3, (4 * cx + cy) * S * S)


@pytest.mark.parametrize('case', list(sc.CASES))
def test_parameter_table_is_the_references(case):
    """keys and shapes equal the reference DDPM_2xSR's state_dict (tools/make_sr_goldens.py asserts score_oracle.ddpm_param_shapes
    against it; the fixture keeps the reference's parameter names of R1), and synthetic weights of those shapes load"""
    import score_oracle as so
    cfg = sc.make_config(case)
    model = _create(cfg, meta=False)
    want = so.ddpm_param_shapes(so.NetCfg.from_config(cfg))
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == want and list(got) == list(want)
    if case == sc.TRAIN_CASE:
        assert list(sc.golden()[case + '_names']) == [k for k, _ in model.named_parameters()]
    res = model.load_state_dict(sc.params(cfg))
    assert not res.missing_keys and not res.unexpected_keys
    # the squeeze has no parameters: the unsqueezed twin on 4c + cy channels has the same table
    twin = _create(sc.make_config(case, name='ddpm_paired'))
    assert {k: tuple(v.shape) for k, v in twin.state_dict().items()} == got


def test_extents_that_do_not_match_are_refused_naming_them():
    for edit in ('x', 'y', 'eff'):
        cfg = sc.make_config('R1')
        if edit == 'x':
            cfg.data.shape_x = [3, 48, 48]
        elif edit == 'y':
            cfg.data.shape_y = [3, 8, 8]
        else:
            cfg.data.effective_image_size = 32
        hi, S, lo = cfg.data.shape_x[1], cfg.data.effective_image_size, cfg.data.shape_y[1]
        with pytest.raises(ValueError, match=r'shape_x\[1\] = %d .*effective_image_size = %d .*shape_y\[1\] = %d' % (hi, S, lo)):
            _create(cfg)


def test_library_refuses_x_squeeze_where_it_does_not_apply():
    rc, msg = _raw_create(x_squeeze=1)
    assert rc == 0, msg
    rc, msg = _raw_create(x_squeeze=1, x_channels=6, out_channels=7)
    assert rc != 0 and 'x_squeeze' in msg and 'x_channels' in msg and '6' in msg
    rc, msg = _raw_create(x_squeeze=2)
    assert rc != 0 and 'x_squeeze' in msg
    rc, msg = _raw_create(x_squeeze=1, out_channels=3)
    assert rc != 0 and 'x_squeeze' in msg and 'out_channels' in msg
    # arch 1 (NCSN++) and arch 2 (the 3-D family), each on a configuration it accepts without the field
    ncsnpp = dict(arch=1, nf=16, x_channels=4, y_channels=0, out_channels=4, n_fir=4, fir_kernel=(1., 3., 3., 1.), embedding_type=0)
    rc, msg = _raw_create(**ncsnpp)
    assert rc == 0, msg
    rc, msg = _raw_create(x_squeeze=1, **ncsnpp)
    assert rc != 0 and 'x_squeeze' in msg and 'arch 1' in msg
    vol = dict(arch=2, resamp_with_conv=0, x_channels=4, y_channels=0, out_channels=4, vol=(8, 8, 8))
    rc, msg = _raw_create(**vol)
    assert rc == 0, msg
    rc, msg = _raw_create(x_squeeze=1, **vol)
    assert rc != 0 and 'x_squeeze' in msg and 'arch 2' in msg


def _digest(model, B, dropout=0.0):
    from conditional_score_diffusion_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).csd_unet_debug_digest
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_uint64)]
    d = (ctypes.c_uint64 * 4)()
    rc = fn(model._h, B, float(dropout), d)
    return rc, [int(v) for v in d], _lib.lib().csd_last_error().decode()


def test_a_zeroed_field_keeps_todays_networks():
    """x_squeeze trails the struct: a caller that never heard of it passes 0.  The unsqueezed twin of every case is today's ddpm_paired
    (same digest whether the adapter sets the field to 0 or a raw zero-initialised struct is used), and the squeezed handle shares its
    parameter table and packed size - the squeeze changes addressing at the boundary only"""
    from conditional_score_diffusion_amd import _lib
    assert _lib.UNetConfig._fields_[-1][0] == 'x_squeeze' and _lib.UNetConfig._fields_[-2][0] == 'vol'
    assert _lib.UNetConfig().x_squeeze == 0
    for case in sc.CASES:
        twin = _create(sc.make_config(case, 'fp16x3', name='ddpm_paired'))
        assert twin._cfg.x_squeeze == 0
        rc, d, msg = _digest(twin, sc.B, 0.1)
        assert rc == 0, msg
        sq = _create(sc.make_config(case, 'fp16x3'))
        l = _lib.lib()
        assert l.csd_unet_packed_bytes(sq._h) == l.csd_unet_packed_bytes(twin._h)
        assert sq._param_table() == twin._param_table()
        rc, _, msg = _digest(sq, sc.B, 0.1)
        assert rc != 0 and 'x_squeeze' in msg


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(sc.CASES))
def test_cases_plan_in_every_precision(case, precision):
    """inference plan, PC scratch and the training dry run; every per-sample element count is the unsqueezed network's, so the sizes are"""
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    sq = _create(sc.make_config(case, precision))
    twin = _create(sc.make_config(case, precision, name='ddpm_paired'))
    for B in (1, sc.B, 3):
        assert l.csd_unet_workspace_bytes(sq._h, B) > 0, l.csd_last_error().decode()
        assert l.csd_pc_scratch_bytes(sq._h, B) == l.csd_pc_scratch_bytes(twin._h, B) > 0
        tw = l.csd_unet_train_workspace_bytes(sq._h, B, 0.0)
        assert tw >= l.csd_unet_train_workspace_bytes(twin._h, B, 0.0) > 0      # (+ the squeezed copies of out, d_out, d_x)


# ---- the fixture: within the bound of the float64 restatement, and sensitive to the channel order of the squeeze -----------------------
def test_squeeze_restatement_is_the_references_order():
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).reshape(2, 3, 4, 6)
    z = sc.squeeze(x)
    for c in range(3):
        for dy in range(2):
            for dx in range(2):
                assert torch.equal(z[:, 4 * c + 2 * dy + dx], x[:, c, dy::2, dx::2])
    for order in sc.ORDERS:
        assert torch.equal(sc.unsqueeze(sc.squeeze(x, order), order), x)
    assert not torch.equal(sc.squeeze(x, 'swap'), z) and not torch.equal(sc.squeeze(x, 'cmajor'), z)


@pytest.mark.parametrize('case', list(sc.CASES))
def test_forward_bound_passes_the_reference_and_catches_a_wrong_squeeze_order(case):
    g = sc.golden()
    cfg = sc.make_config(case)
    p = sc.params(cfg)
    y = sc.case_y(case)
    # (one image channel: 4 * (2dy + dx) + c IS the reference's order)
    wrong = ('swap', 'cmajor') if sc.CASES[case][0] > 1 else ('swap',)
    for j, (x, t) in enumerate(sc.forward_inputs(case)):
        rx, ry = torch.from_numpy(g['%s_x%d' % (case, j)]), torch.from_numpy(g['%s_y%d' % (case, j)])
        assert tuple(rx.shape) == tuple(x.shape) and tuple(ry.shape) == tuple(y.shape)
        labels = sc.labels_of(cfg, t)
        with torch.no_grad():
            ox, oy = sc.forward64(p, case, x, y, labels)
            assert _rel(rx, ox) < FORWARD_BOUND and _rel(ry, oy) < FORWARD_BOUND
            for order in wrong:
                wx, wy = sc.forward64(p, case, x, y, labels, order=order)
                ex, ey = _rel(wx, rx), _rel(wy, ry)
                print('%s t[%d] %s: x %.3e, y %.3e' % (case, j, order, ex, ey))
                assert ex > 10 * FORWARD_BOUND and ey > 10 * FORWARD_BOUND, (case, j, order, ex, ey)


def test_fixture_holds_outputs_only_and_stays_small():
    import os
    g = sc.golden()
    assert os.path.getsize(sc.GOLDEN) < 1 << 20
    want = set()
    for case in sc.CASES:
        want |= {'%s_%s%d' % (case, k, j) for k in 'xy' for j in range(len(sc.FORWARD_TIMES))}
    want |= {c + '_pc' for c in sc.SAMPLER_CASES} | {sc.PATH_CASE + '_path'}
    want |= {sc.TRAIN_CASE + s for s in ('_loss', '_names', '_norms', '_samples')}
    assert set(g.files) == want
    for c in sc.SAMPLER_CASES:
        assert tuple(g[c + '_pc'].shape) == sc.shapes(c)[0]
    assert np.isfinite(g[sc.TRAIN_CASE + '_loss'])
