"""No GPU: the direct Kx super-resolution networks (ddpm_KxSR, ncsnpp_KxSR; csd_unet_config.y_scale) on the host side - the registered
names, the paired classes' parameter tables, what construction and csd_unet_create refuse, that a zeroed y_scale leaves today's networks
alone, the sizes of the low-resolution y draws on a noise tape, that the cases of tests/kxsr_cases.py plan in the four precision modes -
and the fixture itself: the reference's fp32 outputs lie within 1e-5 of a float64 restatement (which pins the resize of the golden
tool's torchvision stand-in: torch's bilinear, align_corners=False, no antialias), restatements with a WRONG resize
(align_corners=True; nearest) miss that bound by more than 100x, and the two closed forms of the integer downsample (the mean of the
2 x 2 centre block for even K, the centre pixel for odd K) equal F.interpolate."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kxsr_cases as kc
from test_sr_host import _create, _digest, _raw_create, _rel

PRECISIONS = ('fp32', 'fp16x3', 'fp16', 'fp16f8')
RESTATEMENT_BOUND = 1e-5      # fp32 reference against its float64 restatement (tools/make_kxsr_goldens.py measures 1.0e-6 .. 2.3e-6)


def test_registered():
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ddpm as ddpm
    import conditional_score_diffusion_amd.models.ncsnpp as ncsnpp
    assert mutils.get_model('ddpm_KxSR') is ddpm.DDPM_KxSR
    assert mutils.get_model('ncsnpp_KxSR') is ncsnpp.NCSNpp_KxSR
    for case, (name, cx, cy, S, K, nf, ch_mult, attn, centered) in kc.CASES.items():
        model = _create(kc.make_config(case))
        assert type(model) is mutils.get_model(name)
        assert (model.x_channels, model.y_channels, model.out_channels, model.image_size) == (cx, cy, cx + cy, S)
        assert model.y_scale == K and model._cfg.y_scale == K and model._cfg.x_squeeze == 0
        assert model._cfg.arch == (0 if name == 'ddpm_KxSR' else 1)
        s = S // K
        assert model._x_shape(3) == (3, cx, S, S) and model._y_shape(3) == (3, cy, s, s)
        assert model._out_shape(3) == (3, cx * S * S + cy * s * s)
        # the low-resolution side comes from target_resolution // scale: data.shape_y of the direct configs still names S
        assert list(kc.make_config(case).data.shape_y[1:]) == [S, S]


@pytest.mark.parametrize('case', list(kc.CASES))
def test_state_dict_keys_are_the_paired_classes(case):
    """no parameters beyond ddpm_paired / ncsnpp_paired: same keys in the same order, same shapes (the reference's Resize modules hold
    none either - tools/make_kxsr_goldens.py asserts that on the imported classes); the seeded weights load"""
    cfg = kc.make_config(case)
    model = _create(cfg, meta=False)
    twin = _create(kc.make_config(case, twin=True), meta=False)
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == [(k, tuple(v.shape)) for k, v in twin.state_dict().items()]
    if cfg.model.name == 'ddpm_KxSR':
        import score_oracle as so
        want = so.ddpm_param_shapes(so.NetCfg.from_config(cfg))
        assert dict(got) == want and [k for k, _ in got] == list(want)
    if case == kc.TRAIN_CASE:
        assert list(kc.golden()[case + '_names']) == [k for k, _ in model.named_parameters()]
    res = model.load_state_dict(kc.params(cfg, dict(got)))
    assert not res.missing_keys and not res.unexpected_keys


def test_constructor_refuses_extents_that_do_not_match_naming_them():
    for case in ('K1', 'K4'):
        name = kc.CASES[case][0]
        for edit in ('target', 'eff', 'shape', 'scale1', 'scale3'):
            cfg = kc.make_config(case)
            d = cfg.data
            if edit == 'target':
                d.target_resolution = 32
                match = r'%s: data.target_resolution = 32.*effective_image_size = 16.*shape_x' % name
            elif edit == 'eff':
                d.effective_image_size = 8
                match = r'%s: data.target_resolution = 16.*effective_image_size = 8' % name
            elif edit == 'shape':
                d.shape_x = [3, 16, 12]
                match = r'%s: .*shape_x\[1:\] = \[16, 12\]' % name
            elif edit == 'scale1':
                d.scale = 1
                match = r'%s: data.scale = 1 must be at least 2' % name
            else:
                d.scale = 3
                match = r'%s: data.scale = 3 must divide data.target_resolution = 16' % name
            with pytest.raises(ValueError, match=match):
                _create(cfg)


def test_library_refuses_y_scale_where_it_does_not_apply():
    ok = dict(x_channels=3, y_channels=3, out_channels=6)
    rc, msg = _raw_create(y_scale=4, **ok)
    assert rc == 0, msg
    rc, msg = _raw_create(y_scale=3, image_size=24, ch_mult=(1, 2), **ok)
    assert rc == 0, msg
    rc, msg = _raw_create(y_scale=1, **ok)
    assert rc != 0 and 'y_scale' in msg
    rc, msg = _raw_create(y_scale=-2, **ok)
    assert rc != 0 and 'y_scale' in msg
    rc, msg = _raw_create(y_scale=3, **ok)                                  # 16 % 3
    assert rc != 0 and 'y_scale' in msg and 'image_size' in msg
    rc, msg = _raw_create(y_scale=2, x_channels=3, y_channels=0, out_channels=3)
    assert rc != 0 and 'y_scale' in msg and 'y_channels' in msg
    rc, msg = _raw_create(y_scale=2, x_squeeze=1, x_channels=4, y_channels=1, out_channels=5)
    assert rc != 0 and 'y_scale' in msg and 'x_squeeze' in msg
    rc, msg = _raw_create(y_scale=2, x_channels=6, y_channels=3, out_channels=9)
    assert rc != 0 and 'y_scale' in msg and '6 + 3' in msg
    rc, msg = _raw_create(x_channels=6, y_channels=3, out_channels=9)       # (fine without the field)
    assert rc == 0, msg
    # arch 1 takes it, arch 2 does not - each on a configuration it accepts without the field
    ncsnpp = dict(arch=1, nf=16, x_channels=3, y_channels=3, out_channels=6, n_fir=4, fir_kernel=(1., 3., 3., 1.), embedding_type=0)
    rc, msg = _raw_create(**ncsnpp)
    assert rc == 0, msg
    rc, msg = _raw_create(y_scale=2, **ncsnpp)
    assert rc == 0, msg
    vol = dict(arch=2, resamp_with_conv=0, x_channels=2, y_channels=2, out_channels=4, vol=(8, 8, 8))
    rc, msg = _raw_create(**vol)
    assert rc == 0, msg
    rc, msg = _raw_create(y_scale=2, **vol)
    assert rc != 0 and 'y_scale' in msg and 'arch 2' in msg


def test_a_zeroed_field_keeps_todays_networks():
    """y_scale is 0 in a zero-initialised struct: a caller that never heard of it passes 0 (it stands in front of vol and x_squeeze, which
    tests/test_sr_host.py pins as the last two fields).  The twin of every case is today's paired network (its
    digest is the one a handle made without the adapter setting the field has), the KxSR handle shares its parameter table and packed
    size, and has no digest of its own"""
    from conditional_score_diffusion_amd import _lib
    names = [f[0] for f in _lib.UNetConfig._fields_]
    assert names[-3:] == ['y_scale', 'vol', 'x_squeeze']
    assert _lib.UNetConfig().y_scale == 0
    l = _lib.lib()
    for case in kc.CASES:
        twin = _create(kc.make_config(case, 'fp16x3', twin=True))
        assert twin._cfg.y_scale == 0 and twin.y_scale == 0
        rc, d, msg = _digest(twin, kc.B, 0.1)
        assert rc == 0, msg
        kx = _create(kc.make_config(case, 'fp16x3'))
        assert l.csd_unet_packed_bytes(kx._h) == l.csd_unet_packed_bytes(twin._h)
        assert kx._param_table() == twin._param_table()
        rc, _, msg = _digest(kx, kc.B, 0.1)
        assert rc != 0 and 'y_scale' in msg


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(kc.CASES))
def test_cases_plan_in_every_precision(case, precision):
    """inference plan (+ the head's full-resolution tensor), PC scratch and the training dry run"""
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    name, cx, cy, S = kc.CASES[case][:4]
    kx = _create(kc.make_config(case, precision))
    twin = _create(kc.make_config(case, precision, twin=True))
    for B in (1, kc.B, 3):
        ws = l.csd_unet_workspace_bytes(kx._h, B)
        assert ws >= 4 * B * (cx + cy) * S * S, l.csd_last_error().decode()
        assert 0 < l.csd_pc_scratch_bytes(kx._h, B) <= l.csd_pc_scratch_bytes(twin._h, B)
        assert l.csd_unet_train_workspace_bytes(kx._h, B, 0.0) >= l.csd_unet_train_workspace_bytes(twin._h, B, 0.0) > 0


def test_tape_lengths_count_low_resolution_y_draws():
    """the draw ORDER of a tape is the paired networks' (prior; per step and phase z_y, z_x - use_path: z_y0; per step z_y, z_x, z_x);
    each y draw has cy (S / K)^2 elements per sample, each x draw cx S^2"""
    for case, (name, cx, cy, S, K, *_) in kc.CASES.items():
        s = S // K
        nx, ny = kc.B * cx * S * S, kc.B * cy * s * s
        tape = kc.pc_tape(case)
        assert len(tape) == 1 + 4 * kc.P_STEPS
        assert [t.numel() for t in tape] == [nx] + [ny, nx, ny, nx] * kc.P_STEPS
        assert sum(t.numel() for t in tape[1:]) == kc.tape_floats(case) == kc.P_STEPS * 2 * (nx + ny)
        path = kc.path_tape(case)
        assert [t.numel() for t in path] == [nx, ny] + [ny, nx, nx] * kc.P_STEPS
        assert sum(t.numel() for t in path[1:]) == kc.tape_floats(case, use_path=True)
        assert tuple(tape[1].shape) == kc.shapes(case)[1] == (kc.B, cy, s, s)


# ---- the resize: closed forms of the integer downsample, and the formula of the upsample ------------------------------------------------
@pytest.mark.parametrize('K', [2, 3, 4, 5, 8])
def test_downsample_identities_against_interpolate(K):
    """for an integer K every output pixel of the bilinear resize S -> S / K (align_corners=False, no antialias) is the mean of the
    2 x 2 block at rows / columns K i + K / 2 - 1, K i + K / 2 (K even) or the pixel K i + (K - 1) / 2 (K odd)"""
    rs = np.random.RandomState(K)
    for s in (1, 3, 4):
        S = s * K
        v = torch.from_numpy(rs.standard_normal((2, 3, S, S)))
        ref = F.interpolate(v, size=(s, s), mode='bilinear', align_corners=False)
        if K % 2:
            c = (K - 1) // 2
            mine = v[:, :, c::K, c::K]
        else:
            a = K // 2 - 1
            mine = 0.25 * (v[:, :, a::K, a::K] + v[:, :, a::K, a + 1::K] + v[:, :, a + 1::K, a::K] + v[:, :, a + 1::K, a + 1::K])
        assert tuple(mine.shape) == tuple(ref.shape)
        assert float((mine - ref).abs().max()) < 1e-14


@pytest.mark.parametrize('K', [2, 3, 4, 8])
def test_upsample_taps_in_exact_integers(K):
    """the library's taps: source coordinate max((o + 0.5) / K - 0.5, 0) = max(2 o + 1 - K, 0) / (2 K); i0 its integer quotient,
    the weight of i1 = min(i0 + 1, s - 1) the remainder over 2 K - against F.interpolate in float64"""
    rs = np.random.RandomState(10 + K)
    for s in (1, 2, 5):
        y = torch.from_numpy(rs.standard_normal((1, 2, s, s)))
        S = s * K
        num = np.maximum(2 * np.arange(S) + 1 - K, 0)
        i0 = num // (2 * K)
        w1 = torch.from_numpy((num - i0 * 2 * K) / (2.0 * K))
        i1 = np.minimum(i0 + 1, s - 1)
        rows = y[:, :, i0, :] * (1 - w1)[None, None, :, None] + y[:, :, i1, :] * w1[None, None, :, None]
        mine = rows[:, :, :, i0] * (1 - w1) + rows[:, :, :, i1] * w1
        ref = F.interpolate(y, size=(S, S), mode='bilinear', align_corners=False)
        assert float((mine - ref).abs().max()) < 1e-14


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(kc.CASES))
def test_restatement_is_within_bound_and_a_wrong_resize_is_not(case):
    g = kc.golden()
    cfg = kc.make_config(case)
    model = _create(cfg)
    p = kc.params(cfg, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    y = kc.case_y(case)
    for j, (x, t) in enumerate(kc.forward_inputs(case)):
        rx, ry = torch.from_numpy(g['%s_x%d' % (case, j)]), torch.from_numpy(g['%s_y%d' % (case, j)])
        assert tuple(rx.shape) == tuple(x.shape) and tuple(ry.shape) == tuple(y.shape)
        labels = kc.labels_of(cfg, t)
        with torch.no_grad():
            ox, oy = kc.forward64(p, case, x, y, labels)
            ex, ey = _rel(rx, ox), _rel(ry, oy)
            print('%s t[%d] ref: x %.3e, y %.3e' % (case, j, ex, ey))
            assert ex < RESTATEMENT_BOUND and ey < RESTATEMENT_BOUND, (case, j, ex, ey)
            for how in kc.RESIZES[1:]:
                wx, wy = kc.forward64(p, case, x, y, labels, how=how)
                ex, ey = _rel(wx, rx), _rel(wy, ry)
                print('%s t[%d] %s: x %.3e, y %.3e' % (case, j, how, ex, ey))
                assert max(ex, ey) > 100 * RESTATEMENT_BOUND, (case, j, how, ex, ey)


def test_fixture_holds_outputs_only_and_stays_small():
    g = kc.golden()
    assert os.path.getsize(kc.GOLDEN) < 1 << 20
    want = set()
    for case in kc.CASES:
        want |= {'%s_%s%d' % (case, k, j) for k in 'xy' for j in range(len(kc.FORWARD_TIMES))}
        want |= {case + '_sx', case + '_sy'}
    want |= {c + '_pc' for c in kc.SAMPLER_CASES} | {kc.PATH_CASE + '_path'}
    want |= {kc.TRAIN_CASE + s for s in ('_loss', '_names', '_norms', '_samples', '_dx')}
    assert set(g.files) == want
    for c in kc.SAMPLER_CASES:
        assert tuple(g[c + '_pc'].shape) == kc.shapes(c)[0]
    for c in kc.CASES:
        assert tuple(g[c + '_sx'].shape) == kc.shapes(c)[0] and tuple(g[c + '_sy'].shape) == kc.shapes(c)[1]
    assert np.isfinite(g[kc.TRAIN_CASE + '_loss']) and tuple(g[kc.TRAIN_CASE + '_dx'].shape) == kc.shapes(kc.TRAIN_CASE)[0]
