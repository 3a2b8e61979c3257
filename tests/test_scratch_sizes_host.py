"""No GPU: every csd_*_bytes entry of the ABI returns, over a fixed grid of arguments, the byte count pinned in
tests/golden/scratch_sizes.json (recorded by tools/make_scratch_sizes.py on the commit that file names).  The scratch layouts of
csrc/ (ScratchCarver, common.h) may be rewritten freely; what a caller has to allocate may not change unnoticed - zeros (arguments an
entry refuses) included.  Also here: GroupNorm refuses more groups than its size query covers."""
import ctypes
import itertools
import json
import os

import torch

import cases
import ddpm3d_cases
import kxsr_cases
import sr_cases
import wide_cases
from test_host_logic import _DIGEST_BATCHES, _digest_configs

PRECISIONS = ('fp32', 'fp16x3', 'fp16', 'fp16f8')
NETWORK_ENTRIES = ('csd_pc_scratch_bytes', 'csd_pc_inpaint_scratch_bytes', 'csd_unet_packed_bytes', 'csd_unet_workspace_bytes',
                   'csd_unet_train_workspace_bytes@0', 'csd_unet_train_workspace_bytes@0.1')
BATCHES = (1, 2, 3, 64)
CHANNELS = (4, 32, 64, 96, 128, 192, 256, 384)
ODD_CHANNELS = (6,)                                # no multiple of 4: the GroupNorm entries return 0
SIDES = (5, 8, 10, 16, 20, 32)
VOLUMES = ((4, 4, 4), (8, 8, 8), (8, 8, 2))
ODE_N = (1, 255, 6146, 10 ** 6)
GN_MAX_GROUPS = 64                                 # CSD_GN_SCRATCH_MAX_GROUPS (include/csd.h)


def _handle_sizes(l, h, batches):
    out = []
    for B in batches:
        out += [l.csd_pc_scratch_bytes(h, B), l.csd_pc_inpaint_scratch_bytes(h, B), l.csd_unet_packed_bytes(h),
                l.csd_unet_workspace_bytes(h, B), l.csd_unet_train_workspace_bytes(h, B, 0.0),
                l.csd_unet_train_workspace_bytes(h, B, 0.1)]
    return out


def _network_sizes():
    """{'config/precision': [the NETWORK_ENTRIES at each batch size, batch-major]}; None where the model refuses the precision"""
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ncsnpp      # noqa: F401  (registers the model names)
    l = _lib.lib()
    out = {}

    def record(key, cfg, batches, meta=True):
        try:
            if meta:
                with torch.device('meta'):                      # (the handle only: no parameter values)
                    model = mutils.create_model(cfg)
            else:
                model = mutils.create_model(cfg)
        except (RuntimeError, NotImplementedError, ValueError):
            out[key] = None
            return
        h = model._h
        if getattr(cfg.model, 'csd_digest_no_resamp_conv', False):      # (as _plan_digests of tests/test_host_logic.py)
            c = model._cfg
            c.resamp_with_conv = 0
            h = ctypes.c_void_p()
            assert l.csd_unet_create(ctypes.byref(c), ctypes.byref(h)) == 0
        out[key] = _handle_sizes(l, h, batches)
        if h is not model._h:
            l.csd_unet_destroy(h)

    for prec in PRECISIONS:
        for name, cfg in _digest_configs().items():
            cfg.model.csd_precision = prec
            record('%s/%s' % (name, prec), cfg, _DIGEST_BATCHES)
        for mod, tag in ((wide_cases, 'wide'), (sr_cases, 'sr'), (kxsr_cases, 'kxsr')):
            for case in sorted(mod.CASES):
                record('%s_%s/%s' % (tag, case, prec), mod.make_config(case, prec), (1, 2, 3))
        for case in sorted(ddpm3d_cases.CASES):
            cfg = ddpm3d_cases.make_config(case, precision=prec)[0]
            cfg.model.csd_planned = True
            record('ddpm3d_%s/%s' % (case, prec), cfg, (1, 2, 3), meta=False)
    return out


def _operator_grid():
    """entry -> list of argument tuples, in a fixed order"""
    ch2 = list(itertools.product(CHANNELS, CHANNELS))
    bcs = list(itertools.product(BATCHES, CHANNELS + ODD_CHANNELS, SIDES))
    g = {}
    g['csd_groupnorm_scratch_bytes'] = [(B, C, S, S) for B, C, S in bcs]
    g['csd_groupnorm_nhwc_scratch_bytes'] = [(B, C, S * S) for B, C, S in bcs]
    g['csd_attention_scratch_bytes'] = [(B, C, S, S) for B, C, S in bcs]
    g['csd_attention_backward_scratch_bytes'] = [(B, C, S, S) for B, C, S in bcs] + [(B, C, S * S, 1) for B, C, S in bcs]
    g['csd_sum_pixels_scratch_bytes'] = [(B, S * S, C) for B, C, S in bcs if C % 4 == 0]
    g['csd_conv_scratch_bytes'] = [(B, ci, co, S, S, k, up) for B, (ci, co), S, k, up in
                                   itertools.product(BATCHES, ch2 + [(6, 3), (3, 6), (32, 3)], SIDES, (1, 3), (0, 1))]
    g['csd_conv_wgrad_scratch_bytes'] = [(B, ci, co, S, S, k, st, up) for B, (ci, co), S, k, st, up in
                                         itertools.product(BATCHES, ch2 + [(6, 3), (3, 6), (32, 3)], SIDES, (1, 3), (1, 2), (0, 1))]
    g['csd_conv3x3_block_scratch_bytes'] = ch2
    g['csd_fir_pyr_conv_scratch_bytes'] = ch2 + [(0, 4), (4, 0), (3, 128)]
    g['csd_conv3d_block_scratch_bytes'] = ch2 + [(0, 4), (4, 0), (2, 32), (1, 1)]
    g['csd_conv3d_wgrad_scratch_bytes'] = [(B, ci, co) + v + (p,) for B, (ci, co), v, p in
                                           itertools.product(BATCHES + (0,), ch2 + [(2, 32), (1, 1)], VOLUMES, (0, 1, 2))]
    g['csd_conv3d_dgrad_scale_scratch_bytes'] = [(B,) for B in BATCHES + (0,)]
    g['csd_groupnorm_scale_shift_scratch_bytes'] = [(B, C, S, G) for B, C, S, G in itertools.product(
        BATCHES + (0,), CHANNELS + ODD_CHANNELS, tuple(s * s for s in SIDES) + tuple(d * h * w for d, h, w in VOLUMES), (1, 4, 32, 96))]
    g['csd_pf_ode_scratch_bytes'] = [(B, n) for B in BATCHES + (0,) for n in ODE_N + (0,)]
    g['csd_ode_scratch_bytes'] = [(n,) for n in ODE_N + (0,)]
    g['csd_update_scratch_bytes'] = [(B,) for B in BATCHES]
    g['csd_global_norm_scratch_bytes'] = [()]
    return g


def _operator_sizes():
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    return {entry: [getattr(l, entry)(*a) for a in args] for entry, args in _operator_grid().items()}


def scratch_sizes():
    return {'network_entries': list(NETWORK_ENTRIES), 'networks': _network_sizes(), 'operators': _operator_sizes()}


def test_the_grid_names_every_sizing_entry():
    from conditional_score_diffusion_amd import _lib
    named = set(_operator_grid()) | {e.split('@')[0] for e in NETWORK_ENTRIES}
    assert named == {n for n in _lib.SIGNATURES if n.endswith('_bytes')}


def test_scratch_sizes_equal_the_pinned_ones(golden_dir):
    want = json.load(open(os.path.join(golden_dir, 'scratch_sizes.json')))
    got = scratch_sizes()
    assert got['network_entries'] == want['network_entries']
    grid = _operator_grid()
    assert sorted(got['operators']) == sorted(want['operators'])
    for entry, values in want['operators'].items():
        assert len(values) == len(grid[entry]), entry
        diff = [(a, w, g) for a, w, g in zip(grid[entry], values, got['operators'][entry]) if w != g]
        assert not diff, '%s: %d of %d sizes differ, first (args, pinned, now): %s' % (entry, len(diff), len(values), diff[:4])
        assert any(values), entry
    assert sorted(got['networks']) == sorted(want['networks'])
    for key, values in want['networks'].items():
        assert got['networks'][key] == values, key
    assert sum(v is not None for v in want['networks'].values()) > len(_digest_configs()) * 4      # (the file is not a list of refusals)


def _gn_call(l, entry, C, groups):
    """the operator on null tensors but a non-null scratch: argument checks run first, so CSD_ERR_INVALID names the refusal"""
    one = ctypes.c_void_p(256)
    if entry == 'csd_groupnorm_act':
        rc = l.csd_groupnorm_act(None, one, one, one, 1, C, 8, 8, groups, 1e-6, 1, one, None)
    else:
        rc = l.csd_groupnorm_act_nhwc(None, one, one, one, one, one, 1, C, 64, groups, 1e-6, 1, one, None)
    return rc, l.csd_last_error().decode()


def test_groupnorm_refuses_more_groups_than_its_scratch_covers():
    """csd_groupnorm_scratch_bytes / csd_groupnorm_nhwc_scratch_bytes do not know `groups`: they cover GN_MAX_GROUPS of them, and the
    operators refuse a larger count before any launch.  x is null in these calls, so a call that passes the group check ends at the
    null-argument check - with another message."""
    from conditional_score_diffusion_amd import _lib
    l = _lib.lib()
    ERR_INVALID = -1
    for entry in ('csd_groupnorm_act', 'csd_groupnorm_act_nhwc'):
        rc, msg = _gn_call(l, entry, 4 * GN_MAX_GROUPS * 2, GN_MAX_GROUPS * 2)
        assert rc == ERR_INVALID and 'groups' in msg and str(GN_MAX_GROUPS) in msg, (entry, rc, msg)
        rc, msg = _gn_call(l, entry, 4 * GN_MAX_GROUPS, GN_MAX_GROUPS)
        assert rc != 0 and 'null argument' in msg, (entry, rc, msg)
