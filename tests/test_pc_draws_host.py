"""No GPU: the noise draws of the fused PC loop, as csd_pc_noise_draws lists them (csrc/pc_loop.h: PCSchedule - the schedule the loop
itself reads its tape offsets and Philox streams from), over a grid of rules, modes, step counts, batch sizes and four tiny handles:
pinned in tests/golden/pc_draws.json (recorded by tools/make_pc_draws.py), and - the fixture is written by the code under test -
anchored to rows written out by hand from the formulas the loop used before it had a schedule.  Also here: the Python-side counts
(sampling/fused.py) against the library's, and the two messages of a tape that does not fit."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

import cases
import ddpm3d_cases
import kxsr_cases

RULES = [(p, c) for p in (0, 1, 2) for c in (0, 1, 2) if (p, c) != (2, 2)]      # (predictor, corrector) ids of csd_pc_params
MODES = {'plain': (0, 0, 0), 'std_y': (1, 0, 0), 'use_path': (0, 1, 0), 'inpaint': (0, 0, 1)}      # (has_std_y, has_path_coef, inpaint)
N_STEPS = (1, 3)
BATCHES = (1, 3)
HANDLES = ('paired_3_1', 'kxsr_K1', 'uncond_tiny', 'ddpm3d_B')
Z_Y0, Z_Y, ZY, Z, Z_BLEND = range(5)               # kinds
CORR, PRED, NONE = range(3)                        # phases

_MODELS = {}


def handle(name):
    """-> (model, per-sample elements of an x draw, of a y draw)"""
    if name not in _MODELS:
        from conditional_score_diffusion_amd.models import utils as mutils
        meta = True
        if name == 'paired_3_1':                       # y_channels != x_channels: an nx / ny mix-up shows
            cfg = cases.make_config(name='ddpm_paired', ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(), image_size=12, x_ch=3, y_ch=1)
            ex, ey = 3 * 12 * 12, 1 * 12 * 12
        elif name == 'kxsr_K1':                        # y_scale: ny at (S / K)^2
            cfg = kxsr_cases.make_config('K1')
            (_, cx, S, _), (_, cy, s, _) = kxsr_cases.shapes('K1')
            ex, ey = cx * S * S, cy * s * s
        elif name == 'uncond_tiny':
            cfg = cases.case_config('uncond_tiny')[0]
            ex, ey = int(np.prod(cfg.data.shape_x)), 0
        else:                                          # arch 2: D*H*W
            cfg = ddpm3d_cases.make_config('B')[0]
            cfg.model.csd_planned = True
            ex, ey = int(np.prod(cfg.data.shape_x)), int(np.prod(cfg.data.shape_y))
            meta = False
        if meta:
            with torch.device('meta'):                 # (the handle only: no parameter values)
                model = mutils.create_model(cfg)
        else:
            model = mutils.create_model(cfg)
        _MODELS[name] = (model, ex, ey)
    return _MODELS[name]


def grid():
    return itertools.product(HANDLES, MODES, RULES, N_STEPS, BATCHES)


def key(name, mode, rules, n, B):
    return '%s/%s/p%dc%d/n%d/B%d' % ((name, mode) + tuple(rules) + (n, B))


def draws(name, mode, rules, n, B):
    """the rows as lists, or None: refused"""
    from conditional_score_diffusion_amd.sampling import fused
    try:
        return [list(r) for r in fused.noise_draws(handle(name)[0]._h, B, rules[0], rules[1], *MODES[mode], n_steps=n)]
    except RuntimeError:
        return None


def pc_draws():
    rec = {key(*g): draws(*g) or 'refused' for g in grid()}
    return {'row': ['step', 'kind', 'phase', 'elems', 'tape_offset', 'philox_stream'], 'draws': rec}


def test_draws_equal_the_pinned_ones(golden_dir):
    want = json.load(open(os.path.join(golden_dir, 'pc_draws.json')))
    got = pc_draws()
    assert got['row'] == want['row'] and sorted(got['draws']) == sorted(want['draws'])
    for k, rows in want['draws'].items():
        assert got['draws'][k] == rows, k
    listed = [r for r in want['draws'].values() if r != 'refused']
    assert len(listed) > len(want['draws']) // 3 and len(listed) < len(want['draws'])      # (neither a list of refusals nor without one)


def _sizes(name, B):
    _, ex, ey = handle(name)
    return B * ex, B * ey


@pytest.mark.parametrize('name', [h for h in HANDLES if h != 'uncond_tiny'])
def test_anchor_rows_of_the_conditional_modes(name):
    """written out from the loop's earlier formulas: plain, per existing phase [zy] z at stream 1 + i*draws_per_step + k; use_path,
    z_y0 at stream 1, then per step z_y, z_predictor, z_corrector from stream 2 + i*(1 + phases)"""
    for n, B in itertools.product(N_STEPS, BATCHES):
        nx, ny = _sizes(name, B)
        assert nx != ny or name == 'ddpm3d_B'          # (the 3-D cases carry one channel each way)
        S = 2 * (nx + ny)
        want = []
        for i in range(n):
            want += [[i, ZY, CORR, ny, i * S, 1 + 4 * i], [i, Z, CORR, nx, i * S + ny, 2 + 4 * i],
                     [i, ZY, PRED, ny, i * S + nx + ny, 3 + 4 * i], [i, Z, PRED, nx, i * S + nx + 2 * ny, 4 + 4 * i]]
        assert draws(name, 'std_y', (0, 0), n, B) == want
        assert draws(name, 'plain', (1, 2), n, B) == [[i, Z, PRED, nx, i * nx, 1 + i] for i in range(n)]
        S = ny + 2 * nx
        want = [[-1, Z_Y0, NONE, ny, 0, 1]]
        for i in range(n):
            want += [[i, Z_Y, NONE, ny, ny + i * S, 2 + 3 * i], [i, Z, PRED, nx, 2 * ny + i * S, 3 + 3 * i],
                     [i, Z, CORR, nx, 2 * ny + nx + i * S, 4 + 3 * i]]
        assert draws(name, 'use_path', (0, 0), n, B) == want


def test_anchor_rows_of_the_unconditional_modes():
    """inpainting: [z_corrector] z_blend [z_predictor] z_blend, stream 1 + i*draws_per_step + k; a 'none' phase keeps its blend draw"""
    for n, B in itertools.product(N_STEPS, BATCHES):
        nx, ny = _sizes('uncond_tiny', B)
        assert ny == 0
        want = []
        for i in range(n):
            want += [[i, Z_BLEND, CORR, nx, 3 * i * nx, 1 + 3 * i], [i, Z, PRED, nx, (3 * i + 1) * nx, 2 + 3 * i],
                     [i, Z_BLEND, PRED, nx, (3 * i + 2) * nx, 3 + 3 * i]]
        assert draws('uncond_tiny', 'inpaint', (0, 2), n, B) == want
        assert draws('uncond_tiny', 'plain', (1, 2), n, B) == [[i, Z, PRED, nx, i * nx, 1 + i] for i in range(n)]


def test_one_rule_under_every_listed_schedule():
    """draw j is stream 1 + j and lies behind the draws before it; x draws have nx elements, y draws ny"""
    for g in grid():
        rows = draws(*g)
        if rows is None:
            continue
        nx, ny = _sizes(g[0], g[4])
        off = 0
        for j, (step, kind, phase, elems, offset, stream) in enumerate(rows):
            assert (offset, stream) == (off, 1 + j), (g, j)
            assert elems == (nx if kind in (Z, Z_BLEND) else ny), (g, j)
            off += elems
        assert [r[0] for r in rows] == sorted(r[0] for r in rows)


def test_refusals_are_those_of_the_sampling_entries():
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd.sampling import fused
    refused = {k for k in (key(*g) for g in grid()) if draws(*_unkey(k)) is None}
    for name, mode, rules, n, B in grid():
        cond = name != 'uncond_tiny'
        want = (mode == 'inpaint' and cond) or (mode in ('std_y', 'use_path') and not cond)
        assert (key(name, mode, rules, n, B) in refused) == want
    for name, rules, flags, words in [('uncond_tiny', (2, 2), (0, 0, 0), "both 'none'"), ('uncond_tiny', (0, 0), (1, 0, 0), 'std_y given'),
                                      ('uncond_tiny', (0, 0), (0, 1, 0), 'use_path needs'), ('paired_3_1', (0, 0), (1, 1, 0), 'use_path needs'),
                                      ('paired_3_1', (0, 0), (0, 0, 1), 'unconditional networks only'), ('kxsr_K1', (0, 0), (0, 0, 1), 'y_scale'),
                                      ('ddpm3d_B', (0, 0), (0, 0, 1), '3-D'), ('uncond_tiny', (0, 0), (1, 0, 1), 'std_y given'),
                                      ('uncond_tiny', (0, 0), (0, 1, 1), 'path_coef belong'), ('uncond_tiny', (3, 0), (0, 0, 0), 'bad predictor')]:
        h = handle(name)[0]._h
        assert _lib.lib().csd_pc_noise_draws(h, 2, rules[0], rules[1], *flags, 2, None, 0) == -1      # CSD_ERR_INVALID
        assert words in _lib.lib().csd_last_error().decode(), (name, rules, flags)
        with pytest.raises(RuntimeError, match=words):
            fused.noise_draws(h, 2, rules[0], rules[1], *flags, n_steps=2)


def _unkey(k):
    name, mode, r, n, B = k.split('/')
    return name, mode, (int(r[1]), int(r[3])), int(n[1:]), int(B[1:])


def test_python_side_counts_equal_the_librarys():
    """inpaint_tape_length (the step-by-step inpainter sizes its tapes with it), the row count fused.prepare checks a tape against, and
    the tape recipes of the test helpers (kxsr_cases, cases) against the count the library returns without a row buffer"""
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd.sampling import fused
    for name, mode, rules, n, B in grid():
        rows = draws(name, mode, rules, n, B)
        count = _lib.lib().csd_pc_noise_draws(handle(name)[0]._h, B, rules[0], rules[1], *MODES[mode], n, None, 0)
        assert count == (len(rows) if rows is not None else -1)
        if mode == 'inpaint' and rows is not None:
            assert fused.inpaint_tape_length(n, rules[1] != 2, rules[0] != 2) == 1 + count
    xs, ys = kxsr_cases.shapes('K1')
    for n in N_STEPS:
        for mode, shapes in (('std_y', [ys, xs, ys, xs] * n), ('use_path', [ys] + [ys, xs, xs] * n)):      # kxsr_cases.pc_tape / path_tape
            rows = draws('kxsr_K1', mode, (0, 0), n, kxsr_cases.B)
            assert [r[3] for r in rows] == [int(np.prod(s)) for s in shapes]
            assert sum(r[3] for r in rows) == kxsr_cases.tape_floats('K1', n, use_path=mode == 'use_path')
        B = cases.CASES['uncond_tiny'][1]
        rows = draws('uncond_tiny', 'plain', (0, 0), n, B)
        assert [r[3] for r in rows] == [int(np.prod(s)) for s in cases.pc_tape_shapes('uncond_tiny', n)[1:]]


def test_messages_of_a_tape_that_does_not_fit():
    from conditional_score_diffusion_amd.sampling import fused
    B, n = kxsr_cases.B, 3
    xs, ys = kxsr_cases.shapes('K1')
    nx, ny = int(np.prod(xs)), int(np.prod(ys))
    rows = fused.noise_draws(handle('kxsr_K1')[0]._h, B, 0, 0, std_y=True, n_steps=n)
    good = [torch.zeros(s) for s in [ys, xs, ys, xs] * n]
    fused.check_tape(rows, good, nx, ny)
    with pytest.raises(RuntimeError, match='noise tape holds %d draws after the prior, the loop needs %d' % (4 * n - 1, 4 * n)):
        fused.check_tape(rows, good[:-1], nx, ny)
    full = [torch.zeros(xs) for _ in range(4 * n)]      # y draws at the x size
    with pytest.raises(RuntimeError, match=r'noise tape holds %d elements after the prior, the loop needs %d \(x draws of %d, y draws of %d\)'
                       % (4 * n * nx, 2 * n * (nx + ny), nx, ny)):
        fused.check_tape(rows, full, nx, ny)
    # every network, not only y_scale ones: a paired handle with another y size
    rows = fused.noise_draws(handle('paired_3_1')[0]._h, 1, 0, 0, use_path=True, n_steps=1)
    px, py = _sizes('paired_3_1', 1)
    fused.check_tape(rows, [torch.zeros(py), torch.zeros(py), torch.zeros(px), torch.zeros(px)], px, py)
    with pytest.raises(RuntimeError, match='elements after the prior'):
        fused.check_tape(rows, [torch.zeros(px)] * 4, px, py)
