"""models/topology.py on the host: the Python module list against the library's parameter table and the models' state_dict for every
seeded case, and the interpreter's skip stack / pyramid handling against a direct count on a recording executor."""
import copy

import pytest

import cases
import ddpm3d_cases
from conditional_score_diffusion_amd.models import utils as mutils
from conditional_score_diffusion_amd.models.topology import run_unet


def _configs():
    out = {c: cases.case_config(c)[0] for c in cases.CASES}
    out['attn_at_top'] = cases.make_config(attn_resolutions=(20, 10))       # resamp_with_conv=True, attention at level 0
    out['no_attn_at_top'] = cases.make_config(attn_resolutions=(5,))
    out.update({c: cases.ncsnpp_case(c)[0] for c in cases.NCSNPP_CASES})
    out.update({'ddpm3d_' + c: ddpm3d_cases.make_config(c)[0] for c in ddpm3d_cases.CASES})
    return out


CONFIGS = _configs()


def _family(cfg):
    name = cfg.model.name
    return 'ddpm3d' if name.startswith('ddpm3D') else 'ncsnpp' if name.startswith('ncsnpp') else 'ddpm'


def _models(cfg):
    """(the model whose module list is under test, the model that owns the library handle)"""
    fam = _family(cfg)
    if fam == 'ddpm3d':
        model = mutils.get_model(cfg.model.name)(cfg, planned=True)
        return model, model
    planned = mutils.create_model(cfg)
    if fam == 'ddpm':
        return planned, planned
    ops_cfg = copy.deepcopy(cfg)
    ops_cfg.model.name = cfg.model.name + '_ops'
    return mutils.create_model(ops_cfg), planned


def _topology(model):
    return model._topology() if callable(model._topology) else model._topology


def _derived_table(mods, fam, cfg):
    """state_dict names and shapes from the module list alone (the rules of csrc/unet.hip's and unet3d.h's parameter tables)"""
    m = cfg.model
    k = (3, 3, 3) if fam == 'ddpm3d' else (3, 3)
    temb = 4 * m.nf
    rows = []
    for i, mod in enumerate(mods):
        def add(name, *shape):
            rows.append(('all_modules.%d.%s' % (i, name), tuple(shape)))

        def pair(sub, w_shape, nb, w='weight', b='bias'):
            add(sub + w, *w_shape)
            add(sub + b, nb)

        ci, co = mod.cin, mod.cout
        if mod.kind == 'fourier':
            add('W', ci)
        elif mod.kind == 'linear':
            pair('', (co, ci), co)
        elif mod.kind == 'conv':
            pair('', (co, ci) + k, co)
        elif mod.kind == 'gn':
            pair('', (ci,), ci)
        elif mod.kind in ('down', 'up'):
            if fam == 'ddpm' and m.resamp_with_conv:
                pair('Conv_0.', (ci, ci, 3, 3), ci)
        elif mod.kind == 'combine':
            pair('Conv_0.', (co, ci, 1, 1), co)
        elif mod.kind == 'pyr_down':
            pair('Conv2d_0.' if m.fir else 'Conv_0.', (co, ci, 3, 3), co)
        elif mod.kind == 'attn':
            pair('GroupNorm_0.', (ci,), ci)
            for j in range(4):
                pair('NIN_%d.' % j, (ci, ci), ci, 'W', 'b')
        else:
            assert mod.kind == 'res'
            pair('GroupNorm_0.', (ci,), ci)
            pair('Conv_0.', (co, ci) + k, co)
            if m.conditional:
                pair('Dense_0.', (co, temb), co)
            pair('GroupNorm_1.', (co,), co)
            pair('Conv_1.', (co, co) + k, co)
            if fam == 'ddpm' and ci != co:
                pair('NIN_0.', (ci, co), co, 'W', 'b')
            elif fam == 'ncsnpp' and (ci != co or mod.up or mod.down):
                pair('Conv_2.', (co, ci, 1, 1), co)
            elif fam == 'ddpm3d' and ci != co:
                pair('Conv_2.', (co, ci) + k, co)
    return rows


@pytest.mark.parametrize('name', list(CONFIGS))
def test_module_list_gives_the_library_table_and_the_state_dict(name):
    cfg = CONFIGS[name]
    fam = _family(cfg)
    model, owner = _models(cfg)
    derived = _derived_table(_topology(model), fam, cfg)
    assert derived == owner._param_table()
    assert derived == [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert len(_topology(model)) == len(model.all_modules)
    # the operator class and the planned class of one NCSN++ config hold the same parameters (the training twin shares them)
    assert derived == [(k, tuple(v.shape)) for k, v in owner.state_dict().items()]


class _Recorder:
    """executor that computes nothing: an activation is its channel count; records (what, role, module index, skip channels)"""

    def __init__(self, mods):
        self.index = {id(m): i for i, m in enumerate(mods)}
        self.calls = []

    def __getattr__(self, what):
        def call(node, m, *args):
            self.calls.append((what, m.role, self.index[id(m)], args))
            if what == 'up_block':
                h, skip = args[0], args[1]
                assert (h, skip) == (m.cin - m.skip, m.skip)
            if what == 'combine':
                return args[0], m.cout
            if what == 'pyr_conv':
                return m.cout
            if what in ('emb_fourier', 'emb_linear'):
                return args[0]
            return m.cout
        return call


@pytest.mark.parametrize('name', list(CONFIGS))
def test_interpreter_pushes_and_pops_by_the_list(name):
    cfg = CONFIGS[name]
    model, _ = _models(cfg)
    mods = _topology(model)
    ex = _Recorder(mods)
    out = run_unet(mods, [None] * len(mods), ex, mods[[m.role for m in mods].index('stem')].cin, 'label')
    # one call per module, in list order, each under its own role
    assert [(c[1], c[2]) for c in ex.calls] == [(m.role, i) for i, m in enumerate(mods)]
    levels, nrb = len(cfg.model.ch_mult), cfg.model.num_res_blocks
    pushes = sum(m.push for m in mods)
    ups = [m for m in mods if m.role == 'up_block']
    assert pushes == 1 + levels * nrb + (levels - 1) == len(ups) == levels * (nrb + 1)       # every skip pushed is popped exactly once
    # the skips come back in reverse order of their pushes, with the channel counts the records state (checked per call above too)
    pushed = [m.cout for m in mods if m.push]
    assert [m.skip for m in ups] == pushed[::-1]
    for m in ups:
        assert m.skip > 0 and m.cin > m.skip
    # mid_res_in reads the top of the stack and leaves it
    mid = [c for c in ex.calls if c[1] == 'mid_res_in']
    assert len(mid) == 1 and mid[0][3][0] == pushed[-1]
    roles = {m.role for m in mods}
    fam = _family(cfg)
    pin = cfg.model.progressive_input if fam == 'ncsnpp' else 'none'
    pout = cfg.model.progressive if fam == 'ncsnpp' else 'none'
    assert ('combine' in roles) == (pin == 'input_skip') and ('pyr_down' in roles) == (pin == 'residual')
    assert ({'pyr_gn', 'pyr_conv'} <= roles) == (pout == 'output_skip') == (not {'head_gn', 'head_conv'} & roles)
    assert ('emb_fourier' in roles) == (fam == 'ncsnpp' and cfg.model.embedding_type == 'fourier')
    assert ('mid_attn' in roles) == (fam != 'ddpm3d')
    assert out == mods[-1].cout
