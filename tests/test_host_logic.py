"""CPU-only tests (-m "not gpu"): the C-ABI library loads and exports every symbol include/csd.h
declares, the host-side planning entry points work without a GPU, the host mirror of the
reference interface (registries, sde_lib, per-step scalars) behaves like the reference, and the
product path fails loudly instead of falling back when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cases
import score_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from conditional_score_diffusion_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'csd.h')).read()
    declared = set(re.findall(r'\b(csd_[a-z0-9_]+)\s*\(', hdr))
    declared -= {'csd_status'}
    assert len(declared) >= 25
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), 'libcsd_hip.so does not export %s' % name
    # and the ctypes signature table covers the header one to one
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert b'gfx950' in _lib.lib().csd_version()


def test_param_table_matches_reference_state_dict_layout():
    from conditional_score_diffusion_amd.models import utils as mutils
    for case in cases.CASES:
        cfg, _ = cases.case_config(case)
        model = mutils.create_model(cfg)
        want = so.ddpm_param_shapes(so.NetCfg.from_config(cfg))
        got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        assert got == want
        assert list(got) == list(want)      # same order as the reference's state_dict


def test_full_size_plan_counts_match_survey():
    """SR3-160 = 43.48 M parameters, 107.0 GFLOP per image-evaluation."""
    import bench
    from conditional_score_diffusion_amd.models import utils as mutils
    model = mutils.create_model(bench.sr3_160_config())
    assert sum(p.numel() for p in model.parameters()) == 43479267
    launches, flops, nbytes = model.stats(1)
    assert abs(flops / 1e9 - 107.0) < 0.5
    assert 850e6 < nbytes - 43479267 * 4 < 1000e6      # ~923.5 MB activations (+ parameters once)
    l64, f64, b64 = model.stats(64)
    # (the launch count may differ by a few with the batch size: which GroupNorm statistics ride in a conv epilogue depends on the tiling;
    # from B = 64 on the <= 20^2 levels run as TWO batch chunks on two streams: their ~125 launches appear once per chunk - the
    # algorithmic flops and bytes are those of the unchunked plan)
    assert -16 <= l64 - launches <= 16 + 130 and abs(f64 / flops - 64) < 1e-6
    pbytes = 43479267 * 4
    assert abs((b64 - pbytes) / (nbytes - pbytes) - 64) < 1e-6
    l32, f32_, b32 = model.stats(32)                    # below 64 images: one chunk, the launch count of B = 1
    assert abs(l32 - launches) <= 16 and abs(f32_ / flops - 32) < 1e-6


def test_init_distribution_follows_reference_rules():
    from conditional_score_diffusion_amd.models import utils as mutils
    torch.manual_seed(0)
    cfg, _ = cases.case_config('sr3_tiny')
    sd = mutils.create_model(cfg).state_dict()
    w = sd['all_modules.3.Conv_0.weight']               # default_init(1.0): U(+-sqrt(3/fan_avg))
    lim = (3.0 / ((w.shape[1] * 9 + w.shape[0] * 9) / 2)) ** 0.5
    assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.9 * lim
    assert float(sd['all_modules.3.Conv_1.weight'].abs().max()) < 1e-4      # init_scale=0 -> 1e-10
    assert float(sd['all_modules.3.Conv_0.bias'].abs().max()) == 0
    assert torch.equal(sd['all_modules.3.GroupNorm_0.weight'], torch.ones_like(sd['all_modules.3.GroupNorm_0.weight']))


def test_registries_behave_like_the_reference():
    from conditional_score_diffusion_amd.models import utils as mutils
    from conditional_score_diffusion_amd.sampling import correctors, predictors
    for n in ('ddpm', 'ddpm_paired', 'ddpm_paired_SR3'):
        assert mutils.get_model(n).__name__.lower().startswith('ddpm')
    with pytest.raises(ValueError):
        mutils.register_model(type('X', (), {}), name='ddpm')
    with pytest.raises(KeyError):
        mutils.get_model('nope')
    assert predictors.get_predictor('conditional_reverse_diffusion').__name__ == 'conditionalReverseDiffusionPredictor'
    assert correctors.get_corrector('conditional_langevin').__name__ == 'conditionalLangevinCorrector'
    with pytest.raises(ValueError):
        predictors.register_predictor(type('P', (), {}), name='reverse_diffusion')
    # every name the reference registers resolves (sampling/predictors.py, correctors.py)
    for n in ('euler_maruyama', 'conditional_euler_maruyama', 'reverse_diffusion', 'conditional_reverse_diffusion',
              'ancestral_sampling', 'conditional_ancestral_sampling', 'none', 'conditional_none'):
        assert predictors.get_predictor(n) is not None
    for n in ('langevin', 'conditional_langevin', 'ald', 'none', 'conditional_none'):
        assert correctors.get_corrector(n) is not None
    from conditional_score_diffusion_amd import sde_lib
    with pytest.raises(NotImplementedError):       # same guard as the reference (predictors.py:110-111)
        predictors.get_predictor('ancestral_sampling')(sde_lib.subVPSDE(0.1, 20., 10), lambda x, t: x)


def test_sde_lib_matches_reference_tables(golden_dir):
    from conditional_score_diffusion_amd import sde_lib
    g = np.load(os.path.join(golden_dir, 'sde_tables.npz'))
    sde = sde_lib.cVESDE(5e-3, np.sqrt(np.prod([3, 160, 160])), 1000)
    assert np.array_equal(sde.discrete_sigmas.numpy(), g['discrete_sigmas'])
    for n in (50, 1000):
        ts = torch.linspace(sde.T, 1e-5, n)
        x = torch.zeros(n, 1, 1, 1)
        assert np.array_equal(sde.discretize(x, ts)[1].numpy(), g['G%d' % n])
        assert np.array_equal(sde.marginal_prob(x, ts)[1].numpy(), g['std%d' % n])
        assert np.array_equal(sde.sde(x, ts)[1].numpy(), g['g%d' % n])
        assert np.array_equal((ts * (sde.N - 1) / sde.T).long().numpy(), g['index%d' % n])
    vy = sde_lib.VESDE(5e-3, 1.0, 1000)
    ts = torch.linspace(1, 1e-5, 8)
    x0, x1 = torch.ones(8, 1, 2, 2) * 0.3, torch.ones(8, 1, 2, 2) * 0.7
    m, s = vy.compute_backward_kernel(x0, x1, ts, torch.ones(8) * 0.02)
    assert np.array_equal(m.numpy(), g['bk_mean']) and np.array_equal(s.numpy(), g['bk_std'])
    assert np.array_equal(vy.sde(x0, ts)[1].numpy(), g['vy_g'])
    vp = sde_lib.VPSDE(0.1, 20., 1000)
    for a, b in zip(vp.marginal_prob(x0, ts), (g['vp_mean'], g['vp_std'])):
        assert np.array_equal(a.numpy(), b)
    for a, b in zip(vp.discretize(x0, ts), (g['vp_f'], g['vp_G'])):
        assert np.array_equal(a.numpy(), b)
    for a, b in zip(vp.sde(x0, ts), (g['vp_drift'], g['vp_diff'])):
        assert np.array_equal(a.numpy(), b)


def test_reverse_sde_objects():
    """reverse() returns a subclass instance with the reference's rsde algebra (sde_lib.py:65-142)."""
    from conditional_score_diffusion_amd import sde_lib
    sde = sde_lib.VESDE(0.01, 50., 100)
    score = lambda x, t: -x                      # noqa: E731
    r = sde.reverse(score)
    assert isinstance(r, sde_lib.VESDE) and r.N == 100 and r.T == 1
    x, t = torch.randn(3, 1, 2, 2), torch.tensor([0.9, 0.5, 0.1])
    f, G = r.discretize(x, t)
    f0, G0 = sde.discretize(x, t)
    assert torch.allclose(f, f0 - G0[:, None, None, None] ** 2 * score(x, t)) and torch.equal(G, G0)
    rp = sde.reverse(score, probability_flow=True)
    f, G = rp.discretize(x, t)
    assert torch.allclose(f, f0 - G0[:, None, None, None] ** 2 * score(x, t) * 0.5) and float(G.abs().max()) == 0
    csde = sde_lib.cVESDE(0.01, 50., 100)
    rc = csde.reverse(lambda x, y, t: -(x - y))
    f, G = rc.discretize(x, x * 0, t)
    assert torch.allclose(f, f0 + G0[:, None, None, None] ** 2 * x)


def test_fused_step_scalars_match_golden(golden_dir):
    from conditional_score_diffusion_amd import sde_lib
    from conditional_score_diffusion_amd.sampling import fused
    g = np.load(os.path.join(golden_dir, 'sde_tables.npz'))
    sde = sde_lib.cVESDE(5e-3, np.sqrt(np.prod([3, 160, 160])), 1000)
    for n in (50, 1000):
        ts, labels, std_x, G, std_y = fused.step_scalars(sde, n, 1e-5)
        assert std_y is None
        assert np.array_equal(labels.numpy(), g['labels%d' % n])
        assert np.array_equal(std_x.numpy(), g['std%d' % n])
        assert np.array_equal(G.numpy(), g['G%d' % n])
    pair = {'x': sde, 'y': sde_lib.VESDE(5e-3, 1.0, 1000)}
    assert fused.step_scalars(pair, 10, 1e-5)[4].shape == (10,)


def test_no_cpu_fallback():
    """CPU tensors must be refused by the product path - loudly."""
    from conditional_score_diffusion_amd import ops
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, B = cases.case_config('sr3_tiny')
    model = mutils.create_model(cfg).eval()
    x = torch.zeros(B, 3, 20, 20)
    with pytest.raises(RuntimeError):
        model({'x': x, 'y': x}, torch.zeros(B))
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros(1, 8, 8, 8), torch.zeros(8, 8, 3, 3))
    with pytest.raises(RuntimeError):
        ops.groupnorm_act(torch.zeros(1, 32, 4, 4), torch.ones(32), torch.zeros(32))


def test_flat_state_is_serialised_per_parameter():
    """optimizer / EMA state leaves FlatParams as a per-parameter list (the reference's layout) and comes back from that list, from a
    raw buffer in this layout, and from the unpadded concatenation older checkpoints hold - the 16-byte padding of the flat buffer
    (a 3-element bias here) never reaches a checkpoint"""
    from conditional_score_diffusion_amd import optim
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))       # biases of 3 and 2 elements: padded to 4
    flat = optim.FlatParams(net.parameters())
    assert flat.numel > sum(p.numel() for p in flat.params)
    buf = torch.arange(flat.numel, dtype=torch.float32) + 1.0
    for p_, o in zip(flat.params, flat.offsets[:-1]):                            # padding holds zeros in a real state buffer
        buf[int(o) + p_.numel():int(o) + (p_.numel() + 3) // 4 * 4] = 0
    parts = flat.split(buf)
    assert [tuple(t.shape) for t in parts] == [tuple(p_.shape) for p_ in flat.params]
    for form in (parts, buf.clone(), torch.cat([t.reshape(-1) for t in parts])):
        back = torch.full((flat.numel,), -1.0)
        flat.merge_into(back, form)
        assert torch.equal(back, buf)
    with pytest.raises(ValueError):
        flat.merge_into(torch.zeros(flat.numel), torch.zeros(flat.numel + 1))
    with pytest.raises(ValueError):
        flat.merge_into(torch.zeros(flat.numel), parts[:-1])


def test_flat_params_are_shared_not_reflattened():
    """get_optimizer(config, model.parameters()) and ExponentialMovingAverage(model.parameters(), decay) - the reference's two
    calls (BaseSdeGenerativeModel.py:75-96) - must land on ONE flat buffer; a second, different flattening must raise
    (silently re-pointing p.data at a second buffer left the optimizer updating storage no Parameter views)."""
    from conditional_score_diffusion_amd import optim
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))
    a = optim.FlatParams.of(net.parameters())
    b = optim.FlatParams.of(net.parameters())
    assert a is b
    for p_, o in zip(a.params, a.offsets[:-1]):
        assert p_.data_ptr() == a.data.data_ptr() + 4 * int(o) and p_.grad.data_ptr() == a.grad.data_ptr() + 4 * int(o)
    with pytest.raises(RuntimeError):
        optim.FlatParams.of(list(net.parameters())[:2])         # a subset of an already flattened list
    with pytest.raises(RuntimeError):
        optim.FlatParams(net.parameters())                      # explicit re-flattening
    assert issubclass(optim.FusedAdam, torch.optim.Optimizer)   # LambdaLR (configure_optimizers) accepts it
    # flattened modules stay picklable / deep-copyable (the owner map lives outside the Parameter: ADVICE r2)
    import copy
    import pickle
    clone = pickle.loads(pickle.dumps(net))
    assert torch.equal(clone[0].weight, net[0].weight)
    copy.deepcopy(net)


def test_configure_sde_dispatches_on_the_lightning_module():
    """checkpoint.configure_sde follows create_lightning_module (lightning_modules/utils.py:23-27): 'conditional' + VP -> cVPSDE,
    'conditional_decreasing_variance' + VP -> plain VPSDE (ConditionalSdeGenerativeModel.py:18-21,144-146), 'base' -> VPSDE"""
    from conditional_score_diffusion_amd import checkpoint, sde_lib
    from conditional_score_diffusion_amd.config_dict import ConfigDict

    def cfg(lm, approach='sr3', name='ddpm_paired_SR3'):
        c = ConfigDict()
        c.training = ConfigDict(); c.model = ConfigDict(); c.data = ConfigDict()
        c.training.sde = 'vpsde'
        if lm is not None:
            c.training.lightning_module = lm
        if approach is not None:
            c.training.conditioning_approach = approach
        c.model.name, c.model.beta_min, c.model.beta_max, c.model.num_scales = name, 0.1, 20., 1000
        c.data.use_data_mean = False
        return c
    assert type(checkpoint.configure_sde(cfg('conditional'))[0]) is sde_lib.cVPSDE
    assert type(checkpoint.configure_sde(cfg('conditional_decreasing_variance'))[0]) is sde_lib.VPSDE
    assert type(checkpoint.configure_sde(cfg('base', approach=None, name='ddpm'))[0]) is sde_lib.VPSDE
    assert type(checkpoint.configure_sde(cfg(None))[0]) is sde_lib.cVPSDE             # no key: the name heuristics
    with pytest.raises(NotImplementedError):
        checkpoint.configure_sde(cfg('conditional', approach='ours_NDV'))


def test_product_code_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'conditional_score_diffusion_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                txt = open(os.path.join(dirpath, f)).read()
                assert 'score_oracle' not in txt and 'import oracle' not in txt and 'from oracle' not in txt, f


def test_config_dict_loads_reference_style_config(tmp_path):
    from conditional_score_diffusion_amd.config_dict import ConfigDict, load_reference_config
    p = tmp_path / 'cfg.py'
    p.write_text('import ml_collections\n'
                 'def get_config():\n'
                 '  config = ml_collections.ConfigDict()\n'
                 '  config.model = model = ml_collections.ConfigDict()\n'
                 '  model.nf = 96\n'
                 '  model.ch_mult = (1, 1, 2)\n'
                 '  config.seed = 42\n'
                 '  return config\n')
    c = load_reference_config(str(p))
    assert isinstance(c, ConfigDict) and c.model.nf == 96 and c.model.ch_mult == (1, 1, 2) and c.seed == 42
    with pytest.raises(AttributeError):
        c.model.missing


def test_lightning_checkpoint_reader(tmp_path):
    """A reference-style Lightning checkpoint (score_model.* keys + VS-CMDE buffers) loads into the adapter."""
    from conditional_score_diffusion_amd import checkpoint
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, _ = cases.case_config('cmde_tiny')
    src = mutils.create_model(cfg)
    sd = {'score_model.' + k: v.clone() + 0.01 for k, v in src.state_dict().items()}
    sd['sigma_max_y'] = torch.tensor(0.37)
    path = os.path.join(tmp_path, 'epoch=1.ckpt')
    torch.save({'state_dict': sd, 'hyper_parameters': {'config': None}, 'epoch': 1}, path)
    dst = mutils.create_model(cfg)
    rest = checkpoint.load_lightning_checkpoint(dst, path)
    assert float(rest['sigma_max_y']) == pytest.approx(0.37)
    for (k, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a + 0.01, b), k
    with pytest.raises(KeyError):
        checkpoint.split_lightning_state_dict({'state_dict': {'other.weight': torch.zeros(1)}})


class _Evil:
    def __reduce__(self):
        import os as _os
        return (_os.system, ('echo pwned > /tmp/csd_pwned',))


def test_checkpoint_with_config_rebuilds_the_sdes_and_refuses_code(tmp_path):
    """hyper_parameters.config + the VS-CMDE buffers -> model, sde['y'] with the checkpoint's sigma_max_y / sigma_min_y
    (ConditionalSdeGenerativeModel.py:136-175, lightning_modules/utils.py:23-27); a pickle that would execute code is refused."""
    from conditional_score_diffusion_amd import checkpoint, sde_lib
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg, _ = cases.case_config('cmde_tiny')
    cfg.training.lightning_module = 'conditional_decreasing_variance'
    cfg.data.use_data_mean = False
    src = mutils.create_model(cfg)
    sd = {'score_model.' + k: v.clone() for k, v in src.state_dict().items()}
    sd['sigma_max_y'], sd['sigma_min_y'] = torch.tensor(0.37), torch.tensor(0.004)
    path = os.path.join(tmp_path, 'vs.ckpt')
    torch.save({'state_dict': sd, 'hyper_parameters': {'config': cfg}, 'epoch': 3, 'global_step': 1234}, path)
    mod = checkpoint.load_score_module(path)
    assert isinstance(mod.sde, dict) and isinstance(mod.sde['x'], sde_lib.cVESDE) and isinstance(mod.sde['y'], sde_lib.VESDE)
    assert mod.sde['y'].sigma_max == pytest.approx(0.37) and mod.sde['y'].sigma_min == pytest.approx(0.004)
    assert mod.sde['x'].sigma_max == pytest.approx(cfg.model.sigma_max_x) and mod.sampling_eps == 1e-5
    assert mod.config.model.nf == cfg.model.nf and tuple(mod.config.model.ch_mult) == tuple(cfg.model.ch_mult)
    for (k, a), (_, b) in zip(src.state_dict().items(), mod.score_model.state_dict().items()):
        assert torch.equal(a, b), k
    # SR3 config: one conditional SDE, no y SDE
    c2, _ = cases.case_config('sr3_tiny')
    c2.data.use_data_mean = False
    s2, eps2 = checkpoint.configure_sde(c2)
    assert isinstance(s2, sde_lib.cVESDE) and eps2 == 1e-5
    evil = os.path.join(tmp_path, 'evil.ckpt')
    torch.save({'state_dict': sd, 'hyper_parameters': {'config': _Evil()}}, evil)
    if os.path.exists('/tmp/csd_pwned'):
        os.remove('/tmp/csd_pwned')
    with pytest.raises(Exception):
        checkpoint.read_checkpoint(evil)
    assert not os.path.exists('/tmp/csd_pwned')


def test_vs_cmde_variance_schedule():
    """get_reduction_fn (lightning_callbacks/callbacks.py:81-86): starts at y0, reaches yk at xk steps, inverse multiplicative in between -
    the edges2shoes values (configs/.../edges2shoes_ours_DV.py:101-104)."""
    from conditional_score_diffusion_amd.train import get_reduction_fn
    y0, xk, yk = float(np.sqrt(3 * 64 * 64)), 300000, 1.0
    f = get_reduction_fn(y0, xk, yk)
    assert abs(f(0) - y0) < 1e-9 and abs(f(xk) - yk) < 1e-9
    assert f(1000) > f(2000) > f(100000) > yk
    assert abs(f(150000) - xk * yk * y0 / (150000 * (y0 - yk) + xk * yk)) < 1e-12


def test_conv_xp_isa_check_catches_unprotected_accumulator_accesses(tmp_path):
    """tools/check_xp_isa.py (run by the build on conv_xk.hip's ISA; the synthetic cases use the conv_xp naming it also knows) accepts matrix instructions + reads behind the tied wait, and
    rejects a register move on an accumulator or a read in the shadow of a matrix instruction"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('check_xp_isa', os.path.join(root, 'tools', 'check_xp_isa.py'))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    name = '_ZN3csd14conv_xp_kernelILi2ELb0ELb0EEEvPKcNS_10ConvFFArgsE'
    mf = ['\tv_mfma_f32_32x32x16_f16 a[%d:%d], v[2:5], v[6:9], a[%d:%d]' % (16 * i, 16 * i + 15, 16 * i, 16 * i + 15) for i in range(4)]
    good = [name + ':'] + mf + ['\ts_nop 15', '\tv_accvgpr_read_b32 v1, a0', '\tv_accvgpr_mov_b32 a100, a101', '\ts_endpgm']
    moved = [name + ':'] + mf + ['\tv_accvgpr_mov_b32 a16, a64', '\ts_nop 15', '\tv_accvgpr_read_b32 v1, a0', '\ts_endpgm']
    early = [name + ':'] + mf + ['\tv_accvgpr_read_b32 v1, a0', '\ts_endpgm']
    five = [name + ':'] + mf + ['\tv_mfma_f32_32x32x16_f16 a[64:79], v[2:5], v[6:9], a[64:79]', '\ts_endpgm']
    # a compiler label between the tied wait and the read: the read is reachable from another block (one that may end in a matrix
    # instruction), so the wait above it proves nothing - the check must see the label (round-5 advisor: labels used to be dropped
    # together with the assembler directives) while directives stay invisible
    label = [name + ':'] + mf + ['\ts_nop 15', '.LBB0_2:', '\tv_accvgpr_read_b32 v1, a0', '\ts_endpgm']
    directive = [name + ':'] + mf + ['\ts_nop 15', '\t.p2align 6', '\tv_accvgpr_read_b32 v1, a0', '\ts_endpgm']
    for lines, rc in ((good, 0), (moved, 1), (early, 1), (five, 1), (label, 1), (directive, 0)):
        p = tmp_path / 'k.s'
        p.write_text('\n'.join(lines) + '\n')
        assert chk.main(str(p)) == rc
    built = os.path.join(root, 'conditional_score_diffusion_amd', 'csrc', 'conv_xk.s')
    if os.path.exists(built):                        # the ISA the in-tree library was built from (the product build generates conv_xk.s)
        assert chk.main(built) == 0


def test_bucket_first_modules_follow_the_module_list():
    """distributed.bucket_first_modules: the module whose backward completes a gradient bucket = the lowest all_modules index among
    the bucket's parameters (the planned backward walks the list back to front and records the bucket's event after that module)"""
    from conditional_score_diffusion_amd.distributed import bucket_first_modules
    names = ['all_modules.0.weight', 'all_modules.0.bias', 'all_modules.1.weight', 'all_modules.3.Conv_0.weight',
             'all_modules.3.Conv_0.bias', 'all_modules.10.NIN_0.W', 'all_modules.11.weight']
    assert bucket_first_modules(names, [[0, 1, 2], [3, 4], [5, 6]]) == [0, 3, 10]
    assert bucket_first_modules(names, [[0, 1, 2, 3], [4, 5, 6]]) == [0, 3]      # a module split over two buckets completes both
    assert bucket_first_modules(names + ['head.weight'], [[0], [7]]) is None      # not the reference's naming: no events, no overlap


# ---- plan digests: everything the host side derives from a configuration, pinned bit for bit --------------------------------------
_DIGEST_BATCHES = (1, 7, 32, 64, 65)        # 64 / 65: two batch chunks, equal and ragged


def _digest_configs():
    """name -> reference-style config.  The GPU tools are not imported: the values of tools/bench_other.py (cmde128_config,
    ncsnpp_config), tests/test_gpu_fullsize.py (build_ncsnpp_256), tools/bench_train.py (the two training shapes) and
    tools/bench_ncsnpp_cifar.py (cifar_config) are restated."""
    import itertools
    import bench
    out = {}
    for case in cases.CASES:
        out[case] = cases.case_config(case)[0]
    for case, (kw, _) in cases.NCSNPP_CASES.items():
        out[case] = cases.make_ncsnpp_config(**kw)
    out['sr3_160'] = bench.sr3_160_config()
    out['cmde_128'] = cases.make_config(name='ddpm_paired', nf=96, ch_mult=(1, 1, 2, 2, 3, 3), attn_resolutions=(16, 8, 4), image_size=128)
    big = dict(channels=6, nf=96, ch_mult=(1, 1, 2, 2, 3, 3), num_res_blocks=2, attn_resolutions=(20, 10, 5), image_size=160,
               embedding_type='positional')
    for name in ('ncsnpp', 'ncsnpp_paired'):
        out[name + '_160'] = cases.make_ncsnpp_config(name=name, **big)
    out['ncsnpp_256'] = cases.make_ncsnpp_config(name='ncsnpp', channels=3, nf=128, ch_mult=(1, 1, 2, 2, 2, 2, 2), num_res_blocks=2,
                                                 attn_resolutions=(16,), image_size=256, embedding_type='fourier')
    out['train_ddpm_paired_64'] = cases.make_config(name='ddpm_paired', nf=128, ch_mult=(1, 1, 2, 2), attn_resolutions=(16, 8), image_size=64)
    out['train_ncsnpp_paired_64'] = cases.make_ncsnpp_config(name='ncsnpp_paired', channels=6, nf=128, ch_mult=(1, 1, 2, 2), num_res_blocks=2,
                                                             attn_resolutions=(16,), image_size=64, embedding_type='positional')
    for pin, fir, emb, prog in itertools.product(('none', 'input_skip', 'residual'), (True, False), ('positional', 'fourier'),
                                                 ('none', 'output_skip')):
        out['cifar_%s_%s_%s_%s' % (pin, 'fir' if fir else 'nofir', emb, prog)] = cases.make_ncsnpp_config(
            nf=128, ch_mult=(1, 2, 2, 2), num_res_blocks=4, attn_resolutions=(16,), image_size=32, channels=3, embedding_type=emb,
            progressive=prog, progressive_input=pin, fir=fir)
    out['ddpm_no_resamp_conv'] = cases.make_config(nf=32, ch_mult=(1, 2, 2, 2), attn_resolutions=(20,), image_size=80)
    out['ddpm_no_resamp_conv'].model.csd_digest_no_resamp_conv = True       # (see _plan_digests)
    out['ddpm_unconditional'] = cases.make_config(name='ddpm', nf=32, ch_mult=(1, 2, 2, 2), attn_resolutions=(10,), image_size=80)
    out['ddpm_unconditional'].model.conditional = False
    # networks that are not SiLU: no fused-prologue conv and no tap-partial head anywhere (build_packed_layout)
    out['sr3_tiny_elu'] = cases.case_config('sr3_tiny')[0]
    out['sr3_tiny_elu'].model.nonlinearity = 'elu'
    out['ncsnpp_fourier_skip_relu'] = cases.make_ncsnpp_config(**cases.NCSNPP_CASES['ncsnpp_fourier_skip'][0])
    out['ncsnpp_fourier_skip_relu'].model.nonlinearity = 'relu'
    return out


def test_unknown_activation_raises_at_construction():
    """config.model.nonlinearity outside swish / relu / lrelu / elu (models/layers.py:29-41) fails when the model is built, in both
    families - never later, never with another activation in its place"""
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ncsnpp      # noqa: F401  (registers the model names)
    for cfg in (cases.case_config('sr3_tiny')[0], cases.make_ncsnpp_config()):
        for bad in ('gelu', 'none'):
            cfg.model.nonlinearity = bad
            with pytest.raises(NotImplementedError):
                mutils.create_model(cfg)


def _plan_digests():
    """{'config/precision': {'B': [params, layout, plan, training dry run]}} from csd_unet_debug_digest (csrc/plan_digest.h)"""
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd.models import utils as mutils
    import conditional_score_diffusion_amd.models.ncsnpp      # noqa: F401  (registers the model names)
    fn = ctypes.CDLL(_lib.LIB_PATH).csd_unet_debug_digest
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_uint64)]
    out = {}
    for name, cfg in _digest_configs().items():
        for prec in ('fp32', 'fp16x3', 'fp16', 'fp16f8'):
            cfg.model.csd_precision = prec
            with torch.device('meta'):                      # (the digests need the handle only: no parameter values)
                model = mutils.create_model(cfg)
            h = model._h
            if getattr(cfg.model, 'csd_digest_no_resamp_conv', False):
                # resamp_with_conv = False: the Python adapter cannot hold a module list with parameter-less entries; the library plans it
                c = model._cfg
                c.resamp_with_conv = 0
                h = ctypes.c_void_p()
                assert _lib.lib().csd_unet_create(ctypes.byref(c), ctypes.byref(h)) == 0
            per_b = out['%s/%s' % (name, prec)] = {}
            for B in _DIGEST_BATCHES:
                d = (ctypes.c_uint64 * 4)()
                assert fn(h, B, float(cfg.model.dropout), d) == 0, (name, prec, B, _lib.lib().csd_last_error())
                per_b[str(B)] = ['%016x' % v for v in d]
            if h is not model._h:
                _lib.lib().csd_unet_destroy(h)
    return out


def test_plan_digests_equal_the_pinned_ones(golden_dir):
    """The parameter table, the packed-weight layout, the inference plan (every launch with its offsets, geometry and tiles) and the
    training graph's dry run (recorded steps, saved-tensor offsets, workspace size) of every configuration the project tests or
    benchmarks, in the four precision modes and at five batch sizes, hash to the values in tests/golden/plan_digests.json.  That file
    was recorded with this same code on the commit it names.  A pull request that MEANS to change a plan, a layout or the training
    graph regenerates the file (json.dump of _plan_digests() plus its own parent's hash) and says so; one that does not must leave
    every digest equal."""
    import json
    want = json.load(open(os.path.join(golden_dir, 'plan_digests.json')))['digests']
    got = _plan_digests()
    assert sorted(got) == sorted(want)
    diff = ['%s B=%s' % (k, b) for k in want for b in want[k] if got[k].get(b) != want[k][b]]
    assert not diff, '%d of %d digests differ, first: %s' % (len(diff), sum(len(v) for v in want.values()), diff[:8])


# the four configurations of test_chunked_plans_of_ragged_batches_build and, per precision, the inference-plan digest of each at
# B = 64 as the commit BEFORE the per-chunk-size block sizing computed it (equal chunks: that sizing leaves them alone)
_RAGGED_CHUNK_CONFIGS = [
    dict(name='ddpm', nf=32, ch_mult=(1, 1, 2, 2), num_res_blocks=2, attn_resolutions=(), image_size=40),
    dict(name='ddpm', nf=96, ch_mult=(1, 1, 2, 2), num_res_blocks=2, attn_resolutions=(), image_size=40),
    dict(name='ddpm_paired_SR3', nf=32, ch_mult=(1, 1, 2, 2), num_res_blocks=3, attn_resolutions=(16, 8), image_size=40),
    dict(name='ddpm_paired_SR3', nf=96, ch_mult=(1, 1, 2, 2), num_res_blocks=3, attn_resolutions=(16, 8), image_size=40),
]
_RAGGED_CHUNK_B64_PLAN_DIGESTS = {
    'fp32': ['d2355ef4eda15497', 'aea9fc5ec0b3f273', '3595f31bcb0a6d9e', 'a6bb53b074b0b7bb'],
    'fp16x3': ['814d3b732d78f5a8', '8e1d015fff298408', 'e5010a65bed97f0d', 'c0ae75b2259dccf0'],
}


def test_chunked_plans_of_ragged_batches_build():
    """From 64 samples on the small levels of a DDPM-family plan run as two batch chunks, each in a private block of the workspace
    (csrc/unet_plan.h: build_plan).  The block is the maximum over the region's chunk sizes of what a dry run of that size needs: a
    chunk's peak is not monotone in its batch (which convs leave never-released tile statistics depends on their tiling), so a block
    sized by the full chunk of 33 alone was too small for the ragged last chunk of 32 in the four configurations below at B = 65 in
    fp16x3, and the plan failed with 'unet: a chunk outgrew its block'.  They build, at B = 65 and B = 64 in fp32 and fp16x3, and so
    does a sweep over widths, depths, image sizes and ragged batches; at B = 64 their plans hash to the values from before the fix."""
    import itertools
    from conditional_score_diffusion_amd import _lib
    from conditional_score_diffusion_amd.models import utils as mutils
    fn = ctypes.CDLL(_lib.LIB_PATH).csd_unet_debug_digest
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_uint64)]

    def meta_model(prec, **kw):
        cfg = cases.make_config(**kw)
        cfg.model.csd_precision = prec
        with torch.device('meta'):                      # (the digests need the handle only: no parameter values)
            model = mutils.create_model(cfg)
        model.digest_dropout = float(cfg.model.dropout)
        return model

    def plan_digest(model, B):
        d = (ctypes.c_uint64 * 4)()
        rc = fn(model._h, B, model.digest_dropout, d)
        return rc, '%016x' % d[2], _lib.lib().csd_last_error()

    failed = []
    for prec in ('fp32', 'fp16x3'):
        for i, kw in enumerate(_RAGGED_CHUNK_CONFIGS):
            model = meta_model(prec, **kw)
            for B in (65, 64):
                rc, dig, err = plan_digest(model, B)
                if rc != 0:
                    failed.append((kw, prec, B, err))
                elif B == 64:
                    assert dig == _RAGGED_CHUNK_B64_PLAN_DIGESTS[prec][i], (kw, prec, dig)
    for nf, ch_mult, image_size in itertools.product((32, 96), ((1, 2, 2), (1, 1, 2, 2)), (20, 40, 80)):
        kw = dict(name='ddpm_paired_SR3', nf=nf, ch_mult=ch_mult, num_res_blocks=2, attn_resolutions=(), image_size=image_size)
        if image_size % (1 << (len(ch_mult) - 1)):      # (20^2 on four levels: there is no such network to plan)
            with pytest.raises(RuntimeError, match='not divisible'):
                meta_model('fp16x3', **kw)
            continue
        model = meta_model('fp16x3', **kw)
        for B in (65, 67, 100, 127):
            rc, _, err = plan_digest(model, B)
            if rc != 0:
                failed.append((dict(nf=nf, ch_mult=ch_mult, image_size=image_size), 'fp16x3', B, err))
    assert not failed, failed


def test_every_sizing_entry_has_a_guarded_buffer_test():
    """tests/guarded.py:SIZING names, for every csd_*_bytes entry of the ABI, the tests of tests/test_gpu_buffers.py that run in a
    buffer of exactly the size the entry declared (those tests assert from the seam's record that it really did): a new sizing entry
    without a row fails here, and so does a row that names no test"""
    import ast
    import guarded
    from conditional_score_diffusion_amd import _lib
    sizing = sorted(n for n in _lib.SIGNATURES if n.endswith('_bytes'))
    assert len(sizing) >= 22
    assert sorted(guarded.SIZING) == sizing, set(guarded.SIZING) ^ set(sizing)
    tree = ast.parse(open(os.path.join(ROOT, 'tests', 'test_gpu_buffers.py')).read())
    tests = {f.name: f for f in tree.body if isinstance(f, ast.FunctionDef) and f.name.startswith('test_')}
    for entry, ids in guarded.SIZING.items():
        assert ids, entry
        for tid in ids:
            fn = tests.get(tid.split('[')[0])
            assert fn is not None, '%s: tests/test_gpu_buffers.py has no %s' % (entry, tid)
            assert 'fills' in [a.arg for a in fn.args.args], '%s does not run through the guarded seam' % tid
            assert entry in guarded.entries_of(tid.split('[')[0], tid)


def test_allocation_seam_defaults_and_guarded_helper():
    """ops._scratch / ops._out allocate what the code always allocated (a declared size of 0 still gets an address); the test seam
    swaps both and the sizing entries in and out, and a guarded buffer notices one changed byte on either side"""
    import guarded
    from conditional_score_diffusion_amd import _lib, ops
    cpu = torch.device('cpu')
    assert ops._scratch(1000, cpu).shape == (1000,) and ops._scratch(1000, cpu).dtype == torch.uint8
    assert ops._scratch(3, cpu).numel() == 3 and ops._scratch(0, cpu).numel() == 256
    t = ops._out((2, 3), torch.float64, cpu)
    assert t.shape == (2, 3) and t.dtype == torch.float64 and t.is_contiguous() and ops._out(5, torch.float32, cpu).shape == (5,)
    saved = (ops._scratch, ops._out, _lib.lib().csd_update_scratch_bytes)
    with guarded.seam(0xFF) as rec:
        n = _lib.lib().csd_update_scratch_bytes(3)
        assert n == saved[2](3) and rec.sizing_calls == [('csd_update_scratch_bytes', n)]
        sc = ops._scratch(n, cpu)
        odd = ops._scratch(n + 1, cpu)
        out = ops._out((3, 5), torch.float32, cpu)
        assert sc.numel() == n and odd.numel() == n + 1 and bool((sc == 0xFF).all())
        assert out.shape == (3, 5) and bool(torch.isnan(out).all()) and bool(torch.isnan(out.view(torch.float16)).all())
        assert rec.sized_by == {'csd_update_scratch_bytes': 1, None: 1} and rec.outputs == 1
        rec.check_guards()
        with pytest.raises(AssertionError):
            rec.assert_sized_by([])                          # (the n + 1 bytes that no entry declared)
        out.view(-1)[-1] = 1.0                               # inside the body: fine
        rec.check_guards()
        sc[:1].as_strided((1,), (1,), sc.storage_offset() + n)[0] = 0      # the first byte behind the scratch
        with pytest.raises(AssertionError, match='1 behind'):
            rec.check_guards()
    assert (ops._scratch, ops._out, _lib.lib().csd_update_scratch_bytes) == saved
    body, chk = guarded.guarded(0, cpu, 0x00)
    assert body.numel() == 0
    chk()
