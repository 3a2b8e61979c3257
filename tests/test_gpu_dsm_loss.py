"""The fused denoising score-matching loss on the GPU: csd_dsm_perturb / csd_dsm_residual against losses._perturb and float64, their
in-register noise against the tape form, and ``fused=True`` end to end against the default route, the reference's fixtures and itself
(keyed noise, resume, accumulation).

Kernel bounds.  r = a h + b z takes three fp32 roundings, d_out = (2 w a) r two more of which 2 w is exact: five roundings of 6e-8
relative to the term magnitudes stay below 1e-6 * max 2 |w a| (|a h| + |b z|); loss_rows squares r (twice three roundings) and adds in
fp64: below 1e-6 * sum w (|a h| + |b z|)^2.  Both bounds are relative to the terms, not to the result, so cancellation cannot trip them.
End to end the bounds are the project's route-against-route bounds (tests/test_gpu_training.py:213-233)."""
import os

import numpy as np
import pytest
import torch

import cases
import guarded
from test_gpu_network import build, dev, sdes_for

pytestmark = pytest.mark.gpu

SEED = 20240607
# (B, [(offset, length)...], net_stride): 75 + 25 (offset and length no multiples of 4), 768 + 768, 768 + 192 (the 2xSR layout),
# one row of 3 x 160^2 (every partial of the per-sample reduction holds several groups)
SHAPES = [(B, segs, stride) for B in (1, 3) for segs, stride in
          [([(0, 75), (75, 25)], 100), ([(0, 768), (768, 768)], 1536), ([(0, 768), (768, 192)], 960)]] + [(2, [(0, 76800)], 76800)]
IDS = ['B%d-%s' % (B, '+'.join(str(n) for _, n in segs)) for B, segs, _ in SHAPES]


def _inputs(B, segs, stride, gap=0):
    g = torch.Generator().manual_seed(7)
    net = torch.randn(B, stride + gap, generator=g) * 3
    out = []
    for k, (off, n) in enumerate(segs):
        a = torch.rand(B, generator=g) * 4 + 0.05
        out.append({'offset': off, 'length': n, 'a': a, 'b': torch.rand(B, generator=g) * 4 + 0.05, 'w': torch.rand(B, generator=g) * 2 + 0.01,
                    'stream_id': (1 << 63) + 10 + k})
    return net, out


def _on_device(segs, z=None):
    return [dict(s, a=s['a'].to(dev()), b=s['b'].to(dev()), w=s['w'].to(dev()), **({'z': z[k]} if z is not None else {}))
            for k, s in enumerate(segs)]


def _tape(B, segs):
    from conditional_score_diffusion_amd import ops
    return [ops.randn((B, s['length']), SEED, s['stream_id'], dev()) for s in segs]


@pytest.mark.parametrize('B,per', [(1, 75), (3, 75), (3, 25), (3, 768), (2, 76800)])
def test_perturb_is_bitwise_the_default_route(B, per):
    from conditional_score_diffusion_amd import losses, ops
    g = torch.Generator().manual_seed(3)
    x, z = torch.rand(B, per, generator=g).to(dev()), torch.randn(B, per, generator=g).to(dev())
    m, std = torch.rand(B, generator=g) * 0.9 + 0.05, torch.rand(B, generator=g) * 30 + 0.01
    assert torch.equal(ops.dsm_perturb(x, std.to(dev()), m.to(dev()), z), losses._perturb(x, z, m, std))
    one = torch.ones(B)
    assert torch.equal(ops.dsm_perturb(x, std.to(dev()), None, z), losses._perturb(x, z, one, std))
    for mm in (m.to(dev()), None):                  # in-register noise == itself fed the fill
        fill = ops.randn((B, per), SEED, 5, dev())
        assert torch.equal(ops.dsm_perturb(x, std.to(dev()), mm, None, SEED, 5), ops.dsm_perturb(x, std.to(dev()), mm, fill))
    # a view that starts 4 bytes into an allocation: the element-wise path
    xo, zo = torch.zeros(B * per + 1, device=dev())[1:].view(B, per), torch.zeros(B * per + 1, device=dev())[1:].view(B, per)
    xo.copy_(x), zo.copy_(z)
    assert torch.equal(ops.dsm_perturb(xo, std.to(dev()), m.to(dev()), zo), losses._perturb(x, z, m, std))


@pytest.mark.parametrize('B,segs,stride', SHAPES, ids=IDS)
def test_residual_vs_float64_and_bitwise_properties(B, segs, stride):
    from conditional_score_diffusion_amd import ops
    net, host = _inputs(B, segs, stride)
    netd = net.to(dev())
    z = _tape(B, host)
    loss, rows, d_out = ops.dsm_residual(netd, _on_device(host, z))
    # float64 on the CPU, from the fp32 inputs
    want_d, want_rows, mag_rows, mag_d = torch.zeros(B, stride, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), torch.zeros(
        B, dtype=torch.float64), 0.0
    for s, zz in zip(host, z):
        a, b, w = (s[c].double()[:, None] for c in 'abw')
        h, zc = net[:, s['offset']:s['offset'] + s['length']].double(), zz.cpu().double()
        want_d[:, s['offset']:s['offset'] + s['length']] = 2 * w * a * (a * h + b * zc)
        want_rows += (w * (a * h + b * zc) ** 2).sum(1)
        mag_rows += (w * ((a * h).abs() + (b * zc).abs()) ** 2).sum(1)
        mag_d = max(mag_d, float((2 * (w * a).abs() * ((a * h).abs() + (b * zc).abs())).max()))
    e_d = float((d_out.cpu().double() - want_d).abs().max())
    e_r = (rows.cpu() - want_rows).abs()
    print('d_out err %.3e (bound %.3e), rows err %s (bound %s)' % (e_d, 1e-6 * mag_d, e_r.tolist(), (1e-6 * mag_rows).tolist()))
    assert e_d <= 1e-6 * mag_d
    assert bool((e_r <= 1e-6 * mag_rows).all())
    assert abs(float(loss) - float(want_rows.sum())) <= 1e-6 * float(mag_rows.sum()) + 6e-8 * abs(float(want_rows.sum()))
    # in-register noise is bitwise the tape form; two runs are bitwise equal; no d_out: same value
    for other in (ops.dsm_residual(netd, _on_device(host), SEED), ops.dsm_residual(netd, _on_device(host, z))):
        assert torch.equal(other[0], loss) and torch.equal(other[1], rows) and torch.equal(other[2], d_out)
    quiet = ops.dsm_residual(netd, _on_device(host), SEED, want_d_out=False)
    assert quiet[2] is None and torch.equal(quiet[0], loss) and torch.equal(quiet[1], rows)
    # sample 0 does not depend on the batch behind it
    if B > 1:
        first = [dict(s, a=s['a'][:1], b=s['b'][:1], w=s['w'][:1]) for s in host]
        l1, r1, d1 = ops.dsm_residual(netd[:1].contiguous(), _on_device(first), SEED)
        assert torch.equal(r1[0], rows[0]) and torch.equal(d1[0], d_out[0])
    # nothing depends on what d_out, the partials and loss_rows held: 0x00 and 0xFF fills between guards
    for fill in (0x00, 0xFF):
        with guarded.seam(fill) as rec:
            lg, rg, dg = ops.dsm_residual(netd, _on_device(host), SEED)
            torch.cuda.synchronize()
        rec.check_guards()
        assert rec.outputs == 4 and torch.equal(lg, loss) and torch.equal(rg, rows) and torch.equal(dg, d_out)


def test_residual_zeroes_row_positions_outside_the_segments():
    from conditional_score_diffusion_amd import ops
    B, segs = 3, [(40, 75), (5, 22)]                 # gaps [0, 5), [27, 40), [115, 130); the segments in descending order
    net, host = _inputs(B, segs, 130)
    with guarded.seam(0xFF):
        loss, rows, d_out = ops.dsm_residual(net.to(dev()), _on_device(host), SEED)
    d = d_out.cpu()
    assert bool((d[:, :5] == 0).all()) and bool((d[:, 27:40] == 0).all()) and bool((d[:, 115:] == 0).all())
    assert bool(torch.isfinite(d).all()) and bool((d[:, 40:115] != 0).any()) and bool(torch.isfinite(rows).all())


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _model(case, precision, dropout):
    cfg, B, x, y, u, tape = cases.grad_case(case)
    cfg.model.dropout = dropout
    cfg, nc, p, model = build(cfg, precision)
    return cfg, model, x.to(dev()), y.to(dev()), u, tape


def _fn(cfg, train, fused, rm=True, lw=True):
    from conditional_score_diffusion_amd import losses
    return losses.get_general_sde_loss_fn(sdes_for(cfg), train, cfg.model.name != 'ddpm', rm, True, lw, fused=fused)


def _default(fn, model, batch, u, tape):
    it = iter(tape)
    o_rand, o_like = torch.rand, torch.randn_like
    torch.rand = lambda *a, **k: u.clone()
    torch.randn_like = lambda t, **k: next(it).to(t.device)
    try:
        return fn(model, batch)
    finally:
        torch.rand, torch.randn_like = o_rand, o_like


def _grads(model):
    g = {k: v.grad.clone() for k, v in model.named_parameters()}
    model.zero_grad()
    return g


def _assert_same_grads(ga, gb, tol):
    total = float(np.sqrt(sum(float((v.double() ** 2).sum()) for v in gb.values())))
    worst = 0.0
    for k, v in gb.items():
        err = float((ga[k].double() - v.double()).abs().max())
        scale = max(float(v.abs().max()), float(v.double().norm()) / np.sqrt(v.numel()))
        assert err <= tol * scale + 1e-7 * total / np.sqrt(v.numel()), (k, err, scale)
        if scale > 1e-6 * total:
            worst = max(worst, err / scale)
    return worst


def _t_of(u):
    return u * (1 - 1e-5) + 1e-5


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('fp16x3', 2e-4)])
@pytest.mark.parametrize('case', list(cases.CASES))
def test_fused_equals_default_route(case, precision, tol):
    """dropout 0.1 on, both routes at call index 1 of their own model: same loss, same gradient of every parameter"""
    out = []
    for fused in (False, True):
        cfg, model, x, y, u, tape = _model(case, precision, 0.1)
        batch = x if cfg.model.name == 'ddpm' else (y, x)
        fn = _fn(cfg, True, fused)
        loss = fn(model, batch, noise=tape, t=_t_of(u)) if fused else _default(fn, model, batch, u, tape)
        assert model.training and loss.requires_grad and model._train_calls == 1
        loss.backward()
        out.append((float(loss.detach()), _grads(model)))
    (lb, gb), (la, ga) = out
    assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    print(case, precision, 'fused vs default: loss %.7f / %.7f, worst gradient difference %.2e' % (la, lb, _assert_same_grads(ga, gb, tol)))


@pytest.mark.parametrize('case', list(cases.CASES))
def test_fused_vs_reference(golden_dir, case):
    from test_oracle_golden import check_grads_vs_fixture
    g = np.load(os.path.join(golden_dir, 'losses.npz'))
    cfg, nc, p, model = build(case)
    sde = sdes_for(cfg)
    B = cases.case_config(case)[1]
    rs = np.random.RandomState(11)
    xs, ys = (B,) + tuple(cfg.data.shape_x), (B,) + tuple(cfg.data.shape_y)
    x = torch.from_numpy(rs.uniform(0, 1, size=xs).astype(np.float32)).to(dev())
    y = cases.case_y(case).to(dev())
    tvals = torch.tensor([0.83, 0.21][:B])
    batch, shapes = (x, [xs]) if cfg.model.name == 'ddpm' else ((y, x), [ys, xs] if isinstance(sde, dict) else [xs])
    for lw in (True, False):
        for rm in (True, False):
            if isinstance(sde, dict) and not lw:
                continue
            v = float(_fn(cfg, False, True, rm, lw)(model, batch, noise=cases.tape(shapes, 3), t=_t_of(tvals)))
            ref = float(g['%s_lw%d_rm%d' % (case, lw, rm)])
            assert not model.training and abs(v - ref) <= 2e-5 * abs(ref), (case, lw, rm, v, ref)
    cfg, model, x, y, u, tape = _model(case, 'fp32', 0.0)
    loss = _fn(cfg, True, True)(model, x if cfg.model.name == 'ddpm' else (y, x), noise=tape, t=_t_of(u))
    loss.backward()
    check_grads_vs_fixture(np.load(os.path.join(golden_dir, 'grads.npz')), case, float(loss.detach()), _grads(model), 1e-3)


@pytest.mark.parametrize('family', ['2xSR', 'KxSR'])
def test_fused_equals_default_route_on_the_sr_networks(family):
    """segments of different length: the x block in image layout + the y block (2xSR), the y block at S / K (KxSR)"""
    from conditional_score_diffusion_amd import losses
    if family == '2xSR':
        import sr_cases as c
        from test_gpu_sr import model_for, sdes_for as sr_sdes
    else:
        import kxsr_cases as c
        from test_gpu_kxsr import model_for, sdes_for as sr_sdes
    cfg, x, y, u, tape = c.grad_inputs(c.TRAIN_CASE)
    out = []
    for fused in (False, True):
        _, model = model_for(c.TRAIN_CASE, 'fp32', dropout=0.1, fresh=True)
        fn = losses.get_general_sde_loss_fn(sr_sdes(cfg), True, True, True, True, True, fused=fused)
        batch = (y.to(dev()), x.to(dev()))
        loss = fn(model, batch, noise=tape, t=_t_of(u)) if fused else _default(fn, model, batch, u, tape)
        loss.backward()
        out.append((float(loss.detach()), _grads(model)))
    (lb, gb), (la, ga) = out
    assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    print(family, 'fused vs default: worst gradient difference %.2e' % _assert_same_grads(ga, gb, 2e-5))


def test_noise_is_keyed_by_seed_and_call():
    vals = []
    for _ in range(2):
        cfg, model, x, y, u, tape = _model('cmde_tiny', 'fp32', 0.1)
        fn = _fn(cfg, True, True)
        step = []
        for _ in range(2):
            loss = fn(model, (y, x), t=_t_of(u), seed=77)
            loss.backward()
            step.append((loss.detach().clone(), _grads(model)))
        vals.append(step)
    (a1, ga1), (a2, _) = vals[0]
    (b1, gb1), (b2, _) = vals[1]
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and all(torch.equal(ga1[k], gb1[k]) for k in ga1)
    assert not torch.equal(a1, a2)
    cfg, model, x, y, u, tape = _model('cmde_tiny', 'fp32', 0.1)
    assert not torch.equal(_fn(cfg, True, True)(model, (y, x), t=_t_of(u), seed=78).detach(), a1)


def _trainer(case, accumulate=1, fused=True):
    from conditional_score_diffusion_amd import train
    cfg, model, x, y, u, tape = _model(case, 'fp32', 0.1)
    cfg.training.csd_fused_loss = fused
    cfg.training.accumulate_grad_batches = accumulate
    cfg.optim.warmup = 2
    cfg.optim.grad_clip = -1.0
    return train.Trainer(cfg, model, sdes_for(cfg)), (x if cfg.model.name == 'ddpm' else (y, x)), u, tape


def test_resumed_trainer_repeats_the_step_without_torch_rng_state():
    """the second step of a run resumed from state_dict(), with torch's generator reseeded differently, is bitwise the second step of
    the uninterrupted run: z is a function of (seed, call index) alone"""
    tr, batch, u, _ = _trainer('sr3_tiny')
    t1, t2 = _t_of(u), _t_of(torch.tensor([0.4, 0.66]))
    torch.manual_seed(1)
    tr.train_step(batch, t=t1)
    sd = tr.state_dict()
    l2 = tr.train_step(batch, t=t2).clone()
    w2 = tr.flat.data.clone()
    tr.close()
    tr_b, batch, _, _ = _trainer('sr3_tiny')
    tr_b.load_state_dict(sd)
    torch.manual_seed(987654321)
    torch.cuda.manual_seed_all(55)
    l2b = tr_b.train_step(batch, t=t2)
    assert torch.equal(l2b, l2) and torch.equal(tr_b.flat.data, w2)
    tr_b.close()


def test_accumulated_window_equals_default_route():
    """accumulate_grad_batches = 2: the flat gradient the optimizer step saw (it stays in .grad until the next window), fused against
    default on the same times and tape"""
    us = [torch.tensor([0.83, 0.21]), torch.tensor([0.35, 0.6])]
    grads, vals = [], []
    for fused in (False, True):
        tr, batch, u, tape = _trainer('cmde_tiny', 2, fused)
        tapes = [tape, cases.tape([tuple(v.shape) for v in tape], 9)]
        for j in range(2):
            assert tr.pending == j
            if fused:
                vals.append(float(tr.train_step(batch, t=_t_of(us[j]), noise=tapes[j])))
            else:
                vals.append(float(_default(lambda m, b: tr.train_step(b), None, batch, us[j], tapes[j])))
        torch.cuda.synchronize()
        assert tr.pending == 0 and tr.step == 1 and tr.model._train_calls == 2
        grads.append({k: v.grad.detach().clone() for k, v in tr.model.named_parameters()})
        tr.close()
    for lb, la in zip(vals[:2], vals[2:]):
        assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    print('accumulated window, fused vs default: worst gradient difference %.2e' % _assert_same_grads(grads[1], grads[0], 2e-5))
