"""Shared by tests/test_gpu_ddpm3d_train.py (the HIP path) and tests/test_ddpm3d_train_host.py (what the bounds mean, on the CPU): the
operator sweep of the 3x3x3 gradient kernels, the float64 references, the bounds, and the float64 restatements of the network
gradients and of the training losses over ddpm3d_cases.forward64.

Every reference is float64 torch on the CPU and is computed once per process (lru_cache); callers must not modify what they get.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ddpm3d_cases as dc

# B, (D, H, W), Cin, Cout
SWEEP = [
    (1, (1, 1, 1), 32, 32),        # the 26 off-centre taps of dw must be exactly 0
    (3, (2, 2, 2), 64, 2),         # the head (thin: fp32 kernel in both precisions)
    (3, (5, 7, 3), 2, 64),         # the stem
    (1, (12, 12, 2), 128, 32),     # the W = 2 brick (8 x 8 x 2)
    (3, (3, 5, 2), 96, 64),        # ragged, three ci tiles, several samples = several K splits
    (1, (9, 17, 16), 64, 64),      # many bricks (36) and several K splits
    (2, (5, 7, 3), 40, 72),        # channels that are no multiple of 16 or 32
]
DY_SCALES = [1.0, 2.0 ** -20]

# bounds (max|got - ref| / max|ref|), all from the project: test_gpu_train_ops.py (dw, db) and test_gpu_ddpm3d.py (conv bound at the data
# gradient's reduction length 27 * Cout)
DW_BOUND = {'fp32': 1e-5, 'fp16x3': 5e-5}
DB_BOUND = 1e-5


def dx_bound(cout):
    return 3e-6 * max(1.0, np.sqrt(27 * cout) / 8)


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


@functools.lru_cache(maxsize=None)
def op_case(idx):
    """fp32 operands of sweep case idx at dy scale 1: a [B,D,H,W,Cin], w [Cout,Cin,3,3,3], dy [B,D,H,W,Cout] (channels-last)"""
    B, vol, Cin, Cout = SWEEP[idx]
    rs = np.random.RandomState(700 + idx)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))    # noqa: E731
    return dict(a=t(B, *vol, Cin), w=t(Cout, Cin, 3, 3, 3) * float(np.sqrt(2.0 / (27 * (Cin + Cout)))), dy=t(B, *vol, Cout))


def conv_grads(a, w, dy, dtype=torch.float64):
    """(dx, dw, db) of y = conv3d(a, w, b, padding 1) by torch autograd in ``dtype``; channels-last in and out"""
    a_ = a.to(dtype).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    w_ = w.to(dtype).clone().requires_grad_(True)
    b_ = torch.zeros(w.shape[0], dtype=dtype, requires_grad=True)
    y = F.conv3d(a_, w_, b_, padding=1)
    dx, dw, db = torch.autograd.grad(y, (a_, w_, b_), dy.to(dtype).permute(0, 4, 1, 2, 3).contiguous())
    return dx.permute(0, 2, 3, 4, 1).contiguous(), dw, db


@functools.lru_cache(maxsize=None)
def op_ref(idx):
    """float64 (dx, dw, db) at dy scale 1 (the gradients are linear in dy: the reference at scale s is s times this, exactly for a power
    of two)"""
    d = op_case(idx)
    return conv_grads(d['a'], d['w'], d['dy'])


# ---- split-bf16 emulation (truncated hi, rounded lo, three product terms, float64 accumulation) ------------------------------------------
def bf16_split(x):
    """fp32 tensor -> (hi, lo) as float64: hi = x with the low 16 mantissa bits cleared, lo = bf16_rne(x - hi)"""
    xi = x.contiguous().view(torch.int32)
    hi = (xi & -65536).view(torch.float32)
    r = (x - hi).contiguous().view(torch.int32)
    r = (r + 0x7fff + ((r >> 16) & 1)) & -65536
    return hi.double(), r.view(torch.float32).double()


def dw_split_bf16(a, dy):
    """dw of the three-term split-bf16 product, accumulated in float64"""
    ah, al = bf16_split(a)
    dh, dl = bf16_split(dy)
    z = torch.zeros(1, 1, 3, 3, 3)

    def dw(x, g):
        return conv_grads(x, z.expand(g.shape[-1], x.shape[-1], 3, 3, 3), g)[1]
    return dw(ah, dh) + dw(al, dh) + dw(ah, dl)


# ---- networks ----------------------------------------------------------------------------------------------------------------------------
def net_g(case):
    """the fixed random cotangent of the model-level loss sum(out * g)"""
    name, nf, ch_mult, nrb, B, vol, xc, yc = dc.CASES[case]
    oc = xc + yc if name == 'ddpm3D_paired' else xc
    rs = np.random.RandomState(4321)
    return torch.from_numpy(rs.standard_normal((B, oc) + vol).astype(np.float32))


def forward_as(p, case, x, y, labels, dtype):
    """ddpm3d_cases.forward64 restated for any dtype (swish, centered = False), so that torch's own float32 can be held to the bounds;
    test_ddpm3d_train_host.py pins it to forward64 at float64"""
    name, nf, ch_mult, nrb, B, vol, xc, yc = dc.CASES[case]
    p = {k: v.to(dtype) for k, v in p.items()}
    P = lambda i, s: p['all_modules.%d.%s' % (i, s)]                                         # noqa: E731
    conv = lambda i, s, v: F.conv3d(v, P(i, s + 'weight'), P(i, s + 'bias'), padding=1)     # noqa: E731
    gn = lambda i, s, v: F.group_norm(v, 32, P(i, s + 'weight'), P(i, s + 'bias'), eps=1e-6)  # noqa: E731

    def res(i, v, temb):
        t = conv(i, 'Conv_0.', F.silu(gn(i, 'GroupNorm_0.', v)))
        t = t + F.linear(F.silu(temb), P(i, 'Dense_0.weight'), P(i, 'Dense_0.bias'))[:, :, None, None, None]
        t = conv(i, 'Conv_1.', F.silu(gn(i, 'GroupNorm_1.', t)))
        return (conv(i, 'Conv_2.', v) if ('all_modules.%d.Conv_2.weight' % i) in p else v) + t

    half = nf // 2
    freq = torch.exp(torch.arange(half, dtype=dtype) * -(np.log(10000.0) / (half - 1)))
    e = labels.to(dtype)[:, None] * freq[None, :]
    temb = F.linear(torch.cat([torch.sin(e), torch.cos(e)], dim=1), P(0, 'weight'), P(0, 'bias'))
    temb = F.linear(F.silu(temb), P(1, 'weight'), P(1, 'bias'))
    h = 2 * (torch.cat([x, y], dim=1) if y is not None else x).to(dtype) - 1.
    i, L = 3, len(ch_mult)
    hs = [conv(2, '', h)]
    for lvl in range(L):
        for _ in range(nrb):
            hs.append(res(i, hs[-1], temb))
            i += 1
        if lvl != L - 1:
            hs.append(F.avg_pool3d(hs[-1], 2, 2))
            i += 1
    h = hs[-1]
    for _ in range(2):
        h = res(i, h, temb)
        i += 1
    for lvl in reversed(range(L)):
        for _ in range(nrb + 1):
            h = res(i, torch.cat([h, hs.pop()], dim=1), temb)
            i += 1
        if lvl != 0:
            h = F.interpolate(h, scale_factor=2, mode='nearest')
            i += 1
    return conv(i + 1, '', F.silu(gn(i, '', h)))


def _grads64(fn, p, x):
    """float64 autograd of the scalar fn(p64, x64) -> (value, {name: grad}, dx)"""
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    x64 = x.double().clone().requires_grad_(True)
    val = fn(p64, x64)
    names = list(p64)
    gs = torch.autograd.grad(val, [p64[k] for k in names] + [x64], allow_unused=True)
    grads = {k: (torch.zeros_like(p64[k]) if g is None else g) for k, g in zip(names, gs[:-1])}
    return float(val.detach()), grads, gs[-1]


@functools.lru_cache(maxsize=None)
def net_ref(case, loss='g'):
    """float64 reference of the model-level test: loss = sum(forward64 * g) ('g') or sum(forward64) ('sum') -> (value, grads, dx)"""
    x, y, labels = dc.case_inputs(case)
    g = net_g(case).double() if loss == 'g' else 1.0

    def fn(p64, x64):
        return (dc.forward64(p64, case, x64, y, labels) * g).sum()
    return _grads64(fn, dc.params(case), x)


def grad_check(got, ref, tol, floor):
    """the per-tensor rule of test_planned_graph_equals_operator_graph / test_training_loss_and_grads_vs_reference:
    err <= tol * scale + floor * total / sqrt(numel); -> (worst err / allowance, its name).  got / ref: {name: tensor}"""
    total = float(np.sqrt(sum(float((v.double() ** 2).sum()) for v in ref.values())))
    worst, where = 0.0, None
    for k, v in ref.items():
        assert got[k] is not None, k
        err = float((got[k].detach().cpu().double() - v.double()).abs().max())
        scale = max(float(v.abs().max()), float(v.double().norm()) / np.sqrt(v.numel()))
        allow = tol * scale + floor * total / np.sqrt(v.numel())
        if err / allow > worst:
            worst, where = err / allow, k
    return worst, where


# ---- the training losses restated in float64 (losses.get_general_sde_loss_fn(sde, True, ...), continuous, likelihood weighting, mean) ----
def loss_sdes(case):
    from conditional_score_diffusion_amd import sde_lib
    name = dc.CASES[case][0]
    if name == 'ddpm3D':
        return sde_lib.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    sx = sde_lib.cVESDE(dc.SIGMA_MIN, dc.SIGMA_MAX, dc.N_SCALES)
    return {'x': sx, 'y': sde_lib.VESDE(dc.SIGMA_MIN, dc.SIGMA_MAX_Y, dc.N_SCALES)} if name == 'ddpm3D_paired' else sx


def loss_tape(case):
    """(u [B] in (0, 1), [normals in the loss's randn_like order])"""
    name, nf, ch_mult, nrb, B, vol, xc, yc = dc.CASES[case]
    rs = np.random.RandomState(77)
    u = torch.from_numpy(rs.uniform(0.05, 0.95, size=(B,)).astype(np.float32))
    shapes = [(B, yc) + vol, (B, xc) + vol] if name == 'ddpm3D_paired' else [(B, xc) + vol]
    return u, [torch.from_numpy(rs.standard_normal(s).astype(np.float32)) for s in shapes]


def loss_batch(case):
    """the clean batch of the loss: x ~ U(0, 1) data (not the 5 N(0, 1) network probe), y as in case_inputs"""
    name, nf, ch_mult, nrb, B, vol, xc, yc = dc.CASES[case]
    rs = np.random.RandomState(78)
    x = torch.from_numpy(rs.uniform(0, 1, size=(B, xc) + vol).astype(np.float32))
    return x, dc.case_inputs(case)[1]


@functools.lru_cache(maxsize=None)
def loss_ref(case):
    """float64 value and parameter gradients of the training loss on (loss_batch, loss_tape)"""
    name = dc.CASES[case][0]
    sde = loss_sdes(case)
    x, y = loss_batch(case)
    u, tape = loss_tape(case)
    eps = 1e-5
    sx = sde['x'] if isinstance(sde, dict) else sde
    t = u * (sx.T - eps) + eps                                    # fp32, as the loss draws it
    B = x.shape[0]
    one = torch.ones(B, 1, 1, 1)

    def mstd(s):
        m, std = s.marginal_prob(one, t)
        return m.flatten().double()[:, None, None, None, None], std.flatten().float().double()[:, None, None, None, None]

    def g2(s):
        return s.sde(torch.zeros(B, 1, 1, 1), t)[1].flatten().double() ** 2

    def fn(p64, _):
        if name == 'ddpm3D':                                      # label = sigma(t)
            z, = tape
            m, std = mstd(sde)
            out = dc.forward64(p64, case, m * x.double() + std * z.double(), None, std.flatten().float())
            d = out / std + z.double() / std
            return (d.flatten(1).pow(2).sum(1) / x[0].numel() * g2(sde)).mean()
        labels = (t * (sx.N - 1)).float()
        if name == 'ddpm3D_paired_SR3':
            z, = tape
            m, std = mstd(sde)
            out = dc.forward64(p64, case, m * x.double() + std * z.double(), y, labels)
            d = out / std + z.double() / std
            return (d.flatten(1).pow(2).sum(1) / x[0].numel() * g2(sde)).mean()
        z_y, z_x = tape
        m_y, std_y = mstd(sde['y'])
        m_x, std_x = mstd(sde['x'])
        out = dc.forward64(p64, case, m_x * x.double() + std_x * z_x.double(), m_y * y.double() + std_y * z_y.double(), labels)
        xc = x.shape[1]
        dx_ = out[:, :xc] / std_x + z_x.double() / std_x
        dy_ = out[:, xc:] / std_y + z_y.double() / std_y
        tot = dx_.flatten(1).pow(2).sum(1) * g2(sde['x']) + dy_.flatten(1).pow(2).sum(1) * g2(sde['y'])
        return (tot / (x[0].numel() + y[0].numel())).mean()

    val, grads, _ = _grads64(fn, dc.params(case), x)
    return val, grads
