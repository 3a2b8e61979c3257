"""Colorization with an unconditional network (controllable_generation.py:95-191 of the reference): the cases shared by
tools/make_colorize_goldens.py (which runs the imported reference on them and writes tests/golden/colorize.npz), tests/test_colorize_host.py
and tests/test_gpu_colorize.py - and a float64 restatement of the operator and of the whole sampler, from the formulas alone.

Every run is `uncond_tiny` (3 channels, 16 x 16), B = 2, an SDE of N = 4 steps, eps = 1e-3, snr = 0.075, the gray image of ``gray()`` and
the tape ``run_tape(pred, corr)``: the prior, then per step [z_corrector] z_colorize [z_predictor] z_colorize, every draw of the
state's size.  The VP / sub-VP SDEs run with beta_min = 0.1, beta_max = 3: the colorizer takes sde.N steps and the discrete betas
beta_max / N must stay below 1.

Draw count (the convention of tests/golden/pc_draws.json: rows ``[step, kind, phase, elems, tape_offset, philox_stream]``, draw j of the
sequence behind the prior on Philox stream 1 + j and behind the draws before it on the tape): a run has 2 N z_colorize draws - one behind
every phase, a 'none' phase included - plus the sampler's own, one per step and phase whose rule is not 'none'; ``draw_rows`` lists them.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')) if p not in sys.path]
import cases  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'colorize.npz')
N, EPS, SNR = 4, 1e-3, 0.075
B = 2
VP_KW = dict(beta_min=0.1, beta_max=3.)
# the reference's orthonormal matrix (controllable_generation.py:117-119): column 0 is (1, 1, 1) / sqrt(3), the gray direction
M = ((5.7735014e-01, -8.1649649e-01, 4.7008697e-08),
     (5.7735026e-01, 4.0824834e-01, 7.0710671e-01),
     (5.7735026e-01, 4.0824822e-01, -7.0710683e-01))
RUNS = [            # name, SDE class, predictor, corrector, probability_flow, denoise
    ('ve_rd_lang', 'VESDE', 'reverse_diffusion', 'langevin', False, True),
    ('ve_rd_lang_noisy', 'VESDE', 'reverse_diffusion', 'langevin', False, False),
    ('vp_rd_lang', 'VPSDE', 'reverse_diffusion', 'langevin', False, True),
    ('ve_em_none', 'VESDE', 'euler_maruyama', 'none', False, True),
    ('vp_em_none', 'VPSDE', 'euler_maruyama', 'none', False, True),
    ('subvp_em_none', 'subVPSDE', 'euler_maruyama', 'none', False, True),
    ('ve_anc_none', 'VESDE', 'ancestral_sampling', 'none', False, True),
    ('vp_anc_none', 'VPSDE', 'ancestral_sampling', 'none', False, True),
    ('ve_rd_none_pf', 'VESDE', 'reverse_diffusion', 'none', True, True),
]
OP_SHAPE, OP_T = (3, 3, 5, 7), 0.4                 # the operator fixture: one re-imposition under VPSDE(**VP_KW, N) at t = 0.4
Z_COLORIZE = 5                                     # kind id of csd_pc_noise_draws
CORR, PRED = 0, 1                                  # phase ids


def run(name):
    return next(r for r in RUNS if r[0] == name)


def config():
    return cases.case_config('uncond_tiny')[0]


def make_sde(sde_lib, scls, n=N):
    """the run's SDE from a module with the reference's class names (the reference's sde_lib or the package's)"""
    cfg = config()
    if scls == 'VESDE':
        return sde_lib.VESDE(cfg.model.sigma_min_x, cfg.model.sigma_max_x, n)
    return getattr(sde_lib, scls)(VP_KW['beta_min'], VP_KW['beta_max'], n)


def scale(scls):
    """what the run bounds are relative to: sigma_max for the VE SDE, 1 for VP and sub-VP (the inpainting row)"""
    return float(config().model.sigma_max_x) if scls == 'VESDE' else 1.0


def shape():
    return (B,) + tuple(config().data.shape_x)


def gray():
    """a gray-scale batch in [0, 1): [B, 3, S, S] with equal channels"""
    S = config().data.image_size
    g = np.random.RandomState(78).uniform(0, 1, size=(B, 1, S, S)).astype(np.float32)
    return torch.from_numpy(np.repeat(g, 3, axis=1).copy())


def n_draws(pred, corr, n=N):
    """draws behind the prior: 2 n z_colorize plus the sampler's own"""
    return (2 + (pred != 'none') + (corr != 'none')) * n


def run_tape(pred, corr, n=N, seed=42):
    return cases.tape([shape()] * (1 + n_draws(pred, corr, n)), seed)


def draw_rows(has_pred, has_corr, n, nx):
    """the rows csd_pc_noise_draws lists for a colorization run (kind 3 = z, 5 = z_colorize)"""
    rows = []
    for i in range(n):
        for phase, has in ((CORR, has_corr), (PRED, has_pred)):
            for kind in ([3] if has else []) + [Z_COLORIZE]:
                rows.append([i, kind, phase, nx, len(rows) * nx, 1 + len(rows)])
    return rows


def op_inputs():
    """the operator fixture's inputs: state, gray image, the full-size draw"""
    rs = np.random.RandomState(91)
    x = torch.from_numpy((rs.standard_normal(OP_SHAPE) * 3.0).astype(np.float32))
    g = torch.from_numpy(np.repeat(rs.uniform(0, 1, size=(OP_SHAPE[0], 1) + OP_SHAPE[2:]).astype(np.float32), 3, axis=1).copy())
    z = torch.from_numpy(rs.standard_normal(OP_SHAPE).astype(np.float32))
    return x, g, z


def golden():
    return np.load(GOLDEN)


class Tape:
    """torch.randn / torch.randn_like read from a list, on the device of the caller's tensor (the step-by-step colorizer draws its
    prior with torch.randn and its noise with torch.randn_like)"""

    def __init__(self, tensors):
        self.t, self.i = list(tensors), 0

    def _next(self, shp, device=None):
        z = self.t[self.i]
        self.i += 1
        assert tuple(z.shape) == tuple(shp), (tuple(z.shape), tuple(shp))
        return z.clone().to(device) if device is not None else z.clone()

    def __enter__(self):
        self._randn, self._randn_like = torch.randn, torch.randn_like
        torch.randn = lambda *s, **k: self._next(s[0] if len(s) == 1 and not isinstance(s[0], int) else s, k.get('device'))
        torch.randn_like = lambda x, **k: self._next(x.shape, x.device)
        return self

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self._randn, self._randn_like


# ---- float64 restatement: the operator -----------------------------------------------------------------------------------------------------
def matrices64(matrix=None):
    m = torch.tensor(M if matrix is None else matrix, dtype=torch.float32).double()
    return m, torch.linalg.inv(m)


def decouple64(v, m):
    return torch.einsum('bihw,ij->bjhw', v.double(), m)


def gray0_64(g, matrix=None):
    return decouple64(g, matrices64(matrix)[0])[:, :1]


def blend64(x, gray0, z, mean_scale, std, matrix=None):
    """the re-imposition on a state x, float64: (x, x_mean).  z: a full-size draw (channel 0 used) or None (masked = masked_mean)"""
    m, inv = matrices64(matrix)
    mask = torch.tensor([1., 0., 0.], dtype=torch.float64).reshape(1, 3, 1, 1)
    mean = torch.cat([mean_scale * gray0.double(), torch.zeros_like(x[:, 1:]).double()], dim=1)
    masked = mean + (z.double() * std if z is not None else 0.)
    xn = decouple64(decouple64(x, m) * (1. - mask) + masked * mask, inv)
    xm = decouple64(decouple64(xn, m) * (1. - mask) + mean * mask, inv)
    return xn, xm


# ---- float64 restatement: the whole sampler ------------------------------------------------------------------------------------------------
class _SDE64:
    """the scalars of the three SDEs (sde_lib.py of the reference) as python floats: evaluated in fp32 with the reference's expressions
    (its marginal std of the VP SDEs, sqrt(1 - exp(2 lmc)), loses digits to cancellation near t = eps; that belongs to what the
    reference computes), then widened.  ``t`` is a 0-d fp32 tensor, one of the reference's timesteps"""

    def __init__(self, scls, n, sigma_max=None):
        self.scls, self.N = scls, n
        m = config().model
        self.smin, self.smax = float(m.sigma_min_x), float(sigma_max if sigma_max is not None else m.sigma_max_x)
        self.b0, self.b1 = VP_KW['beta_min'], VP_KW['beta_max']
        self.sigmas = torch.exp(torch.linspace(np.log(self.smin), np.log(self.smax), n))
        self.betas = torch.linspace(self.b0 / n, self.b1 / n, n)

    @property
    def prior_scale(self):
        return self.smax if self.scls == 'VESDE' else 1.0

    def index(self, t):
        return int((t * (self.N - 1)).long())                      # (the truncation of the fp32 product, as the reference makes it)

    def marginal(self, t):
        """(mean scale, std) of p_t(x | x_0)"""
        if self.scls == 'VESDE':
            smin, smax = torch.tensor(self.smin).type_as(t), torch.tensor(self.smax).type_as(t)
            return 1.0, float(smin * (smax / smin) ** t)
        lmc = -0.25 * t ** 2 * (self.b1 - self.b0) - 0.5 * t * self.b0
        e = torch.exp(2. * lmc)
        return float(torch.exp(lmc)), float(torch.sqrt(1. - e) if self.scls == 'VPSDE' else 1. - e)

    def label(self, t):
        return self.marginal(t)[1] if self.scls == 'VESDE' else float(t * (self.N - 1))

    def sde(self, t):
        """(phi, g): drift = phi x, diffusion g"""
        if self.scls == 'VESDE':
            c = torch.sqrt(torch.tensor(2 * (np.log(self.smax) - np.log(self.smin))).type_as(t))
            return 0.0, float(self.smin * (self.smax / self.smin) ** t * c)
        beta = self.b0 + t * (self.b1 - self.b0)
        if self.scls == 'VPSDE':
            return float(-0.5 * beta), float(torch.sqrt(beta))
        discount = 1. - torch.exp(-2 * self.b0 * t - (self.b1 - self.b0) * t ** 2)
        return float(-0.5 * beta), float(torch.sqrt(beta * discount))

    def discretize(self, t, k):
        """(a, G): f = a x"""
        if self.scls == 'VESDE':
            adj = self.sigmas[k - 1] if k > 0 else torch.zeros(())
            return 0.0, float(torch.sqrt(self.sigmas[k] ** 2 - adj ** 2))
        if self.scls == 'VPSDE':
            return float(torch.sqrt(1. - self.betas[k])) - 1., float(torch.sqrt(self.betas[k]))
        phi, g = self.sde(t)
        return phi * (1 / self.N), g * float(torch.sqrt(torch.tensor(1 / self.N)))


MANGLES = ('transpose', 'prior_order', 'mean_old_x')
EXTRA_MANGLES = ('mean_from_update',)


def colorize64(name, mangle=None, sigma_max=None):
    """The reference's pc_colorizer (controllable_generation.py:166-189) on the run ``name``, restated in float64 from the formulas:
    state, network (wide_cases.forward64 on the synthetic parameters) and updates in float64, the per-step scalars in fp32 (_SDE64).
    ``mangle`` restates it WRONGLY on purpose (tests/test_colorize_host.py): 'transpose' contracts with M^T (and its inverse),
    'prior_order' masks the prior after decouple instead of before it, 'mean_old_x' builds x_mean from the state that enters the phase
    (the ``x`` argument of the reference's update function) instead of the new x, 'mean_from_update' builds it from the x_mean that the
    update returned (the state before the update's noise)."""
    import wide_cases as wc
    assert mangle is None or mangle in MANGLES + EXTRA_MANGLES
    _, scls, pred, corr, pf, denoise = run(name)
    cfg = config()
    p = wc.params(cfg, 0)
    sde = _SDE64(scls, N, sigma_max)
    m = torch.tensor(M, dtype=torch.float32).double()
    if mangle == 'transpose':
        m = m.t().contiguous()
    inv = torch.linalg.inv(m)
    dec = lambda v: torch.einsum('bihw,ij->bjhw', v, m)            # noqa: E731
    cou = lambda v: torch.einsum('bihw,ij->bjhw', v, inv)          # noqa: E731
    mask = torch.tensor([1., 0., 0.], dtype=torch.float64).reshape(1, 3, 1, 1)
    it = iter(run_tape(pred, corr))
    z = lambda: next(it).double()                                  # noqa: E731
    g = gray().double()
    half = 0.5 if pf else 1.0

    def score(x, t):
        out = wc.forward64(p, cfg, x, None, torch.full((B,), sde.label(t), dtype=torch.float64))
        std = sde.marginal(t)[1]
        return out / std

    def norm_mean(v):
        return torch.norm(v.reshape(v.shape[0], -1), dim=-1).mean()

    def update(rule, x, t, k):
        if rule == 'none':
            return x, x
        s = score(x, t)
        zz = z()
        if rule == 'langevin':
            alpha = 1.0 if scls == 'VESDE' else float(1. - sde.betas[k])
            step = (SNR * norm_mean(zz) / norm_mean(s)) ** 2 * 2 * alpha
            x_mean = x + step * s
            return x_mean + torch.sqrt(step * 2) * zz, x_mean
        if rule == 'reverse_diffusion':
            a, G = sde.discretize(t, k)
            x_mean = x - (a * x - G ** 2 * s * half)
            return x_mean + (0. if pf else G) * zz, x_mean
        if rule == 'euler_maruyama':
            phi, gd = sde.sde(t)
            dt = -1. / N
            x_mean = x + (phi * x - gd ** 2 * s * half) * dt
            return x_mean + (0. if pf else gd) * np.sqrt(-dt) * zz, x_mean
        assert rule == 'ancestral_sampling' and not pf
        if scls == 'VESDE':
            s2 = float(sde.sigmas[k]) ** 2
            a2 = float(sde.sigmas[k - 1]) ** 2 if k > 0 else 0.0
            x_mean = x + s * (s2 - a2)
            return x_mean + np.sqrt(a2 * (s2 - a2) / s2) * zz, x_mean
        beta = float(sde.betas[k])
        x_mean = (x + beta * s) / np.sqrt(1. - beta)
        return x_mean + np.sqrt(beta) * zz, x_mean

    prior = z() * sde.prior_scale
    if mangle == 'prior_order':
        x = cou(dec(g) * mask + dec(prior) * (1. - mask))
    else:
        x = cou(dec(g) * mask + dec(prior * (1. - mask)))
    ts = torch.linspace(1, EPS, N)                                 # fp32, as the reference computes them
    x_mean = x
    for i in range(N):
        t, k = ts[i], sde.index(ts[i])
        for rule in (corr, pred):
            x_in = x                                               # the state the phase starts from
            x, x_upd_mean = update(rule, x, t, k)
            ms, std = sde.marginal(t)
            masked_mean = ms * dec(g)
            masked = masked_mean + z() * std
            x_new = cou(dec(x) * (1. - mask) + masked * mask)
            src = x_in if mangle == 'mean_old_x' else x_upd_mean if mangle == 'mean_from_update' else x_new
            x_mean = cou(dec(src) * (1. - mask) + masked_mean * mask)
            x = x_new
    assert next(it, None) is None
    return x_mean if denoise else x
