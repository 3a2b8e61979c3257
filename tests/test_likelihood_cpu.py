"""CPU tests of the probability-flow likelihood (conditional_score_diffusion_amd/likelihood.py): the reference algorithm on an analytic
score model, where the answer is known in closed form."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from conditional_score_diffusion_amd import likelihood, sde_lib


class GaussianScoreNet(nn.Module):
    """Exact score network of data N(0, s^2 I) under a VE SDE: the marginal at t is N(0, v(t) I) with
    v(t) = s^2 + sigma(t)^2 - sigma_min^2, and the VE score function divides the output by sigma(t) (its label)."""

    def __init__(self, s, sigma_min):
        super().__init__()
        self.s2, self.smin2 = s * s, sigma_min * sigma_min

    def forward(self, x, labels):
        std = labels.to(torch.float64)[:, None, None, None]
        v = self.s2 + std * std - self.smin2
        return (-x.to(torch.float64) * std / v).to(x.dtype)


def closed_form_bpd(x, s, sde, eps):
    D = x[0].numel()
    smin = sde.sigma_min

    def v(t):
        return s * s + (smin * (sde.sigma_max / smin) ** t) ** 2 - smin * smin

    ratio = v(1.0) / v(eps)
    z = x.double() * np.sqrt(ratio)                       # dx/dt = (v'/2v) x
    delta = 0.5 * D * np.log(ratio)                       # integral of the divergence D v'/2v
    prior = -D / 2. * np.log(2 * np.pi * sde.sigma_max ** 2) - (z ** 2).sum(dim=(1, 2, 3)) / (2 * sde.sigma_max ** 2)
    bpd = -(prior + delta) / np.log(2) / D
    return bpd + 7. - (-1.)                               # offset of the inverse scaler x -> x (inverse_scaler(-1) = -1)


@pytest.mark.parametrize('s', [0.5, 2.0])
def test_gaussian_data_matches_closed_form(s):
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=5.0, N=1000)
    eps = 1e-5
    fn = likelihood.get_likelihood_fn(sde, lambda v: v, hutchinson_type='Rademacher', rtol=1e-6, atol=1e-6, eps=eps)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.standard_normal((3, 2, 4, 4)).astype(np.float32) * s)
    bpd, z, nfe = fn(GaussianScoreNet(s, sde.sigma_min), x)
    want = closed_form_bpd(x, s, sde, eps)
    assert bpd.shape == (3,) and z.shape == x.shape and nfe > 0
    assert (bpd.double() - want).abs().max().item() <= 1e-3, (bpd, want)


def test_pinned_epsilon_is_used():
    """a Gaussian eps makes the estimate depend on the draw: the same pinned eps gives the same numbers"""
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=5.0, N=1000)
    fn = likelihood.get_likelihood_fn(sde, lambda v: v, hutchinson_type='Gaussian', rtol=1e-4, atol=1e-4)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((2, 1, 4, 4)).astype(np.float32))
    e = torch.from_numpy(np.random.RandomState(2).standard_normal((2, 1, 4, 4)).astype(np.float32))
    net = GaussianScoreNet(1.0, sde.sigma_min)
    b1, _, _ = fn(net, x, epsilon=e)
    b2, _, _ = fn(net, x, epsilon=e.clone())
    assert torch.equal(b1, b2)


def test_div_fn_is_the_hutchinson_estimate():
    A = torch.from_numpy(np.random.RandomState(3).standard_normal((8, 8)))
    div = likelihood.get_div_fn(lambda x, t: (x.reshape(x.shape[0], -1) @ A.T).reshape(x.shape))
    x = torch.zeros(2, 2, 2, 2, dtype=torch.float64)
    e = torch.from_numpy(np.random.RandomState(4).choice([-1.0, 1.0], size=(2, 2, 2, 2)))
    got = div(x, None, e)
    ef = e.reshape(2, -1)
    assert torch.allclose(got, ((ef @ A) * ef).sum(dim=1))


def test_conditional_likelihood_rejects_the_cmde_pair():
    pair = {'x': sde_lib.cVESDE(0.01, 5.0, 1000), 'y': sde_lib.VESDE(0.01, 1.0, 1000)}
    with pytest.raises(NotImplementedError):
        likelihood.get_conditional_likelihood_fn(pair, lambda v: v)
    with pytest.raises(NotImplementedError):
        likelihood.get_conditional_likelihood_fn(sde_lib.VESDE(0.01, 5.0, 1000), lambda v: v)
